"""The route ledger (tests/route_ledger.py): every kernel -- every kernel id, every __global__ function and, as a ratchet, every
template instantiation of the library -- is launched by a checked scenario, and every route switch of
smcp_amd/csrc/switches.hpp is shown taking effect by one -- or is listed with the module that covers it or the reason it is exempt.

Per scenario: every error against the dense definitions is at most dense_ref.device_bound (for a pattern outside GPU_PATTERNS
whose recorded oracle-vs-dense error is beyond the yardstick: 100 x its own recorded value, capped at 1e-12 -- fan40: dot, llt;
tops8: kkt_H, kkt_y, logdiagsum; tail8: dot, hessian, hessian_gadj_g, kkt_x, llt; fan32: llt; for a mixed KKT recipe on a pattern
of GPU_PATTERNS the same rule on the record of that recipe, tests/golden/hybrid_recipe_yardstick.json; route_ledger.bound_of),
the units pass their own checks, the signature holds on the scenario's routes and the opposite signature on the default routes.
No other tolerance; signatures are counts of zero or at least one, over the kernel ids (csp_profile_*: `ran`, `gone`) and over
the kernel functions (csp_census_*: `ran_k`, `gone_k`).

What is counted.  A kernel id stands for a group of kernels (KID_ceig: k_ceig, k_ceig_vec, k_cone_split and the fifteen kernels
of the chip-wide block Jacobi; KID_hess_down_mfma<true>: k_hess_down_mfma<true, *> and k_hess_down_w<1..4>; ...).  The launch
census counts every launch under the function that was launched, one name per template instantiation; the universe is the
kernel descriptors (.kd symbols) of libsmcp_amd.so, which a CPU test holds equal to the __global__ functions of smcp_amd/csrc.
A second CPU test holds the kernels at hipLaunchKernelGGL sites outside the two launch helpers equal to
route_ledger.DIRECT_LAUNCHES.  tests/golden/kernel_census.json records the instantiations that no passing scenario launches,
each with the launch-site condition that selects it: an unlaunched instantiation outside that file fails, and so does a
recorded one that was launched.  It may hold no kernel added since the ledger was written and no arm of the dense-block
products (MUST_BE_LAUNCHED).  To refresh it, run the ledger, read the line "LEDGER unlaunched" and edit the file.

MEASURED on one MI355X in one run (another run or machine will differ in the last digits and in the times):

    kernel ids                142, every one launched by a passing scenario
    kernel functions          209: 199 launched by a passing scenario, 6 exempt (EXEMPT_KERNELS), 2 without a launch site
                              (DEAD_KERNELS: k_selftest_mma, k_exchange_copy), 2 not counted (NOT_COUNTED)
    kernel instantiations     399: 288 launched by a passing scenario, 99 recorded in kernel_census.json, 12 of the exempt,
                              dead and uncounted functions
    before this file counted functions, with the census alone added to the scenarios it had then: 158 functions and 240
    instantiations were launched by a passing scenario

What the census found when it was added: the 40 kernels of clique_eigh .. clique_decompose ran in no scenario (now: units_spectra,
units_factor); the column block of 2 .. 4 columns of k_trmm_n, k_trmm_t and k_symm_fma ran in no unit (now: 3 columns in `trmm` and
`symm`); k_dense_trsv_step, k_stack_gemm_panel, k_qr_shift, k_latch_status, k_res_combine_cliques, k_diag_fingerprint and
k_fingerprint_compare ran in no scenario (now: units_kkt, generic, verify_cache); fz_tail0 never reached the shares it switches
off (k_lf_zero_pairs) and the hybrid Schur route (k_scatter_hd) was checked on one rank only as the reference of a sharded
test; two kernels have no launch site at all.  Since then: hybrid variants of the sparse-input cases -- the
swept constraints a non-contiguous subset, read through kc_ids -- run on the default routes (`hybrid`) and under every switch
that changes a kernel reading the subset; tail8 and fan32 reach k_lf_zero_pairs, so fz_tail0, fz0 and scm0 have signatures.

Worst device-vs-dense error per operation over the scenarios' own routes, against the bound in force for its pattern:

    operation             device worst   bound      scenario (pattern)
    cholesky              2.6e-16        4.1e-14    chol_prep0 (tops8)
    completion            4.0e-16        6.4e-14    generic (arrow_thin)
    dot                   1.8e-16        1.2e-13    generic (arrow_thin)
    hessian               1.6e-15        1.9e-13    default_small (dense600)
    hessian_adjoint       6.5e-17        6.9e-15    default_small (arrow)
    hessian_factor_inv    1.7e-15        1.7e-13    default_small (dense600)
    hessian_gadj_g        1.6e-15        2.0e-13    default_small (dense600)
    hessian_gram          6.2e-16        4.4e-14    large0 (arrow_big)
    hessian_inv           2.3e-15        2.6e-13    default_small (rand2)
    kkt_H                 9.2e-16        2.4e-13    hybrid (tops8)
    kkt_x                 2.0e-15        2.1e-13    fz_tail0 (tail8)
    kkt_y                 2.0e-15        4.9e-13    zsp0 (dense450)
    llt                   2.1e-16        1.8e-14    default_small (rand1)
    logdiagsum            1.9e-16        1.7e-13    trtri0 (two_fronts)
    projected_inverse     9.5e-16        8.4e-14    chol_prep0 (tops8)
    trsm                  6.1e-16        8.6e-14    gram_side (arrow_big)

Per scenario: wall time (child interpreter: start, import and context set-up included; in-proc: the measured cases alone), and the
error closest to its bound over both runs (the scenario's routes and the default routes of the same cases):

    scenario          switches                                      time    where    operation          error    bound
    alds0             ALDS=0                                          7.1 s child    kkt_x              1.4e-15  2.0e-13
    alds_dyn0         ALDS_DYN=0                                      4.1 s child    kkt_x              1.2e-15  2.0e-13
    alds_fill0        ALDS_FILL=0                                     5.7 s child    kkt_x              1.4e-15  2.0e-13
    asm_t             ASM=t                                           3.1 s child    hessian_gram       2.9e-16  4.4e-14
    chol_prep0        CHOL_PREP=0                                     3.4 s child    projected_inverse  9.5e-16  8.4e-14
    default_small     (default routes)                                0.5 s in-proc  llt                2.1e-16  1.8e-14
    down_w0           DOWN_W=0                                        3.3 s child    hessian            1.4e-15  1.9e-13
    fac_partial0      FAC_PARTIAL=0                                   3.2 s child    projected_inverse  8.3e-16  8.4e-14
    faci_lds0         FACI_LDS=0                                      2.8 s child    hessian_gram       2.9e-16  4.4e-14
    fam0              FAM=0                                           3.0 s child    projected_inverse  6.7e-16  8.4e-14
    fam2_0            FAM2=0                                          3.6 s child    kkt_x              1.4e-15  2.0e-13
    famt0             FAMT=0                                          3.4 s child    kkt_x              1.4e-15  2.0e-13
    famt_group0       FAMT_GROUP=0                                    2.7 s child    kkt_x              1.3e-15  2.0e-13
    flow0             FLOW=0                                          2.8 s child    projected_inverse  8.5e-16  8.4e-14
    flow_wg5          FLOW_WG=5                                       2.5 s child    projected_inverse  8.5e-16  8.4e-14
    fz0               FZ=0                                            5.6 s child    kkt_x              1.6e-15  2.0e-13
    fz_tail0          FZ_TAIL=0                                       7.5 s child    kkt_x              2.0e-15  2.1e-13
    generic           GENERIC=1                                       2.8 s child    hessian_adjoint    5.8e-17  6.9e-15
    gram0             GRAM=0                                          2.9 s child    kkt_x              1.7e-15  2.0e-13
    gram_side         GRAM_EARLY=1 LG_SIDE=0                          4.0 s child    hessian_gram       6.1e-16  4.4e-14
    hybrid            (default routes)                                0.5 s in-proc  kkt_x              1.4e-15  2.0e-13
    large0            LARGE=0                                         3.3 s child    hessian_gram       6.2e-16  4.4e-14
    leafgram0         LEAFGRAM=0                                      3.5 s child    kkt_x              1.4e-15  2.0e-13
    lfsp0             LFSP=0                                          4.0 s child    hessian_gram       2.9e-16  4.4e-14
    lg_early0         LG_EARLY=0                                      4.1 s child    hessian_gram       6.1e-16  4.4e-14
    mid0              MID=0                                           2.8 s child    projected_inverse  7.9e-16  8.4e-14
    n16_0             N16=0                                           3.3 s child    hessian            1.4e-15  1.9e-13
    oldlds1           OLDLDS=1                                        2.5 s child    hessian            1.4e-15  1.9e-13
    pd1               PD=1                                            3.5 s child    hessian_gram       6.1e-16  4.4e-14
    products_mm0      TRMM_MM=0 SYR2K_MM=0 SYMM_MM=0 LOWRANK_MM=0     3.7 s child    -                  0.0e+00  0.0e+00
    products_mm2      TRMM_MM=2 SYR2K_MM=2 SYMM_MM=2                  2.7 s child    -                  0.0e+00  0.0e+00
    qr_trsm_f         QR_TRSM=f                                       2.7 s child    kkt_x              1.3e-15  2.0e-13
    scaling_overlap0  SCALING_OVERLAP=0                               3.0 s child    projected_inverse  8.3e-16  8.4e-14
    scm0              SCM=0                                           3.3 s child    kkt_x              1.6e-15  2.0e-13
    streams           FORK=0 NOCACHE=1 POTRF_DEFER=0                  3.4 s child    hessian_gram       6.1e-16  4.4e-14
    trsm_mm0          TRSM_MM=0                                       2.6 s child    trsm               6.1e-16  8.6e-14
    trtri0            TRTRI=0                                         2.5 s child    projected_inverse  6.0e-16  8.4e-14
    units             (default routes)                                5.2 s child    kkt_x              9.6e-16  2.0e-13
    units_factor      (default routes)                                3.0 s child    -                  0.0e+00  0.0e+00
    units_kkt         (default routes)                                5.1 s child    -                  0.0e+00  0.0e+00
    units_spectra     (default routes)                                5.0 s child    -                  0.0e+00  0.0e+00
    verify_cache      tune VERIFY_CACHE=1                             0.7 s in-proc  hessian_gram       6.1e-16  4.4e-14
    zsp0              ZSP=0                                           2.6 s child    kkt_x              1.4e-15  2.0e-13

The units of `units`, `units_spectra`, `units_factor`, `units_kkt`, `products_mm0`, `products_mm2`, and the units inside `generic`
and `flow0`, assert inside their own modules (no figure here).  No bound was exceeded and no signature failed; every one of the
142 kernel ids was launched by a passing scenario.  The whole ledger took 164 s; as the fixture of this module inside the whole suite 165 s,
against 147 s before the hybrid cases, tail8 and fan32 were added.  The largest single item is tail8, about 6 s (its dense reference
of order 1374 is formed in the child of fz_tail0 and again in this process); the hybrid variants add 0.5 .. 2 s to each of the
scenarios they entered (alds0 4.9 -> 7.1 s, fz0 3.7 -> 5.6 s, alds_fill0 4.1 -> 5.7 s, fz_tail0 4.6 -> 7.5 s).
"""
import os
import tempfile

import pytest

from tests import dense_ref
from tests import route_ledger as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# measured wall time of every child, seconds (same run as the table above); a child's timeout is ten times that, rounded up, and
# at least 120 s: a limit that ends trouble, not a performance claim
CHILD_SECONDS = {"alds0": 7.1, "alds_dyn0": 4.1, "alds_fill0": 5.7, "asm_t": 3.1, "chol_prep0": 3.4, "down_w0": 3.3,
                 "fac_partial0": 3.2, "faci_lds0": 2.8, "fam0": 3.0, "fam2_0": 3.6, "famt0": 3.4, "famt_group0": 2.7,
                 "flow0": 2.8, "flow_wg5": 2.5, "fz0": 5.6, "fz_tail0": 7.5, "generic": 2.8, "gram0": 2.9,
                 "gram_side": 4.0, "large0": 3.3, "leafgram0": 3.5, "lfsp0": 4.0, "lg_early0": 4.1, "mid0": 2.8,
                 "n16_0": 3.3, "oldlds1": 2.5, "pd1": 3.5, "products_mm0": 3.7, "products_mm2": 2.7, "qr_trsm_f": 2.7,
                 "scaling_overlap0": 3.0, "scm0": 3.3, "streams": 3.4, "trsm_mm0": 2.6, "trtri0": 2.5, "units": 5.2,
                 "units_factor": 3.0, "units_kkt": 5.1, "units_spectra": 5.0, "zsp0": 2.6}


# kernels of which tests/golden/kernel_census.json may hold no instantiation: everything added since the ledger, and the arms of
# the dense-block products, whose units were written to take every kernel
MUST_BE_LAUNCHED = ["k_ceig*", "k_ceigw*", "k_cone*", "k_clique_gather", "k_clique_scatter", "k_cu_*", "k_cdec_*", "k_lz_*",
                    "k_trmm_n<*", "k_trmm_t<*", "k_trmm_mm<*", "k_syr2k_fma<*", "k_syr2k_mm<*", "k_symm_fma<*", "k_lr_gram<*"]


def timeout_of(name):
    return max(120, int(10 * CHILD_SECONDS.get(name, 12.0) + 0.999))


# ---- on a CPU ----------------------------------------------------------------------------------------------------------
def test_every_route_switch_is_in_the_ledger():
    names = rl.route_switches()
    assert len(names) >= 40 and len(set(names)) == len(names), names
    in_scenarios = {sw for scn in rl.SCENARIOS.values() for sw in scn["env"]}
    assert in_scenarios <= set(names), sorted(in_scenarios - set(names))         # no scenario sets a switch the table does not hold
    assert len(rl.EXEMPT_SWITCHES) <= rl.MAX_EXEMPT_SWITCHES == 6
    assert all(isinstance(r, str) and len(r) > 20 for r in rl.EXEMPT_SWITCHES.values())
    missing = [n for n in names if n not in in_scenarios and n not in rl.COVERED_BY and n not in rl.EXEMPT_SWITCHES]
    assert not missing, "route switches that no scenario runs: %s" % missing
    stale = [n for n in list(rl.COVERED_BY) + list(rl.EXEMPT_SWITCHES) if n not in names]
    assert not stale, stale
    for sw, path in rl.COVERED_BY.items():
        with open(os.path.join(ROOT, path)) as f:
            assert sw in f.read(), (sw, path)
    for name, scn in rl.SCENARIOS.items():                                        # a switched scenario states a signature or why it has none
        if scn["env"]:
            assert scn["ran"] or scn["gone"] or scn["ran_k"] or scn["gone_k"] or scn["note"].startswith("not observable"), name
        if scn["tune"] and not scn["env"]:                                        # a tune alone is there for the kernels it brings
            assert scn["ran_k"] or scn["gone_k"], name


def test_exempt_and_dead_kernel_lists_are_within_their_caps():
    assert len(rl.EXEMPT_KERNELS) <= rl.MAX_EXEMPT_KERNELS == 6
    assert not set(rl.EXEMPT_KERNELS) & set(rl.DEAD_KERNELS)
    assert all(isinstance(r, str) and len(r) > 20 for r in list(rl.EXEMPT_KERNELS.values()) + list(rl.DEAD_KERNELS.values()))
    assert len(rl.NOT_COUNTED) <= rl.MAX_NOT_COUNTED == 4
    assert all(isinstance(r, str) and len(r) > 20 for r in rl.NOT_COUNTED.values())
    assert not set(rl.NOT_COUNTED) & (set(rl.EXEMPT_KERNELS) | set(rl.DEAD_KERNELS))


def test_source_kernels_are_the_kernels_of_the_library():
    """every __global__ function of smcp_amd/csrc is in the built library and the library holds no other: the universe the
    census tests count over is the one the sources define (206 functions in 396 instantiations when this was written)"""
    from tests.helpers import kernel_function, kernel_universe
    universe = kernel_universe()
    built = {kernel_function(p) for p in universe.values()}
    src = rl.source_kernels()
    print("LEDGER universe: %d kernel functions, %d instantiations" % (len(built), len(universe)))
    assert len(universe) >= len(built) >= 200
    assert len(set(universe.values())) == len(universe), "two instantiations share a pretty name"
    assert all(p.startswith("k_") and "(" not in p and "::" not in p.split("<")[0] for p in universe.values()), sorted(universe.values())[:5]
    assert src == built, "in the sources only: %s; in the library only: %s" % (sorted(src - built), sorted(built - src))
    named = set(rl.EXEMPT_KERNELS) | set(rl.DEAD_KERNELS)
    from smcp_amd import _lib
    ids = {_lib.lib().csp_profile_kernel_name(i).decode() for i in range(int(_lib.lib().csp_profile_kinds()))}
    assert named <= ids | built, sorted(named - ids - built)
    assert set(rl.NOT_COUNTED) <= built, sorted(set(rl.NOT_COUNTED) - built)


def test_direct_launch_sites_are_listed():
    """a launch past the two launch helpers is invisible to the profile hooks and to SMCP_TRACE: the kernels at such sites are
    exactly the list of the ledger, and the ones the census does not count are among them"""
    found = rl.direct_launches()
    assert found == {k: sorted(v) for k, v in rl.DIRECT_LAUNCHES.items()}, found
    direct = {k for v in found.values() for k in v}
    assert set(rl.NOT_COUNTED) <= direct, sorted(set(rl.NOT_COUNTED) - direct)
    assert direct <= rl.source_kernels()


def test_kernel_census_file_is_well_formed():
    """tests/golden/kernel_census.json names instantiations of the library, each with the condition that selects it, and none
    of the kernels added since the ledger nor an arm of the dense-block products"""
    import fnmatch
    from tests.helpers import kernel_universe
    universe, rec = kernel_universe(), rl.load_kernel_census()
    assert set(rec) <= set(universe), sorted(set(rec) - set(universe))
    for m, e in rec.items():
        assert e["kernel"] == universe[m] and isinstance(e["condition"], str) and len(e["condition"]) > 20, (m, e)
        assert not any(fnmatch.fnmatchcase(e["kernel"], p) for p in MUST_BE_LAUNCHED), e["kernel"]


@pytest.mark.parametrize("pattern", sorted(rl.NEW_PATTERNS))
def test_new_patterns_against_the_yardstick(pattern):
    """The oracle on the ledger's own patterns stays within 10 x of its recorded error (the rule of tests/test_dense_ref.py), and
    the recorded error is at most 1 / 100 of the bound the ledger applies on that pattern."""
    yard, own = dense_ref.load_yardstick(), rl.load_ledger_yardstick()
    assert set(own) == set(rl.NEW_PATTERNS)
    errs = rl.oracle_errors(pattern)
    assert set(errs) == set(yard) == set(own[pattern])
    print(pattern, " ".join("%s=%.1e" % kv for kv in sorted(errs.items())))
    for op, e in errs.items():
        rec = own[pattern][op]
        assert e <= 10.0 * rec or e <= yard[op]["value"], (op, e, rec)
        assert 100.0 * rec <= rl.bound_of(pattern, op, yard, own) <= dense_ref.BOUND_CAP, (op, rec)


def test_signature_rules():
    """the judging functions on hand-made counts: a swapped signature fails on both runs"""
    here, default = {"k_lf_chol_panel": 2, "k_lf_diag": 1}, {"k_mid_chol": 3, "k_lf_diag": 1}
    ran, gone = ["k_lf_chol_*"], ["k_mid_chol"]
    assert rl.signature_faults(here, ran, gone) == [] and rl.signature_faults(default, gone, ran) == []
    assert len(rl.signature_faults(here, gone, ran)) == 2 and len(rl.signature_faults(default, ran, gone)) == 2
    # the same rules over the census: one id, k_hess_down_mfma<true>, on both runs, and the kernels under it tell them apart
    res = {"a": {"counts": {"k_hess_down_mfma<true>": 2}, "kernels": {"k_hess_down_mfma<true, 0>": 2}},
           "b": {"counts": {"k_hess_down_mfma<true>": 1}, "kernels": {"k_hess_down_mfma<true, 0>": 1}}}
    dflt = {"a": {"counts": {"k_hess_down_mfma<true>": 2}, "kernels": {"k_hess_down_w<2>": 1, "k_hess_down_mfma<true, 0>": 1}}}
    assert rl.union_counts(res) == {"k_hess_down_mfma<true>": 3} and rl.union_counts(res, "kernels") == {"k_hess_down_mfma<true, 0>": 3}
    ran_k, gone_k = ["k_hess_down_mfma<true,*"], ["k_hess_down_w<*"]
    assert rl.signature_faults(rl.union_counts(res, "kernels"), ran_k, gone_k) == []
    assert rl.signature_faults(rl.union_counts(dflt, "kernels"), [], gone_k) == ["k_hess_down_w<* ran (k_hess_down_w<2>)"]
    assert rl.signature_faults(rl.union_counts(dflt, "kernels"), gone_k, []) == []              # the opposite holds on the default routes
    assert len(rl.signature_faults(rl.union_counts(res, "kernels"), gone_k, ran_k)) == 2        # swapped: fails on the scenario's routes
    assert rl.signature_faults(rl.union_counts(dflt, "kernels"), ran_k, gone_k) != []           # and on the default routes
    assert rl.union_counts({"old": {"counts": {"k_axpby": 1}}}, "kernels") == {}                 # a record without a census
    scn = rl.S({}, [], ran_k=["k_a"], gone_k=["k_b<*"])
    assert scn["ran_k"] == ["k_a"] and scn["gone_k"] == ["k_b<*"] and scn["ran"] == scn["gone"] == []
    bad = rl.error_faults({"a": {"errors": {"cholesky": 1.0}, "counts": {}}}, [("unit", "x")], lambda p, op: 1e-12)
    assert bad == ["unit:x: not run"]


# ---- on the MI355X -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ledger():
    """every scenario once, children one after the other (route_ledger.collect)"""
    with tempfile.TemporaryDirectory() as tmp:
        out = rl.collect({name: timeout_of(name) for name in rl.SCENARIOS}, tmp)
    for name, rec in out.items():
        print("LEDGER %-18s rc %s %.1f s %s" % (name, rec["rc"], rec["seconds"], rec["skipped"] or ""))
    return out


def scenario_faults(name, rec):
    """everything that is wrong with one scenario's record; [] when its checks passed"""
    scn = rl.SCENARIOS[name]
    if rec["skipped"]:
        return [rec["skipped"]]
    if rec["run"] is None or rec["rc"] not in (0, 1):
        return ["child ended with %s: %s" % (rec["rc"], rec["tail"])]
    yard, own, mixed = dense_ref.load_yardstick(), rl.load_ledger_yardstick(), dense_ref.load_mix_yardstick()
    bound = lambda case, op: rl.bound_of(case, op, yard, own, mixed)
    bad = rl.error_faults(rec["run"], scn["cases"], bound)
    judged = [rl.case_key(c) for c in scn["cases"][:scn["sig_over"]]]
    if not bad:
        bad += rl.signature_faults(rl.union_counts({k: rec["run"][k] for k in judged}), scn["ran"], scn["gone"])
        bad += rl.signature_faults(rl.union_counts({k: rec["run"][k] for k in judged}, "kernels"), scn["ran_k"], scn["gone_k"])
    if scn["env"] or scn["tune"]:
        dflt = rec["default"] or {}
        dbad = rl.error_faults(dflt, scn["cases"], bound)
        if not dbad:
            dbad = rl.signature_faults(rl.union_counts({k: dflt[k] for k in judged}), scn["gone"], scn["ran"])
            dbad += rl.signature_faults(rl.union_counts({k: dflt[k] for k in judged}, "kernels"), scn["gone_k"], scn["ran_k"])
        bad += ["default routes: " + b for b in dbad]
    if bad and rec["tail"]:
        bad.append(rec["tail"])
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(rl.SCENARIOS))
def test_scenario(name, ledger):
    rec = ledger[name]
    for which in ("run", "default"):
        worst = {}
        for r in (rec[which] or {}).values():
            for op, e in r["errors"].items():
                worst[op] = max(worst.get(op, 0.0), e)
        print("LEDGER", name, which, " ".join("%s=%.2e" % kv for kv in sorted(worst.items())))
    bad = scenario_faults(name, rec)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_every_kernel_is_launched_by_a_checked_scenario(ledger):
    from smcp_amd import _lib
    lib = _lib.lib()
    names = [lib.csp_profile_kernel_name(i).decode() for i in range(int(lib.csp_profile_kinds()))]
    by = {}
    for name, rec in ledger.items():
        if scenario_faults(name, rec):
            continue
        for res in (rec["run"], rec["default"]):
            for k in rl.union_counts(res or {}):
                by.setdefault(k, name)
    print("LEDGER kernels: %d ids, %d launched by a passing scenario" % (len(names), len(set(names) & set(by))))
    from tests.helpers import kernel_function, kernel_universe
    functions = {kernel_function(p) for p in kernel_universe().values()}
    listed = (set(rl.EXEMPT_KERNELS) | set(rl.DEAD_KERNELS)) - (functions - set(names))     # (the lists also hold kernel functions)
    assert listed <= set(names), sorted(listed - set(names))
    unchecked = [k for k in names if k not in by and k not in listed]
    assert not unchecked, "kernels that no passing scenario launches: %s" % unchecked
    stale = sorted(k for k in listed if k in by)
    assert not stale, "exempt or dead, but launched: %s" % {k: by[k] for k in stale}


def launched_kernels(ledger):
    """pretty kernel name -> the first scenario whose checks passed and whose census holds it"""
    by = {}
    for name, rec in ledger.items():
        if scenario_faults(name, rec):
            continue
        for res in (rec["run"], rec["default"]):
            for k in rl.union_counts(res or {}, "kernels"):
                by.setdefault(k, name)
    return by


@pytest.mark.gpu
def test_every_kernel_function_is_launched_by_a_checked_scenario(ledger):
    """the promise of the ledger over kernels, not ids: every __global__ function of the library is launched by a scenario
    whose checks passed, or is listed with its launch-site condition (EXEMPT_KERNELS), as unreachable (DEAD_KERNELS) or as
    not counted (NOT_COUNTED)"""
    from tests.helpers import kernel_function, kernel_universe
    functions = {kernel_function(p) for p in kernel_universe().values()}
    by = {}
    for k, name in launched_kernels(ledger).items():
        by.setdefault(kernel_function(k), name)
    assert set(by) <= functions, "launched, but not in the library: %s" % sorted(set(by) - functions)
    universe = functions - set(rl.NOT_COUNTED)
    listed = (set(rl.EXEMPT_KERNELS) | set(rl.DEAD_KERNELS)) & functions
    print("LEDGER kernel functions: %d in the library, %d not counted, %d launched by a passing scenario, %d exempt or dead"
          % (len(functions), len(rl.NOT_COUNTED), len(universe & set(by)), len(listed)))
    unchecked = sorted(k for k in universe if k not in by and k not in listed)
    assert not unchecked, "kernel functions that no passing scenario launches: %s" % unchecked
    stale = sorted(k for k in listed if k in by)
    assert not stale, "exempt or dead, but launched: %s" % {k: by[k] for k in stale}


@pytest.mark.gpu
def test_kernel_instantiations(ledger):
    """the same over every template instantiation, as a ratchet: the instantiations that no passing scenario launches are
    recorded in tests/golden/kernel_census.json with the launch-site condition that selects each; one that is unlaunched and
    not recorded fails, and so does one that is recorded and launched (a stale entry)"""
    from tests.helpers import kernel_function, kernel_universe
    universe = kernel_universe()
    by = launched_kernels(ledger)
    skip = set(rl.NOT_COUNTED) | (set(rl.DEAD_KERNELS) | set(rl.EXEMPT_KERNELS))
    rec = rl.load_kernel_census()
    pretty = {p: m for m, p in universe.items()}
    assert set(by) <= set(pretty), "launched, but not in the library: %s" % sorted(set(by) - set(pretty))
    counted = {m: p for m, p in universe.items() if kernel_function(p) not in skip}
    missing = sorted(p for m, p in counted.items() if p not in by)
    print("LEDGER kernel instantiations: %d in the library, %d counted, %d launched by a passing scenario, %d recorded as unlaunched"
          % (len(universe), len(counted), len(counted) - len(missing), len(rec)))
    print("LEDGER unlaunched: %s" % missing)
    new = sorted(p for m, p in counted.items() if p not in by and m not in rec)
    assert not new, "instantiations that no passing scenario launches and tests/golden/kernel_census.json does not hold: %s" % new
    stale = sorted(e["kernel"] for m, e in rec.items() if e["kernel"] in by)
    assert not stale, "recorded as unlaunched, but launched: %s" % {k: by[k] for k in stale}
