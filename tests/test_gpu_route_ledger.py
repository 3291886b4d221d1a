"""The route ledger (tests/route_ledger.py): every kernel id is launched by a checked scenario, and every route switch of
smcp_amd/csrc/switches.hpp is shown taking effect by one -- or is listed with the module that covers it or the reason it is exempt.

Per scenario: every error against the dense definitions is at most dense_ref.device_bound (for a pattern outside GPU_PATTERNS
whose recorded oracle-vs-dense error is beyond the yardstick: 100 x its own recorded value, capped at 1e-12 -- fan40: dot, llt;
tops8: kkt_H, kkt_y, logdiagsum; route_ledger.bound_of), the units pass their own checks, the signature holds on the scenario's
routes and the opposite signature on the default routes.  No other tolerance; signatures are counts of zero or at least one.

MEASURED on one MI355X in one run (another run or machine will differ in the last digits and in the times):

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
    kkt_H                 5.9e-16        2.3e-13    qr_trsm_f (nested)
    kkt_x                 1.8e-15        2.0e-13    default_small (arrow_one)
    kkt_y                 2.0e-15        4.9e-13    zsp0 (dense450)
    llt                   2.1e-16        1.8e-14    default_small (rand1)
    logdiagsum            1.9e-16        1.7e-13    trtri0 (two_fronts)
    projected_inverse     9.5e-16        8.4e-14    chol_prep0 (tops8)
    trsm                  6.1e-16        8.6e-14    gram_side (arrow_big)

Per scenario: wall time (child interpreter: start, import and context set-up included; in-proc: the measured cases alone), and the
error closest to its bound over both runs (the scenario's routes and the default routes of the same cases):

    scenario          switches                                      time    where    operation          error    bound
    alds0             ALDS=0                                         4.9 s child    kkt_x              1.5e-15  2.0e-13
    alds_dyn0         ALDS_DYN=0                                     4.1 s child    kkt_x              1.2e-15  2.0e-13
    alds_fill0        ALDS_FILL=0                                    3.7 s child    kkt_x              1.4e-15  2.0e-13
    asm_t             ASM=t                                          3.0 s child    hessian_gram       2.9e-16  4.4e-14
    chol_prep0        CHOL_PREP=0                                    3.2 s child    projected_inverse  9.5e-16  8.4e-14
    default_small     (default routes)                               0.5 s in-proc  llt                2.1e-16  1.8e-14
    down_w0           DOWN_W=0                                       2.6 s child    hessian            1.4e-15  1.9e-13
    fac_partial0      FAC_PARTIAL=0                                  3.0 s child    projected_inverse  8.3e-16  8.4e-14
    faci_lds0         FACI_LDS=0                                     2.5 s child    hessian_gram       2.9e-16  4.4e-14
    fam0              FAM=0                                          2.9 s child    projected_inverse  6.7e-16  8.4e-14
    fam2_0            FAM2=0                                         2.8 s child    kkt_x              1.4e-15  2.0e-13
    famt0             FAMT=0                                         2.8 s child    kkt_x              1.4e-15  2.0e-13
    famt_group0       FAMT_GROUP=0                                   2.5 s child    kkt_x              1.1e-15  2.0e-13
    flow0             FLOW=0                                         2.6 s child    projected_inverse  8.5e-16  8.4e-14
    flow_wg5          FLOW_WG=5                                      2.5 s child    projected_inverse  8.5e-16  8.4e-14
    fz0               FZ=0                                           3.9 s child    kkt_x              1.4e-15  2.0e-13
    fz_tail0          FZ_TAIL=0                                      4.7 s child    kkt_x              1.5e-15  2.0e-13
    generic           GENERIC=1                                      2.5 s child    hessian_adjoint    5.8e-17  6.9e-15
    gram0             GRAM=0                                         3.0 s child    kkt_x              1.8e-15  2.0e-13
    gram_side         GRAM_EARLY=1 LG_SIDE=0                         4.0 s child    hessian_gram       6.1e-16  4.4e-14
    large0            LARGE=0                                        3.1 s child    hessian_gram       6.2e-16  4.4e-14
    leafgram0         LEAFGRAM=0                                     2.9 s child    kkt_x              1.4e-15  2.0e-13
    lfsp0             LFSP=0                                         2.7 s child    hessian_gram       2.9e-16  4.4e-14
    lg_early0         LG_EARLY=0                                     4.0 s child    hessian_gram       6.1e-16  4.4e-14
    mid0              MID=0                                          2.9 s child    projected_inverse  7.9e-16  8.4e-14
    n16_0             N16=0                                          2.7 s child    hessian            1.5e-15  1.9e-13
    oldlds1           OLDLDS=1                                       2.4 s child    hessian            1.4e-15  1.9e-13
    pd1               PD=1                                           3.5 s child    hessian_gram       6.1e-16  4.4e-14
    products_mm0      TRMM_MM=0 SYR2K_MM=0 SYMM_MM=0 LOWRANK_MM=0    3.6 s child    -                  0.0e+00  0.0e+00
    products_mm2      TRMM_MM=2 SYR2K_MM=2 SYMM_MM=2                 2.7 s child    -                  0.0e+00  0.0e+00
    qr_trsm_f         QR_TRSM=f                                      2.6 s child    kkt_x              1.3e-15  2.0e-13
    scaling_overlap0  SCALING_OVERLAP=0                              2.9 s child    projected_inverse  8.3e-16  8.4e-14
    scm0              SCM=0                                          2.6 s child    kkt_x              1.6e-15  2.0e-13
    streams           FORK=0 NOCACHE=1 POTRF_DEFER=0                 3.6 s child    hessian_gram       6.1e-16  4.4e-14
    trsm_mm0          TRSM_MM=0                                      2.6 s child    trsm               6.1e-16  8.6e-14
    trtri0            TRTRI=0                                        2.6 s child    projected_inverse  6.0e-16  8.4e-14
    units             (default routes)                               5.5 s child    kkt_x              9.6e-16  2.0e-13
    zsp0              ZSP=0                                          2.6 s child    kkt_x              1.4e-15  2.0e-13

The units of the scenarios `units`, `products_mm0` and `products_mm2` assert inside their own modules (no figure here).
No bound was exceeded and no signature failed; every one of the 142 kernel ids was launched by a passing scenario, so
EXEMPT_KERNELS and DEAD_KERNELS are empty.
"""
import os
import tempfile

import pytest

from tests import dense_ref
from tests import route_ledger as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# measured wall time of every child, seconds (same run as the table above); a child's timeout is ten times that, rounded up, and
# at least 120 s: a limit that ends trouble, not a performance claim
CHILD_SECONDS = {"alds0": 4.9, "alds_dyn0": 4.1, "alds_fill0": 3.7, "asm_t": 3.0, "chol_prep0": 3.2,
                 "down_w0": 2.6, "fac_partial0": 3.0, "faci_lds0": 2.5, "fam0": 2.9, "fam2_0": 2.8,
                 "famt0": 2.8, "famt_group0": 2.5, "flow0": 2.6, "flow_wg5": 2.5, "fz0": 3.9,
                 "fz_tail0": 4.7, "generic": 2.5, "gram0": 3.0, "gram_side": 4.0, "large0": 3.1,
                 "leafgram0": 2.9, "lfsp0": 2.7, "lg_early0": 4.0, "mid0": 2.9, "n16_0": 2.7,
                 "oldlds1": 2.4, "pd1": 3.5, "products_mm0": 3.6, "products_mm2": 2.7, "qr_trsm_f": 2.6,
                 "scaling_overlap0": 2.9, "scm0": 2.6, "streams": 3.6, "trsm_mm0": 2.6, "trtri0": 2.6,
                 "units": 5.5, "zsp0": 2.6}


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
            assert scn["ran"] or scn["gone"] or scn["note"].startswith("not observable"), name


def test_exempt_and_dead_kernel_lists_are_within_their_caps():
    assert len(rl.EXEMPT_KERNELS) <= rl.MAX_EXEMPT_KERNELS == 8
    assert not set(rl.EXEMPT_KERNELS) & set(rl.DEAD_KERNELS)
    assert all(isinstance(r, str) and len(r) > 20 for r in list(rl.EXEMPT_KERNELS.values()) + list(rl.DEAD_KERNELS.values()))


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
    yard, own = dense_ref.load_yardstick(), rl.load_ledger_yardstick()
    bound = lambda pattern, op: rl.bound_of(pattern, op, yard, own)
    bad = rl.error_faults(rec["run"], scn["cases"], bound)
    judged = [rl.case_key(c) for c in scn["cases"][:scn["sig_over"]]]
    if not bad:
        bad += rl.signature_faults(rl.union_counts({k: rec["run"][k] for k in judged}), scn["ran"], scn["gone"])
    if scn["env"]:
        dflt = rec["default"] or {}
        dbad = rl.error_faults(dflt, scn["cases"], bound)
        if not dbad:
            dbad = rl.signature_faults(rl.union_counts({k: dflt[k] for k in judged}), scn["gone"], scn["ran"])
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
    listed = set(rl.EXEMPT_KERNELS) | set(rl.DEAD_KERNELS)
    assert listed <= set(names), sorted(listed - set(names))
    unchecked = [k for k in names if k not in by and k not in listed]
    assert not unchecked, "kernels that no passing scenario launches: %s" % unchecked
    stale = sorted(k for k in listed if k in by)
    assert not stale, "exempt or dead, but launched: %s" % {k: by[k] for k in stale}
