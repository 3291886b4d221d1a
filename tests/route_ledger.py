"""The route ledger: which checked computation launches which kernel, and which one shows each route switch taking effect.

A SCENARIO is a set of switches (its `env`; empty = the default routes), an optional csp_tune setting, a list of cases and a
SIGNATURE: the kernel ids that must have run (`ran`) and the ones that must not (`gone`) while the cases were measured, and the
same over the kernel FUNCTIONS (`ran_k`, `gone_k`: an id stands for a group of kernels; the launch census of csp_census_* names
the function that was launched, one name per template instantiation).  A case is
either a pattern with the parts of dense_ref.measure to run on it (every error is bounded by dense_ref.device_bound) or a UNIT:
one small call of a unit outside dense_ref.measure, checked by that unit's own reference at that unit's own bound (the helper
or test function of its GPU module is called as it stands).  Every case runs inside helpers.launch_counts and helpers.kernel_census.

The switches are cached per process, so a scenario with a non-empty `env` runs in a child interpreter:

    python tests/route_ledger.py <scenario> <out.json>        ->  {case: {"errors": {...}, "counts": {...}, "kernels": {...}, "seconds": s}}

and the same cases run once more on the default routes, where the OPPOSITE signature must hold (a scenario whose cases never
reach the route it claims to replace fails).  tests/test_gpu_route_ledger.py holds the tests; its docstring holds the measured
figures.  A new kernel, a new route switch or a launch past the launch helpers must enter this file.
"""
import contextlib
import fnmatch
import json
import os
import re
import subprocess
import sys
import time
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from smcp_amd import problems                                  # noqa: E402
from tests import dense_ref                                    # noqa: E402
from tests.helpers import GPU_PATTERNS                         # noqa: E402

SWITCHES_HPP = os.path.join(ROOT, "smcp_amd", "csrc", "switches.hpp")
YARDSTICK_FILE = os.path.join(HERE, "golden", "route_ledger_yardstick.json")
ALL = ("tree", "scaling", "hessian", "trsm", "kkt")


# ---- patterns ----------------------------------------------------------------------------------------------------------
def _two_fronts():
    """two dense fronts that share nothing: 130 columns (three tiles, the last with two columns) and 275 (beyond the
    one-workgroup class of 272 rows, five tiles, the last with nineteen columns)"""
    a, b = np.arange(130), np.arange(130, 405)
    return problems._from_cliques(405, [(a, a), (b, b)])


# the patterns of the ledger that are not in helpers.GPU_PATTERNS; their oracle-vs-dense errors are recorded in
# tests/golden/route_ledger_yardstick.json (make_route_ledger_yardstick.py) and bounded by tests/test_gpu_route_ledger.py
NEW_PATTERNS = {
    "band130": lambda: problems.band_pattern(130, 129),
    "band275": lambda: problems.band_pattern(275, 274),
    "two_fronts": _two_fronts,
    "dense450": lambda: problems.band_pattern(450, 449),       # test_kkt_wide_dense_clique_sparse_first_phase
    "fan40": lambda: problems.nested_block_arrow_pattern(nsub=1, nmid=40, nleaf_per_mid=2, seed=11),   # test_kkt_few_fronts_many_children_...
    # eight top fronts in one level: with 40 right-hand sides 320 (front, right-hand side) pairs, more than the 256 CUs
    "tops8": lambda: problems.nested_block_arrow_pattern(nsub=8, nmid=2, nleaf_per_mid=2, seed=5),
    # nine family parents that share one separator (test_kkt_family_sibling_groups_send_one_summed_update): groups of 8 + 1
    "fam_shared": lambda: problems.nested_block_arrow_pattern(nsub=1, nmid=9, nleaf_per_mid=3, seed=71, shared_mid_sep=True),
    # eight large fronts (nf = 130: beyond the LDS class, within the streaming extend-add) in one level, sixteen family parents under
    # each: with 40 sparse-input right-hand sides 40 queues of eight (front, right-hand side) pairs on 32 queues of workgroups, so
    # the last round holds eight queues of 32 and is dealt in shares of the pairs' children (launch_assemble_fz: tail_first = 32, nzt = 2)
    "tail8": lambda: problems.nested_block_arrow_pattern(nsub=8, nmid=16, nleaf_per_mid=2, leaf=(2, 9), mid=(4, 20), top=(30, 100), root=110),
    # ONE such front with 32 family parents under it: with 20 right-hand sides 20 pairs, fewer than half the CUs, each with 32 children:
    # alds_route deals the children of every pair over two workgroups (launch_assemble_fz: tail_first = 0, every pair shared)
    "fan32": lambda: problems.nested_block_arrow_pattern(nsub=1, nmid=32, nleaf_per_mid=2, leaf=(2, 9), mid=(4, 20), top=(30, 100), root=110),
}
LEDGER_PATTERNS = dict(GPU_PATTERNS)
LEDGER_PATTERNS.update(NEW_PATTERNS)


# ---- cases -------------------------------------------------------------------------------------------------------------
def C(pattern, parts, nrhs=1, m=None, density=None, seed=None, max_rhs=4, tnzcols=None, route="chol", mix=None):
    """a measured case: pattern, parts of dense_ref.measure ('scaling': cholesky_projected_inverse in one call, with and without
    the separator factors), right-hand sides of the Hessians, and the KKT input (m, density, seed: dense_ref's recipe unless
    given; max_rhs also sizes the context; mix: the order of a mixed recipe, dense_ref.interleave -- m counts its wide
    constraints, which tnzcols must send through the Hessian and the others to the SCMcolumn2 columns: the hybrid Schur route)"""
    kkt = dict(m=m, density=density, seed=seed, max_rhs=max_rhs, tnzcols=tnzcols, route=route, mix=mix)
    return ("case", pattern, tuple(parts), nrhs, kkt)


def U(unit):
    return ("unit", unit)


def case_key(case):
    if case[0] == "unit":
        return "unit:" + case[1]
    _, pattern, parts, nrhs, kkt = case
    key = "%s|%s|nrhs=%d" % (pattern, "+".join(parts), nrhs)
    if "kkt" in parts:
        key += "|" + ",".join("%s=%s" % kv for kv in sorted(kkt.items()) if kv[1] is not None)
    return key


class _Capsys:
    """what the test functions of the units ask of pytest's capsys"""

    def disabled(self):
        return contextlib.nullcontext()


def _units():
    """unit -> calls (module, function, arguments): the unit's own check at its own bound, at its smallest shapes that take
    every kernel of the unit"""
    cap = _Capsys()
    return {
        # 1, 3 and 7 columns: the three column blocks of the FMA kernels (1, up to 4, wider; with_column_block in products.hip)
        "trmm": [("tests.test_gpu_trmm", "check_definition", ("arrow_big", (1, 70))), ("tests.test_gpu_trmm", "check_definition", ("fam_odd", (3, 7)))],
        "symm": [("tests.test_gpu_symm", "check_definition", ("arrow_big", (1, 70))), ("tests.test_gpu_symm", "check_definition", ("fam_odd", (3, 7)))],
        "syr2k": [("tests.test_gpu_syr2k", "check_definition", ("arrow_big", (1, 17))), ("tests.test_gpu_syr2k", "check_definition", ("fam_odd", (3,)))],
        "trmm_wide": [("tests.test_gpu_trmm", "check_definition", ("nested_mid", (70,)))],
        "syr2k_wide": [("tests.test_gpu_syr2k", "check_definition", ("nested_mid", (70,)))],
        "symm_1col": [("tests.test_gpu_symm", "check_definition", ("nested_mid", (1,)))],
        "lowrank": [("tests.test_gpu_lowrank", "run_grid", ("arrow_big", ((7, 7), (17, 70)))), ("tests.test_gpu_lowrank", "run_grid", ("rand2", ((8, 17),)))],
        "mrcompletion": [("test_gpu_mrcompletion", "test_parity_patterns", ("nested", 3)), ("test_gpu_mrcompletion", "test_parity_patterns", ("arrow", None))],
        "maxcut_round": [("test_gpu_mrcompletion", "test_maxcut_n200_end_to_end", (cap,))],
        "edmcompletion": [("test_gpu_edmcompletion", "test_parity_patterns", ("nested", 2)), ("test_gpu_edmcompletion", "test_dense", ("arrow", 2))],
        "psdcompletion": [("test_gpu_psdcompletion", "test_parity_pd_known_answer", ("nested", cap)),
                          ("test_gpu_psdcompletion", "test_parity_low_rank_known_answer", ("arrow", cap))],
        "clique_eigvalsh": [("test_gpu_clique_eig", "test_parity_and_contract", ("fam_odd", "definite", cap)),
                            ("test_gpu_clique_eig", "test_parity_and_contract", ("fam_odd", "pencil", cap))],
        "solve_many": [("tests.test_gpu_solve_many", "test_rows_against_the_oracle", ("nested", 3)),
                       ("tests.test_gpu_solve_many", "test_dense_block_solve_against_numpy", (129,))],
        "solve_many_qr": [("tests.test_gpu_solve_many_qr", "test_rows_against_the_oracle", ("nested", 3)),
                          ("tests.test_gpu_solve_many_qr", "test_block_edges", (130,))],
        "residual_refine": [("tests.test_gpu_kkt_residual", "test_rows_against_the_oracle", ("nested", 3)),
                            ("tests.test_gpu_kkt_residual", "test_refinement_does_its_work", ())],
        "dense_potrf_potrs": [("tests.test_gpu_parity", "test_dense_potrf_potrs", (5, 0)), ("tests.test_gpu_parity", "test_dense_potrf_potrs", (130, 0)),
                              ("tests.test_gpu_parity", "test_dense_potrs_of_an_uploaded_factor", (130,))],
        # ---- kernels of the KKT solves that the other cases do not reach: the chip-wide substitution steps of dense_potrs beyond
        # order 1024 (k_dense_trsv_step); the panels of the stack's triangular solve beyond 320 constraints (k_stack_gemm_panel);
        # the shifted Gram matrix of a nearly dependent stack under deferred status (k_qr_shift, k_latch_status)
        "dense_potrs_steps": [("tests.test_gpu_parity", "test_dense_potrf_potrs", (1027, 5))],
        "qr_panels": [("tests.test_gpu_parity", "test_kkt_qr_more_than_320_constraints", ())],
        "qr_shifted": [("tests.test_gpu_parity", "test_kkt_qr_nearly_dependent_constraints", (1e-13, True, True))],
        # the failure flag latched on the device (k_latch_status): a deferred solve against the eager one, and the report of a failure
        "deferred_status": [("tests.test_gpu_parity", "test_deferred_status", ("arrow",))],
        # the residuals alone (the refinement of residual_refine factors by QR, which the generic route does not hold)
        "residual_rows": [("tests.test_gpu_kkt_residual", "test_rows_against_the_oracle", ("nested", 3))],
        # ---- the units behind borrowed kernel ids (KID_ceig, KID_ceig_reduce, KID_gather_level, KID_axpby, KID_vec_axpby,
        # KID_qr_small, KID_lr_apply, KID_lr_small, KID_syr2k_fma, KID_syr2k_mm): the census names their kernels.
        # class_edges: both sides of every LDS class of the Jacobi kernels; fam_odd: gathers and scatters over a tree with levels
        "clique_eigh": [("test_gpu_clique_eigh", "test_eigh_against_lapack", ("class_edges", "indefinite", cap)),
                        ("test_gpu_clique_eigh", "test_project_against_lapack", ("class_edges", "indefinite", cap)),
                        ("test_gpu_clique_eigh", "test_gather_and_scatter_against_dense_definitions", ("fam_odd",))],
        "cone_project": [("test_gpu_cone_project", "test_three_iterations_against_the_restatement", ("nested", "noisy", 1.0, 1.7, cap)),
                         ("test_gpu_cone_project", "test_three_iterations_against_the_restatement", ("class_edges", "indef", 3.0, 1.0, cap))],
        # the chip-wide block Jacobi: orders 64 .. 161 (two to six blocks of 32 rows and the ragged last blocks): eigenvalues, vectors, projections
        "clique_wide": [("test_gpu_clique_wide", "test_parity_and_contract", ("wide_edges", "indefinite", cap)),
                        ("test_gpu_clique_wide", "test_block_sweeps_against_restatement", (65, "indefinite", cap))],
        "cone_wide": [("test_gpu_cone_wide", "test_three_iterations_against_the_restatement", ("wide_root70", "indef", 1.0, 1.7, cap))],
        "pencil_wide": [("test_gpu_pencil_wide", "parity_run", ("wide_edges",)), ("test_gpu_pencil_wide", "test_max_step_along_minus_x", ("wide_edges", cap))],
        # dense: the smallest pattern of FULL (n = 9); random65: a tridiagonal matrix of more rows than a wave has lanes
        "dual_step": [("test_gpu_lanczos", "test_full_krylov_both_forms", ("dense", cap)),
                      ("test_gpu_lanczos", "test_ritz_kernel_against_eigh_tridiagonal", ("random65", cap))],
        # ranks 1 .. 64 (17: the second, ragged pass) on a deep tree of small cliques; ranks 1 and 17 on separators beyond LDS
        "chol_update": [("test_gpu_chol_update", "test_definition", ("band",)), ("test_gpu_chol_update", "test_definition", ("arrow_thin",))],
        # band: the item arm alone (k_cdec_fma); arrow_big: 3 x 3 tiles in the root, the tile arm (k_cdec_mm)
        "clique_decompose": [("test_gpu_clique_decompose", "test_definition", ("band",)), ("test_gpu_clique_decompose", "test_definition", ("arrow_big",))],
    }


PRODUCT_UNITS = [U("trmm"), U("symm"), U("syr2k"), U("lowrank"), U("solve_many")]
ALL_UNITS = PRODUCT_UNITS + [U("trmm_wide"), U("syr2k_wide"), U("symm_1col"), U("mrcompletion"), U("maxcut_round"), U("edmcompletion"), U("psdcompletion"), U("clique_eigvalsh"),
                             U("solve_many_qr"), U("residual_refine"), U("residual_rows"), U("dense_potrf_potrs")]
SPECTRA_UNITS = [U("clique_eigh"), U("cone_project"), U("clique_wide"), U("cone_wide"), U("pencil_wide"), U("dual_step")]
FACTOR_UNITS = [U("chol_update"), U("clique_decompose")]
KKT_UNITS = [U("dense_potrs_steps"), U("qr_panels"), U("qr_shifted"), U("deferred_status")]

# KKT inputs of tests/test_gpu_parity.py that select a route (m, density, seed as there; tnzcols = 0: every constraint swept)
FAM_SPARSE = [C("nested_mid", ("kkt",), m=12, density=0.002, seed=13, max_rhs=12, tnzcols=0.0),
              C("fam_odd", ("kkt",), m=10, density=0.03, seed=13, max_rhs=10, tnzcols=0.0)]
FZ_CASE = C("nested_mid", ("kkt",), m=40, density=0.002, seed=33, max_rhs=40, tnzcols=0.0)
FAN_CASE = C("fan40", ("kkt",), m=20, density=0.01, seed=62, max_rhs=20, tnzcols=0.0)
THIN_CASE = C("arrow_thin", ("hessian", "kkt"), nrhs=8, m=40, density=0.03, seed=32, max_rhs=40, tnzcols=0.0)
LFSP_CASE = C("arrow_big", ("kkt",), m=6, density=0.004, seed=52, max_rhs=6, tnzcols=0.0)
ZSP_CASE = C("dense450", ("kkt",), m=5, density=0.01, seed=42, max_rhs=3, tnzcols=0.0)
DYN_CASE = C("tops8", ("kkt",), m=40, density=0.004, seed=5, max_rhs=40, tnzcols=0.0)
SHARED_CASE = C("fam_shared", ("kkt",), m=13, density=0.003, seed=73, max_rhs=13, tnzcols=0.0)
GRAM130 = C("nested", ("kkt",), m=130, density=0.05, seed=9)      # more than one 128-block of constraints: k_gram_partial
# the thin last round of the fused extend-add (k_lf_zero_pairs behind SMCP_FZ_TAIL) and the pairs shared from the start
# (tail_first = 0: it does not depend on that switch); entries per constraint within 4 * nsn, so that the extend-add stays fused
TAIL_CASE = C("tail8", ("kkt",), m=40, density=0.002, seed=33, max_rhs=40, tnzcols=0.0)
PAIRS_CASE = C("fan32", ("kkt",), m=20, density=0.004, seed=62, max_rhs=20, tnzcols=0.0)


def hybrid(case, tnzcols):
    """the hybrid variant of a sparse-input case: its constraints as the wide class (same m, density, seed, max_rhs: within
    cnnz <= 4 * nsn * m and m <= max_rhs, so the entry-driven family kernels and the fused extend-add stay live, now reading the
    swept subset through kc_ids), 4 few + 3 single dealt among them; the KKT part alone"""
    k = case[4]
    return C(case[1], ("kkt",), m=k["m"], density=k["density"], seed=k["seed"], max_rhs=k["max_rhs"], tnzcols=tnzcols,
             mix=dense_ref.interleave(k["m"], 4, 3))


# tnzcols: int(n * tnzcols) lies between the 6 rows / columns a narrow constraint touches at most and what the wide ones touch
# (test_hybrid_recipes.py holds that on a CPU for every case; the device's classification is asserted where the case runs)
FAM_HYBRID = [hybrid(FAM_SPARSE[0], 0.1), hybrid(FAM_SPARSE[1], 0.1)]
FZ_HYBRID = hybrid(FZ_CASE, 0.1)
THIN_HYBRID = hybrid(THIN_CASE, 0.1)
LFSP_HYBRID = hybrid(LFSP_CASE, 0.1)
DYN_HYBRID = hybrid(DYN_CASE, 0.1)
SHARED_HYBRID = hybrid(SHARED_CASE, 0.1)
PAIRS_HYBRID = hybrid(PAIRS_CASE, 0.1)
NESTED_HYBRID = C("nested", ("kkt",), m=5, density=0.05, seed=9, max_rhs=5, tnzcols=0.2, mix=dense_ref.interleave(5, 4, 3))
HYBRIDS = [NESTED_HYBRID] + FAM_HYBRID + [FZ_HYBRID, THIN_HYBRID, LFSP_HYBRID, DYN_HYBRID, SHARED_HYBRID, PAIRS_HYBRID]
EVERYTHING = [C("nested_mid", ALL), C("arrow_big", ALL), C("nested_mid", ("hessian",), nrhs=4)]


def S(env, cases, ran=(), gone=(), tune=None, note="", sig_over=None, ran_k=(), gone_k=()):
    """sig_over: the signature is judged on the first sig_over cases only (the others are there for their numerics)"""
    return dict(env=env, cases=cases, ran=list(ran), gone=list(gone), ran_k=list(ran_k), gone_k=list(gone_k), tune=tune or {}, note=note,
                sig_over=sig_over)


# name -> scenario.  `ran` / `gone`: kernel names (fnmatch patterns) over the union of the scenario's cases: every `ran`
# pattern has a launch and no `gone` pattern has one; on the default routes the other way round.  The lists are what the
# launch sites say and what both runs showed on the MI355X; `ran_k` / `gone_k`: the same over the kernel functions of the
# census (k_hess_down_w<2>: one name per instantiation); `note` says where neither count can show the switch.
SCENARIOS = {
    # ---- the default routes: every unit outside dense_ref.measure, and the measured cases that no switch below runs
    "units": S({}, ALL_UNITS + [C("nested", ("kkt",), route="qr"), C("band", ("kkt",), route="qr")]),
    "default_small": S({}, [C(name, ALL) for name in ("band", "rand1", "rand2", "diag", "dense", "arrow")]
                       + [C("dense600", ("tree", "scaling", "hessian")), C("arrow_one", ("tree", "scaling", "hessian", "kkt")),
                          C("fam_top", ("hessian", "kkt"), nrhs=4), C("rand2", ("hessian",), nrhs=4), GRAM130]),
    # the units that run behind borrowed kernel ids, in two children so that neither grows long
    "units_spectra": S({}, SPECTRA_UNITS),
    "units_factor": S({}, FACTOR_UNITS),
    "units_kkt": S({}, KKT_UNITS),
    # the hybrid Schur route on the default routes: the Gram block of the swept subset scattered into H (k_scatter_hd) beside the
    # SCMcolumn2 columns (k_unit_columns, k_scm_columns); the scenarios below run the same cases where a switch changes a kernel
    # that reads the subset through kc_ids
    "hybrid": S({}, HYBRIDS, ran_k=["k_scatter_hd", "k_scm_columns", "k_unit_columns"]),
}


def _add(name, env, cases, **kw):
    SCENARIOS[name] = S(env, cases, **kw)


_add("generic", {"SMCP_GENERIC": "1"}, [C("rand2", ALL), C("arrow_thin", ALL), C("nested", ("hessian", "kkt"), nrhs=4), U("residual_rows")],
     ran_k=["k_res_combine_cliques"], gone_k=["k_res_combine"],
     ran=["k_chol_level", "k_llt_level", "k_pinv_level", "k_completion_all", "k_hess_up_level", "k_hess_down_level", "k_hess_up_inv_level",
          "k_hess_down_inv_all", "k_factor_yaa", "k_scale_an"],
     gone=["k_chol_mfma<*", "k_pinv_mfma<*", "k_llt_mfma<*", "k_completion_mfma<*", "k_hess_down_mfma<*", "k_hess_up_inv_mfma<*",
           "k_hess_down_inv_mfma<*", "k_hess_up_n16", "k_hess_up_fam*", "k_hess_down_fam", "k_lf_*", "k_mid_chol", "k_top_chol",
           "k_factor_yaa_lds", "k_factor_inverse_lds", "k_gram_*", "k_fam_terms", "k_chol_fam", "k_pinv_fam"])
_add("large0", {"SMCP_LARGE": "0"}, [C("arrow_thin", ALL), C("arrow_big", ALL), C("arrow_big", ("hessian",), nrhs=4)],
     ran=["k_chol_mfma<false>", "k_pinv_mfma<false>", "k_llt_mfma<false>", "k_completion_mfma<false>", "k_hess_up_mfma<false>",
          "k_hess_down_mfma<false>", "k_hess_down_inv_mfma<false>", "k_factor_inverse", "k_factor_yaa"],
     gone=["k_lf_*", "k_mid_chol", "k_top_chol"])
_add("mid0", {"SMCP_MID": "0"}, [C("arrow_big", ALL), C("band130", ALL)],
     ran=["k_lf_chol_panel", "k_lf_chol_trail"], gone=["k_mid_chol", "k_top_chol", "k_lf_diag_inv"],
     note="k_lf_diag, k_lf_prep_s and k_lf_prep_row run on both routes (the Y_AA blocks of arrow_big take them by default)")
_add("trtri0", {"SMCP_TRTRI": "0"}, [C("two_fronts", ("tree", "hessian", "kkt")), C("two_fronts", ("hessian",), nrhs=4)],
     gone=["k_lf_trtri"], note="k_lf_prep_s and k_lf_prep_row run on both routes (the 275-column front takes them for its rows beyond 128)")
_add("flow0", {"SMCP_FLOW": "0"}, [C("band275", ALL), C("three_tops", ("tree", "scaling", "hessian")), U("dense_potrf_potrs")],
     gone=["k_chol_flow"], note="the per-step kernels k_lf_diag / k_lf_chol_panel / k_lf_chol_trail run on both routes (three_tops' fronts with separators)")
_add("flow_wg5", {"SMCP_FLOW_WG": "5"}, [C("band275", ("tree", "scaling")), C("three_tops", ("tree", "scaling"))],
     note="not observable: the same kernel on fewer workgroups")
_N16 = [C("nested", ("hessian", "kkt")), C("fam_odd", ("hessian", "kkt")), C("nested", ("hessian",), nrhs=4), C("fam_odd", ("hessian",), nrhs=4)]
_add("n16_0", {"SMCP_N16": "0"}, _N16 + FAM_HYBRID, gone=["k_hess_up_n16"], note="k_hess_up_pad runs on both routes (fam_odd's shapes beyond n16)")
_add("oldlds1", {"SMCP_OLDLDS": "1"}, _N16, ran=["k_hess_up_mfma<true>"], gone=["k_hess_up_n16", "k_hess_up_pad"])
_add("down_w0", {"SMCP_DOWN_W": "0"}, _N16, gone_k=["k_hess_down_w<*"],
     note="the id k_hess_down_mfma<true> holds k_hess_down_w<1..4> and k_hess_down_mfma<true, *>: only the census shows the switch")
_add("fam0", {"SMCP_FAM": "0"}, [C(name, ("scaling", "hessian", "kkt"), nrhs=nrhs) for name in ("fam_odd", "fam_max", "fam_nine") for nrhs in (1, 4)],
     gone=["k_hess_up_fam", "k_hess_up_fam1", "k_hess_down_fam", "k_fam_terms", "k_famt_prep", "k_chol_fam", "k_pinv_fam", "k_leaf_*"])
_add("fam2_0", {"SMCP_FAM2": "0"}, FAM_SPARSE + FAM_HYBRID, tune={"LEAFGRAM": 2}, ran=["k_hess_up_fam"], gone=["k_fam_terms", "k_famt_prep"],
     note="k_fam_sparse runs on neither route here: the default is the entry-driven k_fam_terms")
_add("famt0", {"SMCP_FAMT": "0"}, FAM_SPARSE + FAM_HYBRID, tune={"LEAFGRAM": 2}, ran=["k_fam_sparse", "k_fam2_prep"], gone=["k_fam_terms", "k_famt_prep"])
_add("leafgram0", {"SMCP_LEAFGRAM": "0"}, FAM_SPARSE + FAM_HYBRID, tune={"LEAFGRAM": 2}, ran=["k_fam_sparse"], gone=["k_leaf_pairs", "k_leaf_tables", "k_fam_terms"])
_add("famt_group0", {"SMCP_FAMT_GROUP": "0"}, [SHARED_CASE, SHARED_HYBRID], ran=["k_fam_terms"], gone=["k_fam_terms_grp"])
_add("fz0", {"SMCP_FZ": "0"}, [FZ_CASE, FZ_HYBRID, PAIRS_CASE, PAIRS_HYBRID], tune={"LEAFGRAM": 2}, ran=["k_lf_assemble_lds"], gone=["k_lf_assemble_fz"],
     gone_k=["k_lf_zero_pairs"],
     note="k_lf_zero_pairs clears the update blocks of the pairs whose children the fused extend-add deals over several workgroups: on fan32 "
          "every pair from the start (alds_route: nz = 2), whatever SMCP_FZ_TAIL says")
_add("lfsp0", {"SMCP_LFSP": "0"}, [THIN_CASE, LFSP_CASE, THIN_HYBRID, LFSP_HYBRID], gone=["k_lfsp_up", "k_lfsp_prep"])
_add("zsp0", {"SMCP_ZSP": "0"}, [ZSP_CASE], ran=["k_scatter_constraints"], gone=["k_lf_zsp"])
_add("gram0", {"SMCP_GRAM": "0"}, [C("nested", ("kkt",)), C("arrow", ("kkt",)), C("nested_mid", ("kkt",)), GRAM130], gone=["k_gram_*"])
_add("scm0", {"SMCP_SCM": "0"}, [C("rand2", ("kkt",)), C("arrow", ("kkt",)), C("nested_mid", ("kkt",), tnzcols=0.2), NESTED_HYBRID, FAM_HYBRID[0]],
     gone_k=["k_scm_columns", "k_unit_columns", "k_scatter_hd"],
     note="the switch turns the column-sparse class off: every constraint is swept, the hybrid cases run as plain Gram sweeps")
_add("trsm_mm0", {"SMCP_TRSM_MM": "0"}, [C("arrow_big", ("trsm",)), C("nested_mid", ("trsm",))], gone=["k_lf_prep_k", "k_prep_lk"],
     gone_k=["k_trsm_mm_fwd", "k_trsm_mm_bwd"],
     note="the ids show the inverse-form factor the tile products need (k_prep_lk, k_lf_prep_k), the census the tile products themselves, "
          "which run under the ids of the level kernels; k_trsm_*_level run on both routes (blocks of fewer than eight columns)")
_add("alds0", {"SMCP_ALDS": "0"}, [FAN_CASE, THIN_CASE, DYN_CASE, THIN_HYBRID, DYN_HYBRID], gone=["k_lf_assemble_lds", "k_lf_assemble_lds_dyn"],
     note="k_lf_assemble (the gather plan) runs on both routes: the levels below 32 pairs")
_add("alds_dyn0", {"SMCP_ALDS_DYN": "0"}, [DYN_CASE], ran=["k_lf_assemble_lds"], gone=["k_lf_assemble_lds_dyn"])
_add("alds_fill0", {"SMCP_ALDS_FILL": "0"}, [FZ_CASE, FZ_HYBRID, THIN_CASE, THIN_HYBRID], tune={"LEAFGRAM": 2}, ran=["k_lf_assemble_lds"], gone=["k_lf_assemble_fz"], sig_over=2)
_add("asm_t", {"SMCP_ASM": "t"}, [C("arrow_big", ("hessian",), nrhs=2), THIN_CASE, C("arrow_big", ("kkt",))], ran=["k_lf_clear_upd"], ran_k=["k_lf_assemble_tiled"],
     note="the id k_lf_assemble holds the tiled kernel and the gather plan: the ids show the clear pass the tiled kernel needs, the census the kernel")
_add("fz_tail0", {"SMCP_FZ_TAIL": "0"}, [TAIL_CASE, FZ_CASE, FAN_CASE], tune={"LEAFGRAM": 2}, gone_k=["k_lf_zero_pairs"],
     note="the same k_lf_assemble_fz launch without shares in its last round: the shares show as k_lf_zero_pairs, the clear pass of the shared pairs. "
          "tail8 reaches them (40 queues of pairs on 32 queues of workgroups); nested_mid and fan40 do not and are there for their numerics")
_add("faci_lds0", {"SMCP_FACI_LDS": "0"}, [C("nested", ("hessian", "kkt")), C("fam_max", ("hessian", "kkt"))], ran=["k_factor_inverse"], gone=["k_factor_inverse_lds"])
_SCALING = [C("nested_mid", ("scaling", "hessian", "kkt")), C("fam_odd", ("scaling", "hessian", "kkt"))]
_add("chol_prep0", {"SMCP_CHOL_PREP": "0"}, [C("nested_mid", ("scaling",)), C("tops8", ("scaling",)), C("fan40", ("scaling",))] + _SCALING,
     ran=["k_prep_lk"], sig_over=3,
     note="judged on the scaling point alone of trees that take its overlapped form with supernodes of at most 16 columns in the LDS class: "
          "the Hessians and the Schur sweep launch k_prep_lk on both routes")
_add("scaling_overlap0", {"SMCP_SCALING_OVERLAP": "0"}, _SCALING, gone_k=["k_top_chol<true>", "k_chol_fam<*, true>"],
     note="the factorisations that leave the inverse-form factor behind (k_top_chol<true>, k_chol_fam<.., true>) belong to the overlapped form; "
          "their ids hold both arms: only the census shows the switch")
_add("fac_partial0", {"SMCP_FAC_PARTIAL": "0"}, _SCALING, note="not observable: the same kernels, chol(Y_AA) formed at another point")
_add("streams", {"SMCP_FORK": "0", "SMCP_NOCACHE": "1", "SMCP_POTRF_DEFER": "0"}, EVERYTHING,
     note="not observable: the same kernels on one stream, nothing reused between calls")
_add("pd1", {"SMCP_PD": "1"}, EVERYTHING, ran_k=["k_lf_up1<1>", "k_lf_down1<1>", "k_lf_pinv1<1>"], gone_k=["k_lf_*<4>"],
     note="the ids hold both launch shapes of the phase kernels of the large fronts (LAUNCH_PD: the template argument is SMCP_PD): only the census shows the switch")
_add("gram_side", {"SMCP_GRAM_EARLY": "1", "SMCP_LG_SIDE": "0"}, EVERYTHING + FAM_SPARSE, tune={"LEAFGRAM": 2},
     note="not observable: the same kernels on other streams")
_add("lg_early0", {"SMCP_LG_EARLY": "0"}, EVERYTHING + FAM_SPARSE, tune={"LEAFGRAM": 2}, note="not observable: the same kernels at another point of the sweep")
_add("qr_trsm_f", {"SMCP_QR_TRSM": "f"}, [C("nested", ("kkt",), route="qr"), C("band", ("kkt",), route="qr"), C("nested_mid", ("kkt",), route="qr")],
     ran_k=["k_stack_trsm<*"], gone_k=["k_stack_trsm_mfma<*"],
     note="the id k_stack_trsm holds both substitution kernels: only the census shows the switch")
_add("products_mm0", {"SMCP_TRMM_MM": "0", "SMCP_SYR2K_MM": "0", "SMCP_SYMM_MM": "0", "SMCP_LOWRANK_MM": "0", "SMCP_POTRS_MANY_MM": "0"}, PRODUCT_UNITS,
     gone=["k_trmm_mm", "k_syr2k_mm", "k_symm_mm"],
     gone_k=["k_trmm_mm<false>", "k_trmm_mm<true>", "k_syr2k_mm<false>", "k_syr2k_mm<true>", "k_symm_mm", "k_lr_gram<true, 1>", "k_lr_gram<true, 4>"],
     note="every arm of the tile products is named: both directions of trmm, syr2k with and without V, both widths of lowrank's Gram "
          "(the id k_lr_gram holds both routes); SMCP_POTRS_MANY_MM is not observable: the same kernel k_potrs_many_step holds both routes")
_add("products_mm2", {"SMCP_TRMM_MM": "2", "SMCP_SYR2K_MM": "2", "SMCP_SYMM_MM": "2"}, [U("trmm_wide"), U("syr2k_wide"), U("symm_1col")],
     ran=["k_trmm_n", "k_trmm_t", "k_syr2k_fma", "k_symm_mm"], ran_k=["k_trmm_n<*", "k_trmm_t<*", "k_syr2k_fma<*", "k_symm_mm"],
     note="70 columns / ranks: the default sends every front to the tile products, value 2 the large ones only; one column: value 2 sends symm's large fronts there")
# every reuse of a cached derived quantity is guarded by a fingerprint of the matrix it was derived from (csp_tune VERIFY_CACHE):
# a tune alone, so the same cases run once more without it, where neither kernel is launched
_add("verify_cache", {}, EVERYTHING, tune={"VERIFY_CACHE": 1}, ran_k=["k_diag_fingerprint", "k_fingerprint_compare"])

# switch -> the module that already runs it off its default against a dense definition or a reference
COVERED_BY = {
    "SMCP_TOP_FUSED": "tests/test_gpu_top_chol.py",
    "SMCP_SCALING_FAM": "tests/test_gpu_family_scaling.py",
    "SMCP_UP_FAM": "tests/test_gpu_family_up_single_rhs.py",
    "SMCP_DOWN_FAM": "tests/test_gpu_family_single_rhs.py",
    "SMCP_LFSP_GROUP": "tests/test_gpu_parity.py",
}
# switches that change neither arithmetic nor kernel choice, or whose results are wrong by design (at most six)
EXEMPT_SWITCHES = {
    "SMCP_AUX_PRIO": "priority of side stream 0: neither arithmetic nor kernel choice",
    "SMCP_AUX_PRIO1": "priority of side stream 1: neither arithmetic nor kernel choice",
    "SMCP_EVENT_SYSFENCE": "release scope of the internal events: neither arithmetic nor kernel choice",
    "SMCP_ROOT_FUSED": "Y_NN explicit: condition squared, for studies only (switches.hpp)",
}
MAX_EXEMPT_SWITCHES = 6
# kernels (ids or functions) that are reachable, but only at an order beyond about 1100 or with more than one rank: kernel -> the
# launch-site condition
EXEMPT_KERNELS = {
    "k_exchange_roots": "kkt.hip exchange_roots: a context with a subtree partition (csp_set_partition), more than one rank",
    "k_exchange_combine": "kkt.hip kkt_exchange_combine: a context with a subtree partition (csp_set_partition), more than one rank",
    "k_stack_rows": "kkt.hip kkt_stack_rows: the top of the tree sharded by constraint, more than one rank",
    "k_lf_root1": "capi.hip hess_up_fast: SMCP_ROOT_FUSED=1, a study switch (EXEMPT_SWITCHES: the condition number squared)",
    "k_lf_root2": "capi.hip hess_down_fast: SMCP_ROOT_FUSED=1, a study switch (EXEMPT_SWITCHES: the condition number squared)",
    "k_scatter_constraints_ids": "kkt.hip schur_gram: the hybrid Schur route when the entry tables of the sparse-input sweep are absent, which "
                                 "constraints.cpp decides: nsn * (m + 1) > 2^28 or nnz >= 2^31; no test of seconds reaches either",
}
MAX_EXEMPT_KERNELS = 6
# kernels (ids or functions) that no input reaches: kernel -> the launch site
DEAD_KERNELS = {
    "k_selftest_mma": "front_mfma.hip: the self-test of the MFMA operand map has no launch site in the library",
    "k_exchange_copy": "front_large.hip: no launch site in the library (the boundary exchange packs with k_exchange_roots)",
}
# the kernels launched past the launch helpers (hipLaunchKernelGGL outside launch / launch_lds), by source file: a new one fails
# test_direct_launch_sites_are_listed.  Those that produce a result are counted by the census at their sites; csp_axpby has no
# context, k_axpby is counted where the helpers launch it
DIRECT_LAUNCHES = {
    "setup.hip": ["k_fill_sqrt_weights", "k_replicate_plan"],
    "kkt.hip": ["k_latch_status"],
    "capi.hip": ["k_axpby", "k_diag_fingerprint", "k_fingerprint_compare", "k_latch_status", "k_probe_family_stores", "k_race_spin"],
}
# kernels the census does not count (at most four): kernel -> why
NOT_COUNTED = {
    "k_race_spin": "delay injection: a bounded spin that writes nothing, launched from inside the launch helpers",
    "k_probe_family_stores": "csp_tune PLACEMENT: a timing probe whose stores are never read",
}
MAX_NOT_COUNTED = 4
KERNEL_CENSUS_FILE = os.path.join(HERE, "golden", "kernel_census.json")
CSRC = os.path.join(ROOT, "smcp_amd", "csrc")


def _sources():
    """(file name, text without // comments) of smcp_amd/csrc"""
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as f:
            yield name, re.sub(r"//[^\n]*", "", f.read())


def source_kernels():
    """names of the __global__ functions of smcp_amd/csrc: the first k_* name with a parameter list behind the keyword (launch
    bounds and attributes stand between them); a kernel of another name shows as a difference to the library's symbols"""
    out = set()
    for _, text in _sources():
        out |= set(re.findall(r"__global__\b[^;{]*?\b(k_\w+)\s*\(", text))
    return out


def direct_launches():
    """source file -> sorted names of the kernels at its hipLaunchKernelGGL sites, the two launch helpers (`kern`) left out"""
    out = {}
    for name, text in _sources():
        found = sorted(set(re.findall(r"hipLaunchKernelGGL\(\s*([A-Za-z_]\w*)", text)) - {"kern"})
        if found:
            out[name] = found
    return out


def load_kernel_census():
    """the instantiations that no passing scenario launches: mangled -> {"kernel": pretty, "condition": what selects it at its launch site}"""
    with open(KERNEL_CENSUS_FILE) as f:
        return json.load(f)


def route_switches():
    """names of the "routes" section of switches.hpp"""
    with open(SWITCHES_HPP) as f:
        text = f.read()
    section = re.search(r"// ---- routes.*?\n(.*?)\n\s*// ----", text, re.S).group(1)
    return re.findall(r'\{"(SMCP_[A-Z0-9_]+)"', section)


# ---- running -----------------------------------------------------------------------------------------------------------
_CTX, _SETUP, _UNIT_CONTEXTS = {}, {}, []


def _context(pattern, max_rhs):
    """(Symbolic with a device context, DenseCase) of a pattern, made once per process; the census of its device_init is kept
    in _SETUP for the first case that runs on it"""
    from oracle import oracle as orc
    from smcp_amd import _lib
    from smcp_amd.symbolic import Symbolic
    from tests.helpers import census_read
    key = (pattern, max_rhs)
    if key not in _CTX:
        pat = LEDGER_PATTERNS[pattern]()
        symb = Symbolic(pat)
        _lib.lib().csp_census_enable(symb.handle, 1)
        symb.device_init(0, max_rhs)
        _SETUP[key] = census_read(symb.handle)
        _lib.lib().csp_census_enable(symb.handle, 0)
        _CTX[key] = (symb, dense_ref.DenseCase(pat, orc.Sym(symb), dense_ref.YARDSTICK_SEED))
    return _CTX[key]


def recipe_of(kkt):
    """(m, density, seed) or, mixed, (m, density, seed, mix) of a case's KKT input"""
    recipe = (kkt["m"] or dense_ref.KKT_M, kkt["density"] or dense_ref.KKT_DENSITY, kkt["seed"] or dense_ref.KKT_SEED)
    return recipe + (kkt["mix"],) if kkt.get("mix") else recipe


def classes_of(kkt):
    """(swept, sparse) a hybrid case must be classified as; None for a plain recipe"""
    mix = kkt.get("mix")
    return (mix.count("w"), len(mix) - mix.count("w")) if mix else None


def set_recipe(case, kkt):
    """the KKT input of a case: dense_ref's recipe unless the case names its own"""
    recipe = recipe_of(kkt)
    if case.kkt_recipe != recipe:
        case.kkt_recipe, case._kkt = recipe, None


def _scaling_errors(symb, case):
    """the dual scaling point in ONE call, with and without the separator factors left behind (tests/test_gpu_dense_ref.py)"""
    from smcp_amd import chordal
    out = {"cholesky": 0.0, "projected_inverse": 0.0}
    for factors in (True, False):
        L, Y = dense_ref.to_dev(symb, case.Ablk), dense_ref.to_dev(symb, np.zeros(symb.blklen))
        chordal.cholesky_projected_inverse(L, Y, factors=factors)
        out["cholesky"] = max(out["cholesky"], dense_ref.blockwise(case.S, dense_ref.to_host(L), case.cholesky())[1])
        out["projected_inverse"] = max(out["projected_inverse"], dense_ref.blockwise(case.S, dense_ref.to_host(Y), case.Yblk)[1])
    return out


def run_measured(case_, tune):
    from smcp_amd import chordal
    from tests.helpers import kernel_census, launch_counts
    _, pattern, parts, nrhs, kkt = case_
    symb, case = _context(pattern, max(4, kkt["max_rhs"], nrhs))
    classes = classes_of(kkt)
    if classes and os.environ.get("SMCP_SCM") == "0":              # the switch that turns the sparse class off: every constraint swept
        classes = (sum(classes), 0)
    kernels = _SETUP.pop((pattern, max(4, kkt["max_rhs"], nrhs)), {})
    set_recipe(case, kkt)
    errs = {}

    def merge(new):
        for op, e in new.items():
            errs[op] = max(errs.get(op, 0.0), float(e))

    def run():
        ops = dense_ref.device_ops(symb, case, route=kkt["route"], tnzcols=kkt["tnzcols"], max_rhs=kkt["max_rhs"], classes=classes)
        if "scaling" in parts:
            merge(_scaling_errors(symb, case))
        merge(dense_ref.measure(case, ops, nrhs=nrhs, parts=tuple(p for p in parts if p != "scaling")))

    for what, value in tune.items():
        chordal.tune(symb, getattr(chordal, "TUNE_" + what), value)
    box = {}
    try:
        for k, v in kernel_census(symb, lambda: box.update(counts=launch_counts(symb, run))).items():
            kernels[k] = kernels.get(k, 0) + v
    finally:
        for what in tune:
            chordal.tune(symb, getattr(chordal, "TUNE_" + what), 1 if what == "LEAFGRAM" else 0)
    return errs, box["counts"], kernels


def run_unit(unit):
    """the unit's own checks (they assert), with the launches of every context they make counted, those of its device_init included"""
    import ctypes
    import importlib
    import torch
    from smcp_amd import _lib
    from smcp_amd.symbolic import Symbolic
    from tests.helpers import census_read
    lib = _lib.lib()
    nk = int(lib.csp_profile_kinds())
    names = [lib.csp_profile_kernel_name(i).decode() for i in range(nk)]
    made = _UNIT_CONTEXTS           # the modules keep their contexts: a later unit of the process may run on one an earlier unit made
    plain = Symbolic.device_init

    def switch_on(s):
        lib.csp_profile_filter(s.handle, -1)
        lib.csp_profile_enable(s.handle, 1)
        lib.csp_profile_read(s.handle, None, None)

    def counted(self, *a, **k):
        lib.csp_census_enable(self.handle, 1)
        out = plain(self, *a, **k)
        if not any(s is self for s in made):
            made.append(self)
            switch_on(self)
        return out

    for s in made:
        switch_on(s)
        lib.csp_census_enable(s.handle, 1)
        census_read(s.handle)

    from smcp_amd import solvers
    counts, kernels = {}, {}
    Symbolic.device_init = counted
    peo = solvers.options.get("peo", "auto")
    solvers.options["peo"] = "mcs"                    # as tests/conftest.py pins it for every test
    try:
        for module, fn, args in _units()[unit]:
            getattr(importlib.import_module(module), fn)(*args)
        torch.cuda.synchronize()
    finally:
        solvers.options["peo"] = peo
        Symbolic.device_init = plain
        for s in made:
            ms, cnt = (ctypes.c_double * nk)(), (ctypes.c_int64 * nk)()
            lib.csp_profile_read(s.handle, ms, cnt)
            lib.csp_profile_enable(s.handle, 0)
            for i in range(nk):
                if cnt[i]:
                    counts[names[i]] = counts.get(names[i], 0) + int(cnt[i])
            for k, v in census_read(s.handle).items():
                kernels[k] = kernels.get(k, 0) + v
            lib.csp_census_enable(s.handle, 0)
    return {}, counts, kernels


def run_cases(cases, tune):
    """{case key: {errors, counts, seconds}}; stops at the first case that raises (its entry holds `failed`)"""
    out = {}
    for case_ in cases:
        t0 = time.perf_counter()
        try:
            errs, counts, kernels = run_unit(case_[1]) if case_[0] == "unit" else run_measured(case_, tune)
            out[case_key(case_)] = {"errors": errs, "counts": counts, "kernels": kernels, "seconds": time.perf_counter() - t0}
        except Exception:
            out[case_key(case_)] = {"errors": {}, "counts": {}, "kernels": {}, "seconds": time.perf_counter() - t0, "failed": traceback.format_exc()[-3000:]}
            break
    return out


def has_units(scn):
    return any(c[0] == "unit" for c in scn["cases"])


CHILD_SECONDS = 120       # overridden per scenario by the test module (ten times the measured time, at least 120 s)


def run_child(name, env, timeout, tmpdir):
    """one scenario in a fresh interpreter -> (results or None, return code or 'timeout', seconds, tail of its output)"""
    dst = os.path.join(tmpdir, name + ".json")
    full = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    full.update(env)
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name, dst], env=full, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
        rc, tail = r.returncode, r.stdout[-1500:] + r.stderr[-2500:]
    except subprocess.TimeoutExpired as e:
        rc, tail = "timeout", str(e)
    res = None
    if os.path.exists(dst):
        with open(dst) as f:
            res = json.load(f)
    return res, rc, time.perf_counter() - t0, tail


def collect(timeouts, tmpdir, log=lambda *a: None):
    """Every scenario, one after the other -> name -> {"run": results on the scenario's routes, "default": results of the same
    cases on the default routes (None for a default-routes scenario), "rc", "seconds", "tail", "skipped": reason or None}.
    Measured cases on the default routes run in this process, once per (case, tune); units always run in a child (their
    modules keep contexts of their own), the default-routes run of a unit is the one of the scenario `units`.  After a
    child that ended on a signal or on its timeout NO further child is started."""
    out, cache, stopped = {}, {}, None

    def default_run(scn):
        res = {}
        for case_ in scn["cases"]:
            key = case_key(case_)
            if case_[0] == "unit":
                if key in (out.get("units", {}).get("run") or {}):
                    res[key] = out["units"]["run"][key]
                continue
            ck = (key, tuple(sorted(scn["tune"].items())))
            if ck not in cache:
                cache[ck] = run_cases([case_], scn["tune"])[key]
            res[key] = cache[ck]
        return res

    for name in sorted(SCENARIOS, key=lambda n: (n != "units", n)):
        scn = SCENARIOS[name]
        rec = out[name] = dict(run=None, default=None, rc=0, seconds=0.0, tail="", skipped=None)
        if stopped:
            rec["skipped"] = "not run after %s ended abnormally" % stopped
            continue
        if not scn["env"] and not has_units(scn):
            t0 = time.perf_counter()
            rec["run"] = default_run(scn)
            rec["seconds"] = time.perf_counter() - t0
            if scn["tune"]:                                          # a tune alone: the same cases once more without it
                rec["default"] = default_run(dict(scn, tune={}))
        else:
            rec["run"], rec["rc"], rec["seconds"], rec["tail"] = run_child(name, scn["env"], timeouts.get(name, CHILD_SECONDS), tmpdir)
            if rec["rc"] == "timeout" or rec["rc"] < 0:
                stopped = name
                continue
            if scn["env"]:
                rec["default"] = default_run(scn)
        log(name, "rc", rec["rc"], "%.1f s" % rec["seconds"])
    return out


# ---- judging -----------------------------------------------------------------------------------------------------------
def union_counts(results, what="counts"):
    """what: "counts" (launches per kernel id) or "kernels" (per kernel function: the census)"""
    tot = {}
    for r in results.values():
        for k, v in r.get(what, {}).items():
            tot[k] = tot.get(k, 0) + v
    return tot


def launched(counts, pattern):
    return sorted(k for k in counts if fnmatch.fnmatchcase(k, pattern))


def signature_faults(counts, ran, gone):
    """what of a signature does not hold on the launch counts: [] when every `ran` pattern has a launch and no `gone` one"""
    bad = ["%s did not run" % p for p in ran if not launched(counts, p)]
    bad += ["%s ran (%s)" % (p, ", ".join(launched(counts, p))) for p in gone if launched(counts, p)]
    return bad


def error_faults(results, cases, bound_of):
    """cases that failed, did not run, or exceed bound_of(case, operation)"""
    bad = []
    for case_ in cases:
        key = case_key(case_)
        r = results.get(key)
        if r is None:
            bad.append("%s: not run" % key)
        elif "failed" in r:
            bad.append("%s: %s" % (key, r["failed"]))
        else:
            for op, e in sorted(r["errors"].items()):
                b = bound_of(case_, op)
                if not e <= b:
                    bad.append("%s: %s %.2e > %.2e" % (key, op, e, b))
    return bad


def recipes_of(pattern):
    """the KKT inputs (m, density, seed) the ledger uses on a pattern, dense_ref's own first"""
    out = [(dense_ref.KKT_M, dense_ref.KKT_DENSITY, dense_ref.KKT_SEED)]
    for scn in SCENARIOS.values():
        for c in scn["cases"]:
            if c[0] == "case" and c[1] == pattern and "kkt" in c[2]:
                r = recipe_of(c[4])
                if r not in out:
                    out.append(r)
    return out


def hybrid_cases():
    """the hybrid cases of the scenarios in the form of dense_ref.HYBRID_CASES, once each: recipe key -> case"""
    out = {}
    for scn in SCENARIOS.values():
        for c in scn["cases"]:
            if c[0] == "case" and c[4].get("mix"):
                k = c[4]
                hc = dense_ref.hybrid_case(c[1], k["m"], k["density"], k["seed"], k["mix"], k["tnzcols"], max_rhs=k["max_rhs"])
                out[dense_ref.recipe_key(c[1], hc["recipe"])] = hc
    return out


def oracle_errors(pattern):
    """operation -> worst error of the CPU oracle against the dense definitions on a pattern of the ledger (host only)"""
    from oracle import oracle as orc
    from smcp_amd.symbolic import Symbolic
    pat = LEDGER_PATTERNS[pattern]()
    case = dense_ref.DenseCase(pat, orc.Sym(Symbolic(pat)), dense_ref.YARDSTICK_SEED)
    worst = {}
    for i, recipe in enumerate(recipes_of(pattern)):
        case.kkt_recipe, case._kkt = recipe, None
        errs = dense_ref.measure(case, dense_ref.oracle_ops(case)) if i == 0 else dense_ref.kkt_errors(case, dense_ref.oracle_ops(case).kkt)
        for op, e in errs.items():
            worst[op] = max(worst.get(op, 0.0), float(e))
    return worst


def load_ledger_yardstick():
    with open(YARDSTICK_FILE) as f:
        return json.load(f)


def bound_of(case, op, yard=None, own=None, mixed=None):
    """dense_ref.device_bound(op); for a NEW pattern whose recorded oracle-vs-dense error is beyond the yardstick of
    GPU_PATTERNS, 100 x its own recorded value (over every recipe the ledger uses on it, the mixed ones included); for a mixed
    recipe on a pattern of GPU_PATTERNS the same rule on the record of that recipe (dense_ref.hybrid_bound); never looser
    than dense_ref.BOUND_CAP.  case: a case of a scenario, or a pattern name"""
    yard = dense_ref.load_yardstick() if yard is None else yard
    pattern = case if isinstance(case, str) else case[1]
    b = dense_ref.device_bound(op, yard)
    if not isinstance(case, str) and case[0] == "case" and case[4].get("mix") and pattern not in NEW_PATTERNS and op.startswith("kkt_"):
        return dense_ref.hybrid_bound(dense_ref.recipe_key(pattern, recipe_of(case[4])), op, yard, mixed)
    if pattern in NEW_PATTERNS:
        own = load_ledger_yardstick() if own is None else own
        v = float(own[pattern].get(op, 0.0))
        if v > float(yard[op]["value"]):
            b = min(100.0 * v, dense_ref.BOUND_CAP)
    return b


if __name__ == "__main__":      # the child interpreter: every case of one scenario -> json
    scn_ = SCENARIOS[sys.argv[1]]
    res_ = run_cases(scn_["cases"], scn_["tune"])
    with open(sys.argv[2], "w") as f_:
        json.dump(res_, f_)
    sys.exit(1 if any("failed" in r_ for r_ in res_.values()) else 0)
