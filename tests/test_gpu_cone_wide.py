"""chordal.cone_project and csp_cone_project_steps with the wide cliques on the chip-wide block Jacobi (tune(symb,
TUNE_CEIG_WIDE, 65); csrc/front_ceigw.hip: k_ceigw_cone_form, k_ceigw_cone_split, k_ceigw_cone_finish) against the LAPACK
form of the restatement, against the route at 0 and against the contract of the tune.  Patterns and the restatement of the
wide clique step: tests/test_cone_wide_host.py; inputs, units and K: tests/test_cone_project_host.py; the device is held to
the bound of tests/test_gpu_cone_project.py.  The Symbolics are this file's own: the tune is per context."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import smcp_amd
from helpers import GPU_PATTERNS, PATTERNS, launch_census, launch_counts
from smcp_amd import chordal
from smcp_amd.symbolic import Symbolic
from test_clique_eigh_host import lower_slots, unpack
from test_cone_project_host import CONE_UNITS, GPU_FACTOR, K_BOUND, KINDS, PARAMS, cone_project_restatement, norm_V, unit_of
from test_cone_wide_host import WIDE, wide_input, wide_root
from test_gpu_clique_eig import on_device
from test_gpu_clique_wide import WIDE_ORDERS, dense_cliques
from test_gpu_cone_project import run_steps, start
from test_mrcompletion_host import clique_rows, dense_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-8
# band: the pattern without a clique of 65 rows (class_edges has cliques of 89 rows and more, so it is not that pattern)
PATS = {"wide_root70": lambda: wide_root(70), "wide_root97": lambda: wide_root(97), "fam_top": GPU_PATTERNS["fam_top"], "band": PATTERNS["band"],
        "wide_edges": lambda: dense_cliques(WIDE_ORDERS)}
_SYMB, _REF = {}, {}


@pytest.fixture(scope="module", autouse=True)
def leave_no_device_tensor_behind():
    yield
    for symb in _SYMB.values():
        symb._cache.pop("clique_mult", None)
        symb._cache.pop("cone_weights", None)


def device_symb(name, tuned=True):
    """a Symbolic of this file's own per (pattern, tuned or never tuned)"""
    if (name, tuned) not in _SYMB:
        symb = Symbolic(PATS[name]())
        symb.device_init(0, 1)
        if tuned:
            chordal.tune(symb, chordal.TUNE_CEIG_WIDE, WIDE)
        _SYMB[(name, tuned)] = symb
    return _SYMB[(name, tuned)]


def cone_input(symb, kind):
    """the input of tests/test_cone_project_host.py for a Symbolic of device_symb, kept per pattern name (wide_input says why)"""
    return wide_input(next(n for (n, tuned), s in _SYMB.items() if s is symb), symb, kind)


def n_wide(symb):
    return int((np.diff(symb.rowptr) >= WIDE).sum())


def three_steps(symb, blk, rho, relax, split=False):
    """(a, x, U, W, hist) after three iterations from the start, in one call or in 1 + 2"""
    a, x, U, W = start(symb, blk)
    hist = torch.zeros((3, 4), dtype=torch.float64, device="cuda")
    if split:
        run_steps(symb, a, x, U, W, rho, relax, 0, 1, hist)
        run_steps(symb, a, x, U, W, rho, relax, 1, 2, hist)
    else:
        run_steps(symb, a, x, U, W, rho, relax, 0, 3, hist)
    return a, x, U, W, hist


def same_bits(p, q):
    """x, U, W and hist of two runs of three_steps"""
    return all(torch.equal(s.blkval if hasattr(s, "blkval") else s, t.blkval if hasattr(t, "blkval") else t) for s, t in zip(p[1:], q[1:]))


def against_the_restatement(name, kind, rho, relax):
    """case 1 on one input: the worst error in units; asserts everything else"""
    symb = device_symb(name)
    blk = cone_input(symb, kind)
    bd = GPU_FACTOR * CONE_UNITS * unit_of(symb, max(1.0, norm_V(symb, blk)))
    key = (name, kind, rho, relax)
    if key not in _REF:
        _REF[key] = cone_project_restatement(symb, blk, rho=rho, relax=relax, steps=3, near=bd)
    ref = _REF[key]
    one = three_steps(symb, blk, rho, relax)
    assert chordal.clique_eig_wide(symb) == n_wide(symb) > 0, "%s %s: %d wide cliques taken, %d in the pattern" % (name, kind, chordal.clique_eig_wide(symb), n_wide(symb))
    assert same_bits(one, three_steps(symb, blk, rho, relax, split=True)), "%s %s: 1 + 2 steps are not the 3 of one call" % (name, kind)
    assert same_bits(one, three_steps(symb, blk, rho, relax)), "%s %s: two runs differ" % (name, kind)
    a, x, U, W, hist = one
    assert torch.equal(a.blkval.cpu(), torch.from_numpy(np.array(blk))), "%s %s: the input was written" % (name, kind)
    xh, Uh, Wh, hh = x.blkval.cpu().numpy(), U.cpu().numpy(), W.cpu().numpy(), hist.cpu().numpy()
    worst = max(np.abs(xh - ref["x"]).max(), np.abs(Uh - ref["U"]).max(), np.abs(Wh - ref["W"]).max()) / unit_of(symb, ref["scale"])
    tag = "%s %s rho %g relax %g" % (name, kind, rho, relax)
    assert (xh[~lower_slots(symb)] == 0).all(), "%s: %d unused slots of x are not zero" % (tag, int((xh[~lower_slots(symb)] != 0).sum()))
    for k, (Uk, Wk) in enumerate(zip(unpack(symb, Uh), unpack(symb, Wh))):     # mirrored on store
        assert np.array_equal(Uk, Uk.T) and np.array_equal(Wk, Wk.T), "%s: clique %d: |U - U^T| %.3e, |W - W^T| %.3e, bound 0" % (
            tag, k, np.abs(Uk - Uk.T).max(), np.abs(Wk - Wk.T).max())
    assert (np.abs(hh[:, 2] - ref["hist"][:, 2]) <= ref["near"]).all(), "%s: negative eigenvalues per iteration %s, restatement %s, allowed difference %s" % (
        tag, hh[:, 2].tolist(), ref["hist"][:, 2].tolist(), ref["near"].tolist())
    assert (hh[:, 3] == 0).all(), "%s: cliques that did not converge per iteration %s, bound 0" % (tag, hh[:, 3].tolist())
    if kind == "incone":
        assert not Uh.any() and (hh[:, 2] == 0).all(), "%s: max|U| %.3e, negative eigenvalues %s, bound 0" % (tag, np.abs(Uh).max(), hh[:, 2].tolist())
    return worst, hh


# ---- 1. three iterations against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wide_root70", "wide_root97", "fam_top", "wide_edges"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rho,relax", PARAMS)
def test_three_iterations_against_the_restatement(name, kind, rho, relax, capsys):
    worst, hh = against_the_restatement(name, kind, rho, relax)
    with capsys.disabled():
        print("\n%s %s rho %g relax %g: %.2f units, hist %s" % (name, kind, rho, relax, worst, hh[-1, :3].tolist()))
    assert worst <= GPU_FACTOR * CONE_UNITS, "%s %s rho %g relax %g: max error of x, U, W %.3f units, bound %.1f" % (name, kind, rho, relax, worst, GPU_FACTOR * CONE_UNITS)


# ---- 2. the contract of the tune -----------------------------------------------------------------------------------------------
def test_tune_off_and_on_again_on_one_context():
    symb, plain = device_symb("wide_root97"), device_symb("wide_root97", tuned=False)
    blk = cone_input(symb, "noisy")
    try:
        first = three_steps(symb, blk, 1.0, 1.7)
        assert chordal.clique_eig_wide(symb) == 1, "wide cliques taken %d, wanted 1" % chordal.clique_eig_wide(symb)
        chordal.tune(symb, chordal.TUNE_CEIG_WIDE, 0)
        off = three_steps(symb, blk, 1.0, 1.7)
        assert chordal.clique_eig_wide(symb) == 0, "wide cliques taken %d, wanted 0" % chordal.clique_eig_wide(symb)
        assert same_bits(off, three_steps(plain, cone_input(plain, "noisy"), 1.0, 1.7)), "tune off: not the bits of a context never tuned"        # the bits of a context never tuned
        assert chordal.clique_eig_wide(plain) == 0, "wide cliques taken on the plain context %d, wanted 0" % chordal.clique_eig_wide(plain)
    finally:
        chordal.tune(symb, chordal.TUNE_CEIG_WIDE, WIDE)
    assert same_bits(first, three_steps(symb, blk, 1.0, 1.7)), "tune on again: not the bits of the first tuned run"                # the bits of the first tuned run
    assert chordal.clique_eig_wide(symb) == 1, "wide cliques taken %d, wanted 1" % chordal.clique_eig_wide(symb)
    assert not same_bits(first, off), "the routes at 65 and at 0 gave the same bits"                                         # the two routes do differ


def test_no_wide_clique_gives_the_untuned_bits():
    symb, plain = device_symb("band"), device_symb("band", tuned=False)
    assert n_wide(symb) == 0, "band has %d wide cliques, wanted 0" % n_wide(symb)
    for kind in ("noisy", "indef"):
        assert same_bits(three_steps(symb, cone_input(symb, kind), 1.0, 1.7), three_steps(plain, cone_input(plain, kind), 1.0, 1.7)), "%s: tuned and plain context differ without a wide clique" % kind
        assert chordal.clique_eig_wide(symb) == 0, "%s: wide cliques taken %d, wanted 0" % (kind, chordal.clique_eig_wide(symb))
    X, info = chordal.cone_project(on_device(symb, cone_input(symb, "noisy")), return_info=True)
    Xp, infop = chordal.cone_project(on_device(plain, cone_input(plain, "noisy")), return_info=True)
    assert torch.equal(X.blkval, Xp.blkval) and torch.equal(info["hist"], infop["hist"]) and info["wide"] == infop["wide"] == 0, "whole call: X or hist differ, wide %s / %s, wanted 0" % (info["wide"], infop["wide"])


def test_wide_count_is_reported():
    symb = device_symb("fam_top")
    X, info = chordal.cone_project(on_device(symb, cone_input(symb, "noisy")), maxit=2, return_info=True)
    assert chordal.clique_eig_wide(symb) == 3 and info["wide"] == 3, "wide cliques %d (query) / %d (info), wanted 3" % (chordal.clique_eig_wide(symb), info["wide"])
    assert 1 <= info["sweeps"] <= 30, "sweeps %d, bounds 1 and 30" % info["sweeps"]


# ---- 3. no data-dependent host loop ----------------------------------------------------------------------------------------------
def test_launch_chain_does_not_depend_on_the_data():
    symb = device_symb("wide_root97")
    counts = {}
    for kind in ("incone", "indef"):
        a, x, U, W = start(symb, cone_input(symb, kind))
        hist = torch.zeros((4, 4), dtype=torch.float64, device="cuda")
        run_steps(symb, a, x, U, W, 1.0, 1.7, 0, 1, hist)                     # warm: the lists of this tune
        counts[kind, 1] = launch_counts(symb, lambda: run_steps(symb, a, x, U, W, 1.0, 1.7, 1, 1, hist))
        counts[kind, 2] = launch_counts(symb, lambda: run_steps(symb, a, x, U, W, 1.0, 1.7, 2, 2, hist))
    assert counts["incone", 1] == counts["indef", 1] and counts["incone", 2] == counts["indef", 2], counts
    assert counts["indef", 2] == {k: 2 * v for k, v in counts["indef", 1].items()}, counts
    assert set(counts["indef", 1]) == {"k_ceig_reduce", "k_axpby", "k_ceig", "k_gather_level"}, counts["indef", 1]
    # 97 rows: 4 blocks, 3 steps of (pivot, apply) per block sweep; 30 block sweeps, each behind a check, and one check more,
    # then k_cone_resid; under k_ceig: form and begin, the steps, sort, split and finish, and ONE launch of k_cone_split: the
    # two leaves (16 and 18 rows) share the smallest LDS class
    assert counts["indef", 1]["k_ceig_reduce"] == 31 + 1, counts["indef", 1]
    assert counts["indef", 1]["k_ceig"] == 2 + 30 * 6 + 3 + 1, counts["indef", 1]
    assert counts["indef", 1]["k_axpby"] == 1, counts["indef", 1]
    # the kernels behind the ids, one iteration: the chain of cone_wide_pass for the one wide clique, k_cone_split for the leaves
    a, x, U, W = start(symb, cone_input(symb, "indef"))
    _, census = launch_census(symb, lambda: run_steps(symb, a, x, U, W, 1.0, 1.7, 0, 1, hist))
    chain = {"k_ceigw_cone_form": 1, "k_ceigw_begin": 1, "k_ceigw_check": 31, "k_ceigw_pivot": 90, "k_ceigw_apply": 90, "k_ceigw_sort": 1,
             "k_ceigw_cone_split": 1, "k_ceigw_cone_finish": 1, "k_cone_split": 1, "k_cone_update": 1, "k_cone_resid": 1}
    assert {k: census.get(k, 0) for k in chain} == chain, census
    assert set(census) - set(chain) <= {"k_clique_scatter", "k_gather_level"} and census["k_clique_scatter"] == symb.nlev, census


# ---- 4. the whole call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wide_root97", "fam_top"])
def test_whole_call_against_the_route_at_zero(name, capsys):
    symb, plain = device_symb(name), device_symb(name, tuned=False)
    blk = np.array(cone_input(symb, "noisy"))
    s = max(1.0, norm_V(symb, blk))
    A = on_device(symb, blk)
    X, info = chordal.cone_project(A, tol=TOL, return_info=True)
    X0, info0 = chordal.cone_project(on_device(plain, blk), tol=TOL, return_info=True)
    xh = X.blkval.cpu().numpy()
    diff = norm_V(symb, xh - X0.blkval.cpu().numpy())
    Xd = dense_of(symb, xh)
    lam = min(np.linalg.eigvalsh(Xd[np.ix_(clique_rows(symb, k), clique_rows(symb, k))])[0] for k in range(symb.Nsn))
    X2, info2 = chordal.cone_project(A, tol=TOL, U0=info["U"], return_info=True)
    with capsys.disabled():
        print("\n%s: %d iterations (at 0: %d; warm: %d), primal %.1e dual %.1e, %d wide cliques, %d sweeps at most; |X - X_0| %.2e = %.2f "
              "tol max(1, |A|); min lambda_min %.1e" % (name, info["iterations"], info0["iterations"], info2["iterations"], info["primal"],
                                                         info["dual"], info["wide"], info["sweeps"], diff, diff / (TOL * s), lam))
    assert info["converged"] and max(info["primal"], info["dual"]) <= TOL and info["wide"] == n_wide(symb) > 0, "%s: converged %s, primal %.3e dual %.3e (bound %.1e), wide %d of %d" % (name, info["converged"], info["primal"], info["dual"], TOL, info["wide"], n_wide(symb))
    assert info0["converged"] and info0["wide"] == 0, "%s at 0: converged %s, wide %d (wanted 0)" % (name, info0["converged"], info0["wide"])
    # each side is within K_BOUND tol scale of the converged projection
    assert diff <= 2 * K_BOUND * TOL * s, "%s: |X - X_0| %.3e, bound %.3e" % (name, diff, 2 * K_BOUND * TOL * s)
    assert lam >= -info["primal"] * s, "%s: min lambda_min %.3e, bound %.3e" % (name, lam, -info["primal"] * s)
    assert info2["converged"] and info2["iterations"] <= info["iterations"], "%s warm start: converged %s, %d iterations, bound %d" % (name, info2["converged"], info2["iterations"], info["iterations"])


# ---- 5. the scipy form -------------------------------------------------------------------------------------------------------------
def test_scipy_form_takes_the_tune():
    symb = device_symb("wide_root70")
    A = sp.csc_matrix(np.tril(dense_of(symb, np.array(cone_input(symb, "noisy")))))
    X, info = smcp_amd.cone_project(A, wide=WIDE, return_info=True)
    assert info["converged"] and info["wide"] > 0, "scipy form: converged %s, wide %d (wanted > 0)" % (info["converged"], info["wide"])
    X0, info0 = smcp_amd.cone_project(A, wide=0, return_info=True)
    Xn, infon = smcp_amd.cone_project(A, return_info=True)
    assert info0["wide"] == infon["wide"] == 0 and info0["iterations"] == infon["iterations"], "scipy form: wide %d / %d (wanted 0), iterations %d / %d" % (info0["wide"], infon["wide"], info0["iterations"], infon["iterations"])
    assert np.array_equal(X0.toarray(), Xn.toarray()), "scipy form: wide=0 differs from the call without the argument by %.3e, bound 0" % np.abs(X0.toarray() - Xn.toarray()).max()                        # 0: the bits of the call without the argument
    bd = 2 * K_BOUND * TOL * max(1.0, norm_V(symb, cone_input(symb, "noisy")))
    assert np.abs(X.toarray() - X0.toarray()).max() <= bd, "scipy form: |X - X_0| %.3e, bound %.3e" % (np.abs(X.toarray() - X0.toarray()).max(), bd)
    for bad in (10, 1, 64, -1):
        with pytest.raises(ValueError):
            smcp_amd.cone_project(A, wide=bad)


# ---- 6. non-finite input -----------------------------------------------------------------------------------------------------------
def test_non_finite_entry_names_the_wide_clique_at_the_first_look():
    symb = device_symb("wide_root70")
    kr = int(np.flatnonzero(np.diff(symb.rowptr) == 70)[0])
    bad = np.array(cone_input(symb, "noisy"))
    bad[symb.blkptr[kr] + 50 + 40 * 70] = np.nan                              # row 50, column 40 of the root: in no separator
    with pytest.raises(RuntimeError, match="did not converge") as e:
        chordal.cone_project(on_device(symb, bad))
    assert int(str(e.value).split("clique ")[1].split()[0]) == kr and "at iteration 1 " in str(e.value), (str(e.value), kr)
    X, info = chordal.cone_project(on_device(symb, cone_input(symb, "noisy")), return_info=True)
    assert info["converged"] and info["wide"] == 1, "after the NaN: converged %s, wide %d (wanted 1)" % (info["converged"], info["wide"])                           # nothing is left behind for the next call


# ---- 7. poison run -----------------------------------------------------------------------------------------------------------------
POISON_CASES = [("wide_root70", kind) for kind in KINDS] + [("wide_root97", "noisy")]


def poison_line(name, kind, fresh):
    """case 1 on one input, as a line; fresh: on a context made for it, so that its first call finds every buffer as allocated"""
    if fresh:
        _SYMB.pop((name, True), None)
    worst, hh = against_the_restatement(name, kind, *PARAMS[0])
    assert worst <= GPU_FACTOR * CONE_UNITS, "poisoned %s %s: %.3f units, bound %.1f" % (name, kind, worst, GPU_FACTOR * CONE_UNITS)
    return "poisoned workspace %s %s: %.2f units" % (name, kind, worst)


def poisoned_workspace_run():
    for name, kind in POISON_CASES:
        print(poison_line(name, kind, True))


def test_never_written_workspace_is_not_read():
    """SMCP_POISON=1 fills every fp64 buffer with 4.5e150 when it is allocated (the switch is cached per process: a fresh
    child interpreter), the integer words of the wide workspace with it (they lie in a buffer of doubles and read as raised
    flags and huge indices).  Every case runs on a context of its own, so that its first call meets the poison: wide_root70
    (three blocks, a block that meets the phantom player, a last block of 6 rows) with the three kinds, wide_root97 (a last
    block of one row).  The child must print the ratios of this process to two digits."""
    want = [poison_line(name, kind, False) for name, kind in POISON_CASES]
    env = dict(os.environ, SMCP_POISON="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for line in want:
        assert line in r.stdout, (line, r.stdout[-2000:])


if __name__ == "__main__":
    poisoned_workspace_run()
