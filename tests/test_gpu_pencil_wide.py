"""The pencil form on the chip-wide block Jacobi (tune(symb, TUNE_CEIG_WIDE, order) with B given: clique_eigvalsh(A, B),
clique_extremes(A, B), max_step(X, D); csrc/front_ceigw.hip) on the device: against LAPACK on dense clique
blocks, against the route at 0 for what it reports, and against the contract of the route.  Every case runs under
tune(symb, TUNE_CEIG_WIDE, 65).  Bound of an eigenvalue: 16 nf eps max|w_ref| (`bound` of tests/test_gpu_clique_eig.py) with
B = I + G G^T / 8 of condition number <= 40; of max_step: `pencil_bound` there.  Every assertion carries the clique, the ratio
and the bound."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import launch_census
from smcp_amd import _lib, chordal
from smcp_amd.symbolic import Symbolic
from test_clique_eig_host import EPS, clique_blocks, clique_spectra_ref, inputs, max_step_ref, pencil_B_on_V
from test_gpu_clique_eig import bound, on_device, pencil_bound
from test_gpu_clique_wide import PATS, WIDE, device_symb, n_wide
from test_mrcompletion_host import blkval_of, clique_rows, dense_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CW_B, CW_T, CW_STATE = 32, 64, 8                         # csrc/front_ceigw.hip
NAMES = ["wide_edges", "fam_top", "class_edges"]
_CASE = {}


def case(name):
    """(symb, blkA, blkB, reference spectra of the pencils): made once, never changed"""
    if name not in _CASE:
        symb = device_symb(name)
        _, blkA, blkB = inputs(symb, 11)[3]
        _CASE[name] = (symb, blkA, blkB, clique_spectra_ref(symb, blkA, blkB))
    return _CASE[name]


def orders(symb):
    return np.diff(np.asarray(symb.rowptr))


def clique_of_order(symb, nf):
    return int(np.flatnonzero(orders(symb) == nf)[0])


def tuned(symb, fn, value=WIDE):
    chordal.tune(symb, chordal.TUNE_CEIG_WIDE, value)
    try:
        return fn()
    finally:
        chordal.tune(symb, chordal.TUNE_CEIG_WIDE, 0)


def parity(name, symb, w, ref):
    """the worst |w - w_ref| over the cliques in units of bound(ref), every clique asserted"""
    wh = w.cpu().numpy()
    worst = 0.0
    for k in range(symb.Nsn):
        wk = wh[symb.rowptr[k]:symb.rowptr[k + 1]]
        nf = len(wk)
        assert (np.diff(wk) >= 0).all(), "%s clique %d (%d rows): w is not ascending, smallest step %.3e" % (name, k, nf, np.diff(wk).min())
        ratio = np.abs(wk - ref[k]).max() / bound(ref[k])
        assert ratio <= 1.0, "%s clique %d (%d rows): |w - w_ref| = %.3f of 16 nf eps max|w_ref| = %.3e, bound 1" % (name, k, nf, ratio, bound(ref[k]))
        worst = max(worst, ratio)
    return worst


def ext_of(symb, w):
    wh = w.cpu().numpy()
    lo = np.array([wh[symb.rowptr[k]] for k in range(symb.Nsn)])
    hi = np.array([wh[symb.rowptr[k + 1] - 1] for k in range(symb.Nsn)])
    return [lo.min(), float(np.argmin(lo)), hi.max(), float(np.argmax(hi))]


def named_clique(exc):
    return int(re.search(r"\(clique (\d+)\)", str(exc)).group(1))


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
def parity_run(name):
    symb, blkA, blkB, ref = case(name)
    A, B = on_device(symb, blkA), on_device(symb, blkB)

    def run():
        w = chordal.clique_eigvalsh(A, B)
        wide, groups, sweeps = chordal.clique_eig_wide(symb), chordal.clique_eig_groups(symb), chordal.clique_eig_sweeps(symb)
        ext = chordal.clique_extremes(A, B)
        return w, ext, wide, groups, sweeps

    w, ext, wide, groups, sweeps = tuned(symb, run)
    assert torch.equal(A.blkval.cpu(), torch.from_numpy(blkA)) and torch.equal(B.blkval.cpu(), torch.from_numpy(blkB)), "%s: an input was written" % name
    worst = parity(name, symb, w, ref)
    assert ext.cpu().numpy().tolist() == ext_of(symb, w), "%s: clique_extremes %s, from w %s" % (name, ext.cpu().numpy().tolist(), ext_of(symb, w))
    assert sweeps <= 30, "%s: %d sweeps, bound 30" % (name, sweeps)
    return worst, wide, groups, sweeps


@pytest.mark.parametrize("name", NAMES)
def test_parity_and_route_taken(name, capsys):
    symb = device_symb(name)
    worst, wide, groups, sweeps = parity_run(name)
    with capsys.disabled():
        print("\n%s pencil: worst |w - w_ref| = %.3f of 16 nf eps max|w_ref|, %d sweeps at most, %d wide cliques in %d group(s)"
              % (name, worst, sweeps, wide, groups))
    assert wide == n_wide(symb) > 0, "%s: wide cliques taken by the pencil call %d, in the pattern %d" % (name, wide, n_wide(symb))
    assert groups == 1, "%s: %d launch groups, wanted 1" % (name, groups)


# ---- 2. the opt-in contract --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wide_edges", "fam_top"])
def test_opt_in_contract(name):
    symb, blkA, blkB, ref = case(name)
    fresh = Symbolic(PATS[name]())                                           # a context never tuned
    fresh.device_init(0, 1)
    w_never = chordal.clique_eigvalsh(on_device(fresh, blkA), on_device(fresh, blkB))
    e_never = chordal.clique_extremes(on_device(fresh, blkA), on_device(fresh, blkB))
    assert chordal.clique_eig_wide(fresh) == 0 and chordal.clique_eig_groups(fresh) == 0
    A, B = on_device(symb, blkA), on_device(symb, blkB)
    w1 = tuned(symb, lambda: chordal.clique_eigvalsh(A, B))
    w2 = tuned(symb, lambda: chordal.clique_eigvalsh(A, B))
    assert torch.equal(w1, w2), "%s: two tuned runs differ by %.3e, bound 0" % (name, float((w1 - w2).abs().max()))
    w0 = chordal.clique_eigvalsh(A, B)                                       # 65 -> 0
    assert chordal.clique_eig_wide(symb) == 0 and chordal.clique_eig_groups(symb) == 0, "%s: wide cliques %d, groups %d after the tune went back to 0" % (
        name, chordal.clique_eig_wide(symb), chordal.clique_eig_groups(symb))
    assert torch.equal(w0, w_never), "%s: 65 -> 0 differs from a context never tuned by %.3e, bound 0" % (name, float((w0 - w_never).abs().max()))
    assert torch.equal(chordal.clique_extremes(A, B), e_never), "%s: clique_extremes after 65 -> 0 differs from a context never tuned" % name
    a, b = w1.cpu().numpy(), w_never.cpu().numpy()
    for k, nf in enumerate(orders(symb)):
        if nf < WIDE:
            sl = slice(int(symb.rowptr[k]), int(symb.rowptr[k + 1]))
            assert np.array_equal(a[sl], b[sl]), "%s clique %d (%d rows, narrow): differs under the tune by %.3e, bound 0" % (name, k, nf, np.abs(a[sl] - b[sl]).max())


# ---- 3. max_step -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wide_edges", "fam_top"])
def test_max_step_along_minus_x(name, capsys):
    """X = I + G G^T / 8 (pencil_B_on_V): R^-1 X R^-T differs from I by nf eps cond(X_gg), and the bound carries no condition
    number, so X is the well conditioned matrix of the parity cases (cond <= 40); the dense triangular factor of pd_on_V has a
    condition number that grows exponentially with the order of a dense clique and is not used at these orders"""
    symb = device_symb(name)
    blkX = pencil_B_on_V(symb, 5)
    X = on_device(symb, blkX)
    at_0 = chordal.max_step(X, on_device(symb, -blkX))
    alpha, inf = tuned(symb, lambda: (chordal.max_step(X, on_device(symb, -blkX)), chordal.max_step(X, X)))
    with capsys.disabled():
        print("\n%s: |max_step(X, -X) - 1| = %.2f nf_max eps (the route at 0: %.2f), cond(X_gg) <= %.1f"
              % (name, abs(alpha - 1.0) / (symb.max_front * EPS), abs(at_0 - 1.0) / (symb.max_front * EPS), max(np.linalg.cond(F) for F in clique_blocks(symb, blkX))))
    assert inf == math.inf
    assert abs(alpha - 1.0) <= 16 * symb.max_front * EPS, "%s: |max_step(X, -X) - 1| = %.2f nf_max eps, bound 16" % (name, abs(alpha - 1.0) / (symb.max_front * EPS))


@pytest.mark.parametrize("name,scaled,binds", [("wide_edges", 129, "wide"), ("wide_edges", 64, "narrow"), ("fam_top", None, None)])
def test_max_step_names_the_binding_clique(name, scaled, binds, capsys):
    """wide_edges: the cliques are disjoint, so D scaled by 10 on one of them makes that one bind"""
    symb = device_symb(name)
    blkX = pencil_B_on_V(symb, 5)                                            # (well conditioned at every order: see above)
    blkD = np.random.default_rng(6).standard_normal(symb.blklen)
    if scaled is not None:
        ks = clique_of_order(symb, scaled)
        blkD[symb.blkptr[ks]:symb.blkptr[ks + 1]] *= 10.0
    a_ref, k_ref = max_step_ref(symb, blkX, blkD)
    if binds is not None:
        assert k_ref == ks and (orders(symb)[k_ref] >= WIDE) == (binds == "wide")         # (of the input, not of the result)
    X, D = on_device(symb, blkX), on_device(symb, blkD)
    (alpha, k), wide = tuned(symb, lambda: (chordal.max_step(X, D, return_clique=True), chordal.clique_eig_wide(symb)))
    assert wide == n_wide(symb), "%s: wide cliques taken by max_step %d, in the pattern %d" % (name, wide, n_wide(symb))
    tol = pencil_bound(symb, blkD, blkX)                                     # of mu = -1 / alpha, the pencil eigenvalue
    lo_ref = [r[0] for r in clique_spectra_ref(symb, blkD, blkX)]
    with capsys.disabled():
        print("\n%s (D x 10 on order %s): alpha %.6f, clique %d (%d rows), |mu - mu_ref| = %.3f of the bound %.3e"
              % (name, scaled, alpha, k, orders(symb)[k], abs(-1.0 / alpha + 1.0 / a_ref) / tol, tol))
    assert 0 < alpha < math.inf and abs(-1.0 / alpha + 1.0 / a_ref) <= tol, "%s clique %d: |mu - mu_ref| = %.3e = %.3f of the bound %.3e" % (
        name, k, abs(-1.0 / alpha + 1.0 / a_ref), abs(-1.0 / alpha + 1.0 / a_ref) / tol, tol)
    assert abs(lo_ref[k] + 1.0 / alpha) <= tol, "%s: the clique named, %d, has mu_ref %.6e, the step's mu %.6e: apart %.3f of the bound %.3e" % (
        name, k, lo_ref[k], -1.0 / alpha, abs(lo_ref[k] + 1.0 / alpha) / tol, tol)
    if binds is not None:
        assert k == k_ref, "%s: clique %d named, %d binds" % (name, k, k_ref)
    lam = np.linalg.eigvalsh(clique_blocks(symb, blkX + alpha * blkD)[k])    # the binding clique's block is singular at alpha
    assert abs(lam[0]) <= 1e-6 * np.abs(lam).max(), "%s clique %d: lambda_min(X + alpha D) = %.3e, bound %.3e" % (name, k, lam[0], 1e-6 * np.abs(lam).max())


def test_scipy_form_takes_the_route(monkeypatch):
    """smcp_amd.max_step(X, D, wide=65) on a dense pattern of order 97: one clique, on the route; against LAPACK on the dense pencil"""
    import scipy.linalg
    import scipy.sparse as sp
    import smcp_amd
    rng = np.random.default_rng(31)
    G = rng.standard_normal((97, 4))
    Xd = np.eye(97) + G @ G.T / 8.0
    S = rng.standard_normal((97, 97))
    Dd = S + S.T
    ref = scipy.linalg.eigh(Dd, Xd, eigvals_only=True)
    inner, taken = chordal.max_step, []

    def recording(X, D, return_clique=False):
        out = inner(X, D, return_clique)
        taken.append(chordal.clique_eig_wide(X.symb))
        return out

    monkeypatch.setattr(chordal, "max_step", recording)
    a65 = smcp_amd.max_step(sp.csc_matrix(np.tril(Xd)), sp.csc_matrix(np.tril(Dd)), wide=65)
    a0 = smcp_amd.max_step(sp.csc_matrix(np.tril(Xd)), sp.csc_matrix(np.tril(Dd)))
    assert taken == [1, 0], "cliques on the route under wide=65 and wide=0: %s, wanted [1, 0]" % taken
    for what, alpha in (("wide=65", a65), ("wide=0", a0)):
        assert abs(-1.0 / alpha - ref[0]) <= bound(ref), "%s: |mu - mu_ref| = %.3f of 16 nf eps max|w_ref|, bound 1" % (what, abs(-1.0 / alpha - ref[0]) / bound(ref))


# ---- 4. a B that is not positive definite --------------------------------------------------------------------------------
def with_negative_diagonal(symb, blkB, at):
    """blkB with B[r, r] = -1 for the local row r of clique k, for every (k, r) of `at`"""
    Bd = dense_of(symb, blkB)
    for k, r in at:
        i = clique_rows(symb, k)[r]
        Bd[i, i] = -1.0
    return blkval_of(symb, Bd)


def raised_by(fn):
    try:
        fn()
    except Exception as e:                                                    # noqa: BLE001 (the type is what is compared)
        return e
    return None


@pytest.mark.parametrize("name,at", [("129", [(129, 70)]), ("wide_edges", [(64, 3), (129, 70)]), ("wide_edges", [(161, 130)])])
def test_b_not_positive_definite_names_the_clique_of_the_route_at_0(name, at):
    """order 129, row 70: met by the second diagonal tile, after a trailing update.  wide_edges with a narrow and a wide
    clique failing: the lowest, the narrow one, is named.  Order 161, row 130: the third diagonal tile."""
    symb = device_symb(name)
    blkA = np.random.default_rng(21).standard_normal(symb.blklen)
    good = pencil_B_on_V(symb, 22)
    where = [(clique_of_order(symb, nf), r) for nf, r in at]
    bad = with_negative_diagonal(symb, good, where)
    A, Bb, Bg = on_device(symb, blkA), on_device(symb, bad), on_device(symb, good)
    lowest = min(k for k, _ in where)
    assert where[0][0] == lowest                                             # (of the input)
    e0 = raised_by(lambda: chordal.clique_eigvalsh(A, Bb))
    s0 = raised_by(lambda: chordal.max_step(Bb, A))

    def at_65():
        e = raised_by(lambda: chordal.clique_eigvalsh(A, Bb))
        wide = chordal.clique_eig_wide(symb)
        s = raised_by(lambda: chordal.max_step(Bb, A))
        w = chordal.clique_eigvalsh(A, Bg)                                   # the next call on the context is correct
        return e, wide, s, w

    e, wide, s, w = tuned(symb, at_65)
    assert wide == n_wide(symb)
    assert isinstance(e0, ArithmeticError) and type(e) is type(e0), "clique_eigvalsh: %r at 65, %r at 0" % (e, e0)
    assert named_clique(e) == named_clique(e0) == lowest, "clique_eigvalsh: clique %d named at 65, %d at 0, %d is the lowest that fails" % (
        named_clique(e), named_clique(e0), lowest)
    assert type(s) is type(s0) and named_clique(s) == named_clique(s0) == lowest, "max_step: %r at 65, %r at 0" % (s, s0)
    worst = parity(name, symb, w, clique_spectra_ref(symb, blkA, good))
    assert worst <= 1.0


# ---- 5. non-finite entries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B"])
def test_non_finite_entry_is_reported_as_at_0_and_stays_in_its_clique(which):
    symb, blkA, blkB, ref = case("wide_edges")
    kb = clique_of_order(symb, 97)
    badA, badB = blkA.copy(), blkB.copy()
    (badA if which == "A" else badB)[symb.blkptr[kb] + 70] = np.nan         # row 70, column 0 of that clique: its second tile
    A, B = on_device(symb, badA), on_device(symb, badB)
    e0 = raised_by(lambda: chordal.clique_eigvalsh(A, B))
    L = _lib.lib()

    def at_65():
        e = raised_by(lambda: chordal.clique_eigvalsh(A, B))
        w = torch.zeros(int(symb.rowptr[-1]), dtype=torch.float64, device="cuda")
        rc = L.csp_clique_eigvalsh(symb.handle, A.blkval.data_ptr(), B.blkval.data_ptr(), w.data_ptr(), None, None)
        torch.cuda.synchronize()
        return e, rc, w, chordal.clique_eigvalsh(on_device(symb, blkA), on_device(symb, blkB))

    e, rc, w, w_next = tuned(symb, at_65)
    assert e0 is not None and type(e) is type(e0) and str(e) == str(e0), "NaN in %s: %r at 65, %r at 0" % (which, e, e0)
    assert isinstance(e, RuntimeError if which == "A" else ArithmeticError) and (rc == -7 if which == "A" else rc == kb + 1), (which, e, rc)
    wh = w.cpu().numpy()
    for k in range(symb.Nsn):
        wk = wh[symb.rowptr[k]:symb.rowptr[k + 1]]
        if k == kb:
            assert np.isnan(wk).all(), "NaN in %s: clique %d (%d rows) is not NaN throughout" % (which, k, len(wk))
        else:
            ratio = np.abs(wk - ref[k]).max() / bound(ref[k])
            assert np.isfinite(wk).all() and ratio <= 1.0, "NaN in %s of clique %d: clique %d (%d rows) %.3f of 16 nf eps max|w_ref|, bound 1" % (
                which, kb, k, len(wk), ratio)
    assert parity("wide_edges after the NaN", symb, w_next, ref) <= 1.0      # nothing is left behind for the next call


# ---- 6. launch groups ------------------------------------------------------------------------------------------------------
def pencil_ws(nf):
    """ceigw_layout without V, with G (csrc/front_ceigw.hip): doubles of the workspace of one clique, from base 0"""
    nb = -(-nf // CW_B)
    h = (nb + 1) // 2
    o = 2 * nf * nf + h * CW_T * CW_T + h * CW_T + h * (h + 1) // 2 + nf + 2 + (2 * nf + h + CW_STATE + 1) // 2
    return (o + 31) // 32 * 32


def groups_of(symb, limit):
    """ceigw_pass restated: the wide cliques, ascending, in groups whose workspace stays within the limit (0: 2**25)"""
    out, doubles = [], 0
    for nf in (int(v) for v in orders(symb) if v >= WIDE):
        if not out or doubles + pencil_ws(nf) > (limit or 2 ** 25):
            out.append([])
            doubles = 0
        out[-1].append(nf)
        doubles += pencil_ws(nf)
    return len(out)


def test_two_and_three_launch_groups_give_the_bits_of_one():
    symb, blkA, blkB, ref = case("fam_top")
    assert (pencil_ws(130), pencil_ws(110)) == (46560, 32768)                # G moves them to what a workspace with V takes
    limits = [(0, 1), (80000, 2), (1, 3)]
    A, B = on_device(symb, blkA), on_device(symb, blkB)
    out = []

    def run():
        for limit, groups in limits:
            assert groups_of(symb, limit) == groups
            chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, limit)
            w = chordal.clique_eigvalsh(A, B)
            got = chordal.clique_eig_groups(symb)
            assert got == groups, "limit %d: %d launch groups, wanted %d" % (limit, got, groups)
            assert chordal.clique_eig_wide(symb) == n_wide(symb) == 3
            out.append((w, chordal.clique_extremes(A, B), chordal.max_step(B, A, return_clique=True)))

    try:
        tuned(symb, run)
    finally:
        chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, 0)
    assert parity("fam_top in one group", symb, out[0][0], ref) <= 1.0
    for (limit, groups), o in zip(limits[1:], out[1:]):
        assert torch.equal(o[0], out[0][0]), "w under %d groups differs from one group by %.3e, bound 0" % (groups, float((o[0] - out[0][0]).abs().max()))
        assert torch.equal(o[1], out[0][1]) and o[2] == out[0][2], "ext or max_step under %d groups differ from one group" % groups


# ---- 7. the launch chain -----------------------------------------------------------------------------------------------
def chain(symb, block_sweeps, narrow_launches):
    """(k_ceig_reduce, k_ceig) launches of one pencil call with its wide cliques in one group: a k_ceigw_check before each
    block sweep and one behind, k_ceig_reduce; k_ceig per LDS class of the narrow cliques, k_ceigw_form, the reduction
    (3 ntmax + 1: section 24), k_ceigw_begin, (pivot, apply) per step of every block sweep, k_ceigw_sort"""
    nfmax = int(orders(symb).max())
    nb, nt = -(-nfmax // CW_B), -(-nfmax // CW_T)
    steps = nb + (nb & 1) - 1
    return block_sweeps + 2, narrow_launches + 1 + (3 * nt + 1) + 1 + 2 * steps * block_sweeps + 1


def chain_kernels(symb, block_sweeps):
    """the same chain by kernel function (the launch census): what wide_pass of csrc/completions.hip launches for a pencil"""
    nfmax = int(orders(symb).max())
    nb, nt = -(-nfmax // CW_B), -(-nfmax // CW_T)
    steps = nb + (nb & 1) - 1
    return {"k_ceigw_form": 1, "k_ceigw_potrf": nt, "k_ceigw_panel": nt - 1, "k_ceigw_trail": nt - 1, "k_ceigw_solve<true>": 1,
            "k_ceigw_solve<false>": 1, "k_ceigw_symm": 1, "k_ceigw_begin": 1, "k_ceigw_check": block_sweeps + 1,
            "k_ceigw_pivot": steps * block_sweeps, "k_ceigw_apply": steps * block_sweeps, "k_ceigw_sort": 1, "k_ceig_reduce": 1,
            "k_ceigw_out": 0}


@pytest.mark.parametrize("name,narrow", [("129", 0), ("wide_edges", 1)])
def test_launch_chain_depends_on_the_pattern_and_the_block_sweeps_alone(name, narrow):
    symb = device_symb(name)
    blkB = pencil_B_on_V(symb, 22)
    blkS = np.random.default_rng(21).standard_normal(symb.blklen)
    bad = with_negative_diagonal(symb, blkB, [(clique_of_order(symb, 129), 70)])
    B = on_device(symb, blkB)

    def run():
        got = {}
        for kind, A, Bk in (("indefinite", on_device(symb, blkS), B), ("A = B", B, B), ("B not pd", on_device(symb, blkS), on_device(symb, bad))):
            call = lambda: raised_by(lambda: chordal.clique_eigvalsh(A, Bk))
            call()                                                           # buffers of the first call
            counts, census[kind] = launch_census(symb, call)
            got[kind] = (counts.get("k_ceig_reduce", 0), counts.get("k_ceig", 0), chordal.clique_eig_sweeps(symb))
        return got

    census = {}
    got = tuned(symb, run)
    for kind, (n_reduce, n_ceig, sweeps) in got.items():                        # the kernels behind the two ids, by name
        want = chain_kernels(symb, n_reduce - 2)
        assert {k: census[kind].get(k, 0) for k in want} == want, "%s %s: %s, chain %s" % (name, kind, census[kind], want)
        rest = {k: v for k, v in census[kind].items() if k not in want and k != "k_gather_level"}      # (the gathers of A and B: an id of their own)
        assert rest == ({"k_ceig": narrow} if narrow else {}), "%s %s: beside the chain %s" % (name, kind, rest)
    for kind, (n_reduce, n_ceig, sweeps) in got.items():
        block_sweeps = n_reduce - 2                                          # the checks read back, but for the last
        assert 0 <= block_sweeps <= 30
        if name == "129" and kind != "B not pd":
            assert block_sweeps == sweeps, "%s %s: %d checks for %d block sweeps" % (name, kind, n_reduce - 1, sweeps)
        assert (n_reduce, n_ceig) == chain(symb, block_sweeps, narrow), "%s %s: (k_ceig_reduce, k_ceig) launches %s, chain formula %s" % (
            name, kind, (n_reduce, n_ceig), chain(symb, block_sweeps, narrow))
    fixed = {kind: g[1] - (g[0] - 2) * (chain(symb, 1, narrow)[1] - chain(symb, 0, narrow)[1]) for kind, g in got.items()}
    assert len(set(fixed.values())) == 1, "%s: the launches outside the block sweeps differ with the data: %s" % (name, fixed)
    assert got["indefinite"][0] > 2 and got["A = B"][0] < got["indefinite"][0], got      # (a reduced matrix next to I takes fewer block sweeps)
    if name == "129":
        assert got["B not pd"][0] == 2, got                                  # the chain of a failed clique: no block sweep, and as many launches around them


# ---- 8. poison ---------------------------------------------------------------------------------------------------------
def poisoned_pencil_run():
    """the body of the child of test_never_written_workspace_is_not_read: the parity case of wide_edges and fam_top"""
    for name in ("wide_edges", "fam_top"):
        worst, wide, groups, sweeps = parity_run(name)
        print("poisoned pencil %s: %r %d %d %d" % (name, worst, wide, groups, sweeps))


def test_never_written_workspace_is_not_read():
    """SMCP_POISON=1 fills every fp64 buffer with 4.5e150 when it is allocated (the switch is cached per process: a fresh
    child interpreter): the ratios are those of this process, so no never-written word of G, of the ragged last tiles or of
    the new status word is read"""
    env = dict(os.environ, SMCP_POISON="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for name in ("wide_edges", "fam_top"):
        worst, wide, groups, sweeps = parity_run(name)
        line = "poisoned pencil %s: %r %d %d %d" % (name, worst, wide, groups, sweeps)
        assert line in r.stdout, "%s: here %s, the child printed %s" % (name, line, r.stdout[-600:])


if __name__ == "__main__":
    poisoned_pencil_run()
