"""Spectra of the clique blocks on the device (smcp_amd.chordal.clique_eigvalsh / clique_extremes / cone_margin / max_step and
their scipy forms in smcp_amd.base; csrc/front_ceig.hip) against LAPACK on dense clique blocks, against the library's own
cone test (chordal.completion) and against their contract.  References and input makers: tests/test_clique_eig_host.py."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from helpers import EXTRA, GPU_PATTERNS, PATTERNS, launch_counts
from smcp_amd import base, chordal, problems
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic
from test_clique_eig_host import (EPS, clique_blocks, clique_spectra_ref, indefinite_on_V, inputs, margin_ref, max_step_ref,
                                  pencil_B_on_V, shifted)
from test_mrcompletion_host import leaf_clique, low_rank_on_V, pd_on_V

pytestmark = pytest.mark.gpu

LDS_CLASSES = (8192, 16384, 32768, 65536, 131072)       # bytes: the size classes of mrc_launch (csrc/completions.hip)


def slot1(nf):
    return nf * nf + 3 * nf + 3                          # ceig_slot1, csrc/front_ceig.hip:34


def slot2(nf):
    return 2 * nf * nf + 3 * nf + 3                      # ceig_slot2, csrc/front_ceig.hip:35


def class_edges():
    """for every LDS class and both forms: the largest order whose slot fits the class and the smallest that does not"""
    orders = set()
    for slot in (slot1, slot2):
        for cap in LDS_CLASSES:
            nf = 1
            while slot(nf + 1) * 8 <= cap:
                nf += 1
            orders |= {nf, nf + 1}
    return sorted(orders)


def class_edge_pattern():
    """disjoint dense cliques of the orders of class_edges()"""
    cl, first = [], 0
    for nf in class_edges():
        own = np.arange(first, first + nf)
        cl.append((own, own))
        first += nf
    return problems._from_cliques(first, cl)


PATS = dict(PATTERNS)
PATS["diag"] = GPU_PATTERNS["diag"]
PATS["one_clique"] = EXTRA["one_clique"]
PATS["fam_odd"] = GPU_PATTERNS["fam_odd"]
PATS["fam_top"] = GPU_PATTERNS["fam_top"]
PATS["class_edges"] = class_edge_pattern
KINDS = ["definite", "rank3", "indefinite", "pencil"]

_SYMB, _CASE, WORST = {}, {}, {"ratio": 0.0, "sweeps": 0}


def device_symb(name):
    if name not in _SYMB:
        _SYMB[name] = Symbolic(PATS[name]())
        _SYMB[name].device_init(0, 1)
    return _SYMB[name]


def case(name, kind):
    """(symb, blkA, blkB, reference spectra) of a case: made once, never changed"""
    if (name, kind) not in _CASE:
        symb = device_symb(name)
        for knd, blkA, blkB in inputs(symb, 11):
            _CASE[(name, knd)] = (symb, blkA, blkB, clique_spectra_ref(symb, blkA, blkB))
    return _CASE[(name, kind)]


def on_device(symb, blk):
    return cspmatrix(symb, torch.from_numpy(blk.copy()).cuda())


def bound(ref):
    """the parity bound of one clique: 16 nf eps max|w_ref|"""
    return 16 * len(ref) * EPS * np.abs(ref).max()


def pencil_bound(symb, blkA, blkB):
    """the bound of a pencil eigenvalue when B is not well conditioned: the backward error nf eps |B_gg| of the Cholesky
    factor R and of the two solves reaches R^-1 A_gg R^-T magnified by cond(B_gg), so the parity bound of a clique times
    cond(B_gg), the largest over the cliques (the parity cases themselves use B of condition number <= 40 and no such factor)"""
    conds = [np.linalg.cond(B) for B in clique_blocks(symb, blkB)]
    return max(bound(r) * c for r, c in zip(clique_spectra_ref(symb, blkA, blkB), conds))


def test_class_edge_orders_cover_both_sides_of_every_class():
    orders = class_edges()
    for slot in (slot1, slot2):
        for cap in LDS_CLASSES:
            fit = max(nf for nf in orders if slot(nf) * 8 <= cap)
            assert slot(fit + 1) * 8 > cap and fit + 1 in orders
    assert max(orders) > 126 and 1 < min(orders) < 32


@pytest.mark.parametrize("name", sorted(PATS))
@pytest.mark.parametrize("kind", KINDS)
def test_parity_and_contract(name, kind, capsys):
    symb, blkA, blkB, ref = case(name, kind)
    A = on_device(symb, blkA)
    B = None if blkB is None else on_device(symb, blkB)
    w1 = chordal.clique_eigvalsh(A, B)
    sweeps = chordal.clique_eig_sweeps(symb)
    w2 = chordal.clique_eigvalsh(A, B)
    assert torch.equal(w1, w2)                                               # the same bits from call to call
    assert torch.equal(A.blkval.cpu(), torch.from_numpy(blkA))               # neither input is written
    assert B is None or torch.equal(B.blkval.cpu(), torch.from_numpy(blkB))
    assert w1.dtype == torch.float64 and w1.shape == (int(symb.rowptr[-1]),)
    w = w1.cpu().numpy()
    worst = 0.0
    for k in range(symb.Nsn):
        wk = w[symb.rowptr[k]:symb.rowptr[k + 1]]
        assert len(wk) == len(ref[k]) and (np.diff(wk) >= 0).all()           # ascending inside every clique
        scale = len(wk) * EPS * np.abs(ref[k]).max()
        if scale > 0:
            worst = max(worst, np.abs(wk - ref[k]).max() / scale)
        else:
            assert (wk == 0).all()
    WORST["ratio"] = max(WORST["ratio"], worst)
    WORST["sweeps"] = max(WORST["sweeps"], sweeps)
    with capsys.disabled():
        print("\n%s %s: worst |w - w_ref| = %.2f nf eps max|w_ref|, %d sweeps (so far: %.2f, %d)"
              % (name, kind, worst, sweeps, WORST["ratio"], WORST["sweeps"]))
    assert worst <= 16.0
    assert sweeps <= 15
    ext = chordal.clique_extremes(A, B).cpu().numpy()
    lo = np.array([w[symb.rowptr[k]] for k in range(symb.Nsn)])
    hi = np.array([w[symb.rowptr[k + 1] - 1] for k in range(symb.Nsn)])
    assert ext[0] == lo.min() and ext[1] == np.argmin(lo) and ext[2] == hi.max() and ext[3] == np.argmax(hi)


# ---- cone_margin -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_cone_margin_against_reference_and_completion(name):
    symb = device_symb(name)
    blk = pd_on_V(symb, 5)
    ref = clique_spectra_ref(symb, blk)
    m, k = chordal.cone_margin(on_device(symb, blk))
    m_ref, k_ref = margin_ref(symb, blk)
    assert abs(m - m_ref) <= max(bound(ref[k]), bound(ref[k_ref]))
    assert abs(ref[k][0] - m_ref) <= bound(ref[k]) + bound(ref[k_ref])      # the clique named attains the margin
    assert m > 0
    chordal.completion(on_device(symb, shifted(symb, blk, (1 - 1e-6) * m)))  # inside: the library's own cone test agrees
    with pytest.raises(ArithmeticError):
        chordal.completion(on_device(symb, shifted(symb, blk, (1 + 1e-6) * m)))


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_cone_margin_of_singular_blocks_is_zero(name):
    symb = device_symb(name)
    blk = low_rank_on_V(symb, 3, 2)
    ref = clique_spectra_ref(symb, blk)
    m, _ = chordal.cone_margin(on_device(symb, blk))
    tol = max(bound(r) for r in ref)
    assert abs(m - margin_ref(symb, blk)[0]) <= tol
    if min(len(r) for r in ref) > 3:                                         # every block is singular
        assert abs(m) <= tol


# ---- max_step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_max_step_against_completion(name):
    symb = device_symb(name)
    blkX, blkD = pd_on_V(symb, 5), indefinite_on_V(symb, 6)
    X, D = on_device(symb, blkX), on_device(symb, blkD)
    alpha, k = chordal.max_step(X, D, return_clique=True)
    assert alpha == chordal.max_step(X, D)
    a_ref, _ = max_step_ref(symb, blkX, blkD)
    tol = pencil_bound(symb, blkD, blkX)                                     # of mu = -1 / alpha, the pencil eigenvalue
    assert 0 < alpha < math.inf and abs(-1.0 / alpha + 1.0 / a_ref) <= tol
    chordal.completion(on_device(symb, blkX + (1 - 1e-6) * alpha * blkD))
    with pytest.raises(ArithmeticError):
        chordal.completion(on_device(symb, blkX + (1 + 1e-6) * alpha * blkD))
    lam = np.linalg.eigvalsh(clique_blocks(symb, blkX + alpha * blkD)[k])    # the binding clique's block is singular at alpha
    assert abs(lam[0]) <= 1e-6 * np.abs(lam).max()


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_max_step_along_plus_and_minus_x(name, capsys):
    symb = device_symb(name)
    blkX = pd_on_V(symb, 5)
    X = on_device(symb, blkX)
    assert chordal.max_step(X, X) == math.inf
    alpha = chordal.max_step(X, on_device(symb, -blkX))
    with capsys.disabled():
        print("\n%s: |max_step(X, -X) - 1| = %.2f nf_max eps" % (name, abs(alpha - 1.0) / (symb.max_front * EPS)))
    assert abs(alpha - 1.0) <= 16 * symb.max_front * EPS


# ---- errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["arrow", "nested", "rand2"])
def test_x_outside_the_cone_names_the_clique(name):
    symb = device_symb(name)
    blkX = pd_on_V(symb, 5)
    k = leaf_clique(symb)
    blkX[symb.blkptr[k]] *= -1.0                        # X_jj < 0 for the first column of clique k: only clique k holds it
    X, D = on_device(symb, blkX), on_device(symb, indefinite_on_V(symb, 6))
    with pytest.raises(ArithmeticError, match=r"\(clique %d\)" % k):
        chordal.max_step(X, D)
    with pytest.raises(ArithmeticError, match=r"\(clique %d\)" % k):
        chordal.clique_eigvalsh(D, X)


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_non_finite_entry_is_reported(value):
    symb = device_symb("nested")
    blk = pd_on_V(symb, 5)
    blk[symb.blkptr[leaf_clique(symb)] + 1] = value
    with pytest.raises(RuntimeError, match="did not converge"):
        chordal.clique_eigvalsh(on_device(symb, blk))
    chordal.clique_eigvalsh(on_device(symb, pd_on_V(symb, 5)))               # nothing is left behind for the next call


def test_mismatched_symbolics():
    s1 = device_symb("arrow")
    s2 = Symbolic(PATTERNS["arrow"]())
    s2.device_init(0, 1)
    X1, X2 = on_device(s1, pd_on_V(s1, 5)), on_device(s2, pd_on_V(s2, 5))
    for fn in (chordal.clique_eigvalsh, chordal.clique_extremes, chordal.max_step):
        with pytest.raises(ValueError):
            fn(X1, X2)


def test_overlapping_output_is_refused():
    from smcp_amd import _lib
    symb = device_symb("arrow")
    X = on_device(symb, pd_on_V(symb, 5))
    p = X.blkval.data_ptr()
    w = torch.empty(int(symb.rowptr[-1]), dtype=torch.float64, device="cuda")
    L = _lib.lib()
    assert L.csp_clique_eigvalsh(symb.handle, p, None, p + 8, None, None) == -1
    assert L.csp_clique_eigvalsh(symb.handle, p, None, w.data_ptr(), p + 8 * (symb.blklen - 1), None) == -1
    assert L.csp_clique_eigvalsh(symb.handle, None, None, w.data_ptr(), None, None) == -1
    assert L.csp_clique_eigvalsh(symb.handle, p, None, w.data_ptr(), None, None) == 0


def test_scipy_forms():
    """base.max_step refuses a pattern that is not chordal; base.cone_margin / base.max_step on a scrambled vertex order
    (upper triangle given) return what the chordal-order call returns"""
    cyc = sp.coo_matrix((np.ones(4), ([1, 2, 3, 3], [0, 1, 2, 0])), shape=(4, 4)) + 4.0 * sp.identity(4)
    with pytest.raises(ValueError):
        base.max_step(cyc, cyc)
    with pytest.raises(ValueError):
        base.cone_margin(cyc)
    sp0 = Symbolic(problems.random_chordal_pattern(20, max_nn=5, max_na=7, seed=9))
    n = sp0.n
    cp, ri = sp0.sparsity_pattern()                 # chordal, lower triangle, identity a perfect elimination order
    rng = np.random.default_rng(3)
    q = rng.permutation(n)
    J = np.repeat(np.arange(n), np.diff(cp))
    I = np.asarray(ri)
    s0 = Symbolic(sp.csc_matrix((np.ones(len(I)), (I, J)), shape=(n, n)))   # the same graph with (I, J) as its own labels
    Lf = sp.csc_matrix((rng.standard_normal(len(I)) * 0.4 + (I == J) * 2.0, (I, J)), shape=(n, n)).toarray()
    Xd = Lf @ Lf.T
    Dv = rng.standard_normal(len(I))
    blkX = cspmatrix.from_entries(s0, I, J, Xd[I, J], device="cpu").blkval.numpy()
    blkD = cspmatrix.from_entries(s0, I, J, Dv, device="cpu").blkval.numpy()
    ref = clique_spectra_ref(s0, blkX)
    m_ref = margin_ref(s0, blkX)[0]
    tol = max(bound(r) for r in ref)
    a, b = q[I], q[J]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    X0 = sp.coo_matrix((Xd[I, J], (I, J)), shape=(n, n))
    Xs = sp.coo_matrix((Xd[I, J], (lo, hi)), shape=(n, n))                   # relabelled, upper triangle
    m0, ms = base.cone_margin(X0), base.cone_margin(Xs)
    assert abs(m0 - m_ref) <= tol and abs(ms - m_ref) <= tol
    D0 = sp.coo_matrix((Dv, (I, J)), shape=(n, n))
    Ds = sp.coo_matrix((Dv, (lo, hi)), shape=(n, n))
    a_ref = max_step_ref(s0, blkX, blkD)[0]
    tol = pencil_bound(s0, blkD, blkX)                                       # of mu = -1 / alpha, the pencil eigenvalue
    a0, a_s = base.max_step(X0, D0), base.max_step(Xs, Ds)
    assert abs(-1.0 / a0 + 1.0 / a_ref) <= tol and abs(-1.0 / a_s + 1.0 / a_ref) <= tol


# ---- launches --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["band", "arrow"])
@pytest.mark.parametrize("pencil", [False, True])
def test_launch_counts(name, pencil):
    symb = device_symb(name)
    A = on_device(symb, indefinite_on_V(symb, 1))
    B = on_device(symb, pencil_B_on_V(symb, 2)) if pencil else None
    chordal.clique_eigvalsh(A, B)                                            # buffers of the first call
    counts = launch_counts(symb, lambda: chordal.clique_eigvalsh(A, B))
    assert 1 <= counts["k_ceig"] <= 6 and counts["k_ceig_reduce"] == 1
    assert set(counts) <= {"k_ceig", "k_ceig_reduce", "k_gather_level"}     # only the gathers grow with the depth of the tree
    assert counts.get("k_gather_level", 0) <= (2 if pencil else 1) * symb.nlev
