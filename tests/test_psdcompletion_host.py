"""Dense maximum-determinant PSD completion (smcp_amd.chordal.psdcompletion, csrc/front_psd.hip) restated in numpy, and the
properties of its contract checked on that restatement (no GPU needed; tests/test_gpu_psdcompletion.py compares the kernels
with it).

Permuted order; clique k has columns N = snptr[k] : snptr[k + 1] and separator A.  Xh = X on V (both triangles); for
k = Nsn - 1 .. 0 with |A| > 0:  Xh[E, N] = Xh[E, A] W_k for E = {j >= snptr[k + 1]} \\ A, where W_k is the basic solution of
X_AA W = X_AN from a diagonally pivoted Cholesky of X_AA (pivots rho above tol * max diag X_AA):
W_k[rho] = X[rho, rho]^-1 X[rho, N], the other rows zero.  The level schedule (what the device runs) fills, level by level
from the roots, first the rows of all levels done and then the blocks between the cliques of the level.
"""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sla

import smcp_amd
from helpers import GPU_PATTERNS, symb_of
from smcp_amd import _lib
from smcp_amd.symbolic import Symbolic
from test_mrcompletion_host import blkval_of, clique_rows, dense_of, pchol


# ---- the restatement -----------------------------------------------------------------------------------------------
def pchol_pivots(A, thr):
    """pchol (same arithmetic, same pivots) that also returns the pivot sequence rho."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    done = np.zeros(n, dtype=bool)
    cols, piv = [], []
    while n:
        d = np.where(done, -np.inf, np.diag(A))
        p = int(np.argmax(d))
        if not d[p] > thr:
            break
        s = np.sqrt(d[p])
        lv = np.where(done, 0.0, A[:, p] / s)
        lv[p] = 0.0
        col = lv.copy()
        col[p] = s
        cols.append(col)
        piv.append(p)
        done[p] = True
        A -= np.outer(lv, lv)
    return np.array(cols).T.reshape(n, len(cols)), np.array(piv, dtype=np.int64)


def check_completable(symb, X, tol):
    """Pass 1 of mrcompletion: ArithmeticError naming the lowest clique whose block is not PSD."""
    for k in range(symb.Nsn):
        rows = clique_rows(symb, k)
        F = X[np.ix_(rows, rows)]
        _, neg, _ = pchol(F, tol * max(np.diag(F).max(), 0.0))
        if neg:
            raise ArithmeticError("psdcompletion: matrix is not positive definite (clique %d)" % k)


def separator_solve(symb, X, k, tol):
    """(global rows A[rho], W_k[rho, :]) of clique k."""
    rows = clique_rows(symb, k)
    nn = symb.snptr[k + 1] - symb.snptr[k]
    N, A = rows[:nn], rows[nn:]
    F = X[np.ix_(A, A)]
    L, piv = pchol_pivots(F, tol * max(np.diag(F).max(), 0.0))
    if len(piv) == 0:
        return A[:0], np.zeros((0, nn))
    Lp = L[piv]                                         # lower triangular: X[rho, rho] = Lp Lp^T
    Z = sla.solve_triangular(Lp, X[np.ix_(A[piv], N)], lower=True)
    return A[piv], sla.solve_triangular(Lp.T, Z, lower=False)


def psd_sequential(symb, blk, tol=1e-12):
    X = dense_of(symb, blk)
    check_completable(symb, X, tol)
    Xh = X.copy()
    n = symb.n
    for k in range(symb.Nsn - 1, -1, -1):
        rows = clique_rows(symb, k)
        nn = symb.snptr[k + 1] - symb.snptr[k]
        N, A = rows[:nn], rows[nn:]
        if len(A) == 0:
            continue
        idx, W = separator_solve(symb, X, k, tol)
        E = np.setdiff1d(np.arange(symb.snptr[k + 1], n), A)
        Xh[np.ix_(E, N)] = Xh[np.ix_(E, idx)] @ W
        Xh[np.ix_(N, E)] = Xh[np.ix_(E, N)].T
    return Xh


def psd_levels(symb, blk, tol=1e-12):
    X = dense_of(symb, blk)
    check_completable(symb, X, tol)
    Xh = X.copy()
    U = np.zeros(0, dtype=np.int64)
    for l in range(symb.nlev - 1, -1, -1):
        lev = np.sort(np.asarray(symb.levidx[symb.levptr[l]:symb.levptr[l + 1]]))
        sol = {}
        for k in lev:
            rows = clique_rows(symb, k)
            nn = symb.snptr[k + 1] - symb.snptr[k]
            N, A = rows[:nn], rows[nn:]
            if len(A) == 0:
                continue
            sol[k] = (N,) + separator_solve(symb, X, k, tol)
            R = np.setdiff1d(U, A)
            Xh[np.ix_(R, N)] = Xh[np.ix_(R, sol[k][1])] @ sol[k][2]
            Xh[np.ix_(N, R)] = Xh[np.ix_(R, N)].T
        for k in lev:                                   # the blocks between the cliques of the level
            if k not in sol:
                continue
            N, idx, W = sol[k]
            for s in lev[lev > k]:
                Ns = np.arange(symb.snptr[s], symb.snptr[s + 1])
                Xh[np.ix_(Ns, N)] = Xh[np.ix_(Ns, idx)] @ W
                Xh[np.ix_(N, Ns)] = Xh[np.ix_(Ns, N)].T
        U = np.concatenate([U] + [np.arange(symb.snptr[k], symb.snptr[k + 1]) for k in lev])
    return Xh


# ---- inputs ----------------------------------------------------------------------------------------------------------
def pd_known_answer(symb, seed):
    """(blkval of X = P_V(S^-1), S^-1, cond S) for S = L L^T, L lower on V with the off-diagonal entries of column j scaled by
    0.5 / sqrt(their number) and diagonal 1 + U(0, 1): X is positive definite on V and its completion is S^-1."""
    rng = np.random.default_rng(seed)
    mask = np.tril(dense_of(symb, np.ones(symb.blklen)) != 0, -1)
    cnt = np.maximum(mask.sum(axis=0), 1)
    L = np.where(mask, rng.standard_normal((symb.n, symb.n)) * (0.5 / np.sqrt(cnt))[None, :], 0.0)
    L[np.diag_indices(symb.n)] = 1.0 + rng.random(symb.n)
    S = L @ L.T
    Li = sla.solve_triangular(L, np.eye(symb.n), lower=True)
    Z = Li.T @ Li
    return blkval_of(symb, Z), Z, np.linalg.cond(S)


def low_rank_known_answer(symb, k, seed):
    G = np.random.default_rng(seed).standard_normal((symb.n, k))
    Z = G @ G.T
    return blkval_of(symb, Z), Z


def min_separator(symb):
    """Smallest nonempty separator (0: no clique has one) and the number of forest roots."""
    nn, na = symb.clique_sizes()
    na = np.asarray(na)
    return (int(na[na > 0].min()) if (na > 0).any() else 0), int((na == 0).sum())


def low_rank_ks(symb):
    """The ranks of the low-rank known-answer cases on this pattern: {1, 2, min |A| - 1} (1 alone where min |A| = 1); a
    single clique takes 1 and 2; none on a forest."""
    ma, roots = min_separator(symb)
    if roots != 1:
        return []
    if ma == 0:
        return [1, 2]
    return sorted({k for k in (1, 2, ma - 1) if 1 <= k < max(ma, 2)})


def rel_err(A, B):
    return np.abs(A - B).max() / np.abs(B).max()


NAMES = sorted(GPU_PATTERNS)
# ---- properties ------------------------------------------------------------------------------------------------------
def test_pchol_pivots_is_pchol():
    rng = np.random.default_rng(0)
    G = rng.standard_normal((9, 4))
    A = G @ G.T
    thr = 1e-12 * A.diagonal().max()
    L, piv = pchol_pivots(A, thr)
    L0, neg, more = pchol(A, thr)
    assert np.array_equal(L, L0) and len(piv) == 4 and not neg
    assert np.allclose(np.triu(L[piv], 1), 0.0) and np.abs(L[piv] @ L[piv].T - A[np.ix_(piv, piv)]).max() < 1e-13


@pytest.mark.parametrize("name", NAMES)
def test_pd_known_answer(name):
    symb = symb_of(name)
    blk, Z, cond = pd_known_answer(symb, seed=11)
    assert cond <= 1e3
    Xs = psd_sequential(symb, blk)
    Xl = psd_levels(symb, blk)
    e_seq, e_lev, e_two = rel_err(Xs, Z), rel_err(Xl, Z), rel_err(Xl, Xs)
    print(name, "cond %.1f seq %.1e lev %.1e seq-lev %.1e" % (cond, e_seq, e_lev, e_two))
    # fp64 on cond(S) <= 1e3: 1e-12 is three digits above eps * cond
    assert e_seq <= 1e-12 and e_lev <= 1e-12 and e_two <= 1e-12
    mask = dense_of(symb, np.ones(symb.blklen)) != 0
    assert np.array_equal(Xl[mask], dense_of(symb, blk)[mask]) and np.array_equal(Xl, Xl.T)


@pytest.mark.parametrize("name", NAMES)
def test_low_rank_known_answer(name):
    symb = symb_of(name)
    for k in low_rank_ks(symb):
        blk, Z = low_rank_known_answer(symb, k, seed=k)
        Xs = psd_sequential(symb, blk, tol=1e-10)
        Xl = psd_levels(symb, blk, tol=1e-10)
        e_seq, e_lev, e_two = rel_err(Xs, Z), rel_err(Xl, Z), rel_err(Xl, Xs)
        print(name, "k %d seq %.1e lev %.1e seq-lev %.1e" % (k, e_seq, e_lev, e_two))
        # the unique completion G G^T; the observed worst case is 1.3e-12 (nested_mid, k = 30), 1e-10 leaves two digits
        assert e_seq <= 1e-10 and e_lev <= 1e-10 and e_two <= 1e-10


def test_forest_diag_returns_diag():
    symb = symb_of("diag")
    x = 1.0 + np.random.default_rng(0).random(symb.n)
    blk = blkval_of(symb, np.diag(x))
    assert np.array_equal(psd_levels(symb, blk), np.diag(x))
    assert np.array_equal(psd_sequential(symb, blk), np.diag(x))


def two_blocks_pattern():
    """Two disconnected band blocks (orders 7 and 6, bandwidth 2)."""
    n, cols, rows = 13, [], []
    for lo, hi in ((0, 7), (7, 13)):
        for j in range(lo, hi):
            for i in range(j, min(j + 3, hi)):
                rows.append(i)
                cols.append(j)
    cp = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))])
    return n, cp, np.array(rows)


def test_forest_two_blocks_keep_zeros_between_them():
    symb = Symbolic(two_blocks_pattern())
    assert min_separator(symb)[1] == 2
    blk, Z, _ = pd_known_answer(symb, seed=2)
    for f in (psd_sequential, psd_levels):
        Xh = f(symb, blk)
        p = np.asarray(symb.p)
        first = np.isin(p, np.arange(7))                 # permuted positions of the first block
        assert np.all(Xh[np.ix_(first, ~first)] == 0.0) and np.all(Xh[np.ix_(~first, first)] == 0.0)
        assert rel_err(Xh, Z) <= 1e-12


def test_indefinite_clique_block_is_reported_with_its_clique():
    from test_mrcompletion_host import leaf_clique, low_rank_on_V
    symb = symb_of("nested")
    blk = low_rank_on_V(symb, 3, seed=1)
    k = leaf_clique(symb)
    blk[symb.blkptr[k]] = -1.0
    with pytest.raises(ArithmeticError, match=r"\(clique %d\)" % k):
        psd_levels(symb, blk)


# ---- symbols and refusal (host only) -----------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "smcp_amd.h")).read()
    assert "int csp_psdcompletion(csp_ctx* ctx, const double* blkval, double tol, double* Xd, int64_t ldX, void* stream);" in hdr
    assert "csp_psdcompletion" in _lib.SIGNATURES
    assert _lib.lib().csp_psdcompletion.argtypes == _lib.SIGNATURES["csp_psdcompletion"][1]


def test_refused_without_a_device():
    symb = Symbolic(GPU_PATTERNS["arrow"]())            # a fresh context: never initialised on a device
    x = np.zeros(symb.blklen)
    out = np.zeros((symb.n, symb.n))
    rc = _lib.lib().csp_psdcompletion(symb.handle, x.ctypes.data, ctypes.c_double(1e-12), out.ctypes.data, symb.n, None)
    assert rc == -2


def test_package_exports_psdcompletion():
    from smcp_amd import base, chordal
    assert smcp_amd.psdcompletion is base.psdcompletion
    assert callable(chordal.psdcompletion)
