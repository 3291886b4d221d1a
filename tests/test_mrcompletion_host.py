"""Minimum-rank PSD completion (smcp_amd.chordal.mrcompletion, csrc/front_mrc.hip) restated in numpy, and the properties
of its contract checked on that restatement (no GPU needed; tests/test_gpu_mrcompletion.py compares the kernels with it).

Pass 1: r = max over the cliques g of rank_tol(X_gg), the pivots of a diagonally pivoted Cholesky (LAPACK pstrf
semantics) above tol * max diag(X_gg); a remaining pivot below -tol * max diag means X has no PSD completion.
Pass 2, root first: Y_A^T P = Q R (column-pivoted Householder QR, ra steps), Z1 = (F_NA P)[:, :ra] R11^-1,
Z2 = pivoted Cholesky factor of F_NN - Z1 Z1^T (at most r - ra columns), Y_N = [Z1 Z2 0] Q^T.
"""
import numpy as np
import pytest

from helpers import PATTERNS
from smcp_amd import problems
from smcp_amd.symbolic import Symbolic


# ---- the restatement -----------------------------------------------------------------------------------------------
def pchol(A, thr, maxcols=None):
    """Diagonally pivoted Cholesky of the symmetric A: (L with L L^T ~ A, rows in A's order; neg; more) as mrc_pchol."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    maxcols = n if maxcols is None else maxcols
    done = np.zeros(n, dtype=bool)
    cols = []
    more = False
    while True:
        d = np.where(done, -np.inf, np.diag(A))
        p = int(np.argmax(d)) if n else -1
        if p < 0 or not d[p] > thr:
            break
        if len(cols) == maxcols:
            more = True
            break
        s = np.sqrt(d[p])
        lv = np.where(done, 0.0, A[:, p] / s)
        lv[p] = 0.0
        col = lv.copy()
        col[p] = s
        cols.append(col)
        done[p] = True
        A -= np.outer(lv, lv)
    L = np.array(cols).T.reshape(n, len(cols))
    rest = np.diag(A)[~done]
    neg = (not more) and rest.size > 0 and rest.min() < -thr
    return L, bool(neg), more


def qrp(M, thr):
    """Column-pivoted Householder QR of M (m x nc) as mrc_qrp: (R (ra x nc, pivoted columns), V, tau, perm, ra)."""
    M = np.array(M, dtype=np.float64)
    m, nc = M.shape
    perm = np.arange(nc)
    vs, taus = [], []
    j = 0
    while j < min(m, nc):
        cn = (M[j:, j:] ** 2).sum(axis=0)
        p = int(np.argmax(cn))
        if not cn[p] > thr:
            break
        p += j
        M[:, [j, p]] = M[:, [p, j]]
        perm[[j, p]] = perm[[p, j]]
        alpha, nrm = M[j, j], np.sqrt(cn[p - j])
        beta = -nrm if alpha >= 0 else nrm
        v = np.zeros(m)
        v[j] = 1.0
        v[j + 1:] = M[j + 1:, j] / (alpha - beta)
        tau = (beta - alpha) / beta
        M[j + 1:, j] = 0.0
        M[j, j] = beta
        M[:, j + 1:] -= tau * np.outer(v, v @ M[:, j + 1:])
        vs.append(v)
        taus.append(tau)
        j += 1
    return M[:j], vs, taus, perm, j


def blkval_of(symb, Xp):
    """blkval of the dense symmetric Xp (permuted order) on the pattern of symb."""
    b = np.zeros(symb.blklen)
    for k in range(symb.Nsn):
        rows = symb.rowidx[symb.rowptr[k]:symb.rowptr[k + 1]]
        cols = np.arange(symb.snptr[k], symb.snptr[k + 1])
        b[symb.blkptr[k]:symb.blkptr[k + 1]] = Xp[np.ix_(rows, cols)].ravel(order="F")
    return b


def dense_of(symb, blk):
    """Dense symmetric matrix (permuted order) with the values of blk on V and zeros elsewhere."""
    X = np.zeros((symb.n, symb.n))
    for k in range(symb.Nsn):
        rows = symb.rowidx[symb.rowptr[k]:symb.rowptr[k + 1]]
        nn, nf = symb.snptr[k + 1] - symb.snptr[k], len(rows)
        P = blk[symb.blkptr[k]:symb.blkptr[k + 1]].reshape(nn, nf).T
        for t in range(nn):
            X[rows[t:], rows[t]] = P[t:, t]
            X[rows[t], rows[t:]] = P[t:, t]
    return X


def clique_rows(symb, k):
    return symb.rowidx[symb.rowptr[k]:symb.rowptr[k + 1]]


def mrc_rank(symb, blk, tol):
    """Pass 1: (r, per-clique ranks); ArithmeticError naming the lowest clique whose block is not PSD."""
    X = dense_of(symb, blk)
    ranks = []
    for k in range(symb.Nsn):
        rows = clique_rows(symb, k)
        F = X[np.ix_(rows, rows)]
        thr = tol * max(np.diag(F).max(), 0.0)
        L, neg, _ = pchol(F, thr)
        if neg:
            raise ArithmeticError("mrcompletion: matrix is not positive definite (clique %d)" % k)
        ranks.append(L.shape[1])
    return (max(ranks) if ranks else 0), ranks


def mrcompletion(symb, blk, tol=1e-12):
    """Both passes: Y (n x r, permuted order) and the number of cliques that hit the r-column cap."""
    r, _ = mrc_rank(symb, blk, tol)
    X = dense_of(symb, blk)
    Y = np.zeros((symb.n, r))
    clamped = 0
    for l in range(symb.nlev - 1, -1, -1):
        for k in symb.levidx[symb.levptr[l]:symb.levptr[l + 1]]:
            rows = clique_rows(symb, k)
            nn = symb.snptr[k + 1] - symb.snptr[k]
            N, A = rows[:nn], rows[nn:]
            thr = tol * max(np.diag(X)[rows].max(), 0.0)
            W = np.zeros((nn, r))
            R, vs, taus, perm, ra = qrp(Y[A].T, thr) if len(A) else (None, [], [], None, 0)
            if ra:
                B = X[np.ix_(N, A[perm[:ra]])]
                W[:, :ra] = np.linalg.solve(np.triu(R[:, :ra]).T, B.T).T
            S = X[np.ix_(N, N)] - W[:, :ra] @ W[:, :ra].T
            Z2, _, more = pchol(S, thr, r - ra)
            clamped += more
            W[:, ra:ra + Z2.shape[1]] = Z2
            for j in range(ra - 1, -1, -1):
                v = vs[j]
                W -= taus[j] * np.outer(W @ v, v)
            Y[N] = W
    return Y, clamped


# ---- properties ----------------------------------------------------------------------------------------------------
def pattern_cases():
    cases = [(name, PATTERNS[name]) for name in sorted(PATTERNS)]
    cases += [("random_chordal_%d" % s, (lambda s=s: problems.random_chordal_pattern(18, max_nn=5, max_na=7, seed=s)))
              for s in (3, 4)]
    return cases


CASES = pattern_cases()


def low_rank_on_V(symb, k, seed):
    G = np.random.default_rng(seed).standard_normal((symb.n, k))
    return blkval_of(symb, G @ G.T)


def pd_on_V(symb, seed):
    """Positive definite on every clique: L L^T with L lower on V (zero fill: the pattern is chordal in this order)."""
    rng = np.random.default_rng(seed)
    mask = dense_of(symb, np.ones(symb.blklen)) != 0
    L = np.where(np.tril(mask), rng.standard_normal((symb.n, symb.n)) * 0.4, 0.0)
    L[np.diag_indices(symb.n)] = 1.0 + rng.random(symb.n)
    return blkval_of(symb, L @ L.T)


def residual(symb, blk, Y):
    """max |P_V(Y Y^T) - X| over V."""
    return np.abs(blkval_of(symb, Y @ Y.T) - blk).max()


@pytest.mark.parametrize("name,pat", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_low_rank_input_gives_rank_min_k_omega(name, pat, k):
    symb = Symbolic(pat())
    blk = low_rank_on_V(symb, k, seed=k)
    Y, clamped = mrcompletion(symb, blk)
    assert Y.shape == (symb.n, min(k, symb.max_front))
    assert clamped == 0
    assert residual(symb, blk, Y) <= 1e-10 * np.abs(blk).max()


@pytest.mark.parametrize("name,pat", CASES, ids=[c[0] for c in CASES])
def test_positive_definite_input_gives_rank_omega(name, pat):
    symb = Symbolic(pat())
    blk = pd_on_V(symb, seed=5)
    Y, clamped = mrcompletion(symb, blk)
    assert Y.shape == (symb.n, symb.max_front)
    assert clamped == 0
    assert residual(symb, blk, Y) <= 1e-10 * np.abs(blk).max()


def leaf_clique(symb):
    """A clique without children and with a separator (its own columns appear in no other clique)."""
    nch = np.diff(symb.chptr)
    nn, na = symb.clique_sizes()
    return int(np.flatnonzero((nch == 0) & (na > 0))[0])


@pytest.mark.parametrize("name", ["arrow", "nested", "rand2"])
def test_indefinite_clique_block_is_reported_with_its_clique(name):
    symb = Symbolic(PATTERNS[name]())
    blk = low_rank_on_V(symb, 3, seed=1)
    k = leaf_clique(symb)
    j = symb.snptr[k]
    blk[symb.blkptr[k]] = -1.0                     # X_jj < 0: only clique k holds column j
    assert j == clique_rows(symb, k)[0]
    with pytest.raises(ArithmeticError, match=r"\(clique %d\)" % k):
        mrcompletion(symb, blk)


def test_restatement_pieces():
    """pchol / qrp against their definitions: L L^T = A for PSD A of rank 4, Q R = M P with R upper triangular."""
    rng = np.random.default_rng(0)
    G = rng.standard_normal((9, 4))
    A = G @ G.T
    L, neg, more = pchol(A, 1e-12 * A.diagonal().max())
    assert L.shape == (9, 4) and not neg and not more
    assert np.abs(L @ L.T - A).max() < 1e-12 * A.diagonal().max()
    M = rng.standard_normal((6, 8))
    R, vs, taus, perm, ra = qrp(M, 0.0)
    assert ra == 6
    Q = np.eye(6)
    for v, t in zip(reversed(vs), reversed(taus)):
        Q = (np.eye(6) - t * np.outer(v, v)) @ Q
    assert np.allclose(Q @ R, M[:, perm], atol=1e-12)
    assert np.allclose(np.tril(R[:, :6], -1), 0.0)
    _, neg, _ = pchol(np.array([[1.0, 2.0], [2.0, 1.0]]), 1e-12)
    assert neg
