"""Euclidean distance matrix completion (smcp_amd.chordal.edmcompletion, csrc/front_edm.hip) restated in numpy, and the
properties of its contract checked on that restatement (no GPU needed; tests/test_gpu_edmcompletion.py compares the kernels
with it).

Per clique g = N u A the centred Gram matrix G = -1/2 (D_gg - rho 1^T - 1 rho^T + sigma), rho_i = mean_{a in A} D_ia,
sigma = mean_{a,b in A} D_ab (a root: means over g).  Pass 1: r = max over the cliques of rank_tol(G), the pivots of a
diagonally pivoted Cholesky of G without its last row and column (a vertex of the centring set, whose rows of G sum to
zero) above tol * max diag G; a remaining pivot below -tol * max diag G: D_gg is not an EDM.
Pass 2, root first: c = mean of Y_A, W_A = Y_A - 1 c^T, sigma / 2 = mean |W_a|^2, rho_a = |W_a|^2 + sigma / 2; then the
mrcompletion step on G (pivoted QR of W_A^T, Z1, pivoted Cholesky of G_NN - Z1 Z1^T) and Y_N = W_N + 1 c^T.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from smcp_amd import base, problems
from smcp_amd.symbolic import Symbolic
from test_mrcompletion_host import CASES, blkval_of, clique_rows, dense_of, leaf_clique, pchol, qrp


# ---- the restatement -----------------------------------------------------------------------------------------------
def gram(F, nn, na):
    """Centred Gram matrix of the clique block F = D_gg (clique order: own columns, then the separator)."""
    c = slice(nn, nn + na) if na else slice(0, nn)
    rho = F[:, c].mean(axis=1)
    sigma = rho[c].mean()
    return -0.5 * (F - rho[:, None] - rho[None, :] + sigma)


def edm_rank(symb, blk, tol):
    """Pass 1: (r, per-clique ranks); ArithmeticError naming the lowest clique whose block is not an EDM."""
    D = dense_of(symb, blk)
    if np.diag(D).any():
        raise ValueError("edmcompletion: D has a nonzero diagonal entry")
    ranks = []
    for k in range(symb.Nsn):
        rows = clique_rows(symb, k)
        nn = symb.snptr[k + 1] - symb.snptr[k]
        G = gram(D[np.ix_(rows, rows)], nn, len(rows) - nn)
        thr = tol * max(np.diag(G).max(), 0.0)
        L, neg, _ = pchol(G[:-1, :-1], thr)        # G 1_centre = 0: without its last centring row, same rank and sign
        if neg:
            raise ArithmeticError("edmcompletion: not a Euclidean distance matrix (clique %d)" % k)
        ranks.append(L.shape[1])
    return (max(ranks) if ranks else 0), ranks


def edmcompletion(symb, blk, tol=1e-12):
    """Both passes: Y (n x r, permuted order) and the number of cliques that hit the r-column cap."""
    r, _ = edm_rank(symb, blk, tol)
    D = dense_of(symb, blk)
    Y = np.zeros((symb.n, r))
    clamped = 0
    for l in range(symb.nlev - 1, -1, -1):
        for k in symb.levidx[symb.levptr[l]:symb.levptr[l + 1]]:
            rows = clique_rows(symb, k)
            nn = symb.snptr[k + 1] - symb.snptr[k]
            N, A = rows[:nn], rows[nn:]
            if len(A):
                c = Y[A].mean(axis=0)
                WA = Y[A] - c
                wn = (WA ** 2).sum(axis=1)
                h = wn.mean()
                rho = D[np.ix_(N, A)].mean(axis=1)
            else:
                c = np.zeros(r)
                WA, wn = np.zeros((0, r)), np.zeros(0)
                rho = D[np.ix_(N, N)].mean(axis=1)
                h = 0.5 * rho.mean()
            thr = tol * max(np.concatenate([rho - h, wn]).max(), 0.0)
            W = np.zeros((nn, r))
            R, vs, taus, perm, ra = qrp(WA.T, thr) if len(A) else (None, [], [], None, 0)
            if ra:
                GNA = -0.5 * (D[np.ix_(N, A)] - rho[:, None] - wn[None, :] + h)
                W[:, :ra] = np.linalg.solve(np.triu(R[:, :ra]).T, GNA[:, perm[:ra]].T).T
            GNN = -0.5 * (D[np.ix_(N, N)] - rho[:, None] - rho[None, :] + 2.0 * h)
            Z2, _, more = pchol(GNN - W[:, :ra] @ W[:, :ra].T, thr, r - ra)
            clamped += more
            W[:, ra:ra + Z2.shape[1]] = Z2
            for j in range(ra - 1, -1, -1):
                v = vs[j]
                W -= taus[j] * np.outer(W @ v, v)
            Y[N] = W + c
    return Y, clamped


# ---- properties ----------------------------------------------------------------------------------------------------
def sqdist(P):
    """Dense squared-distance matrix of the points P (rows)."""
    g = (P ** 2).sum(axis=1)
    D = g[:, None] + g[None, :] - 2.0 * P @ P.T
    D[np.diag_indices(len(P))] = 0.0
    return np.maximum(D, 0.0)


def points_on_V(symb, k, seed):
    """(blkval of the squared distances of random points in R^k on V, the points; permuted order)."""
    P = np.random.default_rng(seed).standard_normal((symb.n, k))
    return blkval_of(symb, sqdist(P)), P


def residual(symb, blk, Y):
    """max | |Y_i - Y_j|^2 - D_ij | over V."""
    return np.abs(blkval_of(symb, sqdist(Y)) - blk).max()


@pytest.mark.parametrize("name,pat", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_points_in_Rk_give_dimension_min_k_omega(name, pat, k):
    symb = Symbolic(pat())
    blk, _ = points_on_V(symb, k, seed=k)
    Y, clamped = edmcompletion(symb, blk)
    assert Y.shape == (symb.n, min(k, symb.max_front - 1))
    # band (30, 3) in the plane is a chain of 27 levels whose every separator (3 points) spans the whole plane: each level
    # places its point by linear trilateration from rows that carry the rounding of all levels above, and the error
    # grows geometrically down the chain; the Schur complements it leaves exceed the threshold and
    # are cut at r columns
    if (name, k) == ("band", 2):
        assert residual(symb, blk, Y) <= 1e-9 * blk.max()
    else:
        assert clamped == 0
        assert residual(symb, blk, Y) <= 1e-12 * blk.max()


@pytest.mark.parametrize("name,pat", CASES, ids=[c[0] for c in CASES])
def test_generic_points_give_dimension_omega_minus_one(name, pat):
    symb = Symbolic(pat())
    blk, _ = points_on_V(symb, symb.max_front, seed=5)
    Y, clamped = edmcompletion(symb, blk)
    assert Y.shape == (symb.n, symb.max_front - 1)
    assert clamped == 0
    assert residual(symb, blk, Y) <= 1e-12 * blk.max()


def procrustes_error(Y, P):
    """Relative distance of Y from P after the best translation and orthogonal transformation."""
    Yc, Pc = Y - Y.mean(axis=0), P - P.mean(axis=0)
    U, _, Vt = np.linalg.svd(Yc.T @ Pc)
    return np.abs(Yc @ (U @ Vt) - Pc).max() / np.abs(Pc).max()


def rigid_band(k):
    """band (60, k + 2): every separator holds k + 2 points, one more than an affine basis of R^k, so each point is
    overdetermined by its clique.  With separators of exactly k + 1 points (band (60, 4) in R^3) the sequential
    trilateration down the 56-level chain amplifies rounding geometrically."""
    return problems.band_pattern(60, k + 2)


@pytest.mark.parametrize("k", [2, 3])
def test_band_recovers_the_points_up_to_a_rigid_motion(k):
    symb = Symbolic(rigid_band(k))
    blk, P = points_on_V(symb, k, seed=11)
    Y, clamped = edmcompletion(symb, blk)
    assert Y.shape == (symb.n, k) and clamped == 0
    assert procrustes_error(Y, P) <= 1e-9


@pytest.mark.parametrize("name", ["arrow", "nested", "rand2"])
def test_triangle_inequality_violation_is_reported_with_its_clique(name):
    from helpers import PATTERNS
    symb = Symbolic(PATTERNS[name]())
    blk, _ = points_on_V(symb, 2, seed=1)
    k = leaf_clique(symb)
    rows = clique_rows(symb, k)
    assert len(rows) >= 3
    blk[symb.blkptr[k] + 1] = 100.0 * blk.max()        # D_{rows[0], rows[1]}: only clique k holds column rows[0]
    with pytest.raises(ArithmeticError, match=r"\(clique %d\)" % k):
        edmcompletion(symb, blk)


def test_gram_is_the_centred_gram_of_the_points():
    """G of a clique = <P_i - c, P_j - c> for c the centroid of the separator points (of all points at a root)."""
    P = np.random.default_rng(0).standard_normal((7, 3))
    D = sqdist(P)
    for nn, na in [(4, 3), (7, 0), (6, 1)]:
        c = P[nn:].mean(axis=0) if na else P.mean(axis=0)
        assert np.allclose(gram(D, nn, na), (P - c) @ (P - c).T, atol=1e-12)


# ---- base.edmcompletion input checks (host only, before any device work) --------------------------------------------
def test_base_rejects_a_non_chordal_pattern():
    D = sp.coo_matrix((np.ones(4), ([1, 2, 3, 3], [0, 1, 2, 0])), shape=(4, 4))     # the 4-cycle 0-1-2-3-0
    with pytest.raises(ValueError, match="not chordal"):
        base.edmcompletion(D)


def test_base_rejects_a_nonzero_diagonal():
    D = sp.coo_matrix(([1.0, 2.0, 0.5], ([1, 2, 1], [0, 1, 1])), shape=(3, 3))
    with pytest.raises(ValueError, match="diagonal"):
        base.edmcompletion(D)
