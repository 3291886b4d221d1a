"""Euclidean distance matrix completion on the device (smcp_amd.chordal.edmcompletion / edm_dense, base.edmcompletion,
csrc/front_edm.hip) against its contract and the numpy restatement of tests/test_edmcompletion_host.py."""
import re
import time

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.spatial.distance import pdist, squareform

from helpers import PATTERNS
from smcp_amd import base, chordal, problems
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic
from test_edmcompletion_host import edmcompletion as edm_numpy, points_on_V, rigid_band
from test_mrcompletion_host import blkval_of, clique_rows, leaf_clique

pytestmark = pytest.mark.gpu


def device_symb(pat):
    symb = Symbolic(pat)
    symb.device_init(0, 1)
    return symb


def residual_blk(symb, blk, Y):
    """max | |Y_i - Y_j|^2 - D_ij | over V, clique by clique (Y permuted order, numpy)."""
    worst = 0.0
    for k in range(symb.Nsn):
        rows = clique_rows(symb, k)
        nn, nf = symb.snptr[k + 1] - symb.snptr[k], len(rows)
        P = blk[symb.blkptr[k]:symb.blkptr[k + 1]].reshape(nn, nf).T
        Yr, Yn = Y[rows], Y[rows[:nn]]
        E = (Yr ** 2).sum(axis=1)[:, None] + (Yn ** 2).sum(axis=1)[None, :] - 2.0 * Yr @ Yn.T
        low = np.arange(nf)[:, None] > np.arange(nn)[None, :]
        worst = max(worst, np.abs(np.where(low, E - P, 0.0)).max())
    return worst


def blk_of_points(symb, P):
    """blkval of the squared distances of the points P (permuted order) on V, clique by clique (no n x n array)."""
    blk = np.zeros(symb.blklen)
    for k in range(symb.Nsn):
        rows = clique_rows(symb, k)
        nn = symb.snptr[k + 1] - symb.snptr[k]
        diff = P[rows][:, None, :] - P[rows[:nn]][None, :, :]
        blk[symb.blkptr[k]:symb.blkptr[k + 1]] = (diff ** 2).sum(axis=2).ravel(order="F")
    return blk


def case(name, k):
    symb = device_symb(PATTERNS[name]())
    blk, P = points_on_V(symb, symb.max_front if k is None else k, seed=5 if k is None else k)
    return symb, blk, P


@pytest.mark.parametrize("name", sorted(PATTERNS))
@pytest.mark.parametrize("k", [1, 2, 3, None])
def test_parity_patterns(name, k):
    symb, blk, _ = case(name, k)
    D = cspmatrix(symb, torch.from_numpy(blk.copy()).cuda())
    Y1 = chordal.edmcompletion(D)
    Y2 = chordal.edmcompletion(D)
    assert torch.equal(Y1, Y2)                                        # bitwise deterministic
    assert torch.equal(D.blkval.cpu(), torch.from_numpy(blk))         # D untouched
    Y = Y1.cpu().numpy()
    Yr, _ = edm_numpy(symb, blk)
    assert Y.shape == Yr.shape
    assert Y.shape[1] == (symb.max_front - 1 if k is None else min(k, symb.max_front - 1))
    # 1e-10 max D; a chain whose every separator is an affine basis (band in the plane: 27 levels) loses accuracy level by
    # level in any order of operations -- there the bound is the restatement's residual, times 100
    tol = max(1e-10 * blk.max(), 100 * residual_blk(symb, blk, Yr))
    assert residual_blk(symb, blk, Y) <= tol


@pytest.mark.parametrize("k", [2, None])
def test_non_peo_input_order(k):
    """base.edmcompletion on a scipy matrix in a scrambled order (upper triangle, no diagonal): Y comes back in that
    order, and dense=True gives the completed EDM in that order."""
    s0 = Symbolic(problems.random_chordal_pattern(20, max_nn=5, max_na=7, seed=9))
    n = s0.n
    cp, ri = s0.sparsity_pattern()                  # chordal, lower triangle, identity a perfect elimination order
    rng = np.random.default_rng(3)
    q = rng.permutation(n)                          # new label of vertex i: q[i]
    J = np.repeat(np.arange(n), np.diff(cp))
    I = np.asarray(ri)
    off = I != J
    I, J = I[off], J[off]
    P = rng.standard_normal((n, s0.max_front if k is None else k))
    Dfull = squareform(pdist(P, "sqeuclidean"))
    a, b = q[I], q[J]
    Ds = sp.coo_matrix((Dfull[I, J], (np.minimum(a, b), np.maximum(a, b))), shape=(n, n))    # relabelled, upper
    Y = base.edmcompletion(Ds)
    Dq = squareform(pdist(Y, "sqeuclidean"))
    assert np.abs(Dq[a, b] - Dfull[I, J]).max() <= 1e-10 * Dfull.max()
    Dd = base.edmcompletion(Ds, dense=True)
    assert np.array_equal(Dd, Dd.T) and not Dd.diagonal().any()
    assert np.abs(Dd[a, b] - Dfull[I, J]).max() <= 1e-10 * Dfull.max()
    assert np.abs(Dd - Dq).max() <= 1e-12 * Dfull.max()


@pytest.mark.parametrize("name", ["arrow", "nested", "rand2"])
def test_not_an_edm(name):
    symb = device_symb(PATTERNS[name]())
    blk, _ = points_on_V(symb, 2, seed=1)
    c = leaf_clique(symb)
    blk[symb.blkptr[c] + 1] = 100.0 * blk.max()
    with pytest.raises(ArithmeticError) as ref:
        edm_numpy(symb, blk)
    want = int(re.search(r"\(clique (\d+)\)", str(ref.value)).group(1))
    D = cspmatrix(symb, torch.from_numpy(blk).cuda())
    with pytest.raises(ArithmeticError, match=r"not a Euclidean distance matrix \(clique %d\)" % want):
        chordal.edmcompletion(D)


def test_nonzero_diagonal_on_the_device():
    symb, blk, _ = case("nested", 2)
    blk[symb.blkptr[3]] = 1.0
    D = cspmatrix(symb, torch.from_numpy(blk).cuda())
    with pytest.raises(ValueError, match="diagonal"):
        chordal.edmcompletion(D)


@pytest.mark.parametrize("name", sorted(PATTERNS))
@pytest.mark.parametrize("k", [2, None])
def test_dense(name, k):
    symb, blk, _ = case(name, k)
    assert symb.n <= 500
    D = cspmatrix(symb, torch.from_numpy(blk).cuda())
    Y = chordal.edmcompletion(D)
    r = Y.shape[1]
    Dh = chordal.edm_dense(symb, Y).cpu().numpy()          # permuted order
    assert np.array_equal(Dh, Dh.T) and not Dh.diagonal().any()
    Yr, _ = edm_numpy(symb, blk)
    tol = max(1e-10 * blk.max(), 100 * residual_blk(symb, blk, Yr))
    assert np.abs(blkval_of(symb, Dh) - blk).max() <= tol
    n = symb.n
    Jc = np.eye(n) - 1.0 / n
    ev = np.linalg.eigvalsh(-0.5 * Jc @ Dh @ Jc)
    assert ev.min() >= -1e-9 * Dh.max()
    assert int((ev > 1e-9 * Dh.max()).sum()) == r


@pytest.mark.parametrize("k", [2, 3])
def test_dense_rigid_band(k):
    """The completion of a rigid chain is the EDM of the points themselves (base.edmcompletion, original order)."""
    pat = rigid_band(k)
    n, cp, ri = pat
    P = np.random.default_rng(11).standard_normal((n, k))
    J = np.repeat(np.arange(n), np.diff(cp))
    I = np.asarray(ri)
    Dfull = squareform(pdist(P, "sqeuclidean"))
    Ds = sp.coo_matrix((Dfull[I, J], (I, J)), shape=(n, n))           # lower triangle and a zero diagonal
    Dd = base.edmcompletion(Ds, dense=True)
    assert np.abs(Dd - Dfull).max() <= 1e-8 * Dfull.max()


def timed(D, reps=3):
    chordal.edmcompletion(D)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        Yd = chordal.edmcompletion(D)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return Yd.cpu().numpy(), sorted(ts)[len(ts) // 2]


@pytest.mark.parametrize("kind", ["R3", "generic"])
def test_synth50k(kind, capsys):
    symb = device_symb(problems.nested_block_arrow_pattern())
    k = 3 if kind == "R3" else symb.max_front
    P = np.random.default_rng(0).standard_normal((symb.n, k))
    blk = blk_of_points(symb, P)
    D = cspmatrix(symb, torch.from_numpy(blk).cuda())
    Y, t = timed(D)
    assert Y.shape[1] == (3 if kind == "R3" else symb.max_front - 1)
    res = residual_blk(symb, blk, Y)
    assert res <= 1e-10 * blk.max()
    with capsys.disabled():
        print("\nsynth50k %s: r = %d, %.2f ms (median of 3), residual %.2e (max D %.2e)"
              % (kind, Y.shape[1], 1e3 * t, res, blk.max()))


def test_maxcut_graph_embedding(capsys):
    """The chordal embedding of the config-4 graph (wide fronts: HBM slots), distances of points in R^3 on the filled
    pattern."""
    pat, _ = problems.maxcut_graph_pattern()
    symb = device_symb(pat)
    P = np.random.default_rng(1).standard_normal((symb.n, 3))
    blk = blk_of_points(symb, P)
    D = cspmatrix(symb, torch.from_numpy(blk).cuda())
    Y, t = timed(D)
    assert Y.shape[1] == 3
    res = residual_blk(symb, blk, Y)
    assert res <= 1e-10 * blk.max()
    with capsys.disabled():
        print("\nconfig-4 embedding (n %d, max front %d): r = %d, %.2f ms (median of 3), residual %.2e (max D %.2e)"
              % (symb.n, symb.max_front, Y.shape[1], 1e3 * t, res, blk.max()))
