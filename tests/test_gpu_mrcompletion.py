"""Minimum-rank PSD completion on the device (smcp_amd.chordal.mrcompletion / base.mrcompletion, csrc/front_mrc.hip)
against its contract and the numpy restatement of tests/test_mrcompletion_host.py, and the max-cut rounding built on it
(base.maxcut_round)."""
import time

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from helpers import PATTERNS
from smcp_amd import base, chordal, problems, solvers
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic
from test_mrcompletion_host import clique_rows, leaf_clique, low_rank_on_V, mrcompletion as mrc_numpy, pd_on_V

pytestmark = pytest.mark.gpu


def device_symb(pat):
    symb = Symbolic(pat)
    symb.device_init(0, 1)
    return symb


def residual_blk(symb, blk, Y):
    """max |P_V(Y Y^T) - X| over V, clique by clique (Y permuted order, numpy)."""
    worst = 0.0
    for k in range(symb.Nsn):
        rows = clique_rows(symb, k)
        nn, nf = symb.snptr[k + 1] - symb.snptr[k], len(rows)
        P = blk[symb.blkptr[k]:symb.blkptr[k + 1]].reshape(nn, nf).T
        low = np.arange(nf)[:, None] >= np.arange(nn)[None, :]
        worst = max(worst, np.abs(np.where(low, Y[rows] @ Y[rows[:nn]].T - P, 0.0)).max())
    return worst


@pytest.mark.parametrize("name", sorted(PATTERNS))
@pytest.mark.parametrize("k", [1, 3, 8, None])
def test_parity_patterns(name, k):
    symb = device_symb(PATTERNS[name]())
    blk = pd_on_V(symb, seed=7) if k is None else low_rank_on_V(symb, k, seed=k)
    X = cspmatrix(symb, torch.from_numpy(blk.copy()).cuda())
    Y1 = chordal.mrcompletion(X)
    Y2 = chordal.mrcompletion(X)
    assert torch.equal(Y1, Y2)                                        # bitwise deterministic
    assert torch.equal(X.blkval.cpu(), torch.from_numpy(blk))         # X untouched
    Y = Y1.cpu().numpy()
    assert Y.shape == (symb.n, symb.max_front if k is None else min(k, symb.max_front))
    Yr, clamped = mrc_numpy(symb, blk)
    assert clamped == 0 and Yr.shape == Y.shape
    # 1e-10 max|X|; a long chain of separators that hold the whole rank (band, k = 3: 27 levels) loses accuracy level by
    # level in any order of operations -- there the bound is the restatement's own residual, times 100
    tol = max(1e-10 * np.abs(blk).max(), 100 * residual_blk(symb, blk, Yr))
    assert residual_blk(symb, blk, Y) <= tol
    for c in range(symb.Nsn):                                         # clique by clique, up to the orthogonal freedom
        rows = clique_rows(symb, c)
        assert np.abs(Y[rows] @ Y[rows].T - Yr[rows] @ Yr[rows].T).max() <= 2 * tol


@pytest.mark.parametrize("k", [3, None])
def test_non_peo_input_order(k):
    """base.mrcompletion on a scipy matrix in a scrambled order (upper triangle given): Y comes back in that order."""
    s0 = Symbolic(problems.random_chordal_pattern(20, max_nn=5, max_na=7, seed=9))
    n = s0.n
    cp, ri = s0.sparsity_pattern()                  # chordal, lower triangle, identity a perfect elimination order
    rng = np.random.default_rng(3)
    q = rng.permutation(n)                          # new label of vertex i: q[i]
    J = np.repeat(np.arange(n), np.diff(cp))
    I = np.asarray(ri)
    if k is None:
        Lf = sp.csc_matrix((rng.standard_normal(len(I)) * 0.4 + (I == J) * 2.0, (I, J)), shape=(n, n)).toarray()
        Xd = Lf @ Lf.T
    else:
        G = rng.standard_normal((n, k))
        Xd = G @ G.T
    a, b = q[I], q[J]
    Xs = sp.coo_matrix((Xd[I, J], (np.minimum(a, b), np.maximum(a, b))), shape=(n, n))    # relabelled, upper triangle
    Y = base.mrcompletion(Xs)
    Xq = np.zeros((n, n))
    Xq[q[I], q[J]] = Xd[I, J]
    Xq[q[J], q[I]] = Xd[I, J]
    mask = Xq != 0
    assert np.abs(np.where(mask, Y @ Y.T - Xq, 0.0)).max() <= 1e-10 * np.abs(Xd).max()
    if k is not None:
        assert Y.shape[1] == k


def test_not_completable():
    symb = device_symb(PATTERNS["nested"]())
    blk = low_rank_on_V(symb, 3, seed=1)
    c = leaf_clique(symb)
    blk[symb.blkptr[c]] = -1.0
    X = cspmatrix(symb, torch.from_numpy(blk).cuda())
    with pytest.raises(ArithmeticError, match=r"\(clique %d\)" % c):
        chordal.mrcompletion(X)


def solve_maxcut(n, nedges):
    solvers.options.update(show_progress=False, maxiters=80)
    P = base.maxcut_SDP(n, nedges, seed=0)
    C = P.get_A(0)
    y0 = -np.ones(n) * (abs(C).sum(axis=1).max() + 1.0)
    sol = P.solve_feas(scaling="dual", dualstart={"y": y0})
    assert sol["status"] == "optimal"
    return P, sol


def check_maxcut(P, sol, tol, report):
    X = sp.csc_matrix(sol["x"])
    t0 = time.perf_counter()
    Y = base.mrcompletion(X, tol=tol)
    t1 = time.perf_counter()
    Xc = X.tocoo()
    res = np.abs(np.einsum("ij,ij->i", Y[Xc.row], Y[Xc.col]) - Xc.data).max()
    dg = np.abs(np.einsum("ij,ij->i", Y, Y) - 1.0).max()
    # documented bound: 1e-6 at tol = 1e-8 on an interior-point solution
    assert res <= 1e-6 and dg <= 1e-6, (res, dg)
    C = sp.csc_matrix(P.get_A(0))
    pobj = sol["primal objective"]
    t2 = time.perf_counter()
    cut, s = base.maxcut_round(P, X, trials=64, seed=0, tol=tol)
    t3 = time.perf_counter()
    assert set(np.unique(s)) <= {-1.0, 1.0}
    Cl = sp.tril(C, -1).tocoo()
    cut_np = float(np.sum(4.0 * Cl.data * (s[Cl.row] != s[Cl.col])))
    assert cut == cut_np
    assert cut >= 0.878 * (-pobj), (cut, -pobj)
    report.append(dict(n=P.n, r=Y.shape[1], residual=res, diag=dg, mrc_s=t1 - t0, round_s=t3 - t2, cut=cut, sdp=-pobj))


def test_maxcut_n200_end_to_end(capsys):
    P, sol = solve_maxcut(200, 600)
    rep = []
    check_maxcut(P, sol, 1e-8, rep)
    with capsys.disabled():
        print("\nmaxcut n=200:", rep[0])


def test_maxcut_config4_full_size(capsys):
    P, sol = solve_maxcut(1000, 5909)
    rep = []
    check_maxcut(P, sol, 1e-8, rep)          # first call: includes allocation of the workspaces
    check_maxcut(P, sol, 1e-8, rep)
    with capsys.disabled():
        print("\nmaxcut config 4:", rep[1])


@pytest.mark.parametrize("kind", ["rank8", "posdef"])
def test_synth50k(kind, capsys):
    symb = device_symb(problems.nested_block_arrow_pattern())
    if kind == "rank8":
        G = np.random.default_rng(0).standard_normal((symb.n, 8))
        blk = np.zeros(symb.blklen)
        for k in range(symb.Nsn):
            rows = clique_rows(symb, k)
            nn = symb.snptr[k + 1] - symb.snptr[k]
            blk[symb.blkptr[k]:symb.blkptr[k + 1]] = (G[rows] @ G[rows[:nn]].T).ravel(order="F")
        X = cspmatrix(symb, torch.from_numpy(blk).cuda())
    else:
        X = cspmatrix(symb, torch.from_numpy(problems.random_factor_blkval(symb, 3)).cuda())
        chordal.llt(X)
        blk = X.blkval.cpu().numpy()
    chordal.mrcompletion(X)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        Yd = chordal.mrcompletion(X)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    Y = Yd.cpu().numpy()
    assert Y.shape[1] == (8 if kind == "rank8" else symb.max_front)
    res = residual_blk(symb, blk, Y)
    assert res <= 1e-10 * np.abs(blk).max()
    with capsys.disabled():
        print("\nsynth50k %s: r = %d, %.2f ms (median of 3), residual %.2e (max|X| %.2e)"
              % (kind, Y.shape[1], 1e3 * sorted(ts)[1], res, np.abs(blk).max()))
