"""Time chordal.psdcompletion against the older dense route on the same positive definite input:
chordal.completion plus two chordal.trsm with the n x n identity.  Device part only (events), the two routes alternated in
one process, median of five warm calls each; also the fill's useful flops, sum of 2 |R| ra nn over the level schedule
(ra = |A| on a positive definite input), against the fp64 MFMA peak, and the 8 n^2 output bytes against the HBM peak.

    python tools/psd_time.py [case ...]      cases: config4 arrow_big nested_mid big   (default: all)
    python tools/psd_time.py --once case     one warm psdcompletion call and nothing else (for a kernel trace)
"""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import scipy.sparse as sp
import torch

from smcp_amd import base, chordal, problems, solvers
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic

MFMA_PEAK, HBM_PEAK = 78.6e12, 8.0e12


def pd_input(symb, seed=6):
    """X = P_V(S^-1) for S = L L^T, L lower on V, off-diagonal entries of column j scaled by 0.5 / sqrt(their number)."""
    rng = np.random.default_rng(seed)
    cp, ri = symb.sparsity_pattern()
    cnt = np.maximum(np.diff(cp) - 1, 1)
    J = np.repeat(np.arange(symb.n), np.diff(cp))
    v = rng.standard_normal(len(ri)) * (0.5 / np.sqrt(cnt))[J]
    v[cp[:-1]] = 1.0 + rng.random(symb.n)
    blk = np.zeros(symb.blklen)
    blk[symb.ccs_to_blk()] = v
    X = cspmatrix(symb, torch.from_numpy(blk).cuda())
    chordal.projected_inverse(X)
    return X


def fill_flops(symb):
    """Useful flops of the fill on a full-rank input and the number of fill launches."""
    nn, na = (np.asarray(a, dtype=np.int64) for a in symb.clique_sizes())
    U, flops, launches = 0, 0, 0
    for l in range(symb.nlev - 1, -1, -1):
        lev = np.sort(np.asarray(symb.levidx[symb.levptr[l]:symb.levptr[l + 1]]))
        act = lev[na[lev] > 0]
        f1 = int((2 * (U - na[act]) * na[act] * nn[act]).sum())
        after = np.cumsum(nn[lev][::-1])[::-1] - nn[lev]         # columns of the cliques s > k of the level
        f2 = int((2 * after * na[lev] * nn[lev]).sum())
        flops += f1 + f2
        launches += (f1 > 0) + (f2 > 0)
        U += int(nn[lev].sum())
    return flops, launches


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def old_route(X, eye, L, B):
    L.blkval.copy_(X.blkval)
    B.copy_(eye)
    chordal.completion(L)
    chordal.trsm(L, B)
    chordal.trsm(L, B, trans="T")


def maxcut(solve):
    """The config-4 max-cut problem embedded as base.psdcompletion embeds it: its interior-point solution (solve) or its
    cost matrix, which has the same pattern."""
    solvers.options.update(show_progress=False, maxiters=80)
    P = base.maxcut_SDP(1000, 5909, seed=0)
    C = P.get_A(0)
    if not solve:
        return base._on_pattern(sp.csc_matrix(C))[0]
    y0 = -np.ones(1000) * (abs(C).sum(axis=1).max() + 1.0)
    sol = P.solve_feas(scaling="dual", dualstart={"y": y0})
    assert sol["status"] == "optimal"
    return base._on_pattern(sp.csc_matrix(sol["x"]))[0]


CASES = {
    "config4": None,
    "arrow_big": lambda: problems.block_arrow_pattern(12, 64, 128),
    "nested_mid": lambda: problems.nested_block_arrow_pattern(nsub=2, nmid=6, nleaf_per_mid=8, seed=3),
    "big": lambda: problems.nested_block_arrow_pattern(nsub=1, nmid=140, nleaf_per_mid=8, seed=4),
}


def setup(name, solve=True):
    """(Symbolic, positive definite X, the interior-point solution on the same pattern or None)"""
    if name == "config4":
        Xs = maxcut(solve)
        symb = Xs.symb
        Xs = Xs if solve else None
    else:
        Xs, symb = None, Symbolic(CASES[name]())
        symb.device_init(0, 1)
    return symb, pd_input(symb), Xs


def run(name):
    symb, X, Xs = setup(name)
    n = symb.n
    nn, na = symb.clique_sizes()
    flops, launches = fill_flops(symb)
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    L, B = X.copy(), eye.clone()
    old_route(X, eye, L, B)                                      # warm: workspaces for n right-hand sides, fill tables
    Z = chordal.psdcompletion(X)
    err = float((Z - 0.5 * (B + B.T)).abs().max() / Z.abs().max())
    t_new, t_old, t_sol = [], [], []
    for _ in range(5):
        t_new.append(timed(lambda: chordal.psdcompletion(X)))
        t_old.append(timed(lambda: old_route(X, eye, L, B)))
        if Xs is not None:
            t_sol.append(timed(lambda: chordal.psdcompletion(Xs, 1e-8)))
    m_new, m_old = float(np.median(t_new)), float(np.median(t_old))
    print("%s: n %d Nsn %d levels %d max |A| %d; psdcompletion %.3f ms (min %.3f max %.3f), completion + 2 trsm %.3f ms "
          "(min %.3f max %.3f), relative difference of the two results %.1e" % (name, n, symb.Nsn, symb.nlev, int(max(na)), m_new,
                                                                                 min(t_new), max(t_new), m_old, min(t_old),
                                                                                 max(t_old), err))
    if t_sol:
        print("%s: psdcompletion of the interior-point solution, tol 1e-8: %.3f ms (min %.3f max %.3f)"
              % (name, float(np.median(t_sol)), min(t_sol), max(t_sol)))
    print("%s: fill %.3f Gflop in %d launches = %.3f of the fp64 MFMA peak over the whole call; 8 n^2 = %.1f MB written = "
          "%.3f of the HBM peak" % (name, flops / 1e9, launches, flops / (m_new * 1e-3) / MFMA_PEAK, 8.0 * n * n / 1e6,
                                    8.0 * n * n / (m_new * 1e-3) / HBM_PEAK), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    torch.cuda.set_device(0)
    if args and args[0] == "--once":
        symb, X, Xs = setup(args[1], solve=False)
        chordal.psdcompletion(X)
        torch.cuda.synchronize()
        print("%s: n %d Nsn %d levels %d blklen %d" % (args[1], symb.n, symb.Nsn, symb.nlev, symb.blklen))
    else:
        for name in (args or list(CASES)):
            run(name)
