"""Time of chordal.clique_project and of clique_gather + clique_scatter against what a user can do
without them: the clique blocks cut out of the matrix, grouped by order, torch.linalg.eigh per group, clip, multiply back.
The baseline takes its blocks from X.to_dense() (config4) or, where n^2 doubles are too many (synth50k, narrow50k), from
blkval through index lists built once on the host with symb.index_map (their construction is not timed).

Patterns: synth50k, the config-4 max-cut pattern, and narrow50k: the shape of synth50k with no clique wider than 84 rows,
so every clique runs from LDS.  X = L L^T of random_factor_blkval plus 0.3 times standard normal noise on V: a noisy iterate
with some negative eigenvalues in most blocks; bounds (0, inf).  Warm calls, wall clock around a synchronised call, median
(min - max) of --reps (20).  Prints and, with --out FILE, writes as JSON: both times, the largest difference between the
two results in units of nf eps |X_gg|_F, the eigenvalues clipped, the sweeps and the device time per kernel of one call.

    python tools/clique_project_time.py [--reps N] [--out FILE] [case ...]      cases: synth50k config4 narrow50k
"""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from smcp_amd import _lib, chordal, problems
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic, mindegree


def config4():
    pat, _ = problems.maxcut_graph_pattern(1000, 5909, seed=0)
    return Symbolic(pat, mindegree(pat))


CASES = {"synth50k": lambda: Symbolic(problems.nested_block_arrow_pattern()),
         "config4": config4,
         "narrow50k": lambda: Symbolic(problems.nested_block_arrow_pattern(top=(24, 60), root=84))}
DENSE = {"config4"}          # baseline blocks from to_dense()


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def kernel_ms(symb, f):
    """device time per kernel of one call of f (csp_profile_*)"""
    lib, h = _lib.lib(), symb.handle
    nk = int(lib.csp_profile_kinds())
    lib.csp_profile_filter(h, -1)
    lib.csp_profile_enable(h, 1)
    lib.csp_profile_read(h, None, None)
    try:
        f()
        torch.cuda.synchronize()
        ms, cnt = (ctypes.c_double * nk)(), (ctypes.c_int64 * nk)()
        lib.csp_profile_read(h, ms, cnt)
    finally:
        lib.csp_profile_enable(h, 0)
    return {lib.csp_profile_kernel_name(i).decode(): {"launches": int(cnt[i]), "ms": round(ms[i], 4)} for i in range(nk) if cnt[i]}


def groups_by_order(symb):
    """order -> the cliques of that order"""
    nf = np.diff(symb.rowptr)
    return {int(o): np.flatnonzero(nf == o) for o in np.unique(nf)}


def block_lists(symb, dense):
    """order -> (where the entries of the symmetric blocks of that order come from, where they go in the packed tensor): device
    index tensors (count, nf, nf) -- blkval positions, or with dense the rows of each clique (count, nf) -- and (count, nf * nf)"""
    out = {}
    p = np.asarray(symb.p)
    q = chordal.clique_ptr(symb)
    for o, ks in groups_by_order(symb).items():
        rows = np.stack([symb.rowidx[symb.rowptr[k]:symb.rowptr[k + 1]] for k in ks])          # (count, nf), ascending
        if dense:
            src = torch.from_numpy(rows.astype(np.int64)).cuda()
        else:
            i = np.maximum(rows[:, :, None], rows[:, None, :])
            j = np.minimum(rows[:, :, None], rows[:, None, :])
            pos = symb.index_map(p[i.ravel()], p[j.ravel()]).reshape(len(ks), o, o)
            assert (pos >= 0).all()
            src = torch.from_numpy(pos).cuda()
        out[o] = (src, torch.from_numpy(q[ks][:, None] + np.arange(o * o)[None, :]).cuda())
    return out


def baseline(symb, X, lists, dense, lo, hi):
    """the packed projected blocks by torch: blocks per order, eigh, clip, multiply back"""
    Z = torch.empty(int(chordal.clique_ptr(symb)[-1]), dtype=torch.float64, device="cuda")
    if dense:
        Xd = torch.from_numpy(X.to_dense(reordered=True)).cuda()
    for o, (src, dst) in lists.items():
        B = Xd[src[:, :, None], src[:, None, :]] if dense else X.blkval[src]
        w, Q = torch.linalg.eigh(B)
        P = (Q * w.clamp(lo, hi)[:, None, :]) @ Q.transpose(1, 2)
        Z[dst] = P.reshape(len(src), -1)                                  # symmetric up to rounding: either order
    return Z


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": min(ts), "max_ms": max(ts)}


def run(name, reps):
    symb = CASES[name]()
    symb.device_init(0, 1)
    nf = np.diff(symb.rowptr)
    S = cspmatrix(symb, torch.from_numpy(problems.random_factor_blkval(symb, 1)).cuda())
    chordal.llt(S)
    noise = np.random.default_rng(2).standard_normal(symb.blklen) * (np.bincount(symb.ccs_to_blk(), minlength=symb.blklen) > 0)
    X = cspmatrix(symb, S.blkval + 0.3 * torch.from_numpy(noise).cuda())
    lo, hi = 0.0, float("inf")
    t_first, _ = wall(lambda: chordal.clique_project(X, lo, hi))
    t_one, (Z, w, info) = wall(lambda: chordal.clique_project(X, lo, hi, return_info=True))
    sweeps = chordal.clique_eig_sweeps(symb)
    print("%s: n %d Nsn %d levels %d widest clique %d, %d doubles of blocks; first clique_project call %.2f ms, second %.2f ms"
          % (name, symb.n, symb.Nsn, symb.nlev, int(nf.max()), int(chordal.clique_ptr(symb)[-1]), t_first, t_one), flush=True)
    t_new = [wall(lambda: chordal.clique_project(X, lo, hi))[0] for _ in range(reps)]
    t_gs = [wall(lambda: chordal.clique_scatter(symb, chordal.clique_gather(X)))[0] for _ in range(reps)]
    t_g = [wall(lambda: chordal.clique_gather(X))[0] for _ in range(reps)]
    kern = kernel_ms(symb, lambda: chordal.clique_project(X, lo, hi))
    kern_gs = kernel_ms(symb, lambda: chordal.clique_scatter(symb, chordal.clique_gather(X)))
    res = {"case": name, "n": symb.n, "nsn": symb.Nsn, "levels": symb.nlev, "widest_clique": int(nf.max()), "reps": reps,
           "cliques_beyond_89_rows": int((nf > 89).sum()), "block_doubles": int(chordal.clique_ptr(symb)[-1]),
           "clique_project": stats(t_new), "gather_plus_scatter": stats(t_gs), "gather": stats(t_g),
           "eigenvalues": int(nf.sum()), "eigenvalues_clipped": int(info[:, 0].sum().item()), "sweeps": sweeps,
           "kernels_of_one_clique_project": kern, "kernels_of_one_gather_plus_scatter": kern_gs,
           "baseline_blocks_from": "to_dense" if name in DENSE else "blkval index lists"}
    print("%s: clique_project %.3f ms (min %.3f max %.3f), gather + scatter %.3f ms (min %.3f max %.3f), gather %.3f ms, median of %d"
          % (name, res["clique_project"]["median_ms"], min(t_new), max(t_new), res["gather_plus_scatter"]["median_ms"], min(t_gs),
             max(t_gs), res["gather"]["median_ms"], reps), flush=True)
    print("%s: %d of %d eigenvalues clipped, most sweeps %d; kernels of one clique_project: %s"
          % (name, res["eigenvalues_clipped"], res["eigenvalues"], sweeps, json.dumps(kern)), flush=True)
    try:
        lists = block_lists(symb, name in DENSE)
        t_b0, Zb = wall(lambda: baseline(symb, X, lists, name in DENSE, lo, hi))
        t_old = [wall(lambda: baseline(symb, X, lists, name in DENSE, lo, hi))[0] for _ in range(reps)]
        q = chordal.clique_ptr(symb)
        d = (Z - Zb).abs().cpu().numpy()
        Xg = chordal.clique_gather(X).cpu().numpy()
        ratio = max(d[q[k]:q[k + 1]].max() / (nf[k] * np.finfo(float).eps * np.sqrt((Xg[q[k]:q[k + 1]] ** 2).sum())) for k in range(symb.Nsn))
        res.update({"baseline": stats(t_old), "baseline_first_call_ms": t_b0, "largest_difference_units": float(ratio)})
        print("%s: baseline %.3f ms (min %.3f max %.3f), first call %.1f ms; largest difference %.2f nf eps |X_gg|_F"
              % (name, res["baseline"]["median_ms"], min(t_old), max(t_old), t_b0, ratio), flush=True)
    except Exception as e:       # torch without a batched symmetric eigensolver on this device: no baseline, said so
        res["baseline_error"] = repr(e)
        print("%s: baseline failed: %r" % (name, e), flush=True)
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    reps, out = 20, None
    if "--reps" in args:
        i = args.index("--reps")
        reps = int(args[i + 1])
        del args[i:i + 2]
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    torch.cuda.set_device(0)
    results = []
    for name in (args or list(CASES)):
        results.append(run(name, reps))
        if out:
            with open(out, "w") as f:
                json.dump(results, f, indent=1)
                f.write("\n")
