"""Time chordal.chol_update on one MI355X against the route there was before it: syrk(X, V) on the
matrix X = L L^T followed by cholesky(X).  Patterns: synth50k (n = 50 000, 8073 cliques) and the max-cut pattern of config 4
(n = 1000, a 548-row root).  Columns: v = e_i with i the first column of a deepest leaf (k = 1), and 16 such columns in the
16 deepest distinct leaves (k = 16).  Device events around one call, one warm call of each route first, then the two routes
alternated call by call in one process; median of seven with min and max.  An update (a = +1) and the downdate that undoes
it (a = -1) alternate, so L stays what it was; both are timed and reported.  Per case also the launches of one call with
the time of every kernel (csp_profile_*), the cliques on the union of the paths, the time of the walk per visited clique,
and the walk for v = e_i with i the first column of the root: the root alone, which one workgroup sweeps.

    python tools/chol_update_time.py [--out FILE.json] [case ...]      cases: synth50k maxcut   (default: both)
"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from smcp_amd import chordal
from smcp_amd.cspmatrix import cspmatrix
from tools.trmm_time import CASES, factor_input, launches, timed

REPS = 7


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def deepest_leaves(symb, count):
    par = np.asarray(symb.snpar)
    depth = np.zeros(symb.Nsn, dtype=np.int64)
    for s in range(symb.Nsn - 1, -1, -1):                            # parents have larger numbers
        depth[s] = 0 if par[s] < 0 else depth[par[s]] + 1
    leaves = np.setdiff1d(np.arange(symb.Nsn), par[par >= 0])
    order = leaves[np.argsort(-depth[leaves], kind="stable")][:count]
    return [int(s) for s in order], depth


def path_union(symb, cliques):
    par = np.asarray(symb.snpar)
    out = set()
    for s in cliques:
        while s >= 0 and s not in out:
            out.add(s)
            s = int(par[s])
    return out


def unit_rows(symb, cliques):
    V = torch.zeros((len(cliques), symb.n), dtype=torch.float64, device="cuda")
    for j, s in enumerate(cliques):
        V[j, int(symb.snptr[s])] = 1.0
    return V


def measure(symb, L, X, V, with_baseline=True):
    """chol_update(L, V, +1) / (L, V, -1) alternated with syrk + cholesky on a copy of X"""
    k = V.shape[0]
    plus, minus = [1.0] * k, [-1.0] * k
    X2 = X.copy()

    def refactor():
        chordal.syrk(X2, V)
        chordal.cholesky(X2)

    chordal.chol_update(L, V, plus)                                  # warm: the workspace is grown here
    chordal.chol_update(L, V, minus)
    if with_baseline:
        refactor()
    t_up, t_down, t_ref = [], [], []
    for _ in range(REPS):
        t_up.append(timed(lambda: chordal.chol_update(L, V, plus)))
        if with_baseline:
            X2.blkval.copy_(X.blkval)
            chordal.touch(X2)
            t_ref.append(timed(refactor))
        t_down.append(timed(lambda: chordal.chol_update(L, V, minus)))
    lch = launches(symb, lambda: chordal.chol_update(L, V, plus))
    chordal.chol_update(L, V, minus)
    rec = {"k": int(k), "update_ms": stats(t_up), "downdate_ms": stats(t_down),
           "launches": {kk: v[0] for kk, v in lch.items()}, "kernel_ms": {kk: round(v[1], 4) for kk, v in lch.items()}}
    if with_baseline:
        rec["syrk_cholesky_ms"] = stats(t_ref)
        rec["refactor_over_update"] = rec["syrk_cholesky_ms"]["median"] / rec["update_ms"]["median"]
    return rec


def run(name):
    symb = CASES[name]()
    symb.device_init(0, 1)
    L = factor_input(symb)
    L0 = L.blkval.clone()
    X = L.copy()
    chordal.llt(X)
    leaves, depth = deepest_leaves(symb, 16)
    nn, na = symb.clique_sizes()
    root = int(np.flatnonzero(np.asarray(symb.snpar) < 0)[-1])
    out = {"case": name, "n": int(symb.n), "cliques": int(symb.Nsn), "depth_of_deepest_leaf": int(depth[leaves[0]]),
           "root_rows": int(nn[root] + na[root]), "records": []}
    for label, cliques, base in (("k1_deepest_leaf", leaves[:1], True), ("k16_distinct_leaves", leaves, True), ("k1_root_alone", [root], False)):
        rec = measure(symb, L, X, unit_rows(symb, cliques), base)
        visited = path_union(symb, cliques)
        rec.update(label=label, visited_cliques=len(visited), walk_ms_per_visited_clique=rec["kernel_ms"]["k_lr_small"] / len(visited))
        out["records"].append(rec)
        print("%s %s: update %.4f ms (min %.4f max %.4f), downdate %.4f ms; %s; %d cliques visited, walk %.4f ms = %.2f us per clique; launches %s"
              % (name, label, rec["update_ms"]["median"], rec["update_ms"]["min"], rec["update_ms"]["max"], rec["downdate_ms"]["median"],
                 ("syrk + cholesky %.4f ms (min %.4f max %.4f), ratio %.2f" % (rec["syrk_cholesky_ms"]["median"], rec["syrk_cholesky_ms"]["min"],
                                                                             rec["syrk_cholesky_ms"]["max"], rec["refactor_over_update"])) if base else "no baseline",
                 len(visited), rec["kernel_ms"]["k_lr_small"], 1e3 * rec["walk_ms_per_visited_clique"], rec["launches"]), flush=True)
    out["drift_after_all_round_trips"] = float((L.blkval - L0).abs().max())
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if len(args) >= 2 and args[0] == "--out":
        out, args = args[1], args[2:]
    torch.cuda.set_device(0)
    res = {"what": ("tools/chol_update_time.py: chordal.chol_update against syrk + cholesky on one MI355X, device events, the two routes "
                    "alternated in one process, median of %d warm calls (min, max); kernel_ms: events around each launch (csp_profile_*)" % REPS),
           "cases": [run(name) for name in (args or ["synth50k", "maxcut"])]}
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
