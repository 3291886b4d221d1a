"""Time of chordal.cone_project against one iteration written with the public calls of the commit
before it: clique_gather, torch arithmetic on the packed blocks, clique_project(..., 0, inf), clique_scatter, the torch
update and one .item() per iteration for the stopping test.

The public calls cannot run the iteration itself: clique_project takes a cspmatrix, whose clique blocks agree where cliques
overlap, and the blocks T_k of the iteration do not.  The loop here is therefore a model of its COST -- the same calls on
the same shapes in the same order, the eigenvalue work done on the blocks of X instead of T_k -- and its iterates are not
those of the method.  It runs as many iterations as the new call took (at most --base-iters) and is compared per iteration.

Patterns: narrow50k (no clique wider than 84 rows) and synth50k of tools/clique_project_time.py, the same noisy input
(L L^T of random_factor_blkval plus 0.3 standard normal noise on V), tol 1e-6 and 1e-8, rho 1, relax 1.7.  Warm calls, wall
clock around a synchronised call, the two sides alternated, median (min - max) of --reps.  Prints and, with --out FILE,
writes as JSON: totals, times per iteration, iteration counts, residuals, and the device time per kernel of one call.

    python tools/cone_project_time.py [--reps N] [--maxit N] [--base-iters N] [--out FILE] [case ...]    cases: narrow50k synth50k

With --wide N[,N ...] the tool measures something else: the time per iteration of cone_project under
tune(symb, TUNE_CEIG_WIDE, N) for every N given (0: the route is off), on a Symbolic per setting, for a chunk of --chunk
iterations (tol 0: the call runs them all; 3 by default, short enough for a pattern whose iteration takes seconds at 0).
The settings are alternated inside every repetition; median (min - max) of --reps.  Per setting it also records one
clique_project(A, 0, inf) on the same context -- the same eigen work with the host-ended block loop; the difference is the
price of the fixed launch chain -- the most sweeps, the cliques on the route and the device time per kernel of one call.
The case maxcut is the config-4 max-cut pattern (problems.maxcut_graph_pattern) with the same noisy input.

    python tools/cone_project_time.py --wide 0,65 [--chunk K] [--reps N] [--out FILE] [case ...]    cases: maxcut narrow50k synth50k
"""
import json
import math
import os
import sys

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from clique_project_time import CASES, kernel_ms, stats, wall
from smcp_amd import chordal, problems
from smcp_amd.cspmatrix import cspmatrix

RHO, RELAX = 1.0, 1.7


def public_call_loop(A, iters, tol, scale):
    """`iters` iterations of the shape of the method with the public calls (see above); returns the last stopping test"""
    symb = A.symb
    wt = chordal.cone_weights(symb)
    mult = chordal.clique_multiplicity(symb)
    X = A.copy()
    W = chordal.clique_gather(A)
    U = torch.zeros_like(W)
    res = False
    for _ in range(iters):
        Xg = chordal.clique_gather(X)                                  # the packed blocks, once
        Zp = W + U
        T = Zp + RELAX * (Xg - Zp) + U                                 # torch passes over the blocks
        Z = chordal.clique_project(X, 0.0, math.inf)                   # the eigenvalue work (on X_gg: see the module docstring)
        U = T - Z
        W = Z - U                                                      # the packed blocks, twice
        S = chordal.clique_scatter(symb, W)
        Xn = (A.blkval + RHO * S.blkval) / (1.0 + RHO * mult)
        r2 = ((Xg - Z) ** 2).sum()
        s2 = (wt * (Xn - X.blkval) ** 2).sum()
        X = cspmatrix(symb, Xn)
        res = torch.stack((r2, s2)).sqrt().max().item() <= tol * scale  # the one read-back of an iteration; the model runs its
    return res                                                         # count out whatever the test says: the iterates are not the method's


def run(name, reps, maxit, base_iters):
    symb = CASES[name]()
    symb.device_init(0, 1)
    nf = np.diff(symb.rowptr)
    S = cspmatrix(symb, torch.from_numpy(problems.random_factor_blkval(symb, 1)).cuda())
    chordal.llt(S)
    used = chordal.cone_weights(symb) > 0
    noise = torch.from_numpy(np.random.default_rng(2).standard_normal(symb.blklen)).cuda()
    A = cspmatrix(symb, torch.where(used, S.blkval + 0.3 * noise, torch.zeros_like(noise)))
    scale = max(1.0, math.sqrt(float(chordal.dot(A, A))))
    res = {"case": name, "n": symb.n, "nsn": symb.Nsn, "levels": symb.nlev, "widest_clique": int(nf.max()), "reps": reps,
           "cliques_beyond_89_rows": int((nf > 89).sum()), "rho": RHO, "relax": RELAX, "maxit": maxit, "norm_A": scale, "runs": []}
    print("%s: n %d Nsn %d levels %d widest clique %d, |A| %.2f" % (name, symb.n, symb.Nsn, symb.nlev, int(nf.max()), scale), flush=True)
    for tol in (1e-6, 1e-8):
        new = lambda: chordal.cone_project(A, tol=tol, maxit=maxit, rho=RHO, relax=RELAX, return_info=True)
        t_first, (X, info) = wall(new)
        iters = info["iterations"]
        nb = min(iters, base_iters)
        old = lambda: public_call_loop(A, nb, tol, scale)
        wall(old)                                                      # warm: the buffers of the first calls
        t_new, t_old = [], []
        for _ in range(reps):                                          # alternated
            t_new.append(wall(new)[0])
            t_old.append(wall(old)[0])
        kern = kernel_ms(symb, new)
        r = {"tol": tol, "iterations": iters, "converged": info["converged"], "primal": info["primal"], "dual": info["dual"],
             "distance": info["distance"], "sweeps": info["sweeps"], "first_call_ms": t_first,
             "cone_project": stats(t_new), "cone_project_per_iteration": stats([t / iters for t in t_new]),
             "public_call_loop_iterations": nb, "public_call_loop": stats(t_old),
             "public_call_loop_per_iteration": stats([t / nb for t in t_old]), "kernels_of_one_cone_project": kern}
        res["runs"].append(r)
        pi, po = r["cone_project_per_iteration"], r["public_call_loop_per_iteration"]
        print("%s tol %.0e: %d iterations (converged %s, primal %.1e, dual %.1e, most sweeps %d); cone_project %.1f ms (min %.1f max %.1f), "
              "%.3f ms per iteration (min %.3f max %.3f); public-call loop of %d iterations %.3f ms per iteration (min %.3f max %.3f); "
              "median of %d" % (name, tol, iters, info["converged"], info["primal"], info["dual"], info["sweeps"], r["cone_project"]["median_ms"],
                                min(t_new), max(t_new), pi["median_ms"], pi["min_ms"], pi["max_ms"], nb, po["median_ms"], po["min_ms"],
                                po["max_ms"], reps), flush=True)
        print("%s tol %.0e: kernels of one cone_project: %s" % (name, tol, json.dumps(kern)), flush=True)
    return res


WIDE_CASES = dict(CASES, maxcut=CASES["config4"])


def run_wide(name, wides, reps, chunk):
    """per-iteration time of a chunk of cone_project at every setting of TUNE_CEIG_WIDE, one Symbolic per setting"""
    res = {"case": name, "chunk": chunk, "reps": reps, "rho": RHO, "relax": RELAX, "settings": {}}
    ctx = {}
    for wd in wides:
        symb = WIDE_CASES[name]()
        symb.device_init(0, 1)
        chordal.tune(symb, chordal.TUNE_CEIG_WIDE, wd)
        S = cspmatrix(symb, torch.from_numpy(problems.random_factor_blkval(symb, 1)).cuda())
        chordal.llt(S)
        used = chordal.cone_weights(symb) > 0
        noise = torch.from_numpy(np.random.default_rng(2).standard_normal(symb.blklen)).cuda()
        A = cspmatrix(symb, torch.where(used, S.blkval + 0.3 * noise, torch.zeros_like(noise)))
        call = lambda A=A: chordal.cone_project(A, tol=0.0, maxit=chunk, rho=RHO, relax=RELAX, return_info=True)
        t_first, (X, info) = wall(call)                                # warm: the workspace and the lists of this setting
        proj = lambda A=A: chordal.clique_project(A, 0.0, math.inf)
        wall(proj)
        ctx[wd] = (symb, call, proj, info, t_first)
    nf = np.diff(ctx[wides[0]][0].rowptr)
    res.update({"n": ctx[wides[0]][0].n, "nsn": ctx[wides[0]][0].Nsn, "widest_clique": int(nf.max())})
    t_it = {wd: [] for wd in wides}
    t_pr = {wd: [] for wd in wides}
    for _ in range(reps):                                              # alternated
        for wd in wides:
            t_it[wd].append(wall(ctx[wd][1])[0] / chunk)
            t_pr[wd].append(wall(ctx[wd][2])[0])
    for wd in wides:
        symb, call, proj, info, t_first = ctx[wd]
        r = {"first_call_ms": t_first, "per_iteration": stats(t_it[wd]), "clique_project": stats(t_pr[wd]),
             "chain_price_ms": float(np.median(t_it[wd]) - np.median(t_pr[wd])), "sweeps": info["sweeps"], "wide": info.get("wide", 0),
             "primal": info["primal"], "dual": info["dual"], "kernels_of_one_call": kernel_ms(symb, call)}
        res["settings"][str(wd)] = r
        print("%s wide %d: %.3f ms per iteration (min %.3f max %.3f) over chunks of %d; clique_project %.3f ms (min %.3f max %.3f); "
              "%d cliques on the route, most sweeps %d; median of %d" % (name, wd, r["per_iteration"]["median_ms"], min(t_it[wd]), max(t_it[wd]),
                                                                        chunk, r["clique_project"]["median_ms"], min(t_pr[wd]), max(t_pr[wd]),
                                                                        r["wide"], r["sweeps"], reps), flush=True)
        print("%s wide %d: kernels of one call: %s" % (name, wd, json.dumps(r["kernels_of_one_call"])), flush=True)
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--reps": 5, "--maxit": 300, "--base-iters": 20, "--chunk": 3}
    out, wides = None, None
    if "--wide" in args:
        i = args.index("--wide")
        wides = [int(v) for v in args[i + 1].split(",")]
        del args[i:i + 2]
    for key in list(opts):
        if key in args:
            i = args.index(key)
            opts[key] = int(args[i + 1])
            del args[i:i + 2]
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    torch.cuda.set_device(0)
    results = []
    for name in (args or ["narrow50k", "synth50k"]):
        if wides is not None:
            results.append(run_wide(name, wides, opts["--reps"], opts["--chunk"]))
        else:
            results.append(run(name, opts["--reps"], opts["--maxit"], opts["--base-iters"]))
        if out:
            with open(out, "w") as f:
                json.dump(results, f, indent=1)
                f.write("\n")
