"""Time of chordal.max_step against the same question answered as solvers.py's `bisect` answers it:
one completion of the full step plus three chordal.probe_cone rounds of eight trial completions (resolution 1/512 of the
interval).  Patterns: synth50k and the config-4 max-cut pattern; X positive definite on V, D random on V and scaled so
that the boundary lies at 0.37 of the full step.  Warm calls, wall clock around a synchronised call, median of --reps
(20; 5 when one call takes more than two seconds).  Prints both times, both answers, the sweep count and the device time
of the kernels of one max_step call; --out FILE also writes them as JSON.

    python tools/max_step_time.py [--reps N] [--out FILE] [case ...]      cases: synth50k config4 (default: both)
"""
import ctypes
import json
import math
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from smcp_amd import _lib, chordal, problems
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic, mindegree

MINSTEP = 1e-8        # solvers.py


def config4():
    pat, _ = problems.maxcut_graph_pattern(1000, 5909, seed=0)
    return Symbolic(pat, mindegree(pat))


CASES = {"synth50k": lambda: Symbolic(problems.nested_block_arrow_pattern()), "config4": config4}


def probe_search(X, D):
    """bisect of solvers.py with options['batched_linesearch']: the largest g in [MINSTEP, 1] with X + g D inside C_V"""
    lo, hi, g = MINSTEP, 1.0, MINSTEP
    try:
        chordal.completion(X + D)
        return 1.0
    except ArithmeticError:
        pass
    for _ in range(3):
        pts = [lo + (hi - lo) * (k + 1) / 8 for k in range(8)]
        ok = chordal.probe_cone(X, D, pts, "p")
        kmax = max([k for k in range(8) if ok[k]], default=-1)
        if kmax >= 0:
            lo = g = pts[kmax]
        if kmax == 7:
            break
        hi = pts[kmax + 1]
    return g


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


def run(name, reps):
    symb = CASES[name]()
    symb.device_init(0, 1)
    nf = np.diff(symb.rowptr)
    X = cspmatrix(symb, torch.from_numpy(problems.random_factor_blkval(symb, 1)).cuda())
    chordal.llt(X)
    D = cspmatrix(symb, torch.from_numpy(np.random.default_rng(2).standard_normal(symb.blklen)).cuda())
    t_first, a0 = wall(lambda: chordal.max_step(X, D))
    assert 0 < a0 < math.inf
    D *= a0 / 0.37
    t_one, (alpha, clique) = wall(lambda: chordal.max_step(X, D, return_clique=True))
    sweeps = chordal.clique_eig_sweeps(symb)
    print("%s: n %d Nsn %d levels %d widest clique %d; first max_step call %.2f ms, second %.2f ms" % (name, symb.n, symb.Nsn, symb.nlev, int(nf.max()), t_first, t_one), flush=True)
    if reps is None:
        reps = 20 if t_one < 2000.0 else 5
    t_new = [wall(lambda: chordal.max_step(X, D))[0] for _ in range(reps)]
    t_probe0, g = wall(lambda: probe_search(X, D))          # builds the replicated pattern
    t_old = [wall(lambda: probe_search(X, D))[0] for _ in range(reps)]
    kern = kernel_ms(symb, lambda: chordal.max_step(X, D))
    t_std = [wall(lambda: chordal.cone_margin(X))[0] for _ in range(min(reps, 5))]
    res = {"case": name, "n": symb.n, "nsn": symb.Nsn, "levels": symb.nlev, "widest_clique": int(nf.max()), "reps": reps,
           "max_step_ms": float(np.median(t_new)), "max_step_ms_min": min(t_new), "max_step_ms_max": max(t_new),
           "probe_search_ms": float(np.median(t_old)), "probe_search_ms_min": min(t_old), "probe_search_ms_max": max(t_old),
           "probe_search_first_call_ms": t_probe0, "cone_margin_ms": float(np.median(t_std)),
           "alpha": alpha, "binding_clique": clique, "binding_clique_order": int(nf[clique]), "probe_answer": g,
           "sweeps": sweeps, "kernels_of_one_max_step": kern}
    print("%s: max_step %.3f ms (min %.3f max %.3f), probe search %.3f ms (min %.3f max %.3f), median of %d; cone_margin %.3f ms"
          % (name, res["max_step_ms"], min(t_new), max(t_new), res["probe_search_ms"], min(t_old), max(t_old), reps, res["cone_margin_ms"]))
    print("%s: max_step = %.15g at clique %d (order %d), probe search = %.15g (resolution 1/512), most sweeps %d"
          % (name, alpha, clique, int(nf[clique]), g, sweeps))
    print("%s: kernels of one max_step call: %s" % (name, json.dumps(kern)), flush=True)
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    reps, out = None, None
    if "--reps" in args:
        i = args.index("--reps")
        reps = int(args[i + 1])
        del args[i:i + 2]
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    torch.cuda.set_device(0)
    results = [run(name, reps) for name in (args or list(CASES))]
    if out:
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
