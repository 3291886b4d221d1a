"""Time of chordal.dual_max_step against the same question answered as solvers.py's `bisect` answers
it: one cholesky of the full step plus three chordal.probe_cone(kind='d') rounds of eight trial factorisations (resolution
1/512 of the interval).  Patterns: synth50k and the config-4 max-cut pattern; S = L L^T of random_factor_blkval, D random on
V and scaled so that the boundary lies at 0.37 of the full step (by a first dual_max_step at maxit = 128).  Warm calls, wall
clock around a synchronised call, median of --reps (20).  Prints both times, both answers, the steps taken and the device
time of the kernels of one dual_max_step call; --out FILE also writes them as JSON.

    python tools/dual_step_time.py [--reps N] [--out FILE] [case ...]      cases: synth50k config4 (default: both)
"""
import json
import math
import os
import sys

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from max_step_time import CASES, MINSTEP, kernel_ms, wall
from smcp_amd import chordal, problems
from smcp_amd.cspmatrix import cspmatrix


def probe_search(S, D):
    """bisect of solvers.py with options['batched_linesearch'] on the dual cone: the largest g in [MINSTEP, 1] with S + g D
    positive definite"""
    lo, hi, g = MINSTEP, 1.0, MINSTEP
    try:
        chordal.cholesky(S + D)
        return 1.0
    except ArithmeticError:
        pass
    for _ in range(3):
        pts = [lo + (hi - lo) * (k + 1) / 8 for k in range(8)]
        ok = chordal.probe_cone(S, D, pts, "d")
        kmax = max([k for k in range(8) if ok[k]], default=-1)
        if kmax >= 0:
            lo = g = pts[kmax]
        if kmax == 7:
            break
        hi = pts[kmax + 1]
    return g


def run(name, reps, tol=1e-10, maxit=64):
    symb = CASES[name]()
    symb.device_init(0, 1)
    L = cspmatrix(symb, torch.from_numpy(problems.random_factor_blkval(symb, 1)).cuda())
    S = L.copy()
    chordal.llt(S)
    D = cspmatrix(symb, torch.from_numpy(np.random.default_rng(2).standard_normal(symb.blklen)).cuda())
    t_first, (a0, i0) = wall(lambda: chordal.dual_max_step(L, D, tol=1e-12, maxit=128, return_info=True))
    assert 0 < a0 < math.inf
    D *= a0 / 0.37
    t_one, (alpha, info) = wall(lambda: chordal.dual_max_step(L, D, tol=tol, maxit=maxit, return_info=True))
    print("%s: n %d Nsn %d levels %d; scaling call (maxit 128, tol 1e-12) %.2f ms, %d steps, converged %s; first timed-form call %.2f ms"
          % (name, symb.n, symb.Nsn, symb.nlev, t_first, i0["steps"], i0["converged"], t_one), flush=True)
    t_new = [wall(lambda: chordal.dual_max_step(L, D, tol=tol, maxit=maxit))[0] for _ in range(reps)]
    t_probe0, g = wall(lambda: probe_search(S, D))          # builds the replicated pattern
    t_old = [wall(lambda: probe_search(S, D))[0] for _ in range(reps)]
    kern = kernel_ms(symb, lambda: chordal.dual_max_step(L, D, tol=tol, maxit=maxit))
    t_margin, (margin, minfo) = wall(lambda: chordal.dual_margin(L, tol=tol, maxit=maxit, return_info=True))
    t_margin = [wall(lambda: chordal.dual_margin(L, tol=tol, maxit=maxit))[0] for _ in range(min(reps, 5))]
    try:
        chordal.cholesky(S + D * ((1 - 1e-6) * alpha))
        inside = True
    except ArithmeticError:
        inside = False
    try:
        chordal.cholesky(S + D * ((1 + 1e-6) * alpha))
        outside = False
    except ArithmeticError:
        outside = True
    keep = ("theta_min", "theta_max", "resid_min", "resid_max", "steps", "converged", "invariant", "alpha_safe")
    res = {"case": name, "n": symb.n, "nsn": symb.Nsn, "levels": symb.nlev, "reps": reps, "tol": tol, "maxit": maxit,
           "dual_max_step_ms": float(np.median(t_new)), "dual_max_step_ms_min": min(t_new), "dual_max_step_ms_max": max(t_new),
           "probe_search_ms": float(np.median(t_old)), "probe_search_ms_min": min(t_old), "probe_search_ms_max": max(t_old),
           "probe_search_first_call_ms": t_probe0, "dual_margin_ms": float(np.median(t_margin)),
           "alpha": alpha, "info": {k: info[k] for k in keep}, "probe_answer": g,
           "cholesky_succeeds_just_inside": inside, "cholesky_fails_just_outside": outside,
           "margin": margin, "margin_steps": minfo["steps"], "margin_converged": minfo["converged"], "cond_estimate": minfo["cond"],
           "kernels_of_one_dual_max_step": kern}
    print("%s: dual_max_step %.3f ms (min %.3f max %.3f), probe search %.3f ms (min %.3f max %.3f), median of %d; dual_margin %.3f ms"
          % (name, res["dual_max_step_ms"], min(t_new), max(t_new), res["probe_search_ms"], min(t_old), max(t_old), reps, res["dual_margin_ms"]))
    print("%s: dual_max_step = %.15g after %d steps (converged %s, alpha_safe %.15g), probe search = %.15g (resolution 1/512); "
          "cholesky just inside: %s, just outside fails: %s" % (name, alpha, info["steps"], info["converged"], info["alpha_safe"], g, inside, outside))
    print("%s: dual_margin = %.6g after %d steps (converged %s)" % (name, margin, minfo["steps"], minfo["converged"]))
    print("%s: kernels of one dual_max_step call: %s" % (name, json.dumps(kern)), flush=True)
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
    results = [run(name, reps) for name in (args or list(CASES))]
    if out:
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
