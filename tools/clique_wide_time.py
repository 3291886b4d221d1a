"""Time of the spectral calls on wide clique blocks under tune(symb, TUNE_CEIG_WIDE, order): the
chip-wide block Jacobi of csrc/front_ceigw.hip against the one-workgroup route (setting 0), and against what a user can do
without either: torch.linalg.eigh on the blocks, as tools/clique_project_time.py does.

Patterns: the config-4 max-cut pattern (n = 1000, root of 548 rows) and synth50k.  X as in tools/clique_project_time.py.
Calls: clique_eigvalsh(X), cone_margin(X), clique_eigh(X), clique_project(X).  Settings: 0 and 65, 90, 127, 160, 200,
interleaved in one process: every repetition runs every setting once.  Warm, synchronised calls, wall clock; median
(min - max) of --reps (5).  Also recorded per setting: the cliques on the wide route, the most sweeps, and the largest
difference of w from the setting 0 in nf eps max|w|.

    python tools/clique_wide_time.py [--reps N] [--out FILE] [--settings 0,65,...] [--once SETTING] [--pencil] [case ...]

--once SETTING: one warm-up and one clique_project under that setting and nothing else (for a kernel trace of the route);
with --pencil the two calls are clique_eigvalsh(A, B).
--pencil: the pencil form instead -- clique_eigvalsh(A, B) and max_step(B, D) with B = L L^T of
tools/clique_project_time.py (every clique block positive definite), A = X and D the noise of X -- at the settings 0 and 65
(and 90 on synth50k), interleaved in the same way; the difference of w from the setting 0 is counted in nf eps max|w|
cond(B_gg) units of the setting 0's own w.  Writes profiles/pencil_wide_bench.json unless --out names another file.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from clique_project_time import CASES, DENSE, baseline, block_lists, kernel_ms, stats, wall
from smcp_amd import chordal, problems
from smcp_amd.cspmatrix import cspmatrix

SETTINGS = [0, 65, 90, 127, 160, 200]
CALLS = {"clique_eigvalsh": lambda X: chordal.clique_eigvalsh(X), "cone_margin": lambda X: chordal.cone_margin(X),
         "clique_eigh": lambda X: chordal.clique_eigh(X), "clique_project": lambda X: chordal.clique_project(X)}


def make(name):
    symb = CASES[name]()
    symb.device_init(0, 1)
    S = cspmatrix(symb, torch.from_numpy(problems.random_factor_blkval(symb, 1)).cuda())
    chordal.llt(S)
    noise = np.random.default_rng(2).standard_normal(symb.blklen) * (np.bincount(symb.ccs_to_blk(), minlength=symb.blklen) > 0)
    return symb, cspmatrix(symb, S.blkval + 0.3 * torch.from_numpy(noise).cuda())


def make_pencil(name):
    """(symb, A, B, D): B = L L^T, positive definite on every clique; A = B + 0.3 noise, D = the noise"""
    symb = CASES[name]()
    symb.device_init(0, 1)
    B = cspmatrix(symb, torch.from_numpy(problems.random_factor_blkval(symb, 1)).cuda())
    chordal.llt(B)
    noise = np.random.default_rng(2).standard_normal(symb.blklen) * (np.bincount(symb.ccs_to_blk(), minlength=symb.blklen) > 0)
    D = cspmatrix(symb, torch.from_numpy(noise).cuda())
    return symb, cspmatrix(symb, B.blkval + 0.3 * D.blkval), B, D


PENCIL_SETTINGS = {"config4": [0, 65], "synth50k": [0, 65, 90]}


def run_pencil(name, reps, settings):
    symb, A, B, D = make_pencil(name)
    calls = {"clique_eigvalsh_pencil": lambda: chordal.clique_eigvalsh(A, B), "max_step": lambda: chordal.max_step(B, D, return_clique=True)}
    nf = np.diff(symb.rowptr)
    res = {"case": name, "n": symb.n, "nsn": symb.Nsn, "widest_clique": int(nf.max()), "reps": reps, "form": "pencil", "settings": {}}
    times = {s: {c: [] for c in calls} for s in settings}
    w0 = None
    for s in settings:                                                    # first calls: buffers, and what does not change
        chordal.tune(symb, chordal.TUNE_CEIG_WIDE, s)
        first = {c: wall(f)[0] for c, f in calls.items()}
        w = chordal.clique_eigvalsh(A, B)
        entry = {"wide_cliques": chordal.clique_eig_wide(symb), "launch_groups": chordal.clique_eig_groups(symb),
                 "most_sweeps": chordal.clique_eig_sweeps(symb), "first_call_ms": first, "max_step": list(chordal.max_step(B, D, return_clique=True))}
        if s == 0:
            w0 = w
        elif w0 is not None:
            d = (w - w0).abs().cpu().numpy()
            a = w0.abs().cpu().numpy()
            entry["w_against_setting_0_units"] = float(max(
                d[symb.rowptr[k]:symb.rowptr[k + 1]].max() / (nf[k] * np.finfo(float).eps * max(a[symb.rowptr[k]:symb.rowptr[k + 1]].max(), 1e-300))
                for k in range(symb.Nsn)))
        entry["kernels_of_one_clique_eigvalsh_pencil"] = kernel_ms(symb, calls["clique_eigvalsh_pencil"])
        res["settings"][str(s)] = entry
        print("%s pencil setting %d: %s" % (name, s, json.dumps(entry)), flush=True)
    for rep in range(reps):
        for s in settings:
            chordal.tune(symb, chordal.TUNE_CEIG_WIDE, s)
            for c, f in calls.items():
                times[s][c].append(wall(f)[0])
        print("%s pencil repetition %d done" % (name, rep), flush=True)
    chordal.tune(symb, chordal.TUNE_CEIG_WIDE, 0)
    for s in settings:
        for c in calls:
            res["settings"][str(s)][c] = stats(times[s][c])
        print("%s pencil setting %d: " % (name, s) + ", ".join("%s %.2f ms (%.2f - %.2f)" % (
            c, res["settings"][str(s)][c]["median_ms"], min(times[s][c]), max(times[s][c])) for c in calls), flush=True)
    return res


def run(name, reps, settings):
    symb, X = make(name)
    nf = np.diff(symb.rowptr)
    res = {"case": name, "n": symb.n, "nsn": symb.Nsn, "widest_clique": int(nf.max()), "reps": reps, "settings": {}}
    times = {s: {c: [] for c in CALLS} for s in settings}
    w0 = None
    for s in settings:                                                    # first calls: buffers, and what does not change
        chordal.tune(symb, chordal.TUNE_CEIG_WIDE, s)
        first = {c: wall(lambda: f(X))[0] for c, f in CALLS.items()}
        w = chordal.clique_eigvalsh(X)
        entry = {"wide_cliques": chordal.clique_eig_wide(symb), "most_sweeps": chordal.clique_eig_sweeps(symb), "first_call_ms": first}
        if s == 0:
            w0 = w
        elif w0 is not None:
            d = (w - w0).abs().cpu().numpy()
            a = w0.abs().cpu().numpy()
            entry["w_against_setting_0_units"] = float(max(
                d[symb.rowptr[k]:symb.rowptr[k + 1]].max() / (nf[k] * np.finfo(float).eps * max(a[symb.rowptr[k]:symb.rowptr[k + 1]].max(), 1e-300))
                for k in range(symb.Nsn)))
        entry["kernels_of_one_clique_project"] = kernel_ms(symb, lambda: chordal.clique_project(X))
        res["settings"][str(s)] = entry
        print("%s setting %d: %s" % (name, s, json.dumps(entry)), flush=True)
    for rep in range(reps):
        for s in settings:
            chordal.tune(symb, chordal.TUNE_CEIG_WIDE, s)
            for c, f in CALLS.items():
                times[s][c].append(wall(lambda: f(X))[0])
        print("%s repetition %d done" % (name, rep), flush=True)
    chordal.tune(symb, chordal.TUNE_CEIG_WIDE, 0)
    for s in settings:
        for c in CALLS:
            res["settings"][str(s)][c] = stats(times[s][c])
        print("%s setting %d: " % (name, s) + ", ".join("%s %.2f ms (%.2f - %.2f)" % (
            c, res["settings"][str(s)][c]["median_ms"], min(times[s][c]), max(times[s][c])) for c in CALLS), flush=True)
    try:
        lists = block_lists(symb, name in DENSE)
        wall(lambda: baseline(symb, X, lists, name in DENSE, 0.0, float("inf")))
        t_old = [wall(lambda: baseline(symb, X, lists, name in DENSE, 0.0, float("inf")))[0] for _ in range(reps)]
        res["torch_eigh_clip_multiply"] = stats(t_old)
        print("%s: torch.linalg.eigh on the blocks, clip, multiply back: %.2f ms (%.2f - %.2f)"
              % (name, res["torch_eigh_clip_multiply"]["median_ms"], min(t_old), max(t_old)), flush=True)
    except Exception as e:
        res["baseline_error"] = repr(e)
        print("%s: baseline failed: %r" % (name, e), flush=True)
    return res


def take(args, flag, default):
    if flag in args:
        i = args.index(flag)
        v = args[i + 1]
        del args[i:i + 2]
        return v
    return default


if __name__ == "__main__":
    args = sys.argv[1:]
    reps = int(take(args, "--reps", 5))
    out = take(args, "--out", None)
    pencil = "--pencil" in args
    if pencil:
        args.remove("--pencil")
        out = out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pencil_wide_bench.json")
    chosen = take(args, "--settings", None)
    settings = [int(v) for v in (chosen or ",".join(map(str, SETTINGS))).split(",")]
    once = take(args, "--once", None)
    torch.cuda.set_device(0)
    if once is not None and pencil:
        for name in (args or ["config4"]):
            symb, A, B, D = make_pencil(name)
            chordal.tune(symb, chordal.TUNE_CEIG_WIDE, int(once))
            t1 = wall(lambda: chordal.clique_eigvalsh(A, B))[0]
            t2 = wall(lambda: chordal.clique_eigvalsh(A, B))[0]
            print("%s setting %s: clique_eigvalsh(A, B) %.2f ms, then %.2f ms; %d wide cliques, %d sweeps at most"
                  % (name, once, t1, t2, chordal.clique_eig_wide(symb), chordal.clique_eig_sweeps(symb)), flush=True)
        sys.exit(0)
    if once is not None:
        for name in (args or ["config4"]):
            symb, X = make(name)
            chordal.tune(symb, chordal.TUNE_CEIG_WIDE, int(once))
            t1 = wall(lambda: chordal.clique_project(X))[0]
            t2 = wall(lambda: chordal.clique_project(X))[0]
            print("%s setting %s: clique_project %.2f ms, then %.2f ms; %d wide cliques, %d sweeps at most"
                  % (name, once, t1, t2, chordal.clique_eig_wide(symb), chordal.clique_eig_sweeps(symb)), flush=True)
        sys.exit(0)
    results = []
    for name in (args or ["config4", "synth50k"]):
        if pencil:
            results.append(run_pencil(name, reps, settings if chosen else PENCIL_SETTINGS.get(name, [0, 65])))
        else:
            results.append(run(name, reps, settings))
        if out:
            with open(out, "w") as f:
                json.dump(results, f, indent=1)
                f.write("\n")
