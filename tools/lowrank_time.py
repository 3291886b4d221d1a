"""Time LowRankFactor.solve and .trmm on one MI355X, n = 50 000 (the synth50k pattern), k = 16,
kb = 1 and 16: device events around one call, median of five warm calls (min - max), alternated call by call with
  * the same middle product written in torch, B + (T @ (W @ B.T)).T @ W: three library launches and their temporaries,
  * the trsm / trmm calls that surround the middle product, on their own.
Per case also the launches of one call with the time of every kernel (csp_profile_*), and the rate of the two new streaming
kernels (k_lr_gram + k_lr_apply) over the 8 n (2 k + 3 kb) bytes the pair moves: W twice, B read twice and written once.

    python tools/lowrank_time.py [--out FILE.json]
"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from smcp_amd import chordal
from tools.trmm_time import CASES, factor_input, launches, timed

K = 16
COLS = (1, 16)
HBM_PEAK = 8.0e12


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def run():
    symb = CASES["synth50k"]()
    symb.device_init(0, 1)
    L = factor_input(symb)
    n = symb.n
    V = torch.from_numpy(np.random.default_rng(1).standard_normal((K, n))).cuda()
    a = list(0.5 + np.random.default_rng(2).random(K))
    t_fac = []
    for _ in range(4):
        t_fac.append(timed(lambda: chordal.lowrank_factor(L, V, a)))
    lf = chordal.lowrank_factor(L, V, a)
    l_fac = launches(symb, lambda: chordal.lowrank_factor(L, V, a))
    k2 = K * K
    S = lf.state[8 + K + 3 * k2:8 + K + 4 * k2].reshape(K, K)       # the blocks of the state (include/smcp_amd.h)
    C = lf.state[8 + K + k2:8 + K + 2 * k2].reshape(K, K)
    recs = []
    print("lowrank_factor n %d k %d: %.4f ms warm (first call %.4f); launches %s"
          % (n, K, float(np.median(t_fac[1:])), t_fac[0], {k: v[0] for k, v in l_fac.items()}), flush=True)
    for kb in COLS:
        B0 = torch.from_numpy(np.random.default_rng(10 + kb).standard_normal((kb, n))).cuda()
        B = B0.clone()
        ops = {"solve": (lambda: lf.solve(B), S, lambda: (chordal.trsm(L, B, "N"), chordal.trsm(L, B, "T"))),
               "trmm": (lambda: lf.trmm(B), C, lambda: chordal.trmm(L, B, 1.0, "N"))}
        for op, (call, T, around) in ops.items():
            torch_mid = lambda: B + (T @ (lf.W @ B.T)).T @ lf.W
            for f in (call, torch_mid, around):                       # warm
                B.copy_(B0)
                f()
            t_op, t_torch, t_around = [], [], []
            for _ in range(5):
                B.copy_(B0)
                t_op.append(timed(call))
                B.copy_(B0)
                t_torch.append(timed(torch_mid))
                B.copy_(B0)
                t_around.append(timed(around))
            B.copy_(B0)
            lch = launches(symb, call)
            new_ms = lch["k_lr_gram"][1] + lch["k_lr_apply"][1]
            moved = 8 * n * (2 * K + 3 * kb)
            rec = {"n": int(n), "k": K, "kb": kb, "op": op, "call_ms": stats(t_op), "torch_middle_ms": stats(t_torch),
                   "surrounding_trsm_trmm_ms": stats(t_around),
                   "launches": {k: v[0] for k, v in lch.items()}, "kernel_ms": {k: round(v[1], 4) for k, v in lch.items()},
                   "pair_bytes": int(moved), "pair_ms": new_ms, "pair_GBps": moved / (new_ms * 1e-3) / 1e9,
                   "pair_fraction_of_hbm_peak": moved / (new_ms * 1e-3) / HBM_PEAK}
            print("%s kb %d: call %.4f ms (min %.4f max %.4f); torch middle product %.4f ms; surrounding trsm / trmm %.4f ms; "
                  "k_lr_gram %.4f + k_lr_apply %.4f ms = %.1f GB/s over %.1f MB; launches %s"
                  % (op, kb, rec["call_ms"]["median"], rec["call_ms"]["min"], rec["call_ms"]["max"], rec["torch_middle_ms"]["median"],
                     rec["surrounding_trsm_trmm_ms"]["median"], lch["k_lr_gram"][1], lch["k_lr_apply"][1], rec["pair_GBps"], moved / 1e6,
                     rec["launches"]), flush=True)
            recs.append(rec)
    return {"factor_ms": stats(t_fac[1:]), "factor_first_call_ms": t_fac[0], "factor_launches": {k: v[0] for k, v in l_fac.items()},
            "records": recs}


if __name__ == "__main__":
    args = sys.argv[1:]
    out = args[1] if len(args) == 2 and args[0] == "--out" else None
    torch.cuda.set_device(0)
    res = run()
    if out:
        res["what"] = ("tools/lowrank_time.py: LowRankFactor.solve / .trmm on one MI355X, synth50k pattern, k = 16, device events, the call, "
                       "the middle product in torch and the surrounding trsm / trmm alternated in one process, median of five warm calls; "
                       "kernel_ms: events around each launch (csp_profile_*)")
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
