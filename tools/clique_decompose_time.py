"""Time chordal.clique_decompose on one MI355X on its two routes -- the default one (tile products for
the large fronts, the FMA kernel for the rest) and the deterministic one (TUNE_DETERMINISTIC: the FMA kernel for every
front) -- against what there was before it: torch.matmul on the masked panel views of L.blkval, batched by (nf, nn) shape
(per shape one gather of the panels through a prebuilt index, one mask, one batched matmul and one indexed store into the
packed tensor).  Patterns: synth50k (n = 50 000, 8073 cliques) and the max-cut pattern of config 4 (n = 1000, a 548-row
root).  Device events around one call, one warm call of each route first, then the three routes alternated call by call in
one process; median of seven with min and max.  Per case also the launches of one call of either device route with the time
of every kernel (csp_profile_*; the kernels run under the borrowed names k_syr2k_fma and k_syr2k_mm), the bytes the call
must move, 8 (blklen + qlen), over the time of each route, and the largest difference between the baseline and the call.

    python tools/clique_decompose_time.py [--out FILE.json] [case ...]      cases: synth50k maxcut   (default: both)
"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from smcp_amd import chordal
from tools.trmm_time import CASES, HBM_PEAK, factor_input, launches, timed

REPS = 7
BASELINE = "torch.matmul on the masked panel views of L.blkval, batched by (nf, nn) shape"


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def shape_groups(symb):
    """per (nf, nn) shape: the offsets in blkval of the panels of its cliques (b x nn nf), the offsets of their blocks in the
    packed tensor (b x nf nf) and the mask of the owned slots of a panel (nn x nf: row c, column m, m >= c), on the device"""
    blkptr, q = np.asarray(symb.blkptr), chordal.clique_ptr(symb)
    nn, na = symb.clique_sizes()
    by = {}
    for k in range(symb.Nsn):
        by.setdefault((int(nn[k] + na[k]), int(nn[k])), []).append(k)
    out = []
    for (nf, n1), ks in sorted(by.items()):
        ks = np.asarray(ks)
        pidx = torch.from_numpy(blkptr[ks][:, None] + np.arange(nf * n1)[None, :]).cuda()
        qidx = torch.from_numpy(q[ks][:, None] + np.arange(nf * nf)[None, :]).cuda()
        mask = torch.from_numpy(np.arange(nf)[None, :] >= np.arange(n1)[:, None]).cuda()
        out.append((nf, n1, pidx, qidx, mask))
    return out


def baseline(groups, blkval, Z):
    zero = torch.zeros((), dtype=torch.float64, device=blkval.device)
    for nf, n1, pidx, qidx, mask in groups:
        PT = torch.where(mask, blkval[pidx].view(-1, n1, nf), zero)              # PT[b, c, m] = Pt[m, c]
        Z[qidx] = torch.matmul(PT.transpose(1, 2), PT).reshape(-1, nf * nf)


def run(name):
    symb = CASES[name]()
    symb.device_init(0, 1)
    L = factor_input(symb)
    q = chordal.clique_ptr(symb)
    qlen, blklen = int(q[-1]), int(symb.blklen)
    Z = {r: torch.empty(qlen, dtype=torch.float64, device="cuda") for r in ("default", "deterministic", "baseline")}
    groups = shape_groups(symb)

    def device_route(det):
        def call():
            chordal.clique_decompose(L, out=Z["deterministic" if det else "default"])
        return call

    def with_tune(det, f):
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, det)
        try:
            return f()
        finally:
            chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 0)

    routes = {"default": lambda f: with_tune(0, lambda: f(device_route(0))),
              "deterministic": lambda f: with_tune(1, lambda: f(device_route(1))),
              "baseline": lambda f: f(lambda: baseline(groups, L.blkval, Z["baseline"]))}
    for r in routes:                                                 # warm: the plan is built and uploaded here
        routes[r](lambda call: call())
    t = {r: [] for r in routes}
    for _ in range(REPS):
        for r in routes:
            t[r].append(routes[r](timed))
    nbytes = 8 * (blklen + qlen)
    nn, na = symb.clique_sizes()
    out = {"case": name, "n": int(symb.n), "cliques": int(symb.Nsn), "widest_front": int((nn + na).max()), "shapes": len(groups),
           "blklen": blklen, "qlen": qlen, "bytes_to_move": nbytes, "baseline": BASELINE, "routes": {}}
    for r in routes:
        rec = {"ms": stats(t[r])}
        rec["bytes_per_second"] = nbytes / (1e-3 * rec["ms"]["median"])
        rec["fraction_of_hbm_peak"] = rec["bytes_per_second"] / HBM_PEAK
        if r != "baseline":
            lch = routes[r](lambda call: launches(symb, call))
            rec["launches"] = {k: v[0] for k, v in lch.items()}
            rec["kernel_ms"] = {k: round(v[1], 4) for k, v in lch.items()}
        out["routes"][r] = rec
        print("%s %s: %.4f ms (min %.4f max %.4f), %.1f GB/s = %.1f %% of the HBM peak%s"
              % (name, r, rec["ms"]["median"], rec["ms"]["min"], rec["ms"]["max"], 1e-9 * rec["bytes_per_second"], 100 * rec["fraction_of_hbm_peak"],
                 "; launches %s, kernel ms %s" % (rec["launches"], rec["kernel_ms"]) if r != "baseline" else ""), flush=True)
    out["baseline_over_default"] = out["routes"]["baseline"]["ms"]["median"] / out["routes"]["default"]["ms"]["median"]
    out["deterministic_over_default"] = out["routes"]["deterministic"]["ms"]["median"] / out["routes"]["default"]["ms"]["median"]
    out["max_abs_baseline_minus_default"] = float((Z["baseline"] - Z["default"]).abs().max())
    out["max_abs_deterministic_minus_default"] = float((Z["deterministic"] - Z["default"]).abs().max())
    print("%s: baseline / default %.2f, deterministic / default %.2f; |baseline - default| <= %.3g, |deterministic - default| <= %.3g"
          % (name, out["baseline_over_default"], out["deterministic_over_default"], out["max_abs_baseline_minus_default"],
             out["max_abs_deterministic_minus_default"]), flush=True)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if len(args) >= 2 and args[0] == "--out":
        out, args = args[1], args[2:]
    torch.cuda.set_device(0)
    res = {"what": ("tools/clique_decompose_time.py: chordal.clique_decompose on its default and its deterministic route against the "
                    "baseline (%s) on one MI355X, device events, the three routes alternated in one process, median of %d warm calls "
                    "(min, max); kernel_ms: events around each launch (csp_profile_*), under the borrowed kernel names" % (BASELINE, REPS)),
           "cases": [run(name) for name in (args or ["synth50k", "maxcut"])]}
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
