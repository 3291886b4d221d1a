"""Time chordal.symm on one MI355X: device events around one call, median of five warm calls
(min - max), the three settings of SMCP_SYMM_MM (0: FMA kernel only, 1: the default gates, 2: tile products for the large
fronts only) alternated call by call in one process with the route that existed before symm: trmm 'N' plus trmm 'T' on the
same blkval (that route also needs two doctored copies of X and an add, which are NOT charged to it).  Per case also: the
error against X.spmatrix(symmetric=True) @ B (scipy sparse, the full-size check), the launches of one call (csp_profile_*)
and the distance from the traffic floor 8 blklen + 16 ntot nrhs + 16 n nrhs bytes at the HBM rate of bench.py's roofline.

    python tools/symm_time.py [--out FILE.json] [case ...]      cases: synth50k arrow_big dense4096 maxcut   (default: all)
"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from smcp_amd import _lib, chordal
from smcp_amd.cspmatrix import cspmatrix
from tools.trmm_time import CASES, launches, timed

HBM_PEAK = 8.0e12
NRHS = (1, 8, 100)
MODES = ("0", "1", "2")


def matrix_input(symb, seed=6):
    """a symmetric matrix with standard normal entries on the pattern, zeros in the slots of blkval outside it (trmm reads
    the same buffer as a factor)"""
    cp, ri = symb.sparsity_pattern()
    blk = np.zeros(symb.blklen)
    blk[symb.ccs_to_blk()] = np.random.default_rng(seed).standard_normal(len(ri))
    return cspmatrix(symb, torch.from_numpy(blk).cuda())


def run(name):
    symb = CASES[name]()
    if symb._device is None:
        symb.device_init(0, 1)
    X = matrix_input(symb)
    Xs = X.spmatrix(symmetric=True)
    n = symb.n
    ntot = int(_lib.lib().csp_symm_positions(symb.handle))
    recs = []
    for nrhs in NRHS:
        B = torch.from_numpy(np.random.default_rng(nrhs).standard_normal((nrhs, n))).cuda()
        C = torch.empty_like(B)
        T1, T2 = B.clone(), B.clone()
        ref = (Xs @ B.cpu().numpy().T).T
        t = {m: [] for m in MODES}
        t_old = []
        err, lch = {}, {}
        for m in MODES:                                           # warm: workspaces, index tables; the full-size check
            os.environ["SMCP_SYMM_MM"] = m
            chordal.symm(X, B, C)
            err[m] = float(np.abs(C.cpu().numpy() - ref).max() / np.abs(ref).max())
            lch[m] = launches(symb, lambda: chordal.symm(X, B, C))
        chordal.trmm(X, T1, 1.0, "N")
        chordal.trmm(X, T2, 1.0, "T")
        for _ in range(5):
            for m in MODES:
                os.environ["SMCP_SYMM_MM"] = m
                t[m].append(timed(lambda: chordal.symm(X, B, C)))
            T1.copy_(B)
            T2.copy_(B)
            t_old.append(timed(lambda: (chordal.trmm(X, T1, 1.0, "N"), chordal.trmm(X, T2, 1.0, "T"))))
        os.environ["SMCP_SYMM_MM"] = "1"
        floor_bytes = 8 * symb.blklen + 16 * ntot * nrhs + 16 * n * nrhs
        floor_ms = floor_bytes / HBM_PEAK * 1e3
        med = {m: float(np.median(t[m])) for m in MODES}
        m_old = float(np.median(t_old))
        rec = {"case": name, "n": int(n), "Nsn": int(symb.Nsn), "levels": int(symb.nlev), "blklen": int(symb.blklen), "positions": ntot,
               "nrhs": nrhs, "symm_ms": {m: {"median": med[m], "min": min(t[m]), "max": max(t[m])} for m in MODES},
               "two_trmm_ms": {"median": m_old, "min": min(t_old), "max": max(t_old)}, "symm_over_two_trmm": med["1"] / m_old,
               "launches": {m: {k: v[0] for k, v in lch[m].items()} for m in MODES},
               "kernel_ms": {m: {k: round(v[1], 4) for k, v in lch[m].items()} for m in MODES},
               "floor_bytes": int(floor_bytes), "floor_ms": floor_ms, "times_the_floor": med["1"] / floor_ms,
               "rel_err_vs_scipy_sparse": err}
        print("%s nrhs %d: symm MM=0 %.4f, MM=1 %.4f (min %.4f max %.4f), MM=2 %.4f ms; trmm N + trmm T %.4f ms (min %.4f max %.4f); "
              "ratio %.3f; floor %.4f ms (x %.1f); error against X.spmatrix() @ B %.1e; launches %s; kernels (ms) %s"
              % (name, nrhs, med["0"], med["1"], min(t["1"]), max(t["1"]), med["2"], m_old, min(t_old), max(t_old), med["1"] / m_old,
                 floor_ms, med["1"] / floor_ms, max(err.values()), rec["launches"]["1"], rec["kernel_ms"]), flush=True)
        recs.append(rec)
    return recs


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if args and args[0] == "--out":
        out, args = args[1], args[2:]
    torch.cuda.set_device(0)
    records = []
    for name in (args or list(CASES)):
        records += run(name)
    if out:
        with open(out, "w") as f:
            json.dump({"what": "tools/symm_time.py: chordal.symm on one MI355X, device events, SMCP_SYMM_MM = 0 / 1 / 2 and the pair "
                               "trmm N + trmm T alternated in one process, median of five warm calls",
                       "records": records}, f, indent=1)
