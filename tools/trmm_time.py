"""Time chordal.trmm against chordal.trsm on the same factor, the same shape of B and the same trans,
with the inverse-form factor cache of trsm warm (the favourable case for trsm).  Device part only (events), the two calls
alternated in one process, median of five warm calls each.  Per case also: the error against L.spmatrix() @ B (scipy
sparse, the full-size check), the launches of one call of each (csp_profile_*), for nrhs = 1 the bytes of L against the HBM
peak and for nrhs = 100 the useful flops 2 nnz(L) nrhs against the fp64 MFMA peak.

    python tools/trmm_time.py [--out FILE.json] [case ...]      cases: synth50k arrow_big dense4096 maxcut   (default: all)
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import scipy.sparse as sp
import torch

from smcp_amd import _lib, base, chordal, problems
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic

MFMA_PEAK, HBM_PEAK = 78.6e12, 8.0e12
NRHS = (1, 8, 100)


def factor_input(symb, seed=6):
    """L lower on V, off-diagonal entries of column j scaled by 0.5 / sqrt(their number), diagonal 1 + random (the scaling of
    tools/psd_time.py: pd_input); zeros above the diagonals of the diagonal blocks (csp_trsm's inverse-form factor reads them)."""
    rng = np.random.default_rng(seed)
    cp, ri = symb.sparsity_pattern()
    cnt = np.maximum(np.diff(cp) - 1, 1)
    J = np.repeat(np.arange(symb.n), np.diff(cp))
    v = rng.standard_normal(len(ri)) * (0.5 / np.sqrt(cnt))[J]
    v[cp[:-1]] = 1.0 + rng.random(symb.n)
    blk = np.zeros(symb.blklen)
    blk[symb.ccs_to_blk()] = v
    return cspmatrix(symb, torch.from_numpy(blk).cuda())


def maxcut_symbolic():
    """the pattern of the config-4 max-cut problem, embedded as base.psdcompletion embeds it"""
    C = base.maxcut_SDP(1000, 5909, seed=0).get_A(0)
    return base._on_pattern(sp.csc_matrix(C))[0].symb


CASES = {
    "synth50k": lambda: Symbolic(problems.nested_block_arrow_pattern(seed=0)),
    "arrow_big": lambda: Symbolic(problems.block_arrow_pattern(12, 64, 128)),
    "dense4096": lambda: Symbolic(problems.band_pattern(4096, 4095)),
    "maxcut": maxcut_symbolic,
}


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launches(symb, fn):
    """kernel name -> (launches, ms between the events around them) of one call of fn"""
    lib = _lib.lib()
    h = symb.handle
    nk = int(lib.csp_profile_kinds())
    lib.csp_profile_filter(h, -1)
    lib.csp_profile_enable(h, 1)
    lib.csp_profile_read(h, None, None)
    try:
        fn()
        torch.cuda.synchronize()
        ms = (ctypes.c_double * nk)()
        cnt = (ctypes.c_int64 * nk)()
        lib.csp_profile_read(h, ms, cnt)
    finally:
        lib.csp_profile_enable(h, 0)
    return {lib.csp_profile_kernel_name(i).decode(): (int(cnt[i]), float(ms[i])) for i in range(nk) if cnt[i]}


def run(name):
    symb = CASES[name]()
    if symb._device is None:
        symb.device_init(0, 1)
    L = factor_input(symb)
    Ls = L.spmatrix()
    n, nnz = symb.n, symb.nnz
    recs = []
    for nrhs in NRHS:
        B0 = torch.from_numpy(np.random.default_rng(nrhs).standard_normal((nrhs, n))).cuda()
        B = B0.clone()
        for trans in ("N", "T"):
            B.copy_(B0)
            chordal.trmm(L, B, 1.0, trans)                        # warm: workspaces, index tables
            ref = ((Ls.T if trans == "T" else Ls) @ B0.cpu().numpy().T).T
            err = float(np.abs(B.cpu().numpy() - ref).max() / np.abs(ref).max())
            B.copy_(B0)
            chordal.trsm(L, B, trans)                             # warm: the inverse-form factor of L
            t_mm, t_sm = [], []
            for _ in range(5):
                B.copy_(B0)
                t_mm.append(timed(lambda: chordal.trmm(L, B, 1.0, trans)))
                B.copy_(B0)
                t_sm.append(timed(lambda: chordal.trsm(L, B, trans)))
            B.copy_(B0)
            l_mm = launches(symb, lambda: chordal.trmm(L, B, 1.0, trans))
            B.copy_(B0)
            l_sm = launches(symb, lambda: chordal.trsm(L, B, trans))
            m_mm, m_sm = float(np.median(t_mm)), float(np.median(t_sm))
            rec = {"case": name, "n": int(n), "Nsn": int(symb.Nsn), "levels": int(symb.nlev), "nnz_L": int(nnz), "nrhs": nrhs,
                   "trans": trans, "trmm_ms": {"median": m_mm, "min": min(t_mm), "max": max(t_mm)},
                   "trsm_ms": {"median": m_sm, "min": min(t_sm), "max": max(t_sm)}, "trmm_over_trsm": m_mm / m_sm,
                   "trmm_launches": {k: v[0] for k, v in l_mm.items()}, "trmm_kernel_ms": {k: round(v[1], 4) for k, v in l_mm.items()},
                   "trsm_launches": sum(v[0] for v in l_sm.values()), "rel_err_vs_scipy_sparse": err}
            line = ("%s nrhs %d trans %s: trmm %.4f ms (min %.4f max %.4f, %d launches), trsm %.4f ms (min %.4f max %.4f, %d launches), "
                    "ratio %.3f, error against L.spmatrix() @ B %.1e" % (name, nrhs, trans, m_mm, min(t_mm), max(t_mm), sum(v[0] for v in l_mm.values()),
                                                                          m_sm, min(t_sm), max(t_sm), sum(v[0] for v in l_sm.values()), m_mm / m_sm, err))
            line += "; trmm kernels (ms): " + ", ".join("%s %.4f" % (k, v[1]) for k, v in l_mm.items())
            line += "; trsm kernels (ms): " + ", ".join("%s x %d %.4f" % (k, v[0], v[1]) for k, v in l_sm.items())
            if nrhs == 1:
                rec["L_bytes"] = 8 * int(nnz)
                rec["fraction_of_hbm_peak"] = 8.0 * nnz / (m_mm * 1e-3) / HBM_PEAK
                line += "; %.1f MB of L = %.4f of the HBM peak" % (8.0 * nnz / 1e6, rec["fraction_of_hbm_peak"])
            if nrhs == 100:
                rec["useful_flops"] = 2 * int(nnz) * nrhs
                rec["fraction_of_mfma_peak"] = 2.0 * nnz * nrhs / (m_mm * 1e-3) / MFMA_PEAK
                line += "; %.3f Gflop = %.4f of the fp64 MFMA peak" % (2.0 * nnz * nrhs / 1e9, rec["fraction_of_mfma_peak"])
            print(line, flush=True)
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
            json.dump({"what": "tools/trmm_time.py: chordal.trmm against chordal.trsm (inverse-form factor cache warm) on one MI355X, "
                               "device events, the two alternated in one process, median of five warm calls",
                       "records": records}, f, indent=1)
