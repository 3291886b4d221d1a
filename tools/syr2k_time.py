"""Time chordal.syr2k / chordal.syrk on one MI355X: device events, warm calls, medians, the three
settings of SMCP_SYR2K_MM (0: FMA kernel only, 1: the default gate, 2: tile products for the large fronts only) alternated
call by call in one process (the library reads that switch on every call).  Two comparisons per case:
  - a torch restatement that needs nothing of this library's kernels: per clique, index_select of the front rows and two addmm
    into the panel view of blkval (it also writes the slots above the diagonals; it is a timing comparison only);
  - the traffic floor: 16 blklen bytes for X (read and written once) plus 8 k sum(nf) bytes per dense block read (one for
    syrk, two for syr2k), at the HBM rate of bench.py's roofline.
Per case also the largest difference between the two on the pattern (relative to the largest entry) and the launches of one call.

    python tools/syr2k_time.py [--out FILE.json] [case ...]      cases: synth50k arrow2000 dense4096 maxcut   (default: all)
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

HBM_PEAK = 8.0e12          # bench.py: HBM_PEAK_GBS
RANKS = (1, 4, 8, 16, 32, 64, 128)
MODES = ("0", "1", "2")
REPS, TORCH_REPS = 7, 3


def maxcut_symbolic():
    """the pattern of the config-4 max-cut problem, embedded as base.psdcompletion embeds it"""
    C = base.maxcut_SDP(1000, 5909, seed=0).get_A(0)
    return base._on_pattern(sp.csc_matrix(C))[0].symb


CASES = {
    "synth50k": lambda: Symbolic(problems.nested_block_arrow_pattern(seed=0)),
    "arrow2000": lambda: Symbolic(problems.block_arrow_pattern(2000, 64, 128)),
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
    """kernel name -> launches of one call of fn (csp_profile_*)"""
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
    return {lib.csp_profile_kernel_name(i).decode(): int(cnt[i]) for i in range(nk) if cnt[i]}


class TorchRestatement:
    """per clique: panel^T (nn x nf, the row-major view of the column-major panel) <- beta panel^T + alpha (V_N^T U_F + U_N^T V_F)"""

    def __init__(self, symb):
        self.symb = symb
        ri = torch.from_numpy(np.asarray(symb.rowidx, dtype=np.int64)).cuda()
        self.cl = []
        for c in range(symb.Nsn):
            nn = int(symb.snptr[c + 1] - symb.snptr[c])
            r0, r1 = int(symb.rowptr[c]), int(symb.rowptr[c + 1])
            self.cl.append((int(symb.blkptr[c]), nn, r1 - r0, int(symb.snptr[c]), ri[r0:r1]))

    def __call__(self, X, U, V, alpha, beta):
        blk = X.blkval
        for b, nn, nf, first, F in self.cl:
            P = blk[b:b + nn * nf].view(nn, nf)
            UF = U.index_select(1, F)
            UN = U[:, first:first + nn]
            if V is None:
                P.addmm_(UN.t(), UF, beta=beta, alpha=alpha)
            else:
                VF = V.index_select(1, F)
                P.addmm_(V[:, first:first + nn].t(), UF, beta=beta, alpha=alpha)
                P.addmm_(UN.t(), VF, beta=1.0, alpha=alpha)


def run(name):
    symb = CASES[name]()
    if symb._device is None:
        symb.device_init(0, 1)
    n = symb.n
    own = np.zeros(symb.blklen, dtype=bool)
    own[symb.ccs_to_blk()] = True
    own_d = torch.from_numpy(own).cuda()
    X0 = torch.from_numpy(np.where(own, np.random.default_rng(1).standard_normal(symb.blklen), 0.0)).cuda()
    sum_nf = int(symb.rowptr[symb.Nsn])
    restate = TorchRestatement(symb)
    alpha, beta = 0.5, 1.0
    recs = []
    for k in RANKS:
        U = torch.from_numpy(np.random.default_rng(k).standard_normal((k, n))).cuda()
        V = torch.from_numpy(np.random.default_rng(1000 + k).standard_normal((k, n))).cuda()
        for form in ("syr2k", "syrk"):
            Vf = V if form == "syr2k" else None

            def ours(X):
                if Vf is None:
                    chordal.syrk(X, U, alpha, beta)
                else:
                    chordal.syr2k(X, U, Vf, alpha, beta)

            X = cspmatrix(symb, X0.clone())
            Xt = cspmatrix(symb, X0.clone())
            restate(Xt, U, Vf, alpha, beta)                          # warm, and the values of the check below
            results = {}
            for mode in MODES:                                       # warm every route, keep its result
                os.environ["SMCP_SYR2K_MM"] = mode
                X.blkval.copy_(X0)
                ours(X)
                results[mode] = X.blkval.clone()
            scale = float(Xt.blkval[own_d].abs().max())
            err = {m: float((results[m][own_d] - Xt.blkval[own_d]).abs().max()) / scale for m in MODES}
            t = {m: [] for m in MODES}
            for _ in range(REPS):
                for mode in MODES:                                   # alternated call by call
                    os.environ["SMCP_SYR2K_MM"] = mode
                    t[mode].append(timed(lambda: ours(X)))
            t_torch = [timed(lambda: restate(Xt, U, Vf, alpha, beta)) for _ in range(TORCH_REPS)]
            ln = {}
            for mode in MODES:
                os.environ["SMCP_SYR2K_MM"] = mode
                ln[mode] = launches(symb, lambda: ours(X))
            os.environ["SMCP_SYR2K_MM"] = "1"
            floor_bytes = 16 * symb.blklen + 8 * k * sum_nf * (2 if Vf is not None else 1)
            floor_ms = floor_bytes / HBM_PEAK * 1e3
            med = {m: float(np.median(t[m])) for m in MODES}
            m_torch = float(np.median(t_torch))
            rec = {"case": name, "n": int(n), "Nsn": int(symb.Nsn), "levels": int(symb.nlev), "blklen": int(symb.blklen), "sum_nf": sum_nf,
                   "k": k, "form": form,
                   "ms": {m: {"median": med[m], "min": min(t[m]), "max": max(t[m])} for m in MODES},
                   "launches": ln, "torch_ms": {"median": m_torch, "min": min(t_torch), "max": max(t_torch)},
                   "floor_bytes": int(floor_bytes), "floor_ms": floor_ms, "default_over_floor": med["1"] / floor_ms,
                   "torch_over_default": m_torch / med["1"], "max_diff_vs_torch_over_max_entry": err}
            print("%s k %d %s: MM=0 %.4f  MM=1 %.4f  MM=2 %.4f ms (default min %.4f max %.4f; launches %s); torch restatement %.3f ms "
                  "(%.1f x the default); traffic floor %.4f ms (%.1f MB; default = %.1f x floor); diff vs torch %.1e"
                  % (name, k, form, med["0"], med["1"], med["2"], min(t["1"]), max(t["1"]), ln["1"], m_torch, m_torch / med["1"],
                     floor_ms, floor_bytes / 1e6, med["1"] / floor_ms, max(err.values())), flush=True)
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
                json.dump({"what": "tools/syr2k_time.py: chordal.syr2k / syrk on one MI355X, device events, SMCP_SYR2K_MM = 0 / 1 / 2 alternated "
                                   "call by call in one process, median of %d warm calls; a per-clique torch restatement (median of %d) and the "
                                   "traffic floor at %.1f TB/s" % (REPS, TORCH_REPS, HBM_PEAK / 1e12),
                           "records": records}, f, indent=1)
