"""Time KKTSystem.solve_many_qr on one MI355X against k consecutive calls of the factor_qr closure on the
same factorisation, in one process: device events around the call(s), the two alternated, median of seven warm calls
(min - max; the spread of the repeats is the noise quoted with the table).  k = 1, 2, 4, 8, 16 on bench.py's workload builders
with tnzcols = 0 (every constraint swept, as kkt_qr needs): synth50k (m = 100) and dense4096 (m = 16) by default.  For k = 8
also the per-kernel split of one block call and of the eight single calls (csp_profile_*), and for the two products with Q the
achieved bytes/s over their algorithmic bytes ((m + c) * blklen doubles each: Q once and the block once; the write-back of the
second product and the partial sums of the first are not counted) as a share of the 8 TB/s HBM peak.

    python tools/solve_many_qr_time.py [--out FILE.json] [--profile-only K] [case ...]     cases: synth50k dense4096 arrow synth6k ...

--profile-only K: factor, warm up, then exactly one block call of K rows and nothing else -- the body of a
`rocprofv3 --kernel-trace --stats` run of its own.
"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import bench
from smcp_amd import chordal, problems
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.kkt import KKTSystem, solve_many_qr_chunks
from smcp_amd.symbolic import Symbolic
from tools.trmm_time import launches, timed

KS = (1, 2, 4, 8, 16)
REPEATS = 7
WORKLOADS = ("synth50k", "dense4096")
HBM_PEAK = 8.0e12
STACK = {"k_stack_dots_many": "Q^T r", "k_stack_comb_many": "Q x - r"}


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def setup(name):
    """the scaling point and constraints of bench.py's workload `name`, QR-factored once"""
    pat, m, density, label = bench.build_workload(name)
    symb = Symbolic(pat)
    cptr, cidx, cval = problems.random_constraints(symb, m, density=density, seed=1)
    fl = symb.flops()
    max_rhs = int(max(2, min(max(m, 16), (48 << 30) // (8 * (fl["U"] + 3 * fl["B"])))))
    kkt = KKTSystem(symb, cptr, cidx, cval, max_rhs=max_rhs, tnzcols=0.0)
    S = cspmatrix(symb, torch.from_numpy(problems.random_factor_blkval(symb, seed=0)).cuda())
    chordal.llt(S)
    L, Y = S.copy(), S.copy()
    chordal.cholesky_projected_inverse(L, Y)
    solve = kkt.factor_qr(L, Y)
    msk = np.zeros(symb.blklen, dtype=bool)
    msk[symb.ccs_to_blk()] = True
    return symb, kkt, L, Y, solve, msk, m, label


def run_workload(name, profile_only=0):
    symb, kkt, L, Y, solve, msk, m, label = setup(name)
    bl = symb.blklen
    mskd = torch.from_numpy(msk).cuda()
    rng = np.random.default_rng(2)
    recs = []
    for k in ((profile_only,) if profile_only else KS):
        BX0 = torch.from_numpy(rng.standard_normal((k, bl)) * msk).cuda()
        BY0 = torch.from_numpy(rng.standard_normal((k, m))).cuda()
        BX, BY = BX0.clone(), BY0.clone()
        rows = [(cspmatrix(symb, BX0[r].clone()), BY0[r].clone()) for r in range(k)]

        def many():
            kkt.solve_many_qr(L, Y, BX, BY, 1.0)

        def singles():
            for bx, by in rows:
                solve(bx, by, 1.0)

        def reset():
            BX.copy_(BX0)
            BY.copy_(BY0)
            for r, (bx, by) in enumerate(rows):
                bx.blkval.copy_(BX0[r])
                by.copy_(BY0[r])

        many()
        if profile_only:
            reset()
            torch.cuda.synchronize()
            many()
            torch.cuda.synchronize()
            print("%s: one block call of %d rows after the warm-up (chunks %s)" % (name, k, solve_many_qr_chunks(k, symb._max_rhs)))
            return []
        singles()                                                   # warm; and the two routes must agree
        diff = max(float(torch.linalg.norm((BX[r] - rows[r][0].blkval)[mskd]) / torch.linalg.norm(rows[r][0].blkval[mskd])) for r in range(k))
        diffy = max(float(torch.linalg.norm(BY[r] - rows[r][1]) / torch.linalg.norm(rows[r][1])) for r in range(k))
        t_many, t_single = [], []
        for _ in range(REPEATS):
            reset()
            t_many.append(timed(many))
            t_single.append(timed(singles))
        chunks = solve_many_qr_chunks(k, symb._max_rhs)
        rec = {"case": name, "label": label, "m": int(m), "blklen": int(bl), "max_rhs": int(symb._max_rhs), "k": k, "chunks": chunks,
               "qr_passes": int(kkt.qr_passes), "solve_many_qr_ms": stats(t_many), "k_singles_ms": stats(t_single),
               "ratio": float(np.median(t_many) / np.median(t_single)),
               "block_faster_by_more_than_the_spread": bool(max(t_many) < min(t_single)),
               "rel_diff_x_many_vs_single": diff, "rel_diff_y_many_vs_single": diffy}
        line = ("%s k %d: solve_many_qr %.4f ms (min %.4f max %.4f), %d x solve_ %.4f ms (min %.4f max %.4f), ratio %.3f, chunks %s, "
                "x / y of the two routes differ by %.1e / %.1e"
                % (name, k, rec["solve_many_qr_ms"]["median"], min(t_many), max(t_many), k, rec["k_singles_ms"]["median"], min(t_single),
                   max(t_single), rec["ratio"], chunks, diff, diffy))
        if k == 8:
            reset()
            lm = launches(symb, many)
            reset()
            ls = launches(symb, singles)
            rec["many_kernels"] = {n: {"launches": v[0], "ms": round(v[1], 4)} for n, v in lm.items()}
            rec["singles_kernels"] = {n: {"launches": v[0], "ms": round(v[1], 4)} for n, v in ls.items()}
            rec["stack_kernels"] = {}
            for n, what in STACK.items():
                if n in lm and lm[n][1] > 0:
                    nbytes = 8.0 * sum((m + c) * bl for c in chunks)
                    bps = nbytes / (lm[n][1] * 1e-3)
                    rec["stack_kernels"][n] = {"what": what, "algorithmic_bytes": nbytes, "ms": lm[n][1], "bytes_per_s": bps,
                                               "share_of_8TBps": bps / HBM_PEAK}
            line += ("; kernels of the block call (launches, ms between events): "
                     + ", ".join("%s x %d %.4f" % (n, v["launches"], v["ms"]) for n, v in rec["many_kernels"].items())
                     + "; of the eight single calls: " + ", ".join("%s x %d %.4f" % (n, v["launches"], v["ms"]) for n, v in rec["singles_kernels"].items())
                     + "; products with Q: " + ", ".join("%s %.3g B/s = %.0f %% of 8 TB/s" % (n, v["bytes_per_s"], 100 * v["share_of_8TBps"])
                                                         for n, v in rec["stack_kernels"].items()))
        print(line, flush=True)
        recs.append(rec)
    return recs


if __name__ == "__main__":
    args = sys.argv[1:]
    out, profile_only = None, 0
    while args and args[0] in ("--out", "--profile-only"):
        if args[0] == "--out":
            out = args[1]
        else:
            profile_only = int(args[1])
        args = args[2:]
    torch.cuda.set_device(0)
    records = []
    for name in (args or list(WORKLOADS)):
        records += run_workload(name, profile_only)
    if out:
        with open(out, "w") as f:
            json.dump({"what": "tools/solve_many_qr_time.py: KKTSystem.solve_many_qr against k calls of the factor_qr closure on one MI355X, "
                               "device events, alternated in one process, median of seven warm calls",
                       "records": records}, f, indent=1)
