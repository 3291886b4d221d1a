"""Time KKTSystem.residual_many and refine_many on one MI355X against what the drivers do today, in one
process: device events around the call(s), the two sides alternated, median of seven warm calls (min - max; the spread of the
repeats is the noise quoted with the table).  k = 1, 2, 4, 8, 16 on bench.py's workload builders, synth50k by default.

  residual:  residual_many with norms   against   k x (copy, chordal.hessian(inv=True), scale, aadj, add, subtract, amap,
             subtract, two chordal.dot) -- kkt_res of smcp_amd/solvers.py plus the two norms of the reference's DEBUG check
  refine:    refine_many(rounds=1, final=False)   against   k x solve_refined of smcp_amd/solvers.py (solve, kkt_res, solve,
             subtract) on the solve_ closure of the same factorisation

    python tools/kkt_residual_time.py [--out FILE.json] [case ...]     cases: synth50k dense4096 arrow synth6k ...
"""
import json
import math
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import bench
from smcp_amd import chordal, problems
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.kkt import KKTSystem
from smcp_amd.symbolic import Symbolic
from tools.trmm_time import launches, timed

KS = (1, 2, 4, 8, 16)
REPEATS = 7
WORKLOADS = ("synth50k",)


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def setup(name):
    """the scaling point and constraints of bench.py's workload `name`, factored once"""
    pat, m, density, label = bench.build_workload(name)
    symb = Symbolic(pat)
    cptr, cidx, cval = problems.random_constraints(symb, m, density=density, seed=1)
    fl = symb.flops()
    max_rhs = int(max(2, min(max(m, 16), (48 << 30) // (8 * (fl["U"] + 3 * fl["B"])))))
    kkt = KKTSystem(symb, cptr, cidx, cval, max_rhs=max_rhs)
    S = cspmatrix(symb, torch.from_numpy(problems.random_factor_blkval(symb, seed=0)).cuda())
    chordal.llt(S)
    L, Y = S.copy(), S.copy()
    chordal.cholesky_projected_inverse(L, Y)
    solve = kkt.factor(L, Y)
    msk = np.zeros(symb.blklen, dtype=bool)
    msk[symb.ccs_to_blk()] = True
    return symb, kkt, L, Y, solve, msk, m, label


def run_workload(name):
    symb, kkt, L, Y, solve, msk, m, label = setup(name)
    bl = symb.blklen
    kk = 1.0
    rng = np.random.default_rng(2)
    recs = []

    def kkt_res(x, yy, bx, by):
        r = x.copy()
        chordal.hessian(L, Y, r, adj=None, inv=True)
        r *= -kk
        r += kkt.aadj(yy)
        r -= bx
        return r, kkt.amap(x) - by

    for k in KS:
        XS = torch.from_numpy(rng.standard_normal((k, bl)) * msk).cuda()
        YS = torch.from_numpy(rng.standard_normal((k, m))).cuda()
        BX0 = torch.from_numpy(rng.standard_normal((k, bl)) * msk).cuda()
        BY0 = torch.from_numpy(rng.standard_normal((k, m))).cuda()
        RX, RY = torch.empty_like(XS), torch.empty_like(YS)
        norms = torch.empty((k, 4), dtype=torch.float64, device="cuda")
        BX, BY = BX0.clone(), BY0.clone()
        xs = [(cspmatrix(symb, XS[r].clone()), YS[r].clone()) for r in range(k)]
        bs = [(cspmatrix(symb, BX0[r].clone()), BY0[r].clone()) for r in range(k)]
        host = np.zeros((k, 4))

        def res_many():
            kkt.residual_many(L, Y, XS, YS, BX0, BY0, kk, RX, RY, norms)

        def res_singles():
            for r in range(k):
                r1, r2 = kkt_res(xs[r][0], xs[r][1], bs[r][0], bs[r][1])
                host[r] = (math.sqrt(max(chordal.dot(r1, r1), 0.0)), float(torch.linalg.norm(r2)),
                           math.sqrt(max(chordal.dot(bs[r][0], bs[r][0]), 0.0)), float(torch.linalg.norm(bs[r][1])))

        def ref_many():
            kkt.refine_many(L, Y, BX, BY, kk, rounds=1, final=False)

        out = [None] * k

        def ref_singles():
            for r in range(k):
                bx, by = bs[r]
                x, yy = bx.copy(), by.clone()
                solve(x, yy, kk)
                r1, r2 = kkt_res(x, yy, bx, by)
                solve(r1, r2, kk)
                x -= r1
                out[r] = (x, yy - r2)

        res_many()
        res_singles()                                              # warm; and the two sides must agree
        dn = float(np.abs(norms.cpu().numpy() / host - 1.0).max())
        ref_many()
        ref_singles()
        dx = max(float(torch.linalg.norm(BX[r] - out[r][0].blkval) / torch.linalg.norm(out[r][0].blkval)) for r in range(k))
        t = {"res_many": [], "res_singles": [], "ref_many": [], "ref_singles": []}
        for _ in range(REPEATS):
            t["res_many"].append(timed(res_many))
            t["res_singles"].append(timed(res_singles))
            BX.copy_(BX0)
            BY.copy_(BY0)
            t["ref_many"].append(timed(ref_many))
            t["ref_singles"].append(timed(ref_singles))
        rec = {"case": name, "label": label, "m": int(m), "blklen": int(bl), "max_rhs": int(symb._max_rhs), "k": k,
               "residual_many_ms": stats(t["res_many"]), "k_compositions_ms": stats(t["res_singles"]),
               "residual_ratio": float(np.median(t["res_many"]) / np.median(t["res_singles"])),
               "refine_many_ms": stats(t["ref_many"]), "k_solve_refined_ms": stats(t["ref_singles"]),
               "refine_ratio": float(np.median(t["ref_many"]) / np.median(t["ref_singles"])),
               "norms_rel_diff": dn, "refined_x_rel_diff": dx}
        line = ("%s k %d: residual_many %.4f ms (%.4f - %.4f), %d compositions %.4f ms (%.4f - %.4f), ratio %.3f; refine_many %.4f ms "
                "(%.4f - %.4f), %d solve_refined %.4f ms (%.4f - %.4f), ratio %.3f; norms differ by %.1e, refined x by %.1e"
                % (name, k, rec["residual_many_ms"]["median"], min(t["res_many"]), max(t["res_many"]), k, rec["k_compositions_ms"]["median"],
                   min(t["res_singles"]), max(t["res_singles"]), rec["residual_ratio"], rec["refine_many_ms"]["median"], min(t["ref_many"]),
                   max(t["ref_many"]), k, rec["k_solve_refined_ms"]["median"], min(t["ref_singles"]), max(t["ref_singles"]), rec["refine_ratio"], dn, dx))
        if k in (1, 8):
            lm = launches(symb, res_many)
            ls = launches(symb, res_singles)
            rec["residual_many_kernels"] = {n: {"launches": v[0], "ms": round(v[1], 4)} for n, v in lm.items()}
            rec["compositions_kernels"] = {n: {"launches": v[0], "ms": round(v[1], 4)} for n, v in ls.items()}
            line += ("; kernels of the block residual (launches, ms between events): "
                     + ", ".join("%s x %d %.4f" % (n, v["launches"], v["ms"]) for n, v in rec["residual_many_kernels"].items())
                     + "; of the compositions: " + ", ".join("%s x %d %.4f" % (n, v["launches"], v["ms"]) for n, v in rec["compositions_kernels"].items()))
        print(line, flush=True)
        recs.append(rec)
    return recs


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if args and args[0] == "--out":
        out = args[1]
        args = args[2:]
    torch.cuda.set_device(0)
    records = []
    for name in (args or list(WORKLOADS)):
        records += run_workload(name)
    if out:
        with open(out, "w") as f:
            json.dump({"what": "tools/kkt_residual_time.py: KKTSystem.residual_many (with norms) against k Python compositions of kkt_res with "
                               "two dots, and refine_many(rounds=1, final=False) against k solve_refined, on one MI355X, device events, "
                               "alternated in one process, median of seven warm calls",
                       "records": records}, f, indent=1)
