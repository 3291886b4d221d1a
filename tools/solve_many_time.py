"""Time KKTSystem.solve_many on one MI355X against k consecutive calls of the solve_ closure on the
same factorisation, in one process: device events around the call(s), the two alternated, median of seven warm calls
(min - max; the spread of the repeats is the noise quoted with the table).  k = 1, 2, 4, 8 on three of bench.py's workload
builders: synth50k (m = 100), maxcut (m = 1000), dense4096 (m = 16).  Also dense_potrs_many at n = 1000 and 4096 for the
same k against k calls of dense_potrs(nrhs = 1) and against itself with SMCP_POTRS_MANY_MM=0 (the updates on the FMA route
whatever k), and the per-kernel split of one k = 4 call (csp_profile_*).

    python tools/solve_many_time.py [--out FILE.json] [case ...]     cases: synth50k maxcut dense4096 potrs1000 potrs4096  (default: all)
"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import bench
from smcp_amd import _lib, chordal, problems
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.kkt import KKTSystem, solve_many_chunks
from smcp_amd.symbolic import Symbolic
from tools.trmm_time import launches, timed

KS = (1, 2, 4, 8)
REPEATS = 7
WORKLOADS = ("synth50k", "maxcut", "dense4096")


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def run_workload(name):
    """the scaling point and constraints of bench.py's workload `name`, factored once"""
    pat, m, density, label = bench.build_workload(name)
    if name == "maxcut":
        symb, cptr, cidx, cval = bench.maxcut_problem()
    else:
        symb = Symbolic(pat)
        cptr, cidx, cval = problems.random_constraints(symb, m, density=density, seed=1)
    fl = symb.flops()
    max_rhs = int(max(2, min(max(m, 16), (48 << 30) // (8 * (fl["U"] + 3 * fl["B"])))))
    kkt = KKTSystem(symb, cptr, cidx, cval, max_rhs=max_rhs)
    bl = symb.blklen
    S = cspmatrix(symb, torch.from_numpy(problems.random_factor_blkval(symb, seed=0)).cuda())
    chordal.llt(S)
    L, Y = S.copy(), S.copy()
    chordal.cholesky_projected_inverse(L, Y)
    solve = kkt.factor(L, Y)
    msk = np.zeros(bl, dtype=bool)
    msk[symb.ccs_to_blk()] = True
    rng = np.random.default_rng(2)
    recs = []
    for k in KS:
        BX0 = torch.from_numpy(rng.standard_normal((k, bl)) * msk).cuda()
        BY0 = torch.from_numpy(rng.standard_normal((k, m))).cuda()
        BX, BY = BX0.clone(), BY0.clone()
        rows = [(cspmatrix(symb, BX0[r].clone()), BY0[r].clone()) for r in range(k)]

        def many():
            kkt.solve_many(L, Y, BX, BY, 1.0)

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
        singles()                                                   # warm; and the two routes must agree
        diff = max(float(torch.linalg.norm((BX[r] - rows[r][0].blkval)[torch.from_numpy(msk).cuda()]) /
                         torch.linalg.norm(rows[r][0].blkval[torch.from_numpy(msk).cuda()])) for r in range(k))
        t_many, t_single = [], []
        for _ in range(REPEATS):
            reset()
            t_many.append(timed(many))
            t_single.append(timed(singles))
        rec = {"case": name, "label": label, "m": int(m), "blklen": int(bl), "max_rhs": int(symb._max_rhs), "k": k,
               "chunks": solve_many_chunks(k, m, bl, symb._max_rhs), "solve_many_ms": stats(t_many), "k_singles_ms": stats(t_single),
               "ratio": float(np.median(t_many) / np.median(t_single)), "rel_diff_x_many_vs_single": diff}
        if k == 4:
            reset()
            lm = launches(symb, many)
            reset()
            ls = launches(symb, singles)
            rec["many_kernels"] = {n: {"launches": v[0], "ms": round(v[1], 4)} for n, v in lm.items()}
            rec["singles_kernels"] = {n: {"launches": v[0], "ms": round(v[1], 4)} for n, v in ls.items()}
        print("%s k %d: solve_many %.4f ms (min %.4f max %.4f), %d x solve_ %.4f ms (min %.4f max %.4f), ratio %.3f, chunks %s, "
              "x of the two routes differ by %.1e%s"
              % (name, k, rec["solve_many_ms"]["median"], min(t_many), max(t_many), k, rec["k_singles_ms"]["median"], min(t_single),
                 max(t_single), rec["ratio"], rec["chunks"], diff,
                 ("; kernels of the block call (launches, ms): " + ", ".join("%s x %d %.4f" % (n, v["launches"], v["ms"])
                                                                              for n, v in rec["many_kernels"].items())) if k == 4 else ""),
              flush=True)
        recs.append(rec)
    return recs


def run_potrs(n):
    lib = _lib.lib()
    symb = Symbolic(problems.band_pattern(10, 2))
    chordal._ensure(symb)
    h = symb.handle
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n))
    Hh = M @ M.T + n * np.eye(n)
    H = torch.from_numpy(Hh).cuda()
    assert lib.dense_potrf(h, H.data_ptr(), n, n, None) == 0
    recs = []
    for k in KS:
        B0 = torch.from_numpy(rng.standard_normal((k, n))).cuda()
        B, C = B0.clone(), B0.clone()

        def many():
            assert lib.dense_potrs_many(h, H.data_ptr(), n, n, B.data_ptr(), k, n, None) == 0

        def singles():
            for r in range(k):
                assert lib.dense_potrs(h, H.data_ptr(), n, n, C[r].data_ptr(), 1, n, None) == 0

        many()
        singles()
        diff = float(torch.linalg.norm(B - C) / torch.linalg.norm(C))
        err = float(np.linalg.norm(B.cpu().numpy().T - np.linalg.solve(Hh, B0.cpu().numpy().T)) / np.linalg.norm(B.cpu().numpy()))
        t_many, t_fma, t_single = [], [], []
        for _ in range(REPEATS):
            B.copy_(B0)
            C.copy_(B0)
            t_many.append(timed(many))
            t_single.append(timed(singles))
            B.copy_(B0)
            os.environ["SMCP_POTRS_MANY_MM"] = "0"                   # the updates on the FMA route whatever k (the gate: MFMA from 8 columns)
            t_fma.append(timed(many))
            os.environ["SMCP_POTRS_MANY_MM"] = "1"
        rec = {"case": "potrs%d" % n, "n": n, "k": k, "potrs_many_ms": stats(t_many), "potrs_many_fma_only_ms": stats(t_fma),
               "k_singles_ms": stats(t_single), "ratio": float(np.median(t_many) / np.median(t_single)),
               "rel_diff_many_vs_single": diff, "rel_err_vs_numpy": err}
        print("dense_potrs_many n %d k %d: %.4f ms (min %.4f max %.4f), FMA only %.4f ms (min %.4f max %.4f), %d x dense_potrs %.4f ms "
              "(min %.4f max %.4f), ratio %.3f, difference of the two %.1e, error against numpy %.1e"
              % (n, k, rec["potrs_many_ms"]["median"], min(t_many), max(t_many), rec["potrs_many_fma_only_ms"]["median"], min(t_fma), max(t_fma),
                 k, rec["k_singles_ms"]["median"], min(t_single), max(t_single), rec["ratio"], diff, err), flush=True)
        recs.append(rec)
    return recs


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if args and args[0] == "--out":
        out, args = args[1], args[2:]
    torch.cuda.set_device(0)
    records = []
    for name in (args or list(WORKLOADS) + ["potrs1000", "potrs4096"]):
        records += run_potrs(int(name[5:])) if name.startswith("potrs") else run_workload(name)
    if out:
        with open(out, "w") as f:
            json.dump({"what": "tools/solve_many_time.py: KKTSystem.solve_many against k calls of solve_, dense_potrs_many against k calls of "
                               "dense_potrs(nrhs = 1), on one MI355X, device events, alternated in one process, median of seven warm calls",
                       "records": records}, f, indent=1)
