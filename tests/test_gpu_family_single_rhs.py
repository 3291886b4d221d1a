"""Single-right-hand-side Hessians on family trees: the one-launch family down-sweep (k_hess_down_fam, front_downfam.hip).

A family is a small parent front (nn <= 16, na <= 64) with 1 .. 8 childless children (nn <= 16, 1 <= na <= 32).  For one
right-hand side the root -> leaves sweep takes parent and children in one workgroup (the children read their Z_AA from the
parent's front in LDS); SMCP_DOWN_FAM=0 is the previous route (one k_hess_down_w launch per level).  Checked here: the
Hessian against the oracle (bound of tests/test_gpu_parity.py::test_hessian: relative 1e-9 on the pattern's entries), the new
route against the previous one on the same inputs for 1, 2 and 3 right-hand sides (the gate between the routes is crossed), and
kkt's solve_ end to end.  The switch is read once per process, so the previous route runs in a child interpreter.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from smcp_amd import chordal, problems
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.kkt import KKTSystem
from smcp_amd.symbolic import Symbolic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-9


def _hand_tree(root_n, mids, stray=(), seed=0):
    """root (root_n columns, no separator) <- mids [(nn, na, [(leaf nn, leaf na), ...]), ...] <- their leaves; stray: leaves
    (nn, na) that hang off the root directly.  Separators are random subsets of the parent's clique; columns in postorder."""
    rng = np.random.default_rng(seed)
    n = root_n + sum(mn + sum(ln for ln, _ in lv) for mn, _, lv in mids) + sum(ln for ln, _ in stray)
    root = np.arange(n - root_n, n)
    cl, pos = [], 0
    for mn, ma, leaves in mids:
        nl = sum(ln for ln, _ in leaves)
        own = np.arange(pos + nl, pos + nl + mn)
        mid = np.concatenate([own, np.sort(rng.choice(root, size=ma, replace=False))])
        for ln, la in leaves:
            lo = np.arange(pos, pos + ln)
            cl.append((lo, np.concatenate([lo, np.sort(rng.choice(mid, size=la, replace=False))])))
            pos += ln
        cl.append((own, mid))
        pos += mn
    for ln, la in stray:
        lo = np.arange(pos, pos + ln)
        cl.append((lo, np.concatenate([lo, np.sort(rng.choice(root, size=la, replace=False))])))
        pos += ln
    cl.append((root, root))
    return problems._from_cliques(n, cl)


def _nested(**kw):
    return lambda: problems.nested_block_arrow_pattern(nsub=2, nmid=6, **kw)


CASES = {
    # the synth50k shape at reduced size: (15, 64) parents with eight (5, 31) leaves; then one and three leaves per parent
    "synth_8": _nested(nleaf_per_mid=8, seed=3),
    "synth_1": _nested(nleaf_per_mid=1, seed=4),
    "synth_3": _nested(nleaf_per_mid=3, seed=5),
    # other member sizes: the largest a family takes (nn = 16 parents, na = 64; leaves (16, 32)), odd ones, a parent with na <= 16
    "sizes_max": _nested(nleaf_per_mid=8, leaf=(16, 32), mid=(16, 64), seed=6),
    "sizes_odd": _nested(nleaf_per_mid=5, leaf=(3, 17), mid=(7, 33), seed=7),
    "sizes_small": _nested(nleaf_per_mid=4, leaf=(4, 7), mid=(9, 12), top=(20, 30), root=40, seed=8),
    # families directly under the root, with 1 .. 8 children whose na is not a multiple of 16, parents with nn < 16 and nn = 16,
    # na = 64 and na <= 16, and a leaf that hangs off the root (not a family front) beside them
    "under_root": lambda: _hand_tree(70, [(16, 64, [(5, 31), (3, 17), (16, 32), (2, 1), (7, 23), (4, 9), (1, 30), (6, 5)]),
                                          (11, 13, [(4, 7)]),
                                          (15, 40, [(5, 19), (6, 21), (2, 3)]),
                                          (16, 16, [(3, 16), (8, 15)])], stray=[(4, 11), (5, 31)], seed=9),
    # the family parent IS the root (no separator, no Z_AA of its own)
    "root_family": lambda: _hand_tree(12, [], stray=[(3, 7), (5, 11), (2, 4)], seed=10),
}


def _rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb if nb > 0 else np.linalg.norm(a)


def _setup(name, seed):
    symb = Symbolic(CASES[name]())
    symb.device_init(0, 4)
    S = orc.Sym(symb)
    A = problems.random_factor_blkval(symb, seed)
    orc.llt(S, A)
    msk = np.zeros(symb.blklen, dtype=bool)
    msk[symb.ccs_to_blk()] = True
    L = A.copy()
    orc.cholesky(S, L)
    Y = L.copy()
    orc.projected_inverse(S, Y)
    return symb, S, L, Y, msk


def _dev(symb, x):
    return cspmatrix(symb, torch.from_numpy(np.ascontiguousarray(x)).cuda())


def _launch_counts(symb, fn):
    """kernel name -> launches while fn() runs"""
    import ctypes
    from smcp_amd import _lib
    lib = _lib.lib()
    h = symb.handle
    nk = int(lib.csp_profile_kinds())
    names = [lib.csp_profile_kernel_name(i).decode() for i in range(nk)]
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
    return {names[i]: int(cnt[i]) for i in range(nk) if cnt[i]}


def _hessians(name, nrs=(1, 2, 3)):
    """hessian(adj=None) of 1, 2 and 3 seeded right-hand sides on one case -> {nr: output}, launch counts of the nr = 1 call"""
    symb, S, L, Y, msk = _setup(name, 11)
    rng = np.random.default_rng(12)
    Ld, Yd = _dev(symb, L), _dev(symb, Y)
    out, counts = {}, None
    for nr in nrs:
        U = rng.standard_normal((nr, symb.blklen)) * msk
        Ud = torch.from_numpy(U.copy()).cuda()
        c = _launch_counts(symb, lambda: chordal.hessian(Ld, Yd, Ud, adj=None))
        if nr == 1:
            counts = c
        out[nr] = (U, Ud.cpu().numpy())
    return symb, S, L, Y, msk, out, counts


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_hold_families(name):
    """every case really reaches the family kernel with one right-hand side (and only then: the gate is at one)"""
    symb, S, L, Y, msk, out, counts = _hessians(name, nrs=(1,))
    assert counts.get("k_hess_down_fam", 0) >= 1, counts
    Ud = torch.from_numpy(out[1][0].repeat(2, axis=0)).cuda()
    c2 = _launch_counts(symb, lambda: chordal.hessian(_dev(symb, L), _dev(symb, Y), Ud, adj=None))
    assert c2.get("k_hess_down_fam", 0) == 0, c2


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("adj,inv", [(None, False), (False, False), (True, False)])
def test_hessian_one_rhs_against_oracle(name, adj, inv):
    symb, S, L, Y, msk = _setup(name, 3)
    rng = np.random.default_rng(4)
    U = rng.standard_normal(symb.blklen) * msk
    ref = U.copy()
    orc.hessian(S, L, Y, ref, adj=adj, inv=inv)
    Ud = torch.from_numpy(U[None, :].copy()).cuda()
    chordal.hessian(_dev(symb, L), _dev(symb, Y), Ud, adj=adj, inv=inv)
    err = _rel(Ud.cpu().numpy()[0][msk], ref[msk])
    print("%s adj=%s inv=%s: rel err %.3e" % (name, adj, inv, err))
    assert err < BOUND
    one = _dev(symb, U)
    chordal.hessian(_dev(symb, L), _dev(symb, Y), [one], adj=adj, inv=inv)
    assert _rel(one.blkval.cpu().numpy()[msk], ref[msk]) < BOUND


def test_inverse_hessian_unaffected():
    """the inverse modes have kernels of their own"""
    symb, S, L, Y, msk = _setup("synth_8", 3)
    rng = np.random.default_rng(5)
    U = rng.standard_normal(symb.blklen) * msk
    ref = U.copy()
    orc.hessian(S, L, Y, ref, adj=None, inv=True)
    Ud = torch.from_numpy(U[None, :].copy()).cuda()
    counts = _launch_counts(symb, lambda: chordal.hessian(_dev(symb, L), _dev(symb, Y), Ud, adj=None, inv=True))
    assert counts.get("k_hess_down_fam", 0) == 0, counts
    assert _rel(Ud.cpu().numpy()[0][msk], ref[msk]) < BOUND


def test_new_route_against_previous_route():
    """hessian(adj=None) with 1, 2 and 3 right-hand sides on every case: this process (family down-sweep for one right-hand
    side) against a child interpreter with SMCP_DOWN_FAM=0 (k_hess_down_w per level for every count), and both against the
    oracle.  The new kernel runs the products of the old one on the same operand values; the differences printed (measured: 0 to
    8e-17, as large for 2 and 3 right-hand sides, where both processes take the same route, as for 1) are those between two runs
    of one route.  The assertion is the 1e-9 of the oracle comparison."""
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "old.npz")
        env = dict(os.environ, SMCP_DOWN_FAM="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), dst], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        old = dict(np.load(dst))
    for name in sorted(CASES):
        symb, S, L, Y, msk, out, counts = _hessians(name)
        assert counts.get("k_hess_down_fam", 0) >= 1, counts
        assert int(old["%s/fam" % name]) == 0
        for nr, (U, got) in out.items():
            prev = old["%s/%d" % (name, nr)]
            for r_ in range(nr):
                ref = U[r_].copy()
                orc.hessian(S, L, Y, ref, adj=None)
                d = _rel(got[r_][msk], prev[r_][msk])
                print("%s nrhs %d rhs %d: new vs previous %.3e, new vs oracle %.3e, previous vs oracle %.3e"
                      % (name, nr, r_, d, _rel(got[r_][msk], ref[msk]), _rel(prev[r_][msk], ref[msk])))
                assert d < BOUND
                assert _rel(got[r_][msk], ref[msk]) < BOUND and _rel(prev[r_][msk], ref[msk]) < BOUND


def test_kkt_solve_end_to_end():
    """x, y of one Newton-KKT solve against the oracle; solve_ applies two single-right-hand-side Hessians"""
    symb, S, L, Y, msk = _setup("synth_8", 21)
    m = 12
    cptr, cidx, cval = problems.random_constraints(symb, m, density=0.002, seed=22)
    K = orc.KKT(S, cptr, cidx, cval)
    H = K.schur_factor(L, Y)
    sys_ = KKTSystem(symb, cptr, cidx, cval, max_rhs=4)
    solve = sys_.factor(_dev(symb, L), _dev(symb, Y))
    rng = np.random.default_rng(23)
    bx = rng.standard_normal(symb.blklen) * msk
    by = rng.standard_normal(m)
    xr, yr = K.solve(L, Y, H, bx, by, 0.5)
    bxd, byd = _dev(symb, bx), torch.from_numpy(by.copy()).cuda()
    counts = _launch_counts(symb, lambda: solve(bxd, byd, 0.5))
    assert counts.get("k_hess_down_fam", 0) >= 1, counts
    ex, ey = _rel(bxd.blkval.cpu().numpy()[msk], xr[msk]), _rel(byd.cpu().numpy(), yr)
    print("solve_: rel err x %.3e y %.3e" % (ex, ey))
    assert ex < BOUND and ey < BOUND


if __name__ == "__main__":      # child interpreter of test_new_route_against_previous_route: outputs of every case -> npz
    res = {}
    for name_ in sorted(CASES):
        _, _, _, _, _, out_, counts_ = _hessians(name_)
        res["%s/fam" % name_] = np.int64(counts_.get("k_hess_down_fam", 0))
        for nr_, (_, got_) in out_.items():
            res["%s/%d" % (name_, nr_)] = got_
    np.savez(sys.argv[1], **res)
