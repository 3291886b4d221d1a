"""Single-right-hand-side Hessians on family trees: the resident family up-sweep (k_hess_up_fam1, front_upfam.hip).

For dense input and at most SMCP_UP_FAM (default 1) right-hand sides the leaves -> root sweep takes a family -- a small parent
front with its 1 .. 8 childless children, see test_gpu_family_single_rhs.py -- in one four-wave workgroup, and the level-0
cliques outside the families that fit the kernel (nn <= 16, na <= 64) ride along in the same launch as workgroups without
children.  SMCP_UP_FAM=0 is the previous route: k_hess_up_fam, and a launch of their own for those cliques.  Checked here: the
launch counters on both sides of the gate, the Hessian against the oracle (bound of tests/test_gpu_parity.py::test_hessian:
relative 1e-9 on the pattern's entries), the new route against the previous one on the same inputs, and kkt's solve_ end to end.
The switch is read once per process, so the previous route runs in a child interpreter.
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
from smcp_amd.kkt import KKTSystem
from smcp_amd.symbolic import Symbolic
from test_gpu_family_single_rhs import CASES as _DOWN_CASES, _dev, _hand_tree, _launch_counts, _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-9
# new against previous route, one right-hand side: ten times what two runs of the previous route differ by, at least 1e-13 (about
# a thousand units of fp64 rounding): all that changes is the order of the LDS adds of at most nine summands per front entry
FLOOR = 1e-13

CASES = dict(_DOWN_CASES)
# two families and a leaf outside them whose separator (70 rows) is beyond the kernel's size class: it keeps its own launch
CASES["stray_big"] = lambda: _hand_tree(100, [(15, 40, [(5, 19), (6, 21), (2, 3)]), (11, 13, [(4, 7)])], stray=[(4, 70)], seed=13)
# launches of the per-level small-front kernels (what a level-0 clique outside the families takes on the previous route)
PER_LEVEL = ("k_hess_up_n16", "k_hess_up_pad", "k_hess_up_mfma<true>")


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


def _hessians(name, adj, nrs=(1, 1, 2, 3)):
    """hessian(adj) of seeded right-hand sides on one case, one call per entry of nrs (the same count twice: the same inputs twice)
    -> [(nr, input, output, launch counts)]"""
    symb, S, L, Y, msk = _setup(name, 11)
    Ld, Yd = _dev(symb, L), _dev(symb, Y)
    res = []
    for nr in nrs:
        U = np.random.default_rng(12 + nr).standard_normal((nr, symb.blklen)) * msk
        Ud = torch.from_numpy(U.copy()).cuda()
        c = _launch_counts(symb, lambda: chordal.hessian(Ld, Yd, Ud, adj=adj))
        res.append((nr, U, Ud.cpu().numpy(), c))
    return symb, S, L, Y, msk, res


def _child(env_extra, dst):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), dst], env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return dict(np.load(dst))


@pytest.fixture(scope="module")
def previous():
    """every case on the previous route (SMCP_UP_FAM=0, child interpreter): outputs and launch counters"""
    with tempfile.TemporaryDirectory() as tmp:
        return _child({"SMCP_UP_FAM": "0"}, os.path.join(tmp, "old.npz"))


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("adj", [None, False])
def test_launch_counters(name, adj, previous):
    """one right-hand side takes k_hess_up_fam1 and never k_hess_up_fam; two take k_hess_up_fam; SMCP_UP_FAM=0: k_hess_up_fam"""
    symb, S, L, Y, msk, res = _hessians(name, adj, nrs=(1, 2))
    c1, c2 = res[0][3], res[1][3]
    assert c1.get("k_hess_up_fam1", 0) >= 1 and c1.get("k_hess_up_fam", 0) == 0, c1
    assert c2.get("k_hess_up_fam1", 0) == 0 and c2.get("k_hess_up_fam", 0) >= 1, c2
    tag = "%s/%s" % (name, adj)
    assert int(previous[tag + "/fam1"]) == 0 and int(previous[tag + "/fam"]) >= 1
    # the level-0 cliques outside the families: riding along where they fit (one per-level launch fewer than on the previous
    # route), their own launch where they do not
    per_level = sum(c1.get(k, 0) for k in PER_LEVEL)
    print("%s: per-level launches %d, previous route %d" % (tag, per_level, int(previous[tag + "/per_level"])))
    if name == "under_root":
        assert per_level == int(previous[tag + "/per_level"]) - 1
        assert c1.get("k_hess_up_n16", 0) == 0, c1
    if name == "stray_big":
        assert per_level == int(previous[tag + "/per_level"]) and int(previous[tag + "/per_level"]) >= 1


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("adj,inv", [(None, False), (False, False)])
def test_hessian_one_rhs_against_oracle(name, adj, inv):
    """the (adj, inv) combinations that run a leaves -> root sweep of the forward Hessian"""
    symb, S, L, Y, msk = _setup(name, 3)
    rng = np.random.default_rng(4)
    U = rng.standard_normal(symb.blklen) * msk
    ref = U.copy()
    orc.hessian(S, L, Y, ref, adj=adj, inv=inv)
    Ud = torch.from_numpy(U[None, :].copy()).cuda()
    counts = _launch_counts(symb, lambda: chordal.hessian(_dev(symb, L), _dev(symb, Y), Ud, adj=adj, inv=inv))
    assert counts.get("k_hess_up_fam1", 0) >= 1, counts
    err = _rel(Ud.cpu().numpy()[0][msk], ref[msk])
    print("%s adj=%s inv=%s: rel err %.3e" % (name, adj, inv, err))
    assert err < BOUND
    one = _dev(symb, U)
    chordal.hessian(_dev(symb, L), _dev(symb, Y), [one], adj=adj, inv=inv)
    assert _rel(one.blkval.cpu().numpy()[msk], ref[msk]) < BOUND


@pytest.mark.parametrize("adj", [None, False])
def test_new_route_against_previous_route(adj, previous):
    """1, 2 and 3 right-hand sides on every case: this process against the previous route and both against the oracle, within
    1e-9; for one right-hand side also within max(10 x the difference of two runs of the PREVIOUS route on these inputs, 1e-13)"""
    for name in sorted(CASES):
        symb, S, L, Y, msk, res = _hessians(name, adj)
        tag = "%s/%s" % (name, adj)
        noise = _rel(previous[tag + "/0"][0][msk], previous[tag + "/1"][0][msk])      # calls 0 and 1: the same single right-hand side
        for q, (nr, U, got, counts) in enumerate(res):
            prev = previous["%s/%d" % (tag, q)]
            for r_ in range(nr):
                ref = U[r_].copy()
                orc.hessian(S, L, Y, ref, adj=adj)
                d = _rel(got[r_][msk], prev[r_][msk])
                print("%s nrhs %d rhs %d: new vs previous %.3e (two runs of the previous route: %.3e), new vs oracle %.3e, previous vs oracle %.3e"
                      % (tag, nr, r_, d, noise, _rel(got[r_][msk], ref[msk]), _rel(prev[r_][msk], ref[msk])))
                assert d < BOUND
                assert _rel(got[r_][msk], ref[msk]) < BOUND and _rel(prev[r_][msk], ref[msk]) < BOUND
                if nr == 1:
                    assert counts.get("k_hess_up_fam1", 0) >= 1, counts
                    assert d <= max(10.0 * noise, FLOOR)


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
    assert counts.get("k_hess_up_fam1", 0) >= 1 and counts.get("k_hess_up_fam", 0) == 0, counts
    ex, ey = _rel(bxd.blkval.cpu().numpy()[msk], xr[msk]), _rel(byd.cpu().numpy(), yr)
    print("solve_: rel err x %.3e y %.3e" % (ex, ey))
    assert ex < BOUND and ey < BOUND


if __name__ == "__main__":      # child interpreter (the `previous` fixture): outputs and counters of every case -> npz
    out_ = {}
    for name_ in sorted(CASES):
        for adj_ in (None, False):
            tag_ = "%s/%s" % (name_, adj_)
            res_ = _hessians(name_, adj_)[5]
            c_ = res_[0][3]
            out_[tag_ + "/fam1"] = np.int64(c_.get("k_hess_up_fam1", 0))
            out_[tag_ + "/fam"] = np.int64(c_.get("k_hess_up_fam", 0))
            out_[tag_ + "/per_level"] = np.int64(sum(c_.get(k_, 0) for k_ in PER_LEVEL))
            for q_, (_, _, got_, _) in enumerate(res_):
                out_["%s/%d" % (tag_, q_)] = got_
    np.savez(sys.argv[1], **out_)
