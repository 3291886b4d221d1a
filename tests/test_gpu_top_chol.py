"""The register-resident one-workgroup Cholesky of the top fronts with its fused inverse (k_top_chol, front_top.hip).

Fronts of the large-front class with at most 208 rows take k_top_chol; at the scaling point (cholesky_projected_inverse) the
last level's launch also leaves Li = L_NN^-1 behind, and k_lf_diag_inv / k_lf_trtri are not launched for that level.
SMCP_TOP_FUSED=0 is the previous route (k_mid_chol, k_lf_diag_inv, k_lf_trtri); the switch is read once per process, so the
previous route runs in a child interpreter.

Which fronts reach the kernel: a clique whose working set fits LDS is a small clique and never a large front, so the single
dense cliques below about 71 columns (1 .. 65 here) stay with the small-clique kernels on both routes -- their results are
checked all the same.  The kernel's small shapes (nn = 1, 15, 16, 17, 33, fronts (17, 40), (16, 16), (5, 3)) reach it through a
level whose small cliques do not fit LDS TOGETHER ((60, 10) beside (5, 80)): such a level is demoted to the large-front class as
a whole ("mixed": eight fronts of different sizes in one launch).

Bounds: L and Y per clique against the dense definitions, dense_ref.device_bound (100 x the recorded yardstick, capped at
1e-12); one-right-hand-side Hessians of the new route against the previous one within ten times what two runs of the previous
route differ by, floor 1e-13 (the rule of tests/test_gpu_family_up_single_rhs.py).
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
from smcp_amd.symbolic import Symbolic
from tests import dense_ref
from tests.dense_ref import blockwise, to_dev, to_host
from test_gpu_family_single_rhs import _hand_tree, _launch_counts, _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 1e-13
TOP_MAXROWS = 208          # the class limit (front_top.hip)


def _dense(n):
    return lambda: problems.band_pattern(n, n - 1)


CASES = {"dense%d" % n: _dense(n) for n in (1, 15, 16, 17, 33, 64, 65, 129, TOP_MAXROWS, TOP_MAXROWS + 1)}
# a (64, 128) top with a few children under a root of 130 columns (a partial last tile, no separator)
CASES["top64_128"] = lambda: _hand_tree(130, [(64, 128, [(5, 19), (6, 21), (3, 7)])], seed=31)
# one demoted level: eight childless fronts of different sizes in one launch, under a root of 100 columns
CASES["mixed"] = lambda: _hand_tree(100, [], stray=[(60, 10), (5, 80), (17, 40), (16, 16), (5, 3), (1, 5), (15, 16), (33, 7)], seed=32)
# three tops of different sizes in one level (each with children), root 96 = six whole tiles
CASES["three"] = lambda: _hand_tree(96, [(64, 90, [(5, 19)]), (40, 33, [(4, 9), (6, 30)]), (80, 96, [(3, 11)])], seed=33)
# cases whose last level is of the class: the new route must launch k_top_chol and no triangular-inversion kernel for that level
IN_CLASS = ("dense129", "dense%d" % TOP_MAXROWS, "top64_128", "mixed", "three")
INV_KERNELS = ("k_lf_trtri", "k_lf_diag_inv")
MODES = (None, False)


def _case(name):
    pat = CASES[name]()
    symb = Symbolic(pat)
    symb.device_init(0, 4)
    return symb, dense_ref.DenseCase(pat, orc.Sym(symb), dense_ref.YARDSTICK_SEED)


def _run(name):
    """scaling point + one-right-hand-side Hessians (adj None and False), twice on fresh buffers -> results, launch counters"""
    symb, case = _case(name)
    out = {}
    for rep in range(2):
        L, Y = to_dev(symb, case.Ablk), to_dev(symb, np.zeros(symb.blklen))
        counts = _launch_counts(symb, lambda: chordal.cholesky_projected_inverse(L, Y))
        out["L%d" % rep], out["Y%d" % rep] = to_host(L), to_host(Y)
        for adj in MODES:
            U = (np.random.default_rng(7).standard_normal(symb.blklen) * case.low)[None, :]
            Ud = torch.from_numpy(U.copy()).cuda()
            chordal.hessian(L, Y, Ud, adj=adj)
            out["H%d/%s" % (rep, adj)] = Ud.cpu().numpy()[0]
        if rep == 0:
            for kname in ("k_top_chol", "k_mid_chol") + INV_KERNELS:
                out["n/" + kname] = np.int64(counts.get(kname, 0))
    return symb, case, out


@pytest.fixture(scope="module")
def previous():
    """every case on the previous route (SMCP_TOP_FUSED=0, child interpreter)"""
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "old.npz")
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), SMCP_TOP_FUSED="0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), dst], env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return dict(np.load(dst))


@pytest.mark.parametrize("name", sorted(CASES))
def test_scaling_point_and_hessian(name, previous):
    symb, case, out = _run(name)
    yard = dense_ref.load_yardstick()
    # L and Y against the dense definitions, per clique
    eL = blockwise(case.S, out["L0"], case.cholesky())[1]
    eY = blockwise(case.S, out["Y0"], case.Yblk)[1]
    print("%s: L %.2e (bound %.2e)  Y %.2e (bound %.2e)" % (name, eL, dense_ref.device_bound("cholesky", yard), eY,
                                                          dense_ref.device_bound("projected_inverse", yard)))
    assert eL <= dense_ref.device_bound("cholesky", yard)
    assert eY <= dense_ref.device_bound("projected_inverse", yard)
    # launch counters of both routes
    n = {k[2:]: int(v) for k, v in out.items() if k.startswith("n/")}
    old = {k[len(name) + 3:]: int(v) for k, v in previous.items() if k.startswith(name + "/n/")}
    print("%s: launches %s, previous route %s" % (name, n, old))
    assert old["k_top_chol"] == 0
    if name in IN_CLASS:
        # the last level (the root, nn columns): one k_lf_diag_inv launch and two k_lf_trtri launches per doubling level
        # (block sizes 64, 128, ... below nn) on the previous route, none here; the levels below keep theirs on both routes
        nn_root = int(np.diff(symb.snptr)[-1])
        root_trtri = 2 * sum(1 for b in (64, 128) if b < nn_root)
        assert n["k_top_chol"] >= 1, n
        assert n["k_lf_diag_inv"] == old["k_lf_diag_inv"] - 1 and n["k_lf_trtri"] == old["k_lf_trtri"] - root_trtri, (n, old)
        assert old["k_mid_chol"] > n["k_mid_chol"] and old["k_lf_trtri"] >= root_trtri, old
        if name.startswith("dense"):
            assert all(n[k] == 0 for k in INV_KERNELS), n
    if name == "dense%d" % (TOP_MAXROWS + 1):      # beyond the class: the old launches
        assert n["k_top_chol"] == 0 and n == old and n["k_mid_chol"] >= 1, (n, old)
    # the Hessians read Li from the inverse-form factor the scaling point left behind
    for adj in MODES:
        key = "H0/%s" % adj
        got, prev = out[key][case.low], previous[name + "/" + key][case.low]
        noise = _rel(previous[name + "/H1/%s" % adj][case.low], prev)
        d = _rel(got, prev)
        print("%s adj=%s: new vs previous %.3e (two runs of the previous route: %.3e)" % (name, adj, d, noise))
        assert d <= max(10.0 * noise, FLOOR)


@pytest.mark.parametrize("name", ["top64_128", "mixed"])
def test_cholesky_alone_does_not_advertise_an_inverse(name):
    """scaling point on A (Li of A cached), then cholesky ALONE of another matrix in the SAME buffers, projected inverse, Hessian:
    the Hessian is that of the second matrix (dense definition)"""
    symb, case = _case(name)
    yard = dense_ref.load_yardstick()
    L, Y = to_dev(symb, case.Ablk), to_dev(symb, np.zeros(symb.blklen))
    chordal.cholesky_projected_inverse(L, Y)
    other = dense_ref.DenseCase(case.pat, case.S, dense_ref.YARDSTICK_SEED + 1)
    L.blkval.copy_(torch.from_numpy(other.Ablk))
    counts = _launch_counts(symb, lambda: chordal.cholesky(L))
    assert counts.get("k_top_chol", 0) >= 1, counts
    Y.blkval.copy_(L.blkval)
    chordal.projected_inverse(Y)
    assert blockwise(case.S, to_host(L), other.cholesky())[1] <= dense_ref.device_bound("cholesky", yard)
    assert blockwise(case.S, to_host(Y), other.Yblk)[1] <= dense_ref.device_bound("projected_inverse", yard)
    u = np.random.default_rng(8).standard_normal(symb.blklen) * case.low
    Ud = torch.from_numpy(u[None, :].copy()).cuda()
    chordal.hessian(L, Y, Ud, adj=None)
    err = blockwise(case.S, Ud.cpu().numpy()[0], other.hessian(u))[1]
    print("%s: Hessian after cholesky alone, against the dense definition %.2e" % (name, err))
    assert err <= dense_ref.device_bound("hessian", yard)


def _diag_slot(symb, k, j):
    nf = int(symb.rowptr[k + 1] - symb.rowptr[k])
    return int(symb.blkptr[k]) + j * nf + j


def _failures(name):
    """(label, poisoned blkval) of the case: not positive definite at the first pivot of the root, at the last pivot of the
    root's partial last tile, inside the front with the widest separator, and a NaN below the root's diagonal"""
    symb, case = _case(name)
    nn = np.diff(symb.snptr)
    na = np.diff(symb.rowptr) - nn
    root, sep = int(np.flatnonzero(na == 0)[-1]), int(np.argmax(na))
    assert nn[root] % 16 != 0 and na[sep] > 0
    bad = []
    for label, slot, val in (("first pivot", _diag_slot(symb, root, 0), -1.0),
                             ("last partial tile", _diag_slot(symb, root, int(nn[root]) - 1), -1.0e3),
                             ("front with separator", _diag_slot(symb, sep, int(nn[sep]) // 2), -1.0e3),
                             ("nan", _diag_slot(symb, root, 0) + 1, float("nan"))):
        x = case.Ablk.copy()
        x[slot] = val
        bad.append((label, x))
    return symb, case, bad


@pytest.mark.parametrize("name", ["top64_128", "mixed"])
def test_failures_raise_and_the_context_recovers(name):
    symb, case, bad = _failures(name)
    yard = dense_ref.load_yardstick()
    for label, x in bad:
        with pytest.raises(ArithmeticError):
            chordal.cholesky_projected_inverse(to_dev(symb, x), to_dev(symb, np.zeros(symb.blklen)))
        with pytest.raises(ArithmeticError):
            chordal.cholesky(to_dev(symb, x))
        L, Y = to_dev(symb, case.Ablk), to_dev(symb, np.zeros(symb.blklen))
        chordal.cholesky_projected_inverse(L, Y)
        eL, eY = blockwise(case.S, to_host(L), case.cholesky())[1], blockwise(case.S, to_host(Y), case.Yblk)[1]
        print("%s after '%s': L %.2e Y %.2e" % (name, label, eL, eY))
        assert eL <= dense_ref.device_bound("cholesky", yard) and eY <= dense_ref.device_bound("projected_inverse", yard)


if __name__ == "__main__":      # child interpreter (the `previous` fixture): results and counters of every case -> npz
    out_ = {}
    for name_ in sorted(CASES):
        for k_, v_ in _run(name_)[2].items():
            out_[name_ + "/" + k_] = v_
    np.savez(sys.argv[1], **out_)
