"""The second trip of the slot-sharing loop `for (e = blockIdx.x; e < a.cnt; e += gridDim.x)` of every kernel that has it
(k_mrc_rank, k_mrc_factor, k_edm_rank, k_edm_factor, k_psd_solve, k_ceig, k_ceig_vec, k_cone_split; csrc/front_*.hip), which
mrc_launch (csrc/completions.hip) reaches only when the slots in device memory of one launch would take more than
tune(symb, TUNE_SLOT_DOUBLES, value) doubles -- 2**25 by default, about a thousand cliques of more than 126 rows.

Every operation runs four times on one context: at the default limit (slot_share 1), at limit 1 (one workgroup walks every
clique of the launch that runs from device memory through ONE slot), at twice the slot of the largest such launch (two
workgroups, one of which takes two cliques or more) and at 0 again.  All four results are equal bit for bit, every counter
included; the first also meets the reference and the bound of the operation's own test module.  The shares asserted are
restated from the slot formulas below, never assumed: a case cannot pass with a share of 1.

Patterns: slot_walk, disjoint dense cliques of orders 131, 40, 127, 140, 89, 128, 16, 129 -- five beyond LDS by every
formula (127 is the first by mrc_slot1 and ceig_slot1, 90 the first by ceig_slot2), three inside; and sibs, a root of 100
rows under four siblings (nn, na) = (30, 98), (36, 95), (44, 92), (10, 92): one level whose factor slots (mrc_slot2,
edm_slot2) are beyond LDS for three siblings of different orders, and four separators beyond LDS for k_psd_solve while only
three cliques are beyond it in the rank pass, so that the share of 4 is k_psd_solve's own.  sibs gives the per-level kernels a
walk of three and four cliques of different orders; fam_top (tests/helpers.py), whose two 130-row tops share a level of a
deeper tree, runs mrcompletion as well (share 2 at limit 1 in both passes; with two slots every clique has its own, so that
run is left out there).

Shares reached at limit 1 / at two slots (MI355X): slot_walk -- rank passes, clique_eigvalsh (both forms), max_step,
clique_eigh, clique_project, cone_project: 5 / 3; mrcompletion and edmcompletion factor pass: 6 / 3 (full rank), 5 / 3 (rank
3); sibs -- rank passes 3 / 2, factor passes 3 / 2, psdcompletion 4 / 2; fam_top -- mrcompletion 2 in both passes.  Wall time on an MI355X: 0.01 - 1.5 s
per case (cone_project and the NaN case 1.4 s, clique_eigh and clique_project 0.5 - 1.1 s, the completions 0.02 - 0.5 s), the
poison case with its child interpreter 8.4 s."""
import ctypes
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import GPU_PATTERNS
from smcp_amd import _lib, chordal, problems
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic
from test_clique_eig_host import (EPS, clique_blocks, clique_spectra_ref, indefinite_on_V, inputs, max_step_ref)
from test_clique_eigh_host import GPU_FACTOR, UNITS
from test_cone_project_host import CONE_UNITS, PARAMS, cone_project_restatement, norm_V, unit_of
from test_cone_wide_host import wide_input
from test_edmcompletion_host import edmcompletion as edm_numpy, points_on_V
from test_mrcompletion_host import clique_rows, low_rank_on_V, mrcompletion as mrc_numpy, pd_on_V
from test_psdcompletion_host import pd_known_answer, psd_levels, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 128 * 1024                                         # MRC_LDS, csrc/completions.hip: bytes of LDS a slot may take
WALK_ORDERS = [131, 40, 127, 140, 89, 128, 16, 129]
SIBS = [(30, 98), (36, 95), (44, 92), (10, 92)]         # (nn, na) of the siblings under a root of SIBS_ROOT rows
SIBS_ROOT = 100
ORTH, RES, PRJ = (GPU_FACTOR * u for u in UNITS)


# ---- the slot formulas and mrc_launch restated ----------------------------------------------------------------------
def mrc_slot1(nf):
    return nf * nf + 2 * nf + 2                          # csrc/front_mrc.hip (k_mrc_rank, k_edm_rank)


def mrc_slot2(nn, na, r):
    return r * na + nn * r + nn * nn + 3 * na + 2 * nn + 4               # csrc/front_mrc.hip (k_mrc_factor)


def edm_slot2(nn, na, r):
    return mrc_slot2(nn, na, r) + r + na + 2             # csrc/front_edm.hip (k_edm_factor)


def psd_slot(na):
    return 2 * na * na + 2 * na + 2                      # csrc/front_psd.hip (k_psd_solve)


def ceig_slot1(nf):
    return nf * nf + 3 * nf + 3                          # csrc/front_ceig.hip (k_ceig, standard form)


def ceig_slot2(nf):
    return 2 * nf * nf + 3 * nf + 3                      # csrc/front_ceig.hip (k_ceig pencil form, k_ceig_vec, k_cone_split)


def beyond_lds(need):
    return need * 8 > LDS


def hbm_slot(launch):
    """the slot of the launch over device memory of one launch group (its slot sizes in doubles): 0 without such a launch"""
    big = [s for s in launch if beyond_lds(s)]
    return (max(big) + 31) // 32 * 32 if big else 0


def share(launches, limit):
    """CSP_Q_SLOT_SHARE of a call that makes these launch groups (each a list of slot sizes) under this limit: mrc_launch
    gives the cliques beyond LDS G = min(cnt, 4 ncu, max(1, limit / slot)) workgroups; cnt stays far below 4 ncu here"""
    most = 0
    for launch in launches:
        cnt = sum(beyond_lds(s) for s in launch)
        if cnt:
            G = min(cnt, max(1, (limit or 2 ** 25) // hbm_slot(launch)))
            most = max(most, -(-cnt // G))
    return most


def two_slots(launches):
    """the limit that gives the launch with the most cliques beyond LDS two workgroups"""
    best = max(launches, key=lambda L: sum(beyond_lds(s) for s in L))
    return 2 * hbm_slot(best)


def all_cliques(symb, slot):
    nn, na = symb.clique_sizes()
    return [[slot(int(nn[k]), int(na[k])) for k in range(symb.Nsn)]]


def by_level(symb, slot):
    nn, na = symb.clique_sizes()
    lp, li = np.asarray(symb.levptr), np.asarray(symb.levidx)
    return [[slot(int(nn[k]), int(na[k])) for k in li[lp[l]:lp[l + 1]]] for l in range(len(lp) - 1)]


RANK = lambda symb: all_cliques(symb, lambda nn, na: mrc_slot1(nn + na))                       # noqa: E731
EIG1 = lambda symb: all_cliques(symb, lambda nn, na: ceig_slot1(nn + na))                      # noqa: E731
EIG2 = lambda symb: all_cliques(symb, lambda nn, na: ceig_slot2(nn + na))                      # noqa: E731
PSD = lambda symb: RANK(symb) + [[psd_slot(na) for na in symb.clique_sizes()[1] if na > 0]]   # noqa: E731


# ---- patterns ---------------------------------------------------------------------------------------------------------
def slot_walk_pattern():
    cl, first = [], 0
    for nf in WALK_ORDERS:
        own = np.arange(first, first + nf)
        cl.append((own, own))
        first += nf
    return problems._from_cliques(first, cl)


def sibs_pattern():
    first = sum(nn for nn, na in SIBS)
    root = np.arange(first, first + SIBS_ROOT)
    cl, at = [], 0
    for s_, (nn, na) in enumerate(SIBS):
        own = np.arange(at, at + nn)
        sep = root[np.sort(np.random.default_rng(40 + s_).choice(SIBS_ROOT, size=na, replace=False))]
        cl.append((own, np.concatenate([own, sep])))
        at += nn
    cl.append((root, root))
    return problems._from_cliques(first + SIBS_ROOT, cl)


PATS = {"slot_walk": slot_walk_pattern, "sibs": sibs_pattern, "fam_top": GPU_PATTERNS["fam_top"]}
_HOST, _SYMB = {}, {}


def host_symb(name):
    if name not in _HOST:
        _HOST[name] = Symbolic(PATS[name]())
    return _HOST[name]


def device_symb(name):
    """a Symbolic of this file's own: the limit is per context"""
    if name not in _SYMB:
        _SYMB[name] = Symbolic(PATS[name]())
        _SYMB[name].device_init(0, 1)
    return _SYMB[name]


@pytest.fixture(scope="module", autouse=True)
def leave_no_device_tensor_behind():
    yield
    for symb in _SYMB.values():
        symb._cache.pop("clique_mult", None)
        symb._cache.pop("cone_weights", None)
    _SYMB.clear()


def test_patterns_and_slot_edges():
    """no GPU: the orders sit where the formulas say, on both sides of the LDS ceiling, and the patterns are what the shares
    in the docstring assume"""
    assert mrc_slot1(127) == 16385 and not beyond_lds(mrc_slot1(126)) and beyond_lds(mrc_slot1(127))
    assert ceig_slot1(127) == 16513 and not beyond_lds(ceig_slot1(126)) and beyond_lds(ceig_slot1(127))
    assert ceig_slot2(90) == 16473 and not beyond_lds(ceig_slot2(89)) and beyond_lds(ceig_slot2(90))
    symb = host_symb("slot_walk")
    nn, na = symb.clique_sizes()
    assert [int(v) for v in nn] == WALK_ORDERS and not np.asarray(na).any()
    wide = [nf for nf in WALK_ORDERS if nf >= 127]
    assert len(wide) == len(set(wide)) == 5 and wide != sorted(wide) and min(wide) == 127
    assert sum(nf <= 89 for nf in WALK_ORDERS) == 3
    for launches in (RANK(symb), EIG1(symb), EIG2(symb)):
        assert share(launches, 0) == 1 and share(launches, 1) == 5 and share(launches, two_slots(launches)) == 3
    symb = host_symb("sibs")
    nn, na = symb.clique_sizes()
    assert sorted(zip((int(v) for v in nn), (int(v) for v in na))) == sorted(SIBS + [(SIBS_ROOT, 0)])
    r = symb.max_front
    assert r == 136
    for slot2, rr in ((mrc_slot2, r), (edm_slot2, r - 1)):
        launches = by_level(symb, lambda n, a: slot2(n, a, rr))
        assert share(launches, 0) == 1 and share(launches, 1) == 3 and share(launches, two_slots(launches)) == 2
    assert share(RANK(symb), 1) == 3 and share(PSD(symb)[1:], 1) == 4 and share(PSD(symb), 1) == 4
    symb = host_symb("fam_top")
    r = symb.max_front
    assert share(RANK(symb), 1) == 2 and share(by_level(symb, lambda n, a: mrc_slot2(n, a, r)), 1) == 2


# ---- the four runs ----------------------------------------------------------------------------------------------------
def bits(t):
    """what is compared: the bytes of a tensor (NaN included), a number as it is"""
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().contiguous().numpy().tobytes()
    return repr(t).encode()


def digest(result):
    h = hashlib.sha256()
    for t in result:
        h.update(bits(t))
    return h.hexdigest()[:16]


def four_runs(symb, run, launches, what, inputs=(), least=3):
    """run() at the default limit, at 1, at two slots and at 0: the shares are the restated ones, above 1 where the limit is
    lowered (at least `least` at limit 1), the results are the same bits, and the inputs (pairs of a device matrix and its
    host blkval) are unchanged after every run.  Returns the first result.  least = 2: a launch of two cliques, where two
    slots would give every clique its own -- that run is left out."""
    limits = [None, 1, two_slots(launches), 0] if least >= 3 else [None, 1, 0]
    want = [share(launches, v or 0) for v in limits]
    assert want[0] == want[-1] == 1 and want[1] >= least, (what, want)
    assert least < 3 or (want[2] >= 2 and want[1] > want[2]), (what, want)
    out = []
    try:
        for v, s in zip(limits, want):
            if v is not None:
                chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, v)
            out.append(run())
            got = chordal.slot_share(symb)
            assert got == s, "%s at limit %s: slot_share %d, restated %d" % (what, v, got, s)
            for X, blk in inputs:
                unchanged(X, blk, "%s at limit %s" % (what, v))
    finally:
        chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, 0)
    for v, o in zip(limits[1:], out[1:]):
        assert len(o) == len(out[0])
        for i, (p, q) in enumerate(zip(out[0], o)):
            assert bits(p) == bits(q), "%s: output %d at limit %s differs from the default run" % (what, i, v)
    return out[0]


def cone_input(name, symb, kind):
    """the cone_project input of tests/test_cone_project_host.py for a Symbolic of pattern `name`, kept per pattern NAME
    (wide_input says why: a key by id(symb) can hand a new Symbolic the input of a freed one)"""
    return wide_input(name, symb, kind)


def on_device(symb, blk):
    assert len(blk) == symb.blklen, "an input of %d doubles for a pattern of %d" % (len(blk), symb.blklen)
    return cspmatrix(symb, torch.from_numpy(np.array(blk)).cuda())


def unchanged(X, blk, what=""):
    assert bits(X.blkval) == np.ascontiguousarray(blk).tobytes(), "%s: an input was written" % what


def query(symb, what):
    out = ctypes.c_int64(0)
    _lib.lib().csp_symbolic_query(symb.handle, what, ctypes.byref(out))
    return out.value


def rank_of(symb, X, fn, tol=1e-12):
    r = ctypes.c_int64(-1)
    rc = getattr(_lib.lib(), fn)(symb.handle, X.blkval.data_ptr(), tol, ctypes.byref(r), None)
    return rc, r.value


# ---- the completions ------------------------------------------------------------------------------------------------------
def mrc_input(symb, kind):
    return pd_on_V(symb, seed=7) if kind == "definite" else low_rank_on_V(symb, 3, seed=3)


def mrc_residual(symb, blk, Y):
    worst = 0.0
    for k in range(symb.Nsn):
        rows = clique_rows(symb, k)
        nn, nf = symb.snptr[k + 1] - symb.snptr[k], len(rows)
        P = blk[symb.blkptr[k]:symb.blkptr[k + 1]].reshape(nn, nf).T
        low = np.arange(nf)[:, None] >= np.arange(nn)[None, :]
        worst = max(worst, np.abs(np.where(low, Y[rows] @ Y[rows[:nn]].T - P, 0.0)).max())
    return worst


def edm_residual(symb, blk, Y):
    worst = 0.0
    for k in range(symb.Nsn):
        rows = clique_rows(symb, k)
        nn, nf = symb.snptr[k + 1] - symb.snptr[k], len(rows)
        P = blk[symb.blkptr[k]:symb.blkptr[k + 1]].reshape(nn, nf).T
        Yr, Yn = Y[rows], Y[rows[:nn]]
        E = (Yr ** 2).sum(axis=1)[:, None] + (Yn ** 2).sum(axis=1)[None, :] - 2.0 * Yr @ Yn.T
        low = np.arange(nf)[:, None] > np.arange(nn)[None, :]
        worst = max(worst, np.abs(np.where(low, E - P, 0.0)).max())
    return worst


# fam_top: the deeper tree the per-level kernels meet in the suite, two 130-row tops in one level (a walk of two cliques)
MRC_CASES = [("slot_walk", "definite"), ("slot_walk", "rank3"), ("sibs", "definite"), ("fam_top", "definite")]
LEAST = {"slot_walk": 3, "sibs": 3, "fam_top": 2}


def run_mrc_rank(name, kind):
    symb = device_symb(name)
    blk = mrc_input(symb, kind)
    X = on_device(symb, blk)
    out = four_runs(symb, lambda: rank_of(symb, X, "csp_mrcompletion_rank"), RANK(symb), "mrcompletion rank pass", [(X, blk)],
                    least=LEAST[name])
    return out


def run_mrc(name, kind):
    symb = device_symb(name)
    blk = mrc_input(symb, kind)
    X = on_device(symb, blk)
    r = symb.max_front if kind == "definite" else 3
    launches = by_level(symb, lambda nn, na: mrc_slot2(nn, na, r))
    out = four_runs(symb, lambda: (chordal.mrcompletion(X), query(symb, 18)), launches, "mrcompletion factor pass", [(X, blk)],
                    least=LEAST[name])
    return symb, blk, r, out


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", MRC_CASES)
def test_mrcompletion(name, kind):
    rc, r1 = run_mrc_rank(name, kind)
    symb, blk, r, (Y, clamped) = run_mrc(name, kind)
    assert rc == 0 and r1 == r == Y.shape[1] and clamped == 0
    Yh = Y.cpu().numpy()
    Yr, _ = mrc_numpy(symb, blk)
    tol = max(1e-10 * np.abs(blk).max(), 100 * mrc_residual(symb, blk, Yr))    # the bound of tests/test_gpu_mrcompletion.py
    res = mrc_residual(symb, blk, Yh)
    assert res <= tol, "mrcompletion %s %s: residual %.3e, bound %.3e" % (name, kind, res, tol)


EDM_CASES = [("slot_walk", None), ("slot_walk", 3), ("sibs", None)]


def run_edm(name, k):
    symb = device_symb(name)
    blk, _ = points_on_V(symb, symb.max_front if k is None else k, seed=5 if k is None else k)
    D = on_device(symb, blk)
    r = symb.max_front - 1 if k is None else k
    rank = four_runs(symb, lambda: rank_of(symb, D, "csp_edmcompletion_rank"), RANK(symb), "edmcompletion rank pass", [(D, blk)])
    launches = by_level(symb, lambda nn, na: edm_slot2(nn, na, r))
    out = four_runs(symb, lambda: (chordal.edmcompletion(D), query(symb, 19)), launches, "edmcompletion factor pass", [(D, blk)])
    return symb, blk, r, rank, out


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", EDM_CASES)
def test_edmcompletion(name, k):
    symb, blk, r, (rc, r1), (Y, clamped) = run_edm(name, k)
    assert rc == 0 and r1 == r == Y.shape[1] and clamped == 0
    Yr, _ = edm_numpy(symb, blk)
    tol = max(1e-10 * blk.max(), 100 * edm_residual(symb, blk, Yr))            # the bound of tests/test_gpu_edmcompletion.py
    res = edm_residual(symb, blk, Y.cpu().numpy())
    assert res <= tol, "edmcompletion %s k %s: residual %.3e, bound %.3e" % (name, k, res, tol)


def run_psd(name):
    symb = device_symb(name)
    blk, Zs, cond = pd_known_answer(symb, seed=11)
    X = on_device(symb, blk)
    out = four_runs(symb, lambda: (chordal.psdcompletion(X, 1e-12),), PSD(symb), "psdcompletion", [(X, blk)])
    return symb, blk, Zs, cond, out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["slot_walk", "sibs"])
def test_psdcompletion(name):
    symb, blk, Zs, cond, (Z,) = run_psd(name)
    assert cond <= 1e3
    e_ref = rel_err(psd_levels(symb, blk), Zs)
    e_dev = rel_err(Z.cpu().numpy(), Zs)
    assert torch.equal(Z, Z.T)
    assert e_dev <= max(1e-10, 100 * e_ref), "psdcompletion %s: error %.3e, restatement %.3e" % (name, e_dev, e_ref)   # tests/test_gpu_psdcompletion.py


# ---- the spectra ------------------------------------------------------------------------------------------------------------
KINDS = ["definite", "rank3", "indefinite", "pencil"]
_CASE = {}


def eig_case(kind):
    if kind not in _CASE:
        symb = host_symb("slot_walk")
        for knd, blkA, blkB in inputs(symb, 11):
            _CASE[knd] = (blkA, blkB)
    return _CASE[kind]


def eig_bound(ref):
    return 16 * len(ref) * EPS * np.abs(ref).max()       # bound() of tests/test_gpu_clique_eig.py


def eigvalsh_raw(symb, A, B):
    """csp_clique_eigvalsh with its status: (rc, w, ext, sweeps)"""
    w = torch.zeros(int(symb.rowptr[-1]), dtype=torch.float64, device="cuda")
    ext = torch.zeros(4, dtype=torch.float64, device="cuda")
    rc = _lib.lib().csp_clique_eigvalsh(symb.handle, A.blkval.data_ptr(), None if B is None else B.blkval.data_ptr(), w.data_ptr(),
                                        ext.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, w, ext, chordal.clique_eig_sweeps(symb)


def run_eigvalsh(kind):
    symb = device_symb("slot_walk")
    blkA, blkB = eig_case(kind)
    A = on_device(symb, blkA)
    B = None if blkB is None else on_device(symb, blkB)
    out = four_runs(symb, lambda: eigvalsh_raw(symb, A, B), EIG1(symb) if B is None else EIG2(symb), "clique_eigvalsh " + kind,
                    [(A, blkA)] + ([] if B is None else [(B, blkB)]))
    return symb, blkA, blkB, out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_clique_eigvalsh(kind):
    symb, blkA, blkB, (rc, w, ext, sweeps) = run_eigvalsh(kind)
    assert rc == 0 and sweeps <= 15
    ref = clique_spectra_ref(symb, blkA, blkB)
    wh = w.cpu().numpy()
    for k in range(symb.Nsn):
        wk = wh[symb.rowptr[k]:symb.rowptr[k + 1]]
        err = np.abs(wk - ref[k]).max()
        assert err <= eig_bound(ref[k]), "clique_eigvalsh %s clique %d: |w - w_ref| %.3e, bound %.3e" % (kind, k, err, eig_bound(ref[k]))


def run_max_step():
    symb = device_symb("slot_walk")
    blkX, blkD = pd_on_V(symb, 5), indefinite_on_V(symb, 6)
    X, D = on_device(symb, blkX), on_device(symb, blkD)
    out = four_runs(symb, lambda: chordal.max_step(X, D, return_clique=True), EIG2(symb), "max_step", [(X, blkX), (D, blkD)])
    return symb, blkX, blkD, out


@pytest.mark.gpu
def test_max_step():
    symb, blkX, blkD, (alpha, k) = run_max_step()
    a_ref, _ = max_step_ref(symb, blkX, blkD)
    ref = clique_spectra_ref(symb, blkD, blkX)
    conds = [np.linalg.cond(B) for B in clique_blocks(symb, blkX)]
    tol = max(eig_bound(r) * c for r, c in zip(ref, conds))                  # pencil_bound of tests/test_gpu_clique_eig.py
    assert 0 < alpha < math.inf
    assert abs(-1.0 / alpha + 1.0 / a_ref) <= tol, "max_step: |mu - mu_ref| %.3e, bound %.3e" % (abs(-1.0 / alpha + 1.0 / a_ref), tol)


def lapack_check(symb, blkA, w, Q, projections, what):
    """check_against_lapack of tests/test_gpu_clique_wide.py with its bounds"""
    from test_gpu_clique_wide import check_against_lapack
    As = clique_blocks(symb, blkA)
    worst = check_against_lapack(symb, As, [np.linalg.eigh(A) for A in As], w, Q, projections)
    for got, bd, name in zip(worst, (16.0, ORTH, RES, PRJ), ("eigenvalues", "orthogonality", "residual", "projection")):
        assert got <= bd, "%s: %s %.2f units, bound %.2f" % (what, name, got, bd)


def run_eigh(kind):
    symb = device_symb("slot_walk")
    blkA, _ = eig_case(kind)
    A = on_device(symb, blkA)
    out = four_runs(symb, lambda: chordal.clique_eigh(A) + (chordal.clique_eig_sweeps(symb),), EIG2(symb), "clique_eigh " + kind,
                    [(A, blkA)])
    return symb, blkA, out


def run_project(kind, lo=-0.5, hi=0.5):
    symb = device_symb("slot_walk")
    blkA, _ = eig_case(kind)
    A = on_device(symb, blkA)
    out = four_runs(symb, lambda: chordal.clique_project(A, lo, hi, return_info=True) + (chordal.clique_eig_sweeps(symb),), EIG2(symb),
                    "clique_project " + kind, [(A, blkA)])
    return symb, blkA, out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS[:3])
def test_clique_eigh_and_project(kind):
    symb, blkA, (w, Q, sweeps) = run_eigh(kind)
    symb, blkA, (Z, wp, info, sweeps_p) = run_project(kind)
    assert torch.equal(w, wp) and sweeps == sweeps_p
    lapack_check(symb, blkA, w, Q, [(-0.5, 0.5, Z, info)], "clique_eigh / clique_project " + kind)


# ---- cone_project at tune 0: k_cone_split from slots in device memory ----------------------------------------------------------
def cone_steps(symb, blk, rho, relax, n=3):
    from test_gpu_cone_project import run_steps, start
    a, x, U, W = start(symb, blk)
    hist = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    run_steps(symb, a, x, U, W, rho, relax, 0, n, hist)
    torch.cuda.synchronize()
    unchanged(a, blk, "cone_project")                      # after every call: four_runs calls this once per limit
    return x.blkval, U, W, hist


def run_cone(kind):
    symb = device_symb("slot_walk")
    blk = cone_input("slot_walk", symb, kind)
    rho, relax = PARAMS[0]
    return symb, blk, four_runs(symb, lambda: cone_steps(symb, blk, rho, relax), EIG2(symb), "cone_project " + kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["noisy", "indef"])
def test_cone_project_three_iterations(kind):
    symb, blk, (x, U, W, hist) = run_cone(kind)
    assert chordal.clique_eig_wide(symb) == 0
    rho, relax = PARAMS[0]
    bd = GPU_FACTOR * CONE_UNITS * unit_of(symb, max(1.0, norm_V(symb, blk)))
    ref = cone_project_restatement(symb, blk, rho=rho, relax=relax, steps=3, near=bd)
    worst = max(np.abs(x.cpu().numpy() - ref["x"]).max(), np.abs(U.cpu().numpy() - ref["U"]).max(),
                np.abs(W.cpu().numpy() - ref["W"]).max()) / unit_of(symb, ref["scale"])
    assert worst <= GPU_FACTOR * CONE_UNITS, "cone_project %s: %.2f units, bound %.2f" % (kind, worst, GPU_FACTOR * CONE_UNITS)
    hh = hist.cpu().numpy()
    assert (np.abs(hh[:, 2] - ref["hist"][:, 2]) <= ref["near"]).all() and (hh[:, 3] == 0).all()


# ---- a clique that ends early, then another trip ---------------------------------------------------------------------------------
def walked(symb, slot):
    """the cliques beyond LDS in the order one workgroup walks them: ascending slot size"""
    nf = np.diff(np.asarray(symb.rowptr))
    ks = [k for k in range(symb.Nsn) if beyond_lds(slot(int(nf[k])))]
    return sorted(ks, key=lambda k: slot(int(nf[k])))


def blocks_equal_outside(symb, got, ref, kb, ptr, what, nan=True):
    """got is NaN on clique kb (nan) and the bits of ref elsewhere; ptr: the offsets of the cliques in both"""
    for k in range(symb.Nsn):
        g, r = got[int(ptr[k]):int(ptr[k + 1])], ref[int(ptr[k]):int(ptr[k + 1])]
        if k == kb:
            assert not nan or torch.isnan(g).all(), "%s: clique %d is not NaN" % (what, k)
        else:
            assert bits(g) == bits(r), "%s: clique %d differs from the clean run" % (what, k)


def run_nan(limit=1):
    """(w of clique_eigvalsh, Z, w, info of clique_project, x, U, W, hist of one cone_project step) with a NaN in the SECOND
    clique of the walk, and the same of the clean input, at this limit"""
    symb = device_symb("slot_walk")
    good, _ = eig_case("indefinite")
    kb = walked(symb, ceig_slot2)[1]
    assert kb == walked(symb, ceig_slot1)[1]
    bad = good.copy()
    bad[symb.blkptr[kb] + 70] = np.nan
    L = _lib.lib()
    res = {}
    chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, limit)
    try:
        for tag, blk in (("bad", bad), ("good", good)):
            X = on_device(symb, blk)
            rc1, w1, _, _ = eigvalsh_raw(symb, X, None)
            s1 = chordal.slot_share(symb)
            Z = torch.zeros(int(chordal.clique_ptr(symb)[-1]), dtype=torch.float64, device="cuda")
            w2 = torch.zeros_like(w1)
            info = torch.zeros((symb.Nsn, 2), dtype=torch.float64, device="cuda")
            rc2 = L.csp_clique_project(symb.handle, X.blkval.data_ptr(), -0.5, 0.5, Z.data_ptr(), w2.data_ptr(), info.data_ptr(), None)
            s2 = chordal.slot_share(symb)
            cone = cone_steps(symb, np.where(np.isnan(blk), np.nan, cone_input("slot_walk", symb, "indef")), *PARAMS[0], n=1)
            s3 = chordal.slot_share(symb)
            res[tag] = (rc1, rc2, (s1, s2, s3), w1, Z, w2, info) + cone
    finally:
        chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, 0)
    return symb, kb, res


@pytest.mark.gpu
def test_non_finite_clique_in_the_middle_of_a_walk():
    """ceig_jacobi returns early for the clique with the NaN (second of five in the walk of the one workgroup at limit 1): it is
    flagged and NaN as without the walk, and the three cliques behind it have the bits of the clean run"""
    symb, kb, res = run_nan()
    q = chordal.clique_ptr(symb)
    rc1, rc2, shares, w1, Z, w2, info, x, U, W, hist = res["bad"]
    g = res["good"]
    assert shares == g[2] == (5, 5, 5)
    assert rc1 == rc2 == -7 and g[0] == g[1] == 0
    rp = np.asarray(symb.rowptr)
    blocks_equal_outside(symb, w1, g[3], kb, rp, "clique_eigvalsh w", nan=False)      # k_ceig leaves what its sweeps left, as without the walk
    blocks_equal_outside(symb, w2, g[5], kb, rp, "clique_project w")
    blocks_equal_outside(symb, Z, g[4], kb, q, "clique_project Z")
    blocks_equal_outside(symb, info.reshape(-1), g[6].reshape(-1), kb, 2 * np.arange(symb.Nsn + 1), "clique_project info")
    blocks_equal_outside(symb, U, g[8], kb, q, "cone_project U", nan=False)     # disjoint cliques: the others do not see the NaN
    blocks_equal_outside(symb, W, g[9], kb, q, "cone_project W", nan=False)
    symb, kb, at_default = run_nan(limit=0)
    assert at_default["bad"][2] == (1, 1, 1)
    for p, r in zip(res["bad"][3:], at_default["bad"][3:]):
        assert bits(p) == bits(r)                                               # flagged and NaN exactly as without the walk


def run_not_pd(limit):
    symb = device_symb("slot_walk")
    blkA, blkB = eig_case("pencil")
    kb = walked(symb, ceig_slot2)[1]
    bad = blkB.copy()
    bad[symb.blkptr[kb]] = -1.0                              # B_jj < 0 for the first column of clique kb
    chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, limit)
    try:
        out = eigvalsh_raw(symb, on_device(symb, blkA), on_device(symb, bad))
        s = chordal.slot_share(symb)
    finally:
        chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, 0)
    return symb, kb, s, out


@pytest.mark.gpu
def test_pencil_whose_second_walked_clique_is_not_positive_definite():
    """CEIG_NOT_PD skips the Jacobi of that clique before the next trip: the status names it, and every other clique has the
    bits of the pencil with a positive definite B"""
    symb, kb, s1, (rc, w, ext, sweeps) = run_not_pd(1)
    _, _, s0, ref = run_not_pd(0)
    assert (s1, s0) == (5, 1) and rc == ref[0] == kb + 1
    assert bits(w) == bits(ref[1]) and bits(ext) == bits(ref[2]) and sweeps == ref[3]
    clean = run_eigvalsh("pencil")[3][1]
    rp = np.asarray(symb.rowptr)
    for k in range(symb.Nsn):
        if k != kb:
            assert bits(w[int(rp[k]):int(rp[k + 1])]) == bits(clean[int(rp[k]):int(rp[k + 1])]), "clique %d differs from the clean pencil" % k


# ---- poison ------------------------------------------------------------------------------------------------------------------------
def limit_one_digests():
    """the limit-1 runs, each on a context made for it (its first call meets the workspace as allocated), as lines"""
    lines = []

    def one(label, name, run, least=3):
        symb = Symbolic(PATS[name]())
        symb.device_init(0, 1)
        chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, 1)
        out = run(symb)
        assert chordal.slot_share(symb) >= least, label
        lines.append("limit 1 %s: share %d digest %s" % (label, chordal.slot_share(symb), digest(out)))

    A, B = eig_case("indefinite")[0], eig_case("pencil")
    one("mrcompletion fam_top", "fam_top", lambda s: (chordal.mrcompletion(on_device(s, mrc_input(s, "definite"))),), least=2)
    one("mrcompletion rank3", "slot_walk", lambda s: (chordal.mrcompletion(on_device(s, mrc_input(s, "rank3"))),))
    one("edmcompletion k3", "slot_walk", lambda s: (chordal.edmcompletion(on_device(s, points_on_V(s, 3, seed=3)[0])),))
    for kind in ("definite", "rank3"):
        Ak = eig_case(kind)[0]
        one("clique_eigvalsh " + kind, "slot_walk", lambda s: eigvalsh_raw(s, on_device(s, Ak), None))
        one("clique_eigh " + kind, "slot_walk", lambda s: chordal.clique_eigh(on_device(s, Ak)))
        one("clique_project " + kind, "slot_walk", lambda s: chordal.clique_project(on_device(s, Ak), -0.5, 0.5, return_info=True))
    one("max_step", "slot_walk", lambda s: chordal.max_step(on_device(s, pd_on_V(s, 5)), on_device(s, indefinite_on_V(s, 6)), return_clique=True))
    for name in ("slot_walk", "sibs"):
        one("mrcompletion " + name, name, lambda s: (chordal.mrcompletion(on_device(s, mrc_input(s, "definite"))),))
        one("edmcompletion " + name, name, lambda s: (chordal.edmcompletion(on_device(s, points_on_V(s, s.max_front, seed=5)[0])),))
        one("psdcompletion " + name, name, lambda s: (chordal.psdcompletion(on_device(s, pd_known_answer(s, seed=11)[0]), 1e-12),))
    one("clique_eigvalsh", "slot_walk", lambda s: eigvalsh_raw(s, on_device(s, A), None))
    one("clique_eigvalsh pencil", "slot_walk", lambda s: eigvalsh_raw(s, on_device(s, B[0]), on_device(s, B[1])))
    one("clique_eigh", "slot_walk", lambda s: chordal.clique_eigh(on_device(s, A)))
    one("clique_project", "slot_walk", lambda s: chordal.clique_project(on_device(s, A), -0.5, 0.5, return_info=True))
    one("cone_project", "slot_walk", lambda s: cone_steps(s, cone_input("slot_walk", s, "indef"), *PARAMS[0]))
    return lines


@pytest.mark.gpu
def test_never_written_workspace_is_not_read_by_a_later_trip():
    """SMCP_POISON=1 fills every fp64 buffer with 4.5e150 when it is allocated (cached per process: a fresh child
    interpreter).  At limit 1 the one slot is the whole workspace of a launch; the child's digests are this process's."""
    want = limit_one_digests()
    env = dict(os.environ, SMCP_POISON="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for line in want:
        assert line in r.stdout, (line, r.stdout[-3000:])


if __name__ == "__main__":
    for line in limit_one_digests():
        print(line)
