"""GPU: the calling contract of the C ABI (include/smcp_amd.h) that no parity test exercises.

* the strict upper triangle of every X_NN block (blkval slots outside V) is zero on entry and EXACTLY zero on exit of every
  operation (flat axpy / scal / dot rely on it);
* ldu, ldb and ldh may exceed the packed size and the padding is never written;
* more right-hand sides than the context's max_rhs (ragged last chunks of one);
* the caller's stream: work queued on a non-default stream behind a long-running producer, no host synchronisation;
* NaN / Inf in the input of a factorisation is a failure (ArithmeticError), not a result, and the context recovers;
* csp_device_bytes is what the context holds NOW: replacing the constraints, repeating a partition and growing max_rhs
  give back what they replace (exact integer equalities on fresh contexts).

Bounds are those of tests/test_gpu_dense_ref.py (dense_ref.device_bound).
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from smcp_amd import _lib, chordal, problems, shard
from smcp_amd.cspmatrix import _stream, cspmatrix
from smcp_amd.kkt import KKTSystem
from smcp_amd.symbolic import Symbolic
from tests import dense_ref
from tests.dense_ref import HESS_MODES, MODE_OP, blockwise, relvec, to_dev, to_host
from tests.helpers import GPU_PATTERNS
from tests.test_gpu_parity import setup

pytestmark = pytest.mark.gpu
NAMES = sorted(GPU_PATTERNS)
SENTINEL = 7.25
STRIDE_PATTERNS = ["nested_mid", "fam_odd", "arrow_big", "arrow_thin"]
CSP_Q_FAMILY = 17


@pytest.fixture(scope="module")
def yard():
    return dense_ref.load_yardstick()


@pytest.fixture(scope="module")
def cases():
    """name -> (Symbolic with a device context, DenseCase), formed once per pattern and module."""
    cache = {}

    def get(name):
        if name not in cache:
            pat = GPU_PATTERNS[name]()
            symb = Symbolic(pat)
            symb.device_init(0, 4)
            cache[name] = (symb, dense_ref.DenseCase(pat, orc.Sym(symb), dense_ref.YARDSTICK_SEED))
        return cache[name]

    return get


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


class deterministic:
    def __init__(self, symb, on):
        self.symb, self.on = symb, on

    def __enter__(self):
        if self.on:
            chordal.tune(self.symb, chordal.TUNE_DETERMINISTIC, 1)

    def __exit__(self, *exc):
        if self.on:
            chordal.tune(self.symb, chordal.TUNE_DETERMINISTIC, 0)


# ---- unowned slots ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_unowned_slots_stay_exactly_zero(name, cases):
    symb, case = cases(name)
    up = ~case.low
    dirty = []

    def look(tag, out):
        a = np.atleast_2d(out)[:, up]
        if not (a == 0).all():
            dirty.append((tag, int((a != 0).sum()), "nan" if np.isnan(a).any() else float(np.abs(a).max())))

    ops = dense_ref.device_ops(symb, case)
    Lref = case.cholesky()
    look("cholesky", ops.cholesky(case.Ablk.copy()))
    look("llt", ops.llt(Lref.copy()))
    look("projected_inverse", ops.projected_inverse(Lref.copy()))
    look("completion", ops.completion(case.Yblk.copy()))
    for factors in (True, False):
        L, Y = to_dev(symb, case.Ablk), to_dev(symb, np.zeros(symb.blklen))
        chordal.cholesky_projected_inverse(L, Y, factors=factors)
        look("cholesky_projected_inverse L factors=%d" % factors, to_host(L))
        look("cholesky_projected_inverse Y factors=%d" % factors, to_host(Y))
    for nrhs in (1, 4):
        u = case.rhs(nrhs, case.seed + 30)
        for adj, inv in HESS_MODES:
            look("hessian adj=%s inv=%s nrhs=%d" % (adj, inv, nrhs), ops.hessian(u, adj, inv))
    k = case.kkt()
    for route in ("chol", "qr"):
        kkt = dense_ref.device_kkt(symb, route=route)
        _, solve = kkt(k.con, Lref, case.Yblk)
        look("aadj (%s system)" % route, to_host(kkt.last.aadj(cuda(k.by))))
        for kk in dense_ref.KKT_KK:
            look("bx of the %s solve kk=%g" % (route, kk), solve(k.bx.copy(), k.by.copy(), kk)[0])
    assert not dirty, dirty


# ---- strides ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", STRIDE_PATTERNS)
def test_hessian_with_a_leading_dimension_beyond_blklen(name, det, cases, yard):
    symb, case = cases(name)
    ops = dense_ref.device_ops(symb, case)
    bl = symb.blklen
    u = case.rhs(4, case.seed + 40)
    with deterministic(symb, det):
        for adj, inv in [(None, False), (False, False), (True, True)]:
            packed = ops.hessian(u, adj, inv)
            for ldu in (bl + 1, -(-bl // 64) * 64 + 64):
                buf = torch.full((4, ldu), SENTINEL, dtype=torch.float64, device="cuda")
                buf[:, :bl] = cuda(u)
                chordal.hessian(ops.L, ops.Y, buf, adj=adj, inv=inv)
                h = buf.cpu().numpy()
                assert (h[:, bl:] == SENTINEL).all(), ("padding written", adj, inv, ldu)
                if det:
                    assert np.array_equal(h[:, :bl], packed), (adj, inv, ldu)
                else:
                    bound = dense_ref.device_bound(MODE_OP[(adj, inv)], yard)
                    for r in range(4):
                        assert blockwise(case.S, h[r, :bl], packed[r])[1] <= bound, (adj, inv, ldu, r)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", STRIDE_PATTERNS)
def test_trsm_with_a_leading_dimension_beyond_n(name, det, cases, yard):
    symb, case = cases(name)
    n = symb.n
    Ld = to_dev(symb, case.cholesky())
    rng = np.random.default_rng(case.seed + 41)
    bound = dense_ref.device_bound("trsm", yard)
    with deterministic(symb, det):
        for nrhs in (4, 8, 70):
            for trans in ("N", "T"):
                B = rng.standard_normal((nrhs, n))
                packed = cuda(B)
                chordal.trsm(Ld, packed, trans)
                wide = torch.full((nrhs, n + 3), SENTINEL, dtype=torch.float64, device="cuda")
                view = wide[:, :n]
                view.copy_(cuda(B))
                assert view.stride(0) == n + 3
                chordal.trsm(Ld, view, trans)
                w = wide.cpu().numpy()
                assert (w[:, n:] == SENTINEL).all(), ("padding written", nrhs, trans)
                if det:
                    assert np.array_equal(w[:, :n], packed.cpu().numpy()), (nrhs, trans)
                else:
                    assert relvec(w[:, :n], packed.cpu().numpy()) <= bound, (nrhs, trans)
                ref = np.linalg.solve(case.Ld if trans == "N" else case.Ld.T, B.T).T
                assert relvec(w[:, :n], ref) <= bound, (nrhs, trans)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", STRIDE_PATTERNS)
def test_kkt_c_abi_with_leading_dimensions_beyond_m(name, det, cases, yard):
    """kkt_schur_factor + kkt_solve with ldh = m + 3 and dense_potrs with ldb > n, straight through the C ABI (the Python layer
    never passes a non-packed ldh)."""
    symb, case = cases(name)
    k = case.kkt()
    lib = _lib.lib()
    sysk = KKTSystem(symb, *k.con, max_rhs=4)
    m = sysk.m
    ldh = m + 3
    Ld, Yd = to_dev(symb, case.cholesky()), to_dev(symb, case.Yblk)
    kk = 0.25
    with deterministic(symb, det):
        solve = sysk.factor(Ld, Yd)
        Hp = sysk.H.cpu().numpy().copy()                       # row r = column r of the column-major factor
        bxp, byp = to_dev(symb, k.bx), cuda(k.by)
        solve(bxp, byp, kk)
        sysk._own()
        Hs = torch.full((m, ldh), SENTINEL, dtype=torch.float64, device="cuda")
        assert lib.kkt_schur_factor(symb.handle, Ld.blkval.data_ptr(), Yd.blkval.data_ptr(), Hs.data_ptr(), ldh, _stream()) == 0
        bxs, bys = to_dev(symb, k.bx), cuda(k.by)
        assert lib.kkt_solve(symb.handle, Ld.blkval.data_ptr(), Yd.blkval.data_ptr(), Hs.data_ptr(), ldh, kk,
                             bxs.blkval.data_ptr(), bys.data_ptr(), _stream()) == 0
        # dense_potrs on the strided factor with a strided right-hand side
        nrhs, ldb = 3, m + 2
        Bh = np.random.default_rng(case.seed + 42).standard_normal((nrhs, m))
        Bs = torch.full((nrhs, ldb), SENTINEL, dtype=torch.float64, device="cuda")
        Bs[:, :m] = cuda(Bh)
        assert lib.dense_potrs(symb.handle, Hs.data_ptr(), m, ldh, Bs.data_ptr(), nrhs, ldb, _stream()) == 0
        Bp = cuda(Bh)
        assert lib.dense_potrs(symb.handle, sysk.H.data_ptr(), m, m, Bp.data_ptr(), nrhs, m, _stream()) == 0
        torch.cuda.synchronize()
        assert lib.kkt_schur_forget(symb.handle, Hs.data_ptr()) == 0
    hs = Hs.cpu().numpy()
    assert (hs[:, m:] == SENTINEL).all(), "padding of H written"
    bs = Bs.cpu().numpy()
    assert (bs[:, m:] == SENTINEL).all(), "padding of B written"
    Hls, Hlp = np.tril(hs[:, :m].T), np.tril(Hp.T)
    if det:
        assert np.array_equal(Hls, Hlp)
        assert np.array_equal(to_host(bxs), to_host(bxp)) and np.array_equal(bys.cpu().numpy(), byp.cpu().numpy())
        assert np.array_equal(bs[:, :m], Bp.cpu().numpy())
    else:
        assert relvec(Hls @ Hls.T, Hlp @ Hlp.T) <= dense_ref.device_bound("kkt_H", yard)
        assert blockwise(case.S, to_host(bxs), to_host(bxp))[1] <= dense_ref.device_bound("kkt_x", yard)
        assert relvec(bys.cpu().numpy(), byp.cpu().numpy()) <= dense_ref.device_bound("kkt_y", yard)
    # and against the dense definitions
    xr, yr = case.kkt_solve(kk)
    assert relvec(Hls @ Hls.T, k.H) <= dense_ref.device_bound("kkt_H", yard)
    assert blockwise(case.S, to_host(bxs), xr)[1] <= dense_ref.device_bound("kkt_x", yard)
    assert relvec(bys.cpu().numpy(), yr) <= dense_ref.device_bound("kkt_y", yard)
    assert relvec(bs[:, :m].T, np.linalg.solve(k.H, Bh.T)) <= dense_ref.device_bound("kkt_y", yard)


# ---- more right-hand sides than max_rhs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [2, 3, 5, 9])
@pytest.mark.parametrize("name", ["nested_mid", "fam_odd", "fam_top", "arrow_big"])
def test_hessian_with_more_right_hand_sides_than_max_rhs(name, nrhs, cases, yard):
    """csp_hessian walks chunks of max_rhs = 4: 5 = 4 + 1 and 9 = 4 + 4 + 1 leave a last chunk of ONE, which takes the resident
    single-RHS sweeps behind the batched ones.  Every row against the dense definition and against the same row sent alone."""
    _, case = cases(name)
    symb = Symbolic(case.pat)                       # a context of its own: nothing may have grown its workspace
    symb.device_init(0, 4)
    assert symb._max_rhs == 4
    ops = dense_ref.device_ops(symb, case)
    alone = {}

    def hess(U, adj, inv):
        out = ops.hessian(U, adj, inv)
        assert symb._max_rhs == 4
        for r in range(U.shape[0]):
            one = ops.hessian(U[r:r + 1], adj, inv)[0]
            op = "alone " + MODE_OP[(adj, inv)]
            alone[op] = max(alone.get(op, 0.0), blockwise(case.S, out[r], one)[1])
        return out

    errs = dense_ref.hessian_errors(case, hess, case.rhs(nrhs, case.seed + 50), case.rhs(nrhs, case.seed + 51))
    print("DENSEREF maxrhs %s nrhs=%d" % (name, nrhs), " ".join("%s=%.2e" % kv for kv in sorted({**errs, **alone}.items())))
    bad = {op: e for op, e in errs.items() if not e <= dense_ref.device_bound(op, yard)}
    bad.update({op: e for op, e in alone.items() if not e <= dense_ref.device_bound(op[6:], yard)})
    assert not bad, bad


# ---- the caller's stream ------------------------------------------------------------------------------------------------
def _step(symb, case, sysk, src, side):
    """One whole step -- cholesky, projected_inverse, KKT factor + solve, hessian -- on freshly NaN-filled buffers; with `side`
    everything (a long producer first, then the copies of the real input) is queued on a fresh stream without any host
    synchronisation until the results sit in pinned host memory."""
    bl, m = symb.blklen, sysk.m
    A, Yb, bx = (torch.full((bl,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3))
    by = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
    U = torch.full((4, bl), float("nan"), dtype=torch.float64, device="cuda")
    G = torch.ones((6144, 6144), dtype=torch.float64, device="cuda")
    Z = torch.empty_like(G)
    outs = [torch.empty(t.shape, dtype=torch.float64).pin_memory() for t in (A, Yb, bx, by, U, sysk.H)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        for _ in range(4):                                   # 4 x 0.46 Tflop of fp64: tens of ms before the input arrives
            torch.matmul(G, G, out=Z)
        A.copy_(src["A"], non_blocking=True)
        bx.copy_(src["bx"], non_blocking=True)
        by.copy_(src["by"], non_blocking=True)
        U.copy_(src["U"], non_blocking=True)
        L, Y, X = cspmatrix(symb, A), cspmatrix(symb, Yb), cspmatrix(symb, bx)
        chordal.cholesky(L)
        Yb.copy_(A)
        chordal.projected_inverse(Y)
        solve = sysk.factor(L, Y)
        solve(X, by, 0.25)
        chordal.hessian(L, Y, U, adj=None, inv=False)
        for o, t in zip(outs, (A, Yb, bx, by, U, sysk.H)):
            o.copy_(t, non_blocking=True)
    stream.synchronize()
    chordal.check_status(symb)
    res = [o.numpy().copy() for o in outs]
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", ["nested_mid", "fam_odd", "arrow_big", "three_tops"])
def test_work_queued_on_the_callers_stream(name, det, cases, yard):
    """A NaN in the output means a side stream of the library did not wait for the caller's stream (it read the buffers before
    the input was copied in); a stale or wrong value means it did not join back before the results were copied out.  Runs
    under chordal.lazy_status so that the library itself never waits for the device between the calls."""
    symb, case = cases(name)
    k = case.kkt()
    sysk = KKTSystem(symb, *k.con, max_rhs=4)
    src = {key: torch.from_numpy(np.ascontiguousarray(v)).pin_memory() for key, v in
           dict(A=case.Ablk, bx=k.bx, by=k.by, U=case.rhs(4, case.seed + 60)).items()}
    chordal.lazy_status(symb, True)
    try:
        with deterministic(symb, det):
            ref = _step(symb, case, sysk, src, side=False)
            got = _step(symb, case, sysk, src, side=True)
    finally:
        chordal.lazy_status(symb, False)
    tags = ("L", "Y", "x", "y", "hessian", "H")
    for tag, g in zip(tags, got):
        assert not np.isnan(g).any(), "%s holds NaN: a side stream did not wait for the caller's stream" % tag
    if det:
        for tag, g, r in zip(tags, got, ref):
            assert np.array_equal(g, r), tag
        return
    S = case.S
    Hg, Hr = np.tril(got[5].T), np.tril(ref[5].T)
    errs = {"cholesky": blockwise(S, got[0], ref[0])[1], "projected_inverse": blockwise(S, got[1], ref[1])[1],
            "kkt_x": blockwise(S, got[2], ref[2])[1], "kkt_y": relvec(got[3], ref[3]),
            "hessian": max(blockwise(S, got[4][r], ref[4][r])[1] for r in range(4)), "kkt_H": relvec(Hg @ Hg.T, Hr @ Hr.T)}
    bad = {op: e for op, e in errs.items() if not e <= dense_ref.device_bound(op, yard)}
    assert not bad, bad


# ---- NaN and Inf in the input -------------------------------------------------------------------------------------------
def _clique_for(symb, kind):
    nf = np.diff(symb.rowptr)
    fam = np.zeros(symb.Nsn, dtype=np.int64)
    assert _lib.lib().csp_symbolic_query(symb.handle, CSP_Q_FAMILY, fam.ctypes.data_as(ctypes.c_void_p)) == symb.Nsn
    if kind == "family child":
        ks = np.flatnonzero(fam == 1)
        assert len(ks), "no family in this pattern"
        return int(ks[len(ks) // 2])
    if kind == "one-workgroup front":                        # the largest front below the root that is in no family
        ks = np.flatnonzero((fam == 0) & (np.arange(symb.Nsn) < symb.Nsn - 1))
        return int(ks[np.argmax(nf[ks])])
    return symb.Nsn - 1                                      # the root


@pytest.mark.parametrize("value,where", [(float("nan"), "offdiag"), (float("inf"), "diag")])
@pytest.mark.parametrize("name,kind", [("fam_odd", "family child"), ("nested_mid", "one-workgroup front"), ("arrow_one", "root")])
def test_nan_and_inf_in_the_input_are_failures(name, kind, value, where, cases, yard):
    symb, case = cases(name)
    k = _clique_for(symb, kind)
    assert symb.rowptr[k + 1] - symb.rowptr[k] >= 2
    pos = int(symb.blkptr[k]) + (1 if where == "offdiag" else 0)       # (row 1, column 0) / (0, 0) of the clique's panel
    assert case.low[pos]
    S = case.S

    def poisoned(x):
        x = x.copy()
        x[pos] = value
        return x

    def good_cholesky():
        X = to_dev(symb, case.Ablk)
        chordal.cholesky(X)
        assert blockwise(S, to_host(X), case.cholesky())[1] <= dense_ref.device_bound("cholesky", yard)

    with pytest.raises(ArithmeticError):
        chordal.cholesky(to_dev(symb, poisoned(case.Ablk)))
    good_cholesky()
    with pytest.raises(ArithmeticError):
        chordal.completion(to_dev(symb, poisoned(case.Yblk)))
    X = to_dev(symb, case.Yblk)
    chordal.completion(X)
    assert blockwise(S, to_host(X), case.Lblk)[1] <= dense_ref.device_bound("completion", yard)
    with pytest.raises(ArithmeticError):
        chordal.cholesky_projected_inverse(to_dev(symb, poisoned(case.Ablk)), to_dev(symb, np.zeros(symb.blklen)))
    L, Y = to_dev(symb, case.Ablk), to_dev(symb, np.zeros(symb.blklen))
    chordal.cholesky_projected_inverse(L, Y)
    assert blockwise(S, to_host(L), case.cholesky())[1] <= dense_ref.device_bound("cholesky", yard)
    assert blockwise(S, to_host(Y), case.Yblk)[1] <= dense_ref.device_bound("projected_inverse", yard)


# ---- device memory ------------------------------------------------------------------------------------------------------
def _bytes_after_solves(name, ms):
    """A fresh context (device_init(0, 4)); per m of ms a KKTSystem on random_constraints(symb, m, density=0.05, seed=9) and
    one factor + solve of the Cholesky solver; device_bytes() after each."""
    symb, _, A, msk = setup(name, 7)
    L = to_dev(symb, A)
    chordal.cholesky(L)
    Y = L.copy()
    chordal.projected_inverse(Y)
    rng = np.random.default_rng(2)
    out = []
    for m in ms:
        sys_ = KKTSystem(symb, *problems.random_constraints(symb, m, density=0.05, seed=9), max_rhs=4)
        solve = sys_.factor(L, Y)
        solve(to_dev(symb, rng.standard_normal(symb.blklen) * msk), cuda(rng.standard_normal(m)), 1.0)
        torch.cuda.synchronize()
        out.append(symb.device_bytes())
    return out


@pytest.mark.parametrize("name", ["fam_odd", "arrow_big", "dense600"])
def test_replacing_constraints_returns_the_memory(name):
    b1, b2, b3 = _bytes_after_solves(name, (7, 3, 7))
    print("device bytes after m = 7, 3, 7:", b1, b2, b3)
    assert b3 == b1
    # (the first context is gone by now: nothing of it may count for the second)
    assert _bytes_after_solves(name, (7,)) == [b1]


def test_repeating_a_partition_returns_the_memory():
    symb = Symbolic(GPU_PATTERNS["nested_mid"]())
    symb.device_init(0, 4)
    owner = np.ascontiguousarray(shard.subtree_partition(symb, 2).owner, dtype=np.int32)
    assert owner.max() == 1
    lib = _lib.lib()
    assert lib.csp_set_partition(symb.handle, owner.ctypes.data, 0) == 0
    b1 = symb.device_bytes()
    assert lib.csp_set_partition(symb.handle, owner.ctypes.data, 0) == 0
    b2 = symb.device_bytes()
    print("device bytes after the first and the second csp_set_partition:", b1, b2)
    assert b2 == b1


def test_growing_max_rhs_replaces_the_workspaces():
    pat = GPU_PATTERNS["fam_odd"]()
    grown = Symbolic(pat)
    grown.device_init(0, 4)
    b4 = grown.device_bytes()
    grown.device_init(0, 9)
    direct = Symbolic(pat)
    direct.device_init(0, 9)
    print("device bytes at max_rhs 4, grown to 9, 9 at once:", b4, grown.device_bytes(), direct.device_bytes())
    assert grown.device_bytes() == direct.device_bytes() > b4
    grown.device_init(0, 4)
    assert grown.device_bytes() == direct.device_bytes()


# ---- invalid constraint sets ----------------------------------------------------------------------------------------------
def test_an_invalid_constraint_set_leaves_nothing_behind():
    """kkt_set_constraints releases the outgoing set, then refuses a set with a position outside blkval or in the strict upper
    triangle of an NN block.  A valid set installed afterwards gives the Schur complement (fixed-order kernels: bit for bit)
    and the device bytes of a context that never saw the refused ones."""
    pat = problems.band_pattern(40, 3)

    def schur(with_invalid):
        symb = Symbolic(pat)
        symb.device_init(0, 4)
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 1)
        A = problems.random_factor_blkval(symb, 7)
        orc.llt(orc.Sym(symb), A)
        L = to_dev(symb, A)
        chordal.cholesky(L)
        Y = L.copy()
        chordal.projected_inverse(Y)
        cptr, cidx, cval = problems.random_constraints(symb, 3, density=0.2, seed=4)
        if with_invalid:
            nn, na = symb.clique_sizes()
            k = int(np.flatnonzero(nn >= 2)[0])
            upper = int(symb.blkptr[k]) + int(nn[k] + na[k])           # (row 0, column 1) of the clique's panel
            for where, pos in ((0, symb.blklen), (len(cidx) - 1, upper)):
                bad = cidx.copy()
                bad[where] = pos
                with pytest.raises(RuntimeError, match="invalid argument"):
                    KKTSystem(symb, cptr, bad, cval, max_rhs=4)
        sysk = KKTSystem(symb, cptr, cidx, cval, max_rhs=4)
        sysk.build_schur(L, Y)
        torch.cuda.synchronize()
        chordal.check_status(symb)
        return sysk.H.cpu().numpy(), symb.device_bytes()

    H1, b1 = schur(True)
    H0, b0 = schur(False)
    print("device bytes with and without the refused sets:", b1, b0)
    assert np.isfinite(H0).all() and np.abs(H0).max() > 0
    assert np.array_equal(H1, H0)
    assert b1 == b0
