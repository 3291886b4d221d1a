"""KKTSystem.solve_many_qr / kkt_qr_solve_many: the kkt_qr solve (solvers.py:430-471) for a block of right-hand sides on one
factor_qr -- the rows against the oracle's Householder restatement and against the single closure, the state it must leave
alone (L, Y, Q, R, the closure), isolation of the rows, launch counts, refusals, the ledger and the deferred status regime."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from smcp_amd import _lib, chordal, problems, shard
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.kkt import KKTSystem, solve_many_qr_chunks
from smcp_amd.symbolic import Symbolic
from tests.helpers import GPU_PATTERNS, launch_counts
from tests.test_gpu_parity import _kkt_qr_case, dev, rel, setup
from tests.test_gpu_solve_many import SENT, _device_residuals, _padded

pytestmark = pytest.mark.gpu

STACK_KERNELS = ("k_stack_dots_many", "k_stack_comb_many")
NEW_KERNELS = STACK_KERNELS + ("k_qr_many_sum", "k_qr_many_small", "k_qr_many_mid")


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same_bits(a, b):
    return a.shape == b.shape and bool(_bits(a).equal(_bits(b)))


# ---- 1. rows against the oracle ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_case(name):
    """the inputs of test_kkt_qr_factor_and_solve and the Householder solutions of nine rows for both kk: computed once per
    pattern, shared by the two max_rhs, never written to"""
    m = 7
    symb, S, msk, L, Yh, cptr, cidx, cval = _kkt_qr_case(name, m, 21)
    K = orc.KKT(S, cptr, cidx, cval)
    F = K.qr_factor(L, Yh)
    rng = np.random.default_rng(8)
    BXh = rng.standard_normal((9, symb.blklen)) * msk
    BYh = rng.standard_normal((9, m))
    refs = {kk: [K.qr_solve(L, Yh, F, BXh[r], BYh[r], kk) for r in range(9)] for kk in (1.0, 0.25)}
    return dict(m=m, S=S, msk=msk, L=L, Yh=Yh, cons=(cptr, cidx, cval), K=K, BXh=BXh, BYh=BYh, refs=refs)


@pytest.mark.parametrize("max_rhs", [3, 12])
@pytest.mark.parametrize("name", ["arrow", "rand2", "nested_mid", "fam_max", "fam_nine", "nested", "band"])
def test_rows_against_the_oracle(name, max_rhs):
    """Bounds of test_kkt_qr_factor_and_solve on its inputs: 1e-9 for x on the pattern and for y against K.qr_solve, 1e-10 for
    the two residuals of K.residual; 1, 2, 5 and 9 padded rows.  A completion of another matrix before every block call replaces
    chol(Y_AA) in the cache (the stale case of that test).  Afterwards L, Y and R have their bits, Q is orthonormal, and the
    single closure gives the bits it gave before."""
    c = _oracle_case(name)
    m, S, msk, L, Yh, K, BXh, BYh = (c[k] for k in ("m", "S", "msk", "L", "Yh", "K", "BXh", "BYh"))
    symb = Symbolic(GPU_PATTERNS[name]())
    symb.device_init(0, 4)
    sys = KKTSystem(symb, *c["cons"], max_rhs=max_rhs, tnzcols=0.0)
    bl = symb.blklen
    cap = int(_lib.lib().kkt_qr_solve_many_chunk(symb._max_rhs))
    for k in (5, 9):
        ch = solve_many_qr_chunks(k, symb._max_rhs)
        assert sum(ch) == k and all(x == cap for x in ch[:-1])
        if max_rhs == 3:
            assert len(ch) > 1, ch
    Ld, Yd = dev(symb, L), dev(symb, Yh)
    solve = sys.factor_qr(Ld, Yd)
    assert sys.qr_passes == 2 and sys.qr_shift == 0.0
    Rt0, _ = sys.qr_inspect()
    keep = [Ld.blkval.clone(), Yd.blkval.clone()]
    states = (Ld.state(), Yd.state())

    def single():
        # from the same state of the cache both times (chol(Y_AA) replaced by another factorisation and formed again), and with
        # the Hessian sweeps of the closure on the fixed-order route: on the default route the small fronts add their children's
        # updates with LDS atomics and two identical calls of the closure differ in the last bits whatever lies between them
        chordal.completion(dev(symb, Yh * 1.5))
        bx, by = dev(symb, BXh[1]), torch.from_numpy(BYh[1].copy()).cuda()
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 1)
        try:
            solve(bx, by, 0.7)
        finally:
            chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 0)
        return bx.blkval.clone(), by.clone()

    s0 = single()
    for kk in (1.0, 0.25):
        refs = c["refs"][kk]
        for k in (1, 2, 5, 9):
            other = dev(symb, Yh * (1.0 + 0.5 * kk))
            chordal.completion(other)
            BX, BY = _padded(BXh[:k], bl, 3), _padded(BYh[:k], m, 2)
            assert BX.stride(0) == bl + 3 and BY.stride(0) == m + 2
            out = sys.solve_many_qr(Ld, Yd, BX, BY, kk)
            assert out[0] is BX and out[1] is BY
            assert bool((BX[:, bl:] == SENT).all()) and bool((BY[:, m:] == SENT).all())
            gx, gy = BX[:, :bl].cpu().numpy(), BY[:, :m].cpu().numpy()
            for r in range(k):
                xr, yr = refs[r]
                ex, ey = rel(gx[r][msk], xr[msk]), rel(gy[r], yr)
                res, rr = K.residual(L, Yh, gx[r] * msk, gy[r], BXh[r], BYh[r], kk)
                r1 = np.sqrt(orc.dot(S, res, res)) / max(1, np.sqrt(orc.dot(S, BXh[r], BXh[r])))
                r2 = np.linalg.norm(rr) / max(1, np.linalg.norm(BYh[r]))
                print("%s max_rhs %d kk %g k %d row %d: x %.2e y %.2e residuals %.2e %.2e" % (name, max_rhs, kk, k, r, ex, ey, r1, r2))
                assert ex < 1e-9 and ey < 1e-9, (kk, k, r, ex, ey)
                assert r1 < 1e-10 and r2 < 1e-10, (kk, k, r, r1, r2)
    assert _same_bits(Ld.blkval, keep[0]) and _same_bits(Yd.blkval, keep[1])
    assert (Ld.state(), Yd.state()) == states
    Rt1, G = sys.qr_inspect()
    assert np.abs(G.cpu().numpy() - np.eye(m)).max() < 1e-13
    assert np.array_equal(Rt1.view(np.int64), Rt0.view(np.int64))
    s1 = single()
    print("%s max_rhs %d: single closure before / after, largest difference x %.1e y %.1e"
          % (name, max_rhs, float((s1[0] - s0[0]).abs().max()), float((s1[1] - s0[1]).abs().max())))
    assert _same_bits(s1[0], s0[0]) and _same_bits(s1[1], s0[1])


# ---- 2. block edges -----------------------------------------------------------------------------------------------------
def _device_case(name, m, max_rhs, density, seed=7):
    symb, S, A, msk = setup(name, seed)
    L = dev(symb, A)
    chordal.cholesky(L)
    Y = L.copy()
    chordal.projected_inverse(Y)
    cons = problems.random_constraints(symb, m, density=density, seed=9)
    sys = KKTSystem(symb, *cons, max_rhs=max_rhs, tnzcols=0.0)
    return symb, msk, L, Y, sys


@pytest.mark.parametrize("m", [70, 130])
def test_block_edges(m):
    """arrow_big: blklen 172 032, several position chunks of both products.  m = 70: the one-workgroup triangular class with a
    ragged second 64-block; m = 130: three block steps each way and a ragged last tile of sixteen rows of Q.  3, 9 and 17 rows
    (17 crosses a sixteen-column tile).  Each device residual of a row is at most 10 x the single closure's for that row (a
    different summation order, nothing more), floor 1e-10."""
    kk = 0.25
    symb, msk, L, Y, sys = _device_case("arrow_big", m, 20, 0.002)
    bl = symb.blklen
    assert bl == 172032
    solve = sys.factor_qr(L, Y)
    print("m %d: passes %d shift %g, chunks of 17 rows %s" % (m, sys.qr_passes, sys.qr_shift, solve_many_qr_chunks(17, symb._max_rhs)))
    mskd = torch.from_numpy(msk.astype(np.float64)).cuda()
    rng = np.random.default_rng(8)
    BX0 = torch.from_numpy(rng.standard_normal((17, bl)) * msk).cuda()
    BY0 = torch.from_numpy(rng.standard_normal((17, m))).cuda()
    single = []
    for r in range(17):
        bx, by = cspmatrix(symb, BX0[r].clone()), BY0[r].clone()
        solve(bx, by, kk)
        single.append(_device_residuals(symb, sys, L, Y, mskd, bx.blkval, by, BX0[r], BY0[r], kk))
    for k in (3, 9, 17):
        BX, BY = BX0[:k].clone(), BY0[:k].clone()
        sys.solve_many_qr(L, Y, BX, BY, kk)
        got = [_device_residuals(symb, sys, L, Y, mskd, BX[r], BY[r], BX0[r], BY0[r], kk) for r in range(k)]
        for r in range(k):
            print("m %d k %d row %d  block %.3e %.3e   single %.3e %.3e" % ((m, k, r) + got[r] + single[r]))
        for r in range(k):
            assert got[r][0] <= max(10 * single[r][0], 1e-10), (k, r)
            assert got[r][1] <= max(10 * single[r][1], 1e-10), (k, r)


# ---- 3. determinism and isolation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m", [("nested_mid", 7), ("arrow_big", 130)])
def test_determinism_and_isolation(name, m):
    symb, msk, L, Y, sys = _device_case(name, m, 12, 0.05 if m == 7 else 0.002)
    bl = symb.blklen
    rng = np.random.default_rng(11)
    BX0 = torch.from_numpy(rng.standard_normal((5, bl)) * msk).cuda()
    BY0 = torch.from_numpy(rng.standard_normal((5, m))).cuda()
    sys.factor_qr(L, Y)
    assert solve_many_qr_chunks(5, symb._max_rhs) == [5]

    def block(BXi, BYi, pad=0):
        BX = torch.full((5, bl + pad), SENT, dtype=torch.float64, device="cuda")
        BY = torch.full((5, m + 2 * pad), SENT, dtype=torch.float64, device="cuda")
        BX[:, :bl] = BXi
        BY[:, :m] = BYi
        sys.solve_many_qr(L, Y, BX, BY, 0.7)
        assert bool((BX[:, bl:] == SENT).all()) and bool((BY[:, m:] == SENT).all())
        return BX[:, :bl].clone(), BY[:, :m].clone()

    d0, d1 = block(BX0, BY0), block(BX0, BY0)
    print("%s m %d, default route, the same block call twice: largest difference x %.1e y %.1e"
          % (name, m, float((d0[0] - d1[0]).abs().max()), float((d0[1] - d1[1]).abs().max())))
    # the Hessian sweeps on the fixed-order route, as in the same test of solve_many (the LDS classes of the default sweeps add the
    # children's updates with atomics: nested_mid differs in the last bits from call to call there, arrow_big does not); the factor
    # is the one made above on the default route -- kkt_qr_factor has no other
    chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 1)
    try:
        _isolation(block, BX0, BY0)
    finally:
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 0)
    if name == "arrow_big":                                                       # large fronts only: no atomics on the default route
        _isolation(block, BX0, BY0)


def _isolation(block, BX0, BY0):
    a = block(BX0, BY0)
    b = block(BX0, BY0)
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all())
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])                      # the same call twice: the same bits
    for pad in (1, 5):
        p = block(BX0, BY0, pad)
        assert _same_bits(p[0], a[0]) and _same_bits(p[1], a[1]), pad             # the padding width does not matter
    for bad in (0, 3):
        BXn, BYn = BX0.clone(), BY0.clone()
        BXn[bad], BYn[bad] = float("nan"), float("nan")
        c = block(BXn, BYn)                                                       # one row poisoned
        for r in range(5):
            if r != bad:
                assert _same_bits(c[0][r], a[0][r]) and _same_bits(c[1][r], a[1][r]), (bad, r)


# ---- 4. launches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m,density", [("nested_mid", 7, 0.05), ("arrow_big", 130, 0.002)])
def test_launches_do_not_depend_on_the_number_of_rows(name, m, density):
    symb, msk, L, Y, sys = _device_case(name, m, 16, density)
    bl = symb.blklen
    assert solve_many_qr_chunks(8, symb._max_rhs) == [8]
    sys.factor_qr(L, Y)
    rng = np.random.default_rng(12)
    counts = {}
    for k in (2, 8):
        BX = torch.from_numpy(rng.standard_normal((k, bl)) * msk).cuda()
        BY = torch.from_numpy(rng.standard_normal((k, m))).cuda()
        sys.solve_many_qr(L, Y, BX.clone(), BY.clone(), 1.0)                      # warm: caches, workspace
        counts[k] = launch_counts(symb, lambda: sys.solve_many_qr(L, Y, BX, BY, 1.0))
    assert counts[2] == counts[8], (counts[2], counts[8])
    for n in STACK_KERNELS + ("k_qr_many_sum", "k_kkt_many_scale"):
        assert counts[2].get(n, 0) == 1, (n, counts[2])
    for n in ("k_stack_dots", "k_stack_comb", "k_dense_potrs", "k_potrs_many_small"):
        assert n not in counts[2], (n, counts[2])
    if m <= 128:
        assert counts[2].get("k_qr_many_small", 0) == 1 and "k_potrs_many_step" not in counts[2] and "k_qr_many_mid" not in counts[2]
    else:
        assert counts[2].get("k_potrs_many_step", 0) == 2 * ((m + 63) // 64) and counts[2].get("k_qr_many_mid", 0) == 1
        assert "k_qr_many_small" not in counts[2]
    # two chunks: every kernel of the chain twice
    cap = int(_lib.lib().kkt_qr_solve_many_chunk(symb._max_rhs))
    k = cap + 1
    BX = torch.from_numpy(rng.standard_normal((k, bl)) * msk).cuda()
    BY = torch.from_numpy(rng.standard_normal((k, m))).cuda()
    two = launch_counts(symb, lambda: sys.solve_many_qr(L, Y, BX, BY, 1.0))
    for n in STACK_KERNELS:
        assert two.get(n, 0) == 2, (n, two)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = _lib.lib()
    m = 7
    symb, msk, L, Y, sys = _device_case("arrow", m, 12, 0.05)
    bl, h = symb.blklen, symb.handle
    rng = np.random.default_rng(5)
    buf = torch.from_numpy(rng.standard_normal(4 * bl + 64)).cuda()
    buf0 = buf.clone()
    BX = buf[:2 * bl].view(2, bl)
    BY = torch.from_numpy(rng.standard_normal((2, m))).cuda()
    BY0 = BY.clone()
    Lp, Yp = L.blkval.data_ptr(), Y.blkval.data_ptr()

    def call(Lq=Lp, Yq=Yp, bx=BX.data_ptr(), ldbx=bl, by=BY.data_ptr(), ldby=m, nrhs=2):
        return lib.kkt_qr_solve_many(h, Lq, Yq, 1.0, bx, ldbx, by, ldby, nrhs, None)

    def untouched():
        torch.cuda.synchronize()
        return _same_bits(buf, buf0) and _same_bits(BY, BY0)

    # before any factor_qr
    assert call() == -1
    with pytest.raises(RuntimeError):
        sys.solve_many_qr(L, Y, BX, BY, 1.0)
    assert untouched()
    solve = sys.factor_qr(L, Y)
    # another L or Y than the factored one
    L2, Y2 = L.copy(), Y.copy()
    assert call(Lq=L2.blkval.data_ptr()) == -1 and call(Yq=Y2.blkval.data_ptr()) == -1
    with pytest.raises(RuntimeError):
        sys.solve_many_qr(L2, Y, BX, BY, 1.0)
    with pytest.raises(RuntimeError):
        sys.solve_many_qr(L, Y2, BX, BY, 1.0)
    # shapes and overlaps
    assert call(nrhs=0) == -1
    assert call(ldbx=bl - 1) == -1
    assert call(ldby=m - 1) == -1
    assert call(by=buf[bl:].data_ptr()) == -1                      # BY inside BX
    assert call(by=buf[2 * bl - 1:].data_ptr()) == -1              # ... overlapping its last entry
    assert call(bx=buf[2 * bl + 3:].data_ptr(), by=buf[2 * bl:].data_ptr()) == -1      # BX starting inside BY
    with pytest.raises(ValueError):
        sys.solve_many_qr(L, Y, BX, BY[:1], 1.0)
    with pytest.raises(ValueError):
        sys.solve_many_qr(L, Y, BX[:, :bl - 1], BY, 1.0)
    with pytest.raises(ValueError):
        sys.solve_many_qr(L, Y, BX, BY[:, :m - 1], 1.0)
    with pytest.raises(ValueError):
        sys.solve_many_qr(L, Y, BX[:0], BY[:0], 1.0)               # k = 0
    assert untouched()
    assert call(by=buf[2 * bl:].data_ptr()) == 0                   # side by side is fine, and the closure still works
    buf.copy_(buf0)
    solve(cspmatrix(symb, BX[0].clone()), BY[0].clone(), 1.0)
    BY.copy_(BY0)
    # factor() and solve_many() on the same system drop Q
    sys.factor(L, Y)
    assert call() == -1
    with pytest.raises(RuntimeError):
        sys.solve_many_qr(L, Y, BX, BY, 1.0)
    assert untouched()
    sys.factor_qr(L, Y)                                            # (H is still the factor that factor() left)
    X2, Y2b = BX.clone(), BY.clone()
    sys.solve_many(L, Y, X2, Y2b, 1.0)
    with pytest.raises(RuntimeError):
        sys.solve_many_qr(L, Y, BX, BY, 1.0)
    assert untouched()
    # another KKTSystem on the same Symbolic
    sys.factor_qr(L, Y)
    cons2 = problems.random_constraints(symb, m, density=0.05, seed=10)
    other = KKTSystem(symb, *cons2, max_rhs=12, tnzcols=0.0)
    other.factor_qr(L, Y)
    with pytest.raises(RuntimeError, match="another KKTSystem"):
        sys.solve_many_qr(L, Y, BX, BY, 1.0)
    assert untouched()
    # a multi-rank partition on the context (installed after the factorisation: kkt_qr_factor refuses it itself)
    P = shard.subtree_partition(symb, 2)
    owner = np.ascontiguousarray(P.owner, dtype=np.int32)
    assert owner.max() == 1
    assert lib.csp_set_partition(h, owner.ctypes.data, 0) == 0
    assert call() == -1
    assert untouched()
    # a context without constraints
    bare = Symbolic(GPU_PATTERNS["arrow"]())
    bare.device_init(0, 4)
    assert lib.kkt_qr_solve_many(bare.handle, Lp, Yp, 1.0, BX.data_ptr(), bl, BY.data_ptr(), m, 2, None) == -1
    assert untouched()


# ---- 6. the ledger --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m,density", [("nested_mid", 7, 0.05), ("arrow_big", 130, 0.002)])
def test_ledger(name, m, density):
    """the workspace of a shape is (ceil(blklen / p) + 2) * 16 * m doubles, p = 2048 ceil(blklen / 2^22),
    allocated at the first block call and kept"""
    symb, msk, L, Y, sys = _device_case(name, m, 12, density)
    bl = symb.blklen
    solve = sys.factor_qr(L, Y)
    rng = np.random.default_rng(13)
    BX0 = torch.from_numpy(rng.standard_normal((9, bl)) * msk).cuda()
    BY0 = torch.from_numpy(rng.standard_normal((9, m))).cuda()
    solve(cspmatrix(symb, BX0[0].clone()), BY0[0].clone(), 1.0)
    before = symb.device_bytes()
    sys.solve_many_qr(L, Y, BX0[:2].clone(), BY0[:2].clone(), 1.0)
    first = symb.device_bytes()
    p = 2048 * -(-bl // 2 ** 22)
    stated = 8 * (-(-bl // p) + 2) * 16 * m
    print("%s m %d: ledger %d -> %d bytes, stated workspace %d" % (name, m, before, first, stated))
    assert 0 < first - before <= stated
    for k in (2, 9, 1):
        sys.solve_many_qr(L, Y, BX0[:k].clone(), BY0[:k].clone(), 0.5)
        assert symb.device_bytes() == first, k


# ---- 7. deferred status -----------------------------------------------------------------------------------------------------
def test_deferred_status():
    """chordal.lazy_status: a Y whose chol(Y_AA) fails inside the block call (the matrix was changed in place after factor_qr, so
    the cached factors are formed again) is latched and raises from check_status; a clean block call leaves nothing behind."""
    m = 7
    symb, msk, L, Y, sys = _device_case("nested_mid", m, 12, 0.05)
    bl = symb.blklen
    rng = np.random.default_rng(4)
    BX0 = torch.from_numpy(rng.standard_normal((5, bl)) * msk).cuda()
    BY0 = torch.from_numpy(rng.standard_normal((5, m))).cuda()
    sys.factor_qr(L, Y)
    x1, y1 = sys.solve_many_qr(L, Y, BX0.clone(), BY0.clone(), 0.7)
    chordal.lazy_status(symb, True)
    try:
        x2, y2 = sys.solve_many_qr(L, Y, BX0.clone(), BY0.clone(), 0.7)
        chordal.check_status(symb)                        # nothing failed, nothing latched
        for r in range(5):                                # (the bound of the same test of solve_many)
            assert rel(x2[r].cpu().numpy()[msk], x1[r].cpu().numpy()[msk]) < 1e-9 and rel(y2[r].cpu().numpy(), y1[r].cpu().numpy()) < 1e-9
        Y.blkval.neg_()                                   # negative definite separator blocks: every chol(Y_AA) fails
        sys.solve_many_qr(L, Y, BX0.clone(), BY0.clone(), 0.7)      # no hang, no fault; the verdict waits
        with pytest.raises(ArithmeticError):
            chordal.check_status(symb)
        Y.blkval.neg_()
        x3, y3 = sys.solve_many_qr(L, Y, BX0.clone(), BY0.clone(), 0.7)     # the context recovers
        chordal.check_status(symb)
        for r in range(5):
            assert rel(x3[r].cpu().numpy()[msk], x1[r].cpu().numpy()[msk]) < 1e-9 and rel(y3[r].cpu().numpy(), y1[r].cpu().numpy()) < 1e-9
    finally:
        chordal.lazy_status(symb, False)
