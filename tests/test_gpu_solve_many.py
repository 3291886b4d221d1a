"""KKTSystem.solve_many / kkt_solve_many / dense_potrs_many: the Newton-KKT solve (solvers.py:506-541) for a block of
right-hand sides on one factorisation -- the dense block solve against numpy, the whole route against the oracle and against
the single solve_, isolation of the rows, launch counts, refusals and the deferred status regime."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from smcp_amd import _lib, chordal, problems, shard
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.kkt import KKTSystem, solve_many_chunks
from smcp_amd.symbolic import Symbolic
from tests.helpers import GPU_PATTERNS, launch_counts
from tests.test_gpu_parity import dev, host, rel, setup

pytestmark = pytest.mark.gpu

NEW_KERNELS = ("k_potrs_many_small", "k_potrs_many_step", "k_aadj_sub_many", "k_kkt_many_y", "k_kkt_many_scale")
SENT = -7.25e77           # padding sentinel: must come back bit for bit


# ---- 1. the dense block solve against numpy -------------------------------------------------------------------------
def _colmajor(M, ld, fill):
    """device image of the column-major matrix M with ld rows: row r of the array is column r"""
    n = M.shape[0]
    out = np.full((M.shape[1], ld), fill)
    out[:, :n] = M.T
    return torch.from_numpy(out).cuda()


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 128, 129, 200, 1100])
def test_dense_block_solve_against_numpy(n):
    """Hh = M M^T + n I, the recipe and bound (1e-10 relative, here per column) of test_dense_potrf_potrs: the one-workgroup
    class, both sides of every 64-block edge, ragged last blocks, one size beyond POTRS1_MAXN; both sides of eight columns
    and one past sixteen; padded leading dimensions; a factor from dense_potrf and one uploaded with NaN above the diagonal."""
    lib = _lib.lib()
    symb = Symbolic(GPU_PATTERNS["band"]())
    chordal._ensure(symb)
    h = symb.handle
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n))
    Hh = M @ M.T + n * np.eye(n)
    Ball = rng.standard_normal((n, 17))
    Zref = np.linalg.solve(Hh, Ball)
    Lnan = np.linalg.cholesky(Hh)
    Lnan[np.triu_indices(n, 1)] = np.nan
    for lda in (n, n + 3):
        Hd = _colmajor(Hh, lda, SENT)
        assert lib.dense_potrf(h, Hd.data_ptr(), n, lda, None) == 0
        for src, A in (("potrf", Hd), ("upload", _colmajor(Lnan, lda, SENT))):
            if src == "upload":
                lib.kkt_schur_forget(h, Hd.data_ptr())          # the cached diagonal blocks belong to another matrix now
            A0 = A.clone()
            for nrhs in (1, 2, 7, 8, 9, 17):
                for ldb in (n, n + 5):
                    tag = (n, lda, src, nrhs, ldb)
                    B0 = _colmajor(Ball[:, :nrhs], ldb, SENT)
                    B = B0.clone()
                    assert lib.dense_potrs_many(h, A.data_ptr(), n, lda, B.data_ptr(), nrhs, ldb, None) == 0
                    got = B.cpu().numpy()
                    errs = [rel(got[r, :n], Zref[:, r]) for r in range(nrhs)]
                    assert max(errs) < 1e-10, (tag, errs)
                    assert A.view(torch.int64).equal(A0.view(torch.int64)), tag            # NaN-safe bit comparison
                    assert bool((B[:, n:] == SENT).all()), tag
                    B2 = B0.clone()
                    assert lib.dense_potrs_many(h, A.data_ptr(), n, lda, B2.data_ptr(), nrhs, ldb, None) == 0
                    assert torch.equal(B2, B), tag
                    keep = nrhs // 2
                    B3 = B0.clone()
                    B3[:, :n] = float("nan")
                    B3[keep, :n] = B0[keep, :n]
                    assert lib.dense_potrs_many(h, A.data_ptr(), n, lda, B3.data_ptr(), nrhs, ldb, None) == 0
                    assert bool(torch.isfinite(B3[keep, :n]).all()), tag
                    assert torch.equal(B3[keep], B[keep]), tag


# ---- 2. the whole solve against the oracle ----------------------------------------------------------------------------
def _oracle_case(name, m=7):
    symb, S, A, msk = setup(name, 7)
    L = A.copy()
    orc.cholesky(S, L)
    Yh = L.copy()
    orc.projected_inverse(S, Yh)
    cons = problems.random_constraints(symb, m, density=0.05, seed=9)
    return symb, S, msk, L, Yh, cons


def _padded(rows, width, pad):
    t = torch.full((rows.shape[0], width + pad), SENT, dtype=torch.float64, device="cuda")
    t[:, :width] = torch.from_numpy(rows).cuda()
    return t


def _check_rows_against_oracle(K, S, msk, L, Yh, Href, BXh, BYh, kk, gx, gy, refs):
    for r in range(gx.shape[0]):
        xr, yr = refs[r]
        assert rel(gx[r][msk], xr[msk]) < 1e-9, r
        assert rel(gy[r], yr) < 1e-9, r
        res, rr = K.residual(L, Yh, gx[r] * msk, gy[r], BXh[r], BYh[r], kk)
        assert np.sqrt(orc.dot(S, res, res)) / max(1, np.sqrt(orc.dot(S, BXh[r], BXh[r]))) < 1e-10, r
        assert np.linalg.norm(rr) / max(1, np.linalg.norm(BYh[r])) < 1e-10, r


@pytest.mark.parametrize("max_rhs", [3, 12])
@pytest.mark.parametrize("name", ["arrow", "rand2", "nested_mid", "diag", "fam_max", "fam_odd", "nested"])
def test_rows_against_the_oracle(name, max_rhs):
    """The inputs and bounds of test_kkt_factor_and_solve (1e-9 for x on the pattern and y, 1e-10 for the two residuals of
    K.residual), for 1, 2, 5 and 9 rows with padded rows.  max_rhs = 3 on the context setup() made (four rows of workspace):
    five and nine rows go in chunks -- of two on `diag`, whose blkval is shorter than two sets of temporaries."""
    m = 7
    symb, S, msk, L, Yh, cons = _oracle_case(name, m)
    K = orc.KKT(S, *cons)
    Href = K.schur_factor(L, Yh)
    sys = KKTSystem(symb, *cons, max_rhs=max_rhs)
    bl = symb.blklen
    chunks = solve_many_chunks(9, m, bl, symb._max_rhs)
    if max_rhs == 3:
        assert symb._max_rhs == 4 and len(chunks) > 1
        assert chunks[0] == (2 if name == "diag" else 3)
    else:
        # one chunk -- but for `diag`: nine rows and their 63 temporaries need 9 + 5 rows of fifteen doubles
        assert chunks == ([8, 1] if name == "diag" else [9])
    Ld, Yd = dev(symb, L), dev(symb, Yh)
    sys.factor(Ld, Yd)
    rng = np.random.default_rng(8)
    BXh = rng.standard_normal((9, bl)) * msk
    BYh = rng.standard_normal((9, m))
    keep = [t.blkval.clone() for t in (Ld, Yd)] + [sys.H.clone()]
    states = (Ld.state(), Yd.state())
    for kk in (1.0, 0.25):
        refs = [K.solve(L, Yh, Href, BXh[r], BYh[r], kk) for r in range(9)]
        for k in (1, 2, 5, 9):
            BX, BY = _padded(BXh[:k], bl, 3), _padded(BYh[:k], m, 2)
            out = sys.solve_many(Ld, Yd, BX, BY, kk)
            assert out[0] is BX and out[1] is BY
            assert bool((BX[:, bl:] == SENT).all()) and bool((BY[:, m:] == SENT).all())
            _check_rows_against_oracle(K, S, msk, L, Yh, Href, BXh, BYh, kk, BX[:, :bl].cpu().numpy(), BY[:, :m].cpu().numpy(), refs)
    assert torch.equal(Ld.blkval, keep[0]) and torch.equal(Yd.blkval, keep[1]) and torch.equal(sys.H, keep[2])
    assert (Ld.state(), Yd.state()) == states


# ---- 3. block edges of the dense part inside the whole route -------------------------------------------------------------
def _device_case(name, m, max_rhs, density, seed=7):
    symb, S, A, msk = setup(name, seed)
    L = dev(symb, A)
    chordal.cholesky(L)
    Y = L.copy()
    chordal.projected_inverse(Y)
    cons = problems.random_constraints(symb, m, density=density, seed=9)
    sys = KKTSystem(symb, *cons, max_rhs=max_rhs)
    return symb, msk, L, Y, sys


def _device_residuals(symb, sys, L, Y, mskd, x, y, bx, by, kk):
    """the KKT residual as the refinement rounds of the drivers form it (solvers.py:358-364), normalised as in
    test_kkt_factor_and_solve"""
    r = cspmatrix(symb, (x * mskd).clone())
    chordal.hessian(L, Y, r, adj=None, inv=True)
    r.blkval.mul_(-kk)
    r.blkval.add_(sys.aadj(y).blkval)
    r.blkval.sub_(bx)
    r.blkval.mul_(mskd)
    r.touched()
    rr = sys.amap(cspmatrix(symb, (x * mskd).clone())) - by
    B = cspmatrix(symb, bx.clone())
    return (np.sqrt(max(chordal.dot(r, r), 0.0)) / max(1.0, np.sqrt(chordal.dot(B, B))),
            float(torch.linalg.norm(rr)) / max(1.0, float(torch.linalg.norm(by))))


@pytest.mark.parametrize("m", [70, 130])
def test_dense_block_edges_inside_the_route(m):
    """m = 70: the one-workgroup class with a ragged second block; m = 130: three block steps each way, the last two rows wide.
    Each residual of the block solve is at most 10 x the single route's for the same row (a different summation order,
    nothing more), with a floor of 1e-10."""
    kk = 0.25
    symb, msk, L, Y, sys = _device_case("arrow_big", m, 16, 0.002)
    bl = symb.blklen
    assert solve_many_chunks(9, m, bl, symb._max_rhs) == [9]
    solve = sys.factor(L, Y)
    mskd = torch.from_numpy(msk.astype(np.float64)).cuda()
    rng = np.random.default_rng(8)
    BX0 = torch.from_numpy(rng.standard_normal((9, bl)) * msk).cuda()
    BY0 = torch.from_numpy(rng.standard_normal((9, m))).cuda()
    single = []
    for r in range(9):
        bx, by = cspmatrix(symb, BX0[r].clone()), BY0[r].clone()
        solve(bx, by, kk)
        single.append(_device_residuals(symb, sys, L, Y, mskd, bx.blkval, by, BX0[r], BY0[r], kk))
    for k in (3, 9):
        BX, BY = BX0[:k].clone(), BY0[:k].clone()
        sys.solve_many(L, Y, BX, BY, kk)
        for r in range(k):
            got = _device_residuals(symb, sys, L, Y, mskd, BX[r], BY[r], BX0[r], BY0[r], kk)
            print("m %d k %d row %d  block %.3e %.3e   single %.3e %.3e" % ((m, k, r) + got + single[r]))
            assert got[0] <= max(10 * single[r][0], 1e-10), (k, r)
            assert got[1] <= max(10 * single[r][1], 1e-10), (k, r)


# ---- 4. determinism and isolation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m", [("nested_mid", 7), ("arrow_big", 130)])
def test_determinism_and_isolation(name, m):
    symb, msk, L, Y, sys = _device_case(name, m, 12, 0.05 if m == 7 else 0.002)
    bl = symb.blklen
    rng = np.random.default_rng(11)
    BX0 = torch.from_numpy(rng.standard_normal((5, bl)) * msk).cuda()
    BY0 = torch.from_numpy(rng.standard_normal((5, m))).cuda()
    chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 1)
    try:
        solve = sys.factor(L, Y)

        def single():
            bx, by = cspmatrix(symb, BX0[1].clone()), BY0[1].clone()
            solve(bx, by, 0.7)
            return bx.blkval.clone(), by

        def block(BXi, BYi):
            BX, BY = BXi.clone(), BYi.clone()
            sys.solve_many(L, Y, BX, BY, 0.7)
            return BX, BY

        s0 = single()
        a = block(BX0, BY0)
        b = block(BX0, BY0)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])               # the same call twice: the same bits
        BXn, BYn = torch.full_like(BX0, float("nan")), torch.full_like(BY0, float("nan"))
        BXn[3], BYn[3] = BX0[3], BY0[3]
        c = block(BXn, BYn)                                                       # the other rows poisoned
        assert bool(torch.isfinite(c[0][3]).all()) and bool(torch.isfinite(c[1][3]).all())
        assert torch.equal(c[0][3], a[0][3]) and torch.equal(c[1][3], a[1][3])
        s1 = single()                                                             # the single route after block calls
        assert torch.equal(s1[0], s0[0]) and torch.equal(s1[1], s0[1])
    finally:
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 0)


# ---- 5. no host loop over the right-hand sides ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m,density", [("nested_mid", 7, 0.05), ("arrow_big", 130, 0.002)])
def test_launches_do_not_depend_on_the_number_of_rows(name, m, density):
    symb, msk, L, Y, sys = _device_case(name, m, 16, density)
    bl = symb.blklen
    assert solve_many_chunks(8, m, bl, symb._max_rhs) == [8]
    sys.factor(L, Y)
    rng = np.random.default_rng(12)
    counts = {}
    for k in (2, 8):
        BX = torch.from_numpy(rng.standard_normal((k, bl)) * msk).cuda()
        BY = torch.from_numpy(rng.standard_normal((k, m))).cuda()
        sys.solve_many(L, Y, BX.clone(), BY.clone(), 1.0)                         # warm: caches, scratch
        counts[k] = launch_counts(symb, lambda: sys.solve_many(L, Y, BX, BY, 1.0))
        assert "k_dense_potrs" not in counts[k], counts[k]
    new2 = {n: counts[2].get(n, 0) for n in NEW_KERNELS}
    new8 = {n: counts[8].get(n, 0) for n in NEW_KERNELS}
    assert new2 == new8, (new2, new8)
    assert new2["k_kkt_many_y"] == 1 and new2["k_kkt_many_scale"] == 1 and new2["k_aadj_sub_many"] == 1
    if m <= 128:
        assert new2["k_potrs_many_small"] == 1 and new2["k_potrs_many_step"] == 0
    else:
        assert new2["k_potrs_many_small"] == 0 and new2["k_potrs_many_step"] == 2 * ((m + 63) // 64)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = _lib.lib()
    m = 7
    symb, msk, L, Y, sys = _device_case("arrow", m, 12, 0.05)
    bl, h = symb.blklen, symb.handle
    sys.factor(L, Y)
    buf = torch.zeros(4 * bl + 64, dtype=torch.float64, device="cuda")
    BX, BY = buf[:2 * bl].view(2, bl), torch.zeros(2, m, dtype=torch.float64, device="cuda")
    Lp, Yp, Hp = L.blkval.data_ptr(), Y.blkval.data_ptr(), sys.H.data_ptr()

    def call(H=Hp, ldh=m, bx=BX.data_ptr(), ldbx=bl, by=BY.data_ptr(), ldby=m, nrhs=2):
        return lib.kkt_solve_many(h, Lp, Yp, H, ldh, 1.0, bx, ldbx, by, ldby, nrhs, None)

    H0 = sys.H.clone()
    assert call(nrhs=0) == -1
    assert call(ldbx=bl - 1) == -1
    assert call(ldby=m - 1) == -1
    assert call(ldh=m - 1) == -1
    assert call(by=buf[bl:].data_ptr()) == -1                      # BY inside BX
    assert call(by=buf[2 * bl - 1:].data_ptr()) == -1              # ... overlapping its last entry
    assert call(bx=Hp) == -1                                       # BX is H
    assert call(by=sys.H.view(-1)[m * m - 1:].data_ptr(), nrhs=1) == -1      # BY starts at the last entry of H
    torch.cuda.synchronize()
    assert bool((buf == 0.0).all()) and bool((BY == 0.0).all()) and torch.equal(sys.H, H0)     # nothing was written
    assert call(by=buf[2 * bl:].data_ptr()) == 0                   # side by side is fine
    with pytest.raises(ValueError):
        sys.solve_many(L, Y, BX, BY[:1], 1.0)
    with pytest.raises(ValueError):
        sys.solve_many(L, Y, BX[:, :bl - 1], BY, 1.0)
    # the Python method on a sharded pair
    sys.__dict__["_spair"] = (L, Y, (L.state(), Y.state()))
    try:
        with pytest.raises(NotImplementedError):
            sys.solve_many(L, Y, BX, BY, 1.0)
    finally:
        sys.__dict__.pop("_spair", None)
    # a multi-rank partition on the context
    P = shard.subtree_partition(symb, 2)
    owner = np.ascontiguousarray(P.owner, dtype=np.int32)
    assert owner.max() == 1
    assert lib.csp_set_partition(h, owner.ctypes.data, 0) == 0
    assert call() == -1
    # a context without constraints
    bare = Symbolic(GPU_PATTERNS["arrow"]())
    bare.device_init(0, 4)
    assert lib.kkt_solve_many(bare.handle, Lp, Yp, Hp, m, 1.0, BX.data_ptr(), bl, BY.data_ptr(), m, 2, None) == -1


# ---- 7. deferred status ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["arrow", "nested_mid"])
def test_deferred_status(name):
    """chordal.lazy_status: factor leaves H unfactored, solve_many factors it where it stands; the rows agree with the eager run
    to the bounds of the oracle comparison, and a matrix outside the cone ends in ArithmeticError from check_status."""
    m = 7
    symb, S, A, msk = setup(name, 7)
    cons = problems.random_constraints(symb, m, density=0.05, seed=9)
    sys = KKTSystem(symb, *cons, max_rhs=12)
    bl = symb.blklen
    rng = np.random.default_rng(4)
    BX0 = torch.from_numpy(rng.standard_normal((5, bl)) * msk).cuda()
    BY0 = torch.from_numpy(rng.standard_normal((5, m))).cuda()

    def run(mat):
        L = dev(symb, mat)
        chordal.cholesky(L)
        Y = L.copy()
        chordal.projected_inverse(Y)
        sys.factor(L, Y)
        BX, BY = BX0.clone(), BY0.clone()
        sys.solve_many(L, Y, BX, BY, 0.7)
        return BX.cpu().numpy(), BY.cpu().numpy()

    x1, y1 = run(A)
    bad = A.copy()
    bad[symb.blkptr[symb.Nsn // 2]] = -1.0
    chordal.lazy_status(symb, True)
    try:
        x2, y2 = run(A)
        chordal.check_status(symb)                        # nothing failed
        for r in range(5):
            assert rel(x2[r][msk], x1[r][msk]) < 1e-9 and rel(y2[r], y1[r]) < 1e-9
        run(bad)                                          # outside the cone: no hang, no fault
        with pytest.raises(ArithmeticError):
            chordal.check_status(symb)
        x3, y3 = run(A)                                   # the context recovers
        chordal.check_status(symb)
        assert rel(y3, y1) < 1e-9
    finally:
        chordal.lazy_status(symb, False)
