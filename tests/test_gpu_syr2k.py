"""chordal.syr2k / syrk / syr2 on the device (csrc/front_syr2k.hip) against the dense definition
beta Xd + alpha mask o (U V^T + V U^T) in numpy, with the componentwise rounding bound of tests/syr2k_ref.py.  The
contract is asserted on every call of the helper: the slots of blkval outside the pattern hold NaN on entry and exactly
0.0 on exit, beta = 0 on an all-NaN X gives a finite result, U, V and their padding stay bit for bit, the same call gives
the same bits twice, alpha = 0, beta = 1 leaves the owned slots bit for bit, alpha = beta = 0 gives exact zeros."""
import ctypes

import numpy as np
import pytest
import torch

from smcp_amd import _lib, chordal, problems
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic
from tests import helpers
from tests.helpers import GPU_PATTERNS, PATTERNS, launch_counts, random_block
from tests.syr2k_ref import EPS, dense_syr2k, lower_index, matrix_input, owned, pattern_mask, syr2k_bound
from tests.test_mrcompletion_host import low_rank_on_V, mrcompletion as mrc_numpy, pd_on_V

pytestmark = pytest.mark.gpu

RANKS = (1, 3, 8, 17, 70)      # below, at and above the tile gate; 2k = 6 and 34 are no multiples of 4; 2k = 140: more than two k-slices per operand half
AB = ((1.0, 0.0), (-0.5, 1.0), (2.0, -0.25))
FORMS = ("syr2k", "syrk", "alias")
CASES = {}


EXTRA = {name: helpers.EXTRA[name] for name in ("two_components", "one_clique")}


class Case:
    """per pattern, built once: Symbolic on the device, the input matrix (NaN outside the pattern), masks and indices"""

    def __init__(self, name):
        self.symb = symb = Symbolic((GPU_PATTERNS.get(name) or EXTRA[name])())
        symb.device_init(0, 1)
        self.blk, self.Xd = matrix_input(symb, seed=5)
        self.own = owned(symb)
        self.own_d = torch.from_numpy(self.own).cuda()
        self.mask = pattern_mask(symb)
        self.I, self.J = lower_index(symb)
        self.c2b = symb.ccs_to_blk()
        self.blk_d = torch.from_numpy(self.blk).cuda()


def case(name):
    if name not in CASES:
        CASES[name] = Case(name)
    return CASES[name]


def call(X, form, Uv, Vv, alpha, beta):
    if form == "syrk":
        chordal.syrk(X, Uv, alpha, beta)
    else:
        chordal.syr2k(X, Uv, Uv if form == "alias" else Vv, alpha, beta)


def device_update(cs, form, Uv, Ufull, Vv, Vfull, alpha, beta):
    """One update on the device with the contract checked: returns blkval (numpy)."""
    symb = cs.symb
    start = torch.full_like(cs.blk_d, float("nan")) if beta == 0 else cs.blk_d      # beta = 0: X is not read at all
    u0, v0 = Ufull.clone(), Vfull.clone()
    outs = []
    for _ in range(2):                                               # the same call twice, each on a fresh copy of X
        X = cspmatrix(symb, start.clone())
        call(X, form, Uv, Vv, alpha, beta)
        outs.append(X.blkval)
    assert bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0], outs[1])                             # deterministic
    assert bool((outs[0][~cs.own_d] == 0.0).all())                   # NaN on entry, exactly zero on exit
    X = cspmatrix(symb, cs.blk_d.clone())
    call(X, form, Uv, Vv, 0.0, 1.0)
    assert torch.equal(X.blkval[cs.own_d], cs.blk_d[cs.own_d]) and bool((X.blkval[~cs.own_d] == 0.0).all())
    call(X, form, Uv, Vv, 0.0, 0.0)
    assert bool((X.blkval == 0.0).all())
    assert torch.equal(Ufull, u0) and torch.equal(Vfull, v0)         # U, V and their padding bit for bit
    return outs[0].cpu().numpy()


def check_definition(name, ranks=RANKS):
    cs = case(name)
    n = cs.symb.n
    worst = 0.0
    combo = 0
    for k in ranks:
        for form in FORMS:
            for alpha, beta in AB:
                pad = 3 * (combo % 2)                                # ldu = ldv = n on one half of the cases, n + 3 on the other
                combo += 1
                U, Uv, Ufull = random_block(n, k, pad, 100 + combo)
                V, Vv, Vfull = random_block(n, k, pad, 500 + combo)
                got = device_update(cs, form, Uv, Ufull, Vv, Vfull, alpha, beta)
                Vr = None if form == "syrk" else (U if form == "alias" else V)
                ref = dense_syr2k(cs.Xd, cs.mask, U, Vr, alpha, beta)
                bound = syr2k_bound(cs.Xd, U, Vr, alpha, beta)
                err = np.abs(got[cs.c2b] - ref[cs.I, cs.J])
                bd = bound[cs.I, cs.J]
                ratio = float((err / np.maximum(bd, 1e-300)).max())
                worst = max(worst, ratio)
                assert (err <= bd).all(), (name, k, form, alpha, beta, ratio)
    print("%s: largest |got - ref| / bound %.3f" % (name, worst))


@pytest.mark.parametrize("name", sorted(GPU_PATTERNS) + sorted(EXTRA))
def test_definition(name):
    cs = case(name)
    if name == "two_components":
        assert int((np.asarray(cs.symb.snpar) < 0).sum()) >= 2
    if name == "one_clique":
        assert cs.symb.Nsn == 1
    check_definition(name)


@pytest.mark.parametrize("name", ["arrow_big", "nested_mid", "dense600", "three_tops"])
def test_generic_route(name):
    symb = case(name).symb
    chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 1)
    try:
        check_definition(name)
    finally:
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 0)


def test_launch_count_does_not_depend_on_the_tree():
    """band has 27 levels, rand2 7, nested_mid 4: a call is at most two launches on each; one FMA launch at k = 1."""
    levels = {}
    for name in ("band", "rand2", "nested_mid"):
        cs = case(name)
        symb = cs.symb
        levels[name] = symb.nlev
        for k in (1, 8, 70):
            _, Uv, _ = random_block(symb.n, k, 0, 9)
            _, Vv, _ = random_block(symb.n, k, 0, 10)
            X = cspmatrix(symb, cs.blk_d.clone())
            for form in FORMS:
                call(X, form, Uv, Vv, 0.5, 0.5)                      # (the lists are built outside the count)
                cnt = launch_counts(symb, lambda: call(X, form, Uv, Vv, 0.5, 0.5))
                print(name, k, form, cnt)
                assert 1 <= sum(cnt.values()) <= 2, (name, k, form, cnt)
                assert all(kn.startswith("k_syr2k_") for kn in cnt), cnt
                if k == 1:
                    assert cnt == {"k_syr2k_fma": 1}, cnt
    assert levels["band"] > levels["rand2"] > levels["nested_mid"] >= 3


@pytest.mark.parametrize("name", ["rand2", "arrow_big"])
def test_syr2_is_syr2k_with_one_rank(name):
    cs = case(name)
    n = cs.symb.n
    _, Uv, _ = random_block(n, 1, 0, 11)
    _, Vv, _ = random_block(n, 1, 0, 12)
    A = cspmatrix(cs.symb, cs.blk_d.clone())
    B = cspmatrix(cs.symb, cs.blk_d.clone())
    chordal.syr2(A, Uv[0], Vv[0], -0.5, 2.0)
    chordal.syr2k(B, Uv, Vv, -0.5, 2.0)
    assert bool(torch.isfinite(A.blkval).all()) and torch.equal(A.blkval, B.blkval)


@pytest.mark.parametrize("name", ["rand2", "nested_mid", "arrow_big"])
@pytest.mark.parametrize("k", [1, 5, 40])
def test_adjoint_identity_with_trmm(name, k):
    """<W, P_V(U V^T + V U^T)> = 2 sum_r u_r^T (W v_r), the right side from code that exists: W V = tril(W) V + tril(W)^T V
    - diag(W) V by two trmm calls.  Tolerance 2 (n + 2k + 4) 2^-53 times the sum of the absolute values of the terms."""
    cs = case(name)
    symb, n = cs.symb, cs.symb.n
    W = cspmatrix(symb, torch.from_numpy(np.nan_to_num(cs.blk, nan=0.0)).cuda())
    U, Uv, _ = random_block(n, k, 0, 21)
    V, Vv, _ = random_block(n, k, 3, 22)
    Z = cspmatrix(symb, torch.full_like(cs.blk_d, float("nan")))
    chordal.syr2k(Z, Uv, Vv, 1.0, 0.0)
    lhs = chordal.dot(W, Z)
    WN, WT = Vv.clone(), Vv.clone()
    chordal.trmm(W, WN, 1.0, "N")
    chordal.trmm(W, WT, 1.0, "T")
    WV = WN + WT - W.diag().unsqueeze(0) * Vv
    rhs = 2.0 * float((Uv * WV).sum())
    aW = np.abs(cs.Xd)
    terms = float((aW * (np.abs(U) @ np.abs(V).T + np.abs(V) @ np.abs(U).T)).sum()) + 2.0 * float((np.abs(U) * (aW @ np.abs(V))).sum())
    tol = 2.0 * (n + 2 * k + 4) * EPS * terms
    exact = 2.0 * float((U * (cs.Xd @ V)).sum())
    print("%s k %d: lhs %.15e rhs %.15e numpy %.15e tol %.2e" % (name, k, lhs, rhs, exact, tol))
    assert abs(lhs - rhs) <= tol and abs(lhs - exact) <= tol


@pytest.mark.parametrize("name", sorted(PATTERNS))
@pytest.mark.parametrize("k", [1, 3, 8, None])
def test_round_trip_with_mrcompletion(name, k):
    """The inputs and the tolerance of tests/test_gpu_mrcompletion.py::test_parity_patterns: syrk of the factor Y that
    mrcompletion returns reproduces X on the pattern."""
    from tests.test_gpu_mrcompletion import residual_blk
    cs = case(name)
    symb = cs.symb
    blk = pd_on_V(symb, seed=7) if k is None else low_rank_on_V(symb, k, seed=k)
    X = cspmatrix(symb, torch.from_numpy(blk.copy()).cuda())
    Y = chordal.mrcompletion(X)
    Z = cspmatrix(symb, torch.full_like(X.blkval, float("nan")))
    chordal.syrk(Z, Y.t().contiguous(), 1.0, 0.0)
    Yr, _ = mrc_numpy(symb, blk)
    tol = max(1e-10 * np.abs(blk).max(), 100 * residual_blk(symb, blk, Yr))
    got = Z.blkval.cpu().numpy()
    assert (got[~cs.own] == 0.0).all()
    err = np.abs(got[cs.own] - blk[cs.own]).max()
    print("%s k %s: max |syrk(Y) - X| on V %.2e (tol %.2e)" % (name, k, err, tol))
    assert err <= tol


def scaling_point(symb, M, keep):
    """cholesky in place, Y = projected inverse of a copy: (L, Y)"""
    chordal.cholesky(M)
    Y = M.copy()
    chordal.projected_inverse(Y)
    keep.extend([M, Y])
    return M, Y


def hessian_of(symb, L, Y, rhs):
    R = cspmatrix(symb, rhs.clone())
    chordal.hessian(L, Y, R, adj=False, inv=False)
    return R.blkval.clone()


@pytest.mark.parametrize("name", ["nested_mid", "arrow_big"])
def test_cached_factors_are_dropped(name):
    """The library keeps quantities derived from (L, Y) keyed by ADDRESS.  Bit-for-bit comparisons need the fixed-order
    route (the default extend-adds sum in arrival order), so the test runs under TUNE_DETERMINISTIC, where the Hessian reuses
    the separator blocks of Y and their Cholesky factors from call to call.
    (a) the sequence of the issue: factor a matrix, apply a Hessian, put the original matrix back at the same address, add a
    rank-4 term that is PSD on the pattern with syrk, factor and apply the Hessian again: equal to the same sequence on a fresh matrix at a new address.
    (b) the same with the term added to Y, whose cached separator factors the next Hessian would otherwise reuse."""
    cs = case(name)
    symb, n = cs.symb, cs.symb.n
    S = cspmatrix(symb, torch.from_numpy(problems.random_factor_blkval(symb, 3)).cuda())
    chordal.llt(S)                                                   # positive definite on the pattern
    S0 = S.blkval.clone()
    # four ranks, each supported on the front rows of one clique: U U^T then lies inside the pattern, P_V(U U^T) = U U^T is
    # positive semidefinite itself and the updated matrices stay positive definite (the projection of a general PSD term is
    # only PSD-completable and may leave the cone)
    Un = np.zeros((n, 4))
    for r in range(4):
        c = (r * symb.Nsn) // 4
        F = np.asarray(symb.rowidx[symb.rowptr[c]:symb.rowptr[c + 1]], dtype=np.int64)
        Un[F, r] = np.random.default_rng(31 + r).standard_normal(len(F))
    Uv = torch.from_numpy(np.ascontiguousarray(Un.T)).cuda()
    rhs = torch.from_numpy(np.nan_to_num(cs.blk, nan=0.0)).cuda()
    keep = []
    chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 1)
    try:
        M = cspmatrix(symb, S0.clone())
        addr = M.blkval.data_ptr()
        L, Y = scaling_point(symb, M, keep)
        first = hessian_of(symb, L, Y, rhs)                          # caches for the pair at these addresses now exist
        # (a)
        M.blkval.copy_(S0)
        chordal.syrk(M, Uv, 1.0, 1.0)
        assert M.blkval.data_ptr() == addr
        updated = M.blkval.clone()
        L2, Y2 = scaling_point(symb, M, keep)
        again = hessian_of(symb, L2, Y2, rhs)
        fresh = cspmatrix(symb, updated.clone())
        assert fresh.blkval.data_ptr() != addr
        Lf, Yf = scaling_point(symb, fresh, keep)
        ref = hessian_of(symb, Lf, Yf, rhs)
        assert bool(torch.isfinite(again).all()) and torch.equal(again, ref)
        assert not torch.equal(again, first)
        # (b)
        before = hessian_of(symb, L2, Y2, rhs)                       # caches hold the separator factors of Y2
        chordal.syrk(Y2, Uv, 0.5, 1.0)
        after = hessian_of(symb, L2, Y2, rhs)
        Lc, Yc = L2.copy(), Y2.copy()
        keep.extend([Lc, Yc])
        ref2 = hessian_of(symb, Lc, Yc, rhs)
        assert bool(torch.isfinite(after).all()) and torch.equal(after, ref2)
        assert not torch.equal(after, before)
    finally:
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 0)


def test_error_returns():
    cs = case("arrow")
    symb, n = cs.symb, cs.symb.n
    X = cs.blk_d.clone()
    B = torch.zeros((2, n), dtype=torch.float64, device="cuda")
    lib = _lib.lib()
    p, b = X.data_ptr(), B.data_ptr()
    assert lib.csp_syr2k(symb.handle, p, b, b, 0, n, n, 1.0, 1.0, None) == -1
    assert lib.csp_syr2k(symb.handle, p, b, b, 2, n - 1, n, 1.0, 1.0, None) == -1
    assert lib.csp_syr2k(symb.handle, p, b, b, 2, n, n - 1, 1.0, 1.0, None) == -1
    assert lib.csp_syr2k(symb.handle, p, b, None, 2, n, 0, 1.0, 1.0, None) == 0          # syrk: ldv is ignored
    torch.cuda.synchronize()
