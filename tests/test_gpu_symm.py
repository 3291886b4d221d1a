"""chordal.symm on the device (csrc/front_symm.hip) against the dense definition alpha Xd B + beta C in numpy, with the
componentwise rounding bound of tests/symm_ref.py; its contract (same bits from call to call, X, B and the paddings of B
and C untouched, zero-factor terms left out) is asserted on every call of the helper.  The slots of blkval outside the
pattern (the strict upper triangles of the diagonal blocks) hold NaN: they are not part of X."""
import numpy as np
import pytest
import scipy.linalg as sla
import torch

from smcp_amd import _lib, chordal
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic
from tests.helpers import EXTRA, GPU_PATTERNS, launch_counts, padded
from tests.symm_ref import EPS, composed_bound, contribution_index, dense_symm, matrix_input, symm_bound
from tests.trmm_ref import factor_input

pytestmark = pytest.mark.gpu

NRHS = (1, 7, 8, 17, 70)       # below, at and above the tile gate; one past a 16-column block; two 64-column tiles, the second ragged
AB = ((1.0, 0.0), (-0.5, 1.0), (2.0, -0.25))
NAN = float("nan")
CASES = {}


class Case:
    """per pattern, built once: Symbolic on the device, X with NaN outside the pattern, its dense form, an all-NaN matrix"""

    def __init__(self, name):
        self.symb = symb = Symbolic((GPU_PATTERNS.get(name) or EXTRA[name])())
        symb.device_init(0, 1)
        self.blk, self.Xd = matrix_input(symb, seed=5)
        self.X = cspmatrix(symb, torch.from_numpy(self.blk).cuda())
        self.Xnan = cspmatrix(symb, torch.full_like(self.X.blkval, NAN))


def case(name):
    if name not in CASES:
        CASES[name] = Case(name)
    return CASES[name]


def device_symm(name, B, C, padb, padc, alpha, beta):
    """One product on the device, with the contract checked: returns the n x nrhs result.  C is not used for beta == 0:
    the product then goes into a NaN-filled block."""
    cs = case(name)
    n, nrhs = B.shape
    Bv, Bfull = padded(B, padb)
    b0 = Bfull.clone()
    before = cs.X.blkval.clone()
    state = cs.X.state()
    C0 = np.full((n, nrhs), NAN) if beta == 0 else C
    outs = []
    for _ in range(2):                                               # the same call twice, each on a fresh copy of C
        Cv, Cfull = padded(C0, padc)
        assert chordal.symm(cs.X, Bv, Cv, alpha, beta) is Cv
        assert bool((Cfull[:, n:] == 7.25).all())                    # padding of C untouched
        outs.append(Cv.clone())
    assert bool(torch.isfinite(outs[0]).all())                       # beta == 0: C was not read
    assert torch.equal(outs[0], outs[1])                             # deterministic
    assert torch.equal(torch.nan_to_num(before, nan=3.0), torch.nan_to_num(cs.X.blkval, nan=3.0))       # X bit for bit
    assert cs.X.state() == state
    assert torch.equal(Bfull, b0)                                    # B and its padding bit for bit
    # alpha == 0: neither X nor B is read, beta == 1 returns C bit for bit; alpha == beta == 0: exact zeros
    Bn, _ = padded(np.full((n, nrhs), NAN), padb)
    keep = np.random.default_rng(77).standard_normal((n, nrhs))
    Cv, Cfull = padded(keep, padc)
    c0 = Cfull.clone()
    chordal.symm(cs.Xnan, Bn, Cv, 0.0, 1.0)
    assert torch.equal(Cfull, c0)
    Cv, Cfull = padded(np.full((n, nrhs), NAN), padc)
    chordal.symm(cs.Xnan, Bn, Cv, 0.0, 0.0)
    assert bool((Cv == 0.0).all()) and bool((Cfull[:, n:] == 7.25).all())
    return outs[0].cpu().numpy().T


def check_definition(name, nrhs_list=NRHS):
    cs = case(name)
    n = cs.symb.n
    worst = 0.0
    combo = 0
    for nrhs in nrhs_list:
        for alpha, beta in AB:
            padb, padc = 3 * (combo % 2), 3 * ((combo // 2) % 2)     # ldb and ldc: n or n + 3, all four pairs
            combo += 1
            rng = np.random.default_rng(100 + combo)
            B = rng.standard_normal((n, nrhs))
            C = rng.standard_normal((n, nrhs))
            got = device_symm(name, B, C, padb, padc, alpha, beta)
            ref = dense_symm(cs.Xd, B, C, alpha, beta)
            bound = symm_bound(cs.Xd, B, C, alpha, beta)
            ratio = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
            worst = max(worst, ratio)
            print("%s nrhs %d alpha %g beta %g: |got - ref| / bound %.3f" % (name, nrhs, alpha, beta, ratio))
            assert (np.abs(got - ref) <= bound).all(), (name, nrhs, alpha, beta, ratio)
    print("%s: largest |got - ref| / bound %.3f" % (name, worst))


@pytest.mark.parametrize("name", sorted(GPU_PATTERNS) + ["two_components", "one_clique", "wide_arrow"])
def test_definition(name):
    """dense200: 4 chunks, 1 part; dense600: 10 chunks, 3 parts, skipped items; arrow_big: ragged separator chunks;
    wide_arrow: 149 column partials and more per arrow row, the wave-per-entry combine."""
    if name == "wide_arrow":
        assert int(np.diff(contribution_index(case(name).symb)[0]).max()) > 128
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
    """band has 27 levels, nested_mid 4: a call is two launches when one route takes every front and three when small and
    large fronts take different ones, all of this product's kernels, and trees on the same route take the same number."""
    levels = {}
    by_route = {}
    for name in ("band", "rand2", "nested_mid", "arrow_big"):
        cs = case(name)
        levels[name] = cs.symb.nlev
        for nrhs in (1, 8, 70):
            B = np.random.default_rng(9).standard_normal((cs.symb.n, nrhs))
            Bv, _ = padded(B, 0)
            Cv = chordal.symm(cs.X, Bv)                              # (workspaces grown outside the count)
            cnt = launch_counts(cs.symb, lambda: chordal.symm(cs.X, Bv, Cv))
            total = sum(cnt.values())
            print(name, nrhs, cnt)
            assert 2 <= total <= 3, (name, nrhs, cnt)
            assert all(k.startswith("k_symm_") for k in cnt) and cnt.get("k_symm_combine") == 1, cnt
            assert (total == 3) == ("k_symm_fma" in cnt and "k_symm_mm" in cnt), cnt
            by_route.setdefault((nrhs, tuple(sorted(cnt))), set()).add(total)
            if nrhs == 1:
                assert cnt == {"k_symm_fma": 1, "k_symm_combine": 1}, cnt
            if nrhs == 70:
                assert cnt == {"k_symm_mm": 1, "k_symm_combine": 1}, cnt
    assert levels["band"] > levels["rand2"] > levels["nested_mid"] >= 3
    for key, totals in by_route.items():
        assert len(totals) == 1, (key, totals)


@pytest.mark.parametrize("name", ["arrow", "nested_mid", "dense200"])
def test_product_with_llt_is_two_products_with_the_factor(name):
    """S = llt(L): symm(S, B) against trmm N (trmm T (B)), within the sum of the three calls' bounds in terms of
    |Ld| |Ld^T| |B| (symm_ref.composed_bound)."""
    symb = case(name).symb
    blk, Ld = factor_input(symb, seed=5)
    L = cspmatrix(symb, torch.from_numpy(blk).cuda())
    S = cspmatrix(symb, torch.from_numpy(np.nan_to_num(blk, nan=0.0)).cuda())
    chordal.llt(S)
    for nrhs in (3, 20):
        B = np.random.default_rng(31).standard_normal((symb.n, nrhs))
        Bv, _ = padded(B, 0)
        got = chordal.symm(S, Bv).cpu().numpy().T
        chordal.trmm(L, Bv, 1.0, "T")
        chordal.trmm(L, Bv, 1.0, "N")
        two = Bv.cpu().numpy().T
        bound = composed_bound(Ld, B)
        ratio = float((np.abs(got - two) / np.maximum(bound, 1e-300)).max())
        print("%s nrhs %d: |symm - trmm trmm| / bound %.3f" % (name, nrhs, ratio))
        assert (np.abs(got - two) <= bound).all()


def spd_input(symb, seed):
    """(blkval with NaN outside the pattern, dense Xd): matrix_input with the diagonal raised to make every row dominant"""
    blk, Xd = matrix_input(symb, seed)
    d = np.abs(Xd).sum(axis=1) - np.abs(np.diag(Xd)) + 1.0
    Xd[np.diag_indices(symb.n)] = d
    cp, _ = symb.sparsity_pattern()
    blk[np.asarray(symb.ccs_to_blk())[np.asarray(cp[:-1])]] = d
    return blk, Xd


@pytest.mark.parametrize("name", ["arrow", "nested_mid", "dense200", "arrow_big"])
def test_true_residual_of_a_solve(name):
    """R = X W - B for W = L^-T L^-1 B, L = cholesky(X): the residual that trmm cannot give.  The rule of
    test_gpu_trmm.py::test_round_trip_with_trsm: within max(1e-10, 100 x the residual of scipy's cho_solve)."""
    symb = case(name).symb
    blk, Xd = spd_input(symb, seed=8)
    X = cspmatrix(symb, torch.from_numpy(blk).cuda())
    L = cspmatrix(symb, torch.from_numpy(np.nan_to_num(blk, nan=0.0)).cuda())
    chordal.cholesky(L)
    cho = sla.cho_factor(Xd, lower=True)
    for nrhs in (4, 70):
        B = np.random.default_rng(21 + nrhs).standard_normal((symb.n, nrhs))
        Bv, _ = padded(B, 0)
        W = Bv.clone()
        chordal.trsm(L, W, "N")
        chordal.trsm(L, W, "T")
        R = chordal.symm(X, W, C=Bv.clone(), alpha=1.0, beta=-1.0)
        err = float(R.abs().max()) / np.abs(B).max()
        e_ref = np.abs(Xd @ sla.cho_solve(cho, B) - B).max() / np.abs(B).max()
        print("%s nrhs %d: residual %.2e (scipy %.2e)" % (name, nrhs, err, e_ref))
        assert err <= max(1e-10, 100 * e_ref)


@pytest.mark.parametrize("name", ["rand2", "nested_mid", "arrow_big"])
@pytest.mark.parametrize("k", [1, 5, 40])
def test_adjoint_identity_with_syr2k(name, k):
    """<X, P_V(U V^T + V U^T)> = 2 sum (U o (X V)): dot and syr2k on the left, symm on the right.  Tolerance
    2 (n + 2k + 4) 2^-53 times the sum of the absolute values of the terms."""
    cs = case(name)
    symb, n = cs.symb, cs.symb.n
    Xz = cspmatrix(symb, torch.from_numpy(np.nan_to_num(cs.blk, nan=0.0)).cuda())
    U = np.random.default_rng(21).standard_normal((n, k))
    V = np.random.default_rng(22).standard_normal((n, k))
    Uv, _ = padded(U, 0)
    Vv, _ = padded(V, 3)
    Z = cspmatrix(symb, torch.full_like(cs.X.blkval, NAN))
    chordal.syr2k(Z, Uv, Vv, 1.0, 0.0)
    lhs = chordal.dot(Xz, Z)
    rhs = 2.0 * float((Uv * chordal.symm(cs.X, Vv)).sum())
    aX = np.abs(cs.Xd)
    terms = float((aX * (np.abs(U) @ np.abs(V).T + np.abs(V) @ np.abs(U).T)).sum()) + 2.0 * float((np.abs(U) * (aX @ np.abs(V))).sum())
    tol = 2.0 * (n + 2 * k + 4) * EPS * terms
    print("%s k %d: lhs %.15e rhs %.15e tol %.2e" % (name, k, lhs, rhs, tol))
    assert abs(lhs - rhs) <= tol


def test_diagonal_pattern_is_one_rounding():
    """every clique 1 x 1 without a separator: beta = 0 gives alpha (x_ii b_i), one product and the rounding of alpha"""
    cs = case("diag")
    assert cs.symb.Nsn == cs.symb.n and cs.symb.sepptr[-1] == 0
    d = np.diag(cs.Xd)[:, None]
    for alpha in (1.0, -0.5, 2.0):
        B = np.random.default_rng(41).standard_normal((cs.symb.n, 5))
        got = device_symm("diag", B, None, 3, 0, alpha, 0.0)
        assert np.array_equal(got, alpha * (d * B))                  # alpha a power of two: exactly the rounded product


def test_refusals():
    cs = case("arrow")
    symb, n = cs.symb, cs.symb.n
    with pytest.raises(AssertionError):
        chordal.symm(cs.X, torch.zeros((2, n + 1), dtype=torch.float64, device="cuda"))
    with pytest.raises(AssertionError):
        chordal.symm(cs.X, torch.zeros((2, n), dtype=torch.float64, device="cuda"), beta=1.0)      # C=None needs beta == 0
    buf = torch.zeros((6, n), dtype=torch.float64, device="cuda")
    B, C = buf[:2], buf[3:5]
    lib = _lib.lib()
    h, x = symb.handle, cs.X.blkval.data_ptr()
    assert lib.csp_symm(h, x, B.data_ptr(), n, C.data_ptr(), n, 0, 1.0, 0.0, None) == -1
    assert lib.csp_symm(h, x, B.data_ptr(), n - 1, C.data_ptr(), n, 2, 1.0, 0.0, None) == -1
    assert lib.csp_symm(h, x, B.data_ptr(), n, C.data_ptr(), n - 1, 2, 1.0, 0.0, None) == -1
    assert lib.csp_symm(h, x, B.data_ptr(), n, B.data_ptr(), n, 2, 1.0, 0.0, None) == -1                 # C is B
    assert lib.csp_symm(h, x, B.data_ptr(), n, buf[1:3].data_ptr(), n, 2, 1.0, 0.0, None) == -1          # C overlaps B
    assert lib.csp_symm(h, x, B.data_ptr(), n, buf[2:4].data_ptr(), n, 2, 1.0, 0.0, None) == 0           # side by side
    torch.cuda.synchronize()
    assert bool((buf == 0.0).all())


@pytest.mark.parametrize("name", ["nested_mid", "arrow_big"])
def test_caches_are_kept(name):
    """symm reads X and drops nothing the library derived from it.  Under TUNE_DETERMINISTIC (bit-for-bit comparisons need
    the fixed-order route): cholesky of a copy of X, and a Hessian with the cached separator factors of the scaling point
    (L, Y), give the same bits before and after symm calls on X, L and Y, whose state() does not change."""
    symb = case(name).symb
    blk, _ = spd_input(symb, seed=8)
    X = cspmatrix(symb, torch.from_numpy(np.nan_to_num(blk, nan=0.0)).cuda())
    B = np.random.default_rng(3).standard_normal((symb.n, 9))
    Bv, _ = padded(B, 0)
    rhs = torch.from_numpy(np.nan_to_num(case(name).blk, nan=0.0)).cuda()

    def factor():
        M = X.copy()
        chordal.cholesky(M)
        return M.blkval.clone()

    def hessian(L, Y):
        R = cspmatrix(symb, rhs.clone())
        chordal.hessian(L, Y, R, adj=False, inv=False)
        return R.blkval.clone()

    chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 1)
    try:
        first = factor()
        L = X.copy()
        chordal.cholesky(L)
        Y = L.copy()
        chordal.projected_inverse(Y)
        h0 = hessian(L, Y)                                           # caches for the pair at these addresses now exist
        states = [M.state() for M in (X, L, Y)]
        outs = [chordal.symm(M, Bv) for M in (X, L, Y)]
        assert all(bool(torch.isfinite(o).all()) for o in outs)
        assert [M.state() for M in (X, L, Y)] == states
        assert torch.equal(factor(), first)
        assert torch.equal(hessian(L, Y), h0)
    finally:
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 0)
