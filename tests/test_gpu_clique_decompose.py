"""chordal.clique_decompose on the device (csrc/front_cdec.hip) against the numpy restatement of
tests/clique_decompose_ref.py and the dense definitions.  L comes from ``cholesky`` of a random positive definite matrix on
the pattern; every slot of L.blkval that holds no entry of the pattern is then set to NaN: the call must not read it.

Bounds (tests/clique_decompose_ref.py): B_k = 2 (nn + 2) 2^-53 |Pt| |Pt|^T per block, one for the device and one for numpy;
2 (n + 4) 2^-53 |L| |L|^T for the sum.  None comes from the code under test.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import smcp_amd
from smcp_amd import _lib, chordal
from smcp_amd.cspmatrix import _stream, cspmatrix
from smcp_amd.symbolic import Symbolic
from tests import clique_decompose_ref as R
from tests import syr2k_ref
from tests.helpers import EXTRA, GPU_PATTERNS, PATTERNS, launch_census, launch_counts

pytestmark = pytest.mark.gpu

SMALL = tuple(PATTERNS) + ("diag", "one_clique", "two_components")
# arrow_thin: inner dimension 2, no multiple of the MFMA k-slice; arrow_big: nf = 192, exactly 3 x 3 tiles, nn = 64;
# dense200: 3 tiles + 8; three_tops and arrow_one: 310-row roots beside thin top fronts
ALL = SMALL + ("arrow_thin", "arrow_big", "dense200", "three_tops", "arrow_one")
CASES = {}
RESULTS = {}


class Case:
    pass


def case(name):
    """built once per pattern and left unchanged: the Symbolic on the device, L with NaN in every unowned slot, its host
    copy, the dense factor, the blocks of the restatement and their bounds"""
    if name not in CASES:
        c = Case()
        c.symb = symb = Symbolic((GPU_PATTERNS.get(name) or EXTRA[name])())
        symb.device_init(0, 1)
        blk0, _ = R.random_factor(symb, seed=21, junk=0.0)
        L = cspmatrix(symb, torch.from_numpy(blk0).cuda())
        chordal.llt(L)                                   # a random positive definite matrix on the pattern
        c.S = L.copy()
        chordal.cholesky(L)
        c.owned = syr2k_ref.owned(symb)
        assert np.array_equal(~c.owned, R.unowned(symb))
        L.blkval[torch.from_numpy(~c.owned).cuda()] = float("nan")
        c.L = L
        c.blk = L.blkval.cpu().numpy()
        c.bits = L.blkval.view(torch.int64).clone()
        c.Ld = R.dense_factor(symb, c.blk)
        assert np.isfinite(c.Ld).all()
        c.ref = R.decompose(symb, c.blk)
        c.B = R.bounds(symb, c.blk)
        c.nn = np.diff(np.asarray(symb.snptr))
        c.mask = R.pattern_mask(symb)
        CASES[name] = c
    return CASES[name]


def run(name, det):
    """the blocks the device gives on the default route (det = 0) or under TUNE_DETERMINISTIC (det = 1), computed once; L is
    bitwise what it was afterwards, NaNs included"""
    if (name, det) not in RESULTS:
        c = case(name)
        chordal.tune(c.symb, chordal.TUNE_DETERMINISTIC, det)
        try:
            Z = chordal.clique_decompose(c.L)
        finally:
            chordal.tune(c.symb, chordal.TUNE_DETERMINISTIC, 0)
        assert torch.equal(c.L.blkval.view(torch.int64), c.bits)
        RESULTS[name, det] = (Z, R.unpack(c.symb, Z.cpu().numpy()))
    return RESULTS[name, det]


@pytest.mark.parametrize("name", ALL)
def test_definition(name):
    c = case(name)
    worst = {}
    for det in (0, 1):
        Z, blocks = run(name, det)
        assert Z.dtype == torch.float64 and Z.is_cuda and Z.shape[0] == int(chordal.clique_ptr(c.symb)[-1])
        assert bool(torch.isfinite(Z).all())
        w = 0.0
        for k, Zk in enumerate(blocks):
            err, B = np.abs(Zk - c.ref[k]), c.B[k]
            w = max(w, float((err[B > 0] / B[B > 0]).max()))
            assert (err <= 2.0 * B).all(), (name, det, k)
            assert np.array_equal(Zk, Zk.T), (name, det, k)          # the two triangles carry the same bits
        worst[det] = w
    both = 0.0
    for k, (Z0, Z1) in enumerate(zip(run(name, 0)[1], run(name, 1)[1])):
        err, B = np.abs(Z0 - Z1), c.B[k]
        both = max(both, float((err[B > 0] / B[B > 0]).max()))
        assert (err <= 2.0 * B).all(), (name, k)
    print("%s: worst |Z - restatement| / B default %.3f deterministic %.3f, between the routes %.3f (bound 2)"
          % (name, worst[0], worst[1], both))


@pytest.mark.parametrize("name", ALL)
def test_l_is_untouched(name):
    c = case(name)
    for det in (0, 1):
        run(name, det)
    assert torch.equal(c.L.blkval.view(torch.int64), c.bits)
    assert np.isnan(c.L.blkval.cpu().numpy()[~c.owned]).all()


@pytest.mark.parametrize("name", ALL)
def test_sum(name):
    c = case(name)
    symb = c.symb
    bound = R.sum_bound(c.Ld)
    LLt = c.Ld @ c.Ld.T
    L2 = cspmatrix(symb, c.L.blkval.clone())
    L2.blkval[torch.from_numpy(~c.owned).cuda()] = 0.0               # (llt reads whole panels)
    chordal.llt(L2)
    M2 = syr2k_ref.to_dense(symb, L2.blkval.cpu().numpy())
    for det in (0, 1):
        X = chordal.clique_scatter(symb, run(name, det)[0], "sum")
        M = syr2k_ref.to_dense(symb, X.blkval.cpu().numpy())
        e1, e2 = np.abs(M - LLt)[c.mask], np.abs(M - M2)[c.mask]
        b = bound[c.mask]
        print("%s det=%d: worst sum error / bound %.3f (dense), %.3f (llt, bound 2)" % (name, det, (e1 / b).max(), (e2 / b).max()))
        assert (e1 <= b).all() and (e2 <= 2.0 * b).all()


@pytest.mark.parametrize("name", SMALL + ("arrow_thin", "arrow_big"))
def test_cone_membership_and_rank(name):
    c = case(name)
    for det in (0, 1):
        worst = (0.0, 0.0)
        for k, Zk in enumerate(run(name, det)[1]):
            lam, tail = R.cone_defects(Zk, c.B[k], int(c.nn[k]))
            worst = (max(worst[0], lam), max(worst[1], tail))
            assert lam <= 2.0 and tail <= 2.0, (name, det, k, lam, tail)
        print("%s det=%d: worst -lambda_min / |B|_F %.3f, sigma_(nn+1) / |B|_F %.3f (bound 2)" % ((name, det) + worst))


def test_a_wrong_decomposition_fails_the_cone_test():
    """the gathered blocks of L L^T divided by the multiplicity sum to the same matrix and are no such decomposition"""
    c = case("arrow")
    symb = c.symb
    G = chordal.clique_gather(c.S)
    mult = chordal.clique_gather(cspmatrix(symb, chordal.clique_multiplicity(symb).clone()))
    wrong = G / mult
    back = chordal.clique_scatter(symb, wrong, "sum").blkval.cpu().numpy()
    want = c.S.blkval.cpu().numpy()
    assert np.allclose(back[c.owned], want[c.owned], rtol=1e-13, atol=0)
    defects = [R.cone_defects(Zk, c.B[k], int(c.nn[k])) for k, Zk in enumerate(R.unpack(symb, wrong.cpu().numpy()))]
    assert max(max(d) for d in defects) > 2.0


@pytest.mark.parametrize("name", ALL)
def test_duality(name):
    c = case(name)
    symb = c.symb
    xblk, Xd = syr2k_ref.matrix_input(symb, seed=31, junk=0.0)
    G = chordal.clique_gather(cspmatrix(symb, torch.from_numpy(xblk).cuda())).cpu().numpy().astype(np.longdouble)
    aL = np.abs(c.Ld)
    nfmax = int(np.diff(np.asarray(symb.rowptr)).max())
    want = float((Xd * (c.Ld @ c.Ld.T)).astype(np.longdouble).sum())     # (numpy's own rounding is inside the bound)
    bound = 2.0 * (symb.n + nfmax + 4) * R.EPS * float((np.abs(Xd) * (aL @ aL.T)).sum())
    for det in (0, 1):
        got = float(np.dot(G, run(name, det)[0].cpu().numpy().astype(np.longdouble)))
        print("%s det=%d: |sum <X_gg, Z_k> - <X, L L^T>| / bound %.3g" % (name, det, abs(got - want) / bound))
        assert abs(got - want) <= bound


def test_launches():
    """one or two launches whatever the tree, under the borrowed kernel names: the deep band counts what the single clique
    counts; the launch census names the kernels behind the ids, k_cdec_fma (items) and k_cdec_mm (tiles)"""
    for name in ("band", "dense"):
        c = case(name)
        run(name, 0)                                                  # (the plan is built outside the count)
        assert launch_counts(c.symb, lambda: chordal.clique_decompose(c.L)) == {"k_syr2k_fma": 1}
        assert launch_census(c.symb, lambda: chordal.clique_decompose(c.L))[1] == {"k_cdec_fma": 1}
    c = case("arrow_big")
    run("arrow_big", 0)
    counts, census = launch_census(c.symb, lambda: chordal.clique_decompose(c.L))
    print("arrow_big", counts, census)
    assert counts.get("k_syr2k_mm", 0) == 1 and counts.get("k_syr2k_fma", 0) <= 1 and set(counts) <= {"k_syr2k_mm", "k_syr2k_fma"}
    assert census.get("k_cdec_mm", 0) == 1 and census.get("k_cdec_fma", 0) == counts.get("k_syr2k_fma", 0) and set(census) <= {"k_cdec_mm", "k_cdec_fma"}
    chordal.tune(c.symb, chordal.TUNE_DETERMINISTIC, 1)
    try:
        counts, census = launch_census(c.symb, lambda: chordal.clique_decompose(c.L))
    finally:
        chordal.tune(c.symb, chordal.TUNE_DETERMINISTIC, 0)
    print("arrow_big deterministic", counts, census)
    assert counts == {"k_syr2k_fma": 1}
    assert census == {"k_cdec_fma": 1}


@pytest.mark.parametrize("name", ["band", "two_components", "arrow_thin", "arrow_big", "three_tops"])
def test_same_bits(name):
    c = case(name)
    Z = run(name, 0)[0]
    again = chordal.clique_decompose(c.L)
    assert torch.equal(again, Z)
    out = torch.full_like(Z, 7.25)
    back = chordal.clique_decompose(c.L, out=out)
    assert back is out and torch.equal(out, Z)


@pytest.mark.parametrize("name", ["nested", "arrow_thin"])
def test_caches_stay(name):
    """a Hessian, the decomposition, the same Hessian: nothing cached for L was dropped or spoiled"""
    c = case(name)
    symb = c.symb
    chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 1)
    try:
        L = cspmatrix(symb, c.L.blkval.clone())
        L.blkval[torch.from_numpy(~c.owned).cuda()] = 0.0           # (the Hessian reads whole panels)
        Y = L.copy()
        chordal.projected_inverse(Y)
        u = np.zeros(symb.blklen)
        u[symb.ccs_to_blk()] = np.random.default_rng(3).standard_normal(symb.nnz)
        fresh = lambda: cspmatrix(symb, torch.from_numpy(u.copy()).cuda())
        U1, U2 = fresh(), fresh()
        chordal.hessian(L, Y, U1)                                    # leaves the inverse-form factor of L behind
        Z = chordal.clique_decompose(L)
        chordal.hessian(L, Y, U2)
        assert torch.equal(U1.blkval, U2.blkval)
        assert bool(torch.isfinite(U1.blkval[torch.from_numpy(c.owned).cuda()]).all())
        for k, Zk in enumerate(R.unpack(symb, Z.cpu().numpy())):
            assert (np.abs(Zk - c.ref[k]) <= 2.0 * c.B[k]).all()
    finally:
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 0)


def test_errors():
    c = case("arrow_thin")
    symb = c.symb
    lib = _lib.lib()
    Z = torch.empty_like(run("arrow_thin", 0)[0])
    Lp, Zp, blklen = c.L.blkval.data_ptr(), Z.data_ptr(), symb.blklen
    assert lib.csp_clique_decompose(symb.handle, None, Zp, _stream()) == -1
    assert lib.csp_clique_decompose(symb.handle, Lp, None, _stream()) == -1
    assert lib.csp_clique_decompose(symb.handle, Lp, Lp, _stream()) == -1                         # Z overlapping L
    assert lib.csp_clique_decompose(symb.handle, Lp, Lp + 8 * (blklen - 1), _stream()) == -1      # by one entry
    assert lib.csp_clique_decompose(symb.handle, Lp, Zp, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(Z, run("arrow_thin", 0)[0])
    rep = symb.replicate(2)
    rep.device_init(0, 1)
    both = torch.cat([c.L.blkval, c.L.blkval])
    Z2 = torch.empty(2 * Z.shape[0], dtype=torch.float64, device="cuda")
    assert lib.csp_clique_decompose(rep.handle, both.data_ptr(), Z2.data_ptr(), _stream()) == -1
    n = Z.shape[0]
    for out in (torch.empty(n - 1, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda"),
                torch.empty(n, dtype=torch.float64), torch.empty(2 * n, dtype=torch.float64, device="cuda")[::2]):
        with pytest.raises(ValueError):
            chordal.clique_decompose(c.L, out=out)
    assert torch.equal(c.L.blkval.view(torch.int64), c.bits)


def spd_on(pat, seed):
    """a positive definite matrix (dense numpy) whose pattern is exactly that of `pat`, by diagonal dominance"""
    n, cp, ri = pat
    cols = np.repeat(np.arange(n), np.diff(cp))
    rows = np.asarray(ri)
    off = rows != cols
    A = np.zeros((n, n))
    A[rows[off], cols[off]] = np.random.default_rng(seed).standard_normal(int(off.sum()))
    A = A + A.T
    A[np.diag_indices(n)] = np.abs(A).sum(axis=1) + 1.0
    return A


@pytest.mark.parametrize("name", ["band", "rand2"])
def test_scipy_form(name):
    from smcp_amd.base import _on_chordal_pattern
    A = spd_on(PATTERNS[name](), seed=41)
    n = A.shape[0]
    perm = np.random.default_rng(42).permutation(n)
    A = A[np.ix_(perm, perm)]
    As = sp.csc_matrix(np.tril(A))
    cliques, blocks = smcp_amd.clique_decompose(As)
    M = np.zeros((n, n))
    for rows, Zk in zip(cliques, blocks):
        assert isinstance(Zk, np.ndarray) and Zk.shape == (len(rows), len(rows))
        M[np.ix_(rows, rows)] += Zk
    # the bound of test_sum, in the original numbering: the factor of the same matrix on the Symbolic the call builds
    Sc = _on_chordal_pattern([As], "test")[0]
    chordal.cholesky(Sc)
    p = np.asarray(Sc.symb.p)
    bound = np.zeros((n, n))
    bound[np.ix_(p, p)] = R.sum_bound(Sc.to_dense_factor())
    mask = A != 0.0
    print("%s: worst |sum - S| / bound %.3f" % (name, (np.abs(M - A)[mask] / bound[mask]).max()))
    assert (np.abs(M - A)[mask] <= bound[mask]).all()
    assert (M[~mask] == 0.0).all()
    assert sorted(np.concatenate(cliques).tolist()) == sorted(np.concatenate(
        [p[np.asarray(Sc.symb.rowidx)[Sc.symb.rowptr[k]:Sc.symb.rowptr[k + 1]]] for k in range(Sc.symb.Nsn)]).tolist())


def test_scipy_form_errors():
    A = spd_on(PATTERNS["band"](), seed=43)
    A[3, 3] = -1.0                                                   # indefinite
    with pytest.raises(ArithmeticError):
        smcp_amd.clique_decompose(sp.csc_matrix(np.tril(A)))
    C = 4.0 * np.eye(4)                                              # a 4-cycle is not chordal
    for i, j in ((1, 0), (2, 1), (3, 2), (3, 0)):
        C[i, j] = C[j, i] = 1.0
    with pytest.raises(ValueError):
        smcp_amd.clique_decompose(sp.csc_matrix(np.tril(C)))
