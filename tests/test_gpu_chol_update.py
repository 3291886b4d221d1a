"""chordal.chol_update on the device (csrc/front_update.hip, chol_update.hip) against the dense numpy definition
M = Ld Ld^T + V diag(a) V^T.  The measure is eta = |P_V(L' L'^T - M)|_F / |M|_F; the yardstick is the same eta for
numpy.linalg.cholesky(M), floored at n eps (tests/chol_update_ref.py: yardstick) -- never the code under test.  L comes from
trmm_ref.factor_input, the columns of V lie inside cliques (checked with chordal.clique_support) and are scaled so that
|L^-1 v_j| = 1; updates take a in [0.5, 1.5], downdates a_j = -0.5 / k.

The gate is 4 x the worst ratio recorded on the MI355X; a ratio beyond 256 would be a defect.
Worst eta / yardstick per pattern over k and the three sign choices (test_definition), then of the round trip
(update by (V, a), then by (V, -a), against L L^T; test_round_trip).  The yardstick is its floor n eps everywhere: numpy's
own eta is below it.
    diag            0.099  (k = 64, minus)     0.064
    dense           0.457  (k = 64, mixed)     1.061  (k = 17: 17 updates of weight up to 1.5 in dimension 9, then taken back)
    band            0.077  (k = 64, mixed)     0.103
    nested          0.029  (k = 64, mixed)     0.031
    two_components  0.050  (k = 64, minus)     0.038
    arrow_thin      0.013  (k = 17, mixed)     0.016
    arrow_one       0.005  (k = 17, mixed)     0.006
    dense200        0.008  (k = 17, plus)      0.011
The worst of all is 1.061, so the gate is 4.25.
"""
import ctypes

import numpy as np
import pytest
import torch

import smcp_amd
from smcp_amd import _lib, chordal
from smcp_amd.cspmatrix import _stream, cspmatrix
from smcp_amd.symbolic import Symbolic
from tests import chol_update_ref as R
from tests.helpers import EXTRA, GPU_PATTERNS, launch_census, padded
from tests.trmm_ref import factor_input

pytestmark = pytest.mark.gpu

GATE = 4.25                            # 4 x 1.061, the worst ratio recorded on the MI355X (docstring)
SMALL = ("diag", "dense", "band", "nested", "two_components")
LARGE = ("arrow_thin", "arrow_one", "dense200")
RANKS = {"small": (1, 7, 16, 17, 64), "large": (1, 17)}       # one pass (1, 7, 16), a second ragged pass (17), the limit (64)
SIGNS = ("plus", "minus", "mixed")
JUNK = 3.5                             # what the slots outside the pattern hold: never read, never written
CASES = {}
INPUTS = {}
WORST = {}


def case(name):
    """(Symbolic on the device, blkval of L on the device, dense Ld, pattern mask): built once per pattern, left unchanged"""
    if name not in CASES:
        symb = Symbolic((GPU_PATTERNS.get(name) or EXTRA[name])())
        symb.device_init(0, 1)
        blk, Ld = factor_input(symb, seed=5, junk=JUNK)
        CASES[name] = (symb, torch.from_numpy(blk).cuda(), Ld, R.pattern_mask(symb))
    return CASES[name]


def inputs(name, k, signs, seed=0):
    """(V, a, dense M, yardstick): numpy, computed once and left unchanged"""
    key = (name, k, signs, seed)
    if key not in INPUTS:
        symb, _, Ld, mask = case(name)
        V = R.unit_columns(Ld, R.support_columns(symb, k, 1000 + 7 * seed + k, leaves_first=True))
        for j in range(k):
            assert chordal.clique_support(symb, np.flatnonzero(V[:, j])) == R.support_clique(symb, V[:, j]) >= 0
        a = R.coefficients(k, 2000 + k, signs)
        M = R.dense_M(Ld, V, a)
        INPUTS[key] = (V, a, M, R.yardstick(mask, M))
    return INPUTS[key]


def update(name, V, a, pad=3, L=None):
    """chol_update on a clone of the pattern's L (or on L) with V inside a padded tensor: V and the padding are not written"""
    symb, blk, _, _ = case(name)
    L = cspmatrix(symb, blk.clone()) if L is None else L
    view, full = padded(V, pad)
    before = full.clone()
    chordal.chol_update(L, view, a)
    assert torch.equal(full, before)
    return L


def ratio(name, L, M, yard, what):
    _, _, _, mask = case(name)
    Ln = L.to_dense_factor()
    assert np.isfinite(Ln).all()
    r = R.eta(mask, Ln, M) / yard
    if r > WORST.get(name, (0.0, None))[0]:
        WORST[name] = (r, what)
    assert r <= GATE, (name, what, r)
    return r


@pytest.mark.parametrize("name", SMALL + LARGE)
def test_definition(name):
    symb, blk, Ld, _ = case(name)
    for k in RANKS["small" if name in SMALL else "large"]:
        for i, signs in enumerate(SIGNS):
            V, a, M, yard = inputs(name, k, signs)
            r = ratio(name, update(name, V, a, pad=3 * (i % 2)), M, yard, (k, signs))
            print("%s k=%d %s: eta / yardstick %.3f" % (name, k, signs, r))
    print("%s: worst eta / yardstick %.3f at (k, signs) = %s (gate %g)" % ((name,) + WORST[name] + (GATE,)))


@pytest.mark.parametrize("name", SMALL + LARGE)
def test_only_the_paths_are_written(name):
    symb, blk, Ld, _ = case(name)
    outside = np.ones(symb.blklen, dtype=bool)
    outside[symb.ccs_to_blk()] = False
    blkptr = symb.blkptr
    for k, signs in ((1, "plus"), (7, "mixed")) + (((64, "minus"),) if name in SMALL else ()):
        V, a, _, _ = inputs(name, k, signs, seed=1)
        a = a.copy()
        if k > 1:
            a[2] = 0.0                                               # a column that is left out marks no path
        new = update(name, V, a).blkval.cpu().numpy()
        old = blk.cpu().numpy()
        assert np.array_equal(new[outside], old[outside])            # the slots outside the pattern
        union = R.path_union(symb, V, a)
        starts = {R.support_clique(symb, V[:, j]) for j in range(k) if a[j] != 0}
        assert starts and starts <= union
        for s in range(symb.Nsn):
            same = np.array_equal(new[blkptr[s]:blkptr[s + 1]], old[blkptr[s]:blkptr[s + 1]])
            assert same or s in union, (name, k, s)                  # nothing outside the union of the paths is written
            assert not same or s not in starts, (name, k, s)         # and the cliques the columns start in have changed


@pytest.mark.parametrize("name", ["band", "nested", "arrow_thin"])
def test_a_column_of_zeros_changes_nothing(name):
    symb, blk, Ld, _ = case(name)
    assert torch.equal(update(name, np.zeros((symb.n, 1)), [1.0]).blkval, blk)
    assert torch.equal(update(name, np.zeros((symb.n, 3)), [1.0, -1.0, 0.5]).blkval, blk)
    V, a, _, _ = inputs(name, 7, "mixed")
    V0, a0 = np.insert(V, 3, 0.0, axis=1), np.insert(a, 3, 1.0)
    assert torch.equal(update(name, V0, a0).blkval, update(name, V, a).blkval)
    V1 = V.copy()
    V1[:, 4] = np.inf                                                # left out, unread: its coefficient is 0
    a1 = a.copy()
    a1[4] = 0.0
    keep = [0, 1, 2, 3, 5, 6]
    assert torch.equal(update(name, V1, a1).blkval, update(name, V[:, keep], a1[keep]).blkval)


@pytest.mark.parametrize("name", SMALL + LARGE)
def test_round_trip(name):
    symb, blk, Ld, mask = case(name)
    M0 = Ld @ Ld.T
    yard = R.yardstick(mask, M0)
    for k in (1, 17):
        V, a, _, _ = inputs(name, k, "plus")
        L = update(name, V, a)
        update(name, V, -a, L=L)
        r = ratio(name, L, M0, yard, (k, "round trip"))
        print("%s k=%d: round trip eta / yardstick %.3f" % (name, k, r))


@pytest.mark.parametrize("name", ["band", "nested", "two_components", "arrow_thin", "arrow_one"])
def test_same_bits(name):
    """from call to call, and k = 17 in one call against 17 calls of one column in the order the call takes them"""
    symb, blk, Ld, _ = case(name)
    V, a, _, _ = inputs(name, 17, "mixed")
    one, two = update(name, V, a), update(name, V, a, pad=0)
    assert torch.equal(one.blkval, two.blkval)
    L = cspmatrix(symb, blk.clone())
    for j in R.column_order(a):
        update(name, V[:, [j]], a[[j]], L=L)
    assert torch.equal(one.blkval, L.blkval)
    assert smcp_amd.clique_support is chordal.clique_support
    orig = cspmatrix(symb, blk.clone())                              # the form for V in the original order
    Vo = np.empty_like(V)
    Vo[np.asarray(symb.p)] = V
    smcp_amd.chol_update(orig, Vo, a)
    assert torch.equal(one.blkval, orig.blkval)


def test_bad_columns_leave_the_factor_alone():
    for name in ("nested", "arrow_thin"):
        symb, blk, Ld, _ = case(name)
        V, a, _, _ = inputs(name, 7, "mixed")
        s = R.support_clique(symb, V[:, 3])
        first = int(np.flatnonzero(V[:, 3])[0])
        out = [r for r in range(first + 1, symb.n) if r not in set(R.clique_rows(symb, s).tolist())]
        assert out
        bad = V.copy()
        bad[out[-1], 3] = 1e-300                                     # one nonzero outside the clique, however small
        assert chordal.clique_support(symb, np.flatnonzero(bad[:, 3])) == -1
        L = cspmatrix(symb, blk.clone())
        with pytest.raises(ValueError, match=r"column 3\b"):
            update(name, bad, a, L=L)
        assert torch.equal(L.blkval, blk)
        for poison in (np.nan, np.inf):
            bad = V.copy()
            bad[symb.n - 1, 5] = poison
            bad[out[-1], 6] = 1.0                                    # the first refused column is the one that is named
            with pytest.raises(ValueError, match=r"column 5\b"):
                update(name, bad, a, L=L)
            assert torch.equal(L.blkval, blk)
        an = a.copy()
        an[2] = np.nan
        with pytest.raises(ValueError, match=r"column 2\b"):
            update(name, V, an, L=L)
        assert torch.equal(L.blkval, blk)
        update(name, V, a, L=L)                                      # and the context is as good as before
        assert torch.equal(L.blkval, update(name, V, a).blkval)


def test_a_downdate_that_leaves_the_cone():
    for name in ("band", "nested"):
        symb, blk, Ld, _ = case(name)
        V, a, _, _ = inputs(name, 7, "plus")
        good = update(name, V, a).blkval
        bad = np.zeros(7)
        bad[4] = -2.0                                                # 1 + a_j |L^-1 v_j|^2 = -1
        assert np.linalg.eigvalsh(R.dense_M(Ld, V, bad)).min() < 0
        with pytest.raises(ArithmeticError, match=r"column 4\b"):
            update(name, V, bad)
        assert torch.equal(update(name, V, a).blkval, good)          # the next call starts clean


def test_bad_shapes_are_refused():
    symb, blk, Ld, _ = case("arrow_thin")
    n = symb.n
    L = cspmatrix(symb, blk.clone())
    z = lambda *shape, **kw: torch.zeros(shape, dtype=kw.get("dtype", torch.float64), device=kw.get("device", "cuda"))
    for V in (z(0, n), z(65, n), z(2, n - 1), z(n, 2).T, z(2, n, dtype=torch.float32), z(2, n, device="cpu"), z(n)):
        with pytest.raises(ValueError):
            chordal.chol_update(L, V)
    with pytest.raises(ValueError):
        chordal.chol_update(L, z(2, n), [1.0])
    assert torch.equal(L.blkval, blk)
    lib = _lib.lib()
    rep = symb.replicate(2)
    rep.device_init(0, 1)
    both = torch.cat([blk, blk])
    assert lib.csp_chol_update(rep.handle, both.data_ptr(), z(1, 2 * n).data_ptr(), 2 * n, 1, None, _stream()) == -1
    assert lib.csp_chol_update(symb.handle, L.blkval.data_ptr(), z(1, n).data_ptr(), n - 1, 1, None, _stream()) == -1
    col = ctypes.c_int64(7)
    assert lib.csp_chol_update_info(symb.handle, ctypes.byref(col)) == 0 and col.value == -1


@pytest.mark.parametrize("name", ["nested", "arrow_thin"])
def test_cached_inverse_form_factor_is_dropped(name):
    symb, _, _, _ = case(name)
    blk0, _ = factor_input(symb, seed=5, junk=0.0)                   # (the Hessian reads whole panels)
    chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 1)
    try:
        L = cspmatrix(symb, torch.from_numpy(blk0).cuda())
        Y = L.copy()
        chordal.projected_inverse(Y)
        u = np.zeros(symb.blklen)
        u[symb.ccs_to_blk()] = np.random.default_rng(3).standard_normal(symb.nnz)
        fresh = lambda: cspmatrix(symb, torch.from_numpy(u.copy()).cuda())
        U1 = fresh()
        chordal.hessian(L, Y, U1)                                    # leaves the inverse-form factor of L behind
        V, a, _, _ = inputs(name, 7, "mixed")
        update(name, V, a, L=L)
        U2, U3 = fresh(), fresh()
        chordal.hessian(L, Y, U2)                                    # the same address, new contents
        L2 = cspmatrix(symb, L.blkval.clone())
        chordal.hessian(L2, Y, U3)
        assert torch.equal(U2.blkval, U3.blkval)
        assert not torch.equal(U2.blkval, U1.blkval)
        # the same through the C-ABI alone, where nothing but csp_chol_update itself can have dropped the cache
        lib = _lib.lib()
        hess = lambda Lx, U: lib.csp_hessian(symb.handle, Lx.blkval.data_ptr(), Y.blkval.data_ptr(), U.blkval.data_ptr(), 1, symb.blklen, 0, 0, _stream())
        U4, U5, U6 = fresh(), fresh(), fresh()
        assert hess(L, U4) == 0
        Vd = torch.from_numpy(np.ascontiguousarray(V.T)).cuda()
        ah = (ctypes.c_double * 7)(*[-x for x in a])
        assert lib.csp_chol_update(symb.handle, L.blkval.data_ptr(), Vd.data_ptr(), symb.n, 7, ah, _stream()) == 0
        assert hess(L, U5) == 0
        L3 = cspmatrix(symb, L.blkval.clone())
        assert hess(L3, U6) == 0
        assert torch.equal(U5.blkval, U6.blkval) and not torch.equal(U5.blkval, U4.blkval)
    finally:
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 0)


def test_launches():
    """two launches, k_cu_plan under k_lr_apply and k_cu_walk under k_lr_small, whatever the tree and whatever k
    (DESIGN.md section 25): the deep band counts what the single clique counts"""
    counts = {}
    for name in ("band", "dense"):
        symb, blk, Ld, _ = case(name)
        for k in (1, 17, 64):
            V, a, _, _ = inputs(name, k, "mixed")
            Vd = torch.from_numpy(np.ascontiguousarray(V.T)).cuda()
            chordal.chol_update(cspmatrix(symb, blk.clone()), Vd, a)             # (the workspace is grown outside the count)
            L = cspmatrix(symb, blk.clone())
            counts[name, k], census = launch_census(symb, lambda: chordal.chol_update(L, Vd, a))
            print(name, k, counts[name, k], census)
            assert counts[name, k] == {"k_lr_apply": 1, "k_lr_small": 1}
            assert census == {"k_cu_plan": 1, "k_cu_walk": 1}                    # the kernels behind the two ids
    assert len({tuple(sorted(c.items())) for c in counts.values()}) == 1
