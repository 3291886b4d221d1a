"""chordal.trmm on the device (csrc/front_trmm.hip) against the dense definition alpha op(Ld) B in numpy, with the
componentwise inner-product rounding bound of tests/trmm_ref.py; its contract (same bits from call to call, L and the
padding of B untouched, exact zeros for alpha = 0) is asserted on every call of the helper.  The strict upper triangles
of the diagonal blocks of L hold NaN: they are not part of the factor."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from smcp_amd import _lib, chordal, problems
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic
from tests.helpers import EXTRA, GPU_PATTERNS, launch_counts, random_block
from tests.trmm_ref import U, dense_trmm, factor_input, product_bound, transposed_separator_index

pytestmark = pytest.mark.gpu

NRHS = (1, 7, 8, 17, 70)       # below, at and above the tile gate; one past a 16-column block; two 64-column tiles, the second ragged
CASES = {}


def case(name):
    """(Symbolic on the device, L with NaN off the pattern, L with zeros there, dense Ld): built once per pattern"""
    if name not in CASES:
        symb = Symbolic((GPU_PATTERNS.get(name) or EXTRA[name])())
        symb.device_init(0, 1)
        blk, Ld = factor_input(symb, seed=5)
        L = cspmatrix(symb, torch.from_numpy(blk).cuda())
        Lz = cspmatrix(symb, torch.from_numpy(np.nan_to_num(blk, nan=0.0)).cuda())
        CASES[name] = (symb, L, Lz, Ld)
    return CASES[name]


def device_trmm(name, B, pad, alpha, trans):
    """One product on the device, with the contract checked: returns the n x nrhs result."""
    symb, L, _, _ = case(name)
    n, nrhs = B.shape
    outs = []
    before = L.blkval.clone()
    for _ in range(2):                                               # the same call twice, each on a fresh copy of B
        full = torch.full((nrhs, n + pad), 7.25, dtype=torch.float64, device="cuda")
        view = full[:, :n]
        view.copy_(torch.from_numpy(np.ascontiguousarray(B.T)))
        chordal.trmm(L, view, alpha, "T" if trans else "N")
        assert (full[:, n:] == 7.25).all()                           # padding untouched
        outs.append(view.clone())
    assert torch.equal(outs[0], outs[1])                             # deterministic
    assert torch.equal(torch.nan_to_num(before, nan=3.0), torch.nan_to_num(L.blkval, nan=3.0))       # L bit for bit
    full = torch.full((nrhs, n + pad), 7.25, dtype=torch.float64, device="cuda")
    view = full[:, :n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(B.T)))
    chordal.trmm(L, view, 0.0, "T" if trans else "N")
    assert bool((view == 0).all()) and bool((full[:, n:] == 7.25).all())
    return outs[0].cpu().numpy().T


def check_definition(name, nrhs_list=NRHS):
    symb, _, _, Ld = case(name)
    worst = 0.0
    combo = 0
    for trans in (False, True):
        for nrhs in nrhs_list:
            for alpha in (1.0, -0.5):
                pad = 3 * (combo % 2)                                # ldb = n for one half of the cases, n + 3 for the other
                combo += 1
                B = np.random.default_rng(100 + combo).standard_normal((symb.n, nrhs))
                got = device_trmm(name, B, pad, alpha, trans)
                ref = dense_trmm(Ld, B, alpha, trans)
                bound = product_bound(Ld, B, alpha, trans)
                ratio = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
                worst = max(worst, ratio)
                assert np.isfinite(got).all()
                assert (np.abs(got - ref) <= bound).all(), (name, trans, nrhs, alpha, ratio)
    print("%s: largest |got - ref| / bound %.3f" % (name, worst))


@pytest.mark.parametrize("name", sorted(GPU_PATTERNS))
def test_definition(name):
    check_definition(name)


@pytest.mark.parametrize("name", ["arrow_big", "nested_mid", "dense600", "three_tops"])
def test_generic_route(name):
    symb = case(name)[0]
    chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 1)
    try:
        check_definition(name)
    finally:
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 0)


def test_launch_count_does_not_depend_on_the_tree():
    """band has 27 levels, rand2 7, nested_mid 4: a call is at most four launches on each, and trees that take the same
    route (the same set of kernels: with or without tile products for large fronts) take the same number."""
    levels = {}
    by_route = {}
    for name in ("band", "rand2", "nested_mid"):
        symb, L, _, _ = case(name)
        levels[name] = symb.nlev
        for nrhs in (1, 70):
            for trans in ("N", "T"):
                _, view, _ = random_block(symb.n, nrhs, 0, 9)
                chordal.trmm(L, view, 1.0, trans)                    # (workspaces grown outside the count)
                cnt = launch_counts(symb, lambda: chordal.trmm(L, view, 1.0, trans))
                total = sum(cnt.values())
                print(name, nrhs, trans, cnt)
                assert 1 <= total <= 4, (name, nrhs, trans, cnt)
                assert all(k.startswith("k_trmm_") for k in cnt), cnt
                by_route.setdefault((nrhs, trans, tuple(sorted(cnt))), set()).add(total)
                if nrhs == 1:                                        # one route for a single column: equal across all three trees
                    by_route.setdefault((nrhs, trans), set()).add(total)
    assert levels["band"] > levels["rand2"] > levels["nested_mid"] >= 3
    for key, totals in by_route.items():
        assert len(totals) == 1, (key, totals)


@pytest.mark.parametrize("name", sorted(GPU_PATTERNS))
def test_round_trip_with_trsm(name):
    symb, L, Lz, Ld = case(name)
    for trans in (False, True):
        for nrhs in (4, 70):
            B, view, _ = random_block(symb.n, nrhs, 0, 21 + nrhs)
            t = "T" if trans else "N"
            chordal.trmm(L, view, 1.0, t)
            chordal.trsm(Lz, view, t)
            got = view.cpu().numpy().T
            op = Ld.T if trans else Ld
            back = sla.solve_triangular(op, op @ B, lower=not trans)
            e_ref = np.abs(back - B).max() / np.abs(B).max()
            err = np.abs(got - B).max() / np.abs(B).max()
            print("%s trans %s nrhs %d: round trip %.2e (scipy %.2e)" % (name, t, nrhs, err, e_ref))
            assert err <= max(1e-10, 100 * e_ref)


@pytest.mark.parametrize("name", ["arrow", "nested_mid", "dense200"])
def test_composition_is_the_product_with_S(name):
    symb, L, _, Ld = case(name)
    for nrhs in (3, 20):
        B, view, _ = random_block(symb.n, nrhs, 0, 31)
        chordal.trmm(L, view, 1.0, "T")
        chordal.trmm(L, view, 1.0, "N")
        got = view.cpu().numpy().T
        ref = Ld @ (Ld.T @ B)
        bound = 4 * (symb.n + 2) * U * (np.abs(Ld) @ np.abs(Ld.T) @ np.abs(B))
        assert (np.abs(got - ref) <= bound).all()


def test_diagonal_pattern_is_one_rounding():
    """every clique 1 x 1 without a separator: alpha diag(L) B, one product and the rounding of alpha"""
    symb, _, _, Ld = case("diag")
    assert symb.Nsn == symb.n and symb.sepptr[-1] == 0
    d = np.diag(Ld)[:, None]
    for trans in (False, True):
        for alpha in (1.0, -0.5):
            B = np.random.default_rng(41).standard_normal((symb.n, 5))
            got = device_trmm("diag", B, 3, alpha, trans)
            assert np.array_equal(got, alpha * (d * B))              # alpha a power of two: exactly the rounded product


@pytest.mark.parametrize("name", ["two_components", "one_clique"])
def test_forest_and_single_clique(name):
    symb = case(name)[0]
    if name == "two_components":
        assert int((np.asarray(symb.snpar) < 0).sum()) >= 2
    else:
        assert symb.Nsn == 1
    check_definition(name, nrhs_list=(1, 8, 17))


def test_rows_with_many_contributors():
    """150 blocks under one arrow: every arrow row sums 149 contributions, the wave-per-entry path of the combining pass
    (more than 32 contributors), with more than two rounds of its 64 lanes; 40 columns: the tile products on every front"""
    symb = case("wide_arrow")[0]
    assert int(np.diff(transposed_separator_index(symb)[0]).max()) > 128
    check_definition("wide_arrow", nrhs_list=(1, 8, 40))


def test_wrong_layout_is_refused():
    symb, L, _, _ = case("arrow")
    with pytest.raises(AssertionError):
        chordal.trmm(L, torch.zeros((2, symb.n + 1), dtype=torch.float64, device="cuda"))
    with pytest.raises(AssertionError):
        chordal.trmm(L, torch.zeros((symb.n, 2), dtype=torch.float64, device="cuda").T)
    B = torch.zeros((2, symb.n), dtype=torch.float64, device="cuda")
    lib = _lib.lib()
    assert lib.csp_trmm(symb.handle, L.blkval.data_ptr(), B.data_ptr(), 0, symb.n, 1.0, 0, None) == -1
    assert lib.csp_trmm(symb.handle, L.blkval.data_ptr(), B.data_ptr(), 2, symb.n - 1, 1.0, 0, None) == -1
