"""chordal.symm without a GPU: the numpy restatement of the device's two-phase schedule (tests/symm_ref.py) against the
dense definition, the properties of the contribution index, its length against csp_symm_positions (host only), the public
interface, and the refusal to run without a device."""
import inspect

import numpy as np
import pytest
import torch

import smcp_amd
from smcp_amd import _lib
from smcp_amd.symbolic import Symbolic
from tests.helpers import GPU_PATTERNS, PATTERNS, symb_of
from tests.symm_ref import contribution_index, dense_symm, items_of, matrix_input, symm_bound, symm_two_phase

SETTINGS = [(64, 256), (4, 8)]     # the device's; and one at which patterns of at most 30 rows have several chunks, parts and skipped items


@pytest.mark.parametrize("rows,kp", SETTINGS)
@pytest.mark.parametrize("nrhs", [1, 5])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-0.5, 1.0), (2.0, -0.25)])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_two_phase_schedule_is_the_dense_product(name, alpha, beta, nrhs, rows, kp):
    symb = symb_of(name)
    blk, Xd = matrix_input(symb, seed=3)
    rng = np.random.default_rng(4)
    B = rng.standard_normal((symb.n, nrhs))
    C = rng.standard_normal((symb.n, nrhs)) if beta != 0 else np.full((symb.n, nrhs), np.nan)
    got = symm_two_phase(symb, blk, B, C, alpha, beta, rows, kp)
    ref = dense_symm(Xd, B, C, alpha, beta)
    assert np.isfinite(got).all()                            # nothing above a diagonal was read, nor C for beta == 0
    assert (np.abs(got - ref) <= symm_bound(Xd, B, C, alpha, beta)).all()


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_zero_factors_are_left_out(name):
    symb = symb_of(name)
    blk = np.full(symb.blklen, np.nan)
    B = np.full((symb.n, 2), np.nan)
    C = np.random.default_rng(5).standard_normal((symb.n, 2))
    assert np.array_equal(symm_two_phase(symb, blk, B, C, 0.0, 1.0, 4, 8), C)
    assert (symm_two_phase(symb, blk, B, np.full_like(C, np.nan), 0.0, 0.0, 4, 8) == 0.0).all()


def test_the_small_setting_reaches_every_branch():
    """(4, 8) on `dense` (one 9 x 9 clique): three chunks, two parts, and the item (chunk 0, part 1) skipped."""
    its = items_of(symb_of("dense"), 4, 8)
    assert [(r, p) for _, r, p, _, _ in its] == [(0, 0), (1, 0), (2, 0), (2, 1)]
    assert [(nr, nc) for _, _, _, nr, nc in its] == [(4, 3), (4, 7), (1, 8), (1, 0)]
    assert len(items_of(symb_of("dense"), 64, 256)) == 1


@pytest.mark.parametrize("rows,kp", SETTINGS)
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_contribution_index(name, rows, kp):
    """Every partial appears once, under its target row; the runs ascend in (k, side, r, p); every row owns at least its own
    row partial."""
    symb = symb_of(name)
    tptr, rec = contribution_index(symb, rows, kp)
    its = items_of(symb, rows, kp)
    assert len(tptr) == symb.n + 1 and tptr[0] == 0 and tptr[-1] == len(rec)
    assert len(rec) == sum(nr + nc for _, _, _, nr, nc in its)
    listed = {(k, r, p): (nr, nc) for k, r, p, nr, nc in its}
    seen = set()
    for i in range(symb.n):
        run = rec[tptr[i]:tptr[i + 1]]
        keys = [tuple(int(x) for x in q[:4]) for q in run]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        own = False
        for k, side, r, p, j in (tuple(int(x) for x in q) for q in run):
            nr, nc = listed[(k, r, p)]
            nn = int(symb.snptr[k + 1] - symb.snptr[k])
            if side == 0:
                assert j < nr and symb.rowidx[symb.rowptr[k] + rows * r + j] == i
                own = own or (rows * r + j < nn)             # row i of its own supernode
            else:
                assert j < nc and symb.snptr[k] + kp * p + j == i
            seen.add((k, side, r, p, j))
        assert own
    assert len(seen) == len(rec)


@pytest.mark.parametrize("name", sorted(PATTERNS) + ["arrow_big", "dense600", "three_tops"])
def test_positions_of_the_library(name):
    """csp_symm_positions needs no device and equals the length of the restatement's list."""
    symb = symb_of(name)
    tptr, rec = contribution_index(symb)
    assert int(_lib.lib().csp_symm_positions(symb.handle)) == len(rec) == tptr[-1]
    assert len(rec) >= symb.n


def test_a_dropped_term_breaks_the_bound():
    """The bound is tight enough to see one missing product, on either side of the diagonal."""
    symb = symb_of("arrow")
    blk, Xd = matrix_input(symb, seed=3)
    B = np.random.default_rng(4).standard_normal((symb.n, 2))
    ref = dense_symm(Xd, B, None, 1.0, 0.0)
    bound = symm_bound(Xd, B, None, 1.0, 0.0)
    assert Xd[symb.n - 1, 0] != 0.0
    for i, j in ((symb.n - 1, 0), (0, symb.n - 1)):
        X2 = Xd.copy()
        X2[i, j] = 0.0
        assert not (np.abs(dense_symm(X2, B, None, 1.0, 0.0) - ref) <= bound).all()


def test_public_interface():
    assert smcp_amd.symm is smcp_amd.chordal.symm
    par = inspect.signature(smcp_amd.symm).parameters
    assert list(par) == ["X", "B", "C", "alpha", "beta"]
    assert par["C"].default is None and par["alpha"].default == 1.0 and par["beta"].default == 0.0


def test_no_device_no_product():
    if torch.cuda.is_available():                            # (as tests/test_abi.py::test_no_cpu_fallback)
        return
    symb = Symbolic(PATTERNS["band"]())                      # a fresh context: never initialised on a device
    blk, _ = matrix_input(symb, seed=1, junk=0.0)
    B = np.ones((2, symb.n))
    C = np.full((2, symb.n), 3.0)
    rc = _lib.lib().csp_symm(symb.handle, blk.ctypes.data, B.ctypes.data, symb.n, C.ctypes.data, symb.n, 2, 1.0, 0.0, None)
    assert rc == -2                                          # SMCP_ENODEV
    assert (C == 3.0).all() and (B == 1.0).all()
