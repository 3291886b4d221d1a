"""chordal.syr2k / syrk / syr2 without a GPU: the numpy restatement of the device's per-clique schedule
(tests/syr2k_ref.py) against the dense definition, the public interface, the layout checks of the wrappers, and the
refusal to run without a device."""
import inspect

import numpy as np
import pytest
import torch

import smcp_amd
from smcp_amd import _lib
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic
from tests.helpers import PATTERNS, symb_of
from tests.syr2k_ref import (dense_syr2k, lower_index, matrix_input, owned, pattern_mask, syr2k_bound, syr2k_per_clique,
                             to_dense)

@pytest.mark.parametrize("k", [1, 3, 9])
@pytest.mark.parametrize("ab", [(1.0, 0.0), (-0.5, 1.0), (2.0, -0.25)])
@pytest.mark.parametrize("form", ["syr2k", "syrk"])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_per_clique_schedule_is_the_dense_definition(name, form, ab, k):
    symb = symb_of(name)
    alpha, beta = ab
    blk, Xd = matrix_input(symb, seed=3)                     # NaN outside the pattern: reading one shows
    rng = np.random.default_rng(4)
    U = rng.standard_normal((symb.n, k))
    V = rng.standard_normal((symb.n, k)) if form == "syr2k" else None
    if beta == 0:
        blk = np.full(symb.blklen, np.nan)                   # not read at all
    got = syr2k_per_clique(symb, blk, U, V, alpha, beta)
    assert np.isfinite(got).all()
    msk = owned(symb)
    assert (got[~msk] == 0.0).all()                          # unowned slots: exactly zero
    ref = dense_syr2k(Xd, pattern_mask(symb), U, V, alpha, beta)
    bound = syr2k_bound(Xd, U, V, alpha, beta)
    I, J = lower_index(symb)
    assert (np.abs(got[symb.ccs_to_blk()] - ref[I, J]) <= bound[I, J]).all()
    assert np.array_equal(to_dense(symb, got), to_dense(symb, got).T)


def test_zero_factors_leave_their_term_out():
    symb = symb_of("arrow")
    blk, _ = matrix_input(symb, seed=3)
    msk = owned(symb)
    U = np.full((symb.n, 2), np.inf)
    same = syr2k_per_clique(symb, blk, U, U, 0.0, 1.0)       # alpha = 0: U, V not read, owned slots bit for bit
    assert np.array_equal(same[msk], blk[msk]) and (same[~msk] == 0.0).all()
    assert (syr2k_per_clique(symb, blk, U, None, 0.0, 0.0) == 0.0).all()


def test_a_dropped_term_breaks_the_bound():
    """The bound is tight enough to see one missing product."""
    symb = symb_of("arrow")
    _, Xd = matrix_input(symb, seed=3)
    rng = np.random.default_rng(4)
    U, V = rng.standard_normal((symb.n, 3)), rng.standard_normal((symb.n, 3))
    mask = pattern_mask(symb)
    ref = dense_syr2k(Xd, mask, U, V, 1.0, 1.0)
    short = dense_syr2k(Xd, mask, U[:, :2], V[:, :2], 1.0, 1.0) + np.where(mask, np.outer(U[:, 2], V[:, 2]), 0.0)   # V U^T of the last rank missing
    assert not (np.abs(short - ref) <= syr2k_bound(Xd, U, V, 1.0, 1.0)).all()


def test_public_interface():
    for name, args in (("syr2k", ["X", "U", "V", "alpha", "beta"]), ("syrk", ["X", "U", "alpha", "beta"]),
                       ("syr2", ["X", "y", "z", "alpha", "beta"])):
        f = getattr(smcp_amd, name)
        assert f is getattr(smcp_amd.chordal, name)
        par = inspect.signature(f).parameters
        assert list(par) == args
        assert par["alpha"].default == 1.0 and par["beta"].default == 1.0


def test_wrong_layout_is_refused():
    """shape and strides are checked before anything touches a device"""
    symb = symb_of("arrow")
    n = symb.n
    X = cspmatrix(symb, torch.zeros(symb.blklen, dtype=torch.float64))
    good = torch.zeros((2, n), dtype=torch.float64)
    bad = [torch.zeros((2, n + 1), dtype=torch.float64),                 # wrong length
           torch.zeros((n, 2), dtype=torch.float64).T,                   # stride(1) != 1
           torch.zeros((2, 2 * n), dtype=torch.float64)[:, ::2],         # stride(1) == 2
           torch.zeros(n, dtype=torch.float64).expand(2, n),             # stride(0) == 0 < n
           torch.zeros(n, dtype=torch.float64)]                          # not a block
    for B in bad:
        with pytest.raises(AssertionError):
            smcp_amd.syrk(X, B)
        with pytest.raises(AssertionError):
            smcp_amd.syr2k(X, B, good)
        with pytest.raises(AssertionError):
            smcp_amd.syr2k(X, good, B)
    with pytest.raises(AssertionError):
        smcp_amd.syr2k(X, good, torch.zeros((3, n), dtype=torch.float64))       # ranks differ
    with pytest.raises(AssertionError):
        smcp_amd.syr2(X, good, good)                                             # y, z are vectors
    with pytest.raises(AssertionError):
        smcp_amd.syr2(X, torch.zeros(n + 1, dtype=torch.float64), torch.zeros(n, dtype=torch.float64))


def test_no_device_no_update():
    if torch.cuda.is_available():                            # (as tests/test_abi.py::test_no_cpu_fallback)
        return
    symb = Symbolic(PATTERNS["band"]())                      # a fresh context: never initialised on a device
    blk, _ = matrix_input(symb, seed=1, junk=0.0)
    before = blk.copy()
    U = np.ones((2, symb.n))
    lib = _lib.lib()
    assert lib.csp_syr2k(symb.handle, blk.ctypes.data, U.ctypes.data, U.ctypes.data, 2, symb.n, symb.n, 1.0, 1.0, None) == -2   # SMCP_ENODEV
    assert lib.csp_syr2k(symb.handle, blk.ctypes.data, U.ctypes.data, None, 2, symb.n, 0, 1.0, 1.0, None) == -2
    assert np.array_equal(blk, before) and (U == 1.0).all()
