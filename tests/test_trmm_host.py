"""chordal.trmm without a GPU: the numpy restatement of the device's two-phase schedule (tests/trmm_ref.py) against the
dense definition, the public interface, and the refusal to run without a device."""
import inspect

import numpy as np
import pytest
import torch

import smcp_amd
from smcp_amd import _lib
from smcp_amd.symbolic import Symbolic
from tests.helpers import PATTERNS, symb_of
from tests.trmm_ref import dense_trmm, factor_input, product_bound, transposed_separator_index, trmm_two_phase

@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_transposed_separator_index(name):
    """Every separator entry appears once, under its own row, and the cliques of a row ascend."""
    symb = symb_of(name)
    tptr, tk, tq = transposed_separator_index(symb)
    nn = np.diff(symb.snptr)
    assert len(tptr) == symb.n + 1 and len(tk) == len(tq) == symb.sepptr[-1]
    seen = set()
    for i in range(symb.n):
        ks = tk[tptr[i]:tptr[i + 1]]
        assert (np.diff(ks) > 0).all()                       # ascending, and a row is in a separator at most once
        for k, q in zip(ks, tq[tptr[i]:tptr[i + 1]]):
            assert symb.rowidx[symb.rowptr[k] + nn[k] + q] == i
            seen.add((int(k), int(q)))
    assert len(seen) == symb.sepptr[-1]


@pytest.mark.parametrize("nrhs", [1, 5])
@pytest.mark.parametrize("alpha", [1.0, -0.5])
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_two_phase_schedule_is_the_dense_product(name, trans, alpha, nrhs):
    symb = symb_of(name)
    blk, Ld = factor_input(symb, seed=3)
    B = np.random.default_rng(4).standard_normal((symb.n, nrhs))
    got = trmm_two_phase(symb, blk, B, alpha, trans)
    ref = dense_trmm(Ld, B, alpha, trans)
    assert np.isfinite(got).all()                            # nothing above the diagonal of a diagonal block was read
    assert (np.abs(got - ref) <= product_bound(Ld, B, alpha, trans)).all()


def test_a_dropped_term_breaks_the_bound():
    """The bound is tight enough to see one missing product."""
    symb = symb_of("arrow")
    blk, Ld = factor_input(symb, seed=3)
    B = np.random.default_rng(4).standard_normal((symb.n, 2))
    L2 = Ld.copy()
    L2[symb.n - 1, 0] = 0.0
    assert Ld[symb.n - 1, 0] != 0.0
    assert not (np.abs(dense_trmm(L2, B, 1.0, False) - dense_trmm(Ld, B, 1.0, False)) <= product_bound(Ld, B, 1.0, False)).all()


def test_public_interface():
    assert smcp_amd.trmm is smcp_amd.chordal.trmm
    par = inspect.signature(smcp_amd.trmm).parameters
    assert list(par) == ["L", "B", "alpha", "trans"]
    assert par["alpha"].default == 1.0 and par["trans"].default == "N"


def test_no_device_no_product():
    if torch.cuda.is_available():                            # (as tests/test_abi.py::test_no_cpu_fallback)
        return
    symb = Symbolic(PATTERNS["band"]())                      # a fresh context: never initialised on a device
    blk, _ = factor_input(symb, seed=1, junk=0.0)
    B = np.ones((2, symb.n))
    rc = _lib.lib().csp_trmm(symb.handle, blk.ctypes.data, B.ctypes.data, 2, symb.n, 1.0, 0, None)
    assert rc == -2                                          # SMCP_ENODEV
    assert (B == 1.0).all()
