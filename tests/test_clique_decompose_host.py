"""The definition of chordal.clique_decompose without a GPU: the numpy restatement of tests/clique_decompose_ref.py against
long double, the sum against the dense L L^T, cone membership and rank of every block, on factors whose unowned slots hold
NaN; and that the call is offered by the package, documented and declared."""
import os

import numpy as np
import pytest

from smcp_amd.symbolic import Symbolic
from tests import clique_decompose_ref as R
from tests.helpers import EXTRA, GPU_PATTERNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("band", "arrow", "nested", "rand1", "rand2", "dense", "diag", "two_components", "arrow_thin")


@pytest.mark.parametrize("name", NAMES)
def test_definition_sum_and_cone(name):
    symb = Symbolic((GPU_PATTERNS.get(name) or EXTRA[name])())
    blk, Ld = R.random_factor(symb, seed=11)
    un = R.unowned(symb)
    assert np.isnan(blk[un]).all() and np.isfinite(blk[~un]).all()        # NaN in every unowned slot, and only there
    before = blk.copy()
    Z = R.decompose(symb, blk)
    X = R.exact(symb, blk)
    B = R.bounds(symb, blk)
    snptr = np.asarray(symb.snptr)
    worst = 0.0
    for k in range(symb.Nsn):
        nn = int(snptr[k + 1] - snptr[k])
        assert np.isfinite(Z[k]).all()
        err = np.abs(Z[k] - X[k]).astype(np.float64)
        assert (err <= B[k]).all(), (name, k)
        worst = max(worst, float((err[B[k] > 0] / B[k][B[k] > 0]).max()))
        assert np.array_equal(Z[k], Z[k].T)
        lam, tail = R.cone_defects(Z[k], B[k], nn)
        assert lam <= 1.0 and tail <= 1.0, (name, k, lam, tail)
    M = R.sum_blocks(symb, Z)
    LLt = Ld @ Ld.T
    mask = R.pattern_mask(symb)
    assert (np.abs(M - LLt)[mask] <= R.sum_bound(Ld)[mask]).all()
    assert (M[~mask] == 0.0).all()
    assert np.array_equal(blk, before, equal_nan=True)                     # the input is unchanged
    # the packed layout round trip
    q = R.qptr(symb)
    packed = R.pack(Z)
    assert len(packed) == q[-1] and all(np.array_equal(a, b) for a, b in zip(R.unpack(symb, packed), Z))
    print("%s: worst |Z - exact| / B %.3f" % (name, worst))


def test_the_call_is_offered_documented_and_declared():
    import smcp_amd
    from smcp_amd import chordal
    assert callable(chordal.clique_decompose) and callable(smcp_amd.clique_decompose)
    assert smcp_amd.clique_decompose is not chordal.clique_decompose       # the scipy form and the cspmatrix form
    doc = chordal.clique_decompose.__doc__
    assert "clique_scatter" in doc and "llt" in doc
    src = open(os.path.join(ROOT, "include", "smcp_amd.h")).read()
    assert "int csp_clique_decompose(csp_ctx* ctx, const double* L, double* Z, void* stream);" in src
