"""Pins the CPU oracle to the dense definitions (tests/dense_ref.py) at the shapes the GPU suite uses.

tests/test_oracle_identities.py ties the oracle to dense linear algebra on the six small PATTERNS only; here every operation runs
on every entry of GPU_PATTERNS (n <= 1000), on the product's symbolic arrays and on oracle.symbolic_ref, with the suite's input
recipe (random_factor_blkval, random_constraints(m = 7, density = 0.05), kk in {1.0, 0.25}).  The worst oracle-vs-dense error per
operation is recorded in tests/golden/dense_ref_yardstick.json (tests/golden/make_dense_ref_yardstick.py); the oracle must stay
within 10 x of it, and the device checks take their bounds from the same file (tests/test_gpu_dense_ref.py).
"""
import numpy as np
import pytest

from oracle import oracle as orc
from smcp_amd.symbolic import Symbolic
from tests import dense_ref
from tests.helpers import GPU_PATTERNS

# fp64 on inputs of condition number 5 - 9, n <= 1000: an oracle-vs-dense error beyond this is not rounding, whatever the file says
YARDSTICK_SANITY = 1e-14


@pytest.fixture(scope="module")
def yard():
    return dense_ref.load_yardstick()


def test_yardstick_file_is_sane(yard):
    ops = {"cholesky", "llt", "projected_inverse", "completion", "logdiagsum", "dot", "hessian", "hessian_inv", "hessian_gadj_g",
           "hessian_gram", "hessian_adjoint", "hessian_factor_inv", "trsm", "kkt_H", "kkt_x", "kkt_y"}
    assert set(yard) == ops
    for op, rec in yard.items():
        assert 0.0 < rec["value"] < YARDSTICK_SANITY, (op, rec)
        assert rec["pattern"] in GPU_PATTERNS and rec["symbolic"] in ("product", "ref")
        assert dense_ref.device_bound(op, yard) <= dense_ref.BOUND_CAP


@pytest.mark.parametrize("which", ["product", "ref"])
@pytest.mark.parametrize("name", sorted(GPU_PATTERNS))
def test_oracle_against_dense_definitions(name, which, yard):
    errs = dense_ref.oracle_yardstick(name, which)
    assert set(errs) == set(yard)
    print(name, which, " ".join("%s=%.1e" % kv for kv in sorted(errs.items())))
    for op, e in errs.items():
        assert e <= 10.0 * yard[op]["value"], (op, e, yard[op])


def test_blockwise_notices_a_single_clique_error_that_the_global_measure_does_not(yard):
    """An error of 1e-11 confined to the smallest clique of nested_mid (996 columns): the per-clique measure exceeds the device
    bound of projected_inverse, the measure of the parity suite (relative 2-norm of the whole vector < 1e-10) does not see it."""
    pat = GPU_PATTERNS["nested_mid"]()
    S = orc.Sym(Symbolic(pat))
    case = dense_ref.DenseCase(pat, S, dense_ref.YARDSTICK_SEED)
    y = case.cholesky()
    orc.projected_inverse(S, y)
    bound = dense_ref.device_bound("projected_inverse", yard)
    glob, worst = dense_ref.blockwise(S, y, case.Yblk)
    assert worst < bound and glob <= worst
    k = int(np.argmin(np.diff(S.blkptr)))
    bad = y.copy()
    bad[S.blkptr[k]:S.blkptr[k + 1]] *= 1.0 + 1e-11
    glob_bad, worst_bad = dense_ref.blockwise(S, bad, case.Yblk)
    assert worst_bad > bound
    assert worst_bad > 0.5e-11
    msk = case.low
    old = np.linalg.norm((bad - case.Yblk)[msk]) / np.linalg.norm(case.Yblk[msk])
    assert old < 1e-10 and glob_bad < 1e-10                 # the old measure passes the same vector


def test_blockwise_zero_blocks_and_nonfinite():
    pat = GPU_PATTERNS["nested"]()
    S = orc.Sym(Symbolic(pat))
    low = dense_ref.lower_mask(S)
    ref = np.random.default_rng(0).standard_normal(S.blklen) * low
    ref[S.blkptr[0]:S.blkptr[1]] = 0.0                       # a clique whose reference block is zero: measured against the whole
    got = ref.copy()
    got[S.blkptr[0]] = 1e-3
    glob, worst = dense_ref.blockwise(S, got, ref)
    assert glob == pytest.approx(1e-3 / np.linalg.norm(ref)) and worst == pytest.approx(glob)
    got[~low] = 5.0                                          # slots outside V are not part of the measure
    assert dense_ref.blockwise(S, got, ref) == (glob, worst)
    got[S.blkptr[1]] = np.nan
    assert dense_ref.blockwise(S, got, ref) == (np.inf, np.inf)
