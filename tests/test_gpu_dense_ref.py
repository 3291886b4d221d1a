"""GPU: every device operation against its DENSE definition (tests/dense_ref.py), measured per clique.

The parity suite compares the device with the CPU oracle at 1e-9 .. 1e-10 over whole vectors; here the same operations run
against plain numpy / LAPACK on every entry of GPU_PATTERNS, and an error confined to one small clique counts in full
(dense_ref.blockwise).  Bound per operation: 100 x the oracle-vs-dense worst case recorded in
tests/golden/dense_ref_yardstick.json, never looser than 1e-12 (dense_ref.device_bound states the reasoning).

Measured device-vs-dense worst cases (MI355X, every pattern, every route of this file), against the bound in force:

    operation             device worst   bound      worst case
    cholesky              1.0e-16        4.1e-14    rand1
    llt                   2.1e-16        1.8e-14    rand1
    projected_inverse     8.5e-16        8.4e-14    dense600 (cholesky_projected_inverse in one call)
    completion            2.4e-16        6.4e-14    fam_top
    logdiagsum            2.1e-16        1.7e-13    fam_top
    dot                   1.4e-16        1.2e-13    dense200
    hessian               1.7e-15        1.9e-13    fam_top, 2 right-hand sides (dense600 with one: 1.6e-15)
    hessian_inv           2.3e-15        2.6e-13    rand2, 4 right-hand sides
    hessian_gadj_g        1.8e-15        2.0e-13    fam_top, 9 right-hand sides on max_rhs = 4
    hessian_gram          6.2e-16        4.4e-14    arrow_big, 4 right-hand sides
    hessian_adjoint       6.5e-17        6.9e-15    arrow
    hessian_factor_inv    1.7e-15        1.7e-13    dense600
    trsm                  8.5e-16        8.6e-14    dense600
    kkt_H                 5.9e-16        2.3e-13    nested, factor_qr (factor: 4.8e-16, rand1)
    kkt_y                 1.6e-15        4.9e-13    arrow_one, factor
    kkt_x                 2.0e-15        2.0e-13    arrow_one, factor_qr

The device is as close to the dense definitions as the CPU oracle is (the yardstick values are the bounds / 100): no bound was
exceeded and none was raised.  The Hessian rows include the runs of tests/test_gpu_contract.py with more right-hand sides than
max_rhs.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from smcp_amd import chordal
from smcp_amd.symbolic import Symbolic
from tests import dense_ref
from tests.helpers import GPU_PATTERNS

pytestmark = pytest.mark.gpu
NAMES = sorted(GPU_PATTERNS)
# patterns whose trees have small parents with childless children: the closed-form Gram route can be forced there
FAMILY_PATTERNS = ["nested", "nested_mid", "fam_max", "fam_odd", "fam_nine", "fam_top"]


@pytest.fixture(scope="module")
def yard():
    return dense_ref.load_yardstick()


@pytest.fixture(scope="module")
def cases():
    """name -> (Symbolic with a device context, DenseCase): the dense matrices (an inverse and a few products, n <= 1000) are
    formed once per pattern and module."""
    cache = {}

    def get(name):
        if name not in cache:
            pat = GPU_PATTERNS[name]()
            symb = Symbolic(pat)
            symb.device_init(0, 4)
            cache[name] = (symb, dense_ref.DenseCase(pat, orc.Sym(symb), dense_ref.YARDSTICK_SEED))
        return cache[name]

    return get


def check(tag, errs, yard):
    print("DENSEREF", tag, " ".join("%s=%.2e" % kv for kv in sorted(errs.items())))
    bad = {op: (e, dense_ref.device_bound(op, yard)) for op, e in errs.items() if not e <= dense_ref.device_bound(op, yard)}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("name", NAMES)
def test_tree_operations_and_trsm(name, cases, yard):
    symb, case = cases(name)
    ops = dense_ref.device_ops(symb, case)
    errs = dense_ref.measure(case, ops, parts=("tree", "trsm"))
    check("tree %s" % name, errs, yard)
    # the dual scaling point in ONE call, with and without the separator factors left behind
    for factors in (True, False):
        L, Y = dense_ref.to_dev(symb, case.Ablk), dense_ref.to_dev(symb, np.zeros(symb.blklen))
        chordal.cholesky_projected_inverse(L, Y, factors=factors)
        errs = {"cholesky": dense_ref.blockwise(case.S, dense_ref.to_host(L), case.cholesky())[1],
                "projected_inverse": dense_ref.blockwise(case.S, dense_ref.to_host(Y), case.Yblk)[1]}
        check("scaling_point %s factors=%d" % (name, factors), errs, yard)


@pytest.mark.parametrize("nrhs", [1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_hessian_all_modes(name, nrhs, cases, yard):
    """All six modes: the two full ones against P_V(Ai U Ai) and its preimage, the four factor modes through the identities
    of dense_ref with densely evaluated right-hand sides.  One right-hand side takes the resident single-RHS sweeps, four the
    batched (family) kernels."""
    symb, case = cases(name)
    ops = dense_ref.device_ops(symb, case)
    errs = dense_ref.measure(case, ops, nrhs=nrhs, parts=("hessian",))
    check("hessian %s nrhs=%d" % (name, nrhs), errs, yard)


@pytest.mark.parametrize("route", ["chol", "chol_tnz0", "qr"])
@pytest.mark.parametrize("name", NAMES)
def test_kkt_against_dense(name, route, cases, yard):
    """Schur complement, y and x (per clique) of KKTSystem.factor with the reference's tnzcols default (column-sparse
    constraints take the SCMcolumn2 route) and with tnzcols = 0 (every constraint swept), and of factor_qr."""
    symb, case = cases(name)
    kkt = dense_ref.device_kkt(symb, route="qr" if route == "qr" else "chol", tnzcols=0.0 if route == "chol_tnz0" else None)
    check("kkt %s %s" % (name, route), dense_ref.kkt_errors(case, kkt), yard)


@pytest.mark.parametrize("name", FAMILY_PATTERNS)
def test_kkt_closed_form_gram_against_dense(name, cases, yard):
    """TUNE_LEAFGRAM = 2: the children's Gram blocks in closed form wherever the tree has families (the cost rule would not
    pick the route on problems this small)."""
    symb, case = cases(name)
    chordal.tune(symb, chordal.TUNE_LEAFGRAM, 2)
    try:
        check("kkt %s leafgram" % name, dense_ref.kkt_errors(case, dense_ref.device_kkt(symb, tnzcols=0.0)), yard)
    finally:
        chordal.tune(symb, chordal.TUNE_LEAFGRAM, 1)
