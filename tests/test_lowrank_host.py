"""The k x k construction behind chordal.lowrank_factor (tests/lowrank_ref.py: the numpy restatement of k_lr_small) against
the dense definitions, on dense random lower factors, and the argument checks of lowrank_factor, which must raise before a
device is needed.  Bounds: 100 n eps cond(I + W A W^T) relative to the norms of the factors of the identity under test --
every identity is a product of a few matrices of order n whose rounding errors the condition number of the middle factor
amplifies at most once."""
import numpy as np
import pytest
import torch

from smcp_amd import chordal, problems
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic
from tests.lowrank_ref import EPS, NotPositiveDefinite, RefFactor, coefficients, compact, dense_M, unit_columns

RANKS = (1, 7, 8, 17, 64)
ORDERS = {1: 29, 7: 40, 8: 64, 17: 200, 64: 101}       # order of the factor per rank (29 ... 200)


def factor(n, seed):
    rng = np.random.default_rng(seed)
    Ld = np.tril(rng.standard_normal((n, n)) * 0.3)
    Ld[np.diag_indices(n)] = 1.0 + rng.random(n)
    return Ld


def setting(k, mixed, seed=0):
    n = ORDERS[k]
    Ld = factor(n, 10 + k + seed)
    V = unit_columns(Ld, np.random.default_rng(20 + k + seed).standard_normal((n, k)))
    a = coefficients(k, 30 + k + seed, mixed)
    R = RefFactor(Ld, V, a)
    G = np.eye(n) + R.W @ np.diag(a) @ R.W.T
    return n, Ld, V, a, R, 100 * n * EPS * np.linalg.cond(G)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("k", RANKS)
def test_identities(k, mixed):
    n, Ld, V, a, R, tol = setting(k, mixed)
    M = dense_M(Ld, V, a)
    I = np.eye(n)
    P = I + R.W @ R.C @ R.W.T
    F = Ld @ P
    assert np.linalg.norm(F @ F.T - M, 2) <= tol * np.linalg.norm(F, 2) ** 2
    Pi = I + R.W @ R.D @ R.W.T
    assert np.linalg.norm(P @ Pi - I, 2) <= tol * np.linalg.norm(P, 2) * np.linalg.norm(Pi, 2)
    Sref = -np.linalg.inv(np.diag(1.0 / a) + R.K)          # a has no zero entry here
    assert np.linalg.norm(R.S - Sref, 2) <= tol * np.linalg.cond(np.diag(1.0 / a) + R.K) * np.linalg.norm(Sref, 2)
    sign, ld = np.linalg.slogdet(M)
    assert sign > 0 and abs(R.logdet() - ld) <= tol * n
    B = np.random.default_rng(5).standard_normal((n, 3))
    assert np.linalg.norm(R.mul(B) - M @ B) <= tol * np.linalg.norm(M, 2) * np.linalg.norm(B)
    X = R.solve(B)
    assert np.linalg.norm(M @ X - B) <= tol * np.linalg.norm(M, 2) * np.linalg.norm(X)
    assert np.linalg.norm(R.trmm(R.trmm(B, True)) - M @ B) <= tol * np.linalg.norm(M, 2) * np.linalg.norm(B)
    for trans in (False, True):
        assert np.linalg.norm(R.trsm(R.trmm(B, trans), trans) - B) <= tol * np.linalg.cond(F) * np.linalg.norm(B)


@pytest.mark.parametrize("k", RANKS[1:])
def test_order_of_the_columns(k):
    """the columns in another order: the same M, so the same S (it is unique), the same log-determinant and again F F^T = M"""
    n, Ld, V, a, R, tol = setting(k, True)
    p = np.random.default_rng(k).permutation(k)
    Rp = RefFactor(Ld, V[:, p], a[p])
    assert np.linalg.norm(Rp.S - R.S[np.ix_(p, p)], 2) <= tol * np.linalg.cond(np.diag(1.0 / a) + R.K) * np.linalg.norm(R.S, 2)
    assert abs(Rp.logdet() - R.logdet()) <= tol * n
    Fp = Ld @ (np.eye(n) + Rp.W @ Rp.C @ Rp.W.T)
    assert np.linalg.norm(Fp @ Fp.T - dense_M(Ld, V, a), 2) <= tol * np.linalg.norm(Fp, 2) ** 2
    # and within the same sign class the construction may take any order
    order = list(reversed([j for j in range(k) if a[j] > 0])) + [j for j in range(k) if a[j] < 0]
    C2, D2, S2, ls2 = compact(R.K, a, order)
    assert np.linalg.norm(S2 - R.S, 2) <= tol * np.linalg.cond(np.diag(1.0 / a) + R.K) * np.linalg.norm(R.S, 2)
    assert abs(ls2 - R.logsum) <= tol * n


@pytest.mark.parametrize("k", RANKS[1:])
def test_zero_coefficients_change_nothing(k):
    n, Ld, V, a, R, tol = setting(k, True)
    a0 = a.copy()
    a0[::2] = 0.0
    keep = np.flatnonzero(a0)
    R0 = RefFactor(Ld, V, a0)
    Rk = RefFactor(Ld, V[:, keep], a0[keep])
    for full, part in ((R0.C, Rk.C), (R0.D, Rk.D), (R0.S, Rk.S)):
        assert np.linalg.norm(full[np.ix_(keep, keep)] - part, 2) <= tol * max(1.0, np.linalg.norm(part, 2))
        rest = full.copy()
        rest[np.ix_(keep, keep)] = 0.0
        assert not rest.any()                                        # exact zeros: a skipped column never enters
    assert abs(R0.logsum - Rk.logsum) <= tol * n


def test_not_positive_definite_names_the_column():
    n, Ld, V, a, R, tol = setting(7, False)
    bad = np.zeros(7)
    bad[1] = -1.5 / R.K[1, 1]
    with pytest.raises(NotPositiveDefinite) as e:
        compact(R.K, bad)
    assert e.value.column == 1
    assert np.linalg.eigvalsh(dense_M(Ld, V, bad)).min() < 0


def test_argument_checks_need_no_device():
    symb = Symbolic(problems.band_pattern(30, 3))
    L = cspmatrix(symb, torch.ones(symb.blklen, dtype=torch.float64))
    n = symb.n
    assert symb._device is None
    for V in (torch.zeros((0, n), dtype=torch.float64), torch.zeros((65, n), dtype=torch.float64),
              torch.zeros((3, n), dtype=torch.float32), torch.zeros((3, n + 1), dtype=torch.float64),
              torch.zeros((n, 3), dtype=torch.float64).T, torch.zeros(n, dtype=torch.float64)):
        with pytest.raises(ValueError):
            chordal.lowrank_factor(L, V)
    with pytest.raises(ValueError):
        chordal.lowrank_factor(L, torch.zeros((3, n), dtype=torch.float64), a=[1.0, 2.0])
    with pytest.raises(ValueError):                                  # a host tensor: refused, not copied
        chordal.lowrank_factor(L, torch.zeros((3, n), dtype=torch.float64))
    assert symb._device is None                                      # nothing above initialised a device
