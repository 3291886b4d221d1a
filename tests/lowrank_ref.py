"""Chordal plus low rank (smcp_amd.chordal.lowrank_factor, csrc/front_lowrank.hip): the numpy restatement of the k x k
construction and the dense definitions.  Shared by tests/test_lowrank_host.py (no GPU) and tests/test_gpu_lowrank.py.

M = Ld Ld^T + V diag(a) V^T = Ld (I + W A W^T) Ld^T with W = Ld^-1 V and K = W^T W.  compact(K, a) returns C, D, S and
sum log t_j with
    (I + W C W^T)(I + W C W^T)^T = I + W A W^T,   (I + W C W^T)^-1 = I + W D W^T,   (I + W A W^T)^-1 = I + W S W^T,
built one column at a time (a_j > 0 first, then a_j < 0, a_j = 0 skipped) from K and a alone.
"""
import numpy as np

EPS = 2.0 ** -52


class NotPositiveDefinite(ArithmeticError):
    def __init__(self, column):
        ArithmeticError.__init__(self, "column %d" % column)
        self.column = column


def column_order(a):
    return [j for j in range(len(a)) if a[j] > 0] + [j for j in range(len(a)) if a[j] < 0]


def compact(K, a, order=None):
    """(C, D, S, sum of log t_j); NotPositiveDefinite(j) when t_j <= 0."""
    a = np.asarray(a, dtype=float)
    k = len(a)
    C = np.zeros((k, k))
    D = np.zeros((k, k))
    logsum = 0.0
    for j in (column_order(a) if order is None else order):
        if a[j] == 0:
            continue
        c = D @ K[:, j]
        c[j] += 1.0
        Kc = K @ c
        t = 1.0 + a[j] * (c @ Kc)
        if not t > 0:
            raise NotPositiveDefinite(j)
        logsum += np.log(t)
        sigma = a[j] / (1.0 + np.sqrt(t))
        tau = sigma / np.sqrt(t)
        C, D = C + sigma * np.outer(c + C @ Kc, c), D - tau * np.outer(c, c + D.T @ Kc)
    S = D + D.T + D.T @ K @ D
    return C, D, S, logsum


class RefFactor:
    """The restatement as an object with the methods of LowRankFactor, on n x kb numpy blocks (returned, not in place)."""

    def __init__(self, Ld, V, a=None):
        import scipy.linalg as sla
        self.sla = sla
        self.Ld = Ld
        self.a = np.ones(V.shape[1]) if a is None else np.asarray(a, dtype=float)
        self.W = sla.solve_triangular(Ld, V, lower=True)
        self.K = self.W.T @ self.W
        self.C, self.D, self.S, self.logsum = compact(self.K, self.a)

    def _mid(self, T, B):
        return B + self.W @ (T @ (self.W.T @ B))

    def trmm(self, B, trans=False):
        return self._mid(self.C.T, self.Ld.T @ B) if trans else self.Ld @ self._mid(self.C, B)

    def trsm(self, B, trans=False):
        if trans:
            return self.sla.solve_triangular(self.Ld.T, self._mid(self.D.T, B), lower=False)
        return self._mid(self.D, self.sla.solve_triangular(self.Ld, B, lower=True))

    def solve(self, B):
        Y = self._mid(self.S, self.sla.solve_triangular(self.Ld, B, lower=True))
        return self.sla.solve_triangular(self.Ld.T, Y, lower=False)

    def mul(self, B):
        return self.Ld @ self._mid(np.diag(self.a), self.Ld.T @ B)

    def logdet(self):
        return 2.0 * np.log(np.diag(self.Ld)).sum() + self.logsum


def dense_M(Ld, V, a=None):
    a = np.ones(V.shape[1]) if a is None else np.asarray(a, dtype=float)
    return Ld @ Ld.T + (V * a) @ V.T


def unit_columns(Ld, V):
    """V with its columns scaled so that |Ld^-1 v_j| = 1."""
    import scipy.linalg as sla
    return V / np.linalg.norm(sla.solve_triangular(Ld, V, lower=True), axis=0)


def coefficients(k, seed, mixed):
    """a drawn from [0.5, 1.5]; mixed: every third entry (1, 4, ...) is -0.5 / k, so that for unit columns of W
    lambda_min(I + W A W^T) >= 1 - sum |a_j| over the negative ones >= 0.5."""
    a = 0.5 + np.random.default_rng(seed).random(k)
    if mixed:
        a[1::3] = -0.5 / k
    return a
