"""Rank-k update and downdate of the supernodal factor (smcp_amd.chordal.chol_update, csrc/front_update.hip): a numpy
restatement of the path walk with the recurrences of the kernel, the dense definitions and the builders of valid input.
Shared by tests/test_chol_update_host.py (no GPU) and tests/test_gpu_chol_update.py.

Permuted order throughout.  `S` is anything with snptr, snpar, rowptr, rowidx and blkptr, as attributes (smcp_amd.Symbolic,
oracle.Sym) or as keys (the dict of oracle.symbolic_ref).  Clique s has the columns N = snptr[s] : snptr[s + 1], the rows
F = rowidx[rowptr[s] : rowptr[s + 1]] (N, then the separator A, ascending) and the nf x nn column-major panel at blkptr[s].

With w = sqrt|a_j| v_j, the step of V column j on panel column c (diagonal d, x = w_c; x == 0: nothing is done):
    r^2 = d^2 + x^2 (a_j > 0) or (d - x)(d + x) (a_j < 0; <= 0: NotPositiveDefinite(j));  rc = d / r, cc = r / d, ss = x / d
    d <- r;  every row i of the panel below c:  l <- (l +- ss w_i) rc,  then  w_i <- cc w_i - ss l
A panel column takes the steps of the columns of V in the order column_order(a): a_j > 0 first, then a_j < 0.
"""
import numpy as np

EPS = 2.0 ** -52
KC = 16                                # columns of V per pass of the device walk (front_update.hip: CU_KC)


class NotPositiveDefinite(ArithmeticError):
    def __init__(self, column):
        ArithmeticError.__init__(self, "column %d" % column)
        self.column = column


def arr(S, name):
    v = S[name] if isinstance(S, dict) else getattr(S, name)
    return np.asarray(v)


def sizes(S):
    snptr, rowptr = arr(S, "snptr"), arr(S, "rowptr")
    return len(snptr) - 1, int(snptr[-1])


def clique_rows(S, s):
    rowptr = arr(S, "rowptr")
    return np.asarray(arr(S, "rowidx")[rowptr[s]:rowptr[s + 1]], dtype=np.int64)


def column_order(a):
    return [j for j in range(len(a)) if a[j] > 0] + [j for j in range(len(a)) if a[j] < 0]


def clique_support_brute(S, idx):
    """the clique whose rows contain all of idx and whose supernode holds min(idx), by a search over every row list; -1"""
    nsn, n = sizes(S)
    snptr = arr(S, "snptr")
    idx = [int(i) for i in idx]
    if not idx or min(idx) < 0 or max(idx) >= n:
        return -1
    for s in range(nsn):
        if snptr[s] <= min(idx) < snptr[s + 1] and set(idx) <= set(clique_rows(S, s).tolist()):
            return s
    return -1


def support_clique(S, v):
    """the clique a column selects, -1 for a column of zeros; ValueError when a nonzero lies outside its rows"""
    nz = np.flatnonzero(v)
    if len(nz) == 0:
        return -1
    s = int(np.searchsorted(arr(S, "snptr"), nz[0], side="right") - 1)
    if not set(nz.tolist()) <= set(clique_rows(S, s).tolist()):
        raise ValueError("support outside clique %d" % s)
    return s


def path_union(S, V, a=None):
    """the cliques on the leaf-to-root paths of the columns of V (n x k) with a_j != 0, from the parent array"""
    par = arr(S, "snpar")
    out = set()
    for j in range(V.shape[1]):
        if a is not None and a[j] == 0:
            continue
        s = support_clique(S, V[:, j])
        while s >= 0 and s not in out:
            out.add(s)
            s = int(par[s])
    return out


def walk(S, blk, V, a=None, order=None):
    """blkval of the factor of L L^T + V diag(a) V^T, by the supernodal walk: the columns in `order` (column_order(a)) in
    passes of KC, every pass visiting the marked cliques in ascending number.  blk is not changed; positions outside the
    lower triangles of the panels, and every clique outside path_union, are returned as they came."""
    nsn, n = sizes(S)
    snptr, rowptr, blkptr = arr(S, "snptr"), arr(S, "rowptr"), arr(S, "blkptr")
    k = V.shape[1]
    a = np.ones(k) if a is None else np.asarray(a, dtype=float)
    if not np.isfinite(a).all():
        raise ValueError("not finite")
    order = column_order(a) if order is None else list(order)
    if not np.isfinite(V[:, order]).all():                           # (a column with a_j = 0 is left out, unread)
        raise ValueError("not finite")
    marks = {j: path_union(S, V[:, [j]]) for j in order}          # (also the support check of every column, before any write)
    out = np.array(blk, dtype=float)
    W = {j: np.sqrt(abs(a[j])) * V[:, j] for j in order}
    for p0 in range(0, len(order), KC):
        cols = order[p0:p0 + KC]
        visit = sorted(set().union(*[marks[j] for j in cols]))
        for s in visit:
            f, nn = int(snptr[s]), int(snptr[s + 1] - snptr[s])
            rows = clique_rows(S, s)
            nf = len(rows)
            P = out[blkptr[s]:blkptr[s] + nf * nn].reshape((nf, nn), order="F")       # a view: written in place
            for c in range(nn):
                below = rows[c + 1:]
                for j in cols:
                    w = W[j]
                    x = w[f + c]
                    if x == 0.0:
                        continue
                    d = P[c, c]
                    t2 = d * d + x * x if a[j] > 0 else (d - x) * (d + x)
                    if not t2 > 0:
                        raise NotPositiveDefinite(j)
                    r = np.sqrt(t2)
                    rc, cc, ss = d / r, r / d, x / d
                    P[c, c] = r
                    l = (P[c + 1:, c] + (ss if a[j] > 0 else -ss) * w[below]) * rc
                    w[below] = cc * w[below] - ss * l
                    P[c + 1:, c] = l
    return out


def rank_one_walks(S, blk, V, a=None):
    """the same matrix by len(order) successive walks of one column each, in the order of column_order(a)"""
    k = V.shape[1]
    a = np.ones(k) if a is None else np.asarray(a, dtype=float)
    out = np.array(blk, dtype=float)
    for j in column_order(a):
        out = walk(S, out, V[:, [j]], a[[j]])
    return out


def dense_factor(S, blk):
    """the dense lower-triangular factor that blkval holds"""
    nsn, n = sizes(S)
    snptr, blkptr = arr(S, "snptr"), arr(S, "blkptr")
    Ld = np.zeros((n, n))
    for s in range(nsn):
        f, nn = int(snptr[s]), int(snptr[s + 1] - snptr[s])
        rows = clique_rows(S, s)
        P = np.asarray(blk[blkptr[s]:blkptr[s] + len(rows) * nn]).reshape((len(rows), nn), order="F")
        for c in range(nn):
            Ld[rows[c:], f + c] = P[c:, c]
    return Ld


def random_factor(S, seed, junk=np.nan):
    """(blkval, dense Ld) of a factor on the pattern: off-diagonal entries of a column standard_normal * 0.5 / sqrt(their
    count), diagonal 1 + random (the recipe of trmm_ref.factor_input); the strict upper triangles of the panels hold `junk`"""
    rng = np.random.default_rng(seed)
    nsn, n = sizes(S)
    snptr, blkptr = arr(S, "snptr"), arr(S, "blkptr")
    blk = np.full(int(blkptr[-1]), junk)
    for s in range(nsn):
        nn = int(snptr[s + 1] - snptr[s])
        nf = len(clique_rows(S, s))
        P = blk[blkptr[s]:blkptr[s] + nf * nn].reshape((nf, nn), order="F")
        for c in range(nn):
            P[c + 1:, c] = rng.standard_normal(nf - c - 1) * 0.5 / np.sqrt(max(nf - c - 1, 1))
            P[c, c] = 1.0 + rng.random()
    return blk, dense_factor(S, blk)


def pattern_mask(S):
    nsn, n = sizes(S)
    snptr = arr(S, "snptr")
    M = np.zeros((n, n), dtype=bool)
    for s in range(nsn):
        rows = clique_rows(S, s)
        N = np.arange(snptr[s], snptr[s + 1])
        M[np.ix_(rows, N)] = True
        M[np.ix_(N, rows)] = True
    return M


def support_columns(S, k, seed, leaves_first=False):
    """n x k: column j has its support inside one clique, from a random column of that supernode on: the clique is drawn at
    random (leaves_first: the cliques without children come first, one column each, so that paths start in different
    leaves and merge), about three rows in four below the first are kept"""
    rng = np.random.default_rng(seed)
    nsn, n = sizes(S)
    snptr, par = arr(S, "snptr"), arr(S, "snpar")
    parents = set(par.tolist())
    leaves = [s for s in range(nsn) if s not in parents]
    V = np.zeros((n, k))
    for j in range(k):
        s = leaves[j] if leaves_first and j < len(leaves) else int(rng.integers(nsn))
        rows = clique_rows(S, s)
        t0 = int(rng.integers(snptr[s + 1] - snptr[s]))
        keep = rows[t0:][np.concatenate([[True], rng.random(len(rows) - t0 - 1) < 0.75])]
        V[keep, j] = rng.standard_normal(len(keep))
        V[keep[0], j] = 1.0 + rng.random()
    return V


def unit_columns(Ld, V):
    """V with its columns scaled so that |Ld^-1 v_j| = 1 (columns of zeros stay)"""
    import scipy.linalg as sla
    nrm = np.linalg.norm(sla.solve_triangular(Ld, V, lower=True), axis=0)
    return V / np.where(nrm > 0, nrm, 1.0)


def coefficients(k, seed, signs):
    """updates from [0.5, 1.5]; downdates -0.5 / k, so that for unit columns of L^-1 V the smallest eigenvalue of
    I + W A W^T stays above 0.5.  signs: "plus", "minus", or "mixed" (every third, 1, 4, ..., negative)"""
    a = 0.5 + np.random.default_rng(seed).random(k)
    if signs == "minus":
        a[:] = -0.5 / k
    elif signs == "mixed":
        a[1::3] = -0.5 / k
    return a


def dense_M(Ld, V, a=None):
    a = np.ones(V.shape[1]) if a is None else np.asarray(a, dtype=float)
    return Ld @ Ld.T + (V * a) @ V.T


def eta(mask, Lnew, M):
    """|P_V(L' L'^T - M)|_F / |M|_F"""
    return float(np.linalg.norm(np.where(mask, Lnew @ Lnew.T - M, 0.0)) / np.linalg.norm(M))


def yardstick(mask, M):
    """the same measure for numpy.linalg.cholesky(M), floored at n eps"""
    return max(eta(mask, np.linalg.cholesky(M), M), M.shape[0] * EPS)
