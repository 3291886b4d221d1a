"""Products of a chordal symmetric matrix with a dense block (smcp_amd.chordal.symm, csrc/front_symm.hip): the dense
definition with its rounding bound, and a numpy restatement of the device's two-phase schedule and of its contribution
index.  Shared by tests/test_symm_host.py (no GPU) and tests/test_gpu_symm.py.  The input is syr2k_ref.matrix_input: a
symmetric matrix with N(0, 1) entries on the pattern and NaN in every slot of blkval outside it.

Permuted order throughout; B and C are n x nrhs.  Clique k has columns N = snptr[k] : snptr[k + 1], front rows
F = rowidx[rowptr[k] : rowptr[k + 1]] = [N; A] and the panel P (nf x nn, column-major) at blkptr[k].

    item (k, r, p)   the panel rows rows * r .. rows * r + rows - 1 (clipped to nf) and the panel columns
                     kp * p .. kp * p + kp - 1 (clipped to nn); listed when kp * p <= last, the last row of the chunk:
                     otherwise every entry of it lies above the diagonal of the N N block
    row partial      of each row m of the item:  sum over its columns kk of P[m, kk] B[N_kk] (m < nn: only kk <= m, the
                     diagonal is taken here); target row F_m of C
    column partial   of each column kk < last of the item:  sum over its rows m > kk of P[m, kk] B[F_m]; target row N_kk
    index            row i of C owns the positions [tptr[i], tptr[i + 1]) of the list of all partials, its own in
                     ascending (k, side, r, p), side 0 = row partial, 1 = column partial
    phase 1          every partial is stored at its position
    phase 2          C[i] = beta C[i] + alpha (the run of row i summed in ascending position), a term with a zero factor
                     left out
The device uses rows = 64, kp = 256 (SYMM_ROWS, SYMM_KP).
"""
import numpy as np

from tests.syr2k_ref import matrix_input  # noqa: F401  (the input of every symm test)

EPS = 2.0 ** -53


def dense_symm(Xd, B, C, alpha, beta):
    """alpha Xd B + beta C; a term with a zero factor is left out (C may be None for beta == 0)"""
    out = np.zeros_like(B)
    if beta != 0:
        out = beta * C
    if alpha != 0:
        out = out + alpha * (Xd @ B)
    return out


def symm_bound(Xd, B, C, alpha, beta):
    """Componentwise |got - ref| <= 2 (n + 4) 2^-53 (|beta| |C| + |alpha| |Xd| |B|).  An inner product of at most n terms in
    any order, with the roundings of its products, is within n u of its value relative to sum |terms| (gamma_n); the
    rounding of alpha, of beta C and of the last add make n + 3, and one more absorbs the second-order terms.  Taken once
    for the device and once for numpy: the factor 2 (the construction of trmm_ref.product_bound)."""
    n = Xd.shape[0]
    t = abs(alpha) * (np.abs(Xd) @ np.abs(B))
    if beta != 0:
        t = t + abs(beta) * np.abs(C)
    return 2.0 * (n + 4) * EPS * t


def composed_bound(Ld, B):
    """Bound on |symm(S, B) - trmm_N(trmm_T(B))| for S = llt(L), both sides computed on the device, in terms of
    T = |Ld| |Ld^T| |B|, with u = 2^-53 and second-order terms left to the slack named at the end.
        S~ = fl(Ld Ld^T) on the pattern (exact zero fill: Ld Ld^T has no entry outside it):  |S~ - S| <= (n + 1) u |Ld| |Ld^T|
        symm:    |fl(S~ B) - S~ B| <= (n + 4) u |S~| |B| <= (n + 4) u T,   and |S~ B - S B| <= (n + 1) u T
        trmm T:  y = fl(Ld^T B),  |y - Ld^T B| <= (n + 2) u |Ld^T| |B|,  which Ld carries to (n + 2) u T
        trmm N:  |fl(Ld y) - Ld y| <= (n + 2) u |Ld| |y| <= (n + 2) u T
    together (4 n + 11) u T.  The test takes the sum of the three calls' own test bounds, each of which carries the factor 2
    of a comparison with numpy that is not made here: symm_bound 2 (n + 4) u T and trmm_ref.product_bound 2 (n + 2) u T
    twice, (6 n + 16) u T; the difference (2 n + 5) u T covers the rounding of llt and the second-order terms."""
    n = Ld.shape[0]
    T = np.abs(Ld) @ (np.abs(Ld.T) @ np.abs(B))
    return (2.0 * (n + 4) + 2 * 2.0 * (n + 2)) * EPS * T


def items_of(symb, rows=64, kp=256):
    """The listed items in ascending (k, r, p): tuples (k, r, p, rows of the chunk, columns with a column partial)."""
    out = []
    nn_all, nf_all = np.diff(symb.snptr), np.diff(symb.rowptr)
    for k in range(symb.Nsn):
        nn, nf = int(nn_all[k]), int(nf_all[k])
        for r in range(-(-nf // rows)):
            last = min(rows * r + rows, nf) - 1
            for p in range(-(-nn // kp)):
                if kp * p > last:
                    continue
                out.append((k, r, p, last - rows * r + 1, max(0, min(nn, kp * p + kp, last) - kp * p)))
    return out


def contribution_index(symb, rows=64, kp=256):
    """(tptr, rec): rec is an (ntot, 5) array whose row q = (k, side, r, p, j) names the partial at position q: side 0 the
    row partial of row rows * r + j of item (k, r, p), side 1 the column partial of its column kp * p + j.  Row i of the
    matrix owns the positions tptr[i] : tptr[i + 1], in ascending (k, side, r, p).  The device's index (products.hip:
    symm_setup) is specified by this one; csp_symm_positions returns len(rec)."""
    snptr, rowptr, rowidx = symb.snptr, symb.rowptr, symb.rowidx
    tgt, rec = [], []
    for k, r, p, nrows, ncol in items_of(symb, rows, kp):
        F = rowidx[rowptr[k]:rowptr[k + 1]]
        for j in range(nrows):
            tgt.append(int(F[rows * r + j]))
            rec.append((k, 0, r, p, j))
        for j in range(ncol):
            tgt.append(int(snptr[k]) + kp * p + j)
            rec.append((k, 1, r, p, j))
    tgt = np.asarray(tgt, dtype=np.int64)
    rec = np.asarray(rec, dtype=np.int64).reshape((-1, 5))
    order = np.lexsort((rec[:, 3], rec[:, 2], rec[:, 1], rec[:, 0], tgt))
    tptr = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=symb.n))]).astype(np.int64)
    return tptr, rec[order]


def symm_two_phase(symb, blk, B, C, alpha, beta, rows=64, kp=256):
    """alpha X B + beta C by the schedule of the header; B, C are n x nrhs (C is not read for beta == 0)."""
    n, nrhs = B.shape
    snptr, rowptr, rowidx, blkptr = symb.snptr, symb.rowptr, symb.rowidx, symb.blkptr
    tptr, rec = contribution_index(symb, rows, kp)
    where = {tuple(int(x) for x in rec[q]): q for q in range(len(rec))}
    assert len(where) == len(rec)
    Uw = np.full((len(rec), nrhs), np.nan)
    if alpha != 0:                                           # phase 1 (alpha == 0: neither X nor B is read)
        for k, r, p, nrows, ncol in items_of(symb, rows, kp):
            nn = int(snptr[k + 1] - snptr[k])
            F = np.asarray(rowidx[rowptr[k]:rowptr[k + 1]], dtype=np.int64)
            nf = len(F)
            P = blk[blkptr[k]:blkptr[k] + nf * nn].reshape((nf, nn), order="F")
            m = np.arange(rows * r, rows * r + nrows)
            kk = np.arange(kp * p, min(nn, kp * p + kp))
            sub = P[np.ix_(m, kk)]
            counts = (m[:, None] >= nn) | (kk[None, :] <= m[:, None])        # of the N N block: the lower triangle
            below = m[:, None] > kk[None, :]                                 # strictly below the diagonal
            rowp = np.where(counts, sub, 0.0) @ B[F[kk]]
            colp = np.where(below, sub, 0.0).T @ B[F[m]]
            for j in range(nrows):
                Uw[where[(k, 0, r, p, j)]] = rowp[j]
            for j in range(ncol):
                Uw[where[(k, 1, r, p, j)]] = colp[j]
    out = np.empty_like(B)
    for i in range(n):                                       # phase 2
        s = np.zeros(nrhs)
        if alpha != 0:
            for q in range(tptr[i], tptr[i + 1]):
                s = s + Uw[q]
        if alpha != 0 and beta != 0:
            out[i] = beta * C[i] + alpha * s
        elif alpha != 0:
            out[i] = alpha * s
        elif beta != 0:
            out[i] = beta * C[i]
        else:
            out[i] = 0.0
    return out
