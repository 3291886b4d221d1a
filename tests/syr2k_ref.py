"""Rank-k updates projected on the chordal pattern (smcp_amd.chordal.syr2k / syrk / syr2, csrc/front_syr2k.hip): the test
input, the dense definition with its rounding bound, and a numpy restatement of the device's per-clique schedule on
blkval.  Shared by tests/test_syr2k_host.py (no GPU) and tests/test_gpu_syr2k.py.

Permuted order throughout.  U, V are n x k numpy arrays (column r = rank r); V None is the syrk form U U^T.  Clique c has
columns N = snptr[c] : snptr[c + 1], front rows F = rowidx[rowptr[c] : rowptr[c + 1]] = [N; A] and the panel (nf x nn,
column-major) at blkptr[c]:
    panel[m, j] = beta panel[m, j] + alpha sum_r (U[F_m, r] V[N_j, r] + V[F_m, r] U[N_j, r])
on the rows m >= j of the N N part and all rows of the A N part; every other slot of blkval (the strict upper triangles of
the N N blocks) is not read and becomes exactly 0.0.  A term whose factor (alpha or beta) is zero is left out, not
multiplied by zero.
"""
import numpy as np

EPS = 2.0 ** -53


def owned(symb):
    """boolean mask over blkval: the slots that hold an entry of the pattern"""
    msk = np.zeros(symb.blklen, dtype=bool)
    msk[symb.ccs_to_blk()] = True
    return msk


def lower_index(symb):
    """(rows, cols) of the lower-triangular entries of the pattern, in the order of ccs_to_blk()"""
    cp, ri = symb.sparsity_pattern()
    return np.asarray(ri), np.repeat(np.arange(symb.n), np.diff(cp))


def pattern_mask(symb):
    I, J = lower_index(symb)
    M = np.zeros((symb.n, symb.n), dtype=bool)
    M[I, J] = True
    M[J, I] = True
    return M


def matrix_input(symb, seed, junk=np.nan):
    """(blkval, Xd): a symmetric matrix with standard normal entries on the pattern, `junk` in every slot of blkval outside
    it; Xd its dense form."""
    I, J = lower_index(symb)
    v = np.random.default_rng(seed).standard_normal(len(I))
    blk = np.full(symb.blklen, junk)
    blk[symb.ccs_to_blk()] = v
    Xd = np.zeros((symb.n, symb.n))
    Xd[I, J] = v
    Xd[J, I] = v
    return blk, Xd


def to_dense(symb, blk):
    I, J = lower_index(symb)
    v = blk[symb.ccs_to_blk()]
    Xd = np.zeros((symb.n, symb.n))
    Xd[I, J] = v
    Xd[J, I] = v
    return Xd


def dense_syr2k(Xd, mask, U, V, alpha, beta):
    """beta Xd + alpha mask o (U V^T + V U^T) (V None: U U^T); a term with a zero factor is left out"""
    out = np.zeros_like(Xd)
    if beta != 0:
        out = beta * Xd
    if alpha != 0:
        T = U @ U.T if V is None else U @ V.T + V @ U.T
        out = out + alpha * np.where(mask, T, 0.0)
    return out


def syr2k_bound(Xd, U, V, alpha, beta):
    """Componentwise |got - ref| <= 2 (2k + 4) 2^-53 (|beta| |Xd| + |alpha| (|U| |V|^T + |V| |U|^T)): the inner-product rounding
    bound for any summation order (gamma_2k) plus the roundings of alpha and beta, taken once for the device and once for
    numpy -- the construction of trmm_ref.product_bound."""
    k = U.shape[1]
    aU = np.abs(U)
    T = aU @ aU.T if V is None else aU @ np.abs(V).T + np.abs(V) @ aU.T
    return 2.0 * (2 * k + 4) * EPS * (abs(beta) * np.abs(Xd) + abs(alpha) * T)


def syr2k_per_clique(symb, blk, U, V, alpha, beta):
    """The update by the schedule of the header: a new blkval."""
    snptr, rowptr, rowidx, blkptr = symb.snptr, symb.rowptr, symb.rowidx, symb.blkptr
    out = np.empty(symb.blklen)
    k = U.shape[1]
    for c in range(symb.Nsn):
        nn = int(snptr[c + 1] - snptr[c])
        F = np.asarray(rowidx[rowptr[c]:rowptr[c + 1]], dtype=np.int64)
        N = F[:nn]
        nf = len(F)
        own = np.arange(nf)[:, None] >= np.arange(nn)[None, :]
        acc = np.zeros((nf, nn))
        if alpha != 0:
            for r in range(k):                                   # ascending rank, the order of the device's FMA kernel
                if V is None:
                    acc = acc + np.outer(U[F, r], U[N, r])
                else:
                    acc = acc + np.outer(U[F, r], V[N, r])
                    acc = acc + np.outer(V[F, r], U[N, r])
        new = np.zeros((nf, nn))
        if beta != 0:
            P = blk[blkptr[c]:blkptr[c] + nf * nn].reshape((nf, nn), order="F")
            new[own] = beta * P[own]                             # (the slots above the diagonal are not read)
        if alpha != 0:
            new[own] = new[own] + alpha * acc[own]
        out[blkptr[c]:blkptr[c] + nf * nn] = new.ravel(order="F")
    assert blkptr[symb.Nsn] == symb.blklen if len(blkptr) > symb.Nsn else True
    return out
