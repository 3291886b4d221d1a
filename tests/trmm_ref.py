"""Products with the supernodal factor (smcp_amd.chordal.trmm, csrc/front_trmm.hip): the test input, the dense
definition with its rounding bound, and a numpy restatement of the device's two-phase schedule.  Shared by
tests/test_trmm_host.py (no GPU) and tests/test_gpu_trmm.py.

Permuted order throughout.  Clique k has columns N = snptr[k] : snptr[k + 1], separator rows A (the last na entries of its
row list) and the panel [L_NN; L_AN] (nf x nn, column-major) at blkptr[k].
    phase 1   N:  X_N = tril(L_NN) B_N,  U_k = L_AN B_N (na x nrhs, one block per clique in the update workspace)
              T:  X_N = tril(L_NN)^T B_N + L_AN^T B[A]
    phase 2   N:  B[i] = alpha (X[i] + sum of U_k[q] over the separator entries (k, q) with row i, ascending k)
              T:  B = alpha X
"""
import numpy as np

U = 2.0 ** -53


def factor_input(symb, seed, junk=np.nan):
    """(blkval, Ld): L on the pattern of symb.sparsity_pattern(), off-diagonal entries of column j
    standard_normal * 0.5 / sqrt(their count), diagonal 1 + random, placed with ccs_to_blk(); every OTHER position of blkval
    (the strict upper triangles of the diagonal blocks) holds `junk`: it is not part of L.  Ld: the dense factor."""
    rng = np.random.default_rng(seed)
    cp, ri = symb.sparsity_pattern()
    cnt = np.maximum(np.diff(cp) - 1, 1)
    J = np.repeat(np.arange(symb.n), np.diff(cp))
    v = rng.standard_normal(len(ri)) * (0.5 / np.sqrt(cnt))[J]
    v[cp[:-1]] = 1.0 + rng.random(symb.n)
    blk = np.full(symb.blklen, junk)
    blk[symb.ccs_to_blk()] = v
    Ld = np.zeros((symb.n, symb.n))
    Ld[ri, J] = v
    return blk, Ld


def product_bound(Ld, B, alpha, trans, factor=2.0):
    """Componentwise |got - ref| <= factor (n + 2) 2^-53 (|alpha| |op(Ld)| @ |B|): the inner-product rounding bound for any
    summation order (gamma_n, plus the rounding of alpha), taken once for the device and once for numpy."""
    n = Ld.shape[0]
    A = np.abs(Ld.T if trans else Ld)
    return factor * (n + 2) * U * (abs(alpha) * (A @ np.abs(B)))


def dense_trmm(Ld, B, alpha, trans):
    return alpha * ((Ld.T if trans else Ld) @ B)


def transposed_separator_index(symb):
    """(tptr, tk, tq): row i of the matrix appears as separator entry q of clique k for the pairs
    (tk[p], tq[p]), p in [tptr[i], tptr[i + 1]), in ascending k.  Built from snptr / rowptr / rowidx / sepptr; the device's
    index (products.hip: trmm_setup) is specified by this one: it keeps tptr and, per separator entry, its position p here, and
    stores U_k[q] at position p, so that the contributions to a row lie side by side in the order of the sum."""
    snptr, rowptr, rowidx, sepptr = symb.snptr, symb.rowptr, symb.rowidx, symb.sepptr
    rows, ks, qs = [], [], []
    for k in range(symb.Nsn):
        nn = snptr[k + 1] - snptr[k]
        A = rowidx[rowptr[k] + nn:rowptr[k + 1]]
        assert len(A) == sepptr[k + 1] - sepptr[k]
        rows.append(np.asarray(A, dtype=np.int64))
        ks.append(np.full(len(A), k, dtype=np.int64))
        qs.append(np.arange(len(A), dtype=np.int64))
    rows, ks, qs = (np.concatenate(x) if x else np.zeros(0, dtype=np.int64) for x in (rows, ks, qs))
    order = np.lexsort((ks, rows))
    tptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=symb.n))]).astype(np.int64)
    assert tptr[-1] == sepptr[-1]
    return tptr, ks[order], qs[order]


def trmm_two_phase(symb, blk, B, alpha, trans):
    """alpha op(L) B by the schedule of the header; B is n x nrhs."""
    n, nrhs = B.shape
    snptr, rowptr, rowidx, sepptr, blkptr = symb.snptr, symb.rowptr, symb.rowidx, symb.sepptr, symb.blkptr
    X = np.zeros_like(B)
    Uw = np.full(int(sepptr[-1]) * nrhs, np.nan)
    for k in range(symb.Nsn):
        f, nn = int(snptr[k]), int(snptr[k + 1] - snptr[k])
        rows = np.asarray(rowidx[rowptr[k]:rowptr[k + 1]], dtype=np.int64)
        nf = len(rows)
        na = nf - nn
        P = blk[blkptr[k]:blkptr[k] + nf * nn].reshape((nf, nn), order="F")
        Lnn, Lan = np.tril(P[:nn]), P[nn:]
        if not trans:
            X[f:f + nn] = Lnn @ B[f:f + nn]
            Uw[int(sepptr[k]) * nrhs:int(sepptr[k]) * nrhs + na * nrhs] = (Lan @ B[f:f + nn]).ravel(order="F")
        else:
            X[f:f + nn] = Lnn.T @ B[f:f + nn] + Lan.T @ B[rows[nn:]]
    if trans:
        return alpha * X
    tptr, tk, tq = transposed_separator_index(symb)
    na_of = np.diff(rowptr) - np.diff(snptr)
    out = np.empty_like(B)
    for i in range(n):
        v = X[i].copy()
        for p in range(tptr[i], tptr[i + 1]):
            k, q = int(tk[p]), int(tq[p])
            v = v + Uw[int(sepptr[k]) * nrhs + q + np.arange(nrhs) * int(na_of[k])]
        out[i] = alpha * v
    return out
