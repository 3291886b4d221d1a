"""The factor as a sum of positive semidefinite clique blocks (smcp_amd.chordal.clique_decompose, csrc/front_cdec.hip): a
numpy restatement on blkval, the rounding bounds and the helpers of the packed layout.  Shared by
tests/test_clique_decompose_host.py (no GPU) and tests/test_gpu_clique_decompose.py.

Permuted order throughout.  `S` is anything with snptr, rowptr, rowidx and blkptr, as attributes (smcp_amd.Symbolic,
oracle.Sym) or as keys (the dict of oracle.symbolic_ref), as in tests/chol_update_ref.py.  Clique k has nn own columns and
nf = nn + na rows; its panel P is nf x nn, column-major with leading dimension nf, at blkptr[k].  With Pt[m, c] = P[m, c]
for m >= c and 0 otherwise (the slots m < c < nn are never read)
    Z_k[i, j] = sum_{c = 0}^{min(i, j, nn - 1)} Pt[i, c] Pt[j, c],        0 <= i, j < nf,        c ascending,
stored at qptr[k] + i + j nf of the packed block tensor.  Every column of L belongs to one supernode and its nonzeros lie
in that clique's rows, so L L^T = sum_k E_k Z_k E_k^T; Z_k = Pt Pt^T is positive semidefinite of rank <= nn.
"""
import numpy as np

from tests.chol_update_ref import arr, clique_rows, dense_factor, pattern_mask, random_factor, sizes  # noqa: F401

EPS = 2.0 ** -53


def panel(S, blk, k, dtype=np.float64):
    """Pt of clique k (nf x nn): the owned slots of the panel, zeros above the diagonal, which are not read"""
    snptr, blkptr = arr(S, "snptr"), arr(S, "blkptr")
    nn = int(snptr[k + 1] - snptr[k])
    nf = len(clique_rows(S, k))
    P = np.asarray(blk[blkptr[k]:blkptr[k] + nf * nn]).reshape((nf, nn), order="F")
    Pt = np.zeros((nf, nn), dtype=dtype)
    for c in range(nn):
        Pt[c:, c] = P[c:, c]
    return Pt


def decompose(S, blk):
    """the blocks Z_k by the definition, c ascending: a list of nf x nf arrays"""
    out = []
    for k in range(sizes(S)[0]):
        Pt = panel(S, blk, k)
        Z = np.zeros((Pt.shape[0], Pt.shape[0]))
        for c in range(Pt.shape[1]):
            Z = Z + np.outer(Pt[:, c], Pt[:, c])
        out.append(Z)
    return out


def exact(S, blk):
    """Pt Pt^T of every clique in long double"""
    out = []
    for k in range(sizes(S)[0]):
        Pt = panel(S, blk, k, dtype=np.longdouble)
        out.append(Pt @ Pt.T)
    return out


def bounds(S, blk):
    """B_k = 2 (nn + 2) 2^-53 |Pt| |Pt|^T: the inner-product rounding bound of nn terms for any summation order (gamma_nn
    with room for the roundings of the reference), taken once for each side -- the construction of syr2k_ref.syr2k_bound"""
    out = []
    for k in range(sizes(S)[0]):
        aP = np.abs(panel(S, blk, k))
        out.append(2.0 * (aP.shape[1] + 2) * EPS * (aP @ aP.T))
    return out


def sum_bound(Ld):
    """2 (n + 4) 2^-53 |L| |L|^T: the same bound for the dense product of n terms"""
    aL = np.abs(Ld)
    return 2.0 * (Ld.shape[0] + 4) * EPS * (aL @ aL.T)


def unowned(S):
    """boolean mask over blkval: the slots above the diagonals of the N N blocks, which hold no entry of the pattern"""
    snptr, blkptr = arr(S, "snptr"), arr(S, "blkptr")
    msk = np.zeros(int(blkptr[-1]), dtype=bool)
    for k in range(sizes(S)[0]):
        nn = int(snptr[k + 1] - snptr[k])
        nf = len(clique_rows(S, k))
        M = msk[blkptr[k]:blkptr[k] + nf * nn].reshape((nf, nn), order="F")       # a view
        M[:nn, :][np.triu_indices(nn, 1)] = True
    return msk


# ---- the packed layout (chordal.clique_ptr) -----------------------------------------------------------------------------
def qptr(S):
    rowptr = arr(S, "rowptr")
    q = np.zeros(len(rowptr), dtype=np.int64)
    q[1:] = np.cumsum(np.diff(rowptr) ** 2)
    return q


def pack(blocks):
    return np.concatenate([np.asarray(Z).ravel(order="F") for Z in blocks]) if blocks else np.zeros(0)


def unpack(S, Z):
    """the nf x nf blocks of the packed tensor Z (numpy): copies"""
    q, rowptr = qptr(S), arr(S, "rowptr")
    return [np.array(Z[q[k]:q[k + 1]]).reshape((int(rowptr[k + 1] - rowptr[k]),) * 2, order="F") for k in range(len(q) - 1)]


def sum_blocks(S, blocks, rows=None):
    """sum_k E_k Z_k E_k^T as a dense n x n matrix (rows: per clique the row indices, default the clique's rows)"""
    n = sizes(S)[1]
    M = np.zeros((n, n), dtype=np.asarray(blocks[0]).dtype)
    for k, Z in enumerate(blocks):
        r = clique_rows(S, k) if rows is None else np.asarray(rows[k])
        M[np.ix_(r, r)] += Z
    return M


def cone_defects(Z, B, nn):
    """(-lambda_min(Z) / |B|_F, sigma_{nn + 1}(Z) / |B|_F; 0 where B is 0 and so is the defect): by Weyl both are at most the
    number of error bounds B that Z carries when the exact block is positive semidefinite of rank <= nn"""
    nb = float(np.linalg.norm(B))
    lam = float(np.linalg.eigvalsh(Z)[0])
    sv = np.linalg.svd(Z, compute_uv=False)
    tail = float(sv[nn]) if nn < len(sv) else 0.0
    ratio = lambda x: 0.0 if x <= 0.0 else (x / nb if nb > 0 else np.inf)
    return ratio(-lam), ratio(tail)
