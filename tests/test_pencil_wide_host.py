"""The reduction of the pencil (A_gg, B_gg) to standard form on the chip-wide route (csp_tune(CSP_TUNE_CEIG_WIDE) with B given;
csrc/front_ceigw.hip) restated in numpy, tile by tile in the order of the kernels, and measured against
pencil_matrix of tests/test_clique_eig_host.py and against LAPACK (no GPU needed; tests/test_gpu_pencil_wide.py imports this
file).  The block Jacobi behind the reduction is the one of tests/test_clique_wide_host.py and is not run again here: the
reduced matrix goes to np.linalg.eigvalsh.

Unit: the parity bound of tests/test_gpu_clique_eig.py, 16 nf eps max|w_ref|.  A numpy simulation of this blocking stayed within
0.23 of it on orders 65 - 548 with cond(B) 11 - 80, so the host asserts 1 unit and prints the ratio."""
import numpy as np
import pytest
import scipy.linalg

from helpers import GPU_PATTERNS
from smcp_amd.symbolic import Symbolic
from test_clique_eig_host import EPS, clique_blocks, indefinite_on_V, pencil_B_on_V, pencil_matrix

CW_T = 64                            # csrc/front_ceigw.hip
ORDERS = [65, 96, 97, 128, 129, 161]
WIDE = 65
HOST_UNITS = 1.0                     # of 16 nf eps max|w_ref|


def bound(ref):
    """the parity bound of one clique (tests/test_gpu_clique_eig.py): 16 nf eps max|w_ref|"""
    return 16 * len(ref) * EPS * np.abs(ref).max()


def tiles(nf):
    """the row ranges of the 64-row tiles of a block of order nf; the last may be a single row"""
    return [slice(o, min(nf, o + CW_T)) for o in range(0, nf, CW_T)]


def potrf_tile(T):
    """wg::potrf on one tile: (lower factor, 0) or (None, j + 1) for the first pivot j that is not > 0 (a NaN is not)"""
    T = np.array(T)
    n = T.shape[0]
    for j in range(n):
        d = T[j, j]
        if not d > 0.0:
            return None, j + 1
        T[j:, j] = np.concatenate(([np.sqrt(d)], T[j + 1:, j] * (1.0 / np.sqrt(d))))
        T[j + 1:, j + 1:] -= np.outer(T[j + 1:, j], T[j + 1:, j])
    return np.tril(T), 0


def reduction_restatement(A, B):
    """(M, launches, None) with M = R^-1 A R^-T, B = R R^T, resymmetrised, or (None, launches, (tile, pivot)) when the
    diagonal tile `tile` met the pivot `pivot` (counted inside the tile) that is not > 0.  The order of the kernels: per block
    column the diagonal tile (k_ceigw_potrf), the panel below it (k_ceigw_panel), the trailing tiles on and below the diagonal
    (k_ceigw_trail); then the slabs of 64 columns of F <- R^-1 F and of 64 rows of F <- F R^-T, each walking its tiles in order
    and subtracting the products with the tiles it has solved, ascending, before the solve with the diagonal tile
    (k_ceigw_solve); then (F + F^T) / 2 (k_ceigw_symm).  launches: what the host enqueues, 3 nt + 1 whatever the data."""
    F = np.array(A, dtype=np.float64)
    G = np.array(B, dtype=np.float64)
    tl = tiles(F.shape[0])
    nt = len(tl)
    launches = 3 * nt + 1
    for j in range(nt):
        R, fail = potrf_tile(G[tl[j], tl[j]])
        if fail:
            return None, launches, (j, fail - 1)
        G[tl[j], tl[j]] = R
        for i in range(j + 1, nt):
            G[tl[i], tl[j]] = scipy.linalg.solve_triangular(R, G[tl[i], tl[j]].T, lower=True, check_finite=False).T
        for i in range(j + 1, nt):
            for l in range(j + 1, i + 1):
                G[tl[i], tl[l]] -= G[tl[i], tl[j]] @ G[tl[l], tl[j]].T
    for s in range(nt):                                  # F <- R^-1 F by slabs of columns
        for t in range(nt):
            T = F[tl[t], tl[s]].copy()
            for k in range(t):
                T -= G[tl[t], tl[k]] @ F[tl[k], tl[s]]
            F[tl[t], tl[s]] = scipy.linalg.solve_triangular(G[tl[t], tl[t]], T, lower=True, check_finite=False)
    for s in range(nt):                                  # F <- F R^-T by slabs of rows
        for t in range(nt):
            T = F[tl[s], tl[t]].copy()
            for k in range(t):
                T -= F[tl[s], tl[k]] @ G[tl[t], tl[k]].T
            F[tl[s], tl[t]] = scipy.linalg.solve_triangular(G[tl[t], tl[t]], T.T, lower=True, check_finite=False).T
    return 0.5 * (F + F.T), launches, None


def single_block(nf):
    """A = S + S^T, B = I + G G^T / 8 (the B of pencil_B_on_V) of order nf"""
    rng = np.random.default_rng(nf)
    S = rng.standard_normal((nf, nf))
    G = rng.standard_normal((nf, 4))
    return S + S.T, np.eye(nf) + G @ G.T / 8.0


def check_block(A, B, seen):
    nf = A.shape[0]
    M, launches, fail = reduction_restatement(A, B)
    assert fail is None and launches == 3 * len(tiles(nf)) + 1
    assert np.array_equal(M, M.T)
    ref = scipy.linalg.eigh(A, B, eigvals_only=True)
    w = np.linalg.eigvalsh(M)
    Mp = pencil_matrix(A, B)
    unit = bound(ref)
    r_eig = np.abs(w - ref).max() / unit
    r_mat = np.abs(np.linalg.eigvalsh(Mp) - w).max() / unit     # against the unblocked reduction, as eigenvalues
    r_ent = np.abs(M - Mp).max() / (16 * nf * EPS * np.abs(Mp).max() * np.linalg.cond(B))   # entries: backward error times cond(B)
    seen.append((nf, r_eig, r_mat, r_ent))
    assert r_eig <= HOST_UNITS, "order %d: eigenvalues %.3f of 16 nf eps max|w|, bound %.1f" % (nf, r_eig, HOST_UNITS)
    assert r_mat <= HOST_UNITS, "order %d: against pencil_matrix %.3f of 16 nf eps max|w|, bound %.1f" % (nf, r_mat, HOST_UNITS)
    assert r_ent <= HOST_UNITS, "order %d: entries against pencil_matrix %.3f of 16 nf eps max|M| cond(B), bound %.1f" % (nf, r_ent, HOST_UNITS)


@pytest.mark.parametrize("nf", ORDERS)
def test_reduction_meets_lapack_on_single_blocks(nf, capsys):
    A, B = single_block(nf)
    seen = []
    check_block(A, B, seen)
    with capsys.disabled():
        print("\norder %d (%d tiles, last of %d rows): eigenvalues %.3f, against pencil_matrix %.3f (entries %.3f) of the bound"
              % (nf, len(tiles(nf)), nf - CW_T * (len(tiles(nf)) - 1), seen[0][1], seen[0][2], seen[0][3]))


def test_reduction_meets_lapack_on_the_wide_cliques_of_fam_top(capsys):
    symb = Symbolic(GPU_PATTERNS["fam_top"]())
    As = clique_blocks(symb, indefinite_on_V(symb, 12))
    Bs = clique_blocks(symb, pencil_B_on_V(symb, 13))
    seen = []
    for A, B in zip(As, Bs):
        if A.shape[0] >= WIDE:
            check_block(A, B, seen)
    assert sorted(s[0] for s in seen) == [110, 130, 130]
    with capsys.disabled():
        print("\nfam_top: " + ", ".join("order %d eigenvalues %.3f, pencil_matrix %.3f" % s[:3] for s in seen) + " of the bound")


def test_tiles_cover_the_block_and_the_last_may_be_one_row():
    for nf in ORDERS + [64, 548]:
        tl = tiles(nf)
        assert len(tl) == -(-nf // CW_T) and tl[0].start == 0 and tl[-1].stop == nf
        assert all(a.stop == b.start for a, b in zip(tl, tl[1:])) and all(t.stop - t.start == CW_T for t in tl[:-1])
    assert tiles(65)[-1] == slice(64, 65) and tiles(129)[-1] == slice(128, 129)


@pytest.mark.parametrize("nf,row", [(129, 70), (97, 64), (129, 128), (161, 5)])
def test_negative_pivot_is_reported_from_its_tile(nf, row):
    """B positive definite except for a negative diagonal entry: met by the diagonal tile that holds the row, after the
    trailing updates of the block columns before it, at that row or (rounding aside, never) later in the tile; the launches
    are those of a positive definite B"""
    A, B = single_block(nf)
    good = reduction_restatement(A, B)[1]
    B[row, row] = -1.0
    M, launches, fail = reduction_restatement(A, B)
    assert M is None and launches == good
    assert fail == (row // CW_T, row % CW_T), "order %d row %d: reported from tile %d pivot %d" % ((nf, row) + fail)
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(B)


def test_non_finite_entry_of_b_ends_in_a_pivot_that_is_not_positive():
    """a NaN below the diagonal of B reaches the diagonal of its row through the panel and the trailing update (or inside the
    diagonal tile) and fails that pivot: the route reports B as not positive definite, as wg::potrf on the whole block does"""
    for i, j in [(100, 3), (70, 66), (128, 64)]:
        A, B = single_block(129)
        B[i, j] = B[j, i] = np.nan
        M, _, fail = reduction_restatement(A, B)
        assert M is None and fail == (i // CW_T, i % CW_T), (i, j, fail)


def test_scipy_max_step_refuses_a_wide_below_three_blocks():
    """smcp_amd.max_step(X, D, wide=...) takes what tune(symb, TUNE_CEIG_WIDE, value) takes: 0 or at least 65 (refused before
    anything is built, so no device is needed)"""
    import scipy.sparse as sp
    import smcp_amd
    X = sp.identity(4, format="csc")
    for wide in (1, 64, -1):
        with pytest.raises(ValueError, match="wide"):
            smcp_amd.max_step(X, X, wide=wide)
