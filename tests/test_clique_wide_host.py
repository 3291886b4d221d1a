"""The chip-wide block Jacobi for wide clique blocks (csp_tune(CSP_TUNE_CEIG_WIDE), csrc/front_ceigw.hip) restated in numpy
on top of jacobi_vec_restatement and measured against LAPACK (no GPU needed; tests/test_gpu_clique_wide.py imports this
file).

Units as in tests/test_clique_eigh_host.py (u = nf eps for orthogonality, u |A|_F for residuals and projections; UNITS are
asserted) and 1.0 nf eps max|w| for the eigenvalues.  The measured ratios and the block sweeps are printed per case."""
import numpy as np
import pytest

from helpers import GPU_PATTERNS
from smcp_amd.symbolic import Symbolic
from test_clique_eig_host import EPS, MAX_SWEEPS, clique_blocks, inputs
from test_clique_eigh_host import BOUNDS, UNITS, jacobi_vec_restatement, measure, project_restatement

EIG_UNIT = 1.0                       # |w - w_LAPACK| in nf eps max|w|
ORDERS = [65, 96, 97, 128, 129, 161]
KINDS = ["definite", "rank3", "indefinite", "graded"]
_RESULT = {}


def block_pairs(nb, r):
    """the block pairs (I, J), I < J, of step r of the tournament of ceig_pair on nb blocks; J = None: block I meets the
    phantom player of an odd nb and is a pivot of its own"""
    m = nb + (nb & 1)
    out = []
    for t in range(m // 2):
        x, y = (m - 1, r) if t == 0 else ((r + t) % (m - 1), (r - t + m - 1) % (m - 1))
        p, q = min(x, y), max(x, y)
        out.append((p, q if q < nb else None))
    return out


def block_jacobi_restatement(M, b=32):
    """front_ceigw.hip in numpy: (w ascending, Q with column j for w[j], block sweeps, converged).

    Blocks of b columns (the last may be narrower).  At the start of a block sweep: max |off-diagonal| <= eps |M|_F ends the
    iteration, MAX_SWEEPS block sweeps fail it; a non-finite |M|_F fails at once.  A step (k_ceigw_pivot, k_ceigw_apply): every
    pivot [F_II F_IJ; F_JI F_JJ] goes through jacobi_vec_restatement (cyclic Jacobi, then its rank sort: U_P has its columns
    in ascending order of the pivot's eigenvalues); every tile (P, Q), P > Q, of F in the pair coordinates of the step becomes
    U_P^T T U_Q and is mirrored to (Q, P); a diagonal tile is SET to diag(eigenvalues of the pivot) with exact zeros; a tile
    whose two pivots took no sweep and moved no column is left alone; V[:, Q] <- V[:, Q] U_Q."""
    F = np.array(M, dtype=np.float64)
    nf = F.shape[0]
    nb = (nf + b - 1) // b
    blk = [np.arange(i * b, min(nf, (i + 1) * b)) for i in range(nb)]
    V = np.eye(nf)
    fro = np.sqrt((F * F).sum())
    if not fro < np.inf:
        return np.full(nf, np.nan), np.full((nf, nf), np.nan), 0, False
    stop = EPS * fro
    sweeps, ok = 0, True
    while True:
        off = np.abs(F - np.diag(np.diag(F))).max()
        if off <= stop:
            break
        if sweeps == MAX_SWEEPS:
            ok = False
            break
        sweeps += 1
        for r in range(nb + (nb & 1) - 1):
            piv = []
            for I, J in block_pairs(nb, r):
                idx = blk[I] if J is None else np.concatenate([blk[I], blk[J]])
                w, U, s, good = jacobi_vec_restatement(F[np.ix_(idx, idx)])
                assert good, "a pivot of order %d did not converge" % len(idx)
                same = s == 0 and np.array_equal(w, np.diag(F)[idx])
                piv.append((idx, w, U, same))
            for P, (ip, wp, Up, sp) in enumerate(piv):
                for Q, (iq, wq, Uq, sq) in enumerate(piv[:P]):
                    if sp and sq:
                        continue
                    T = Up.T @ F[np.ix_(ip, iq)] @ Uq
                    F[np.ix_(ip, iq)] = T
                    F[np.ix_(iq, ip)] = T.T
                F[np.ix_(ip, ip)] = np.diag(wp)
                if not sp:
                    V[:, ip] = V[:, ip] @ Up
    if not ok:
        return np.full(nf, np.nan), np.full((nf, nf), np.nan), sweeps, False
    order = np.argsort(np.diag(F), kind="stable")
    return np.diag(F)[order], V[:, order], sweeps, True


def wide_block(nf, kind):
    """one block of the four kinds of this file"""
    rng = np.random.default_rng(2000 + nf)
    S = rng.standard_normal((nf, nf))
    if kind == "definite":
        return S @ S.T + np.eye(nf)
    if kind == "rank3":
        G = rng.standard_normal((nf, 3))
        return G @ G.T
    if kind == "indefinite":
        return S + S.T
    Q = np.linalg.qr(S)[0]
    A = (Q * np.logspace(0, -12, nf)) @ Q.T
    return 0.5 * (A + A.T)


def restated(nf, kind):
    """(A, w, Q, block sweeps) of a single block: made once, shared with the GPU tests"""
    if (nf, kind) not in _RESULT:
        A = wide_block(nf, kind)
        w, Q, sweeps, ok = block_jacobi_restatement(A)
        assert ok, (nf, kind, sweeps)
        _RESULT[(nf, kind)] = (A, w, Q, sweeps)
    return _RESULT[(nf, kind)]


def ratios(A, w, Q):
    """(eigenvalues, orthogonality, residual, projection) of one block in their units"""
    nf = A.shape[0]
    ref = np.linalg.eigvalsh(A)
    scale = nf * EPS * np.abs(ref).max()
    eig = np.abs(w - ref).max() / scale if scale else np.abs(w - ref).max()
    return (eig,) + measure(A, w, Q, [(lo, hi, project_restatement(A, w, Q, lo, hi)[0]) for lo, hi in BOUNDS])


def held(got, what):
    for g, unit in zip(got, (EIG_UNIT,) + UNITS):
        assert g <= unit, (what, got)


@pytest.mark.parametrize("nf", ORDERS)
def test_restatement_meets_lapack_on_single_blocks(nf, capsys):
    for kind in KINDS:
        A, w, Q, sweeps = restated(nf, kind)
        assert (np.diff(w) >= 0).all() and sweeps <= MAX_SWEEPS
        got = ratios(A, w, Q)
        with capsys.disabled():
            print("\norder %d %s: eigenvalues %.2f, orthogonality %.2f u, residual %.2f u|A|, projection %.2f u|A|, %d block sweeps"
                  % ((nf, kind) + got + (sweeps,)))
        held(got, (nf, kind))


def test_restatement_meets_lapack_on_the_wide_cliques_of_fam_top(capsys):
    symb = Symbolic(GPU_PATTERNS["fam_top"]())
    orders = set()
    for kind, blkA, blkB in inputs(symb, 11):
        if blkB is not None:
            continue
        for A in clique_blocks(symb, blkA):
            if A.shape[0] < 65:
                continue
            orders.add(A.shape[0])
            w, Q, sweeps, ok = block_jacobi_restatement(A)
            assert ok
            got = ratios(A, w, Q)
            with capsys.disabled():
                print("\nfam_top %s order %d: eigenvalues %.2f, orthogonality %.2f u, residual %.2f u|A|, projection %.2f u|A|, "
                      "%d block sweeps" % ((kind, A.shape[0]) + got + (sweeps,)))
            held(got, ("fam_top", kind, A.shape[0]))
    assert {110, 130} <= orders


@pytest.mark.parametrize("nb", [3, 4, 5, 6])
def test_block_tournament_meets_every_block_pair_once(nb):
    met, alone = [], []
    for r in range(nb + (nb & 1) - 1):
        pairs = block_pairs(nb, r)
        used = [I for I, J in pairs] + [J for I, J in pairs if J is not None]
        assert sorted(used) == list(range(nb))                           # every block in exactly one pivot of a step
        met += [(I, J) for I, J in pairs if J is not None]
        alone += [I for I, J in pairs if J is None]
    assert sorted(met) == [(i, j) for i in range(nb) for j in range(i + 1, nb)]
    assert sorted(alone) == (list(range(nb)) if nb & 1 else [])


def test_diagonal_block_takes_no_sweep_and_non_finite_is_reported():
    d = np.random.default_rng(5).standard_normal(97)
    w, Q, sweeps, ok = block_jacobi_restatement(np.diag(d))
    assert ok and sweeps == 0 and np.array_equal(w, np.sort(d)) and np.array_equal(np.abs(Q).sum(axis=0), np.ones(97))
    A = wide_block(97, "indefinite")
    A[70, 3] = A[3, 70] = np.nan
    w, Q, sweeps, ok = block_jacobi_restatement(A)
    assert not ok and sweeps == 0 and np.isnan(w).all() and np.isnan(Q).all()
    A[70, 3] = A[3, 70] = np.inf
    assert not block_jacobi_restatement(A)[3]
