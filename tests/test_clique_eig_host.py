"""Spectra of the clique blocks (smcp_amd.chordal.clique_eigvalsh / cone_margin / max_step, csrc/front_ceig.hip): the
references the GPU tests compare with (LAPACK on dense clique blocks), the kernel's cyclic Jacobi restated in numpy, and
the identities the margin and the step rest on, checked on the references (no GPU needed;
tests/test_gpu_clique_eig.py imports this file)."""
import math

import numpy as np
import pytest
import scipy.linalg

from helpers import PATTERNS
from smcp_amd import chordal  # noqa: F401
from smcp_amd.chordal import clique_eigvalsh, cone_margin, max_step  # noqa: F401  (what this file is the reference of)
from smcp_amd.symbolic import Symbolic
from test_mrcompletion_host import blkval_of, clique_rows, dense_of, low_rank_on_V, pd_on_V

EPS = np.finfo(np.float64).eps
MAX_SWEEPS = 30                     # CEIG_MAX_SWEEPS, csrc/front_ceig.hip


# ---- references ----------------------------------------------------------------------------------------------------
def clique_blocks(symb, blk):
    """the dense symmetric block of every clique"""
    X = dense_of(symb, blk)
    return [X[np.ix_(clique_rows(symb, k), clique_rows(symb, k))] for k in range(symb.Nsn)]


def clique_spectra_ref(symb, blkA, blkB=None):
    """per clique the ascending eigenvalues of A_gg (LAPACK), or of the pencil (A_gg, B_gg)"""
    As = clique_blocks(symb, blkA)
    if blkB is None:
        return [np.linalg.eigvalsh(A) for A in As]
    return [scipy.linalg.eigh(A, B, eigvals_only=True) for A, B in zip(As, clique_blocks(symb, blkB))]


def margin_ref(symb, blk):
    """(m, clique) of cone_margin from the reference spectra"""
    lo = np.array([w[0] for w in clique_spectra_ref(symb, blk)])
    return float(lo.min()), int(np.argmin(lo))


def max_step_ref(symb, blkX, blkD):
    """(alpha, clique) of max_step from the reference spectra of the pencils (D_gg, X_gg)"""
    lo = np.array([w[0] for w in clique_spectra_ref(symb, blkD, blkX)])
    mu = float(lo.min())
    return (-1.0 / mu if mu < 0 else math.inf), int(np.argmin(lo))


def tournament(nf, r):
    """the pairs (p < q) of step r of the round-robin order of ceig_pair: m = nf rounded up to even players, player m - 1
    stays in place; pairs with the dummy player of an odd order (a bye) are left out"""
    m = nf + (nf & 1)
    out = []
    for t in range(m // 2):
        x, y = (m - 1, r) if t == 0 else ((r + t) % (m - 1), (r - t + m - 1) % (m - 1))
        p, q = min(x, y), max(x, y)
        if q < nf:
            out.append((p, q))
    return out


def jacobi_restatement(M):
    """ceig_jacobi in numpy: (ascending eigenvalues, sweeps taken, converged).  The same pair order, Rutishauser's
    rotation (t, c, s, tau; the 2 x 2 block set exactly), the skip rule |a_pq| <= eps |M|_F / nf, the stopping rule
    max |off-diagonal| <= eps |M|_F at the start of a sweep, and the cap of 30 sweeps."""
    F = np.array(M, dtype=np.float64)
    nf = F.shape[0]
    m = nf + (nf & 1)
    fro = np.sqrt((F * F).sum())
    if not fro < np.inf:
        return np.sort(np.diag(F)), 0, False
    stop = EPS * fro
    skip = stop / nf
    sweeps, ok = 0, True
    while True:
        off = np.abs(F - np.diag(np.diag(F))).max() if nf > 1 else 0.0
        if off <= stop:
            break
        if sweeps == MAX_SWEEPS:
            ok = False
            break
        for r in range(m - 1):
            pq = [(p, q) for p, q in tournament(nf, r) if abs(F[q, p]) > skip]
            if not pq:
                continue
            p = np.array([x[0] for x in pq])
            q = np.array([x[1] for x in pq])
            app, aqq, apq = F[p, p], F[q, q], F[q, p]
            with np.errstate(over="ignore", divide="ignore"):
                theta = 0.5 * (aqq - app) / apq
                tn = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            tn = np.where(theta < 0, -tn, tn)
            c = 1.0 / np.sqrt(tn * tn + 1.0)
            s = tn * c
            tau = s / (1.0 + c)
            live = s != 0.0
            p, q, s, tau, tn, app, aqq, apq = (v[live] for v in (p, q, s, tau, tn, app, aqq, apq))
            g, h = F[p, :].copy(), F[q, :].copy()                     # rows
            F[p, :] = g - s[:, None] * (h + g * tau[:, None])
            F[q, :] = h + s[:, None] * (g - h * tau[:, None])
            g, h = F[:, p].copy(), F[:, q].copy()                     # columns
            F[:, p] = g - s[None, :] * (h + g * tau[None, :])
            F[:, q] = h + s[None, :] * (g - h * tau[None, :])
            F[p, p] = app - tn * apq
            F[q, q] = aqq + tn * apq
            F[p, q] = 0.0
            F[q, p] = 0.0
        sweeps += 1
    return np.sort(np.diag(F)), sweeps, ok


def pencil_matrix(A, B):
    """M = R^-1 A R^-T with B = R R^T, resymmetrised: what the kernel hands to its Jacobi in the pencil form"""
    R = np.linalg.cholesky(B)
    Y = scipy.linalg.solve_triangular(R, A, lower=True)
    Mx = scipy.linalg.solve_triangular(R, Y.T, lower=True).T
    return 0.5 * (Mx + Mx.T)


# ---- inputs --------------------------------------------------------------------------------------------------------
def indefinite_on_V(symb, seed):
    """a random symmetric blkval: indefinite clique blocks"""
    return np.random.default_rng(seed).standard_normal(symb.blklen)


def pencil_B_on_V(symb, seed):
    """blkval of I + G G^T / 8, G n x 4 standard normal: clique blocks of condition number <= 40 up to order 208"""
    G = np.random.default_rng(seed).standard_normal((symb.n, 4))
    return blkval_of(symb, np.eye(symb.n) + G @ G.T / 8.0)


def shifted(symb, blk, t):
    """blkval of X - t I"""
    out = blk.copy()
    nn, na = symb.clique_sizes()
    for k in range(symb.Nsn):
        out[symb.blkptr[k] + np.arange(nn[k]) * (nn[k] + na[k] + 1)] -= t
    return out


def all_blocks_pd(symb, blk):
    return all(np.linalg.eigvalsh(F)[0] > 0 for F in clique_blocks(symb, blk))


def inputs(symb, seed):
    """(kind, blkA, blkB) of the four kinds of input"""
    return [("definite", pd_on_V(symb, seed), None), ("rank3", low_rank_on_V(symb, 3, seed), None),
            ("indefinite", indefinite_on_V(symb, seed), None),
            ("pencil", indefinite_on_V(symb, seed + 1), pencil_B_on_V(symb, seed + 2))]


SYMBS = {}


def host_symb(name):
    if name not in SYMBS:
        SYMBS[name] = Symbolic(PATTERNS[name]())
    return SYMBS[name]


def check_restatement(A, B, seen):
    """the restatement against LAPACK on one block: within 2 nf eps max|lambda| in at most 15 sweeps"""
    nf = A.shape[0]
    ref = np.linalg.eigvalsh(A) if B is None else scipy.linalg.eigh(A, B, eigvals_only=True)
    w, sweeps, ok = jacobi_restatement(A if B is None else pencil_matrix(A, B))
    scale = np.abs(ref).max()
    err = np.abs(w - ref).max()
    seen.append((nf, err / (nf * EPS * scale) if scale else 0.0, sweeps))
    assert ok and sweeps <= 15, (nf, sweeps)
    assert err <= 2 * nf * EPS * scale, (nf, err / (nf * EPS * scale))


# ---- tests ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_restatement_meets_lapack_on_patterns(name, capsys):
    symb = host_symb(name)
    seen = []
    for kind, blkA, blkB in inputs(symb, 11):
        As = clique_blocks(symb, blkA)
        Bs = [None] * len(As) if blkB is None else clique_blocks(symb, blkB)
        for A, B in zip(As, Bs):
            check_restatement(A, B, seen)
    with capsys.disabled():
        print("\n%s: worst error %.2f nf eps max|lambda|, most sweeps %d" % (name, max(s[1] for s in seen), max(s[2] for s in seen)))


@pytest.mark.parametrize("nf", [1, 2, 3, 17, 33, 64, 129])
def test_restatement_meets_lapack_on_single_blocks(nf, capsys):
    rng = np.random.default_rng(nf)
    S = rng.standard_normal((nf, nf))
    G3 = rng.standard_normal((nf, 3))
    G4 = rng.standard_normal((nf, 4))
    seen = []
    check_restatement(S + S.T, None, seen)                                  # indefinite
    check_restatement(G3 @ G3.T, None, seen)                                # rank 3 (or full for nf <= 3)
    check_restatement(S @ S.T + np.eye(nf), None, seen)                     # definite
    check_restatement(S + S.T, np.eye(nf) + G4 @ G4.T / 8.0, seen)          # pencil
    with capsys.disabled():
        print("\norder %d: worst error %.2f nf eps max|lambda|, most sweeps %d" % (nf, max(s[1] for s in seen), max(s[2] for s in seen)))


def test_tournament_meets_every_pair_once():
    for nf in (1, 2, 3, 4, 7, 8, 20, 33):
        m = nf + (nf & 1)
        steps = [tournament(nf, r) for r in range(m - 1)]
        assert len(steps) == (nf - 1 if nf % 2 == 0 else nf) or nf == 1
        for st in steps:
            flat = [i for pq in st for i in pq]
            assert len(flat) == len(set(flat)) and len(st) == nf // 2          # disjoint pairs, one bye for odd order
        allp = sorted(pq for st in steps for pq in st)
        assert allp == [(p, q) for p in range(nf) for q in range(p + 1, nf)]


def test_restatement_reports_non_finite_input_and_order_one():
    w, sweeps, ok = jacobi_restatement(np.array([[3.5]]))
    assert ok and sweeps == 0 and w[0] == 3.5
    A = np.eye(4)
    A[2, 1] = A[1, 2] = np.nan
    assert not jacobi_restatement(A)[2]
    A[2, 1] = A[1, 2] = np.inf
    assert not jacobi_restatement(A)[2]


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_margin_identity_on_reference(name):
    """every clique block of X - (1 - 1e-6) m I is positive definite, some block of X - (1 + 1e-6) m I is not"""
    symb = host_symb(name)
    blk = pd_on_V(symb, 5)
    m, k = margin_ref(symb, blk)
    assert m > 0 and 0 <= k < symb.Nsn
    assert all_blocks_pd(symb, shifted(symb, blk, (1 - 1e-6) * m))
    assert not all_blocks_pd(symb, shifted(symb, blk, (1 + 1e-6) * m))
    assert np.linalg.eigvalsh(clique_blocks(symb, shifted(symb, blk, (1 + 1e-6) * m))[k])[0] < 0


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_max_step_identity_on_reference(name):
    """every clique block of X + (1 - 1e-6) alpha D is positive definite, some block of X + (1 + 1e-6) alpha D is not"""
    symb = host_symb(name)
    X = pd_on_V(symb, 5)
    D = indefinite_on_V(symb, 6)
    alpha, k = max_step_ref(symb, X, D)
    assert 0 < alpha < math.inf
    assert all_blocks_pd(symb, X + (1 - 1e-6) * alpha * D)
    assert not all_blocks_pd(symb, X + (1 + 1e-6) * alpha * D)
    assert np.linalg.eigvalsh(clique_blocks(symb, X + (1 + 1e-6) * alpha * D)[k])[0] < 0
    assert max_step_ref(symb, X, X)[0] == math.inf
