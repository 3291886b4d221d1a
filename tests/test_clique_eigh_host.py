"""Eigenvectors and spectral projections of the clique blocks, and the packed clique blocks they live in
(smcp_amd.chordal.clique_eigh / clique_project / clique_gather / clique_scatter / clique_ptr, csrc/front_ceig.hip): the
kernel's Jacobi with the rotations accumulated, its rank sort and its "A + correction" projection restated in numpy and
measured against LAPACK; the scatter restated level by level and checked against its dense definition; the declarations
of the five entry points (no GPU needed; tests/test_gpu_clique_eigh.py imports this file).

Units: u = nf eps for orthogonality, u |A|_F for residuals and projections.  Asserted here: 1, 1 and 3 units.  Measured:
0.75, 0.42 and 2.56 (the printed lines): the projection of a 4 x 4 block of `band` on [-0.5, 0.5]
takes away 6.5 q q^T with a q that is itself good to 0.6 u, which is 2.56 u |A|_F for so small an nf; single blocks alone
had shown 1.35.  The GPU tests allow 16 times the asserted values."""
import os
import re

import numpy as np
import pytest

from helpers import EXTRA, GPU_PATTERNS, PATTERNS
from smcp_amd import _lib, chordal
from smcp_amd.symbolic import Symbolic
from test_clique_eig_host import EPS, MAX_SWEEPS, clique_blocks, inputs, tournament
from test_mrcompletion_host import blkval_of, clique_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = (1.0, 1.0, 3.0)              # orthogonality, residual, projection: what the restatement is held to
GPU_FACTOR = 16.0                    # the device is held to GPU_FACTOR times these
BOUNDS = ((0.0, np.inf), (-0.5, 0.5))

HOST_PATS = dict(PATTERNS)
HOST_PATS["diag"] = GPU_PATTERNS["diag"]
HOST_PATS["one_clique"] = EXTRA["one_clique"]
_SYMB = {}


def host_symb(name):
    if name not in _SYMB:
        _SYMB[name] = Symbolic(HOST_PATS[name]())
    return _SYMB[name]


# ---- the kernel restated ---------------------------------------------------------------------------------------------
def jacobi_vec_restatement(M):
    """ceig_jacobi<true> and the rank sort of k_ceig_vec in numpy: (w ascending, Q with column j for w[j], sweeps, converged).
    The pair order, rotations, skip and stop rules are those of test_clique_eig_host.jacobi_restatement; V starts as I and
    every step rotates its columns p, q by the step's (s, tau); the stable sort of the diagonal places column i of V."""
    F = np.array(M, dtype=np.float64)
    nf = F.shape[0]
    V = np.eye(nf)
    m = nf + (nf & 1)
    fro = np.sqrt((F * F).sum())
    if not fro < np.inf:
        return np.full(nf, np.nan), np.full((nf, nf), np.nan), 0, False
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
            g, h = V[:, p].copy(), V[:, q].copy()                     # the V pass
            V[:, p] = g - s[None, :] * (h + g * tau[None, :])
            V[:, q] = h + s[None, :] * (g - h * tau[None, :])
        sweeps += 1
    if not ok:
        return np.full(nf, np.nan), np.full((nf, nf), np.nan), sweeps, False
    order = np.argsort(np.diag(F), kind="stable")                     # rank by value, ties by index
    return np.diag(F)[order], V[:, order], sweeps, True


def project_restatement(A, w, Q, lo, hi):
    """the projection of k_ceig_vec: A + the corrections of the eigenvalues outside [lo, hi], ascending, entry by entry;
    (Z, eigenvalues changed, sum of the squared changes)"""
    Z = np.array(A, dtype=np.float64)
    cnt, sq = 0, 0.0
    for j in range(len(w)):
        f = lo if w[j] < lo else hi if w[j] > hi else w[j]
        if f != w[j]:
            Z += (f - w[j]) * (Q[:, j][:, None] * Q[:, j][None, :])
            cnt += 1
            sq += (f - w[j]) ** 2
    return Z, cnt, sq


def project_ref(A, lo, hi):
    """the same from LAPACK: (Z, eigenvalues, clipped eigenvalues)"""
    w, Q = np.linalg.eigh(A)
    f = np.clip(w, lo, hi)
    Z = (Q * f) @ Q.T
    return 0.5 * (Z + Z.T), w, f


def measure(A, w, Q, projections):
    """the three quantities of one block in their units; projections: [(lo, hi, Z)]"""
    nf = A.shape[0]
    u = nf * EPS
    fro = np.sqrt((A * A).sum())
    orth = np.abs(Q.T @ Q - np.eye(nf)).max() / u
    res = np.abs(A @ Q - Q * w).max() / (u * fro) if fro else 0.0
    prj = 0.0
    for lo, hi, Z in projections:
        d = np.abs(Z - project_ref(A, lo, hi)[0]).max()
        prj = max(prj, d / (u * fro) if fro else d)
    return orth, res, prj


def check_block(A, seen):
    w, Q, sweeps, ok = jacobi_vec_restatement(A)
    assert ok and sweeps <= MAX_SWEEPS, (A.shape[0], sweeps)
    assert (np.diff(w) >= 0).all()
    got = measure(A, w, Q, [(lo, hi, project_restatement(A, w, Q, lo, hi)[0]) for lo, hi in BOUNDS])
    seen.append(got + (sweeps,))
    for g, unit in zip(got, UNITS):
        assert g <= unit, (A.shape[0], got)


def report(capsys, what, seen):
    with capsys.disabled():
        print("\n%s: orthogonality %.2f u, residual %.2f u|A|, projection %.2f u|A|, most sweeps %d"
              % ((what,) + tuple(max(s[i] for s in seen) for i in range(4))))


def single_blocks(nf):
    """(kind, block) of the five kinds of one order"""
    rng = np.random.default_rng(1000 + nf)
    S = rng.standard_normal((nf, nf))
    G3 = rng.standard_normal((nf, 3))
    Qo = np.linalg.qr(rng.standard_normal((nf, nf)))[0]
    d = np.where(np.arange(nf) % 2 == 0, 1.0, -1.0) + 1e-13 * rng.standard_normal(nf)
    C = (Qo * d) @ Qo.T
    G = rng.standard_normal((nf, nf)) / np.sqrt(nf)
    return [("definite", S @ S.T + np.eye(nf)), ("rank3", G3 @ G3.T), ("indefinite", S + S.T),
            ("clustered", 0.5 * (C + C.T)), ("near_psd", G @ G.T - 0.05 * np.eye(nf))]


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_restatement_meets_lapack_on_patterns(name, capsys):
    symb = host_symb(name)
    seen = []
    for kind, blkA, blkB in inputs(symb, 11):
        if blkB is None:                                               # definite, rank 3, indefinite
            for A in clique_blocks(symb, blkA):
                check_block(A, seen)
    report(capsys, name, seen)


@pytest.mark.parametrize("nf", [1, 2, 3, 4, 7, 17, 33, 64, 89, 90, 129])
def test_restatement_meets_lapack_on_single_blocks(nf, capsys):
    seen = []
    for kind, A in single_blocks(nf):
        check_block(A, seen)
    report(capsys, "order %d" % nf, seen)


def test_restatement_projection_contract():
    """a block inside [lo, hi] comes back as its own bits with nothing counted; counts and distances match LAPACK's; a
    non-finite entry is reported"""
    A = single_blocks(17)[0][1]
    w, Q, _, ok = jacobi_vec_restatement(A)
    Z, cnt, sq = project_restatement(A, w, Q, 0.0, np.inf)
    assert ok and cnt == 0 and sq == 0.0 and np.array_equal(Z, A)
    B = single_blocks(17)[2][1]
    w, Q, _, ok = jacobi_vec_restatement(B)
    for lo, hi in BOUNDS + ((-np.inf, 0.0),):
        Z, cnt, sq = project_restatement(B, w, Q, lo, hi)
        Zr, wr, fr = project_ref(B, lo, hi)
        assert cnt == int((fr != wr).sum())
        assert abs(sq - ((fr - wr) ** 2).sum()) <= 16 * 17 * EPS * (B * B).sum()
        assert np.array_equal(Z, Z.T)
    B[3, 2] = B[2, 3] = np.nan
    assert not jacobi_vec_restatement(B)[3]


# ---- packed clique blocks: dense definitions -------------------------------------------------------------------------
def pack(blocks):
    """blocks (nf x nf each) -> the packed block tensor as a numpy vector"""
    return np.concatenate([np.asarray(B, dtype=np.float64).ravel(order="F") for B in blocks]) if blocks else np.zeros(0)


def unpack(symb, Z):
    q = chordal.clique_ptr(symb)
    nf = np.diff(symb.rowptr)
    return [Z[q[k]:q[k + 1]].reshape(nf[k], nf[k], order="F") for k in range(symb.Nsn)]


def gather_ref(symb, blk):
    """the packed clique blocks of a blkval: the dense definition of clique_gather"""
    return pack(clique_blocks(symb, blk))


def lower_slots(symb):
    """per slot of blkval: True except above the diagonal of a supernode's diagonal block"""
    m = np.ones(symb.blklen, dtype=bool)
    nn, na = symb.clique_sizes()
    for k in range(symb.Nsn):
        nf = nn[k] + na[k]
        i, j = np.meshgrid(np.arange(nf), np.arange(nn[k]), indexing="ij")
        m[symb.blkptr[k]:symb.blkptr[k + 1]] = (i >= j).ravel(order="F")
    return m


def scatter_dense(symb, Z, absolute=False):
    """the dense definition of clique_scatter(..., "sum"): the blkval of sum_k E_k Z_k E_k^T on V, each Z_k read from its
    lower triangle, zeros above the diagonal of the diagonal blocks; absolute: the sum of the absolute values of the terms"""
    X = np.zeros((symb.n, symb.n))
    for k, B in enumerate(unpack(symb, Z)):
        L = np.tril(B)
        if absolute:
            L = np.abs(L)
        rows = clique_rows(symb, k)
        X[np.ix_(rows, rows)] += L + np.tril(L, -1).T
    return np.where(lower_slots(symb), blkval_of(symb, X), 0.0)


def scatter_restatement(symb, Z):
    """csp_clique_scatter in numpy: level by level, leaves first, a clique's panel and update block from the lower triangle
    of Z_k, then its children's update blocks added in the order of its child list (add_children, front_generic.hip)"""
    nn, na = symb.clique_sizes()
    blocks = unpack(symb, Z)
    x = np.zeros(symb.blklen)
    U = [None] * symb.Nsn
    for l in range(symb.nlev):
        for k in symb.levidx[symb.levptr[l]:symb.levptr[l + 1]]:
            nf = nn[k] + na[k]
            F = np.tril(blocks[k]).copy()
            for c in symb.chidx[symb.chptr[k]:symb.chptr[k + 1]]:
                rel = symb.relidx[symb.sepptr[c]:symb.sepptr[c + 1]]
                F[np.ix_(rel, rel)] += U[c]                            # lower + lower: rel ascends
            x[symb.blkptr[k]:symb.blkptr[k + 1]] = F[:, :nn[k]].ravel(order="F")
            U[k] = np.tril(F[nn[k]:, nn[k]:])
            assert F.shape == (nf, nf)
    return x


def multiplicity_count(symb):
    """per slot of blkval the number of cliques that hold the entry (1 on the unused slots), by counting"""
    C = np.zeros((symb.n, symb.n))
    for k in range(symb.Nsn):
        rows = clique_rows(symb, k)
        C[np.ix_(rows, rows)] += 1.0
    return np.where(lower_slots(symb), blkval_of(symb, C), 1.0)


def multiplicity_restatement(symb):
    return np.maximum(scatter_restatement(symb, np.ones(int(chordal.clique_ptr(symb)[-1]))), 1.0)


def integer_on_V(symb, seed):
    """an integer-valued blkval (zeros on the unused slots): sums and means of its copies are exact"""
    b = np.random.default_rng(seed).integers(-50, 51, symb.blklen).astype(np.float64)
    return np.where(lower_slots(symb), b, 0.0)


@pytest.mark.parametrize("name", sorted(HOST_PATS))
def test_clique_ptr_against_clique_sizes(name):
    symb = host_symb(name)
    q = chordal.clique_ptr(symb)
    nn, na = symb.clique_sizes()
    assert q.dtype == np.int64 and q.shape == (symb.Nsn + 1,) and q[0] == 0
    assert (np.diff(q) == (nn + na) ** 2).all()
    assert chordal.clique_ptr(symb) is q                                # made once
    import torch
    Z = torch.arange(int(q[-1]), dtype=torch.float64)
    k = symb.Nsn - 1
    B = chordal.clique_block(symb, Z, k)
    nf = int(nn[k] + na[k])
    assert B.shape == (nf, nf) and B[nf - 1, 0] == q[k] + nf - 1 and B[0, nf - 1] == q[k] + (nf - 1) * nf
    with pytest.raises(ValueError):
        chordal.clique_block(symb, Z[:-1], 0)


@pytest.mark.parametrize("name", sorted(HOST_PATS))
def test_scatter_sum_against_dense_definition(name):
    symb = host_symb(name)
    rng = np.random.default_rng(7)
    Z = rng.standard_normal(int(chordal.clique_ptr(symb)[-1]))
    got, ref = scatter_restatement(symb, Z), scatter_dense(symb, Z)
    assert (np.abs(got - ref) <= symb.nlev * EPS * scatter_dense(symb, Z, absolute=True)).all()
    assert (got[~lower_slots(symb)] == 0).all()
    Zi = np.rint(8 * Z)
    assert np.array_equal(scatter_restatement(symb, Zi), scatter_dense(symb, Zi))     # integers: exact


@pytest.mark.parametrize("name", sorted(HOST_PATS))
def test_multiplicity_and_mean_of_gather(name):
    symb = host_symb(name)
    mult = multiplicity_restatement(symb)
    assert np.array_equal(mult, multiplicity_count(symb)) and mult.min() >= 1
    X = integer_on_V(symb, 3)
    Z = gather_ref(symb, X)
    for B in unpack(symb, Z):
        assert np.array_equal(B, B.T)
    assert np.array_equal(scatter_restatement(symb, Z) / mult, X)       # scatter-mean(gather(X)) == X


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def header_arguments(name):
    src = open(os.path.join(ROOT, "include", "smcp_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    mt = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert mt, name + " is not declared in include/smcp_amd.h"
    return [" ".join(a.split()) for a in mt.group(1).split(",")]


@pytest.mark.parametrize("name,argnames", [
    ("csp_clique_ptr", ["ctx", "qptr_host"]),
    ("csp_clique_gather", ["ctx", "x", "Z", "stream"]),
    ("csp_clique_scatter", ["ctx", "Z", "x", "stream"]),
    ("csp_clique_eigh", ["ctx", "a", "w", "Q", "ext", "stream"]),
    ("csp_clique_project", ["ctx", "a", "lo", "hi", "Z", "w", "info", "stream"])])
def test_entry_points_are_declared_and_bound(name, argnames):
    args = header_arguments(name)
    assert [a.split()[-1].lstrip("*") for a in args] == argnames
    assert name in _lib.SIGNATURES
    res, argtypes = _lib.SIGNATURES[name]
    assert res.__name__ == "c_int" and len(argtypes) == len(args)
    for a, t in zip(args, argtypes):
        if "*" in a:
            assert t is _lib.c_vp, (a, t)
        elif a.startswith("double"):
            assert t.__name__ == "c_double", (a, t)
    assert getattr(_lib.lib(), name).argtypes == argtypes
