"""The chip-wide block Jacobi for wide clique blocks on the device (tune(symb, TUNE_CEIG_WIDE, order); csrc/front_ceigw.hip)
behind clique_eigvalsh, clique_eigh and clique_project: against LAPACK on dense clique blocks, against the restatement of
tests/test_clique_wide_host.py for the block sweeps, and against the contract of the route.  Every case runs under
tune(symb, TUNE_CEIG_WIDE, 65).  Bounds: 16 nf eps max|w_ref| for the eigenvalues (the bound of tests/test_gpu_clique_eig.py),
GPU_FACTOR x UNITS of tests/test_clique_eigh_host.py for orthogonality, residual and projection."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import GPU_PATTERNS
from smcp_amd import _lib, chordal, problems
from smcp_amd.symbolic import Symbolic
from test_clique_eig_host import EPS, clique_blocks, inputs
from test_clique_eigh_host import GPU_FACTOR, UNITS, unpack
from test_clique_wide_host import block_jacobi_restatement, wide_block
from test_gpu_clique_eig import class_edge_pattern, on_device
from test_mrcompletion_host import blkval_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = 65
WIDE_ORDERS = [64, 65, 96, 97, 128, 129, 161]
KINDS = ["definite", "rank3", "indefinite"]
BOUNDS = [(0.0, math.inf), (-0.5, 0.5)]
ORTH, RES, PRJ = (GPU_FACTOR * u for u in UNITS)


def dense_cliques(orders):
    """disjoint dense cliques of these orders"""
    cl, first = [], 0
    for nf in orders:
        own = np.arange(first, first + nf)
        cl.append((own, own))
        first += nf
    return problems._from_cliques(first, cl)


PATS = {"wide_edges": lambda: dense_cliques(WIDE_ORDERS), "fam_top": GPU_PATTERNS["fam_top"], "class_edges": class_edge_pattern}
_SYMB, _CASE = {}, {}


def device_symb(name):
    """a Symbolic of this file's own: the tune is per context, and the contexts of the other files stay at 0"""
    if name not in _SYMB:
        _SYMB[name] = Symbolic(PATS[name]() if name in PATS else dense_cliques([int(name)]))
        _SYMB[name].device_init(0, 1)
    return _SYMB[name]


def case(name, kind):
    """(symb, blkA, dense blocks, their LAPACK eigendecompositions): made once, never changed"""
    if (name, kind) not in _CASE:
        symb = device_symb(name)
        for knd, blkA, blkB in inputs(symb, 11):
            if blkB is None:
                As = clique_blocks(symb, blkA)
                _CASE[(name, knd)] = (symb, blkA, As, [np.linalg.eigh(A) for A in As])
    return _CASE[(name, kind)]


def fro(A):
    return float(np.sqrt((A * A).sum()))


def n_wide(symb):
    return int((np.diff(symb.rowptr) >= WIDE).sum())


def check_against_lapack(symb, As, eigs, w, Q, projections):
    """parity of one call of each kind with LAPACK; projections: [(lo, hi, Z, info)]; the worst ratios"""
    wh = w.cpu().numpy()
    worst = [0.0, 0.0, 0.0, 0.0]
    Qs = unpack(symb, Q.cpu().numpy())
    for k, (A, (wr, Qr)) in enumerate(zip(As, eigs)):
        nf = len(wr)
        wk = wh[symb.rowptr[k]:symb.rowptr[k + 1]]
        assert (np.diff(wk) >= 0).all(), "clique %d (%d rows): w is not ascending, smallest step %.3e" % (k, nf, np.diff(wk).min())
        scale = nf * EPS * np.abs(wr).max()
        if scale > 0:
            worst[0] = max(worst[0], np.abs(wk - wr).max() / scale)
        else:
            assert (wk == 0).all(), "clique %d (%d rows): max|w| %.3e of a zero block, bound 0" % (k, nf, np.abs(wk).max())
        worst[1] = max(worst[1], np.abs(Qs[k].T @ Qs[k] - np.eye(nf)).max() / (nf * EPS))
        if fro(A) > 0:
            worst[2] = max(worst[2], np.abs(A @ Qs[k] - Qs[k] * wk).max() / (nf * EPS * fro(A)))
    for lo, hi, Z, info in projections:
        ih = info.cpu().numpy()
        for k, Zk in enumerate(unpack(symb, Z.cpu().numpy())):
            A, (wr, Qr) = As[k], eigs[k]
            nf = len(wr)
            unit = nf * EPS * fro(A)
            fr = np.clip(wr, lo, hi)
            Zr = (Qr * fr) @ Qr.T
            assert np.array_equal(Zk, Zk.T), "clique %d (%d rows): |Z - Z^T| %.3e, bound 0" % (k, nf, np.abs(Zk - Zk.T).max())   # symmetric bit for bit
            err = np.abs(Zk - 0.5 * (Zr + Zr.T)).max()
            if unit > 0:
                worst[3] = max(worst[3], err / unit)
            amb = (np.abs(wr - lo) <= PRJ * unit) | (np.abs(wr - hi) <= PRJ * unit)
            sure = int(((fr != wr) & ~amb).sum())
            assert sure <= ih[k, 0] <= sure + int(amb.sum()), "clique %d (%d rows): %d eigenvalues clipped by info, between %d and %d by LAPACK" % (
                k, nf, ih[k, 0], sure, sure + int(amb.sum()))        # the counts of info match
            assert abs(ih[k, 1] - ((fr - wr) ** 2).sum()) <= GPU_FACTOR * nf * EPS * fro(A) ** 2, "clique %d (%d rows): info distance off by %.3e = %.2f nf eps |A|^2, bound %.1f" % (
                k, nf, abs(ih[k, 1] - ((fr - wr) ** 2).sum()), abs(ih[k, 1] - ((fr - wr) ** 2).sum()) / (nf * EPS * fro(A) ** 2), GPU_FACTOR)
    return worst


def all_three(X):
    w = chordal.clique_eigvalsh(X)
    we, Q = chordal.clique_eigh(X)
    prj = []
    for lo, hi in BOUNDS:
        Z, wp, info = chordal.clique_project(X, lo, hi, return_info=True)
        prj.append((lo, hi, Z, info, wp))
    return w, we, Q, prj


@pytest.mark.parametrize("name", sorted(PATS))
@pytest.mark.parametrize("kind", KINDS)
def test_parity_and_contract(name, kind, capsys):
    symb, blkA, As, eigs = case(name, kind)
    X = on_device(symb, blkA)
    chordal.tune(symb, chordal.TUNE_CEIG_WIDE, 0)
    before = all_three(X)
    assert chordal.clique_eig_wide(symb) == 0, "wide cliques taken %d at tune 0, wanted 0" % chordal.clique_eig_wide(symb)
    chordal.tune(symb, chordal.TUNE_CEIG_WIDE, WIDE)
    try:
        w, we, Q, prj = all_three(X)
        assert chordal.clique_eig_wide(symb) == n_wide(symb) > 0, "%s %s: wide cliques taken %d, in the pattern %d" % (name, kind, chordal.clique_eig_wide(symb), n_wide(symb))             # the last call: a clique_project
        chordal.clique_eigvalsh(X)
        assert chordal.clique_eig_wide(symb) == n_wide(symb), "%s %s: wide cliques taken %d, in the pattern %d" % (name, kind, chordal.clique_eig_wide(symb), n_wide(symb))
        sweeps = chordal.clique_eig_sweeps(symb)
        w2, we2, Q2, prj2 = all_three(X)
        assert torch.equal(w, w2) and torch.equal(we, we2) and torch.equal(Q, Q2), "%s %s: w, w of eigh or Q differ from call to call" % (name, kind)                # the same bits from call to call
        for p, p2 in zip(prj, prj2):
            assert torch.equal(p[2], p2[2]) and torch.equal(p[3], p2[3]) and torch.equal(p[4], p2[4]), "%s %s: Z, info or w of clique_project differ from call to call" % (name, kind)
            assert torch.equal(p[4], w), "%s %s: w of clique_project differs from clique_eigvalsh by %.3e, bound 0" % (name, kind, float((p[4] - w).abs().max()))
        assert torch.equal(we, w), "%s %s: w of clique_eigh differs from clique_eigvalsh by %.3e, bound 0" % (name, kind, float((we - w).abs().max()))                                                # w of clique_eigh: the bits of clique_eigvalsh
        assert torch.equal(X.blkval.cpu(), torch.from_numpy(blkA)), "%s %s: the input was written" % (name, kind)               # the input is not written
        worst = check_against_lapack(symb, As, eigs, w, Q, [p[:4] for p in prj])
        with capsys.disabled():
            print("\n%s %s: eigenvalues %.2f nf eps max|w|, orthogonality %.2f u, residual %.2f u|A|, projection %.2f u|A|, "
                  "%d sweeps at most, %d wide cliques" % ((name, kind) + tuple(worst) + (sweeps, n_wide(symb))))
        assert worst[0] <= 16.0 and worst[1] <= ORTH and worst[2] <= RES and worst[3] <= PRJ, "%s %s: eigenvalues %.2f (bound 16), orthogonality %.2f (%.0f), residual %.2f (%.0f), projection %.2f (%.0f)" % (
            name, kind, worst[0], worst[1], ORTH, worst[2], RES, worst[3], PRJ)
        assert sweeps <= 30, "%s %s: %d sweeps, bound 30" % (name, kind, sweeps)
        if kind == "definite":                                                   # a block inside [lo, hi]: the bits of A_gg
            assert torch.equal(prj[0][2], chordal.clique_gather(X)) and not prj[0][3].any(), "%s %s: a block inside [lo, hi] is not the bits of A_gg, or info is not zero" % (name, kind)
    finally:
        chordal.tune(symb, chordal.TUNE_CEIG_WIDE, 0)
    after = all_three(X)
    assert chordal.clique_eig_wide(symb) == 0, "wide cliques taken %d after the tune went back to 0, wanted 0" % chordal.clique_eig_wide(symb)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and torch.equal(before[2], after[2]), "%s %s: the route at 0 after the tune differs from before it" % (name, kind)
    for p, p2 in zip(before[3], after[3]):
        assert torch.equal(p[2], p2[2]) and torch.equal(p[3], p2[3]) and torch.equal(p[4], p2[4]), "%s %s: clique_project at 0 after the tune differs from before it" % (name, kind)


@pytest.mark.parametrize("nf", [65, 97, 129])
@pytest.mark.parametrize("kind", ["indefinite", "graded"])
def test_block_sweeps_against_restatement(nf, kind, capsys):
    """one clique per context, so that CSP_Q_CEIG_SWEEPS is that clique's block sweeps: at most the restatement's on the
    block the device sees + 2 (one for a stop test that rounding moves, one of margin)"""
    symb = device_symb(str(nf))
    blk = blkval_of(symb, wide_block(nf, kind))
    A = clique_blocks(symb, blk)[0]
    wr, Qr, host_sweeps, ok = block_jacobi_restatement(A)
    assert ok, "order %d %s: the restatement did not converge" % (nf, kind)
    X = on_device(symb, blk)
    chordal.tune(symb, chordal.TUNE_CEIG_WIDE, WIDE)
    try:
        w = chordal.clique_eigvalsh(X)
        s1 = chordal.clique_eig_sweeps(symb)
        we, Q = chordal.clique_eigh(X)
        s2 = chordal.clique_eig_sweeps(symb)
        assert chordal.clique_eig_wide(symb) == 1, "order %d %s: wide cliques taken %d, wanted 1" % (nf, kind, chordal.clique_eig_wide(symb))
    finally:
        chordal.tune(symb, chordal.TUNE_CEIG_WIDE, 0)
    ref = np.linalg.eigvalsh(A)
    ratio = np.abs(w.cpu().numpy() - ref).max() / (nf * EPS * np.abs(ref).max())
    with capsys.disabled():
        print("\norder %d %s: %d block sweeps on the device, %d in the restatement, eigenvalues %.2f nf eps max|w|"
              % (nf, kind, s1, host_sweeps, ratio))
    assert s1 == s2 and torch.equal(w, we), "order %d %s: block sweeps %d without and %d with eigenvectors" % (nf, kind, s1, s2)
    assert s1 <= host_sweeps + 2, "order %d %s: %d block sweeps, bound %d" % (nf, kind, s1, host_sweeps + 2)
    assert ratio <= 16.0, "order %d %s: eigenvalues %.2f nf eps max|w|, bound 16" % (nf, kind, ratio)
    Qh = unpack(symb, Q.cpu().numpy())[0]
    orth, res = np.abs(Qh.T @ Qh - np.eye(nf)).max() / (nf * EPS), np.abs(A @ Qh - Qh * w.cpu().numpy()).max() / (nf * EPS * fro(A))
    assert np.abs(Qh.T @ Qh - np.eye(nf)).max() <= ORTH * nf * EPS, "order %d %s: orthogonality %.2f units, bound %.0f" % (nf, kind, orth, ORTH)
    assert np.abs(A @ Qh - Qh * w.cpu().numpy()).max() <= RES * nf * EPS * fro(A), "order %d %s: residual %.2f units, bound %.0f" % (nf, kind, res, RES)


def test_diagonal_block_takes_no_sweep():
    symb = device_symb("97")
    d = np.random.default_rng(5).standard_normal(97)
    blk = blkval_of(symb, np.diag(d))
    A = clique_blocks(symb, blk)[0]
    X = on_device(symb, blk)
    chordal.tune(symb, chordal.TUNE_CEIG_WIDE, WIDE)
    try:
        w, Q = chordal.clique_eigh(X)
        assert chordal.clique_eig_sweeps(symb) == 0 and chordal.clique_eig_wide(symb) == 1, "diagonal block: %d sweeps (wanted 0), %d wide cliques (wanted 1)" % (chordal.clique_eig_sweeps(symb), chordal.clique_eig_wide(symb))
    finally:
        chordal.tune(symb, chordal.TUNE_CEIG_WIDE, 0)
    assert np.array_equal(w.cpu().numpy(), np.sort(np.diag(A))), "diagonal block: w differs from the sorted diagonal by %.3e, bound 0" % np.abs(w.cpu().numpy() - np.sort(np.diag(A))).max()
    Qh = unpack(symb, Q.cpu().numpy())[0]
    assert np.array_equal(np.abs(Qh).sum(axis=0), np.ones(97)) and np.array_equal(Qh[np.argsort(np.diag(A), kind="stable")], np.eye(97)), "diagonal block: Q is not the permutation of the sort"


def test_non_finite_entry_is_reported_and_stays_in_its_clique():
    symb, good, As, eigs = case("wide_edges", "indefinite")
    kb = int(np.flatnonzero(np.diff(symb.rowptr) == 97)[0])
    bad = good.copy()
    bad[symb.blkptr[kb] + 70] = np.nan
    q = chordal.clique_ptr(symb)
    chordal.tune(symb, chordal.TUNE_CEIG_WIDE, WIDE)
    try:
        with pytest.raises(RuntimeError, match="did not converge"):
            chordal.clique_eigvalsh(on_device(symb, bad))
        with pytest.raises(RuntimeError, match="did not converge"):
            chordal.clique_eigh(on_device(symb, bad))
        with pytest.raises(RuntimeError, match="did not converge"):
            chordal.clique_project(on_device(symb, bad))
        L = _lib.lib()
        Xb, Xg = on_device(symb, bad), on_device(symb, good)
        wg, Qg = chordal.clique_eigh(Xg)
        Zg, _, ig = chordal.clique_project(Xg, -0.5, 0.5, return_info=True)
        w, w1, w2 = torch.zeros_like(wg), torch.zeros_like(wg), torch.zeros_like(wg)
        Q, Z, info = torch.zeros_like(Qg), torch.zeros_like(Zg), torch.zeros_like(ig)
        assert L.csp_clique_eigvalsh(symb.handle, Xb.blkval.data_ptr(), None, w1.data_ptr(), None, None) == -7
        assert L.csp_clique_eigh(symb.handle, Xb.blkval.data_ptr(), w.data_ptr(), Q.data_ptr(), None, None) == -7
        assert L.csp_clique_project(symb.handle, Xb.blkval.data_ptr(), -0.5, 0.5, Z.data_ptr(), w2.data_ptr(), info.data_ptr(), None) == -7
        torch.cuda.synchronize()
        wm = torch.ones_like(wg, dtype=torch.bool)
        wm[int(symb.rowptr[kb]):int(symb.rowptr[kb + 1])] = False
        qm = torch.ones_like(Qg, dtype=torch.bool)
        qm[int(q[kb]):int(q[kb + 1])] = False
        im = torch.ones(symb.Nsn, dtype=torch.bool, device="cuda")
        im[kb] = False
        for got, ref, m in ((w, wg, wm), (w1, wg, wm), (w2, wg, wm), (Q, Qg, qm), (Z, Zg, qm), (info, ig, im)):
            assert torch.isnan(got[~m]).all() and torch.equal(got[m], ref[m]), "NaN case: an output is not NaN in clique %d alone, or differs elsewhere" % kb     # NaN in that clique only
        w3, Q3 = chordal.clique_eigh(Xg)                                          # nothing is left behind for the next call
        assert torch.equal(w3, wg) and torch.equal(Q3, Qg), "the call after the NaN differs from the clean run"
    finally:
        chordal.tune(symb, chordal.TUNE_CEIG_WIDE, 0)


def test_orders_without_three_blocks_are_refused():
    symb = device_symb("wide_edges")
    for value in (1, 64, -1):
        with pytest.raises(RuntimeError, match="invalid argument"):
            chordal.tune(symb, chordal.TUNE_CEIG_WIDE, value)
        assert _lib.lib().csp_tune(symb.handle, 7, value) == -1
    chordal.tune(symb, chordal.TUNE_CEIG_WIDE, 65)
    chordal.tune(symb, chordal.TUNE_CEIG_WIDE, 0)


def poisoned_workspace_run():
    """the body of the child of test_never_written_workspace_is_not_read: wide_edges, indefinite, all three calls"""
    symb, blkA, As, eigs = case("wide_edges", "indefinite")
    X = on_device(symb, blkA)
    chordal.tune(symb, chordal.TUNE_CEIG_WIDE, WIDE)
    w, we, Q, prj = all_three(X)
    assert chordal.clique_eig_wide(symb) == n_wide(symb), "poison: wide cliques taken %d, in the pattern %d" % (chordal.clique_eig_wide(symb), n_wide(symb))
    assert torch.equal(w, we) and torch.equal(prj[0][4], w), "poison: w of the three calls differ"
    worst = check_against_lapack(symb, As, eigs, w, Q, [p[:4] for p in prj])
    print("poisoned workspace: eigenvalues %.2f, orthogonality %.2f, residual %.2f, projection %.2f" % tuple(worst))
    assert worst[0] <= 16.0 and worst[1] <= ORTH and worst[2] <= RES and worst[3] <= PRJ, (worst, (16.0, ORTH, RES, PRJ))


def test_never_written_workspace_is_not_read():
    """SMCP_POISON=1 fills every fp64 buffer with 4.5e150 when it is allocated (the switch is cached per process: a fresh
    child interpreter); the ragged last blocks of wide_edges are where a never-written workspace word would be read"""
    env = dict(os.environ, SMCP_POISON="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "poisoned workspace" in r.stdout


if __name__ == "__main__":
    poisoned_workspace_run()
