"""Eigenvectors and spectral projections of the clique blocks and the packed clique blocks on the device
(smcp_amd.chordal.clique_eigh / clique_project / clique_gather / clique_scatter; csrc/front_ceig.hip) against LAPACK on
dense clique blocks, against the dense definitions and against their contract.  Restatements, references and units:
tests/test_clique_eigh_host.py; the bounds here are 16 times what the restatement is held to there."""
import math

import numpy as np
import pytest
import torch

from helpers import PATTERNS, launch_census
from smcp_amd import _lib, chordal, problems
from smcp_amd.symbolic import Symbolic
from test_clique_eig_host import EPS, clique_blocks
from test_clique_eigh_host import (GPU_FACTOR, UNITS, gather_ref, integer_on_V, lower_slots, multiplicity_count, pack,
                                   scatter_dense, unpack)
from test_gpu_clique_eig import PATS, case, device_symb, on_device
from test_mrcompletion_host import leaf_clique, pd_on_V

pytestmark = pytest.mark.gpu

KINDS = ["definite", "rank3", "indefinite"]
BOUNDS = [(0.0, math.inf), (-0.5, 0.5), (-math.inf, 0.0)]
ORTH, RES, PRJ = (GPU_FACTOR * u for u in UNITS)        # in u = nf eps, u |A|_F, u |A|_F
_REF, WORST = {}, {"orth": 0.0, "res": 0.0, "prj": 0.0, "sweeps": 0}


@pytest.fixture(scope="module", autouse=True)
def leave_no_device_tensor_behind():
    """the Symbolics are shared with tests/test_gpu_clique_eig.py and live as long as the process: the multiplicities cached
    on them here are dropped again, so that no device tensor of this module outlives it"""
    yield
    import gc
    from test_gpu_clique_eig import _SYMB
    for symb in _SYMB.values():
        symb._cache.pop("clique_mult", None)
    gc.collect()


def reference(name, kind):
    """(dense blocks, their LAPACK eigenvalues) of a case: made once, never changed"""
    if (name, kind) not in _REF:
        symb, blkA, _, _ = case(name, kind)
        As = clique_blocks(symb, blkA)
        _REF[(name, kind)] = (As, [np.linalg.eigh(A) for A in As])
    return _REF[(name, kind)]


def host_blocks(symb, Z):
    return unpack(symb, Z.cpu().numpy())


def fro(A):
    return float(np.sqrt((A * A).sum()))


@pytest.mark.parametrize("name", sorted(PATS))
@pytest.mark.parametrize("kind", KINDS)
def test_eigh_against_lapack(name, kind, capsys):
    symb, blkA, _, _ = case(name, kind)
    As, _ = reference(name, kind)
    A = on_device(symb, blkA)
    w, Q = chordal.clique_eigh(A)
    sweeps = chordal.clique_eig_sweeps(symb)
    w2, Q2 = chordal.clique_eigh(A)
    assert torch.equal(w, w2) and torch.equal(Q, Q2)                          # the same bits from call to call
    assert torch.equal(w, chordal.clique_eigvalsh(A))                         # the spectrum of the call without vectors
    assert torch.equal(A.blkval.cpu(), torch.from_numpy(blkA))                # the input is not written
    assert Q.dtype == torch.float64 and Q.shape == (int(chordal.clique_ptr(symb)[-1]),)
    wh = w.cpu().numpy()
    last = symb.Nsn - 1
    assert torch.equal(chordal.clique_block(symb, Q, last).cpu(), torch.from_numpy(host_blocks(symb, Q)[last]))
    orth = res = 0.0
    for k, Qk in enumerate(host_blocks(symb, Q)):
        Ak, wk = As[k], wh[symb.rowptr[k]:symb.rowptr[k + 1]]
        nf = len(wk)
        orth = max(orth, np.abs(Qk.T @ Qk - np.eye(nf)).max() / (nf * EPS))
        if fro(Ak) > 0:
            res = max(res, np.abs(Ak @ Qk - Qk * wk).max() / (nf * EPS * fro(Ak)))
        else:
            assert (wk == 0).all()
    for key, v in (("orth", orth), ("res", res), ("sweeps", sweeps)):
        WORST[key] = max(WORST[key], v)
    with capsys.disabled():
        print("\n%s %s: orthogonality %.2f u, residual %.2f u|A|, %d sweeps (so far: %.2f, %.2f, %d)"
              % (name, kind, orth, res, sweeps, WORST["orth"], WORST["res"], WORST["sweeps"]))
    assert orth <= ORTH and res <= RES
    assert sweeps <= 30


@pytest.mark.parametrize("name", sorted(PATS))
@pytest.mark.parametrize("kind", KINDS)
def test_project_against_lapack(name, kind, capsys):
    """Z against Q clip(w) Q^T of LAPACK, its symmetry and spectrum, and info.  The count of clipped eigenvalues is compared
    with the reference's up to the eigenvalues that lie within the bound of lo or hi, which either side may count: those are
    at most 1 % of all on the definite and indefinite kinds and on rank 3 with (-0.5, 0.5) (asserted); a rank 3 block has
    nf - 3 eigenvalues AT a bound of 0, so there the count is only held between the sure and the possible ones."""
    symb, blkA, _, _ = case(name, kind)
    As, eigs = reference(name, kind)
    X = on_device(symb, blkA)
    worst = 0.0
    for lo, hi in BOUNDS:
        Z, w, info = chordal.clique_project(X, lo, hi, return_info=True)
        assert torch.equal(Z, chordal.clique_project(X, lo, hi))              # the same bits, with or without w
        assert info.shape == (symb.Nsn, 2)
        ih = info.cpu().numpy()
        near = total = 0
        for k, Zk in enumerate(host_blocks(symb, Z)):
            Ak, (wr, Qr) = As[k], eigs[k]
            nf = len(wr)
            unit = nf * EPS * fro(Ak)
            fr = np.clip(wr, lo, hi)
            Zr = (Qr * fr) @ Qr.T
            assert np.array_equal(Zk, Zk.T)                                   # symmetric bit for bit
            err = np.abs(Zk - 0.5 * (Zr + Zr.T)).max()
            if unit > 0:
                worst = max(worst, err / unit)
            assert err <= PRJ * unit
            lam = np.linalg.eigvalsh(Zk)
            assert lam[0] >= lo - PRJ * unit and lam[-1] <= hi + PRJ * unit
            amb = (np.abs(wr - lo) <= PRJ * unit) | (np.abs(wr - hi) <= PRJ * unit)
            sure = int(((fr != wr) & ~amb).sum())
            assert sure <= ih[k, 0] <= sure + int(amb.sum())
            near += int(amb.sum())
            total += nf
            assert abs(ih[k, 1] - ((fr - wr) ** 2).sum()) <= GPU_FACTOR * nf * EPS * fro(Ak) ** 2
        if kind != "rank3" or (lo, hi) == (-0.5, 0.5):
            assert near <= 0.01 * total, (near, total)
        if kind == "definite" and (lo, hi) == (0.0, math.inf):               # nothing to clip: the bits of the gather
            assert torch.equal(Z, chordal.clique_gather(X)) and not info.any()
    assert torch.equal(X.blkval.cpu(), torch.from_numpy(blkA))
    WORST["prj"] = max(WORST["prj"], worst)
    with capsys.disabled():
        print("\n%s %s: projection %.2f u|A| (so far: %.2f)" % (name, kind, worst, WORST["prj"]))


@pytest.mark.parametrize("name", sorted(PATS))
def test_gather_and_scatter_against_dense_definitions(name):
    symb, blkA, _, _ = case(name, "indefinite")
    X = on_device(symb, blkA)
    Zg = chordal.clique_gather(X)
    assert torch.equal(Zg.cpu(), torch.from_numpy(gather_ref(symb, blkA)))
    assert torch.equal(Zg, chordal.clique_gather(X)) and torch.equal(X.blkval.cpu(), torch.from_numpy(blkA))
    low = lower_slots(symb)
    Zh = np.random.default_rng(7).standard_normal(int(chordal.clique_ptr(symb)[-1]))
    Z = torch.from_numpy(Zh.copy()).cuda()
    got = chordal.clique_scatter(symb, Z)
    assert torch.equal(got.blkval, chordal.clique_scatter(symb, Z, "sum").blkval) and torch.equal(Z.cpu(), torch.from_numpy(Zh))
    g = got.blkval.cpu().numpy()
    assert (np.abs(g - scatter_dense(symb, Zh)) <= symb.nlev * EPS * scatter_dense(symb, Zh, absolute=True)).all()
    assert (g[~low] == 0).all()                                               # above the diagonal of the diagonal blocks
    Zi = np.rint(8 * Zh)
    gi = chordal.clique_scatter(symb, torch.from_numpy(Zi).cuda()).blkval.cpu().numpy()
    assert np.array_equal(gi, scatter_dense(symb, Zi))                        # integers: exact
    assert np.array_equal(chordal.clique_multiplicity(symb).cpu().numpy(), multiplicity_count(symb))
    assert chordal.clique_multiplicity(symb) is chordal.clique_multiplicity(symb)
    Xi = integer_on_V(symb, 3)
    back = chordal.clique_scatter(symb, chordal.clique_gather(on_device(symb, Xi)), reduce="mean")
    assert np.array_equal(back.blkval.cpu().numpy(), Xi)                      # scatter-mean(gather(X)) == X


# ---- contract ---------------------------------------------------------------------------------------------------------
def test_cliques_of_order_one_and_two():
    for bw in (0, 1):
        symb = Symbolic(problems.band_pattern(12, bw))
        symb.device_init(0, 1)
        blk = np.random.default_rng(bw).standard_normal(symb.blklen)
        X = on_device(symb, blk)
        w, Q = chordal.clique_eigh(X)
        Z = chordal.clique_project(X)
        wh = w.cpu().numpy()
        assert max(np.diff(symb.rowptr)) == bw + 1
        for k, (A, Qk, Zk) in enumerate(zip(clique_blocks(symb, blk), host_blocks(symb, Q), host_blocks(symb, Z))):
            nf, wk = A.shape[0], wh[symb.rowptr[k]:symb.rowptr[k + 1]]
            wr, Qr = np.linalg.eigh(A)
            assert np.abs(wk - wr).max() <= ORTH * nf * EPS * fro(A)
            assert np.abs(Qk.T @ Qk - np.eye(nf)).max() <= ORTH * nf * EPS
            assert np.abs(A @ Qk - Qk * wk).max() <= RES * nf * EPS * fro(A)
            assert np.abs(Zk - (Qr * np.clip(wr, 0, None)) @ Qr.T).max() <= PRJ * nf * EPS * fro(A)


def test_non_finite_entry_is_reported_and_stays_in_its_clique():
    symb = device_symb("nested")
    good = pd_on_V(symb, 5)
    bad = good.copy()
    kb = leaf_clique(symb)
    bad[symb.blkptr[kb] + 1] = np.nan
    q = chordal.clique_ptr(symb)
    with pytest.raises(RuntimeError, match="did not converge"):
        chordal.clique_eigh(on_device(symb, bad))
    with pytest.raises(RuntimeError, match="did not converge"):
        chordal.clique_project(on_device(symb, bad))
    L = _lib.lib()
    Xb, Xg = on_device(symb, bad), on_device(symb, good)
    wg, Qg = chordal.clique_eigh(Xg)
    Zg, _, ig = chordal.clique_project(Xg, -0.5, 0.5, return_info=True)
    w = torch.zeros_like(wg)
    Q = torch.zeros_like(Qg)
    info = torch.zeros_like(ig)
    assert L.csp_clique_eigh(symb.handle, Xb.blkval.data_ptr(), w.data_ptr(), Q.data_ptr(), None, None) == -7
    Z = torch.zeros_like(Zg)
    w2 = torch.zeros_like(wg)
    assert L.csp_clique_project(symb.handle, Xb.blkval.data_ptr(), -0.5, 0.5, Z.data_ptr(), w2.data_ptr(), info.data_ptr(), None) == -7
    torch.cuda.synchronize()
    wm = torch.ones_like(wg, dtype=torch.bool)
    wm[int(symb.rowptr[kb]):int(symb.rowptr[kb + 1])] = False
    qm = torch.ones_like(Qg, dtype=torch.bool)
    qm[int(q[kb]):int(q[kb + 1])] = False
    im = torch.ones(symb.Nsn, dtype=torch.bool, device="cuda")
    im[kb] = False
    for got, ref, m in ((w, wg, wm), (w2, wg, wm), (Q, Qg, qm), (Z, Zg, qm), (info, ig, im)):
        assert torch.isnan(got[~m]).all() and torch.equal(got[m], ref[m])     # NaN in that clique only
    w3, Q3 = chordal.clique_eigh(Xg)                                          # nothing is left behind for the next call
    assert torch.equal(w3, wg) and torch.equal(Q3, Qg)


def test_bad_bounds_and_foreign_symbolic():
    symb = device_symb("arrow")
    X = on_device(symb, pd_on_V(symb, 5))
    for lo, hi in ((1.0, 0.5), (math.nan, 1.0), (0.0, math.nan), (math.inf, -math.inf)):
        with pytest.raises(ValueError):
            chordal.clique_project(X, lo, hi)
    info = torch.empty((symb.Nsn, 2), dtype=torch.float64, device="cuda")
    Z = chordal.clique_gather(X)
    L = _lib.lib()
    assert L.csp_clique_project(symb.handle, X.blkval.data_ptr(), 1.0, 0.5, Z.data_ptr(), None, info.data_ptr(), None) == -1
    assert L.csp_clique_project(symb.handle, X.blkval.data_ptr(), math.nan, 0.5, Z.data_ptr(), None, info.data_ptr(), None) == -1
    other = device_symb("band")
    with pytest.raises(ValueError):
        chordal.clique_scatter(other, Z)                                      # blocks of another Symbolic
    with pytest.raises(ValueError):
        chordal.clique_block(other, Z, 0)
    with pytest.raises(ValueError):
        chordal.clique_scatter(symb, Z, reduce="max")
    with pytest.raises(ValueError):
        chordal.clique_scatter(symb, Z.cpu())


def test_overlapping_pointers_are_refused():
    symb = device_symb("arrow")
    X = on_device(symb, pd_on_V(symb, 5))
    p, bl = X.blkval.data_ptr(), symb.blklen
    qlen, wlen = int(chordal.clique_ptr(symb)[-1]), int(symb.rowptr[-1])
    buf = torch.zeros(qlen + wlen + 2 * symb.Nsn + 8, dtype=torch.float64, device="cuda")
    Z, w, info = buf.data_ptr(), buf.data_ptr() + 8 * qlen, buf.data_ptr() + 8 * (qlen + wlen)
    last = p + 8 * (bl - 1)
    L = _lib.lib()
    h = symb.handle
    assert L.csp_clique_gather(h, p, last, None) == -1 and L.csp_clique_gather(h, None, Z, None) == -1
    assert L.csp_clique_gather(h, p, Z, None) == 0
    assert L.csp_clique_scatter(h, Z, Z + 8 * (qlen - 1), None) == -1 and L.csp_clique_scatter(h, Z, None, None) == -1
    assert L.csp_clique_eigh(h, p, last, Z, None, None) == -1                 # w in a
    assert L.csp_clique_eigh(h, p, w, last, None, None) == -1                 # Q in a
    assert L.csp_clique_eigh(h, p, w, Z, last, None) == -1                    # ext in a
    assert L.csp_clique_eigh(h, p, Z + 8 * (qlen - 1), Z, None, None) == -1   # w in Q
    assert L.csp_clique_eigh(h, p, w, Z, w + 8 * (wlen - 1), None) == -1      # ext in w
    assert L.csp_clique_eigh(h, p, None, Z, None, None) == -1
    assert L.csp_clique_eigh(h, p, w, Z, info, None) == 0
    assert L.csp_clique_project(h, p, 0.0, 1.0, last, w, info, None) == -1    # Z in a
    assert L.csp_clique_project(h, p, 0.0, 1.0, Z, w, last, None) == -1       # info in a
    assert L.csp_clique_project(h, p, 0.0, 1.0, Z, Z, info, None) == -1       # w in Z
    assert L.csp_clique_project(h, p, 0.0, 1.0, Z, w, w + 8 * (wlen - 1), None) == -1
    assert L.csp_clique_project(h, p, 0.0, 1.0, Z, None, None, None) == -1
    assert L.csp_clique_project(h, p, 0.0, 1.0, Z, None, info, None) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["band", "arrow", "fam_top"])
def test_launch_counts(name):
    symb = device_symb(name)
    X = on_device(symb, pd_on_V(symb, 5) if name in PATTERNS else case(name, "indefinite")[1])
    Z = chordal.clique_gather(X)
    chordal.clique_eigh(X), chordal.clique_project(X), chordal.clique_scatter(symb, Z)       # buffers of the first calls
    for fn in (lambda: chordal.clique_eigh(X), lambda: chordal.clique_project(X, -0.5, 0.5, return_info=True)):
        counts, census = launch_census(symb, fn)
        assert 1 <= counts["k_ceig"] <= 6 and counts["k_ceig_reduce"] == 1
        assert set(counts) <= {"k_ceig", "k_ceig_reduce", "k_gather_level"}  # only the gathers grow with the depth of the tree
        assert counts.get("k_gather_level", 0) <= symb.nlev
        # the kernels behind the ids: the Jacobi kernel with eigenvectors, one launch per LDS class in use, and the gathers
        assert census.get("k_ceig_vec", 0) == counts["k_ceig"] and census["k_ceig_reduce"] == 1, census
        assert census.get("k_gather_level", 0) == counts.get("k_gather_level", 0), census
        assert set(census) <= {"k_ceig_vec", "k_ceig_reduce", "k_gather_level"}, census
    counts, census = launch_census(symb, lambda: chordal.clique_scatter(symb, Z))
    assert counts == {"k_gather_level": symb.nlev} and census == {"k_clique_scatter": symb.nlev}, census
    counts, census = launch_census(symb, lambda: chordal.clique_gather(X))
    assert set(counts) == {"k_gather_level"} and counts["k_gather_level"] <= symb.nlev + 1
    assert census.get("k_clique_gather", 0) >= 1 and sum(census.values()) == counts["k_gather_level"], census
    assert set(census) <= {"k_clique_gather", "k_gather_level"}, census


def test_device_bytes_grow_on_the_first_call_only():
    symb = Symbolic(PATS["fam_top"]())
    symb.device_init(0, 1)
    X = on_device(symb, case("fam_top", "indefinite")[1])

    def everything():
        Z = chordal.clique_gather(X)
        chordal.clique_scatter(symb, Z, "mean")
        chordal.clique_eigh(X)
        chordal.clique_project(X)
        chordal.clique_project(X, -1.0, 1.0, return_info=True)
        torch.cuda.synchronize()

    b0 = symb.device_bytes()
    everything()
    b1 = symb.device_bytes()
    everything()
    assert b1 > b0 and symb.device_bytes() == b1
