"""chordal.cone_project and csp_cone_project_steps on the device (csrc/front_ceig.hip: k_cone_split, k_cone_update,
k_cone_resid) against the numpy restatement of the iteration, against the definition of the projection and against their
contract.  Restatement, inputs, units and K: tests/test_cone_project_host.py; the device is held to 16 times the units the
kernel's form is held to there."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import smcp_amd
from helpers import EXTRA, launch_census
from smcp_amd import _lib, chordal
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.symbolic import Symbolic
from test_clique_eig_host import EPS
from test_clique_eigh_host import lower_slots, unpack
from test_cone_project_host import (CONE_UNITS, GPU_FACTOR, K_BOUND, KINDS, PARAMS, SMALL, cone_input, cone_project_restatement,
                                    norm_V, scatter_blocks, unit_of)
from test_gpu_clique_eig import PATS, device_symb, on_device
from test_mrcompletion_host import clique_rows, dense_of, leaf_clique

pytestmark = pytest.mark.gpu

ALL = SMALL + ["diag", "one_clique", "class_edges", "fam_top"]
TOL = 1e-8
_OWN, _REF = {}, {}


@pytest.fixture(scope="module", autouse=True)
def leave_no_device_tensor_behind():
    """the Symbolics are shared with other modules and live as long as the process: what this module caches on them on the
    device is dropped again"""
    yield
    import gc
    from test_gpu_clique_eig import _SYMB
    for symb in list(_SYMB.values()) + list(_OWN.values()):
        symb._cache.pop("clique_mult", None)
        symb._cache.pop("cone_weights", None)
    _OWN.clear()
    gc.collect()


def symb_of(name):
    if name in PATS:
        return device_symb(name)
    if name not in _OWN:
        _OWN[name] = Symbolic(EXTRA[name]())
        _OWN[name].device_init(0, 1)
    return _OWN[name]


def reference(name, kind, **kw):
    """a run of the restatement: made once per case, never changed"""
    key = (name, kind) + tuple(sorted(kw.items()))
    if key not in _REF:
        symb = symb_of(name)
        _REF[key] = cone_project_restatement(symb, cone_input(symb, kind), **kw)
    return _REF[key]


def bound(symb, scale):
    return GPU_FACTOR * CONE_UNITS * unit_of(symb, scale)


def start(symb, blk):
    """the state of iteration 0: (a, x, U, W) on the device"""
    a = on_device(symb, blk)
    W = chordal.clique_gather(a)
    return a, a.copy(), torch.zeros_like(W), W


def run_steps(symb, a, x, U, W, rho, relax, it0, n, hist):
    rc = _lib.lib().csp_cone_project_steps(symb.handle, a.blkval.data_ptr(), x.blkval.data_ptr(), U.data_ptr(), W.data_ptr(), rho, relax,
                                           it0, n, hist.data_ptr(), None)
    assert rc == 0, rc


def next_look(it):
    return min(e for e in (b + n for b, n in chordal.cone_looks(10 ** 4)) if e >= it)


# ---- 1. three iterations against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rho,relax", PARAMS)
def test_three_iterations_against_the_restatement(name, kind, rho, relax, capsys):
    symb = symb_of(name)
    blk = cone_input(symb, kind)
    bd = bound(symb, max(1.0, norm_V(symb, blk)))
    ref = reference(name, kind, rho=rho, relax=relax, steps=3, near=bd)
    a, x, U, W = start(symb, blk)
    hist = torch.zeros((3, 4), dtype=torch.float64, device="cuda")
    run_steps(symb, a, x, U, W, rho, relax, 0, 3, hist)
    a2, x2, U2, W2 = start(symb, blk)
    hist2 = torch.zeros((3, 4), dtype=torch.float64, device="cuda")
    run_steps(symb, a2, x2, U2, W2, rho, relax, 0, 1, hist2)
    run_steps(symb, a2, x2, U2, W2, rho, relax, 1, 2, hist2)
    for p, q in ((x.blkval, x2.blkval), (U, U2), (W, W2), (hist, hist2)):
        assert torch.equal(p, q)                                              # 1 + 2 steps are the 3 of one call
    assert torch.equal(a.blkval.cpu(), torch.from_numpy(np.array(blk)))       # the input is not written
    xh, Uh, Wh, hh = x.blkval.cpu().numpy(), U.cpu().numpy(), W.cpu().numpy(), hist.cpu().numpy()
    worst = max(np.abs(xh - ref["x"]).max(), np.abs(Uh - ref["U"]).max(), np.abs(Wh - ref["W"]).max()) / unit_of(symb, ref["scale"])
    with capsys.disabled():
        print("\n%s %s rho %g relax %g: %.2f units, hist %s" % (name, kind, rho, relax, worst, hh[-1, :3].tolist()))
    assert worst <= GPU_FACTOR * CONE_UNITS
    assert (xh[~lower_slots(symb)] == 0).all()                                # above the diagonal of the diagonal blocks
    for Uk, Wk in zip(unpack(symb, Uh), unpack(symb, Wh)):
        assert np.array_equal(Uk, Uk.T) and np.array_equal(Wk, Wk.T)          # mirrored on store
    # entries differ by at most bd, so the norms differ by at most bd sqrt(number of entries)
    assert (np.abs(np.sqrt(hh[:, 0]) - np.sqrt(ref["hist"][:, 0])) <= 3 * bd * math.sqrt(len(Uh))).all()       # x, Z = W + U
    assert (np.abs(np.sqrt(hh[:, 1]) - np.sqrt(ref["hist"][:, 1])) <= 2 * bd * symb.n).all()
    assert (np.abs(hh[:, 2] - ref["hist"][:, 2]) <= ref["near"]).all()
    assert (hh[:, 3] == 0).all()


# ---- 2. convergence and certificate ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_convergence_and_certificate(name, capsys):
    symb = symb_of(name)
    blk = cone_input(symb, "noisy")
    ref = reference(name, "noisy", tol=1e-12, maxit=5000, snapshots=(TOL,))
    A = on_device(symb, blk)
    X, info = chordal.cone_project(A, tol=TOL, return_info=True)
    s = ref["scale"]
    with capsys.disabled():
        print("\n%s: %d iterations (restatement %d), primal %.1e dual %.1e, sweeps %d"
              % (name, info["iterations"], ref["snap"][TOL][0], info["primal"], info["dual"], info["sweeps"]))
    assert info["converged"] and max(info["primal"], info["dual"]) <= TOL
    assert info["iterations"] <= next_look(ref["snap"][TOL][0]) + chordal.CONE_CHUNK
    assert info["hist"].shape == (info["iterations"], 4) and 0 <= info["sweeps"] <= 30
    xh = X.blkval.cpu().numpy()
    margin = 4 * K_BOUND * TOL * s
    assert norm_V(symb, xh - ref["x"]) <= margin
    assert abs(info["distance"] - norm_V(symb, xh - blk)) <= 1e-12 * s
    Xd, Ad = dense_of(symb, xh), dense_of(symb, np.array(blk))
    lam = min(np.linalg.eigvalsh(Xd[np.ix_(clique_rows(symb, k), clique_rows(symb, k))])[0] for k in range(symb.Nsn))
    assert lam >= -margin and np.linalg.eigvalsh(Xd - Ad)[0] >= -margin and abs((Xd * (Xd - Ad)).sum()) <= margin * s
    Uh = info["U"].cpu().numpy()
    for Uk in unpack(symb, Uh):
        assert np.linalg.eigvalsh(Uk)[-1] <= bound(symb, s)
    # X - A = -rho sum E_k U_k E_k^T + rho sum E_k (Z_k - X_gg) E_k^T: within sqrt(Nsn) r + Nsn s of the first term
    gap = np.sqrt(((Xd - Ad + scatter_blocks(symb, Uh)) ** 2).sum())
    assert gap <= (math.sqrt(symb.Nsn) * info["primal"] + symb.Nsn * info["dual"]) * s + symb.Nsn * bound(symb, s)


# ---- 3. exact cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL + ["diag", "one_clique", "class_edges"])
def test_input_inside_the_cone_comes_back_bit_for_bit(name):
    symb = symb_of(name)
    A = on_device(symb, cone_input(symb, "incone"))
    X, info = chordal.cone_project(A, return_info=True)
    used = torch.from_numpy(lower_slots(symb)).cuda()
    assert torch.equal(X.blkval[used], A.blkval[used]) and not X.blkval[~used].any()
    assert info["iterations"] == 1 and info["converged"] and not info["U"].any()


@pytest.mark.parametrize("name", ["class_edges", "diag"])
@pytest.mark.parametrize("kind", ["noisy", "indef"])
def test_disjoint_cliques_are_projected_clique_by_clique(name, kind):
    symb = symb_of(name)
    A = on_device(symb, cone_input(symb, kind))
    X, info = chordal.cone_project(A, return_info=True)
    ref = chordal.clique_scatter(symb, chordal.clique_project(A), "mean")
    assert info["converged"] and info["iterations"] <= 2
    assert (X.blkval - ref.blkval).abs().max().item() <= bound(symb, max(1.0, norm_V(symb, cone_input(symb, kind))))


@pytest.mark.parametrize("kind", ["noisy", "indef"])
def test_one_clique_is_the_dense_projection(kind):
    symb = symb_of("one_clique")
    blk = cone_input(symb, kind)
    X, info = chordal.cone_project(on_device(symb, blk), return_info=True)
    Ad = dense_of(symb, np.array(blk))
    w, Q = np.linalg.eigh(Ad)
    P = (Q * np.maximum(w, 0.0)) @ Q.T
    assert info["converged"] and info["iterations"] <= 2
    assert np.abs(dense_of(symb, X.blkval.cpu().numpy()) - 0.5 * (P + P.T)).max() <= bound(symb, max(1.0, norm_V(symb, blk)))


# ---- 4. the dual cone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_dual_projection_by_moreau(name):
    symb = symb_of(name)
    blk = np.array(cone_input(symb, "noisy"))
    s = max(1.0, norm_V(symb, blk))
    margin = 4 * K_BOUND * TOL * s
    B = on_device(symb, -blk)                                                 # far from the PSD matrices: most of it is cut off
    D = chordal.cone_project(B, cone="dual", tol=TOL)
    P = chordal.cone_project(cspmatrix(symb, -B.blkval), tol=TOL)
    assert torch.equal(D.blkval, B.blkval + P.blkval)                         # B + P_K(-B), bit for bit
    assert not D.blkval[torch.from_numpy(~lower_slots(symb)).cuda()].any()
    Dd, Pd = dense_of(symb, D.blkval.cpu().numpy()), dense_of(symb, P.blkval.cpu().numpy())
    assert np.linalg.eigvalsh(Dd)[0] >= -margin                               # PSD as a dense matrix
    assert abs((Pd * Dd).sum()) <= margin * s                                 # <P_K(A), P_K*(-A)> = 0 with A = -B


# ---- 5. honest stop ------------------------------------------------------------------------------------------------------------
def test_reaching_maxit_is_not_an_error():
    symb = symb_of("band")
    X, info = chordal.cone_project(on_device(symb, cone_input(symb, "indef")), maxit=16, return_info=True)
    h = info["hist"].cpu().numpy()
    s = max(1.0, norm_V(symb, cone_input(symb, "indef")))
    assert not info["converged"] and info["iterations"] == 16 and h.shape == (16, 4) and np.isfinite(h).all()
    assert abs(info["primal"] - math.sqrt(h[-1, 0]) / s) <= 1e-14 * info["primal"]
    assert abs(info["dual"] - math.sqrt(h[-1, 1]) / s) <= 1e-14 * info["dual"]
    assert max(info["primal"], info["dual"]) > TOL


# ---- 6. warm start -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nested", "rand1", "band"])
def test_warm_start_converges_at_the_first_or_second_look(name):
    symb = symb_of(name)
    A = on_device(symb, cone_input(symb, "noisy"))
    X, info = chordal.cone_project(A, tol=TOL, return_info=True)
    X2, info2 = chordal.cone_project(A, tol=TOL, U0=info["U"], return_info=True)
    assert info["iterations"] > 1 + chordal.CONE_CHUNK
    assert info2["converged"] and info2["iterations"] <= 1 + chordal.CONE_CHUNK
    s = max(1.0, norm_V(symb, cone_input(symb, "noisy")))
    assert norm_V(symb, (X2.blkval - X.blkval).cpu().numpy()) <= 8 * K_BOUND * TOL * s


# ---- 7. failure and hygiene --------------------------------------------------------------------------------------------------
def test_non_finite_entry_names_a_clique_that_holds_it():
    symb = symb_of("nested")
    bad = np.array(cone_input(symb, "noisy"))
    kb = leaf_clique(symb)
    bad[symb.blkptr[kb] + 1] = np.nan                                         # row 1, column 0 of the leaf's panel
    rows = clique_rows(symb, kb)
    holders = [k for k in range(symb.Nsn) if {rows[0], rows[1]} <= set(clique_rows(symb, k).tolist())]
    with pytest.raises(RuntimeError, match="did not converge") as e:
        chordal.cone_project(on_device(symb, bad))
    assert int(str(e.value).split("clique ")[1].split()[0]) in holders
    good = on_device(symb, cone_input(symb, "noisy"))
    assert chordal.cone_project(good, return_info=True)[1]["converged"]       # nothing is left behind for the next call


def test_unused_slots_are_ignored_and_calls_repeat_bit_for_bit():
    symb = symb_of("rand1")
    blk = np.array(cone_input(symb, "noisy"))
    A = on_device(symb, blk)
    X, info = chordal.cone_project(A, return_info=True)
    X2, info2 = chordal.cone_project(A, return_info=True)
    assert torch.equal(X.blkval, X2.blkval) and torch.equal(info["U"], info2["U"]) and torch.equal(info["hist"], info2["hist"])
    assert torch.equal(A.blkval.cpu(), torch.from_numpy(blk))                 # the input is not written
    dirty = blk.copy()
    dirty[~lower_slots(symb)] = np.nan
    X3, info3 = chordal.cone_project(on_device(symb, dirty), return_info=True)
    assert torch.equal(X.blkval, X3.blkval) and torch.equal(info["hist"], info3["hist"]) and info3["distance"] == info["distance"]


def test_device_bytes_grow_on_the_first_call_only():
    symb = Symbolic(PATS["fam_top"]())
    symb.device_init(0, 1)
    A = on_device(symb, cone_input(symb, "noisy"))
    b0 = symb.device_bytes()
    chordal.cone_project(A, maxit=3)
    torch.cuda.synchronize()
    b1 = symb.device_bytes()
    chordal.cone_project(A, maxit=3, return_info=True)
    torch.cuda.synchronize()
    assert b1 > b0 and symb.device_bytes() == b1
    symb._cache.pop("cone_weights", None)


def test_bad_arguments():
    symb = symb_of("arrow")
    A = on_device(symb, cone_input(symb, "noisy"))
    qlen = int(chordal.clique_ptr(symb)[-1])
    good = torch.zeros(qlen, dtype=torch.float64, device="cuda")
    for kw in ({"rho": 0.0}, {"rho": -1.0}, {"rho": math.nan}, {"relax": 0.0}, {"relax": 2.0}, {"relax": math.nan}, {"tol": -1e-9},
               {"maxit": 0}, {"cone": "polar"}, {"U0": good[:-1]}, {"U0": good.float()}, {"U0": good.cpu()}):
        with pytest.raises(ValueError):
            chordal.cone_project(A, **kw)
    rep = symb_of("arrow").replicate(2)
    with pytest.raises(NotImplementedError):
        chordal.cone_project(cspmatrix(rep, torch.zeros(rep.blklen, dtype=torch.float64, device="cuda")))
    L, h = _lib.lib(), symb.handle
    a, x, U, W = start(symb, cone_input(symb, "noisy"))
    hist = torch.zeros((4, 4), dtype=torch.float64, device="cuda")
    pa, px, pU, pW, ph = a.blkval.data_ptr(), x.blkval.data_ptr(), U.data_ptr(), W.data_ptr(), hist.data_ptr()
    call = lambda *p, rho=1.0, relax=1.7, it0=0, n=1: L.csp_cone_project_steps(h, p[0], p[1], p[2], p[3], rho, relax, it0, n, p[4], None)
    for i in range(5):
        p = [pa, px, pU, pW, ph]
        p[i] = None
        assert call(*p) == -1                                                 # null pointers
    last = lambda q, n: q + 8 * (n - 1)
    assert call(pa, last(pa, symb.blklen), pU, pW, ph) == -1                  # x in a
    assert call(pa, px, last(pa, symb.blklen), pW, ph) == -1                  # U in a
    assert call(pa, px, pU, last(pU, qlen), ph) == -1                         # W in U
    assert call(pa, px, pU, pW, last(px, symb.blklen)) == -1                  # hist in x
    assert call(pa, px, pU, pW, last(pW, qlen)) == -1                         # hist in W
    assert call(pa, px, pU, pW, last(pa, symb.blklen)) == -1                  # hist in a
    for kw in ({"rho": 0.0}, {"rho": math.nan}, {"relax": 0.0}, {"relax": 2.0}, {"n": 0}, {"it0": -1}):
        assert call(pa, px, pU, pW, ph, **kw) == -1
    assert call(pa, px, pU, pW, ph) == 0
    torch.cuda.synchronize()


def test_scipy_form():
    symb = symb_of("rand1")
    blk = np.array(cone_input(symb, "noisy"))
    Ad = dense_of(symb, blk)
    X, info = smcp_amd.cone_project(sp.csc_matrix(np.tril(Ad)), return_info=True)
    ref = reference("rand1", "noisy", tol=1e-12, maxit=5000, snapshots=(TOL,))
    assert info["converged"] and "hist" not in info and "U" not in info
    # the scipy form chooses its own elimination order: compared through the projection, which does not depend on it
    Xd = X.toarray()
    assert np.sqrt(((Xd - dense_of(symb, ref["x"])) ** 2).sum()) <= 4 * K_BOUND * TOL * ref["scale"]


# ---- 8. the launch chain -------------------------------------------------------------------------------------------------------
def test_launch_chain():
    symb = symb_of("nested")
    a, x, U, W = start(symb, cone_input(symb, "noisy"))
    hist = torch.zeros((9, 4), dtype=torch.float64, device="cuda")
    run_steps(symb, a, x, U, W, 1.0, 1.7, 0, 1, hist)                         # the workspace of the first call
    counts, census = launch_census(symb, lambda: run_steps(symb, a, x, U, W, 1.0, 1.7, 1, 8, hist))
    assert counts["k_ceig_reduce"] == 8 and counts["k_axpby"] == 8 and 8 <= counts["k_ceig"] <= 48
    assert counts["k_gather_level"] <= 8 * (2 * symb.nlev + 1)
    assert set(counts) == {"k_ceig_reduce", "k_axpby", "k_ceig", "k_gather_level"}
    # the kernels behind the four ids, per iteration: the gather of x, k_cone_split per slot class, the scatter of W per level,
    # k_cone_update, k_cone_resid
    assert census["k_cone_resid"] == 8 and census["k_cone_update"] == 8 and census["k_cone_split"] == counts["k_ceig"], census
    assert census["k_clique_scatter"] == 8 * symb.nlev and census["k_gather_level"] == counts["k_gather_level"] - 8 * symb.nlev, census
    assert set(census) == {"k_cone_resid", "k_cone_update", "k_cone_split", "k_clique_scatter", "k_gather_level"}, census
