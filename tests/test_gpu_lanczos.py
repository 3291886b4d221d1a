"""Lanczos on the dual cone on the device (smcp_amd.chordal.dual_max_step / dual_margin / lanczos_extremes and their scipy
forms in smcp_amd.base; csrc/front_lanczos.hip, csrc/lanczos.hip) against the dense definition on the host -- L (read back
from the device's ``cholesky``) and D expanded to dense, eigvalsh(L^-1 D L^-T) -- against the library's own cone test and
against their contract.  Inputs, the numpy restatement and the measured figures the bounds come from:
tests/test_lanczos_host.py.

Bounds: 16 x what the restatement reaches, RESTATEMENT_ERR = 0.5 n eps max|theta| on the Ritz values (measured 0.448 at most),
RESTATEMENT_ORTH = 0.005 n eps on max|V V^T - I| and RESTATEMENT_REC = 0.0015 n eps |op| on the three-term recurrence (measured
0.0039 and 0.0012 on arrow_big); the planted cases may take one chunk of eight steps more than the restatement's 16, 8 and 16.

Measured on one MI355X, same units: Ritz values at full Krylov dimension at most 0.236 (arrow, pencil form), planted cases at
most 0.0068 in 16, 8 and 16 steps; max|V V^T - I| at most 0.0045 n eps, the recurrence at most 0.0011 n eps |op| (j = 1, 8, 64,
65, 80); k_lz_ritz alone within 9.8 eps |T| of eigh_tridiagonal."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from helpers import GPU_PATTERNS, launch_census, launch_counts, padded
from smcp_amd import _lib, base, chordal, problems
from smcp_amd.cspmatrix import _stream, cspmatrix
from smcp_amd.symbolic import Symbolic
from test_lanczos_host import (DEF_STEPS, EPS, FULL, GPU_FACTOR, PLANTED, PLANTED_MAXIT, PLANTED_TOL, RESTATEMENT_ERR,
                               RESTATEMENT_ORTH, RESTATEMENT_REC, RESTATEMENT_STEPS, definition_errors, dense_factor,
                               dense_operator, full_case, planted_case, ritz_extremes, tridiagonal_cases, tridiagonal_reference)

pytestmark = pytest.mark.gpu

_SYMB, _FACTOR, WORST = {}, {}, {"ritz": 0.0, "orth": 0.0, "rec": 0.0}


def device_symb(name):
    if name not in _SYMB:
        _SYMB[name] = Symbolic(GPU_PATTERNS[name]())
        _SYMB[name].device_init(0, 1)
    return _SYMB[name]


def on_device(symb, blk):
    return cspmatrix(symb, torch.from_numpy(np.ascontiguousarray(blk).copy()).cuda())


def factored(kind, name):
    """(symb, L on the device, its dense form, blkS, Sd, blkD, Dd) of a case: factored once, never changed"""
    if (kind, name) not in _FACTOR:
        _, blkS, Sd, blkD, Dd = (full_case if kind == "full" else planted_case)(name)
        symb = device_symb(name)
        L = on_device(symb, blkS)
        chordal.cholesky(L)
        _FACTOR[(kind, name)] = (symb, L, dense_factor(symb, L.blkval.cpu().numpy()), blkS, Sd, blkD, Dd)
    return _FACTOR[(kind, name)]


def ritz_bound(n, ref):
    return GPU_FACTOR * RESTATEMENT_ERR * n * EPS * np.abs(ref).max()


def note(key, value, capsys, what):
    WORST[key] = max(WORST[key], value)
    with capsys.disabled():
        print("\n%s (worst so far %.4f)" % (what, WORST[key]))


# ---- 1. full Krylov dimension --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FULL)
def test_full_krylov_both_forms(name, capsys):
    symb, L, Ld, blkS, Sd, blkD, Dd = factored("full", name)
    n = symb.n
    assert n <= chordal.LANCZOS_JMAX                 # maxit = n is not clamped (rand2 has n = 65, the others less)
    D = on_device(symb, blkD)
    ref = np.linalg.eigvalsh(dense_operator(Ld, Dd))
    bound = ritz_bound(n, ref)
    alpha, info = chordal.dual_max_step(L, D, tol=0.0, maxit=n, return_info=True)      # tol = 0: all n steps are taken
    e = max(abs(info["theta_min"] - ref[0]), abs(info["theta_max"] - ref[-1]))
    note("ritz", e / (n * EPS * np.abs(ref).max()), capsys, "%s pencil: %.3f n eps max|theta|, %d steps, invariant %s"
         % (name, e / (n * EPS * np.abs(ref).max()), info["steps"], info["invariant"]))
    assert e <= bound
    assert info["converged"] and (info["steps"] == n or info["invariant"])
    assert ref[0] < 0 and alpha == -1.0 / info["theta_min"] and abs(-1.0 / alpha - ref[0]) <= bound
    assert info["alpha_safe"] <= alpha
    if name == "diag":                               # every clique is 1 x 1: the answer is min d_i / s_i
        assert abs(info["theta_min"] - (np.diag(Dd) / np.diag(Sd)).min()) <= bound
    refi = np.linalg.eigvalsh(dense_operator(Ld))
    boundi = ritz_bound(n, refi)
    margin, infi = chordal.dual_margin(L, tol=0.0, maxit=n, return_info=True)
    e = max(abs(infi["theta_min"] - refi[0]), abs(infi["theta_max"] - refi[-1]))
    note("ritz", e / (n * EPS * refi[-1]), capsys, "%s inverse: %.3f n eps max|theta|, %d steps" % (name, e / (n * EPS * refi[-1]), infi["steps"]))
    assert e <= boundi and infi["converged"] and (infi["steps"] == n or infi["invariant"])
    assert margin == 1.0 / infi["theta_max"] and infi["cond"] == infi["theta_max"] / infi["theta_min"]
    # against eigvalsh(S)[0]: the bound of theta_max carried over to 1 / theta_max, plus the reference's own n eps |S|
    lam = np.linalg.eigvalsh(Ld @ Ld.T)
    assert abs(margin - lam[0]) <= boundi * margin * margin + n * EPS * lam[-1]
    assert abs(margin - np.linalg.eigvalsh(Sd)[0]) <= boundi * margin * margin + 4 * n * EPS * lam[-1]   # (and the factor's backward error)


# ---- 2. converged before the Krylov space is exhausted -------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PLANTED))
def test_planted_eigenvalue_converges_early(name, capsys):
    symb, L, Ld, blkS, Sd, blkD, Dd = factored("planted", name)
    n = symb.n
    D = on_device(symb, blkD)
    ref = np.linalg.eigvalsh(dense_operator(Ld, Dd))
    alpha, info = chordal.dual_max_step(L, D, tol=PLANTED_TOL, maxit=PLANTED_MAXIT, return_info=True)
    e = abs(info["theta_min"] - ref[0]) / (n * EPS * np.abs(ref).max())
    note("ritz", e, capsys, "%s planted: %.4f n eps max|theta|, %d steps (restatement %d)" % (name, e, info["steps"], RESTATEMENT_STEPS[name]))
    assert e <= GPU_FACTOR * RESTATEMENT_ERR
    assert info["converged"] and not info["invariant"]
    assert info["steps"] <= RESTATEMENT_STEPS[name] + chordal.LANCZOS_CHUNK
    assert 0 < alpha < math.inf
    chordal.cholesky(on_device(symb, blkS + (1 - 1e-6) * alpha * blkD))     # the library's own cone test agrees
    with pytest.raises(ArithmeticError):
        chordal.cholesky(on_device(symb, blkS + (1 + 1e-6) * alpha * blkD))


# ---- 3. what holds before convergence; the kernels at definition level ---------------------------------------------------
def read_back(info, n):
    """(V (m + 1 rows), alpha (m), beta (m + 1)) from the workspace of a lanczos_extremes(return_work=True)"""
    m, jmax = info["steps"], info["jmax"]
    state, basis, ld, total = chordal.lanczos_layout(n, jmax)
    w = info["work"].cpu().numpy()
    V = w[basis:basis + (m + 1) * ld].reshape(m + 1, ld)[:, :n]
    return V, w[16:16 + m], w[16 + jmax:16 + jmax + m + 1]


@pytest.mark.parametrize("maxit", [8, 80])
def test_unconverged_ritz_values_stay_inside_the_spectrum(maxit):
    symb, L, Ld, blkS, Sd, blkD, Dd = factored("full", "arrow_big")
    n = symb.n
    D = on_device(symb, blkD)
    M = dense_operator(Ld, Dd)
    ref = np.linalg.eigvalsh(M)
    bound = ritz_bound(n, ref)
    for tol in (0.0, 1e-10):                         # tol = 0: every step is taken
        info = chordal.lanczos_extremes(L, D, tol=tol, maxit=maxit, return_work=True)
        assert info["theta_min"] >= ref[0] - bound and info["theta_max"] <= ref[-1] + bound
        assert info["steps"] == maxit or tol > 0
        # `converged` is honest: the residual of the Ritz pair, computed here from the basis read back
        V, al, be = read_back(info, n)
        m = info["steps"]
        wT, Z = tridiagonal_reference(al, np.append(be[1:m], be[m]))
        y = V[:m].T @ Z[:, 0]
        true_res = np.linalg.norm(M @ y - wT[0] * y)
        scale = max(abs(info["theta_min"]), abs(info["theta_max"]))
        floor = GPU_FACTOR * RESTATEMENT_REC * n * EPS * np.abs(ref).max() * math.sqrt(n * m)
        assert info["resid_min"] <= 2 * true_res + floor and true_res <= 2 * info["resid_min"] + floor
        assert info["converged"] == (info["resid_min"] <= tol * scale)
        if info["converged"]:
            assert true_res <= 2 * tol * scale + floor


@pytest.mark.parametrize("j", DEF_STEPS)
def test_basis_and_recurrence_at_definition_level(j, capsys):
    symb, L, Ld, blkS, Sd, blkD, Dd = factored("full", "arrow_big")
    n = symb.n
    info = chordal.lanczos_extremes(L, on_device(symb, blkD), tol=0.0, maxit=j, return_work=True)
    assert info["steps"] == j and not info["invariant"]
    V, al, be = read_back(info, n)
    orth, rec = definition_errors(dense_operator(Ld, Dd), V, al, be)
    note("orth", orth, capsys, "j = %d: max|V V^T - I| = %.5f n eps" % (j, orth))
    note("rec", rec, capsys, "j = %d: recurrence %.5f n eps |op|" % (j, rec))
    assert orth <= GPU_FACTOR * RESTATEMENT_ORTH
    assert rec <= GPU_FACTOR * RESTATEMENT_REC
    # and the Ritz values the device extracted are those of the (alpha, beta) it stored
    tmin, rmin, tmax, rmax = ritz_extremes(al, be[1:j], be[j])
    tn = max(abs(tmin), abs(tmax))
    assert abs(info["theta_min"] - tmin) <= 16 * j * EPS * tn and abs(info["theta_max"] - tmax) <= 16 * j * EPS * tn


# ---- 4. csp_lanczos_ritz alone -------------------------------------------------------------------------------------------
def run_ritz(symb, alpha, beta):
    """the four outputs of csp_lanczos_ritz for uploaded alpha_0 .. alpha_{m-1}, beta_1 .. beta_m"""
    m, n = len(alpha), symb.n
    total = chordal.lanczos_layout(n, m)[3]
    w = np.zeros(total)
    w[1] = m
    w[16:16 + m] = alpha
    w[16 + m + 1:16 + 2 * m + 1] = beta
    work = torch.from_numpy(w).cuda()
    assert _lib.lib().csp_lanczos_ritz(symb.handle, work.data_ptr(), m, _stream()) == 0
    return work[4:8].cpu().numpy()


@pytest.mark.parametrize("case", sorted(tridiagonal_cases()))
def test_ritz_kernel_against_eigh_tridiagonal(case, capsys):
    symb = device_symb("band")
    alpha, beta = tridiagonal_cases()[case]
    m = len(alpha)
    out = run_ritz(symb, alpha, beta)
    assert (out == run_ritz(symb, alpha, beta)).all()                       # the same bits for the same input
    w, Z = tridiagonal_reference(alpha, beta)
    if m == 1:
        assert out[0] == alpha[0] and out[2] == alpha[0] and out[1] == beta[0] and out[3] == beta[0]
        return
    tn = np.abs(w).max()
    with capsys.disabled():
        print("\n%s: extremes off by %.2f, %.2f eps |T|" % (case, abs(out[0] - w[0]) / (EPS * tn), abs(out[2] - w[-1]) / (EPS * tn)))
    assert abs(out[0] - w[0]) <= 16 * m * EPS * tn and abs(out[2] - w[-1]) <= 16 * m * EPS * tn
    # the bottom component is known to m eps |T| / gap (perturbation of the eigenvector): with gap > 1e-3 |T| that is the floor
    floor = abs(beta[-1]) * 16 * m * EPS * 1e3
    for est, col, gap in ((out[1], 0, w[1] - w[0]), (out[3], m - 1, w[-1] - w[-2])):
        if gap > 1e-3 * tn:
            r = abs(beta[-1] * Z[-1, col])
            assert est <= 2 * r + floor and r <= 2 * est + floor, (case, col, est, r)


# ---- 5. edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["band", "arrow", "diag", "dense"])
def test_directions_along_s(name):
    symb, L, Ld, blkS, Sd, blkD, Dd = factored("full", name)
    n = symb.n
    alpha, info = chordal.dual_max_step(L, on_device(symb, -blkS), return_info=True)
    assert info["invariant"] and info["steps"] == 1 and info["converged"]    # L^-1 (-S) L^-T = -I: breakdown at the first step
    assert abs(info["theta_min"] + 1.0) <= GPU_FACTOR * RESTATEMENT_ERR * n * EPS
    assert abs(alpha - 1.0) <= 2 * GPU_FACTOR * RESTATEMENT_ERR * n * EPS
    assert chordal.dual_max_step(L, on_device(symb, blkS)) == math.inf
    alpha, info = chordal.dual_max_step(L, on_device(symb, 0.0 * blkS), return_info=True)
    assert alpha == math.inf and info["invariant"] and info["theta_min"] == 0.0 and info["alpha_safe"] == math.inf


def test_start_vector_of_the_caller():
    symb, L, Ld, blkS, Sd, blkD, Dd = factored("full", "diag")               # n = 15: less than one slab, no multiple of anything
    n = symb.n
    D = on_device(symb, blkD)
    ref = np.linalg.eigvalsh(dense_operator(Ld, Dd))
    v0 = np.random.default_rng(77).standard_normal(n)
    a = chordal.lanczos_extremes(L, D, maxit=n, v0=v0)
    b = chordal.lanczos_extremes(L, D, maxit=n, v0=torch.from_numpy(v0).cuda())
    c = chordal.lanczos_extremes(L, D, maxit=n)
    assert a == b and a != c
    assert abs(a["theta_min"] - ref[0]) <= ritz_bound(n, ref) and abs(a["theta_max"] - ref[-1]) <= ritz_bound(n, ref)
    with pytest.raises(ValueError):
        chordal.lanczos_extremes(L, D, v0=np.ones(n + 1))


def test_mismatched_symbolics():
    symb, L, *_ = factored("full", "arrow")
    s2 = Symbolic(GPU_PATTERNS["arrow"]())
    s2.device_init(0, 1)
    D2 = on_device(s2, full_case("arrow")[3])
    with pytest.raises(ValueError):
        chordal.dual_max_step(L, D2)
    with pytest.raises(ValueError):
        chordal.lanczos_extremes(L, D2)


def test_padded_workspace_and_the_c_abi_rules():
    symb, L, Ld, blkS, Sd, blkD, Dd = factored("full", "diag")
    n, jmax, pad = symb.n, 15, 37
    D = on_device(symb, blkD)
    lib = _lib.lib()
    state, basis, ld, total = chordal.lanczos_layout(n, jmax)
    assert lib.csp_lanczos_work_len(n, jmax) == total and lib.csp_lanczos_work_len(n, 0) == -1
    assert lib.csp_lanczos_work_len(n, 129) == -1 and lib.csp_lanczos_work_len(n, 128) > 0
    view, full = padded(np.zeros((total, 1)), pad)
    view.fill_(7.25)                                                           # nothing may depend on what the workspace held
    work = full[0]
    work[basis:basis + n].copy_(torch.from_numpy(chordal.lanczos_default_v0(n)))
    h, Lp, Dp, wp = symb.handle, L.blkval.data_ptr(), D.blkval.data_ptr(), work.data_ptr()
    assert lib.csp_lanczos_steps(h, Lp, Dp, wp, jmax, 0, 8, _stream()) == 0
    assert lib.csp_lanczos_ritz(h, wp, jmax, _stream()) == 0
    w = work.cpu().numpy()
    assert (w[total:] == 7.25).all() and len(w) == total + pad
    rows = w[basis:total].reshape(jmax + 3, ld)
    assert (rows[:, n:] == 7.25).all()                                         # entries n .. ld of every row
    assert (rows[9:jmax + 1] == 7.25).all()                                    # basis rows beyond v_8 are not written yet
    assert np.isfinite(rows[:9, :n]).all()
    ref = chordal.lanczos_extremes(L, D, tol=0.0, maxit=8)                     # the same eight steps from a zeroed workspace
    assert [w[4], w[5], w[6], w[7]] == [ref[k] for k in ("theta_min", "resid_min", "theta_max", "resid_max")]
    assert lib.csp_lanczos_steps(h, Lp, Dp, wp, jmax, 8, 8, _stream()) == -1  # beyond jmax
    assert lib.csp_lanczos_steps(h, Lp, Dp, wp, 129, 0, 1, _stream()) == -1
    assert lib.csp_lanczos_steps(h, None, Dp, wp, jmax, 0, 1, _stream()) == -1
    assert lib.csp_lanczos_steps(h, Lp, Dp, None, jmax, 0, 1, _stream()) == -1
    assert lib.csp_lanczos_ritz(h, None, jmax, _stream()) == -1
    torch.cuda.synchronize()


# ---- 6. contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rand2", "arrow_big"])
def test_inputs_untouched_and_bits_repeat(name):
    symb, L, Ld, blkS, Sd, blkD, Dd = factored("full", name)
    D = on_device(symb, blkD)
    L0, D0 = L.blkval.clone(), D.blkval.clone()
    a1, i1 = chordal.dual_max_step(L, D, maxit=24, return_info=True)
    a2, i2 = chordal.dual_max_step(L, D, maxit=24, return_info=True)
    m1, j1 = chordal.dual_margin(L, maxit=24, return_info=True)
    m2, j2 = chordal.dual_margin(L, maxit=24, return_info=True)
    assert a1 == a2 and i1 == i2 and m1 == m2 and j1 == j2
    assert torch.equal(L.blkval, L0) and torch.equal(D.blkval, D0)


@pytest.mark.parametrize("pencil", [True, False])
def test_launch_counts(pencil):
    symb, L, Ld, blkS, Sd, blkD, Dd = factored("full", "arrow_big")
    D = on_device(symb, blkD) if pencil else None
    info = chordal.lanczos_extremes(L, D, tol=0.0, maxit=32, return_work=True)    # a filled workspace; buffers of the first call
    lib = _lib.lib()
    h, Lp, Dp, wp, jmax = symb.handle, L.blkval.data_ptr(), None if D is None else D.blkval.data_ptr(), info["work"].data_ptr(), info["jmax"]
    one = launch_counts(symb, lambda: lib.csp_lanczos_steps(h, Lp, Dp, wp, jmax, 8, 1, _stream()))
    eight = launch_counts(symb, lambda: lib.csp_lanczos_steps(h, Lp, Dp, wp, jmax, 8, 8, _stream()))
    later = launch_counts(symb, lambda: lib.csp_lanczos_steps(h, Lp, Dp, wp, jmax, 24, 8, _stream()))
    ritz = launch_counts(symb, lambda: lib.csp_lanczos_ritz(h, wp, jmax, _stream()))
    assert one["k_vec_axpby"] == 7                                       # copy, dots, update, dots, update, finish, scale
    assert eight == {k: 8 * v for k, v in one.items()} and later == eight    # eight steps, whatever j
    assert ritz == {"k_qr_small": 1}
    assert set(one) <= {"k_vec_axpby", "k_trsm_fwd_level", "k_trsm_bwd_level", "k_symm_fma", "k_symm_mm", "k_symm_combine"}
    assert ("k_symm_combine" in one) == pencil
    first = launch_counts(symb, lambda: lib.csp_lanczos_steps(h, Lp, Dp, wp, jmax, 0, 1, _stream()))
    assert first["k_vec_axpby"] == 7 + 3                                 # the start vector is normalised at j0 = 0
    # the kernels behind k_vec_axpby and k_qr_small, by name (the launch census)
    lz = lambda census: {k: v for k, v in census.items() if k.startswith("k_lz_")}
    counts, census = launch_census(symb, lambda: lib.csp_lanczos_steps(h, Lp, Dp, wp, jmax, 8, 1, _stream()))
    assert counts == one and lz(census) == {"k_lz_copy": 1, "k_lz_dots": 2, "k_lz_update": 2, "k_lz_finish": 1, "k_lz_scale": 1}, census
    assert "k_vec_axpby" not in census and "k_vec_axpby_parts" not in census, census
    assert launch_census(symb, lambda: lib.csp_lanczos_ritz(h, wp, jmax, _stream()))[1] == {"k_lz_ritz": 1}
    census = launch_census(symb, lambda: lib.csp_lanczos_steps(h, Lp, Dp, wp, jmax, 0, 1, _stream()))[1]
    assert sum(lz(census).values()) == 7 + 3 and set(lz(census)) == {"k_lz_copy", "k_lz_dots", "k_lz_update", "k_lz_finish", "k_lz_scale"}, census


# ---- the scipy forms -----------------------------------------------------------------------------------------------------
def test_scipy_forms():
    cyc = sp.coo_matrix((np.ones(4), ([1, 2, 3, 3], [0, 1, 2, 0])), shape=(4, 4)) + 4.0 * sp.identity(4)
    with pytest.raises(ValueError):
        base.dual_max_step(cyc, cyc)
    with pytest.raises(ValueError):
        base.dual_margin(cyc)
    s0 = Symbolic(problems.random_chordal_pattern(20, max_nn=5, max_na=7, seed=9))
    n = s0.n
    cp, ri = s0.sparsity_pattern()
    rng = np.random.default_rng(3)
    J = np.repeat(np.arange(n), np.diff(cp))
    I = np.asarray(ri)
    Lf = sp.csc_matrix((rng.standard_normal(len(I)) * 0.4 + (I == J) * 2.0, (I, J)), shape=(n, n)).toarray()
    Sd = Lf @ Lf.T                                   # on the pattern: no fill in this order
    Dv = rng.standard_normal(len(I))
    Dd = sp.coo_matrix((Dv, (I, J)), shape=(n, n)).toarray()
    Dd = Dd + np.tril(Dd, -1).T
    Ld = np.linalg.cholesky(Sd)
    ref = np.linalg.eigvalsh(dense_operator(Ld, Dd))
    S0 = sp.coo_matrix((Sd[I, J], (I, J)), shape=(n, n))
    D0 = sp.coo_matrix((Dv, (I, J)), shape=(n, n))
    q = rng.permutation(n)
    a, b = q[I], q[J]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    Ss = sp.coo_matrix((Sd[I, J], (lo, hi)), shape=(n, n))                    # relabelled, upper triangle
    Ds = sp.coo_matrix((Dv, (lo, hi)), shape=(n, n))
    # (the factor is the device's own: its backward error reaches theta through cond(S))
    tol = ritz_bound(n, ref) * np.linalg.cond(Sd)
    for Sx, Dx in ((S0, D0), (Ss, Ds)):
        alpha = base.dual_max_step(Sx, Dx, maxit=n)
        assert abs(-1.0 / alpha - ref[0]) <= tol
        lam = np.linalg.eigvalsh(Sd)
        assert abs(base.dual_margin(Sx, maxit=n) - lam[0]) <= 16 * n * EPS * lam[-1]
    with pytest.raises(ArithmeticError):
        base.dual_max_step(sp.coo_matrix((-Sd[I, J], (I, J)), shape=(n, n)), D0)
    with pytest.raises(ArithmeticError):
        base.dual_margin(sp.coo_matrix((-Sd[I, J], (I, J)), shape=(n, n)))
