"""Lanczos on the dual cone (smcp_amd.chordal.dual_max_step / dual_margin / lanczos_extremes, csrc/front_lanczos.hip): the
iteration restated in numpy, the inputs and dense references of the GPU tests, and the plain-Python rules of the driver
(no GPU needed; tests/test_gpu_lanczos.py imports this file).

The restatement takes the same steps as the device: the operator on v_j, classical Gram-Schmidt twice against v_0 .. v_j,
alpha_j = c_j of pass one + c_j of pass two, beta_{j+1} = |w|, breakdown when beta_{j+1} <= n eps max(|alpha|, beta seen so far),
v_{j+1} = w (1 / beta_{j+1}); the Ritz values through scipy.linalg.eigh_tridiagonal, the residual estimates
beta_m |bottom component|; the driver looks at them every eight steps.

Measured here (numpy, this file's inputs), in units of n eps max|theta| unless said otherwise:
  * Ritz values at full Krylov dimension against eigvalsh of the dense operator, both operator forms, all full-Krylov cases:
    at most 0.448 (dense, inverse form); the planted cases at convergence: at most 0.017.  RESTATEMENT_ERR = 0.5 is asserted
    here, the GPU bound is 16 x that.
  * steps to tol = 1e-12 of the planted cases (the driver looks every eight): arrow_big 16, nested_mid 8, fam_odd 16
    (RESTATEMENT_STEPS); the GPU may take one chunk of eight more.
  * on arrow_big (n = 896) at j = 1, 8, 64, 65, 80: max|V V^T - I| <= 0.0039 n eps (3.5 eps) and
    |op V_j - V_j T_j - beta_j v_{j+1} e_j^T|_max <= 0.0012 n eps |op|.  RESTATEMENT_ORTH = 0.005 and RESTATEMENT_REC = 0.0015
    are asserted here, the GPU bounds are 16 x those.
  * D = -S: beta_1 is 0.3 .. 2.3 eps on the small patterns (the rounding of the two solves and the product), so a threshold
    of eps (j + 1) max(|alpha|, beta) would call the breakdown on some patterns and miss it on others; the rule is n eps.
"""
import math

import numpy as np
import pytest
import scipy.linalg

from helpers import PATTERNS, random_spd_on_V, symb_of
from smcp_amd.chordal import (LANCZOS_CHUNK, LANCZOS_JMAX, dual_margin, dual_max_step, lanczos_chunks,  # noqa: F401
                              lanczos_converged, lanczos_default_v0, lanczos_extremes, lanczos_layout, lanczos_maxit)
from test_mrcompletion_host import blkval_of, dense_of

EPS = np.finfo(np.float64).eps
RESTATEMENT_ERR = 0.5        # units of n eps max|theta|: what the restatement must reach; the GPU gets 16 x
RESTATEMENT_ORTH = 0.005      # units of n eps: max|V V^T - I|
RESTATEMENT_REC = 0.0015      # units of n eps |op|: the three-term recurrence
GPU_FACTOR = 16.0
FULL = ["band", "arrow", "nested", "rand1", "rand2", "dense", "diag"]
PLANTED = {"arrow_big": (4.0, 0.02), "nested_mid": (4.0, 0.02), "fam_odd": (4.0, 0.02)}     # name -> (gamma, t) of planted()
PLANTED_TOL, PLANTED_MAXIT = 1e-12, 40
RESTATEMENT_STEPS = {"arrow_big": 16, "nested_mid": 8, "fam_odd": 16}   # chunks of eight: where the driver stops
DEF_STEPS = (1, 8, 64, 65, 80)


# ---- dense definitions ---------------------------------------------------------------------------------------------------
class _OnV:
    """what helpers.random_spd_on_V asks of a pattern"""

    def __init__(self, symb):
        self.n = symb.n
        self._mask = dense_of(symb, np.ones(symb.blklen)) != 0

    def mask(self):
        return self._mask


def spd_on_V(symb, seed):
    """(blkval of S, dense S) for S = helpers.random_spd_on_V"""
    Sd, _ = random_spd_on_V(_OnV(symb), seed)
    return blkval_of(symb, Sd), Sd


def normal_on_V(symb, seed):
    """(blkval, dense) of a symmetric matrix with standard normal entries on V"""
    blk = np.random.default_rng(seed).standard_normal(symb.blklen)
    Dd = dense_of(symb, blk)
    return blkval_of(symb, Dd), Dd


def planted(symb, Sd, gamma, t, seed):
    """(blkval, dense, i) of D = -S - g e_i e_i^T + t R with R normal on V.  L^-1 D L^-T = -I - g y y^T + t M with y = L^-1 e_i,
    |y|^2 = (S^-1)_ii, and M = L^-1 R L^-T; g = gamma t |M|_2 / (S^-1)_ii puts the planted eigenvalue gamma times the spread
    of t M below the rest.  On the large patterns cond(S) is 1e10 to 1e13 and |M|_2 about 1e10: t M, not -I, sets the scale of
    the spectrum, which keeps the rounding of the operator itself below n eps max|theta|.  The binding direction of S + alpha D
    is close to x = S^-1 e_i, whose Rayleigh quotient in S is q_i = (S^-1)_ii / (S^-2)_ii; i is the index with the largest
    q_i: where a Cholesky factorisation has the best chance to tell (1 - 1e-6) alpha from (1 + 1e-6) alpha."""
    Si = np.linalg.inv(Sd)
    i = int(np.argmax(np.diag(Si) / (Si * Si).sum(axis=0)))
    Rd = normal_on_V(symb, seed)[1]
    Ld = np.linalg.cholesky(Sd)
    spread = t * np.abs(np.linalg.eigvalsh(dense_operator(Ld, Rd))).max()
    Dd = -Sd + t * Rd
    Dd[i, i] -= gamma * spread / Si[i, i]
    return blkval_of(symb, Dd), Dd, i


def dense_factor(symb, blkL):
    """the dense lower-triangular factor held in blkL"""
    return np.tril(dense_of(symb, blkL))


def dense_operator(Ld, Dd=None):
    """L^-1 D L^-T, or L^-T L^-1 without D, symmetrised"""
    if Dd is None:
        Li = scipy.linalg.solve_triangular(Ld, np.eye(Ld.shape[0]), lower=True)
        M = Li.T @ Li
    else:
        Y = scipy.linalg.solve_triangular(Ld, Dd, lower=True)
        M = scipy.linalg.solve_triangular(Ld, Y.T, lower=True).T
    return 0.5 * (M + M.T)


def apply_operator(Ld, Dd=None):
    """v -> op v by the device's sequence of solves and one product"""
    if Dd is None:
        return lambda v: scipy.linalg.solve_triangular(Ld, scipy.linalg.solve_triangular(Ld, v, lower=True), lower=True, trans="T")
    return lambda v: scipy.linalg.solve_triangular(Ld, Dd @ scipy.linalg.solve_triangular(Ld, v, lower=True, trans="T"), lower=True)


# ---- the restatement -----------------------------------------------------------------------------------------------------
def lanczos_restatement(op, v0, steps):
    """k_lz_dots / k_lz_update / k_lz_finish / k_lz_scale in numpy: dict with alpha (m), beta (m + 1, beta[0] = |v0|), V
    (m + 1 rows; the last one zeros after a breakdown), steps = m, invariant."""
    v0 = np.asarray(v0, dtype=np.float64)
    n = len(v0)
    b0 = np.sqrt(v0 @ v0)
    V = [v0 * (1.0 / b0)]
    alpha, beta, seen, invariant = [], [b0], 0.0, False
    for j in range(steps):
        w = op(V[j])
        B = np.array(V)
        c1 = B @ w
        w = w - B.T @ c1
        c2 = B @ w
        w = w - B.T @ c2
        al, be = c1[j] + c2[j], np.sqrt(w @ w)
        alpha.append(al)
        beta.append(be)
        seen = max(seen, abs(al))
        if be <= EPS * n * seen:
            invariant = True
            V.append(np.zeros(n))
            break
        seen = max(seen, be)
        V.append(w * (1.0 / be))
    return {"alpha": np.array(alpha), "beta": np.array(beta), "V": np.array(V), "steps": len(alpha), "invariant": invariant}


def ritz_extremes(alpha, beta_off, beta_last):
    """(theta_min, resid_min, theta_max, resid_max) of the tridiagonal with diagonal alpha and off-diagonal beta_off"""
    if len(alpha) == 1:
        return alpha[0], abs(beta_last), alpha[0], abs(beta_last)
    w, Z = scipy.linalg.eigh_tridiagonal(alpha, beta_off)
    return w[0], abs(beta_last * Z[-1, 0]), w[-1], abs(beta_last * Z[-1, -1])


def driver_restatement(op, v0, tol=1e-10, maxit=64, which="min"):
    """chordal.lanczos_extremes on the restatement: chunks of eight steps, the stopping rule after each"""
    n = len(v0)
    jmax = lanczos_maxit(n, maxit)
    run = lanczos_restatement(op, v0, jmax)
    info = None
    for j0, ns in lanczos_chunks(jmax):
        m = min(j0 + ns, run["steps"])
        inv = run["invariant"] and m == run["steps"]
        tmin, rmin, tmax, rmax = ritz_extremes(run["alpha"][:m], run["beta"][1:m], run["beta"][m])
        info = {"theta_min": tmin, "resid_min": rmin, "theta_max": tmax, "resid_max": rmax, "steps": m, "invariant": inv}
        info["converged"] = lanczos_converged(rmax if which == "max" else rmin, tmin, tmax, tol, m, n, inv)
        if info["converged"]:
            break
    return info


def units(err, n, scale):
    return err / (n * EPS * scale)


# ---- the cases of the GPU tests (made once) ------------------------------------------------------------------------------
_CASES = {}


def pattern_symb(name):
    return symb_of(name)                             # host only


def full_case(name):
    """(symb, blkS, Sd, blkD, Dd) of a full-Krylov case"""
    if ("full", name) not in _CASES:
        symb = pattern_symb(name)
        blkS, Sd = spd_on_V(symb, 3)
        blkD, Dd = normal_on_V(symb, 4)
        _CASES[("full", name)] = (symb, blkS, Sd, blkD, Dd)
    return _CASES[("full", name)]


def planted_case(name):
    if ("planted", name) not in _CASES:
        symb = pattern_symb(name)
        blkS, Sd = spd_on_V(symb, 5)
        blkD, Dd, _ = planted(symb, Sd, PLANTED[name][0], PLANTED[name][1], 6)
        _CASES[("planted", name)] = (symb, blkS, Sd, blkD, Dd)
    return _CASES[("planted", name)]


def tridiagonal_cases():
    """name -> (alpha, beta_1 .. beta_m): the inputs of csp_lanczos_ritz alone"""
    out = {}
    for m in (1, 2, 3, 63, 64, 65, 128):
        rng = np.random.default_rng(100 + m)
        out["random%d" % m] = (rng.standard_normal(m), np.abs(rng.standard_normal(m)) + 0.1)
        out["constdiag%d" % m] = (np.full(m, 2.0), np.full(m, 1.0))
    out["wilkinson21"] = (np.abs(np.arange(21) - 10.0), np.ones(21))
    a, b = np.random.default_rng(7).standard_normal(64), np.abs(np.random.default_rng(8).standard_normal(64)) + 0.1
    b[31] = 0.0                                      # beta_32 = 0: T is two blocks
    out["zerobeta64"] = (a, b)
    return out


def tridiagonal_reference(alpha, beta):
    """(w, Z) of T (beta[:-1] off the diagonal; beta[-1] is the residual beta_m)"""
    if len(alpha) == 1:
        return np.array(alpha), np.ones((1, 1))
    return scipy.linalg.eigh_tridiagonal(alpha, beta[:-1])


# ---- tests ---------------------------------------------------------------------------------------------------------------
def check_full(Ld, Dd, n, seen):
    M = dense_operator(Ld, Dd)
    ref = np.linalg.eigvalsh(M)
    run = lanczos_restatement(apply_operator(Ld, Dd), lanczos_default_v0(n), n)
    m = run["steps"]
    assert m == n or run["invariant"]
    tmin, rmin, tmax, rmax = ritz_extremes(run["alpha"], run["beta"][1:m], run["beta"][m])
    scale = np.abs(ref).max()
    e = max(units(abs(tmin - ref[0]), n, scale), units(abs(tmax - ref[-1]), n, scale))
    seen.append(e)
    assert e <= RESTATEMENT_ERR, e


@pytest.mark.parametrize("name", sorted(set(PATTERNS) | set(FULL)))
def test_restatement_meets_eigvalsh_at_full_dimension(name, capsys):
    symb, blkS, Sd, blkD, Dd = full_case(name)
    assert symb.n <= LANCZOS_JMAX                   # full Krylov dimension is reachable (rand2 has n = 65, the others less)
    Ld = np.linalg.cholesky(Sd)
    seen = []
    check_full(Ld, Dd, symb.n, seen)
    check_full(Ld, None, symb.n, seen)
    with capsys.disabled():
        print("\n%s (n = %d): pencil %.3f, inverse %.3f n eps max|theta|" % (name, symb.n, seen[0], seen[1]))


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_planted_cases_converge_in_the_restatement(name, capsys):
    symb, blkS, Sd, blkD, Dd = planted_case(name)
    Ld = np.linalg.cholesky(Sd)
    ref = np.linalg.eigvalsh(dense_operator(Ld, Dd))
    info = driver_restatement(apply_operator(Ld, Dd), lanczos_default_v0(symb.n), PLANTED_TOL, PLANTED_MAXIT)
    e = units(abs(info["theta_min"] - ref[0]), symb.n, np.abs(ref).max())
    with capsys.disabled():
        print("\n%s (n = %d): %d steps, error %.5f n eps max|theta|, gap %.3g, spread %.3g"
              % (name, symb.n, info["steps"], e, ref[1] - ref[0], ref[-1] - ref[1]))
    assert info["converged"] and not info["invariant"] and info["steps"] <= PLANTED_MAXIT
    assert info["steps"] == RESTATEMENT_STEPS[name]
    assert e <= RESTATEMENT_ERR
    assert ref[0] < 0


@pytest.mark.parametrize("j", DEF_STEPS)
def test_restatement_at_definition_level(j, capsys):
    symb, blkS, Sd, blkD, Dd = full_case("arrow_big")
    n = symb.n
    Ld = np.linalg.cholesky(Sd)
    M = dense_operator(Ld, Dd)
    run = lanczos_restatement(apply_operator(Ld, Dd), lanczos_default_v0(n), j)
    orth, rec = definition_errors(M, run["V"], run["alpha"], run["beta"])
    with capsys.disabled():
        print("\nj = %d: max|V V^T - I| = %.5f n eps, recurrence %.5f n eps |op|" % (j, orth, rec))
    assert run["steps"] == j and not run["invariant"]
    assert orth <= RESTATEMENT_ORTH and rec <= RESTATEMENT_REC


def definition_errors(M, V, alpha, beta):
    """(max|V V^T - I| / (n eps), |op V_j - V_j T_j - beta_j v_{j+1} e_j^T|_max / (n eps |op|_2)) for the m + 1 rows of V"""
    m, n = len(alpha), M.shape[0]
    orth = np.abs(V @ V.T - np.eye(m + 1)).max() / (n * EPS)
    T = np.diag(alpha) + np.diag(beta[1:m], 1) + np.diag(beta[1:m], -1)
    R = M @ V[:m].T - V[:m].T @ T
    R[:, m - 1] -= beta[m] * V[m]
    return orth, np.abs(R).max() / (n * EPS * np.abs(np.linalg.eigvalsh(M)).max())


def test_tol_zero_runs_every_step_in_the_restatement():
    """the GPU tests of what holds unconverged use tol = 0: the estimate never stops the driver before maxit"""
    symb, blkS, Sd, blkD, Dd = full_case("arrow_big")
    Ld = np.linalg.cholesky(Sd)
    for maxit in (8, 80):
        info = driver_restatement(apply_operator(Ld, Dd), lanczos_default_v0(symb.n), 0.0, maxit)
        assert info["steps"] == maxit and not info["converged"] and not info["invariant"]


@pytest.mark.parametrize("name", ["band", "arrow", "diag", "dense"])
def test_minus_s_breaks_down_at_step_one(name):
    symb, blkS, Sd, _, _ = full_case(name)
    Ld = np.linalg.cholesky(Sd)
    run = lanczos_restatement(apply_operator(Ld, -Sd), lanczos_default_v0(symb.n), 8)
    assert run["invariant"] and run["steps"] == 1
    assert abs(run["alpha"][0] + 1.0) <= RESTATEMENT_ERR * symb.n * EPS
    run = lanczos_restatement(apply_operator(Ld, 0.0 * Sd), lanczos_default_v0(symb.n), 8)
    assert run["invariant"] and run["steps"] == 1 and run["alpha"][0] == 0.0


def test_chunk_rule_and_clamp():
    assert lanczos_chunks(64) == [(8 * k, 8) for k in range(8)]
    assert lanczos_chunks(9) == [(0, 8), (8, 1)]
    assert lanczos_chunks(1) == [(0, 1)]
    assert lanczos_chunks(80)[-1] == (72, 8) and len(lanczos_chunks(80)) == 10
    assert LANCZOS_CHUNK == 8 and LANCZOS_JMAX == 128
    assert lanczos_maxit(9, 64) == 9 and lanczos_maxit(896, 64) == 64 and lanczos_maxit(896, 1000) == 128
    assert lanczos_maxit(5, 0) == 1 and lanczos_maxit(1, 64) == 1
    assert lanczos_converged(1e-13, -2.0, 1.0, 1e-12, 8, 100, False)
    assert not lanczos_converged(1e-11, -2.0, 1.0, 1e-12, 8, 100, False)
    assert lanczos_converged(1.0, -2.0, 1.0, 1e-12, 100, 100, False)          # exhausted
    assert lanczos_converged(1.0, -2.0, 1.0, 1e-12, 3, 100, True)             # invariant
    state, basis, ld, total = lanczos_layout(15, 15)
    assert state == 48 and ld == 16 and basis == 48 + 2 * 1920 + 8 and total == basis + 18 * 16
    a, b = lanczos_default_v0(40), lanczos_default_v0(40)
    assert (a == b).all() and a.shape == (40,)


def test_tridiagonal_cases_have_the_gaps_the_gpu_test_relies_on():
    cases = tridiagonal_cases()
    w, _ = tridiagonal_reference(*cases["wilkinson21"])
    assert w[-1] - w[-2] < 1e-12 and w[1] - w[0] > 1e-3 * np.abs(w).max()       # the top pair is the famous close one
    w, Z = tridiagonal_reference(*cases["zerobeta64"])
    assert min(abs(Z[-1, 0]), abs(Z[0, 0])) < 1e-12                             # an eigenvector lives in one block
    assert math.isfinite(w[0])
