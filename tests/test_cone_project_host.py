"""The Frobenius projection onto the cone K of PSD-completable matrices and, by Moreau, onto its dual
(smcp_amd.chordal.cone_project, csp_cone_project_steps, csrc/front_ceig.hip: k_cone_split / k_cone_update / k_cone_resid):
the clique-splitting ADMM restated in numpy on the supernodal cliques, checked against the definition of the projection
and against cyclic Dykstra, its iteration counts, and the kernel's form of the clique step ("sum over the negative
eigenvalues, ascending", on the Jacobi of jacobi_vec_restatement) measured against the form with LAPACK's eigh (no GPU
needed; tests/test_gpu_cone_project.py imports this file).

Measured (the printed lines), inputs of seed 3, noisy kind, (rho, relax) = (1, 1.7), in parentheses
relax = 1: iterations to 1e-6 / 1e-8 -- band 15 (24) / 25 (42), nested 42 (56) / 82 (125), rand1 31 (42) / 60 (93),
two_components 18 (21) / 28 (35); arrow, dense and rand2 are inside the cone with this seed: 1 (1).  To 1e-12: 45, 163, 118,
53; the indef kind 69 (arrow), 508 (nested), 154 (rand1).  K, the distance of the point returned at tol from the converged
projection over tol max(1, |A|): 4.60 at 1e-6 and 4.65 at 1e-8 (nested); asserted: 5.  The kernel's form against the LAPACK
form after 3 iterations, in units nf_max eps max(1, |A|): at most 0.45 (band); asserted: 1, the device is held to 16 and
measured at 0.47 (band, indef).  Dykstra reaches 1e-11 in 1 - 3 cycles on arrow, rand1 and nested and agrees to 4.4e-12.
A warm start begins at X = A - rho sum_k E_k U0_k E_k^T; from X = A it saved nothing (81 iterations after 82 on nested)."""
import numpy as np
import pytest

import test_clique_eigh_host as ceh
from helpers import EXTRA, GPU_PATTERNS, PATTERNS
from smcp_amd import _lib, chordal, problems
from smcp_amd.symbolic import Symbolic
from test_clique_eig_host import EPS
from test_clique_eigh_host import jacobi_vec_restatement, lower_slots, pack
from test_mrcompletion_host import blkval_of, clique_rows, dense_of, pd_on_V

HOST_PATS = dict(PATTERNS)
HOST_PATS["diag"] = GPU_PATTERNS["diag"]
HOST_PATS["one_clique"] = EXTRA["one_clique"]
HOST_PATS["two_components"] = EXTRA["two_components"]
SMALL = sorted(PATTERNS) + ["two_components"]            # where the iteration has something to do
INDEF_OK = ["arrow", "nested", "rand1"]                   # random symmetric input converges linearly on these only
KINDS = ["noisy", "incone", "indef"]
PARAMS = [(1.0, 1.7), (3.0, 1.0)]                         # (rho, relax) of the three-iteration comparisons
CONE_UNITS = 1.0                                          # kernel form against LAPACK form after 3 iterations, asserted here
GPU_FACTOR = ceh.GPU_FACTOR                               # the device is held to GPU_FACTOR times that
K_BOUND = 5.0                                             # |X_tol - X_1e-12| <= K_BOUND tol max(1, |A|), asserted here
_SYMB, _INPUT, _RUN = {}, {}, {}


def host_symb(name):
    if name not in _SYMB:
        _SYMB[name] = Symbolic(HOST_PATS[name]())
    return _SYMB[name]


# ---- inputs ----------------------------------------------------------------------------------------------------------
def noisy_on_V(symb, seed):
    """factor factor^T of problems.random_factor_blkval plus 0.3 standard normal noise on V (the input of
    tools/clique_project_time.py): a point near the cone with negative eigenvalues in most clique blocks"""
    L = np.tril(dense_of(symb, problems.random_factor_blkval(symb, seed)))
    noise = np.random.default_rng(seed + 1).standard_normal(symb.blklen)
    return np.where(lower_slots(symb), blkval_of(symb, L @ L.T) + 0.3 * noise, 0.0)


def indef_on_V(symb, seed):
    return np.where(lower_slots(symb), np.random.default_rng(seed).standard_normal(symb.blklen), 0.0)


def cone_input(symb, kind, seed=3):
    """a blkval with zeros on the unused slots: made once per (Symbolic, kind), never changed"""
    key = (id(symb), kind, seed)
    if key not in _INPUT:
        blk = {"noisy": noisy_on_V, "indef": indef_on_V, "incone": lambda s, sd: np.where(lower_slots(s), pd_on_V(s, sd), 0.0)}[kind](symb, seed)
        blk.setflags(write=False)
        _INPUT[key] = blk
    return _INPUT[key]


def norm_V(symb, blk):
    """sqrt(dot(X, X)): off-diagonal entries count twice"""
    X = dense_of(symb, blk)
    return float(np.sqrt((X * X).sum()))


# ---- the iteration restated --------------------------------------------------------------------------------------------
def negative_part(T, form):
    """(U = P_-(T), number of negative eigenvalues, sweeps, eigenvalues): with LAPACK's eigh, or as k_cone_split forms it -- every entry
    of the lower triangle the sum over the negative eigenvalues of the kernel's Jacobi, ascending, mirrored"""
    if form == "lapack":
        w, Q = np.linalg.eigh(T)
        neg = w < 0
        U = (Q[:, neg] * w[neg]) @ Q[:, neg].T
        return 0.5 * (U + U.T), int(neg.sum()), 0, w
    w, Q, sweeps, ok = jacobi_vec_restatement(T)
    assert ok
    U = np.zeros_like(T)
    for j in range(len(w)):
        if w[j] < 0:
            U += w[j] * (Q[:, j][:, None] * Q[:, j][None, :])
    U = np.tril(U)
    return U + np.tril(U, -1).T, int((w < 0).sum()), sweeps, w


def cone_project_restatement(symb, blk, rho=1.0, relax=1.7, tol=1e-8, maxit=500, U0=None, steps=None, form="lapack",
                             snapshots=(), near=0.0):
    """csp_cone_project_steps and the stopping rule of chordal.cone_project in numpy, on dense matrices in the permuted
    order.  steps: run exactly that many iterations, without the test.  Returns a dict: x (blkval, zeros on the unused
    slots), U and W (packed block vectors), hist (iterations, 4: sum_k r_k^2, s^2, negative eigenvalues, 0), iterations,
    converged, scale = max(1, |A|), sweeps, snap (tolerance -> (iteration, x) at the first iteration that met it), near (per
    iteration the eigenvalues of all T_k within `near` of 0, which either side of a comparison may count as negative)."""
    A = dense_of(symb, np.asarray(blk))
    n = symb.n
    rows = [clique_rows(symb, k) for k in range(symb.Nsn)]
    mult = np.zeros((n, n))
    for r in rows:
        mult[np.ix_(r, r)] += 1.0
    on_V = mult > 0
    scale = max(1.0, float(np.sqrt((A * A).sum())))
    U = [np.zeros((len(r), len(r))) for r in rows] if U0 is None else [np.array(B) for B in ceh.unpack(symb, np.asarray(U0))]
    X = A.copy() if U0 is None else A - rho * scatter_blocks(symb, np.asarray(U0))      # the X that belongs to U0 at a fixed point
    W = [X[np.ix_(r, r)] - Uk for r, Uk in zip(rows, U)]
    hist, snap, converged, most, close = [], {}, False, 0, []
    for it in range(steps if steps is not None else maxit):
        r2, neg, amb = 0.0, 0, 0
        SW = np.zeros((n, n))
        for k, r in enumerate(rows):
            Xg = X[np.ix_(r, r)]
            Zp = W[k] + U[k]
            T = Zp + relax * (Xg - Zp) + U[k]
            U[k], cnt, sweeps, w = negative_part(T, form)
            amb += int((np.abs(w) <= near).sum())
            D = Xg - (T - U[k])
            r2 += float((D * D).sum())
            W[k] = T - 2.0 * U[k]
            SW[np.ix_(r, r)] += W[k]
            neg += cnt
            most = max(most, sweeps)
        Xn = np.where(on_V, (A + rho * SW) / (1.0 + rho * mult), 0.0)
        s2 = float(((Xn - X) ** 2).sum())
        X = Xn
        hist.append((r2, s2, float(neg), 0.0))
        close.append(amb)
        res = max(np.sqrt(r2), np.sqrt(s2))
        for t in snapshots:
            if t not in snap and res <= t * scale:
                snap[t] = (it + 1, np.where(lower_slots(symb), blkval_of(symb, X), 0.0))
        if steps is None and res <= tol * scale:
            converged = True
            break
    return {"x": np.where(lower_slots(symb), blkval_of(symb, X), 0.0), "U": pack(U), "W": pack(W), "hist": np.array(hist),
            "iterations": len(hist), "converged": converged, "scale": scale, "sweeps": most, "snap": snap, "near": np.array(close)}


def reference_run(name, kind):
    """the restatement at tol 1e-12 with (rho, relax) = (1, 1.7) and its iterates at 1e-6 and 1e-8: made once, never changed"""
    if (name, kind) not in _RUN:
        symb = host_symb(name)
        _RUN[(name, kind)] = cone_project_restatement(symb, cone_input(symb, kind), tol=1e-12, maxit=5000, snapshots=(1e-6, 1e-8))
    return _RUN[(name, kind)]


def dykstra(symb, blk, tol=1e-11, cycles=20000):
    """cyclic Dykstra over the sets {X on V : X_gg PSD}: (blkval, cycles used, converged)"""
    A = dense_of(symb, np.asarray(blk))
    rows = [clique_rows(symb, k) for k in range(symb.Nsn)]
    X = A.copy()
    P = [np.zeros((len(r), len(r))) for r in rows]
    scale = max(1.0, float(np.sqrt((A * A).sum())))
    for c in range(cycles):
        X0 = X.copy()
        for k, r in enumerate(rows):
            ix = np.ix_(r, r)
            Y = X[ix] + P[k]
            w, Q = np.linalg.eigh(Y)
            Z = (Q * np.maximum(w, 0.0)) @ Q.T
            Z = 0.5 * (Z + Z.T)
            P[k] = Y - Z
            X[ix] = Z
        if np.sqrt(((X - X0) ** 2).sum()) <= tol * scale:
            return blkval_of(symb, X), c + 1, True
    return blkval_of(symb, X), cycles, False


def scatter_blocks(symb, Z):
    """dense sum_k E_k Z_k E_k^T of a packed block vector"""
    S = np.zeros((symb.n, symb.n))
    for k, B in enumerate(ceh.unpack(symb, Z)):
        r = clique_rows(symb, k)
        S[np.ix_(r, r)] += B
    return S


# ---- against the definition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [(n, "noisy") for n in SMALL] + [(n, "indef") for n in INDEF_OK])
def test_fixed_point_is_the_projection(name, kind, capsys):
    """X in K, X - A in K*, <X, X - A> = 0 and X - A = -rho sum_k E_k U_k E_k^T, each to 1e-10 max(1, |A|)"""
    symb = host_symb(name)
    run = reference_run(name, kind)
    assert run["converged"], (name, kind, run["iterations"])
    A, X, s = dense_of(symb, cone_input(symb, kind)), dense_of(symb, run["x"]), run["scale"]
    lam_blocks = min(np.linalg.eigvalsh(X[np.ix_(clique_rows(symb, k), clique_rows(symb, k))])[0] for k in range(symb.Nsn))
    lam_dual = np.linalg.eigvalsh(X - A)[0]
    inner = abs(float((X * (X - A)).sum()))
    stat = float(np.sqrt(((X - A + 1.0 * scatter_blocks(symb, run["U"])) ** 2).sum()))
    with capsys.disabled():
        print("\n%s %s: %d iterations to 1e-12; block lambda_min %.1e, lambda_min(X - A) %.1e, |<X, X - A>| %.1e, stationarity %.1e"
              % (name, kind, run["iterations"], lam_blocks, lam_dual, inner, stat))
    assert lam_blocks >= -1e-10 * s and lam_dual >= -1e-10 * s and inner <= 1e-10 * s * s and stat <= 1e-10 * s


@pytest.mark.parametrize("name", ["arrow", "nested", "rand1"])
def test_against_dykstra(name, capsys):
    symb = host_symb(name)
    run = reference_run(name, "noisy")
    Xd, cycles, ok = dykstra(symb, cone_input(symb, "noisy"))
    d = norm_V(symb, Xd - run["x"]) / run["scale"]
    with capsys.disabled():
        print("\n%s: Dykstra %d cycles (converged %s), difference %.1e max(1, |A|)" % (name, cycles, ok, d))
    assert ok and d <= 1e-9


# ---- iteration counts and K ----------------------------------------------------------------------------------------------
def test_iteration_counts_and_distance_to_the_converged_projection(capsys):
    """relax 1.7 needs no more iterations than 1.0, every noisy case converges at 1e-8 within 200 iterations, and the point
    returned at tol is within K_BOUND tol max(1, |A|) of the projection"""
    K = 0.0
    for name in SMALL:
        symb = host_symb(name)
        run = reference_run(name, "noisy")
        plain = cone_project_restatement(symb, cone_input(symb, "noisy"), relax=1.0, tol=1e-8, maxit=5000, snapshots=(1e-6, 1e-8))
        line = []
        for tol in (1e-6, 1e-8):
            it17, x17 = run["snap"][tol]
            it10 = plain["snap"][tol][0]
            k = norm_V(symb, x17 - run["x"]) / (tol * run["scale"])
            K = max(K, k)
            line.append("%.0e: %d (relax 1.0: %d), K %.2f" % (tol, it17, it10, k))
            assert it17 <= it10, (name, tol, it17, it10)
        assert run["snap"][1e-8][0] <= 200
        with capsys.disabled():
            print("\n%s noisy: %s; |A| %.2f" % (name, "; ".join(line), run["scale"]))
    with capsys.disabled():
        print("\nK = %.2f" % K)
    assert K <= K_BOUND


@pytest.mark.parametrize("name", ["diag", "one_clique"])
def test_trivial_cases_finish_at_once(name):
    symb = host_symb(name)
    for kind in ("noisy", "indef"):
        run = cone_project_restatement(symb, cone_input(symb, kind), tol=1e-10)
        assert run["converged"] and run["iterations"] <= 2
    run = cone_project_restatement(host_symb("nested"), cone_input(host_symb("nested"), "incone"), tol=1e-10)
    assert run["converged"] and run["iterations"] <= 2 and not run["U"].any() and run["hist"][0, 2] == 0


# ---- the kernel's arithmetic -------------------------------------------------------------------------------------------
def three_iterations(symb, kind, rho, relax):
    """the LAPACK restatement after three iterations: made once per case"""
    key = (id(symb), kind, rho, relax)
    if key not in _RUN:
        _RUN[key] = cone_project_restatement(symb, cone_input(symb, kind), rho=rho, relax=relax, steps=3)
    return _RUN[key]


def unit_of(symb, scale):
    return float(np.diff(symb.rowptr).max()) * EPS * scale


@pytest.mark.parametrize("name", sorted(HOST_PATS))
def test_kernel_form_against_lapack_form(name, capsys):
    symb = host_symb(name)
    worst = 0.0
    for kind in KINDS:
        for rho, relax in PARAMS:
            ref = three_iterations(symb, kind, rho, relax)
            got = cone_project_restatement(symb, cone_input(symb, kind), rho=rho, relax=relax, steps=3, form="kernel")
            u = unit_of(symb, ref["scale"])
            worst = max(worst, max(np.abs(got[key] - ref[key]).max() for key in ("x", "U", "W")) / u)
            assert got["sweeps"] <= ceh.MAX_SWEEPS
            if kind == "incone":
                assert not got["U"].any() and (got["hist"][:, 2] == 0).all()
    with capsys.disabled():
        print("\n%s: kernel form against LAPACK form after 3 iterations: %.2f units" % (name, worst))
    assert worst <= CONE_UNITS


# ---- declarations --------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_bound():
    ceh.test_entry_points_are_declared_and_bound("csp_cone_project_steps", ["ctx", "a", "x", "U", "W", "rho", "relax", "it0", "nsteps",
                                                                           "hist", "stream"])
    args = ceh.header_arguments("csp_cone_project_steps")
    assert [a for a in args if a.startswith("int64_t")] == ["int64_t it0", "int64_t nsteps"]
    assert [t is _lib.c_i64 for t in _lib.SIGNATURES["csp_cone_project_steps"][1]].count(True) == 2
    assert ceh.header_arguments("csp_cone_project_sweeps") == ["csp_ctx* ctx", "int64_t* out", "void* stream"]
    assert "csp_cone_project_sweeps" in _lib.SIGNATURES
    assert chordal.CONE_CHUNK == 8 and chordal.cone_looks(20) == [(0, 1), (1, 1), (2, 7), (9, 8), (17, 3)]
    assert chordal.cone_looks(1) == [(0, 1)] and chordal.cone_looks(2) == [(0, 1), (1, 1)] and chordal.cone_looks(9)[-1] == (2, 7)
    import smcp_amd
    assert smcp_amd.cone_project is smcp_amd.base.cone_project
