"""Dense definitions of the chordal operations (plain numpy, fp64 LAPACK) and the blockwise comparator.

Everything here works in PERMUTED dense coordinates.  The mask of V comes from the input pattern, permuted by the symbolic
object's `p`; the clique arrays are used for the blkval <-> dense layout only (`Sym.dense` / `Sym.project`), so a wrong clique
structure shows up as an error instead of cancelling on both sides.

With A = Ld Ld^T (Ld: the dense image of a random factor) and Ai = inv(A):

    cholesky             np.linalg.cholesky(A)              hessian(adj=None, inv=False)   P_V(Ai U Ai)
    llt                  A on V                             hessian(adj=None, inv=True)    applied to P_V(Ai U Ai): U
    projected_inverse    P_V(Ai)                            trsm                           solve(Ld, B), solve(Ld^T, B)
    completion(P_V(Ai))  Ld                                 Schur complement               H_ij = sum(A_i o (Ai A_j Ai))
    logdiagsum           log(diag Ld).sum()                 KKT solve                      H y = kk by + A(P_V(Ai Bx Ai)),
    dot                  trace(X Y)                                                        x = P_V(Ai (sum y_j A_j - Bx) Ai) / kk

The two factor modes G (adj=False) and G^adj (adj=True) have no dense definition of their own (they depend on the factorisation);
they are pinned by the identities of tests/test_oracle_identities.py with the right-hand sides evaluated densely:
G^adj(G(U)) = P_V(Ai U Ai), <G U, G U> = tr(Ai U Ai U), <G U, W> = <U, G^adj W>, and each factor inverse undoes its factor.

`measure(ops, ...)` runs every one of these checks on an implementation handed over as a table of callables -- the CPU oracle
(tests/test_dense_ref.py, tests/golden/make_dense_ref_yardstick.py) or the HIP library (tests/test_gpu_dense_ref.py) -- and
returns operation -> error.  Matrix results are measured per clique (`blockwise`), scalars and vectors relatively.
"""
import json
import os
import types

import numpy as np

from oracle import oracle as orc
from smcp_amd import problems

YARDSTICK_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_ref_yardstick.json")
# no device bound may be looser than this, whatever the yardstick says
BOUND_CAP = 1e-12
# the suite's KKT input recipe
# (seed 9, as tests/test_gpu_parity.py: on `diag` every constraint is a single entry, and these seven are distinct)
KKT_M, KKT_DENSITY, KKT_KK, KKT_SEED = 7, 0.05, (1.0, 0.25), 9
# the mixed recipe: entries of the two narrow kinds of constraint (a constraint of k entries touches at most 2 k rows / columns)
FEW_ENTRIES, SINGLE_ENTRIES = 3, 1
MIX_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hybrid_recipe_yardstick.json")


# ---- the mixed KKT recipe ----------------------------------------------------------------------------------------------
def interleave(nwide, nfew, nsingle):
    """the order of a mixed recipe as a string over 'f' (few), 'w' (wide), 's' (single): the kinds dealt in turn
    (f, w, s, f, w, s, ...) until each has run out, so that neither class of the device is a contiguous range"""
    left, out = {"f": nfew, "w": nwide, "s": nsingle}, []
    while any(left.values()):
        for kind in "fws":
            if left[kind]:
                left[kind] -= 1
                out.append(kind)
    return "".join(out)


def mixed_constraints(lay, m, density, seed, mix):
    """(cptr, cidx, cval) of len(mix) constraints in the order `mix`: its 'w' constraints are random_constraints(lay, m, density,
    seed) unchanged and in their order (mix holds m of them), an 'f' has FEW_ENTRIES entries and an 's' one entry, at V slots
    drawn without replacement over all narrow constraints together (so no two of them are multiples of each other)"""
    assert set(mix) <= set("fws") and mix.count("w") == m, (mix, m)
    wptr, widx, wval = problems.random_constraints(lay, m, density=density, seed=seed) if m else (np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0))
    rng = np.random.default_rng(seed + 1000)
    need = FEW_ENTRIES * mix.count("f") + SINGLE_ENTRIES * mix.count("s")
    slots = rng.choice(problems.lower_positions(lay), size=need, replace=False)
    # values bounded away from zero and scaled so that a narrow constraint has about the Frobenius norm of a wide one (per: the
    # entries of a wide one, each standard normal): H is then not badly scaled by construction -- a single entry of 0.005 beside
    # hundreds of order one put cond(H) at 2e6 on nested_mid and the ORACLE's kkt_y at 5e-14, which says nothing about any route
    vals = rng.standard_normal(need)
    vals = np.sign(vals) * (0.5 + np.abs(vals))
    per = max(1, int(wptr[1])) if m else 1
    idx, val, ptr, w, t = [], [], [0], 0, 0
    for kind in mix:
        if kind == "w":
            i, v = widx[wptr[w]:wptr[w + 1]], wval[wptr[w]:wptr[w + 1]]
            w += 1
        else:
            k = FEW_ENTRIES if kind == "f" else SINGLE_ENTRIES
            order = np.argsort(slots[t:t + k])
            i, v = slots[t:t + k][order], vals[t:t + k][order] * np.sqrt(per / k)
            t += k
        idx.append(i)
        val.append(v)
        ptr.append(ptr[-1] + len(i))
    return np.array(ptr, dtype=np.int64), np.concatenate(idx).astype(np.int64), np.concatenate(val)


def touched(S, con):
    """per constraint, the number of distinct rows / columns (permuted coordinates) its entries touch: what the device's
    classification compares with int(n * tnzcols)"""
    cptr, cidx, cval = con
    out = []
    for j in range(len(cptr) - 1):
        u = np.zeros(S.blklen)
        u[cidx[cptr[j]:cptr[j + 1]]] = 1.0
        r, c = np.nonzero(S.dense(u))
        out.append(len(set(r.tolist()) | set(c.tolist())))
    return out


def hybrid_case(pattern, m, density, seed, mix, tnzcols, max_rhs=None):
    """a hybrid case: the mixed recipe (m wide ones at `density`, order `mix`) on a pattern, the tnzcols that must separate its
    wide constraints (swept) from its narrow ones (column-sparse), and the max_rhs of the context (default: all wide ones in one block)"""
    return dict(pattern=pattern, recipe=(m, density, seed, mix), tnzcols=tnzcols, max_rhs=max_rhs or max(4, m))


_NESTED = ("nested", 5, KKT_DENSITY, KKT_SEED)
# name -> hybrid case of tests/test_gpu_hybrid_schur.py.  The seven patterns with 4 few + 3 single constraints dealt among the wide
# ones (`diag` has no wide class); then the class-size edges on `nested`; then many single-entry constraints (chunks)
HYBRID_CASES = {
    "nested": hybrid_case(*_NESTED, interleave(5, 4, 3), 0.2),
    "rand2": hybrid_case("rand2", 5, KKT_DENSITY, KKT_SEED, interleave(5, 4, 3), 0.2),
    "arrow": hybrid_case("arrow", 5, KKT_DENSITY, KKT_SEED, interleave(5, 4, 3), 0.25),
    "fam_odd": hybrid_case("fam_odd", 6, 0.03, 13, interleave(6, 4, 3), 0.1),
    "nested_mid": hybrid_case("nested_mid", 12, 0.002, 13, interleave(12, 4, 3), 0.1),
    "arrow_big": hybrid_case("arrow_big", 4, 0.004, 52, interleave(4, 4, 3), 0.1),
    "arrow_thin": hybrid_case("arrow_thin", 8, 0.03, 32, interleave(8, 4, 3), 0.1),
    "md1": hybrid_case("nested", 1, KKT_DENSITY, KKT_SEED, interleave(1, 3, 2), 0.2),                   # one swept, five sparse
    "ns1": hybrid_case("nested", 5, KKT_DENSITY, KKT_SEED, interleave(5, 0, 1), 0.2),                   # five swept, one sparse
    "two_blocks": hybrid_case(*_NESTED, interleave(5, 4, 3), 0.2, max_rhs=4),                         # five swept in blocks of 4 + 1 into one D.hd
    "gram130": hybrid_case("nested", 130, KKT_DENSITY, KKT_SEED, interleave(130, 2, 1), 0.2, max_rhs=4),   # md > GRAM_BLK = 128
    "ends": hybrid_case("nested", 5, KKT_DENSITY, KKT_SEED, "w" + interleave(3, 4, 3) + "w", 0.2),       # swept at index 0 and at index m - 1
    # two chunks of sparse constraints: fam_odd has the smallest trsm_cap per right-hand side of the seven patterns (29), so with
    # max_rhs = 4 the 70 single-entry constraints (one or two columns of the inverse each) pass vcols = trsm_cap = 117 columns
    "chunks": hybrid_case("fam_odd", 2, 0.03, 13, interleave(2, 0, 70), 0.1, max_rhs=4),
}


def recipe_key(pattern, recipe):
    m, density, seed, mix = recipe
    return "%s|m=%d,density=%s,seed=%d,mix=%s" % (pattern, m, density, seed, mix)


def load_mix_yardstick():
    with open(MIX_FILE) as f:
        return json.load(f)


def hybrid_bound(key, op, yard=None, own=None):
    """bound of a device-vs-dense check on a mixed recipe: 100 x the larger of the global yardstick value and the recorded
    oracle-vs-dense error of this (pattern, recipe) (tests/golden/hybrid_recipe_yardstick.json), never looser than BOUND_CAP"""
    yard = load_yardstick() if yard is None else yard
    own = load_mix_yardstick() if own is None else own
    return min(100.0 * max(float(yard[op]["value"]), float(own[key][op])), BOUND_CAP)


# ---- layout helpers ----------------------------------------------------------------------------------------------------
def pattern_mask(pat, p):
    """Symmetric boolean mask of the INPUT pattern in permuted coordinates (p[new] = orig)."""
    n, cp, ri = pat
    cols = np.repeat(np.arange(n), np.diff(cp))
    M = np.zeros((n, n), dtype=bool)
    M[ri, cols] = True
    M |= M.T
    p = np.asarray(p)
    return M[np.ix_(p, p)]


def lower_mask(S):
    """True at the blkval positions that belong to V (everything but the strict upper triangle of every X_NN)."""
    m = np.ones(S.blklen, dtype=bool)
    for k, nn, rows in S._iter():
        nf = len(rows)
        b = m[S.blkptr[k]:S.blkptr[k] + nf * nn].reshape((nf, nn), order="F")
        b[:nn, :nn][np.triu_indices(nn, 1)] = False
    return m


def layout(S):
    """What smcp_amd.problems' generators read of a Symbolic, for any oracle.Sym (the product's arrays or symbolic_ref's)."""
    low = np.flatnonzero(lower_mask(S))
    return types.SimpleNamespace(blklen=S.blklen, snptr=S.snptr, rowptr=S.rowptr, blkptr=S.blkptr, Nsn=S.nsn, n=S.n,
                                 nnz=len(low), ccs_to_blk=lambda: low)


# ---- comparator --------------------------------------------------------------------------------------------------------
def blockwise(S, got, ref):
    """(global relative 2-norm error, worst per-clique relative error) over the V slots of two blkval vectors.
    Per clique k: |got_k - ref_k| / |ref_k|; a clique whose reference block is exactly zero is measured against the global norm."""
    msk = lower_mask(S)
    d = np.where(msk, got - ref, 0.0)
    r = np.where(msk, ref, 0.0)
    if not np.isfinite(d).all():
        return np.inf, np.inf
    starts = S.blkptr[:-1]
    dk = np.sqrt(np.add.reduceat(d * d, starts))
    rk = np.sqrt(np.add.reduceat(r * r, starts))
    rg = np.sqrt((r * r).sum())
    dg = np.sqrt((d * d).sum())
    if rg == 0.0:
        return dg, float(dk.max())
    per = dk / np.where(rk > 0, rk, rg)
    return dg / rg, float(per.max())


def relvec(got, ref):
    nr = np.linalg.norm(ref)
    if not np.isfinite(got).all():
        return np.inf
    return np.linalg.norm(got - ref) / nr if nr > 0 else np.linalg.norm(got)


# ---- the dense case of one pattern -------------------------------------------------------------------------------------
class DenseCase:
    """Dense matrices of one (pattern, symbolic, seed): the factor, A, inv(A), and the definitions above."""

    def __init__(self, pat, S, seed):
        self.pat, self.S, self.seed = pat, S, seed
        self.lay = layout(S)
        self.low = lower_mask(S)
        self.mask = pattern_mask(pat, S.p)
        self.Lblk = problems.random_factor_blkval(self.lay, seed)
        self.Ld = S.dense(self.Lblk, symmetric=False)
        self.A = self.Ld @ self.Ld.T
        Ai = np.linalg.inv(self.A)
        self.Ai = 0.5 * (Ai + Ai.T)
        self.Ablk = S.project(self.proj(self.A))
        self.Yblk = S.project(self.proj(self.Ai))
        self._kkt = None
        # (m, density, seed) or, mixed, (wide ones, density, seed, order: interleave); tests/route_ledger.py sets its own before kkt()
        self.kkt_recipe = (KKT_M, KKT_DENSITY, KKT_SEED)

    def proj(self, M):
        return np.where(self.mask, M, 0.0)

    def blk(self, M):
        """blkval of P_V(M), M dense symmetric."""
        return self.S.project(self.proj(M))

    def cholesky(self):
        return self.S.project(np.where(self.mask, np.linalg.cholesky(self.A), 0.0))

    def hessian(self, u):
        """P_V(Ai U Ai) for the blkval u."""
        return self.blk(self.Ai @ self.S.dense(u) @ self.Ai)

    def tr_hess(self, u):
        """tr(Ai U Ai U)"""
        U = self.S.dense(u)
        W = self.Ai @ U
        return float(np.sum(W * W.T))

    def dot(self, x, y):
        return float(np.sum(self.S.dense(x) * self.S.dense(y)))

    def rhs(self, nrhs, seed):
        """The suite's right-hand sides: standard normal on the V slots, zero elsewhere."""
        return np.random.default_rng(seed).standard_normal((nrhs, self.S.blklen)) * self.low

    # ---- KKT
    def kkt(self):
        if self._kkt is None:
            S = self.S
            m, density, seed = self.kkt_recipe[:3]
            mix = self.kkt_recipe[3] if len(self.kkt_recipe) > 3 else None
            if mix:                                          # (m: the wide ones; the definitions below do not know about kinds)
                cptr, cidx, cval = mixed_constraints(self.lay, m, density, seed, mix)
            else:
                cptr, cidx, cval = problems.random_constraints(self.lay, m, density=density, seed=seed)
            K = orc.KKT(S, cptr, cidx, cval)
            Ad = [S.dense(K.constraint(j)) for j in range(K.m)]
            W = [self.Ai @ Aj @ self.Ai for Aj in Ad]
            H = np.array([[np.sum(Ad[i] * W[j]) for j in range(K.m)] for i in range(K.m)])
            rng = np.random.default_rng(self.seed + 3)
            bx = rng.standard_normal(S.blklen) * self.low
            by = rng.standard_normal(K.m)
            self._kkt = types.SimpleNamespace(con=(cptr, cidx, cval), K=K, Ad=Ad, H=0.5 * (H + H.T), bx=bx, by=by)
        return self._kkt

    def kkt_solve(self, kk):
        """(x as blkval, y) of [-kk H^-1 A^adj; A 0][x; y] = [bx; by] from the dense definitions."""
        k = self.kkt()
        Bx = self.S.dense(k.bx)
        R = self.proj(self.Ai @ Bx @ self.Ai)
        rhs = kk * k.by + np.array([np.sum(Aj * R) for Aj in k.Ad])
        y = np.linalg.solve(k.H, rhs)
        T = sum(yj * Aj for yj, Aj in zip(y, k.Ad)) - Bx
        return self.blk(self.Ai @ T @ self.Ai) / kk, y


# ---- every check, on any implementation --------------------------------------------------------------------------------
HESS_MODES = [(None, False), (None, True), (False, False), (True, False), (False, True), (True, True)]


def hessian_errors(case, hess, u, w):
    """Errors of the six Hessian modes on the right-hand sides u (nrhs x blklen; w: a second set for the adjoint identity).
    hess(U, adj, inv) -> result rows for input rows U.  Returns operation -> worst error over the rows."""
    S = case.S
    nr = u.shape[0]
    href = [case.hessian(u[r]) for r in range(nr)]
    out = {}
    full = hess(u, None, False)
    out["hessian"] = max(blockwise(S, full[r], href[r])[1] for r in range(nr))
    back = hess(np.array(href), None, True)
    out["hessian_inv"] = max(blockwise(S, back[r], u[r])[1] for r in range(nr))
    g = hess(u, False, False)
    gg = hess(g, True, False)
    out["hessian_gadj_g"] = max(blockwise(S, gg[r], href[r])[1] for r in range(nr))
    out["hessian_gram"] = max(abs(case.dot(g[r], g[r]) - case.tr_hess(u[r])) / case.tr_hess(u[r]) for r in range(nr))
    ga = hess(w, True, False)
    out["hessian_adjoint"] = max(abs(case.dot(g[r], w[r]) - case.dot(u[r], ga[r]))
                                 / np.sqrt(case.tr_hess(u[r]) * case.dot(w[r], w[r])) for r in range(nr))
    gi = hess(g, False, True)
    gai = hess(ga, True, True)
    out["hessian_factor_inv"] = max(max(blockwise(S, gi[r], u[r])[1], blockwise(S, gai[r], w[r])[1]) for r in range(nr))
    return out


def measure(case, ops, nrhs=1, parts=("tree", "hessian", "trsm", "kkt")):
    """operation -> error of the implementation `ops` against the dense definitions of `case`.

    ops: namespace of callables on host numpy arrays, each returning its result --
      cholesky(a), llt(l), projected_inverse(l), completion(y) -> blkval;  logdiagsum(l), dot(x, y) -> float;
      hessian(U, adj, inv) -> rows;  trsm(l, B, trans) -> B (nrhs x n);
      kkt(con, l, y) -> (Hl, solve) with Hl the lower Cholesky factor of the Schur complement and solve(bx, by, kk) -> (x, y)."""
    S = case.S
    out = {}
    Lref = case.cholesky()
    if "tree" in parts:
        out["cholesky"] = blockwise(S, ops.cholesky(case.Ablk.copy()), Lref)[1]
        out["llt"] = blockwise(S, ops.llt(Lref.copy()), case.Ablk)[1]
        out["projected_inverse"] = blockwise(S, ops.projected_inverse(Lref.copy()), case.Yblk)[1]
        out["completion"] = blockwise(S, ops.completion(case.Yblk.copy()), case.Lblk)[1]
        lds = np.log(np.diag(case.Ld)).sum()
        out["logdiagsum"] = abs(ops.logdiagsum(Lref.copy()) - lds) / abs(lds)
        d = np.trace(case.Ai @ case.A)                      # tr(P_V(Ai) A): A lies on V
        out["dot"] = abs(ops.dot(case.Yblk.copy(), case.Ablk.copy()) - d) / abs(d)
    if "hessian" in parts:
        u = case.rhs(nrhs, case.seed + 10)
        w = case.rhs(nrhs, case.seed + 11)
        out.update(hessian_errors(case, ops.hessian, u, w))
    if "trsm" in parts:
        rng = np.random.default_rng(case.seed + 4)
        e = 0.0
        for nb in (4, 8, 70):
            B = rng.standard_normal((nb, S.n))
            e = max(e, relvec(ops.trsm(Lref.copy(), B.copy(), "N").T, np.linalg.solve(case.Ld, B.T)),
                    relvec(ops.trsm(Lref.copy(), B.copy(), "T").T, np.linalg.solve(case.Ld.T, B.T)))
        out["trsm"] = e
    if "kkt" in parts:
        out.update(kkt_errors(case, ops.kkt))
    return out


def kkt_errors(case, kkt):
    k = case.kkt()
    Hl, solve = kkt(k.con, case.cholesky(), case.Yblk.copy())
    Hl = np.tril(Hl)
    out = {"kkt_H": relvec(Hl @ Hl.T, k.H), "kkt_x": 0.0, "kkt_y": 0.0}
    for kk in KKT_KK:
        xr, yr = case.kkt_solve(kk)
        x, y = solve(k.bx.copy(), k.by.copy(), kk)
        out["kkt_x"] = max(out["kkt_x"], blockwise(case.S, x, xr)[1])
        out["kkt_y"] = max(out["kkt_y"], relvec(y, yr))
    return out


# ---- the CPU oracle as an implementation -------------------------------------------------------------------------------
def oracle_ops(case):
    S = case.S
    L = case.cholesky()

    def inplace(f):
        def run(x):
            f(S, x)
            return x
        return run

    def hessian(U, adj, inv):
        out = np.array(U, dtype=float)
        for r in range(out.shape[0]):
            orc.hessian(S, L, case.Yblk, out[r], adj=adj, inv=inv)
        return out

    def trsm(l, B, trans):
        orc.trsm(S, l, B, trans)
        return B

    def kkt(con, l, y):
        K = orc.KKT(S, *con)
        H = K.schur_factor(l, y)
        return np.tril(H), lambda bx, by, kk: K.solve(l, y, H, bx, by, kk)

    return types.SimpleNamespace(cholesky=inplace(orc.cholesky), llt=inplace(orc.llt),
                                 projected_inverse=inplace(orc.projected_inverse), completion=inplace(orc.completion),
                                 logdiagsum=lambda x: orc.logdiagsum(S, x), dot=lambda x, y: orc.dot(S, x, y),
                                 hessian=hessian, trsm=trsm, kkt=kkt)


YARDSTICK_SEED = 1


def oracle_yardstick(name, which, seed=YARDSTICK_SEED):
    """operation -> oracle-vs-dense error on GPU_PATTERNS[name]; which: 'product' (smcp_amd.symbolic) or 'ref' (symbolic_ref)."""
    from oracle.symbolic_ref import symbolic_ref
    from smcp_amd.symbolic import Symbolic
    from tests.helpers import GPU_PATTERNS, edges_of
    pat = GPU_PATTERNS[name]()
    S = orc.Sym(Symbolic(pat)) if which == "product" else orc.Sym(symbolic_ref(pat[0], edges_of(pat)))
    case = DenseCase(pat, S, seed)
    return measure(case, oracle_ops(case))


def load_yardstick():
    with open(YARDSTICK_FILE) as f:
        return json.load(f)


def device_bound(op, yard=None):
    """Bound of a device-vs-dense check: 100 x the recorded oracle-vs-dense worst case, never looser than BOUND_CAP.
    Reason for the factor: the device sweeps use explicit inverses of the 16 x 16 / 64 x 64 diagonal blocks instead of
    substitutions, which amplifies rounding by about the block's condition number (<= 9 on these inputs), and they sum in
    another order and with fp64 atomics: two orders over an independent fp64 implementation."""
    yard = load_yardstick() if yard is None else yard
    return min(100.0 * float(yard[op]["value"]), BOUND_CAP)


# Hessian mode -> the yardstick entry that bounds a comparison of two results of that mode
MODE_OP = {(None, False): "hessian", (None, True): "hessian_inv", (False, False): "hessian_gadj_g", (True, False): "hessian_gadj_g",
           (False, True): "hessian_factor_inv", (True, True): "hessian_factor_inv"}


# ---- the HIP library as an implementation (GPU tests only) -------------------------------------------------------------
def to_dev(symb, x):
    import torch
    from smcp_amd.cspmatrix import cspmatrix
    return cspmatrix(symb, torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda())


def to_host(X):
    return X.blkval.cpu().numpy()


def constraint_classes(sysk):
    """(swept through the Hessian, column-sparse) as the device classified the constraints of a KKTSystem (kkt_constraint_classes)"""
    import ctypes
    from smcp_amd import _lib
    cnt = (ctypes.c_int64 * 2)()
    assert _lib.lib().kkt_constraint_classes(sysk.symb.handle, cnt) == 0
    return int(cnt[0]), int(cnt[1])


def device_kkt(symb, route="chol", tnzcols=None, max_rhs=4, classes=None):
    """kkt(con, l, y) of `measure` on the device: route 'chol' (KKTSystem.factor) or 'qr' (factor_qr, tnzcols = 0).
    The last system built is kept in kkt.last (the contract tests look at its aadj), its classes in kkt.classes; `classes`:
    the (swept, sparse) counts the caller expects -- another classification fails here instead of passing on another route."""
    import torch
    from smcp_amd.kkt import KKTSystem

    def kkt(con, l, y):
        sysk = KKTSystem(symb, *con, max_rhs=max_rhs, tnzcols=0.0 if route == "qr" else tnzcols)
        kkt.classes = constraint_classes(sysk)
        assert classes is None or kkt.classes == tuple(classes), "constraint classes (swept, sparse) %s, expected %s" % (kkt.classes, tuple(classes))
        Ld, Yd = to_dev(symb, l), to_dev(symb, y)
        if route == "qr":
            solve_ = sysk.factor_qr(Ld, Yd)
            Rt, _ = sysk.qr_inspect()                        # R^T R = H: the device's inner product carries the svec weights
            Hl = np.tril(Rt)
        else:
            solve_ = sysk.factor(Ld, Yd)
            Hl = np.tril(sysk.H.cpu().numpy().T)             # device H is column-major m x m
        kkt.last = sysk

        def solve(bx, by, kk):
            bxd, byd = to_dev(symb, bx), torch.from_numpy(by.copy()).cuda()
            solve_(bxd, byd, kk)
            return to_host(bxd), byd.cpu().numpy()

        return Hl, solve

    return kkt


def device_ops(symb, case, **kkt_args):
    import torch
    from smcp_amd import chordal

    def inplace(f):
        def run(x):
            X = to_dev(symb, x)
            f(X)
            return to_host(X)
        return run

    Ld, Yd = to_dev(symb, case.cholesky()), to_dev(symb, case.Yblk)

    def hessian(U, adj, inv):
        Ud = torch.from_numpy(np.ascontiguousarray(U, dtype=np.float64)).cuda()
        chordal.hessian(Ld, Yd, Ud, adj=adj, inv=inv)
        return Ud.cpu().numpy()

    def trsm(l, B, trans):
        Bd = torch.from_numpy(B).cuda()
        chordal.trsm(to_dev(symb, l), Bd, trans)
        return Bd.cpu().numpy()

    return types.SimpleNamespace(cholesky=inplace(chordal.cholesky), llt=inplace(chordal.llt),
                                 projected_inverse=inplace(chordal.projected_inverse), completion=inplace(chordal.completion),
                                 logdiagsum=lambda x: chordal.logdiagsum(to_dev(symb, x)),
                                 dot=lambda x, y: chordal.dot(to_dev(symb, x), to_dev(symb, y)),
                                 hessian=hessian, trsm=trsm, kkt=device_kkt(symb, **kkt_args), L=Ld, Y=Yd)
