"""CHOMPACK-named entry points over the C-ABI (the calls imported at solvers.py:82-97).

Every function mutates its argument in place and raises ``ArithmeticError`` when the matrix is
not positive definite / not PD-completable, exactly as the reference's callers expect
(solvers.py:623-630,638-645).  All arithmetic happens in HIP kernels; there is no CPU path.
"""
import ctypes
import math

import torch

from . import _lib
from .cspmatrix import cspmatrix, _stream, note_cache, sync_cache


def _chk(rc, what):
    if rc > 0:
        raise ArithmeticError("%s: matrix is not positive definite (clique %d)" % (what, rc - 1))
    if rc < 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, {
            -1: "invalid argument", -2: "no MI355X device initialised (no CPU fallback)",
            -3: "HIP error", -4: "out of memory",
            -5: "stale derived quantities (prepared sharded factor overwritten, or a matrix changed without csp_touch)",
            -6: "in-launch dependency wait timed out (one-launch blocked Cholesky)",
            -7: "the Jacobi iteration of a clique block did not converge in 30 sweeps (a non-finite entry?)"}.get(rc, "?")))


def _ensure(symb, nrhs=1):
    if symb._device is None or symb._max_rhs < 1:
        if not torch.cuda.is_available():
            raise RuntimeError("smcp_amd needs an MI355X (HIP) device; there is no CPU fallback")
        symb.device_init(torch.cuda.current_device(), max(1, nrhs))


def lazy_status(symb, on=True):
    """Deferred failure reports (include/smcp_amd.h: csp_lazy_status): with on=True the factorisations on `symb` no
    longer wait for the device to tell whether the matrix was positive definite -- they return at once and the first
    failure is latched on the device until ``check_status`` reads it.  The reference's calls raise immediately
    (solvers.py:881-891); a driver that knows its scaling point is inside the cone (the line search has just factored
    it) can run a whole KKT solve with ONE host synchronisation this way."""
    _ensure(symb)
    _chk(_lib.lib().csp_lazy_status(symb.handle, 1 if on else 0), "csp_lazy_status")
    symb.__dict__["_lazy_status"] = bool(on)


TUNE_LEAFGRAM, TUNE_VERIFY_CACHE, TUNE_DETERMINISTIC, TUNE_PLACEMENT, TUNE_RACE, TUNE_RACE_DROP_JOINS = 1, 2, 3, 4, 5, 6
TUNE_CEIG_WIDE = 7
TUNE_SLOT_DOUBLES = 8


def tune(symb, what, value):
    """include/smcp_amd.h: csp_tune -- TUNE_LEAFGRAM (0 never / 1 when cheaper / 2 whenever possible: closed-form Gram
    blocks of childless small cliques), TUNE_VERIFY_CACHE (1: every reuse of a cached derived quantity checks a
    fingerprint of the matrix it came from; a forgotten ``touch`` raises instead of serving stale factors),
    TUNE_DETERMINISTIC (1: fixed-order summation, bit-identical results from run to run), TUNE_PLACEMENT (an action: value =
    tries; after the constraints are set, moves the packed exchange buffer to the fastest of up to `tries` fresh allocations
    for the store pattern of the family sweep -- for runs of many Newton steps on one problem), TUNE_RACE (value = seed,
    0 = off, process-wide: seeded delay injection on every internal stream hand-over, tools/race_hunt.sh).

    TUNE_CEIG_WIDE (per Symbolic; value = the smallest order of a clique that takes the wide route, 0 = never, the default;
    1 .. 64 and negative values are refused: RuntimeError, invalid argument): ``clique_eigvalsh`` (with and without B), ``cone_margin``, ``max_step``,
    ``clique_eigh`` and ``clique_project`` diagonalise such cliques by a block Jacobi spread over the whole chip (csrc/front_ceigw.hip) instead of
    one workgroup per clique, and so does every iteration of ``cone_project`` (a fixed chain of launches per iteration, with
    nothing read back; its ``info["wide"]``).  With B given (``max_step``) the Cholesky of B_gg and the two triangular solves run
    by 64-row tiles over the chip in front of the block Jacobi.  ``clique_eig_wide`` tells how
    many cliques took the route, and ``clique_eig_sweeps`` counts block sweeps for them.

    TUNE_SLOT_DOUBLES (per Symbolic; value = the doubles that the slots in device memory of one launch of the completions and
    clique spectra, or the workspace of one launch group of wide cliques, may take; 0 = the default, 2**25; negative values are
    refused): a launch always keeps one slot and a group one clique, so 1 makes one workgroup walk every clique too wide for
    LDS through one slot and puts every wide clique into a group of its own.  It is there so that the tests reach those two
    paths at small sizes, and it caps workspace memory; results do not depend on it, bit for bit.  ``slot_share`` and
    ``clique_eig_groups`` tell what it did to the last call."""
    _ensure(symb)
    _chk(_lib.lib().csp_tune(symb.handle, int(what), int(value)), "csp_tune")


def race_injected(symb):
    """Delay kernels injected so far in this process (csp_tune_report: TUNE_RACE)."""
    import ctypes
    rep = (ctypes.c_double * 3)()
    _chk(_lib.lib().csp_tune_report(symb.handle, rep), "csp_tune_report")
    return int(rep[2])


def touch(X):
    """Tell the library that X.blkval was rewritten by means it cannot see (torch arithmetic on the tensor, a copy into
    it): whatever it had derived from the old contents at that address is dropped (csp_touch).  The wrappers of this
    module track torch's in-place version counter and do this themselves; the call is for code that goes through raw
    pointers, as the reference does with blas.scal(a, X.blkval) (solvers.py:407, 905)."""
    if X.symb._device is not None:
        _chk(_lib.lib().csp_touch(X.symb.handle, X.blkval.data_ptr()), "csp_touch")
    X.touched()


def check_status(symb, what="factorisation (deferred status)"):
    """Synchronises and raises the ArithmeticError a factorisation since the last check would have raised."""
    _chk(_lib.lib().csp_status(symb.handle, _stream()), what)


def cholesky(X):
    _ensure(X.symb)
    X.touched()
    try:
        _chk(_lib.lib().csp_cholesky(X.symb.handle, X.blkval.data_ptr(), _stream()), "cholesky")
    finally:
        note_cache(X.symb, X)


def llt(L):
    _ensure(L.symb)
    L.touched()
    try:
        _chk(_lib.lib().csp_llt(L.symb.handle, L.blkval.data_ptr(), _stream()), "llt")
    finally:
        note_cache(L.symb, L)


def projected_inverse(L):
    _ensure(L.symb)
    L.touched()
    try:
        _chk(_lib.lib().csp_projected_inverse(L.symb.handle, L.blkval.data_ptr(), _stream()), "projected_inverse")
    finally:
        note_cache(L.symb, L)


def cholesky_projected_inverse(L, Y, factors=True):
    """The dual scaling point (solvers.py:881-891): L holds S on entry; on return L = cholesky(S) and Y = projected_inverse(L),
    from ONE library call whose independent stages overlap (csp_cholesky_projected_inverse).  factors: also leave the
    Cholesky factors of the separator blocks of Y behind (what hessian(adj=False / True) and the Schur sweeps use next)."""
    _ensure(L.symb)
    L.touched()
    Y.touched()
    try:
        _chk(_lib.lib().csp_cholesky_projected_inverse(L.symb.handle, L.blkval.data_ptr(), Y.blkval.data_ptr(), 1 if factors else 0,
                                                       _stream()), "cholesky")
    finally:
        note_cache(L.symb, L)
        note_cache(L.symb, Y)


def completion(X):
    _ensure(X.symb)
    X.touched()
    try:
        _chk(_lib.lib().csp_completion(X.symb.handle, X.blkval.data_ptr(), _stream()), "completion")
    finally:
        note_cache(X.symb, X)


def mrcompletion(X, tol=1e-12):
    """chompack.mrcompletion(X): Y (n x r, float64 device tensor, rows in the PERMUTED order) with P_V(Y Y^T) = X, where
    r is the largest numerical rank of a clique block X_gg (pivots of a diagonally pivoted Cholesky above
    tol * max diag(X_gg)).  X is not changed.  ArithmeticError (naming the clique) when a clique block has a pivot below
    -tol * max diag(X_gg): X has no positive semidefinite completion."""
    symb = X.symb
    _ensure(symb)
    L = _lib.lib()
    r = ctypes.c_int64(0)
    _chk(L.csp_mrcompletion_rank(symb.handle, X.blkval.data_ptr(), float(tol), ctypes.byref(r), _stream()), "mrcompletion")
    Y = torch.zeros((symb.n, r.value), dtype=torch.float64, device=X.blkval.device)
    if r.value:
        _chk(L.csp_mrcompletion(symb.handle, X.blkval.data_ptr(), float(tol), r.value, Y.data_ptr(), r.value, _stream()),
             "mrcompletion")
    return Y


def psdcompletion(X, tol=1e-12):
    """chompack.psdcompletion(X): the maximum-determinant positive semidefinite completion of X as a dense n x n float64
    device tensor, rows and columns in the PERMUTED order; it equals X on V bit for bit and is exactly symmetric.  For X
    positive definite on V its inverse vanishes off V (what base.completion returns); X may also be singular: the
    separator blocks X_AA are solved with a diagonally pivoted Cholesky whose pivots count while above
    tol * max diag(X_AA), and nothing else is inverted.  Entries between different components of the pattern are zero.
    X is not changed.  ArithmeticError (naming the clique) when a clique block has a pivot below -tol * max diag(X_gg): X
    has no positive semidefinite completion."""
    symb = X.symb
    _ensure(symb)
    out = torch.empty((symb.n, symb.n), dtype=torch.float64, device=X.blkval.device)
    _chk(_lib.lib().csp_psdcompletion(symb.handle, X.blkval.data_ptr(), float(tol), out.data_ptr(), symb.n, _stream()),
         "psdcompletion")
    return out


def edmcompletion(D, tol=1e-12):
    """chompack.edmcompletion(D): points Y (n x r, float64 device tensor, rows in the PERMUTED order) with
    |Y_i - Y_j|^2 = D_ij on V, for D holding squared distances on a chordal pattern with a zero diagonal.  r is the
    largest numerical affine dimension of a clique: the pivots of a diagonally pivoted Cholesky of the clique's centred
    Gram matrix G above tol * max diag(G).  Y is determined up to a rigid motion; the same D gives the same Y bit for bit.
    D is not changed.  ValueError for a nonzero diagonal entry; ArithmeticError (naming the clique) when a clique block
    is not a Euclidean distance matrix (its G has a pivot below -tol * max diag(G)): D has no Euclidean completion."""
    symb = D.symb
    _ensure(symb)
    L = _lib.lib()
    r = ctypes.c_int64(0)
    rc = L.csp_edmcompletion_rank(symb.handle, D.blkval.data_ptr(), float(tol), ctypes.byref(r), _stream())
    if rc == -1 and bool((D.diag() != 0).any()):
        raise ValueError("edmcompletion: D has a nonzero diagonal entry")
    if rc > 0:
        raise ArithmeticError("edmcompletion: not a Euclidean distance matrix (clique %d)" % (rc - 1))
    _chk(rc, "edmcompletion")
    Y = torch.zeros((symb.n, r.value), dtype=torch.float64, device=D.blkval.device)
    if r.value:
        _chk(L.csp_edmcompletion(symb.handle, D.blkval.data_ptr(), float(tol), r.value, Y.data_ptr(), r.value, _stream()),
             "edmcompletion")
    return Y


def _clique_eig(A, B, what):
    """csp_clique_eigvalsh: (w, ext) as device tensors; ext = [min, its clique, max, its clique]."""
    symb = A.symb
    if B is not None and B.symb is not symb:
        raise ValueError("%s: A and B live on different Symbolics" % what)
    _ensure(symb)
    dev = A.blkval.device
    w = torch.empty(int(symb.rowptr[-1]), dtype=torch.float64, device=dev)
    ext = torch.empty(4, dtype=torch.float64, device=dev)
    _chk(_lib.lib().csp_clique_eigvalsh(symb.handle, A.blkval.data_ptr(), None if B is None else B.blkval.data_ptr(),
                                        w.data_ptr(), ext.data_ptr(), _stream()), what)
    return w, ext


def clique_eigvalsh(A, B=None):
    """The spectra of the clique blocks: w, a float64 device tensor of length symb.rowptr[-1] whose entries
    w[rowptr[k]:rowptr[k + 1]] are the eigenvalues, ascending, of A_gg for clique k = g -- with B given, of the pencil
    (A_gg, B_gg), that is of B_gg^-1 A_gg.  A and B are cspmatrices on the same Symbolic (ValueError otherwise) read as
    symmetric matrices (of a supernode's diagonal block the lower triangle counts, as ``symm`` reads it); neither is written.
    ArithmeticError naming the clique when a B_gg is not positive definite, RuntimeError when a clique did not converge in
    30 Jacobi sweeps (a non-finite entry ends this way).  The same input gives the same bits (csp_clique_eigvalsh).
    A clique wider than 89 rows (126 without B) runs on one workgroup from device memory and is slow, unless
    ``tune(symb, TUNE_CEIG_WIDE, 65)`` sends it through the chip-wide route, which both forms take; errors and the clique they
    name are the same either way."""
    return _clique_eig(A, B, "clique_eigvalsh")[0]


def clique_extremes(A, B=None):
    """The (4,) float64 device tensor [smallest eigenvalue over all cliques, lowest clique attaining it, largest eigenvalue,
    lowest clique attaining that] of ``clique_eigvalsh(A, B)``.  It stays on the device: nothing waits for its values."""
    return _clique_eig(A, B, "clique_extremes")[1]


def clique_eig_sweeps(symb):
    """The most Jacobi sweeps any clique took in the last ``clique_eigvalsh``, ``clique_eigh`` or ``clique_project`` on symb
    (CSP_Q_CEIG_SWEEPS); for a clique on the wide route (TUNE_CEIG_WIDE) its block sweeps are counted."""
    out = ctypes.c_int64(0)
    _lib.lib().csp_symbolic_query(symb.handle, 20, ctypes.byref(out))
    return out.value


def clique_eig_wide(symb):
    """The number of cliques that took the wide route (``tune(symb, TUNE_CEIG_WIDE, order)``) in the last ``clique_eigvalsh``
    (with or without B, so ``clique_extremes``, ``cone_margin`` and ``max_step`` as well), ``clique_eigh``, ``clique_project`` or
    ``cone_project`` on symb (CSP_Q_CEIG_WIDE)."""
    out = ctypes.c_int64(0)
    _lib.lib().csp_symbolic_query(symb.handle, 21, ctypes.byref(out))
    return out.value


def slot_share(symb):
    """The most cliques any one workgroup served from its slot in device memory in the last completion (either pass),
    ``clique_eigvalsh``, ``max_step``, ``clique_eigh``, ``clique_project`` or ``cone_project`` chunk on symb: the largest
    ceil(cliques / workgroups) over the launches of that call that ran from slots in device memory, 0 when there was none
    (CSP_Q_SLOT_SHARE; above 1 only under ``tune(symb, TUNE_SLOT_DOUBLES, value)`` or with about a thousand such cliques)."""
    out = ctypes.c_int64(0)
    _lib.lib().csp_symbolic_query(symb.handle, 22, ctypes.byref(out))
    return out.value


def clique_eig_groups(symb):
    """The number of launch groups the wide cliques (TUNE_CEIG_WIDE) were split into in the last ``clique_eigvalsh`` (with or
    without B, so ``max_step`` as well; with B a clique's workspace holds B_gg too), ``clique_eigh``, ``clique_project`` or
    ``cone_project`` chunk on symb (CSP_Q_CEIG_GROUPS): 1 unless their workspace exceeds the limit of TUNE_SLOT_DOUBLES, 0
    without a wide clique."""
    out = ctypes.c_int64(0)
    _lib.lib().csp_symbolic_query(symb.handle, 23, ctypes.byref(out))
    return out.value


def cone_margin(X):
    """(m, clique) with m = min over the cliques g of lambda_min(X_gg), attained at `clique` (the lowest such).  X lies in
    the interior of the cone C_V of matrices with a positive definite completion exactly when m > 0, and X - t I stays
    inside exactly for t < m: m is the distance to the boundary along -I, -m the shift that brings an outside X to it."""
    e = _clique_eig(X, None, "cone_margin")[1].cpu()
    return float(e[0]), int(e[1])


def max_step(X, D, return_clique=False):
    """sup{alpha >= 0 : X + alpha D in int C_V} for X inside C_V: with mu the smallest eigenvalue over all cliques of the
    pencils (D_gg, X_gg) it is -1 / mu for mu < 0 and math.inf otherwise.  return_clique=True: (alpha, clique) with the
    binding clique (the one whose block of X + alpha D is singular; the clique of mu when alpha is inf).  ArithmeticError
    naming the clique when X is outside the cone (the Cholesky of X_gg inside the pencil), ValueError for different
    Symbolics.  One ``clique_eigvalsh``: no trial factorisation.  Under ``tune(symb, TUNE_CEIG_WIDE, 65)`` the wide cliques
    take the chip-wide route (the pencil form of it), which is what makes the call usable on a root of several hundred rows."""
    import math
    e = _clique_eig(D, X, "max_step")[1].cpu()
    mu = float(e[0])
    alpha = -1.0 / mu if mu < 0.0 else math.inf
    return (alpha, int(e[1])) if return_clique else alpha


def clique_ptr(symb):
    """The offsets of the packed clique blocks: a numpy int64 array qptr of length Nsn + 1.  A packed block tensor is a
    float64 device tensor of length qptr[-1] in which clique k holds an nf x nf column-major block at
    [qptr[k], qptr[k + 1]), nf = nn + na, rows and columns in the order of the clique's rows in symb.rowidx: the
    supernode's own columns, then its separator rows (csp_clique_ptr; host only, made once per Symbolic)."""
    if "clique_ptr" not in symb._cache:
        import numpy as np
        q = np.zeros(symb.Nsn + 1, dtype=np.int64)
        _chk(_lib.lib().csp_clique_ptr(symb.handle, q.ctypes.data), "clique_ptr")
        symb._cache["clique_ptr"] = q
    return symb._cache["clique_ptr"]


def clique_block(symb, Z, k):
    """The (nf, nf) view of block k of the packed block tensor Z, indexed [row, column] (no copy)."""
    q = clique_ptr(symb)
    _packed(symb, Z, "clique_block")
    nf = int(symb.rowptr[k + 1] - symb.rowptr[k])
    return Z[int(q[k]):int(q[k + 1])].view(nf, nf).t()


def _packed(symb, Z, what):
    """refuses what is not a packed block tensor of symb"""
    if not (torch.is_tensor(Z) and Z.dtype == torch.float64 and Z.dim() == 1 and Z.is_contiguous()
            and Z.shape[0] == int(clique_ptr(symb)[-1])):
        raise ValueError("%s: Z is not a contiguous float64 tensor of length clique_ptr(symb)[-1]" % what)
    return Z


def clique_gather(X):
    """The clique blocks of the cspmatrix X as a packed block tensor (``clique_ptr``): block k is the full symmetric
    X_gg of clique k = g (of a supernode's diagonal block the lower triangle counts).  X is not written.  One launch
    over all cliques behind the top-down gathers of the separator blocks (csp_clique_gather)."""
    symb = X.symb
    _ensure(symb)
    Z = torch.empty(int(clique_ptr(symb)[-1]), dtype=torch.float64, device=X.blkval.device)
    _chk(_lib.lib().csp_clique_gather(symb.handle, X.blkval.data_ptr(), Z.data_ptr(), _stream()), "clique_gather")
    return Z


def clique_scatter(symb, Z, reduce="sum"):
    """The cspmatrix P_V(sum_k E_k Z_k E_k^T) of the packed block tensor Z: every entry of the pattern is the sum
    (reduce="sum") or the mean (reduce="mean": the sum divided by ``clique_multiplicity``) of that entry over the cliques
    that hold it.  Only the lower triangle of each block is read; Z is not written.  The slots above the diagonal of a
    supernode's diagonal block are zero, as ``syr2k`` leaves them.  One launch per level of the clique tree, leaves first,
    every sum in a fixed order: the same input gives the same bits (csp_clique_scatter).  ValueError for another
    `reduce` or a tensor that is not a packed block tensor of symb."""
    if reduce not in ("sum", "mean"):
        raise ValueError("clique_scatter: reduce must be 'sum' or 'mean'")
    _ensure(symb)
    if not _packed(symb, Z, "clique_scatter").is_cuda:
        raise ValueError("clique_scatter: Z is not a device tensor")
    X = cspmatrix(symb, torch.empty(symb.blklen, dtype=torch.float64, device=Z.device))
    _chk(_lib.lib().csp_clique_scatter(symb.handle, Z.data_ptr(), X.blkval.data_ptr(), _stream()), "clique_scatter")
    if reduce == "mean":
        X.blkval /= clique_multiplicity(symb).to(Z.device)
    return X


def clique_decompose(L, out=None):
    """The factor as a sum of positive semidefinite clique blocks (Agler's theorem read off the supernodal factor): a packed
    block tensor Z (``clique_ptr``; the layout and dtype of ``clique_gather``).  L is a cspmatrix read as a factor, as
    ``cholesky`` leaves it.  Clique k has nn own columns and nf = nn + na rows and its panel P is nf x nn; with
    Pt[m, c] = P[m, c] for m >= c and 0 otherwise (the slots of blkval above the diagonal of a supernode's diagonal block
    are never read)
        Z_k[i, j] = sum over c = 0 .. min(i, j, nn - 1), ascending, of Pt[i, c] Pt[j, c],        0 <= i, j < nf,
    the full symmetric block, both triangles with the same bits.  Three properties: the blocks sum to the matrix,
    sum_k E_k Z_k E_k^T = L L^T, so ``clique_scatter(symb, Z, "sum")`` is ``llt(L)`` to rounding; every Z_k is positive
    semidefinite; and its rank is at most nn.  With ``clique_gather`` this is the duality of the two cones:
    <X, L L^T> = sum_k <X_gg, Z_k>.  On the factor that ``completion(X)`` leaves the call decomposes the inverse of the
    completion.  L is only read, and nothing cached for it is dropped or created.  One launch, two when the large fronts take
    the tile products (under ``tune(symb, TUNE_DETERMINISTIC, 1)`` everything runs on the plain FMA kernel), whatever the
    tree; no atomics, every entry has one writer: the same L gives the same bits from call to call.  out: a packed block
    tensor on the device that is written and returned (ValueError for anything else, or for one that shares memory with L).
    A positive semidefinite matrix that is singular has no factor here, and so is out of reach of this call: the
    decomposition of such a matrix (an optimal dual slack, say) needs a semidefinite sweep of its own
    (csp_clique_decompose)."""
    symb = L.symb
    _ensure(symb)
    if out is None:
        out = torch.empty(int(clique_ptr(symb)[-1]), dtype=torch.float64, device=L.blkval.device)
    elif not _packed(symb, out, "clique_decompose").is_cuda:
        raise ValueError("clique_decompose: out is not a device tensor")
    rc = _lib.lib().csp_clique_decompose(symb.handle, L.blkval.data_ptr(), out.data_ptr(), _stream())
    if rc == -1:
        raise ValueError("clique_decompose: out overlaps L, or the Symbolic is replicated or partitioned")
    _chk(rc, "clique_decompose")
    return out


def clique_multiplicity(symb):
    """Per slot of blkval the number of cliques that hold the entry, a float64 device tensor: the scatter of all-ones
    blocks, made once per Symbolic; 1 on the unused slots above the diagonal of a supernode's diagonal block."""
    if "clique_mult" not in symb._cache:
        _ensure(symb)
        ones = torch.ones(int(clique_ptr(symb)[-1]), dtype=torch.float64, device="cuda:%d" % symb._device)
        symb._cache["clique_mult"] = clique_scatter(symb, ones).blkval.clamp_(min=1.0)
    return symb._cache["clique_mult"]


def clique_eigh(A):
    """(w, Q): w as ``clique_eigvalsh(A)`` gives it (the same bits), Q a packed block tensor (``clique_ptr``) whose block
    k has as column j a unit eigenvector of A_gg for w[rowptr[k] + j]; ``clique_block(symb, Q, k)`` is that matrix.
    Signs and the basis inside a degenerate eigenspace are unspecified, but the same input gives the same bits.  A is
    not written.  RuntimeError when a clique did not converge in 30 Jacobi sweeps (a non-finite entry ends this way).
    A clique wider than 89 rows does not fit the on-chip memory of its workgroup and is slow: one workgroup works on it
    from device memory, unless ``tune(symb, TUNE_CEIG_WIDE, 65)`` sends it through the chip-wide block Jacobi (csp_clique_eigh)."""
    symb = A.symb
    _ensure(symb)
    dev = A.blkval.device
    w = torch.empty(int(symb.rowptr[-1]), dtype=torch.float64, device=dev)
    Q = torch.empty(int(clique_ptr(symb)[-1]), dtype=torch.float64, device=dev)
    _chk(_lib.lib().csp_clique_eigh(symb.handle, A.blkval.data_ptr(), w.data_ptr(), Q.data_ptr(), None, _stream()), "clique_eigh")
    return w, Q


def clique_project(X, lo=0.0, hi=math.inf, return_info=False):
    """Z, a packed block tensor (``clique_ptr``): block k is X_gg with its eigenvalues clipped to [lo, hi], the nearest
    matrix to X_gg in the Frobenius norm with lo I <= Z_k <= hi I.  With return_info=True: (Z, w, info), w the
    eigenvalues of the blocks of X as ``clique_eigh`` gives them and info an (Nsn, 2) float64 device tensor, per clique
    the number of eigenvalues changed and sum_j (clip(w_j) - w_j)^2 = |Z_k - X_gg|_F^2.
    This projects every clique block on its own.  It is NOT the Frobenius projection of X onto the cone C_V of
    PSD-completable matrices: it is the building block of the methods that compute it or solve over it (clique-splitting
    ADMM, Dykstra's alternating projections).  The blocks of Z disagree on the separators until they are averaged
    (``clique_scatter(symb, Z, "mean")``).
    A block whose spectrum lies inside [lo, hi] comes back as the bits of ``clique_gather(X)``; every block is exactly
    symmetric; the work grows with the number of eigenvalues clipped.  Wide cliques are slow: beyond 89 rows one workgroup
    works on the block from device memory.  X is not written; lo = -inf and hi = inf are allowed.  ValueError unless
    lo <= hi (a NaN bound included), RuntimeError when a clique did not converge in 30 Jacobi sweeps (a non-finite entry
    ends this way; csp_clique_project)."""
    lo, hi = float(lo), float(hi)
    if not lo <= hi:
        raise ValueError("clique_project: needs lo <= hi (got %r, %r)" % (lo, hi))
    symb = X.symb
    _ensure(symb)
    dev = X.blkval.device
    Z = torch.empty(int(clique_ptr(symb)[-1]), dtype=torch.float64, device=dev)
    w = torch.empty(int(symb.rowptr[-1]), dtype=torch.float64, device=dev) if return_info else None
    info = torch.empty((symb.Nsn, 2), dtype=torch.float64, device=dev)
    _chk(_lib.lib().csp_clique_project(symb.handle, X.blkval.data_ptr(), lo, hi, Z.data_ptr(), None if w is None else w.data_ptr(),
                                       info.data_ptr(), _stream()), "clique_project")
    return (Z, w, info) if return_info else Z


CONE_CHUNK = 8        # iterations of cone_project between two looks at the residuals


def cone_looks(maxit, chunk=CONE_CHUNK):
    """[(it0, nsteps)] of the calls of csp_cone_project_steps up to maxit iterations: the looks come after iteration 1 (an
    input inside the cone is known by then) and then every `chunk`, at 1 + chunk, 1 + 2 chunk, ..., and at maxit; one more
    look after iteration 2 catches the separable cases (one clique, disjoint cliques), which are done by then."""
    ends = sorted({1, min(2, maxit), maxit} | set(range(1 + chunk, maxit, chunk)))
    return [(b, e - b) for b, e in zip([0] + ends, ends) if e > b]


def cone_weights(symb):
    """Per slot of blkval the weight of the entry in ``dot``: 1 on the diagonal of the matrix, 2 below it, 0 on the unused
    slots above the diagonal of a supernode's diagonal block.  A float64 device tensor, made once per Symbolic."""
    if "cone_weights" not in symb._cache:
        import numpy as np
        _ensure(symb)
        nn, na = symb.clique_sizes()
        w = np.empty(symb.blklen)
        for k in range(symb.Nsn):
            i = np.arange(nn[k] + na[k])[:, None]
            j = np.arange(nn[k])[None, :]
            w[symb.blkptr[k]:symb.blkptr[k + 1]] = np.where(i > j, 2.0, np.where(i == j, 1.0, 0.0)).ravel(order="F")
        symb._cache["cone_weights"] = torch.from_numpy(w).to("cuda:%d" % symb._device)
    return symb._cache["cone_weights"]


def cone_project(A, cone="primal", tol=1e-8, maxit=500, rho=1.0, relax=1.7, U0=None, return_info=False):
    """The nearest point to the cspmatrix A, in the norm of ``dot``, of the cone K of matrices on the pattern that have a
    positive semidefinite completion (cone="primal": every clique block of the result is PSD), or of its dual K*, the
    positive semidefinite matrices with the pattern (cone="dual"), which is A + P_K(-A) by Moreau's decomposition.  A new
    cspmatrix on the Symbolic of A; A is read as ``symm`` reads it and not written; the unused slots of the result are 0.

    ``clique_project`` followed by an average is NOT this projection; this is the iteration that makes it one, a
    clique-splitting ADMM with penalty rho and over-relaxation relax that runs on the device (csp_cone_project_steps): per
    iteration the clique blocks of X are gathered, every clique k forms T_k from X_gg, its copy Z_k and its scaled dual U_k,
    keeps the negative part of T_k as U_k and the positive part as Z_k, and X is averaged again with A.  The host looks at
    the residuals after the first and the second iteration and then every CONE_CHUNK = 8 (``cone_looks``), and stops when both the primal residual
    sqrt(sum_k |X_gg - Z_k|_F^2) and the dual one |X_new - X_old| are at most tol max(1, |A|).  X - A = -rho sum_k E_k U_k E_k^T
    is in K* by construction, whatever the accuracy: the result carries its own certificate (X in K, X - A in K*,
    <X, X - A> = 0, each to about the residuals).

    This is a first-order method.  A noisy point near the cone (a PSD-completable matrix plus noise on the pattern, an iterate
    to be repaired) converges to 1e-8 in tens of iterations on patterns of tens of cliques; a matrix without structure (random
    symmetric entries on a band, say) can take thousands, and so can the noisy kind on a pattern of thousands of cliques
    (DESIGN.md section 21, 8073 cliques: 1e-4 after 16 iterations, 1e-5 after 428, 1e-6 after 1998).  Reaching maxit is not an error: the call returns what it has with converged False.  An A inside
    K comes back bit for bit after one iteration.  Wide cliques are slow, now in every iteration: beyond 89 rows one
    workgroup works on the block from device memory, and with a root of several hundred rows the call is not usable --
    unless ``tune(A.symb, TUNE_CEIG_WIDE, 65)`` sends the cliques of at least that order through the chip-wide block Jacobi
    (csrc/front_ceigw.hip) in every iteration: a fixed chain of launches, nothing read back inside a chunk.  With the tune
    at 0 (the default), or with no clique that wide, the call gives the bits it gives without it.

    return_info=True: (X, info) with iterations, converged, primal and dual (the residuals over max(1, |A|)), distance
    (|X - A|), hist (a device tensor (iterations, 4): the squares of the two residuals, the negative eigenvalues of all T_k,
    1 + the lowest clique that failed), U (the packed scaled duals, each block negative semidefinite, the U0 of a later call
    with the same rho on a nearby A, which then starts from X = A - rho sum_k E_k U0_k E_k^T), sweeps (the most sweeps of a
    clique in any iteration: Jacobi sweeps, or block sweeps of a clique on the wide route, whichever is larger) and wide (the
    number of cliques that took the wide route).
    ValueError for rho <= 0, relax outside (0, 2), tol < 0, maxit < 1, another `cone`, or a U0 that is not a packed block
    tensor on the device of A; NotImplementedError on a replicated or sharded Symbolic; RuntimeError naming the clique when a
    Jacobi iteration did not converge (a non-finite entry of A ends this way), seen at the next look."""
    if cone not in ("primal", "dual"):
        raise ValueError("cone_project: cone must be 'primal' or 'dual'")
    tol, rho, relax, maxit = float(tol), float(rho), float(relax), int(maxit)
    if not rho > 0.0 or not 0.0 < relax < 2.0 or not tol >= 0.0 or maxit < 1:
        raise ValueError("cone_project: needs rho > 0, 0 < relax < 2, tol >= 0 and maxit >= 1")
    symb = A.symb
    if getattr(symb, "copies", 1) != 1:
        raise NotImplementedError("cone_project has no form on a replicated Symbolic")
    _ensure(symb)
    dev = A.blkval.device
    if U0 is not None and (_packed(symb, U0, "cone_project").device != dev or not U0.is_cuda):
        raise ValueError("cone_project: U0 is not on the device of A")
    wt = cone_weights(symb).to(dev)
    used = wt > 0
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    a = cspmatrix(symb, torch.where(used, A.blkval if cone == "primal" else -A.blkval, zero))
    if U0 is None:                                     # X = A, U = 0, W = the blocks of A: the Z before the first iteration
        X = a.copy()
        W = clique_gather(a)
        U = torch.zeros_like(W)
    else:                                              # the X that belongs to U0 at a fixed point, A - rho sum_k E_k U_k E_k^T
        U = U0.clone()
        X = cspmatrix(symb, torch.where(used, a.blkval - rho * clique_scatter(symb, U).blkval, zero))
        W = clique_gather(X) - U
    hist = torch.zeros((maxit, 4), dtype=torch.float64, device=dev)
    scale = max(1.0, math.sqrt(float((wt * a.blkval * a.blkval).sum())))
    lib, h = _lib.lib(), symb.handle
    done, converged, rows = 0, False, None
    for it0, ns in cone_looks(maxit):
        rc = lib.csp_cone_project_steps(h, a.blkval.data_ptr(), X.blkval.data_ptr(), U.data_ptr(), W.data_ptr(), rho, relax, it0, ns,
                                        hist.data_ptr(), _stream())
        if rc == -1:
            raise NotImplementedError("cone_project has no form on a sharded or replicated context")
        _chk(rc, "cone_project")
        X.touched()
        done = it0 + ns
        rows = hist[it0:done].cpu()                    # the one read-back of a look
        bad = torch.nonzero(rows[:, 3])
        if len(bad):
            i = int(bad[0])
            raise RuntimeError("cone_project: the Jacobi iteration of clique %d did not converge in 30 sweeps (block sweeps on the "
                               "wide route) at iteration %d (a non-finite entry?)" % (int(rows[i, 3]) - 1, it0 + i + 1))
        r2, s2 = float(rows[-1, 0]), float(rows[-1, 1])
        if it0 == 0 and U0 is None and float(rows[0, 2]) == 0.0:       # A is inside the cone: its own bits
            X.blkval.copy_(a.blkval)
            converged = True
            break
        if max(math.sqrt(r2), math.sqrt(s2)) <= tol * scale:
            converged = True
            break
    if cone == "dual":
        X = cspmatrix(symb, torch.where(used, A.blkval + X.blkval, zero))
    if not return_info:
        return X
    sw = ctypes.c_int64(0)
    _chk(lib.csp_cone_project_sweeps(h, ctypes.byref(sw), _stream()), "cone_project")
    d = X.blkval - torch.where(used, A.blkval, zero)
    return X, {"iterations": done, "converged": converged, "primal": math.sqrt(float(rows[-1, 0])) / scale,
               "dual": math.sqrt(float(rows[-1, 1])) / scale, "distance": math.sqrt(float((wt * d * d).sum())),
               "hist": hist[:done], "U": U, "sweeps": int(sw.value), "wide": clique_eig_wide(symb)}


LANCZOS_JMAX = 128    # csrc/front_lanczos.hip: LZ_JMAX
LANCZOS_CHUNK = 8     # steps between two looks at the Ritz values
_LANCZOS_SEED = 20240607


def lanczos_maxit(n, maxit):
    """The Krylov dimension a call may reach: maxit clamped to 1 .. min(n, LANCZOS_JMAX)."""
    return max(1, min(int(maxit), int(n), LANCZOS_JMAX))


def lanczos_chunks(jmax, chunk=LANCZOS_CHUNK):
    """[(j0, nsteps)] of the calls of csp_lanczos_steps up to dimension jmax: chunks of `chunk`, the last one shorter."""
    return [(j0, min(chunk, jmax - j0)) for j0 in range(0, jmax, chunk)]


def lanczos_layout(n, jmax):
    """(state length, offset of basis row 0, row stride, total length) of the workspace of csp_lanczos_steps in doubles
    (include/smcp_amd.h)."""
    up8 = lambda x: (x + 7) & ~7
    state = up8(16 + 2 * jmax + 1)
    basis = state + 2 * up8(128 * jmax) + up8(-(-n // 256))
    ld = up8(n)
    return state, basis, ld, basis + (jmax + 3) * ld


def lanczos_default_v0(n):
    """The start vector used when none is given: standard normal from a fixed seed, made on the host."""
    import numpy as np
    return np.random.default_rng(_LANCZOS_SEED).standard_normal(n)


def lanczos_converged(resid, theta_min, theta_max, tol, steps, n, invariant):
    """The stopping rule: the residual estimate of the wanted end is below tol max(|theta_min|, |theta_max|), or the Krylov
    space is exhausted (steps == n) or invariant (the iteration broke down)."""
    return bool(invariant or steps >= n or resid <= tol * max(abs(theta_min), abs(theta_max)))


def lanczos_extremes(L, D=None, tol=1e-10, maxit=64, v0=None, which="min", return_work=False):
    """The extreme Ritz values of L^-1 D L^-T (D a cspmatrix on the Symbolic of L, read as symmetric exactly as ``symm`` reads
    it) or, with D None, of L^-T L^-1 = (L L^T)^-1, by Lanczos with full reorthogonalisation on the device
    (csp_lanczos_steps / csp_lanczos_ritz): chunks of eight steps, then one look at the four numbers of the state block.
    Returns a dict: theta_min, theta_max, resid_min, resid_max (the estimates beta_j |bottom component of the Ritz vector|),
    steps, invariant (the iteration broke down: the Ritz values are eigenvalues), converged (``lanczos_converged`` for the end
    named by `which`, 'min' or 'max').  maxit is clamped to min(n, LANCZOS_JMAX); v0 is a start vector of length n in the
    PERMUTED order (sequence, numpy array or tensor; default ``lanczos_default_v0``).  The same inputs give the same bits.
    L and D are not written.  ValueError for different Symbolics or a v0 of the wrong length."""
    import numpy as np
    symb = L.symb
    if D is not None and D.symb is not symb:
        raise ValueError("lanczos_extremes: L and D live on different Symbolics")
    if which not in ("min", "max"):
        raise ValueError("lanczos_extremes: which must be 'min' or 'max'")
    n = int(symb.n)
    if v0 is None:
        v0 = lanczos_default_v0(n)
    if isinstance(v0, torch.Tensor):
        v0t = v0.detach().to(dtype=torch.float64).reshape(-1)
    else:
        v0t = torch.from_numpy(np.ascontiguousarray(np.asarray(v0, dtype=np.float64).reshape(-1)))
    if v0t.numel() != n:
        raise ValueError("lanczos_extremes: v0 has %d entries, the pattern has %d rows" % (v0t.numel(), n))
    _ensure(symb)
    lib = _lib.lib()
    _fit_workspace(symb, int(symb.sepptr[-1]), 1)
    if D is not None:
        _fit_workspace(symb, int(lib.csp_symm_positions(symb.handle)), 1)
    jmax = lanczos_maxit(n, maxit)
    state_len, basis, ld, total = lanczos_layout(n, jmax)
    assert total == int(lib.csp_lanczos_work_len(n, jmax))
    dev = L.blkval.device
    work = torch.zeros(total, dtype=torch.float64, device=dev)
    work[basis:basis + n].copy_(v0t)
    h, Lp, Dp, wp = symb.handle, L.blkval.data_ptr(), None if D is None else D.blkval.data_ptr(), work.data_ptr()
    info = None
    for j0, ns in lanczos_chunks(jmax):
        _chk(lib.csp_lanczos_steps(h, Lp, Dp, wp, jmax, j0, ns, _stream()), "lanczos_extremes")
        _chk(lib.csp_lanczos_ritz(h, wp, jmax, _stream()), "lanczos_extremes")
        s = work[:8].cpu().tolist()                  # the one read-back of a chunk: status, steps and the four outputs
        if s[0] == 2.0:
            raise RuntimeError("lanczos_extremes: a non-finite value at step %d (is L a Cholesky factor?)" % int(s[2]))
        info = {"theta_min": s[4], "resid_min": s[5], "theta_max": s[6], "resid_max": s[7], "steps": int(s[1]),
                "invariant": s[0] == 1.0}
        info["converged"] = lanczos_converged(info["resid_" + which], s[4], s[6], tol, info["steps"], n, info["invariant"])
        if info["converged"]:
            break
    if return_work:
        info["work"], info["jmax"] = work, jmax
    return info


def dual_max_step(L, D, tol=1e-10, maxit=64, v0=None, return_info=False):
    """sup{alpha >= 0 : L L^T + alpha D is positive definite} for the factor L that ``cholesky`` leaves and a direction D on
    the same Symbolic (ValueError otherwise), read as symmetric exactly as ``symm`` reads it: -1 / theta_min when the
    smallest Ritz value theta_min of L^-1 D L^-T is negative, math.inf otherwise (``lanczos_extremes``).  return_info=True:
    (alpha, info) with info the dict of ``lanczos_extremes`` plus alpha_safe = -1 / (theta_min - resid_min), or inf.

    What is rigorous: Ritz values lie inside the spectrum, so theta_min is never below the smallest eigenvalue and the
    returned alpha is never BELOW the true step, up to rounding -- it is an upper estimate that decreases to the step as the
    iteration converges.  What is not: alpha_safe is a lower bound of the step only once theta_min has converged to the
    SMALLEST eigenvalue (then that eigenvalue is no further than resid_min below theta_min); the residual estimate says
    that a Ritz pair has converged to SOME eigenvalue, which indicates but does not prove it, and `converged` reports only
    that estimate.  A caller who needs a guarantee takes a fraction of alpha_safe or confirms it with one ``cholesky``."""
    import math
    info = lanczos_extremes(L, D, tol, maxit, v0, "min")
    th = info["theta_min"]
    alpha = -1.0 / th if th < 0.0 else math.inf
    lo = th - info["resid_min"]
    info["alpha_safe"] = -1.0 / lo if lo < 0.0 else math.inf
    return (alpha, info) if return_info else alpha


def dual_margin(L, tol=1e-10, maxit=64, v0=None, return_info=False):
    """lambda_min(L L^T) for the factor L that ``cholesky`` leaves, as 1 / theta_max of L^-T L^-1 (``lanczos_extremes``
    without D): S = L L^T is positive definite, and S - t I stays so exactly for t < margin -- the dual counterpart of
    ``cone_margin``.  return_info=True: (margin, info) with info the dict of ``lanczos_extremes`` (converged refers to
    theta_max) plus cond = theta_max / theta_min, the Ritz estimate of the condition number of S (1 / theta_min estimates
    lambda_max(S)).  theta_max is never above the largest eigenvalue of S^-1, so the margin returned is never below the
    true one, up to rounding; 1 / (theta_max + resid_max) is a lower bound only once theta_max has converged to the largest
    eigenvalue, which the residual estimate indicates and does not prove."""
    info = lanczos_extremes(L, None, tol, maxit, v0, "max")
    margin = 1.0 / info["theta_max"]
    info["cond"] = info["theta_max"] / info["theta_min"]
    return (margin, info) if return_info else margin


def edm_dense(symb, Y, perm=None):
    """The completed EDM as a dense n x n device tensor: D[i, j] = |Y[p_i] - Y[p_j]|^2 (csp_edm_dense) for Y of
    edmcompletion, p = perm (int64 device tensor of row indices of Y; None: the identity, the permuted order)."""
    _ensure(symb)
    n, r = Y.shape
    Y = Y.contiguous()
    out = torch.empty((n, n), dtype=torch.float64, device=Y.device)
    pp = 0 if perm is None else perm.data_ptr()
    _chk(_lib.lib().csp_edm_dense(symb.handle, Y.data_ptr() if r else 0, max(r, 1), r, pp, out.data_ptr(), n, _stream()),
         "edm_dense")
    return out


_ADJ = {False: 0, True: 1, None: 2}


def hessian(L, Y, U, adj=False, inv=False):
    """hessian(L, Y, U, adj, inv); U is a cspmatrix, a list of cspmatrices, or a
    (nrhs x ldu) torch tensor whose rows are blkvals (the batched form)."""
    symb = L.symb
    _ensure(symb)
    lib = _lib.lib()
    sync_cache(symb, L, Y)
    a, i = _ADJ[adj], 1 if inv else 0
    if isinstance(U, cspmatrix):
        U.touched()
        _chk(lib.csp_hessian(symb.handle, L.blkval.data_ptr(), Y.blkval.data_ptr(), U.blkval.data_ptr(), 1,
                             symb.blklen, a, i, _stream()), "hessian")
    elif isinstance(U, torch.Tensor):
        assert U.dim() == 2 and U.stride(1) == 1 and U.shape[1] >= symb.blklen
        _chk(lib.csp_hessian(symb.handle, L.blkval.data_ptr(), Y.blkval.data_ptr(), U.data_ptr(), U.shape[0],
                             U.stride(0), a, i, _stream()), "hessian")
    else:
        for Uj in U:
            Uj.touched()
            _chk(lib.csp_hessian(symb.handle, L.blkval.data_ptr(), Y.blkval.data_ptr(), Uj.blkval.data_ptr(), 1,
                                 symb.blklen, a, i, _stream()), "hessian")


def _fit_workspace(symb, positions, k):
    """Grows max_rhs so that `positions` partial results for each of k columns fit the workspace (the library returns
    SMCP_ENOMEM otherwise)."""
    need = -(-positions * k // max(1, 2 * symb.blklen))
    if symb._max_rhs < need:
        symb.device_init(symb._device, need)


def trsm(L, B, trans="N"):
    """B: (n x k) column-major dense right-hand side given as a torch tensor of shape (k, n)
    (row r of the tensor = column r of B), rows in the PERMUTED order."""
    symb = L.symb
    _ensure(symb)
    assert B.dim() == 2 and B.stride(1) == 1 and B.shape[1] == symb.n
    _fit_workspace(symb, int(symb.sepptr[-1]), B.shape[0])
    _chk(_lib.lib().csp_trsm(symb.handle, L.blkval.data_ptr(), B.data_ptr(), B.shape[0], B.stride(0),
                             1 if trans in ("T", 1, True) else 0, _stream()), "trsm")


def trmm(L, B, alpha=1.0, trans="N"):
    """chompack.trmm(L, B, alpha, trans): B <- alpha L B ('N') or alpha L^T B ('T'; also 1, True), with L read as a
    lower-triangular factor (as ``cholesky`` / ``completion`` leave it) and B laid out as for ``trsm``: a float64 device
    tensor of shape (k, n) with stride(1) == 1 whose row r is column r of B, rows in the PERMUTED order; the entries
    B[r, n:stride(0)] of a padded tensor are not touched.  L is not changed.  Two or three launches whatever the tree, and
    the same arguments give the same bits from call to call (csp_trmm)."""
    symb = L.symb
    _ensure(symb)
    assert B.dim() == 2 and B.stride(1) == 1 and B.shape[1] == symb.n
    _fit_workspace(symb, int(symb.sepptr[-1]), B.shape[0])
    _chk(_lib.lib().csp_trmm(symb.handle, L.blkval.data_ptr(), B.data_ptr(), B.shape[0], B.stride(0), float(alpha),
                             1 if trans in ("T", 1, True) else 0, _stream()), "trmm")


def _dense_block(symb, B, what):
    assert B.dim() == 2 and B.stride(1) == 1 and B.shape[1] == symb.n and B.shape[0] >= 1, what
    assert B.shape[0] == 1 or B.stride(0) >= symb.n, what
    assert B.dtype == torch.float64, what
    return B.stride(0) if B.shape[0] > 1 else max(B.stride(0), symb.n)


def syr2k(X, U, V, alpha=1.0, beta=1.0):
    """X <- beta X + alpha P_V(U V^T + V U^T), in place: the rank-2k form of chompack.syr2.  U and V are dense n x k blocks
    laid out as for ``trsm`` / ``trmm``: float64 device tensors of shape (k, n) with stride(1) == 1 and stride(0) >= n whose
    row r is column r of the block, rows in the PERMUTED order.  They are not written; V may be U.  Every slot of X.blkval is
    written (those outside the pattern as exactly 0.0), X is not read when beta == 0, U and V are not read when alpha == 0,
    and the same arguments give the same bits from call to call.  One or two launches whatever the tree (csp_syr2k)."""
    _rank_update(X, U, V, alpha, beta, "syr2k")


def syrk(X, U, alpha=1.0, beta=1.0):
    """X <- beta X + alpha P_V(U U^T), in place, for U as in ``syr2k``: P_V(Y Y^T) of a low-rank factor (the Y of
    ``mrcompletion`` as ``Y.t().contiguous()``) without an n x n intermediate."""
    _rank_update(X, U, None, alpha, beta, "syrk")


def _rank_update(X, U, V, alpha, beta, name):
    """csp_syr2k; V None: the rank-k form (V absent)."""
    symb = X.symb
    ldu = _dense_block(symb, U, "U")
    ldv = 0 if V is None else _dense_block(symb, V, "V")
    assert V is None or U.shape[0] == V.shape[0]
    assert U.is_cuda and (V is None or V.is_cuda)
    _ensure(symb)
    X.touched()
    try:
        _chk(_lib.lib().csp_syr2k(symb.handle, X.blkval.data_ptr(), U.data_ptr(), None if V is None else V.data_ptr(),
                                  U.shape[0], ldu, ldv, float(alpha), float(beta), _stream()), name)
    finally:
        note_cache(symb, X)


def syr2(X, y, z, alpha=1.0, beta=1.0):
    """chompack.syr2(X, y, z, alpha, beta): X <- beta X + alpha P_V(y z^T + z y^T) for 1-D float64 device tensors y, z of
    length n in the PERMUTED order (``syr2k`` with k = 1)."""
    assert y.dim() == 1 and z.dim() == 1
    syr2k(X, y.unsqueeze(0), z.unsqueeze(0), alpha, beta)


def symm(X, B, C=None, alpha=1.0, beta=0.0):
    """C <- alpha X B + beta C for the cspmatrix X read as a symmetric matrix (of the diagonal block of a supernode only the
    lower triangle counts) and dense n x k blocks B, C laid out as for ``trsm`` / ``trmm`` / ``syr2k``: float64 device
    tensors of shape (k, n) with stride(1) == 1 and stride(0) >= n whose row r is column r of the block, rows in the
    PERMUTED order.  Returns C; ``C=None`` allocates a contiguous (k, n) tensor and needs beta == 0.  X and B are not
    written, C must not overlap B, and a term whose factor is zero is left out: beta == 0 does not read C, alpha == 0
    reads neither X nor B.  Nothing cached for X is dropped.  Two or three launches whatever the tree, and the same
    arguments give the same bits from call to call (csp_symm)."""
    symb = X.symb
    ldb = _dense_block(symb, B, "B")
    assert B.is_cuda
    if C is None:
        assert beta == 0, "C=None needs beta == 0"
        C = torch.empty((B.shape[0], symb.n), dtype=torch.float64, device=B.device)
    ldc = _dense_block(symb, C, "C")
    assert C.is_cuda and C.shape[0] == B.shape[0]
    _ensure(symb)
    lib = _lib.lib()
    _fit_workspace(symb, int(lib.csp_symm_positions(symb.handle)), B.shape[0])
    _chk(lib.csp_symm(symb.handle, X.blkval.data_ptr(), B.data_ptr(), ldb, C.data_ptr(), ldc, B.shape[0], float(alpha),
                      float(beta), _stream()), "symm")
    return C


LOWRANK_KMAX = 64
_LR_OPS = {"F": 0, "FT": 1, "FINV": 2, "FINVT": 3, "MINV": 4, "M": 5}     # include/smcp_amd.h: CSP_LR_*


def _lowrank_block(symb, B, what):
    """The checks of a (kb, n) block of the low-rank calls: ValueError, before the device is touched."""
    if not isinstance(B, torch.Tensor) or B.dim() != 2:
        raise ValueError("%s: a 2-D torch tensor of shape (k, n) is needed" % what)
    if B.shape[0] < 1:
        raise ValueError("%s: at least one column is needed, got %d" % (what, B.shape[0]))
    if B.dtype != torch.float64:
        raise ValueError("%s: float64 is needed, got %s" % (what, B.dtype))
    if B.shape[1] != symb.n:
        raise ValueError("%s: %d rows, the pattern has %d" % (what, B.shape[1], symb.n))
    if B.stride(1) != 1 or (B.shape[0] > 1 and B.stride(0) < symb.n):
        raise ValueError("%s: stride(1) == 1 and stride(0) >= n are needed" % what)
    if not B.is_cuda:
        raise ValueError("%s: a device tensor is needed" % what)
    return B.stride(0) if B.shape[0] > 1 else max(B.stride(0), symb.n)


class LowRankFactor:
    """M = L L^T + V diag(a) V^T = F F^T held as the chordal factor L, W = L^-1 V and a k x k state on the device
    (``lowrank_factor``).  F = L (I + W C W^T) is neither triangular nor unique.  All methods work in place on float64
    device tensors of shape (kb, n), any kb, laid out as for ``trsm`` / ``trmm`` (row r of the tensor is column r of the
    block, stride(1) == 1, rows in the PERMUTED order; the entries B[r, n:stride(0)] of a padded tensor are not touched).
    L, W and the state are only read, and the same arguments give the same bits from call to call.

    The object REFERS to L: changing ``L.blkval`` afterwards invalidates it (W and the state were derived from the old
    factor); build a new one with ``lowrank_factor``."""

    def __init__(self, L, W, state):
        self.L, self.W, self.state = L, W, state
        self.k = int(W.shape[0])

    def _apply(self, B, op, what):
        symb = self.L.symb
        ldb = _lowrank_block(symb, B, what)
        if B.device != self.W.device:
            raise ValueError("%s: B is on %s, the factor on %s" % (what, B.device, self.W.device))
        _ensure(symb)
        _fit_workspace(symb, int(symb.sepptr[-1]), min(B.shape[0], 512))
        _chk(_lib.lib().csp_lowrank_apply(symb.handle, self.L.blkval.data_ptr(), self.W.data_ptr(), self.W.stride(0), self.k,
                                          self.state.data_ptr(), B.data_ptr(), ldb, B.shape[0], _LR_OPS[op], _stream()), what)

    def trmm(self, B, trans="N"):
        """B <- F B ('N') or F^T B ('T'; also 1, True)."""
        self._apply(B, "FT" if trans in ("T", 1, True) else "F", "LowRankFactor.trmm")

    def trsm(self, B, trans="N"):
        """B <- F^-1 B ('N') or F^-T B ('T'; also 1, True)."""
        self._apply(B, "FINVT" if trans in ("T", 1, True) else "FINV", "LowRankFactor.trsm")

    def solve(self, B):
        """B <- M^-1 B."""
        self._apply(B, "MINV", "LowRankFactor.solve")

    def mul(self, B):
        """B <- M B."""
        self._apply(B, "M", "LowRankFactor.mul")

    def logdet(self):
        """log det M."""
        out = ctypes.c_double(0.0)
        _chk(_lib.lib().csp_lowrank_logdet(self.L.symb.handle, self.L.blkval.data_ptr(), self.state.data_ptr(), ctypes.byref(out),
                                           _stream()), "LowRankFactor.logdet")
        return out.value


def lowrank_factor(L, V, a=None):
    """The factor of M = L L^T + V diag(a) V^T as a ``LowRankFactor``: L a Cholesky factor on the pattern (as ``cholesky`` /
    ``completion`` leave it), V a float64 device tensor of shape (k, n), 1 <= k <= 64, with stride(1) == 1, laid out as for
    ``trsm`` / ``trmm`` (row j is column j of V, rows in the PERMUTED order), a a sequence of k floats (None: all ones; a
    negative entry is a downdate, a zero entry leaves its column out).  V is not written: the object keeps its own
    W = L^-1 V, 8 n k bytes beside L, and refers to L.  Nothing n x n is formed.  ValueError for a bad k, shape, dtype or
    device, raised before the device is touched; ArithmeticError naming the column when M is not positive definite."""
    symb = L.symb
    if not isinstance(V, torch.Tensor) or V.dim() != 2:
        raise ValueError("lowrank_factor: V must be a 2-D torch tensor of shape (k, n)")
    k = int(V.shape[0])
    if k < 1 or k > LOWRANK_KMAX:
        raise ValueError("lowrank_factor: k = %d is outside 1 .. %d" % (k, LOWRANK_KMAX))
    _lowrank_block(symb, V, "lowrank_factor: V")
    coef = None
    if a is not None:
        coef = [float(x) for x in a]
        if len(coef) != k or not all(x == x and abs(x) != float("inf") for x in coef):
            raise ValueError("lowrank_factor: a must hold %d finite numbers" % k)
    if not L.blkval.is_cuda or L.blkval.device != V.device:
        raise ValueError("lowrank_factor: L and V must be on the same device")
    _ensure(symb)
    lib = _lib.lib()
    _fit_workspace(symb, int(symb.sepptr[-1]), k)
    W = V.clone(memory_format=torch.contiguous_format)
    state = torch.zeros(int(lib.csp_lowrank_state_len(k)), dtype=torch.float64, device=V.device)
    ah = None if coef is None else (ctypes.c_double * k)(*coef)
    rc = lib.csp_lowrank_factor(symb.handle, L.blkval.data_ptr(), W.data_ptr(), W.stride(0), k, ah, state.data_ptr(), _stream())
    if rc > 0:
        raise ArithmeticError("lowrank_factor: L L^T + V diag(a) V^T is not positive definite (column %d)" % (rc - 1))
    _chk(rc, "lowrank_factor")
    return LowRankFactor(L, W, state)


CHOL_UPDATE_KMAX = 64
_E_SUPPORT, _E_VALUE = -8, -9        # include/smcp_amd.h: SMCP_ESUPPORT, SMCP_EVALUE


def clique_support(symb, idx):
    """The clique k whose rows [N_k; A_k] contain every index of `idx` (PERMUTED order) and whose supernode N_k holds the
    smallest of them, or -1 when there is none: the clique that a column of V with that support selects in ``chol_update``,
    which accepts the column exactly when this is not -1.  Needs no device (csp_clique_support)."""
    import numpy as np
    ix = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).ravel())
    return int(_lib.lib().csp_clique_support(symb.handle, ix.shape[0], ix.ctypes.data_as(ctypes.c_void_p)))


def chol_update(L, V, a=None):
    """Rank-k update and downdate of the factor itself: L (a ``cspmatrix`` as ``cholesky`` leaves it) is overwritten in place
    so that L L^T becomes L L^T + V diag(a) V^T.  V: a float64 device tensor of shape (k, >= n), 1 <= k <= 64, with
    stride(1) == 1, laid out as for ``trsm`` / ``trmm`` / ``lowrank_factor`` (row j is column j of V, rows in the PERMUTED
    order); it is not written and its entries beyond n are neither read nor touched.  a: k floats (None: all ones); a
    negative entry is a downdate, a zero entry leaves its column out.

    Every column of V must have its support inside one clique: with j0 its first nonzero and s the supernode of column
    j0, all its nonzeros lie in the rows of clique s (``clique_support`` finds s, or -1).  That is the condition under which
    the new factor has no fill; ``lowrank_factor`` takes any V and leaves L alone.  A column that violates it, or a NaN or
    an infinity in V or a, is a ValueError naming the column, and L is then bit for bit what it was: the columns are checked
    on the device before anything is written.

    The columns with a_j > 0 are taken first, then those with a_j < 0, each group in the caller's order; the arithmetic is
    that of k successive rank-one updates, cliques outside the leaf-to-root paths of the columns are not written, and the
    same arguments give the same bits.  Two launches whatever the tree and k.  What the library had derived from the old
    contents of L (the inverse-form factor a ``hessian`` left behind) is dropped.

    ArithmeticError naming the column when a downdate leaves the cone (l_cc^2 - w_c^2 <= 0).  L IS THEN NOT USABLE, as
    after a failed ``cholesky``: keep ``L.copy()`` where that matters."""
    symb = L.symb
    if not isinstance(V, torch.Tensor) or V.dim() != 2:
        raise ValueError("chol_update: V must be a 2-D torch tensor of shape (k, n)")
    k = int(V.shape[0])
    if k < 1 or k > CHOL_UPDATE_KMAX:
        raise ValueError("chol_update: k = %d is outside 1 .. %d" % (k, CHOL_UPDATE_KMAX))
    if V.dtype != torch.float64:
        raise ValueError("chol_update: float64 is needed, got %s" % V.dtype)
    if V.shape[1] < symb.n:
        raise ValueError("chol_update: V has %d rows, the pattern has %d" % (V.shape[1], symb.n))
    if V.stride(1) != 1 or (k > 1 and V.stride(0) < symb.n):
        raise ValueError("chol_update: stride(1) == 1 and stride(0) >= n are needed")
    if not V.is_cuda or not L.blkval.is_cuda or L.blkval.device != V.device:
        raise ValueError("chol_update: L and V must be on the same device")
    ah = None
    if a is not None:
        coef = [float(x) for x in a]
        if len(coef) != k:
            raise ValueError("chol_update: a must hold %d numbers" % k)
        for j, x in enumerate(coef):
            if x != x or abs(x) == float("inf"):
                raise ValueError("chol_update: the coefficient of column %d is not finite" % j)
        ah = (ctypes.c_double * k)(*coef)
    _ensure(symb)
    lib = _lib.lib()
    L.touched()
    try:
        rc = lib.csp_chol_update(symb.handle, L.blkval.data_ptr(), V.data_ptr(), V.stride(0) if k > 1 else max(V.stride(0), symb.n),
                                 k, ah, _stream())
    finally:
        note_cache(symb, L)
    if rc > 0:
        raise ArithmeticError("chol_update: the downdate by column %d leaves the cone; L is not usable" % (rc - 1))
    if rc in (_E_SUPPORT, _E_VALUE):
        col = ctypes.c_int64(-1)
        lib.csp_chol_update_info(symb.handle, ctypes.byref(col))
        raise ValueError("chol_update: column %d of V %s; L is unchanged" % (
            col.value, "has a nonzero outside the clique of its first nonzero" if rc == _E_SUPPORT else "is not finite"))
    _chk(rc, "chol_update")


def dot(X, Y):
    _ensure(X.symb)
    out = ctypes.c_double(0.0)
    _chk(_lib.lib().csp_dot(X.symb.handle, X.blkval.data_ptr(), Y.blkval.data_ptr(), ctypes.byref(out), _stream()), "dot")
    return out.value


def logdiagsum(X):
    _ensure(X.symb)
    out = ctypes.c_double(0.0)
    _chk(_lib.lib().csp_logdiagsum(X.symb.handle, X.blkval.data_ptr(), ctypes.byref(out), _stream()), "logdiagsum")
    return out.value


PROBE_WIDTH = 8       # trial factorisations per probe round (copies of the pattern in the replicated context)


def _forest(symb, K):
    """The K-fold replicated Symbolic of `symb` on the same device, with its persistent trial buffer."""
    import torch
    fs = symb.__dict__.setdefault("_forests", {})
    if K not in fs:
        _ensure(symb)
        F = symb.replicate(K)
        F.device_init(symb._device, 1)
        F.__dict__["_trial_T"] = torch.empty((K, symb.blklen), dtype=torch.float64, device="cuda:%d" % symb._device)
        fs[K] = F
    return fs[K]


def probe_factors(base, d, alphas, kind):
    """Trial factorisations of base + alpha * d for every alpha in `alphas` in ONE factorisation of the K-fold
    replicated pattern (include/smcp_amd.h csp_symbolic_replicate): the launches of a single cholesky (kind 'd': the
    dual cone K_V) or completion (kind 'p': the primal cone C_V), K times as wide, one failure flag per trial.  The
    reference factors its trial points one after the other (solvers.py:615-689, 928-939, 2172-2209).
    Returns (ok, factors): ok[k] = trial k is inside the cone; factors[k] = its factor as a cspmatrix VIEW of the
    trial buffer (valid until the next probe on this pattern), or None where the trial failed."""
    import torch
    symb = base.symb
    K = len(alphas)
    # one replicated pattern per base pattern (building it costs about as much as the base context): rounds of fewer
    # than PROBE_WIDTH trials repeat their last trial, longer lists are split
    if K > PROBE_WIDTH:
        ok, fac = [], []
        for k0 in range(0, K, PROBE_WIDTH):
            o, f = probe_factors(base, d, alphas[k0:k0 + PROBE_WIDTH], kind)
            if k0 + PROBE_WIDTH < K:
                f = [None if x is None else x.copy() for x in f]     # the next round overwrites the trial buffer
            ok += o
            fac += f
        return ok, fac
    alphas = list(alphas) + [alphas[-1]] * (PROBE_WIDTH - K)
    F = _forest(symb, PROBE_WIDTH)
    T = F.__dict__["_trial_T"]
    al = torch.as_tensor(alphas, dtype=torch.float64, device=T.device)
    torch.mul(al.unsqueeze(1), d.blkval.unsqueeze(0), out=T)
    T.add_(base.blkval.unsqueeze(0))
    L = _lib.lib()
    rc = (L.csp_completion if kind == "p" else L.csp_cholesky)(F.handle, T.data_ptr(), _stream())
    if rc < 0:
        _chk(rc, "probe")
    flags = (ctypes.c_int * PROBE_WIDTH)()
    if rc > 0:
        _chk(L.csp_trial_flags(F.handle, PROBE_WIDTH, flags), "csp_trial_flags")
    ok = [flags[k] == 0 for k in range(K)]
    return ok, [cspmatrix(symb, T[k]) if ok[k] else None for k in range(K)]


def probe_cone(base, d, alphas, kind):
    """ok[k]: is base + alphas[k] * d inside the cone?  (probe_factors without the factors.)"""
    return probe_factors(base, d, alphas, kind)[0]
