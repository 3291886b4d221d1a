/*
 * smcp_amd.h -- C ABI of the MI355X-native chordal-matrix Newton-KKT kernels.
 *
 * The reference (cvxopt/smcp) has no plugin registry: its hot path is the set of Python
 * callables it imports from CHOMPACK / CVXOPT / its own misc extension inside
 * chordalsolver_feas/_esd (src/python/solvers.py:77-99).  Every entry point below names the
 * call it replaces.  Conventions (observed at the reference's call sites):
 *   - operations are IN PLACE on a flat fp64 vector `blkval` (clique k owns a dense
 *     column-major (nn+na) x nn block at blkptr[k]); the caller owns all numeric buffers;
 *   - the strict upper triangle of every X_NN block (the blkval slots that belong to no entry of V) is zero on entry
 *     and left zero on exit of every operation; the leading dimensions ldu, ldb and ldh may exceed the packed size
 *     (blklen, n, m), and the padding between the columns is never written;
 *   - all numeric pointers are DEVICE pointers (HBM) unless a parameter says "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - return value: 0 ok; k>0 = clique k-1 (or pivot) was not positive definite, which the
 *     Python shim turns into ArithmeticError exactly like CHOMPACK does
 *     (caught at solvers.py:628,643,658,...); <0 = usage / HIP error.
 * No CPU fallback exists: compute entry points fail with SMCP_ENODEV when no GPU is present.
 */
#ifndef SMCP_AMD_H
#define SMCP_AMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct csp_ctx csp_ctx;

#define SMCP_EINVAL (-1)
#define SMCP_ENODEV (-2)
#define SMCP_EHIP (-3)
#define SMCP_ENOMEM (-4)
#define SMCP_ESTALE (-5)  /* the prepared sharded factor was overwritten by another call (kkt_prepare_part again), or -- with
                             CSP_TUNE_VERIFY_CACHE -- a cached quantity is older than the matrix it was derived from */
#define SMCP_ETIMEOUT (-6) /* a workgroup of the one-launch blocked Cholesky (csrc/front_flow.hip) waited longer than 3 s for a tile
                             of another workgroup: the launch gave up instead of hanging (never seen; the results are invalid) */
#define SMCP_ENOCONV (-7) /* the Jacobi iteration of csp_clique_eigvalsh / csp_clique_eigh / csp_clique_project did not converge
                             on some clique within 30 sweeps, or the clique block holds a non-finite entry */
#define SMCP_ESUPPORT (-8) /* csp_chol_update: a column of V has a nonzero outside the clique its first nonzero selects */
#define SMCP_EVALUE (-9)   /* csp_chol_update: a column of V, or its coefficient, holds a NaN or an infinity */

/* ---- symbolic layer (host only, no GPU needed) ------------------------------------- */

/* chompack.symbolic(A, p) (solvers.py:305,308,314; analysis.py:49-51).
 * colptr/rowind: CCS lower-triangular pattern of the n x n aggregate sparsity pattern (host,
 * 64-bit indices as cvxopt int_t, src/C/cvxopt.h:46); perm: perm[new] = orig or NULL.
 * On failure returns NULL and writes a negative code to *info. */
csp_ctx* csp_symbolic_create(int64_t n, const int64_t* colptr, const int64_t* rowind,
                             const int64_t* perm, int64_t* info);
void csp_symbolic_destroy(csp_ctx* ctx);
/* K (<= 16) independent copies of the pattern of `base` as one symbolic object: copy t owns cliques t*nsn .., columns
 * t*n .. and the blkval range [t*blklen, (t+1)*blklen).  csp_cholesky / csp_completion on it factor K trial matrices
 * (stored one after the other) with the kernel launches of ONE factorisation, each copy with its own failure flag:
 * the trial factorisations of the reference's step-length searches (solvers.py:615-689, 928-939, 2172-2209), which
 * the reference runs one after the other.  The factorisation returns the first failing copy's code;
 * csp_trial_flags then gives every copy's flag (0 = inside the cone, else 1 + failing clique within the copy). */
csp_ctx* csp_symbolic_replicate(const csp_ctx* base, int64_t K, int64_t* info);
int csp_trial_flags(csp_ctx* ctx, int64_t K, int* out);

/* Deferred status.  The factorisations (csp_cholesky, csp_completion, the chol(Y_AA) inside the Hessians and the Schur
 * sweeps, dense_potrf) report "not positive definite" by reading a device flag back, which synchronises the stream:
 * the reference's calls raise at once (CHOMPACK cholesky -> ArithmeticError, solvers.py:881-891).  With
 * csp_lazy_status(ctx, 1) they return 0 without waiting and the first failure is latched on the device;
 * csp_status(ctx, stream) synchronises, returns the latched code (0 = none; otherwise what the failing call would
 * have returned) and clears it.  After a failure the calls that follow run on meaningless data until the status is
 * read -- safe (no index depends on values), but their results are void.  One KKT solve then costs one host
 * synchronisation instead of four. */
int csp_lazy_status(csp_ctx* ctx, int on);
int csp_status(csp_ctx* ctx, void* stream);

/* symb.p / snode / snptr / relptr / blkptr ... (cspmatrix internals [EXT], SURVEY App. A.1;
 * supernodes()/separators()/cliques() at analysis.py:173-175).  Returns the number of
 * elements of array `what`; when out != NULL copies them as int64 (host). */
enum {
  CSP_Q_SCALARS = 0, /* [n, nnz, nsn, fill, blklen, updlen, nlev, max_nn, max_na, max_front] */
  CSP_Q_PERM = 1, CSP_Q_IPERM = 2, CSP_Q_SNPTR = 3, CSP_Q_SNPAR = 4, CSP_Q_ROWPTR = 5,
  CSP_Q_ROWIDX = 6, CSP_Q_SEPPTR = 7, CSP_Q_RELIDX = 8, CSP_Q_BLKPTR = 9, CSP_Q_UPDPTR = 10,
  CSP_Q_CHPTR = 11, CSP_Q_CHIDX = 12, CSP_Q_LEVPTR = 13, CSP_Q_LEVIDX = 14, CSP_Q_CCSPTR = 15,
  CSP_Q_SNODE = 16,
  CSP_Q_FAMILY = 17, /* nsn, after csp_device_init: 2 = small front swept together with its childless children in one
                        workgroup (family kernel of the sparse-input Schur sweeps), 1 = such a child, 0 = neither */
  CSP_Q_MRC_CLAMPED = 18, /* 1 value: cliques of the last csp_mrcompletion on this context whose Schur-complement factor had
                             more pivots above the threshold than the r columns left room for (0 when r came from
                             csp_mrcompletion_rank with the same X and tol, up to rounding) */
  CSP_Q_EDM_CLAMPED = 19, /* 1 value: the same for the last csp_edmcompletion (r from csp_edmcompletion_rank) */
  CSP_Q_CEIG_SWEEPS = 20, /* 1 value: the most Jacobi sweeps any clique took in the last csp_clique_eigvalsh, csp_clique_eigh or
                             csp_clique_project on this context; for a clique on the wide route (CSP_TUNE_CEIG_WIDE) its BLOCK
                             sweeps are what is counted */
  CSP_Q_CEIG_WIDE = 21,   /* 1 value: the cliques that took the wide route in the last csp_clique_eigvalsh, csp_clique_eigh,
                             csp_clique_project or csp_cone_project_steps on this context */
  CSP_Q_SLOT_SHARE = 22,  /* 1 value: the most cliques any one workgroup served from its slot in device memory in the last
                             completion (rank or factor pass), csp_clique_eigvalsh, csp_clique_eigh, csp_clique_project or
                             csp_cone_project_steps on this context: ceil(cliques / workgroups) of a launch over slots in
                             device memory, the largest over the launches of the call; 0: the call made no such launch.  A
                             host integer: nothing is read back */
  CSP_Q_CEIG_GROUPS = 23  /* 1 value: the launch groups the wide cliques (CSP_TUNE_CEIG_WIDE) were split into in the last
                             csp_clique_eigvalsh, csp_clique_eigh, csp_clique_project or csp_cone_project_steps on this context
                             (CSP_TUNE_SLOT_DOUBLES; 0: no wide clique).  A host integer */
};
int64_t csp_symbolic_query(const csp_ctx* ctx, int what, int64_t* out);

/* chompack.maxcardsearch (solvers.py:301); order[new] = orig (host). */
int csp_maxcardsearch(int64_t n, const int64_t* colptr, const int64_t* rowind, int64_t* order);
/* fill-reducing ordering for non-chordal input, in place of cvxopt.amd.order (solvers.py:278-279). */
int csp_mindegree(int64_t n, const int64_t* colptr, const int64_t* rowind, int64_t* order);
/* position in blkval of original-coordinate entries (I[e],J[e]); -1 outside V (host arrays).
 * Replaces the LI/lp/Ip/Jp index algebra of solvers.py:310-319. */
int csp_index_map(const csp_ctx* ctx, int64_t cnt, const int64_t* I, const int64_t* J, int64_t* out);

/* ---- device context ---------------------------------------------------------------- */

/* Upload the index arrays to `device` and allocate the internal update-matrix workspace for
 * up to max_rhs simultaneous right-hand sides (>= 1).  Idempotent for the same arguments; a larger max_rhs
 * grows the workspace.  One process drives ONE device: a different device for an initialised context, or for
 * another context of the same process, returns SMCP_EINVAL (one rank per GPU is the multi-GPU model). */
int csp_device_init(csp_ctx* ctx, int device, int64_t max_rhs);
/* Bytes of device memory this context holds now (index arrays, tables, workspaces, scratch). */
int64_t csp_device_bytes(const csp_ctx* ctx);

/* ---- chordal kernels (all in place, device pointers) ------------------------------- */

/* chompack.cholesky(X): X -> L, L L^T = X with zero fill (solvers.py:640,884,...). */
int csp_cholesky(csp_ctx* ctx, double* blkval, void* stream);
/* chompack.llt(L): L -> L L^T on V (solvers.py:904,1721). */
int csp_llt(csp_ctx* ctx, double* blkval, void* stream);
/* chompack.projected_inverse(L): L -> P_V((L L^T)^-1) (solvers.py:891,2361). */
int csp_projected_inverse(csp_ctx* ctx, double* blkval, void* stream);
/* The dual scaling point in one call (solvers.py:881-891: `L = S.copy(); cholesky(L); Y = projected_inverse(L)`, and
 * 2341-2361 in the embedding driver): on entry L holds S, on return L = chol(S) and Y = P_V(S^-1) -- the results of
 * csp_cholesky(L), a copy into Y and csp_projected_inverse(Y), status as csp_cholesky.  As ONE entry point the clique-local
 * stages that need finished levels only (the inverse-form factor of the lower levels, the copy into Y, and with
 * with_factors != 0 the Cholesky factors of the separator blocks Y_AA that the Hessian / Schur sweeps use next -- CHOMPACK's
 * factored updates) run on side streams beside the few-workgroup chains of the top fronts instead of after them.  L and Y
 * must be distinct blkval buffers. */
int csp_cholesky_projected_inverse(csp_ctx* ctx, double* L, double* Y, int with_factors, void* stream);
/* chompack.completion(X): X -> L with P_V((L L^T)^-1) = X (solvers.py:625,874,...). */
int csp_completion(csp_ctx* ctx, double* blkval, void* stream);
/* chompack.hessian(L, Y, U, adj, inv) (solvers.py:405,415,483,524,531,...): U holds nrhs
 * matrices, matrix r at U + r*ldu (the reference passes a Python list).  adj: 0 = False,
 * 1 = True, 2 = None (both factors).  inv: 0/1. */
int csp_hessian(csp_ctx* ctx, const double* L, const double* Y, double* U, int64_t nrhs,
                int64_t ldu, int adj, int inv, void* stream);
/* chompack.trsm(L, B, trans) (solvers.py:491-492): B is a dense n x nrhs column-major matrix
 * with rows in the permuted (symbolic) order; trans 0: L^-1 B, 1: L^-T B. */
int csp_trsm(csp_ctx* ctx, const double* L, double* B, int64_t nrhs, int64_t ldb, int trans,
             void* stream);
/* chompack.trmm(L, B, alpha, trans): B <- alpha L B (trans 0) or alpha L^T B (trans != 0), L read as a lower-triangular
 * factor (what csp_cholesky / csp_completion leave: of the diagonal block of a supernode only the lower triangle counts).
 * B has the layout of csp_trsm: a dense n x nrhs column-major matrix with leading dimension ldb >= n, rows in the
 * permuted (symbolic) order; entries between n and ldb of a column are not touched.  L is not changed and nothing cached
 * for it is dropped.  alpha is applied once, at the last write.  Two or three kernel launches whatever the depth of the
 * clique tree (the products of all cliques at once, then one combining pass).  Deterministic on every route: the
 * contributions to an entry are summed in a fixed order, there are no floating-point atomics, and the same arguments
 * give the same bits from call to call.  Does not synchronise: the work is queued on `stream`, the return value reports
 * launch failures only.  Needs sepptr[nsn] * nrhs doubles of update workspace for trans 0 (SMCP_ENOMEM otherwise: call
 * csp_device_init with a larger max_rhs, as chordal.trmm does).  SMCP_EINVAL for nrhs < 1 or above 2^18, ldb < n, or a
 * context under a subtree partition over more than one rank (csp_set_partition). */
int csp_trmm(csp_ctx* ctx, const double* L, double* B, int64_t nrhs, int64_t ldb, double alpha, int trans,
             void* stream);
/* chompack.syr2(X, y, z, alpha, beta) for a block of k columns: X <- beta X + alpha P_V(U V^T + V U^T), or, with V == NULL,
 * X <- beta X + alpha P_V(U U^T) (ldv is then ignored).  U and V have the layout of csp_trsm: dense n x k column-major
 * matrices with leading dimensions ldu, ldv >= n, rows in the permuted (symbolic) order; they are never written, and V may
 * alias U (the result is then 2 alpha P_V(U U^T), computed as the rank-2k update).  For clique c with columns N, front rows
 * F = [N; A] and its nf x nn panel, panel[m, j] = beta panel[m, j] + alpha sum_r (U[F_m, r] V[N_j, r] + V[F_m, r] U[N_j, r])
 * on the rows m >= j of the N N part and all rows of the A N part, r ascending.  The call writes EVERY slot of X (blklen
 * doubles): the slots outside the pattern, the strict upper triangles of the N N blocks, are never read and are stored as
 * exactly 0.0.  beta == 0: X is not read (NaN / Inf in it do not propagate); alpha == 0: U and V are not read.  X is read
 * once and written once, every entry has one owner and a fixed order of summation: no atomics, and the same arguments
 * give the same bits from call to call.  One or two kernel launches whatever the clique tree.  Whatever the library had
 * derived from the old contents at X's address is dropped.  Does not synchronise: the work is queued on `stream`, the
 * return value reports launch failures only.  SMCP_EINVAL for k < 1 or above 2^18, ldu < n, ldv < n (V given), or a
 * context under a subtree partition over more than one rank (csp_set_partition). */
int csp_syr2k(csp_ctx* ctx, double* X, const double* U, const double* V, int64_t k, int64_t ldu, int64_t ldv, double alpha,
              double beta, void* stream);
/* C <- alpha X B + beta C for the symmetric matrix X stored on the pattern and dense n x nrhs blocks B and C in the layout
 * of csp_trsm (column-major, leading dimensions ldb, ldc >= n, rows in the permuted (symbolic) order).  X is read as a
 * symmetric matrix: of the N N block of a supernode only the lower triangle counts, what is stored above it is never
 * used.  X is never written and nothing cached for it is dropped.  B and the entries between n and the leading dimension
 * of a column of B and of C are never written.  C must not overlap B: overlapping address ranges are SMCP_EINVAL.  A term
 * whose factor is zero is left out, not multiplied by zero: beta == 0 does not read C (NaN / Inf there do not propagate),
 * alpha == 0 reads neither X nor B and returns beta C (bit for bit for beta == 1), alpha == beta == 0 stores exact zeros.
 * alpha and beta are applied once, in the last pass.  Two or three kernel launches whatever the clique tree: the partial
 * products of all cliques at once (every stored entry of X is read once per block of columns and used for both of its
 * outputs, row i and row j), stored through a contribution index built once per context, then one combining pass.  The
 * order of every sum is fixed by that index: no floating-point atomics, and the same arguments give the same bits from
 * call to call.  Does not synchronise: the work is queued on `stream`, the return value reports launch failures only.
 * Needs csp_symm_positions(ctx) * nrhs doubles of update workspace (SMCP_ENOMEM otherwise: call csp_device_init with a
 * larger max_rhs, as chordal.symm does).  SMCP_EINVAL for nrhs < 1 or above 2^18, ldb < n, ldc < n, or a context under a
 * subtree partition over more than one rank (csp_set_partition); SMCP_ENODEV without a device. */
int csp_symm(csp_ctx* ctx, const double* X, const double* B, int64_t ldb, double* C, int64_t ldc, int64_t nrhs, double alpha,
             double beta, void* stream);
/* The number of partial products of one column of csp_symm (the length of its contribution index): one per row of every
 * listed (clique, 64 panel rows, 256 panel columns) item and one per column of it with a row strictly below.  Host only:
 * needs no device. */
int64_t csp_symm_positions(csp_ctx* ctx);
/* Chordal plus low rank: M = L L^T + V diag(a) V^T with V dense n x k (layout of csp_trsm), 1 <= k <= 64, held as the factor
 * L, W = L^-1 V and a state block of csp_lowrank_state_len(k) doubles on the device: [0] status, [1] sum of log t_j, [2] k,
 * then a (k), K = W^T W, C, D and S (k x k each, row-major) with
 *   M = F F^T, F = L (I + W C W^T);  F^-1 = (I + W D W^T) L^-1;  M^-1 = L^-T (I + W S W^T) L^-1;  M = L (I + W A W^T) L^T.
 * C and D are built one column of V at a time from K and a alone (the columns with a_j > 0 first, then those with a_j < 0,
 * a_j = 0 skipped), with no division by anything that dependent columns of V make small.  W and the state block belong to the
 * caller.  All three calls return SMCP_EINVAL for k outside 1 .. 64, a leading dimension below n or a context under a subtree
 * partition over more than one rank, SMCP_ENODEV without a device.  -1 from csp_lowrank_state_len for k outside 1 .. 64. */
int64_t csp_lowrank_state_len(int64_t k);
/* W (ldw >= n) holds V on entry and L^-1 V on return (one csp_trsm); a_host: k coefficients on the HOST, NULL for all ones.
 * At most three launches beside those of csp_trsm: the slab-wise partial products of K = W^T W and one workgroup for the
 * k x k construction.  Synchronises the stream and returns 0, or 1 + j when column j (in the caller's order) shows that M is
 * not positive definite (t_j = 1 + a_j c^T K c <= 0); the state block is then not usable. */
int csp_lowrank_factor(csp_ctx* ctx, const double* L, double* W, int64_t ldw, int64_t k, const double* a_host, double* state,
                       void* stream);
/* B <- op B in place for a dense n x nrhs block B in the layout of csp_trsm (ldb >= n; entries between n and ldb of a column
 * are not touched).  L, W and the state block are only read.  Exactly two launches (the partial products of W^T B by row
 * slabs, then B += W (T W^T B) with the partials summed in ascending slab) beside the csp_trsm / csp_trmm launches the
 * operation wraps, per block of 512 columns; no floating-point atomics, the same arguments give the same bits from call to
 * call.  Does not synchronise.  Needs the update workspace of csp_trmm / csp_trsm (SMCP_ENOMEM otherwise). */
enum { CSP_LR_F = 0, CSP_LR_FT = 1, CSP_LR_FINV = 2, CSP_LR_FINVT = 3, CSP_LR_MINV = 4, CSP_LR_M = 5 };
int csp_lowrank_apply(csp_ctx* ctx, const double* L, const double* W, int64_t ldw, int64_t k, const double* state, double* B,
                      int64_t ldb, int64_t nrhs, int op, void* stream);
/* *out (host) = log det M = 2 csp_logdiagsum(L) + sum of log t_j.  Synchronises the stream. */
int csp_lowrank_logdet(csp_ctx* ctx, const double* L, const double* state, double* out, void* stream);
/* Rank-k update and downdate of the factor itself: L (as csp_cholesky leaves it) is overwritten so that L L^T becomes
 * L L^T + V diag(a) V^T.  V: dense n x k in the layout of csp_trsm (column j at V + j ldv, ldv >= n, rows in the permuted
 * order), 1 <= k <= 64, only read, entries between n and ldv of a column neither read nor touched; a_host: k coefficients on
 * the HOST, NULL for all ones; a_j < 0 is a downdate, a_j = 0 leaves its column out.  Every column v must have its support
 * inside one clique: with j0 its first nonzero and s the supernode of column j0, all its nonzeros lie in the rows [N_s; A_s]
 * (csp_clique_support finds s on the host) -- the condition under which the storage of L holds the new factor without fill.
 * The columns with a_j > 0 are taken first, then those with a_j < 0, each group in the caller's order (the order of
 * csp_lowrank_factor); the arithmetic is that of successive rank-one updates of the whole factor, whatever k.
 * Two launches whatever the tree and whatever k; cliques outside the leaf-to-root paths of the columns are not written, nor
 * is a panel column whose rotations are all the identity.  No floating-point atomics: the same arguments give the same bits.
 * Synchronises the stream and returns
 *   0              L holds the new factor;
 *   1 + j          the downdate by column j (caller's numbering) met (l - w)(l + w) <= 0: the matrix is no longer positive
 *                  definite and L IS NOT USABLE (as after a failed csp_cholesky: keep a copy where that matters);
 *   SMCP_ESUPPORT  a column violates the support condition, SMCP_EVALUE a column or its coefficient is not finite: L is bit for
 *                  bit what it was (the columns are checked on the device before anything is written); the first such column
 *                  is what csp_chol_update_info reports;
 *   SMCP_EINVAL    a null L or V, k outside 1 .. 64, ldv < n, a replicated context or one under a subtree partition over
 *                  more than one rank; SMCP_ENODEV without a device.
 * Whatever the library had derived from the old contents at L's address is dropped, as by csp_touch. */
int csp_chol_update(csp_ctx* ctx, double* L, const double* V, int64_t ldv, int64_t k, const double* a_host, void* stream);
/* *column = the column of V (caller's numbering) that the last csp_chol_update on this context refused or failed at, -1 when
 * it returned 0 or an argument error.  Host only. */
int csp_chol_update_info(const csp_ctx* ctx, int64_t* column);
/* The clique whose rows contain all of idx[0 .. cnt) (permuted order) and whose supernode holds the smallest of them: the s
 * of csp_chol_update for a column with that support; -1 when there is none (also for cnt = 0, an index outside 0 .. n - 1, a
 * null idx or a replicated context).  Host only: needs no device. */
int64_t csp_clique_support(const csp_ctx* ctx, int64_t cnt, const int64_t* idx);
/* chompack.mrcompletion(X), pass 1: *r = max over the cliques g of the numerical rank of X_gg -- the pivots of a
 * diagonally pivoted Cholesky (LAPACK pstrf semantics) above tol * max diag(X_gg).  Returns 1 + k when clique k has a
 * remaining pivot below -tol * max diag(X_gg): X has no positive semidefinite completion.  Synchronises the stream. */
int csp_mrcompletion_rank(csp_ctx* ctx, const double* blkval, double tol, int64_t* r, void* stream);
/* chompack.mrcompletion(X), pass 2: Y (n x r, row i at Y + i*ldY, rows in the permuted order) with P_V(Y Y^T) = X, for
 * the r of csp_mrcompletion_rank (same X and tol).  Top-down over the clique tree: per clique a column-pivoted QR of
 * Y_A^T, a triangular solve and the pivoted Cholesky factor of the Schur complement.  Deterministic; synchronises. */
int csp_mrcompletion(csp_ctx* ctx, const double* blkval, double tol, int64_t r, double* Y, int64_t ldY, void* stream);
/* Goemans-Williamson rounding of a Y of csp_mrcompletion (device arrays): for trial t, s[t*n + i] = sign(Y_i . g_t) with
 * 0 -> +1 (g_t = G + t*r), and cut[t] = sum of w[e] over the edges (ei[e], ej[e]) (permuted indices) whose ends get
 * different signs, summed in a fixed order. */
int csp_maxcut_cuts(csp_ctx* ctx, const double* Y, int64_t ldY, int64_t r, int64_t trials, const double* G, int64_t nedges,
                    const int64_t* ei, const int64_t* ej, const double* w, int8_t* s, double* cut, void* stream);
/* chompack.edmcompletion(D), pass 1: D holds squared distances on V (zero diagonal).  *r = max over the cliques g of the
 * numerical affine dimension of D_gg -- the pivots above tol * max diag(G) of a diagonally pivoted Cholesky of the
 * centred Gram matrix G = -1/2 (D_gg - rho 1^T - 1 rho^T + sigma 1 1^T), centred on the separator points of g (on g itself
 * at a root).  Returns 1 + k when clique k has a remaining pivot below -tol * max diag(G): D_gg is not a Euclidean
 * distance matrix, so D has no Euclidean completion; SMCP_EINVAL for a nonzero diagonal entry.  Synchronises the stream. */
int csp_edmcompletion_rank(csp_ctx* ctx, const double* blkval, double tol, int64_t* r, void* stream);
/* chompack.edmcompletion(D), pass 2: points Y (n x r, row i at Y + i*ldY, rows in the permuted order) with
 * |Y_i - Y_j|^2 = D_ij on V, for the r of csp_edmcompletion_rank (same D and tol); Y is determined up to a rigid motion.
 * Top-down over the clique tree, per clique the step of csp_mrcompletion on G, centred on the centroid of the separator
 * rows.  Columns dropped at the r cap: csp_symbolic_query(CSP_Q_EDM_CLAMPED).  Deterministic; synchronises. */
int csp_edmcompletion(csp_ctx* ctx, const double* blkval, double tol, int64_t r, double* Y, int64_t ldY, void* stream);
/* chompack.edmcompletion's return form, the dense completed EDM (device arrays): D[i*ldD + j] = |Y_p(i) - Y_p(j)|^2 for
 * i, j < n, p = perm (n int64 row indices of Y; NULL: the identity), summed over the r columns in a fixed order: exactly
 * symmetric with a zero diagonal.  perm = the inverse permutation of the symbolic order gives the original order. */
int csp_edm_dense(csp_ctx* ctx, const double* Y, int64_t ldY, int64_t r, const int64_t* perm, double* D, int64_t ldD,
                  void* stream);
/* chompack.psdcompletion(X): the dense maximum-determinant positive semidefinite completion Xd (n x n device array, entry
 * (i, j) at Xd + i*ldX + j, the permuted order; exactly symmetric, equal to X on V bit for bit).  For X positive definite on
 * V its inverse vanishes off V.  Top-down over the levels of the clique tree: Xd[E, N] = Xd[E, A] W for the columns N and
 * separator A of a clique and the rows E completed before, W the basic solution of X_AA W = X_AN from a diagonally pivoted
 * Cholesky of X_AA (pivots above tol * max diag(X_AA)): no inverse but those of the separator blocks, no Schur complement,
 * so X may be singular.  Entries between different components of the pattern are zero.  Returns 1 + k when clique k is
 * not positive semidefinite (the test of csp_mrcompletion_rank), SMCP_EINVAL for ldX < n.  X is not changed.
 * Deterministic; synchronises the stream. */
int csp_psdcompletion(csp_ctx* ctx, const double* blkval, double tol, double* Xd, int64_t ldX, void* stream);
/* Spectra of the clique blocks: w[rowptr[k] .. rowptr[k + 1]) (device, rowptr[nsn] doubles) = the eigenvalues, ascending, of
 * A_gg for clique k = g, or with b given of the pencil (A_gg, B_gg) -- of B_gg^-1 A_gg.  a and b are blkvals read as symmetric
 * matrices (of a supernode's diagonal block the lower triangle counts) and are not written.  X is in the interior of the
 * cone of PSD-completable matrices exactly when every X_gg is positive definite, so min w decides membership and
 * -1 / min w of the pencil (D, X) is the step to the boundary along D.  ext (device, 4 doubles, may be NULL) receives the
 * smallest eigenvalue over all cliques, the lowest clique attaining it, the largest, and the lowest clique attaining that.
 * One workgroup per clique: a Cholesky of B_gg and two triangular solves (pencil form), a two-sided cyclic Jacobi in a
 * fixed parallel order without eigenvectors, a rank sort; at most six launches plus one whatever the tree, beside the
 * top-down gathers of the separator blocks (under CSP_TUNE_CEIG_WIDE the wide cliques leave these launches, in both forms,
 * for a block Jacobi over the whole chip: two launches per step of a block sweep, one integer read back per block sweep; in
 * pencil form the Cholesky of B_gg and the two solves run in front of it by 64-row tiles over the chip, 3 ceil(nf / 64) + 1
 * launches for the widest clique whatever the data, and a B_gg that is not positive definite is reported as without the tune).
 * The same input gives the same bits.  Returns 0, 1 + k when B_gg of clique k
 * is not positive definite, SMCP_ENOCONV when a clique did not converge in 30 sweeps (a non-finite entry ends this way),
 * SMCP_EINVAL for a null a or w, a replicated context, or w / ext overlapping a, b or each other.  The most sweeps of a
 * clique: csp_symbolic_query(CSP_Q_CEIG_SWEEPS).  Synchronises the stream (the status is read back; w and ext are not). */
int csp_clique_eigvalsh(csp_ctx* ctx, const double* a, const double* b, double* w, double* ext, void* stream);
/* Packed clique blocks: qptr[nsn] doubles in which clique k holds an nf_k x nf_k column-major block at
 * [qptr[k], qptr[k + 1]), nf_k = nn_k + na_k, rows and columns in the order of the clique's rowidx (the supernode's own
 * columns, then its separator rows).  Writes the nsn + 1 offsets to qptr_host (host).  Host only: no device is needed.
 * SMCP_EINVAL for a null argument. */
int csp_clique_ptr(csp_ctx* ctx, int64_t* qptr_host);
/* Z (device, packed clique blocks) = the full symmetric block X_gg of every clique g of the blkval x, which is read as
 * csp_clique_eigvalsh reads it and not written: the top-down gathers of the separator blocks, then one launch over all
 * cliques.  SMCP_EINVAL for a null x or Z, a replicated context, or Z overlapping x.  Does not synchronise. */
int csp_clique_gather(csp_ctx* ctx, const double* x, double* Z, void* stream);
/* x (blkval) = P_V(sum_k E_k Z_k E_k^T) for packed clique blocks Z (device, not written), E_k the columns of the identity
 * of clique k: every entry of V is the sum of that entry over the cliques that hold it.  Only the lower triangle of each Z_k
 * is read.  Every slot of x is written; the slots above the diagonal of a supernode's diagonal block get zeros (the contract
 * of csp_syr2k).  One launch per level, leaves first: a clique's own block, then its children's contributions in the order
 * of its child list, no atomics: the same input gives the same bits.  SMCP_EINVAL for a null x or Z, a replicated or
 * partitioned context, or x overlapping Z.  Does not synchronise. */
int csp_clique_scatter(csp_ctx* ctx, const double* Z, double* x, void* stream);
/* Z_k = P_k P_k^T for every clique: the Agler decomposition of L L^T (no reference counterpart; CHOMPACK has none).
 * L (device, blkval) is a factor as csp_cholesky leaves it and is only read; Z (device, packed clique blocks) is written.
 * Clique k has nn own columns and nf = nn + na rows, its panel P is nf x nn, column-major with leading dimension nf, at
 * blkptr[k] of L.  With Pt[m, c] = P[m, c] for m >= c and 0 otherwise (the slots m < c < nn of L are never read)
 *     Z_k[i, j] = sum_{c = 0}^{min(i, j, nn - 1)} Pt[i, c] Pt[j, c],    0 <= i, j < nf,    c ascending,
 * stored at Z + qptr[k] + i + j nf: the full symmetric block, both triangles carrying the same bits, every entry of Z with
 * exactly one writer.  Every Z_k is positive semidefinite of rank <= nn and sum_k E_k Z_k E_k^T = L L^T: csp_clique_scatter
 * of Z is csp_llt of L to rounding.  One launch, two when the large fronts take the tile products (everything runs on the
 * plain FMA kernel under CSP_TUNE_DETERMINISTIC), whatever the tree; no atomics: the same L gives the same bits.  Nothing
 * cached for L is dropped or created.  A positive semidefinite matrix that is singular has no factor here and is out of
 * reach of this call.  SMCP_EINVAL for a null L or Z, a replicated or partitioned context, or Z overlapping L.  Does not
 * synchronise. */
int csp_clique_decompose(csp_ctx* ctx, const double* L, double* Z, void* stream);
/* Eigenvectors of the clique blocks: w and ext as csp_clique_eigvalsh gives them in standard form (the same bits); Q
 * (device, packed clique blocks): column j of block k is a unit eigenvector of A_gg for w[rowptr[k] + j].  The Jacobi
 * iteration of csp_clique_eigvalsh with the rotations accumulated, in the slot of its pencil form; signs and the basis
 * inside a degenerate eigenspace are unspecified but repeatable: the same input gives the same bits.  A clique wider
 * than 89 rows runs from a slot in device memory on one workgroup and is slow unless CSP_TUNE_CEIG_WIDE sends it through the
 * chip-wide block Jacobi.  Returns 0, SMCP_ENOCONV when a clique did
 * not converge in 30 sweeps (a non-finite entry ends this way; w and Q of that clique are NaN, the others correct),
 * SMCP_EINVAL for a null a, w or Q, a replicated context, or w / Q / ext overlapping a or each other.  The most sweeps of
 * a clique: csp_symbolic_query(CSP_Q_CEIG_SWEEPS).  Synchronises the stream (the status is read back). */
int csp_clique_eigh(csp_ctx* ctx, const double* a, double* w, double* Q, double* ext, void* stream);
/* Clique-wise spectral projection: Z (device, packed clique blocks), block k = A_gg with its eigenvalues clipped to
 * [lo, hi], formed as A_gg + sum over the eigenvalues w_j outside [lo, hi], ascending, of (clip(w_j) - w_j) q_j q_j^T: a
 * block whose spectrum lies inside [lo, hi] is A_gg bit for bit (what csp_clique_gather gives), every block is exactly
 * symmetric, and the work grows with the number of eigenvalues clipped.  This projects every block on its own; it is NOT
 * the projection of A onto the cone of PSD-completable matrices, and the blocks of Z disagree where cliques overlap.
 * w (device, rowptr[nsn] doubles, may be NULL) receives the eigenvalues of A_gg as csp_clique_eigh gives them; info
 * (device, 2 nsn doubles): per clique the number of eigenvalues changed and sum_j (clip(w_j) - w_j)^2, which is
 * |Z_k - A_gg|_F^2 in exact arithmetic.  lo = -inf and hi = +inf are allowed.  Returns 0, SMCP_ENOCONV as csp_clique_eigh
 * (w, Z and info of that clique are NaN), SMCP_EINVAL unless lo <= hi (a NaN bound included), for a null a, Z or info, a
 * replicated context, or Z / w / info overlapping a or each other.  Synchronises the stream. */
int csp_clique_project(csp_ctx* ctx, const double* a, double lo, double hi, double* Z, double* w, double* info, void* stream);
/* The Frobenius projection of the blkval a (read as csp_clique_eigvalsh reads it, never written) onto the cone K of matrices
 * on the pattern whose clique blocks are all positive semidefinite, in the norm of csp_dot: iterations it0 .. it0 + nsteps - 1
 * of a clique-splitting ADMM with penalty rho and over-relaxation relax on a state the caller owns, in place: x (blkval),
 * U and W (device, packed clique blocks: U_k the scaled dual of clique k, negative semidefinite; W_k = Z_k - U_k with Z_k the
 * clique's positive semidefinite copy).  The caller starts with x = a, U = 0 (or the U of an earlier run with the same rho)
 * and W = the clique blocks of a (csp_clique_gather) minus U.  One iteration, every clique on its own:
 *   T_k = Z_k + relax (x_gg - Z_k) + U_k;  U_k <- the negative part of T_k;  Z_k <- T_k - U_k;  W_k <- T_k - 2 U_k,
 * then x <- (a + rho sum_k E_k W_k E_k^T) / (1 + rho mult) entry by entry, mult = the cliques that hold the entry; the slots
 * above the diagonal of a supernode's diagonal block become 0 whatever a holds there.  Row it of hist (device, 4 doubles per
 * iteration, rows 0 .. it0 + nsteps - 1 must exist): sum_k |x_gg - Z_k|_F^2 with the x before the update, |x_new - x_old|^2
 * in the norm of csp_dot, the negative eigenvalues of all T_k, and 1 + the lowest clique whose Jacobi iteration did not
 * converge in 30 sweeps (0: none; a non-finite entry ends this way, and U_k, W_k and the sums are then NaN).  A block T_k
 * without a negative eigenvalue leaves U_k exactly 0.  At the fixed point x is the projection and x - a = -rho sum_k E_k U_k E_k^T
 * lies in the dual cone, the positive semidefinite matrices on the pattern.  Every sum in a fixed order, no atomics: the same
 * input gives the same bits, and 1 + 2 steps in two calls are the 3 steps of one.  A clique wider than 89 rows runs on one
 * workgroup from device memory, in every iteration, unless CSP_TUNE_CEIG_WIDE sends it through the chip-wide block Jacobi:
 * per iteration and launch group of wide cliques the form, 30 block sweeps with the stop test in front of each and one behind
 * the last, the rank sort and the split -- a number of launches that depends on the pattern and the tune alone; the launches
 * behind the test that ended a clique return at once.  hist[4 it + 3] names a wide clique that 30 block sweeps did not
 * finish as it names the others.  Does not synchronise and reads nothing back (the first call on a context, and the first
 * after the tune changed, builds the workspace and may wait).  SMCP_EINVAL for a null pointer, any overlap among a, x, U, W
 * and hist, rho <= 0, relax outside (0, 2), it0 < 0, nsteps < 1, a replicated or partitioned context; SMCP_EHIP when the
 * device does not grant the wide route its 128 KiB of LDS.
 * csp_cone_project_sweeps: *out (host) = the most sweeps of a clique in any iteration since the call with it0 = 0 (Jacobi
 * sweeps, or block sweeps of a clique on the wide route); waits for the stream.  SMCP_EINVAL before the first
 * csp_cone_project_steps on the context. */
int csp_cone_project_steps(csp_ctx* ctx, const double* a, double* x, double* U, double* W, double rho, double relax, int64_t it0,
                           int64_t nsteps, double* hist, void* stream);
int csp_cone_project_sweeps(csp_ctx* ctx, int64_t* out, void* stream);
/* Lanczos on the dual cone: the extreme Ritz values of L^-1 D L^-T (D a blkval read as csp_symm reads it; -1 / theta_min is
 * the step at which L L^T + alpha D stops being positive definite) or, with D NULL, of L^-T L^-1 (1 / theta_max is the
 * smallest eigenvalue of L L^T), with full reorthogonalisation (classical Gram-Schmidt twice) and no host round trip per step.
 * The workspace belongs to the caller: csp_lanczos_work_len(n, jmax) doubles on the device (host only; -1 for n < 1 or jmax
 * outside 1 .. 128), laid out as
 *   the state block, 16 + 2 jmax + 1 doubles rounded up to a multiple of 8: [0] status (0 running, 1 the iteration broke
 *     down: the Krylov space is invariant and the Ritz values are eigenvalues, 2 a non-finite alpha or beta), [1] steps done m,
 *     [2] the step count at which it broke down (-1: never), [3] the pending scale, [4 .. 7] theta_min, resid_min, theta_max,
 *     resid_max, [8] max(|alpha|, beta) seen so far, [16 + j] alpha_j, [16 + jmax + j] beta_j (beta_0 = |v0|);
 *   the partial sums of the two Gram-Schmidt passes (2 x 128 x jmax, each rounded up to a multiple of 8) and of |w|^2
 *     (ceil(n / 256), rounded up likewise);
 *   the basis: rows v_0 .. v_jmax of ld = n rounded up to a multiple of 8 doubles (entries n .. ld of a row are not touched);
 *   two scratch rows of ld doubles.
 * csp_lanczos_steps runs steps j0 .. j0 + nsteps - 1 (j0 + nsteps <= jmax).  Before j0 = 0 the caller puts v0 into basis row 0;
 * the call normalises it and resets the state block.  Step j applies the operator to v_j (csp_trsm, csp_symm, csp_trsm on one
 * column, or csp_trsm twice: those calls' own launches), orthogonalises the result against v_0 .. v_j, stores alpha_j and
 * beta_{j+1} and writes v_{j+1}; beta_{j+1} <= n eps max(|alpha|, beta seen so far) is a breakdown: status 1, v_{j+1} and
 * everything after it exact zeros, later steps of the call count nothing and stay finite.  Seven launches per step beside the
 * operator's, three more at j0 = 0; every sum in a fixed order, no floating-point atomics: the same input gives the same bits.
 * Does not synchronise and reads nothing back.  L and D are not written.  Needs the update workspace of csp_trsm and csp_symm
 * for one column (SMCP_ENOMEM otherwise).  SMCP_EINVAL for a null L or work, jmax outside 1 .. 128, a step range outside
 * 0 .. jmax, a replicated context or one under a subtree partition over more than one rank; SMCP_ENODEV without a device. */
int64_t csp_lanczos_work_len(int64_t n, int64_t jmax);
int csp_lanczos_steps(csp_ctx* ctx, const double* L, const double* D, double* work, int64_t jmax, int64_t j0, int64_t nsteps,
                      void* stream);
/* From alpha_0 .. alpha_{m-1}, beta_1 .. beta_m of the m steps done so far: the extreme eigenvalues theta_min, theta_max of the
 * tridiagonal T_m to eps |T_m| (multisection by Sturm counts from the Gershgorin interval, eight rounds of 128 shifts per
 * end) and the residual estimates beta_m |bottom component of the normalised eigenvector| (two steps of inverse iteration
 * with a pivoted tridiagonal solve), left in the state block.  m = 1: alpha_0 and beta_1.  One launch of one workgroup; the
 * same input gives the same bits.  Does not synchronise. */
int csp_lanczos_ritz(csp_ctx* ctx, double* work, int64_t jmax, void* stream);
/* chompack.dot(X, Y) = tr(XY) on V (solvers.py:399,836,...); result written to *out (host). */
int csp_dot(csp_ctx* ctx, const double* X, const double* Y, double* out, void* stream);
/* sum(log(X.diag())) (solvers.py:395,925,934); *out host. */
int csp_logdiagsum(csp_ctx* ctx, const double* X, double* out, void* stream);
/* cspmatrix copy / +,- / a*X and blas.scal(a, X.blkval) (solvers.py:407,622,905):
 * y <- a*x + b*y over len doubles. */
int csp_axpby(int64_t len, double a, const double* x, double b, double* y, void* stream);

/* ---- KKT layer --------------------------------------------------------------------- */

/* Constraint data in blkval coordinates (replaces Av/Ip/Jp/Id, solvers.py:323-349):
 * host CSC arrays: constraint j has entries cptr[j]..cptr[j+1]-1 at blkval positions cidx with
 * values cval (lower-triangle values, diagonal positions flagged by the context itself). */
int kkt_set_constraints(csp_ctx* ctx, int64_t m, const int64_t* cptr, const int64_t* cidx,
                        const double* cval);
/* options['tnzcols'] (solvers.py:31,210-216; default 0.1): a constraint whose entries touch at most
 * int(n * tnzcols) distinct rows/columns is handled as misc.SCMcolumn2 does (misc.c:620-663, solvers.py:489-497:
 * S^-1[:, K] by two chompack.trsm calls, then pairwise contractions) instead of a Hessian sweep; misc.nzcolumns /
 * misc.matperm (misc.c:682-773) are folded into kkt_set_constraints.  Call before kkt_set_constraints. */
int kkt_set_tnzcols(csp_ctx* ctx, double tnzcols);
/* Amap (solvers.py:369-380): y[i] = <A_i, X>, i < m;  y device, length m. */
int kkt_amap(csp_ctx* ctx, const double* X, double* y, void* stream);
/* Aadj (solvers.py:382-386): X <- sum_i y[i] A_i (overwrites X). */
int kkt_aadj(csp_ctx* ctx, const double* y, double* X, void* stream);
/* kkt_chol factor step (solvers.py:479-501 + misc.c:620-663): builds the m x m Schur
 * complement H_ij = <A_i, hessian(L,Y)(A_j)> (lower) into H (device, ldh >= m) and factors it
 * in place (lapack.potrf, solvers.py:501).
 * DEFERRED CONTRACT.  Under csp_lazy_status(ctx, 1) (and unless SMCP_POTRF_DEFER=0) the call returns with H holding the
 * RAW Schur complement: its Cholesky factorisation waits for the first call of this library that reads H -- kkt_solve
 * (which runs it on a side stream beside its first Hessian sweep), dense_potrs, csp_status -- and is dropped when
 * dense_potrf / kkt_schur_columns / kkt_schur_factor is called on the same H again.  Until then the caller must keep H
 * alive and unmodified and must not read it by its own means (a copy, an all-reduce, its own potrs would see the raw
 * matrix): call csp_status or dense_potrs first, or factor eagerly (csp_lazy_status(ctx, 0), the default).  ONE matrix
 * per context can wait: kkt_schur_factor on another H, or kkt_set_constraints, first factors the waiting one where it
 * stands.  A caller that frees H while it may still be waiting calls kkt_schur_forget first. */
int kkt_schur_factor(csp_ctx* ctx, const double* L, const double* Y, double* H, int64_t ldh,
                     void* stream);
/* H is about to be freed or reused: drops what the context remembers about it (the deferred factorisation above, the
 * cached inverses of its diagonal blocks).  Nothing is launched. */
int kkt_schur_forget(csp_ctx* ctx, const double* H);
/* Columns j0..j1-1 of the (unfactored) Schur complement only: the unit that is sharded over
 * GPUs (each rank builds its column range, then one RCCL all-gather of H). */
int kkt_schur_columns(csp_ctx* ctx, const double* L, const double* Y, double* H, int64_t ldh,
                      int64_t j0, int64_t j1, void* stream);
/* N > 1 GPUs with REPLICATED factors (L, Y valid on every rank) and column-sparse constraints (the SCMcolumn2 route,
 * solvers.py:489-497, misc.c:620-663): caller `part` of `nparts` computes the columns of its contiguous share of the
 * column-sparse constraints (trsm x 2 + SCMcolumn2 per chunk) and, as part 0, the Gram block of the swept ones, into a
 * CLEARED H; one all-reduce (sum) of H over the callers completes the Schur complement (both triangles; a pair of sparse
 * constraints owned by two callers is written by the owner of the smaller index only).  Then dense_potrf on every rank. */
int kkt_schur_gram_part(csp_ctx* ctx, const double* L, const double* Y, double* H, int64_t ldh, int64_t part,
                        int64_t nparts, void* stream);
/* counts[0] = constraints swept through the Hessian, counts[1] = column-sparse ones (misc.nzcolumns / matperm,
 * misc.c:682-773; as classified by the last kkt_set_constraints under the current kkt_set_tnzcols). */
int kkt_constraint_classes(csp_ctx* ctx, int64_t* counts);
/* lapack.potrf / potrs on a dense device matrix (solvers.py:501,526). */
int dense_potrf(csp_ctx* ctx, double* A, int64_t n, int64_t lda, void* stream);
int dense_potrs(csp_ctx* ctx, const double* A, int64_t n, int64_t lda, double* B, int64_t nrhs,
                int64_t ldb, void* stream);
/* solve_ closure (solvers.py:506-541): given the factored H, overwrites bx (blkval) with x
 * and by (length m) with y for  [-kk*W^-1  A^adj; A 0][x;y] = [bx;by]. */
int kkt_solve(csp_ctx* ctx, const double* L, const double* Y, const double* H, int64_t ldh,
              double kk, double* bx, double* by, void* stream);
/* The same solve for a BLOCK of nrhs right-hand sides on one factorisation (solvers.py:506-541, the dense solve at 526): row r of
 * BX is a blkval at BX + r * ldbx, row r of BY a vector of length m at BY + r * ldby; every pair is overwritten with the
 * (x, y) kkt_solve computes for it, with the same kk for all rows.  Every stage is one launch sequence for the rows of a
 * chunk: the number of launches does not depend on nrhs within a chunk.  Entries of a row beyond blklen / m are never
 * written; L, Y and H are only read.  A row's result does not depend on what the other rows hold.
 * WORKSPACE.  The W(bx) of a chunk of c rows live in c rows of the constraint stack and the c x m temporaries behind
 * them: c + ceil(c m / blklen) <= max_rhs (csp_device_init).  A larger nrhs is processed in chunks of the largest such c
 * (kkt_solve_many_chunk), so any nrhs works on the workspace the context has; SMCP_ENOMEM when max_rhs < 2 or no c fits.
 * SMCP_EINVAL: nrhs < 1; ldh < m; ldbx < blklen or ldby < m with nrhs > 1; no constraints installed; BX, BY and H
 * overlapping one another by address range (nothing is written); a context under a subtree partition over more than one
 * rank (csp_set_partition: the sharded solve_ has no block form).
 * A Schur complement whose factorisation waits under csp_lazy_status is factored first, on `stream`, where it stands (no
 * side stream).  The Q factor of kkt_qr_factor is dropped as by kkt_solve, and a failure of chol(Y_AA) is reported or
 * latched as by kkt_solve.  Does not synchronise. */
int kkt_solve_many(csp_ctx* ctx, const double* L, const double* Y, const double* H, int64_t ldh, double kk, double* BX,
                   int64_t ldbx, double* BY, int64_t ldby, int64_t nrhs, void* stream);
/* The chunk rule of kkt_solve_many: the largest c with c + ceil(c m / blklen) <= max_rhs, 0 when max_rhs < 2 or none fits.
 * Host only: needs neither a context nor a device. */
int64_t kkt_solve_many_chunk(int64_t m, int64_t blklen, int64_t max_rhs);
/* L L^T Z = B for a block of nrhs columns (column r at B + r * ldb, ldb >= n) with a lower Cholesky factor A from anywhere
 * (dense_potrf, or uploaded: only the lower triangle is read).  n <= 128: one launch with the factor in LDS; beyond,
 * 2 ceil(n / 64) block steps spread over the chip, whatever nrhs is; the factor is read once per triangle and block of 32
 * columns.  The diagonal blocks are solved by substitution (no explicit inverse is formed or used, cached or not).  A, the
 * rows of A beyond n and the entries B[r * ldb + n ...] are not written; a column's result does not depend on the other
 * columns; the order of every sum is fixed.  SMCP_EINVAL: n < 1, lda < n, nrhs < 1, ldb < n with nrhs > 1, B overlapping
 * A.  Does not synchronise.  What kkt_solve_many calls; dense_potrs keeps its own routes. */
int dense_potrs_many(csp_ctx* ctx, const double* A, int64_t n, int64_t lda, double* B, int64_t nrhs, int64_t ldb, void* stream);
/* kkt_res (solvers.py:401-411) for a BLOCK of nrhs iterates, with the norms of the DEBUG check of solve_ (534-538)
 * (csrc/kkt_res_many.hip).  Rows as in kkt_solve_many: row r of XS / BX / RX is a blkval, row r of YS / BY / RY a vector of length m:
 *   RX_r = -kk * W^-1(XS_r) + Aadj(YS_r) - BX_r      (W^-1 = csp_hessian(L, Y, ., adj = 2, inv = 1))
 *   RY_r = Amap(XS_r) - BY_r
 * norms: device pointer to 4 * nrhs doubles, or null.  norms[4 r + 0 .. 3] = ||RX_r||, ||RY_r||, ||BX_r||, ||BY_r||: the blkval
 * norms are sqrt(dot(., .)) in the trace inner product of csp_dot (weight 1 on the diagonal of a supernode's diagonal block, 2 below
 * it, the slots above it are not summed), the vector norms are Euclidean.  They stay on the device: the call does not wait for them.
 * XS, YS, BX, BY, L and Y are only read; entries of a row of RX / RY beyond blklen / m are never written; a row's results are a
 * function of that row alone.  What RX holds in the slots above the diagonal of a diagonal block is not specified.
 * Needs the constraints and nothing else: no Schur complement, no Q; the constraint stack is not written, so the call is valid
 * after kkt_schur_factor, after kkt_qr_factor (whose Q stays valid) or after neither.
 * chol(Y_AA) and the inverse-form factors are prepared as csp_hessian(inv = 1) prepares them and the status of that preparation is
 * returned as csp_hessian returns it (latched under csp_lazy_status); when they are cached for Y -- after any factor or solve on the
 * pair -- nothing is read back and the call does not synchronise.  The inverse Hessian goes in chunks of max_rhs rows; the number
 * of launches of a chunk does not depend on the rows in it.
 * WORKSPACE, in the context's ledger (csp_device_bytes), released with the constraint set: blklen int32 (blkval position -> entry of
 * Aadj, built at the first call after kkt_set_constraints; that call waits for the stream once) and min(max_rhs, 65535) * 1026
 * doubles of partial sums.  Neither grows afterwards.
 * Every sum has an order fixed by the shapes (a fixed partition of the positions, per-workgroup partial sums, one fixed-order
 * final pass): the same RX gives the same norms bit for bit, and under CSP_TUNE_DETERMINISTIC the whole call repeats bit for bit.
 * SMCP_EINVAL, nothing written: nrhs < 1; a leading dimension below blklen / m with nrhs > 1; no constraints installed; a null
 * pointer among the eight blocks, L or Y; RX or RY overlapping, by address range, an input block, L, Y, each other or norms; norms
 * overlapping an input; a context under a subtree partition over more than one rank. */
int kkt_residual_many(csp_ctx* ctx, const double* L, const double* Y, double kk, const double* XS, int64_t ldxs,
                      const double* YS, int64_t ldys, const double* BX, int64_t ldbx, const double* BY, int64_t ldby,
                      double* RX, int64_t ldrx, double* RY, int64_t ldry, double* norms, int64_t nrhs, void* stream);
/* The update of a refinement round for a block: XS_r <- XS_r - DX_r over the blkval, YS_r <- YS_r - DY_r over the m entries, one
 * launch for all rows (65535 rows per launch).  Entries of a row beyond blklen / m are neither read nor written.  SMCP_EINVAL:
 * nrhs < 1, a short leading dimension with nrhs > 1, no constraints installed (m is theirs), a null pointer, XS or YS overlapping
 * another block.  Does not synchronise. */
int kkt_update_many(csp_ctx* ctx, double* XS, int64_t ldxs, double* YS, int64_t ldys, const double* DX, int64_t lddx,
                    const double* DY, int64_t lddy, int64_t nrhs, void* stream);

/* kkt_qr(solvers.py:413-475 feas, 1843-1905 esd): the QR-based KKT solver.  kkt_qr_factor builds the stack of
 * half-Hessian images of ALL m constraints (call kkt_set_tnzcols(ctx, 0) before kkt_set_constraints: the reference
 * does not split off column-sparse constraints on this path, solvers.py:242,551-556) and factors it, At = Q R, by
 * Cholesky-QR iterations on the device (csrc/kkt_qr.hip; a shifted first pass when chol(At^T At) breaks down).  Q
 * (orthonormal in the Schur complement's inner product) stays on the device in place of the stack, R^T as an m x m
 * lower-triangular matrix.  *passes (optional) receives the number of passes taken, *shift the relative shift of
 * the first pass (0: none).  Returns 0, a negative error, or j+1 > 0 when chol(Y_AA) of a clique or the Gram
 * matrix is not positive definite (lapack.geqrf's ArithmeticError at solvers.py:425-428 has no counterpart: a
 * rank-deficient stack shows up here).  any m (factors wider than 320 columns are processed in panels of 256).
 * kkt_qr_solve is its solve_ closure (solvers.py:430-471): overwrites bx (blkval) with x and by (length m) with y;
 * valid until the next call that rewrites the stack (kkt_qr_factor, kkt_schur_*, kkt_solve, kkt_gram_*).
 * NOT sharded: Q lives on one device.  After csp_set_partition with more than one owning rank kkt_qr_factor returns
 * SMCP_EINVAL (the multi-GPU step uses kkt_chol: kkt_gram_* / csp_*_part); a partition of one rank is accepted. */
int kkt_qr_factor(csp_ctx* ctx, const double* L, const double* Y, int64_t* passes, double* shift, void* stream);
int kkt_qr_solve(csp_ctx* ctx, const double* L, const double* Y, double kk, double* bx, double* by, void* stream);
/* test hook: Rt_host (m*m doubles, host, optional) <- R^T (lower, column-major); G_dev (m*m doubles, device,
 * optional) <- Gram matrix of the current stack in the weighted inner product (Q^T Q; the identity after a
 * factorisation).  Synchronises the stream. */
int kkt_qr_inspect(csp_ctx* ctx, double* Rt_host, double* G_dev, void* stream);
/* kkt_qr_solve for a BLOCK of nrhs right-hand sides on one kkt_qr_factor (csrc/kkt_qr_many.hip): row r of BX is a blkval at
 * BX + r * ldbx, row r of BY a vector of length m at BY + r * ldby; every pair is overwritten with the (x, y) kkt_qr_solve
 * computes for it, with the same kk for all rows.  Q is read twice per chunk of rows instead of twice per row; every stage is
 * one launch sequence for the rows of a chunk.  Entries of a row beyond blklen / m are never written; L, Y, Q and R are only
 * read: THE Q FACTOR STAYS VALID and kkt_qr_solve keeps working afterwards.  A row's result does not depend on what the other
 * rows hold.
 * CHUNKS.  A chunk is min(max_rhs, 16) rows (kkt_qr_solve_many_chunk): what the Hessian sweeps take on this context, capped at
 * the sixteen columns of one tile of the two products with Q.  A larger nrhs is processed in chunks of that size.
 * WORKSPACE.  (ceil(blklen / p) + 2) * 16 * m doubles with p = 2048 * ceil(blklen / 2^22) -- at most (ceil(blklen / 2048) + 2) * 16 * m
 * -- of its own in the context's ledger (csp_device_bytes), allocated at the first call and kept; the workspace of kkt_qr_factor, which holds R, is not touched.
 * SMCP_EINVAL, nothing written: nrhs < 1; ldbx < blklen or ldby < m with nrhs > 1; no constraints installed; no valid Q, or Q
 * factored for another (L, Y) (as kkt_qr_solve); BX and BY overlapping by address range; BX or BY overlapping the stack or a QR
 * workspace; a context under a subtree partition over more than one rank.  The any-size route (CSP_TUNE_DETERMINISTIC /
 * SMCP_GENERIC) is accepted, as by kkt_qr_solve (kkt_qr_factor refuses it): the Hessian sweeps then sum in a fixed order, as the
 * kernels of this call always do, and the same call gives the same bits on every pattern -- on the default route only where the
 * sweeps themselves do (no small front with several children).
 * chol(Y_AA) is formed again when another factorisation has replaced it in the cache, as by kkt_qr_solve, which reads no
 * verdict of it back; under csp_lazy_status a failure is latched for csp_status.  Does not synchronise. */
int kkt_qr_solve_many(csp_ctx* ctx, const double* L, const double* Y, double kk, double* BX, int64_t ldbx, double* BY,
                      int64_t ldby, int64_t nrhs, void* stream);
/* The chunk rule of kkt_qr_solve_many: min(max_rhs, 16), 0 when max_rhs < 1.  Host only: needs neither a context nor a device. */
int64_t kkt_qr_solve_many_chunk(int64_t max_rhs);

/* ---- subtree-sharded multi-GPU Schur complement (Gram formulation) ---------------------------
 * The elimination tree is cut into subtrees owned by single ranks plus a replicated top
 * (owner[k] = rank, or -1 for the top).  Per solve: kkt_gram_prepare; for every chunk of right-hand
 * sides: kkt_gram_sweep(set 1 = owned) -> exchange of the subtree roots' packed update blocks
 * (csp_exchange_pack -> one all-gather -> csp_exchange_unpack) -> kkt_gram_sweep(set 2 = top); then kkt_gram_accumulate over
 * the blkval ranges this rank owns and one all-reduce of H. */
int csp_set_partition(csp_ctx* ctx, const int32_t* owner, int rank);
int kkt_gram_prepare(csp_ctx* ctx, const double* L, const double* Y, void* stream);
int kkt_gram_sweep(csp_ctx* ctx, int set, int64_t j0, int64_t j1, void* stream);
int kkt_gram_accumulate(csp_ctx* ctx, int64_t nranges, const int64_t* ranges, double* H, int64_t ldh,
                        void* stream);
/* boundary exchange (after csp_set_partition): doubles per right-hand side every rank contributes; pack of THIS rank's
 * subtree roots into buf ([root][rhs][packed block]); unpack of all OTHER ranks' roots from the all-gathered buffers
 * (`width` doubles per rank).  One launch each, no host synchronisation. */
int csp_exchange_sizes(csp_ctx* ctx, int64_t world, int64_t* sizes_per_rhs);
int csp_exchange_pack(csp_ctx* ctx, int64_t nrhs, double* buf, void* stream);
int csp_exchange_unpack(csp_ctx* ctx, int64_t nrhs, const double* buf, int64_t width, void* stream);
/* The exchange BY CONSTRAINT SHARE (the top of the tree sharded by constraint: rank q sweeps the top for its share J_q of the
 * constraints only, instead of every rank for all of them; SURVEY 8e "one exchange step per sweep", as an all-to-all):
 * after kkt_gram_sweep(set 1) over a chunk, csp_exchange_pack_range packs the right-hand sides r0 .. r0 + nrhs - 1 of that chunk
 * -- the share of ONE destination rank -- as [root][rhs][packed block] (once per destination, into that destination's slot of
 * the all-to-all's send buffer); csp_exchange_unpack_all unpacks the roots of EVERY rank, this one's too, from the receive
 * buffer (`width` doubles per source rank) into the slots 0 .. nrhs - 1, where kkt_gram_sweep(set 2, c0, c1) of the own share
 * reads them.  kkt_stack_rows moves the rows [a, b) of the swept stack of the constraints j0 .. j1 - 1 to / from
 * buf[(j - j0) (b - a) + row - a] (dir 0: stack -> buf, 1: buf -> stack): the top's panels of a share travel to the rank that
 * accumulates the top's block of H. */
int csp_exchange_pack_range(csp_ctx* ctx, int64_t r0, int64_t nrhs, double* buf, void* stream);
int csp_exchange_unpack_all(csp_ctx* ctx, int64_t nrhs, const double* buf, int64_t width, void* stream);
int kkt_stack_rows(csp_ctx* ctx, int dir, int64_t j0, int64_t j1, int64_t a, int64_t b, double* buf, void* stream);
/* The boundary blocks of a sweep whose input is a linear combination of inputs that were swept (and exchanged) before
 * need no collective: the second Hessian of solve_ is applied to Aadj(y) - bx (solvers.py:528-531), so the other
 * ranks' root blocks are sum_i y_i (blocks gathered for constraint i during the Schur sweeps) - (blocks gathered for
 * bx).  gbuf: the gathered buffer of a chunk of nrhs constraints (region width gwidth per rank), y: its nrhs
 * multipliers (device), out: a buffer in the layout of a one-right-hand-side gather (region width owidth);
 * mode 0: out <- sum - out (out holds the blocks of bx), mode 1: out <- out + sum (further chunks). */
int csp_exchange_combine(csp_ctx* ctx, int64_t nrhs, const double* y, const double* gbuf, int64_t gwidth, double* out,
                         int64_t owidth, int mode, void* stream);

/* ---- subtree-sharded factorisation and solve (every leaves->root / root->leaves sweep of the path
 * shards; reference call sites of the sweeps: solvers.py:881-891 cholesky + projected_inverse, 521-532 the two
 * Hessians of solve_).  set: 1 = the cliques this rank owns, 2 = the replicated top.
 *   leaves->root (cholesky, hessian dir 0): part(set 1) -> csp_exchange_pack / all-gather / csp_exchange_unpack of the subtree roots' packed updates
 *     (nrhs = 1) around one collective -> part(set 2);
 *   root->leaves (projected_inverse, kkt_prepare_part, hessian dir 1): part(set 2) -> part(set 1), no communication.
 * After them a matrix is valid on the owned cliques and the top; the other blkval ranges keep what they held.
 * kkt_prepare_part: Y_AA blocks and their Cholesky factors (and, with_lk != 0, the inverse-form factor of L) of one set;
 * kkt_gram_prepare_part: what is left of kkt_gram_prepare once both sets are prepared;
 * csp_hessian_sweep_part: one half of hessian(L, Y, U, adj=None, inv=False) over one set (dir 0 up, 1 down).
 * The prepared state lives in the context's shared lk / yaa / fac buffers: any call that rewrites them for other
 * matrices (csp_projected_inverse, csp_hessian, kkt_* on another pair) makes the sweeps return SMCP_ESTALE until
 * kkt_prepare_part (with_lk = 1) has been called again for set 2, then set 1. */
int csp_cholesky_part(csp_ctx* ctx, double* blkval, int set, void* stream);
int csp_projected_inverse_part(csp_ctx* ctx, double* blkval, int set, void* stream);
int kkt_prepare_part(csp_ctx* ctx, const double* L, const double* Y, int set, int with_lk, void* stream);
int kkt_gram_prepare_part(csp_ctx* ctx, void* stream);
int csp_hessian_sweep_part(csp_ctx* ctx, double* U, int64_t nrhs, int64_t ldu, int set, int dir, void* stream);

/* ---- derived-quantity cache ------------------------------------------------------------
 * csp_hessian, csp_completion and the kkt_* entry points keep quantities derived from their (L, Y)
 * arguments on the device (the inverse-form factor of L, the separator blocks Y_AA, their Cholesky
 * factors and the inverses of those), keyed by the DEVICE ADDRESS of L and Y, so that the many
 * Hessian applications of one interior-point iteration (solvers.py:803-1050: kkt_res, Newton
 * decrements, step computation) do not redo them.  Every entry point of this library that writes
 * to a buffer drops the cache entries derived from it.  A caller that changes the contents of L or
 * Y by any other means (its own kernels, memcpy) must call csp_cache_reset() before the next call. */
int csp_cache_reset(csp_ctx* ctx);
/* The explicit form of that contract: the caller has written to the matrix (or right-hand side) stored at `ptr` by
 * means the library cannot see -- the reference does so with blas.scal(a, X.blkval) (solvers.py:407, 905) -- and
 * whatever was derived from the old contents at that address is dropped (cheaper than csp_cache_reset: quantities
 * derived from other matrices stay). */
int csp_touch(csp_ctx* ctx, const void* ptr);

/* ---- tuning / debugging knobs ------------------------------------------------------------ */
#define CSP_TUNE_LEAFGRAM 1       /* closed-form Gram blocks of childless small cliques (front_leafgram.hip): 0 never,
                                     1 when the entry lists are short enough to beat the panel route (default), 2 always */
#define CSP_TUNE_VERIFY_CACHE 2   /* 1: every reuse of a cached derived quantity first checks a fingerprint of the matrix
                                     it was derived from -- every entry of every panel, one pass over blkval + a stream
                                     synchronisation per reuse (which makes csp_lazy_status pointless while it is on: a
                                     debug aid); a caller that forgot csp_touch gets SMCP_ESTALE instead of stale factors */
#define CSP_TUNE_DETERMINISTIC 3  /* 1: every sum in a fixed order (no floating-point atomics): results are bit-identical
                                     from run to run; slower */
#define CSP_TUNE_PLACEMENT 4      /* value = tries (1..16): an ACTION, not a setting -- call it after kkt_set_constraints.  The
                                     family sweep of the Schur complement streams into two multi-GB buffers at once, and how fast
                                     the memory system takes that depends on where the buffers physically lie (+-20 % on that
                                     kernel from one allocation to the next).  A store-only probe of the pattern is timed, the
                                     two buffers -- the packed exchange buffer and the swept stack -- are moved in turn to fresh
                                     allocations, `tries` in all, and the fastest placement is kept (a few ms per try; the buffers
                                     set aside are freed at the end: up to 16 GB of transient memory).  The contents of both
                                     buffers are NOT preserved (the probe zeroes the family parents' panels and update slots):
                                     call it between Newton steps; a kkt_qr factor held in the stack is invalidated and
                                     kkt_qr_solve returns SMCP_EINVAL until the next kkt_qr_factor.  Worth it for runs of many
                                     Newton steps on one problem; off unless called */
#define CSP_TUNE_RACE 5           /* value = seed (low 32 bits; 0: off) | longest delay in us << 32 (0: 200), PROCESS-wide: delay injection for race hunting -- a spin kernel of a
                                     seeded random 5 .. 200 us at the head and tail of every internal side-stream branch, behind every
                                     fork on the caller's stream and before one launch in four (tools/race_hunt.sh; the environment
                                     variable SMCP_RACE=<seed> does the same from the first call on).  Results must not change. */
#define CSP_TUNE_RACE_DROP_JOINS 6 /* 1: the harness's own sensitivity test -- side branches are no longer joined (their join event is
                                     recorded, the caller's stream does not wait for it): results are WRONG by design and must
                                     change under CSP_TUNE_RACE, which is what tests/test_gpu_parity.py asserts.  0: back to normal
                                     (waits for the device).  PROCESS-wide. */
#define CSP_TUNE_CEIG_WIDE 7      /* per context: the smallest order of a clique whose spectrum (csp_clique_eigvalsh with
                                     and without b, csp_clique_eigh, csp_clique_project) is computed by the
                                     chip-wide block Jacobi of front_ceigw.hip (pivots of two 32-column blocks on one workgroup
                                     each, 64 x 64 tile products on the matrix cores over all compute units) instead of one
                                     workgroup per clique; 0 (default): never.  1 .. 64 and negative values: SMCP_EINVAL (the
                                     route needs three blocks).  csp_cone_project_steps sends the same cliques through it in
                                     every iteration, by a fixed chain of launches that reads nothing back; the first call
                                     after the value changed builds its lists again and may wait.  The pencil form (b given) reduces (A_gg, B_gg) to standard
                                     form by tiles over the chip first.  With 0
                                     every call gives the bits it gave before the route existed; with it set, results are
                                     still the same bits from call to call.  Recommended value: 65 (the smallest
                                     scanned value at which the route was not slower than 0 on config 4 and on synth50k) */
#define CSP_TUNE_SLOT_DOUBLES 8   /* per context: the doubles that the slots in device memory of one launch of the completions and
                                     clique spectra, or the workspace of one launch group of wide cliques (CSP_TUNE_CEIG_WIDE), may
                                     take; 0 (default): 2^25, 256 MiB.  Negative: SMCP_EINVAL.  Needs no device; holds from the next
                                     call on (csp_cone_project_steps builds its lists again and may wait).  A launch always keeps
                                     one slot and a group one clique, so 1 means one workgroup walking every such clique of a
                                     launch through one slot, and one wide clique per group.  It exists so that the tests can run
                                     the slot-sharing loop of those kernels and the group split at small sizes (at the default
                                     both need about a thousand cliques of more than 126 rows in one launch); a caller may also
                                     use it to cap workspace memory.  Results do not depend on it, bit for bit; what it changed is
                                     read with CSP_Q_SLOT_SHARE and CSP_Q_CEIG_GROUPS */
int csp_tune(csp_ctx* ctx, int what, int64_t value);
/* out[0], out[1]: milliseconds of the store-pattern probe of the last CSP_TUNE_PLACEMENT before / after (zeros: not run);
 * out[2]: delay kernels injected so far in this process (CSP_TUNE_RACE).  out holds three doubles. */
int csp_tune_report(csp_ctx* ctx, double* out);

/* ---- measurement hooks (bench.py roofline leg) --------------------------------------- */
/* When enabled every kernel launch is bracketed by HIP events on its own stream. */
int csp_profile_enable(csp_ctx* ctx, int on);
/* Restrict the timing to launches of one kernel id (so that a throughput measurement can carry the HIP events of
 * its dominant kernel without paying for events around every launch); kid < 0 times all kernels again. */
int csp_profile_filter(csp_ctx* ctx, int kid);
/* Number of kernel kinds = required length of the arrays passed to csp_profile_read. */
int64_t csp_profile_kinds(void);
/* Synchronises, then writes per-kernel accumulated milliseconds and launch counts (host arrays of
 * csp_profile_kinds() entries; the return value repeats that length) and clears the record. */
int64_t csp_profile_read(csp_ctx* ctx, double* ms, int64_t* count);
const char* csp_profile_kernel_name(int kid);

/* ---- launch census: launches per kernel FUNCTION ------------------------------------------------ */
/* The ids of csp_profile_* stand for groups of kernels (a template's instantiations, the kernels of a unit launched
 * under one id).  The census counts every launch under the kernel function that was launched, one entry per template
 * instantiation.  Off by default; when on, a launch costs one counter increment (no events, no name look-up).
 * csp_census_enable needs no device, so it may be called before csp_device_init to see the set-up kernels. */
int csp_census_enable(csp_ctx* ctx, int on);
/* Synchronises as csp_profile_read does, then writes one line "mangled<TAB>pretty<TAB>count\n" per kernel launched
 * since the last successful read (a NUL-terminated text, sorted by mangled name) and clears the counts.  pretty is the
 * demangled name without namespace and parameter list: k_ceigw_solve<true>, k_hess_down_fam<3, 2>.  Returns the bytes
 * needed, the terminating NUL included; when buf is NULL or cap is smaller than that, nothing is written and nothing
 * is cleared: call again with a buffer of that size.  Negative: an SMCP_E* code. */
int64_t csp_census_read(csp_ctx* ctx, char* buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif
