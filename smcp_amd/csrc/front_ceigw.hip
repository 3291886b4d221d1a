// Spectra of WIDE clique blocks on the whole chip (csp_tune(CSP_TUNE_CEIG_WIDE)): a two-sided block
// Jacobi in standard form, for the cliques that k_ceig / k_ceig_vec (front_ceig.hip) would run from a slot in device memory
// on one workgroup.  Block width CW_B = 32; a clique of order nf has nb = ceil(nf / 32) column blocks (the last may be
// narrower), at least three.  Per clique, in device memory (CeigwDesc): F in full, V (with eigenvectors; starts as I), per
// pair of a step the orthogonal factor U (ld 64) and the eigenvalues of its pivot, a flag per pair, a slot per tile for
// the largest |off-diagonal entry|, |F|_F and the stop threshold, the status.
//
// A block sweep is the round-robin tournament of ceig_pair on the nb blocks: nb - 1 steps (nb for odd nb) of h = ceil(nb / 2)
// disjoint block pairs; for odd nb the block that meets the phantom player is a "pair" of that block alone.  A step is two
// launches:
//   k_ceigw_pivot, a workgroup per (clique, pair P = (I, J)): the pivot block [F_II F_IJ; F_JI F_JJ] (order m <= 64) into
//     LDS, ceig_jacobi<true> on it as it stands (its skip and stop rules relative to the pivot), then the rank sort of
//     k_ceig_vec: U_P = the accumulated rotations with their columns in ascending order of the pivot's eigenvalues, and those
//     eigenvalues, to memory; flag[P] = no sweep was taken and no column moved (U_P = I);
//   k_ceigw_apply, a workgroup per 64 x 64 tile (P, Q), P >= Q, of F in the pair coordinates of the step:
//     T <- U_P^T T U_Q by two wg_mma products from LDS, written in place and mirrored to (Q, P).  Every tile has one owner
//     and an owner reads nothing but its own tile (P, Q) of F, so a launch has no hazard between workgroups; no atomics, no
//     waits.  A diagonal tile (P, P) is not multiplied: it is set to diag(eigenvalues of the pivot) with exact zeros, as
//     ceig_jacobi sets its 2 x 2 blocks -- this is what lets the stop rule be met (section 22).  A tile with both flags
//     raised is only read.  Every workgroup leaves the largest |entry| of its tile (0 for a diagonal tile) in its slot.
//     Further workgroups of the same launch: V[64 rows, Q] <- V[64 rows, Q] U_Q.
// k_ceigw_check, one workgroup, at the start of every block sweep: per running clique the maximum over its slots; the rule
// of k_ceig on the whole block (max |off-diagonal| <= eps |F|_F ends the clique, CEIG_MAX_SWEEPS block sweeps flag it), and
// the number of cliques still running for the host.  A clique that has ended does nothing in later launches.
// k_ceigw_sort / k_ceigw_out: the rank sort of the diagonal (ties by index) into w, then V by rank into Q (vmode 0) or the
// projection of k_ceig_vec (vmode 1), entries spread over the workgroups of a launch.
// Every sum and maximum is a fixed tree or one thread's loop: the same input gives the same bits; the arithmetic on F does
// not depend on V, so w has the same bits with and without eigenvectors.
// The pencil form (csp_clique_eigvalsh with b): G = B_gg beside F, and between k_ceigw_form and
// k_ceigw_begin the reduction F <- R^-1 F R^-T, G = R R^T, on tiles of CW_T rows (k_ceigw_potrf / _panel / _trail / _solve /
// _symm, described where they stand); the chain above then runs unchanged.
// The clique step of csp_cone_project_steps on the same cliques, at the end of the file:
// k_ceigw_cone_form (F = T_k) in the place of k_ceigw_form, the kernels above unchanged in a chain of fixed length that the
// host never looks into, then k_ceigw_sort, k_ceigw_cone_split (U_k and W_k per entry of the lower triangle, the partial
// sums of r_k^2) and k_ceigw_cone_finish (pinfo, rank, flag) in the place of k_ceigw_out.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "context.hpp"
#include "wgblas.hpp"

namespace smcp {

constexpr int CW_B = 32, CW_T = 64, CW_LD = 65;       // block width, tile order, leading dimension of a tile in LDS
constexpr int CW_STATE = 8;                           // status integers per clique (below)
constexpr int CW_DONE = 0, CW_SWEEPS = 1, CW_NOCONV = 2, CW_NLO = 3, CW_NHI = 4, CW_NNEG = 5;
constexpr int CW_NOTPD = 6;                           // pencil mode: a diagonal tile of B_gg met a pivot that is not > 0
constexpr int CW_VMODE_CONE = 2;                      // MrcArgs::vmode of the cone pass (k_ceigw_cone_*)
constexpr size_t CW_APPLY_LDS = (size_t)3 * CW_T * CW_LD * sizeof(double);
constexpr size_t CW_PIVOT_LDS = (size_t)2 * CW_T * CW_T * sizeof(double);

// One wide clique of a call: offsets in doubles into the workspace.  h: pairs of a step.  V: -1 without eigenvectors.
// G: B_gg in full and then its Cholesky factor (pencil mode), -1 in standard form.
struct CeigwDesc {
  int32_t k, nf, nb, h;
  int64_t F, V, U, ev, slot, sw, st, ints, G;
};
// doubles of the workspace of one clique and its layout from `base` on; pencil: room for G behind V (no other offset moves
// without it)
__host__ inline int64_t ceigw_layout(CeigwDesc& w, int32_t k, int64_t nf, bool vec, int64_t base, bool pencil = false) {
  w.k = k;
  w.nf = (int32_t)nf;
  w.nb = (int32_t)((nf + CW_B - 1) / CW_B);
  w.h = (w.nb + 1) / 2;
  int64_t o = base;
  w.F = o; o += nf * nf;
  w.V = vec ? o : -1; o += vec ? nf * nf : 0;
  w.G = pencil ? o : -1; o += pencil ? nf * nf : 0;
  w.U = o; o += (int64_t)w.h * CW_T * CW_T;
  w.ev = o; o += (int64_t)w.h * CW_T;                  // (>= nf doubles: k_ceigw_sort keeps the diagonal here)
  w.slot = o; o += (int64_t)w.h * (w.h + 1) / 2;
  w.sw = o; o += nf;
  w.st = o; o += 2;
  w.ints = o; o += (2 * nf + w.h + CW_STATE + 1) / 2;
  return (o - base + 31) / 32 * 32;
}

struct CeigwView {
  double *F, *V, *G, *U, *ev, *slot, *sw, *st;
  int32_t *rk, *col, *uflag, *state;
};
__device__ inline CeigwView ceigw_view(const CeigwDesc& w, double* ws) {
  CeigwView v;
  v.F = ws + w.F; v.V = w.V >= 0 ? ws + w.V : nullptr; v.G = w.G >= 0 ? ws + w.G : nullptr; v.U = ws + w.U; v.ev = ws + w.ev; v.slot = ws + w.slot;
  v.sw = ws + w.sw; v.st = ws + w.st;
  v.rk = (int32_t*)(ws + w.ints); v.col = v.rk + w.nf; v.uflag = v.col + w.nf; v.state = v.uflag + w.h;
  return v;
}

// MrcArgs m as k_ceig_vec reads them (standard form); wd / nw: the wide cliques of this launch group, ws: their workspace,
// vec: eigenvectors are accumulated; nrun: the cliques still running (k_ceigw_check); pencil: m.x2 / m.upd2 hold B and the
// reduction to standard form runs between k_ceigw_form and k_ceigw_begin
struct CeigwArgs {
  MrcArgs m;
  const CeigwDesc* wd;
  double* ws;
  int nw, vec;
  int32_t* nrun;
  int pencil;
};

// pair t of step r on the nb blocks of a clique of order nf: rows r0 .. r0 + n0 of block I, then r1 .. r1 + n1 of block J
// (n1 = 0: block I alone)
struct CeigwPair { int r0, n0, r1, n1; };
__device__ inline CeigwPair ceigw_pair(int nf, int nb, int r, int t) {
  int p, q;
  ceig_pair(nb + (nb & 1), r, t, p, q);
  CeigwPair P;
  P.r0 = p * CW_B; P.n0 = min(CW_B, nf - P.r0);
  P.r1 = q * CW_B; P.n1 = q < nb ? min(CW_B, nf - P.r1) : 0;
  return P;
}
__device__ inline int ceigw_row(const CeigwPair& P, int a) { return a < P.n0 ? P.r0 + a : P.r1 + (a - P.n0); }

__device__ inline double ceigw_nanmax(double x, double y) { return (y > x || y != y) ? y : x; }

// F = A_gg in full (ceig_form on gridDim.x workgroups per clique), V = I; pencil mode: G = B_gg in full as well, and the two
// status words that the reduction reads before k_ceigw_begin has run
__global__ void __launch_bounds__(MRC_NT) k_ceigw_form(CeigwArgs a) {
  const CeigwDesc w = a.wd[blockIdx.y];
  const CeigwView v = ceigw_view(w, a.ws);
  const CliqueDesc d = a.m.cl[w.k];
  ceig_form(d, a.m.x + d.blk, a.m.upd + d.upd, v.F, blockIdx.x, gridDim.x);
  if (a.pencil) {
    ceig_form(d, a.m.x2 + d.blk, a.m.upd2 + d.upd, v.G, blockIdx.x, gridDim.x);
    if (blockIdx.x == 0 && SMCP_TID == 0) v.state[CW_DONE] = v.state[CW_NOTPD] = 0;
  }
  if (a.vec)
    for (int e = blockIdx.x * MRC_NT + SMCP_TID; e < w.nf * w.nf; e += gridDim.x * MRC_NT) v.V[e] = (e % (w.nf + 1) == 0) ? 1.0 : 0.0;
}

// ---- pencil mode: F <- R^-1 F R^-T with G = R R^T, between k_ceigw_form and k_ceigw_begin ----------
// Tiles of CW_T rows: nt = ceil(nf / CW_T), the last one may be a single row.  Only the tiles (i, l), i >= l, of G are kept
// up: they end as R (a diagonal tile with zeros above its diagonal); the tiles above stay B_gg and nobody reads them.
// The launches, for the most tiles ntmax of a group: per block column j a k_ceigw_potrf (the diagonal tile), and for
// j < ntmax - 1 a k_ceigw_panel (the tiles below it) and a k_ceigw_trail (the tiles right of the panel); then k_ceigw_lsolve,
// k_ceigw_rsolve, k_ceigw_symm: 3 ntmax + 1, whatever the data.  Every tile written in a launch has one owner, which reads
// beside it only what earlier launches wrote, or (the slab solves) what it wrote itself.  No atomics, no waits.
// A pivot that is not > 0 (a NaN is not): k_ceigw_potrf raises CW_NOTPD and CW_DONE, and every later launch of the chain
// returns at its top for that clique.
__device__ inline int ceigw_tn(int nf, int t) { return min(CW_T, nf - t * CW_T); }
__device__ inline int ceigw_nt(int nf) { return (nf + CW_T - 1) / CW_T; }
// the mr x mc tile at (r0, c0) of the matrix M of order nf to and from a tile in LDS
__device__ inline void ceigw_tile_in(const double* M, int nf, int r0, int mr, int c0, int mc, double* T) {
  for (int e = SMCP_TID; e < mr * mc; e += MRC_NT) T[e % mr + (e / mr) * CW_LD] = M[(r0 + e % mr) + (int64_t)(c0 + e / mr) * nf];
}
__device__ inline void ceigw_tile_out(double* M, int nf, int r0, int mr, int c0, int mc, const double* T) {
  for (int e = SMCP_TID; e < mr * mc; e += MRC_NT) M[(r0 + e % mr) + (int64_t)(c0 + e / mr) * nf] = T[e % mr + (e / mr) * CW_LD];
}

// Block column j, one workgroup per clique: G_jj = R_jj R_jj^T by wg::potrf in LDS
__global__ void __launch_bounds__(MRC_NT) k_ceigw_potrf(CeigwArgs a, int j) {
  extern __shared__ double mrc_lds[];
  const CeigwDesc w = a.wd[blockIdx.x];
  const int nf = w.nf;
  if (j >= ceigw_nt(nf)) return;
  const CeigwView v = ceigw_view(w, a.ws);
  if (v.state[CW_DONE]) return;
  double* T = mrc_lds;
  const int o = j * CW_T, n = ceigw_tn(nf, j);
  ceigw_tile_in(v.G, nf, o, n, o, n, T);
  __syncthreads();
  if (wg::potrf(n, T, CW_LD)) {                        // (uniform)
    if (SMCP_TID == 0) v.state[CW_NOTPD] = v.state[CW_DONE] = 1;
    return;
  }
  for (int e = SMCP_TID; e < n * n; e += MRC_NT) v.G[(o + e % n) + (int64_t)(o + e / n) * nf] = e % n >= e / n ? T[e % n + (e / n) * CW_LD] : 0.0;
}

// Block column j, tile i = j + 1 + blockIdx.x of clique blockIdx.y: G_ij <- G_ij R_jj^-T
__global__ void __launch_bounds__(MRC_NT) k_ceigw_panel(CeigwArgs a, int j) {
  extern __shared__ double mrc_lds[];
  const CeigwDesc w = a.wd[blockIdx.y];
  const int nf = w.nf, i = j + 1 + (int)blockIdx.x;
  if (i >= ceigw_nt(nf)) return;
  const CeigwView v = ceigw_view(w, a.ws);
  if (v.state[CW_DONE]) return;
  double* T = mrc_lds;
  double* R = T + CW_T * CW_LD;
  const int oi = i * CW_T, mi = ceigw_tn(nf, i), oj = j * CW_T;
  ceigw_tile_in(v.G, nf, oi, mi, oj, CW_T, T);
  ceigw_tile_in(v.G, nf, oj, CW_T, oj, CW_T, R);
  __syncthreads();
  wg::trsm_rlT(mi, CW_T, R, CW_LD, T, CW_LD);
  ceigw_tile_out(v.G, nf, oi, mi, oj, CW_T, T);
}

// Block column j, clique blockIdx.y, blockIdx.x: tile (i, l) = (j + 1 + P, j + 1 + Q), P >= Q: G_il <- G_il - G_ij G_lj^T
__global__ void __launch_bounds__(MRC_NT) k_ceigw_trail(CeigwArgs a, int j) {
  extern __shared__ double mrc_lds[];
  const CeigwDesc w = a.wd[blockIdx.y];
  const int nf = w.nf;
  int x = blockIdx.x, Pi = 0;
  while (x > Pi) { x -= Pi + 1; ++Pi; }
  const int i = j + 1 + Pi, l = j + 1 + x;
  if (i >= ceigw_nt(nf)) return;
  const CeigwView v = ceigw_view(w, a.ws);
  if (v.state[CW_DONE]) return;
  double* Li = mrc_lds;
  double* Ll = Li + CW_T * CW_LD;
  const int oi = i * CW_T, mi = ceigw_tn(nf, i), ol = l * CW_T, ml = ceigw_tn(nf, l), oj = j * CW_T;
  ceigw_tile_in(v.G, nf, oi, mi, oj, CW_T, Li);
  ceigw_tile_in(v.G, nf, ol, ml, oj, CW_T, Ll);
  __syncthreads();
  double* G = v.G;
  wg_mma(mi, ml, CW_T, [=](int r, int kk) { return Li[r + kk * CW_LD]; }, [=](int kk, int c) { return Ll[c + kk * CW_LD]; },
         [=](int r, int c, double s) { G[(oi + r) + (int64_t)(ol + c) * nf] -= s; });
}

// One workgroup per slab of CW_T columns (LEFT: F <- R^-1 F) or of CW_T rows (F <- F R^-T) of clique blockIdx.y: it walks the
// tiles of its slab in order, tile t <- (tile t - the sum over k < t, ascending, of the products with the tiles it has
// already solved) and then the solve with R_tt, in LDS; the slabs of a launch are independent.
template <bool LEFT>
__global__ void __launch_bounds__(MRC_NT) k_ceigw_solve(CeigwArgs a) {
  extern __shared__ double mrc_lds[];
  const CeigwDesc w = a.wd[blockIdx.y];
  const int nf = w.nf, nt = ceigw_nt(nf), sl = blockIdx.x;
  if (sl >= nt) return;
  const CeigwView v = ceigw_view(w, a.ws);
  if (v.state[CW_DONE]) return;
  double* T = mrc_lds;
  double* R = T + CW_T * CW_LD;
  double* X = R + CW_T * CW_LD;
  const int os = sl * CW_T, ms = ceigw_tn(nf, sl);
  for (int t = 0; t < nt; ++t) {
    const int ot = t * CW_T, mt = ceigw_tn(nf, t);
    if (LEFT) ceigw_tile_in(v.F, nf, ot, mt, os, ms, T);
    else ceigw_tile_in(v.F, nf, os, ms, ot, mt, T);
    for (int k = 0; k < t; ++k) {
      const int ok = k * CW_T;
      __syncthreads();                                 // (T is loaded, the product before this one has read R and X)
      ceigw_tile_in(v.G, nf, ot, mt, ok, CW_T, R);     // R_tk
      if (LEFT) ceigw_tile_in(v.F, nf, ok, CW_T, os, ms, X);
      else ceigw_tile_in(v.F, nf, os, ms, ok, CW_T, X);
      __syncthreads();
      if (LEFT)
        wg_mma(mt, ms, CW_T, [=](int r, int kk) { return R[r + kk * CW_LD]; }, [=](int kk, int c) { return X[kk + c * CW_LD]; },
               [=](int r, int c, double s) { T[r + c * CW_LD] -= s; });
      else
        wg_mma(ms, mt, CW_T, [=](int r, int kk) { return X[r + kk * CW_LD]; }, [=](int kk, int c) { return R[c + kk * CW_LD]; },
               [=](int r, int c, double s) { T[r + c * CW_LD] -= s; });
    }
    __syncthreads();
    ceigw_tile_in(v.G, nf, ot, mt, ot, mt, R);         // R_tt
    __syncthreads();
    if (LEFT) {
      wg::trsm_llN(mt, ms, R, CW_LD, T, CW_LD);
      ceigw_tile_out(v.F, nf, ot, mt, os, ms, T);
    } else {
      wg::trsm_rlT(ms, mt, R, CW_LD, T, CW_LD);
      ceigw_tile_out(v.F, nf, os, ms, ot, mt, T);
    }
    __threadfence_block();                             // the tile is read back from memory as X by this workgroup
    __syncthreads();
  }
}

// F <- (F + F^T) / 2 on gridDim.x workgroups per clique: the thread of an entry below the diagonal writes it and its mirror
// image (the expression of k_ceig)
__global__ void __launch_bounds__(MRC_NT) k_ceigw_symm(CeigwArgs a) {
  const CeigwDesc w = a.wd[blockIdx.y];
  const CeigwView v = ceigw_view(w, a.ws);
  if (v.state[CW_DONE]) return;
  const int nf = w.nf;
  for (int e = blockIdx.x * MRC_NT + SMCP_TID; e < nf * nf; e += gridDim.x * MRC_NT) {
    const int i = e % nf, j = e / nf;
    if (i > j) {
      const double s = 0.5 * (v.F[i + (int64_t)j * nf] + v.F[j + (int64_t)i * nf]);
      v.F[i + (int64_t)j * nf] = s;
      v.F[j + (int64_t)i * nf] = s;
    }
  }
}

// |F|_F and the stop threshold, the largest |off-diagonal entry| of F into slot 0 (zeros into the others), the status: one
// workgroup per clique; a non-finite |F|_F flags the clique at once.  Pencil mode: CW_NOTPD is kept as the reduction left
// it, and a clique that carries it stays ended (and is not one that did not converge).
__global__ void __launch_bounds__(MRC_NT) k_ceigw_begin(CeigwArgs a) {
  __shared__ double red[MRC_NT];
  const CeigwDesc w = a.wd[blockIdx.x];
  const CeigwView v = ceigw_view(w, a.ws);
  const int nf = w.nf;
  double acc = 0.0, off = 0.0;
  for (int e = SMCP_TID; e < nf * nf; e += MRC_NT) acc += v.F[e] * v.F[e];
  const double fro = sqrt(ceig_reduce(acc, false, red));
  for (int j = 0; j < nf; ++j)
    for (int i = SMCP_TID; i < nf; i += MRC_NT)
      if (i != j) off = ceigw_nanmax(off, fabs(v.F[i + (int64_t)j * nf]));
  off = ceig_reduce(off, true, red);
  for (int s = SMCP_TID; s < w.h * (w.h + 1) / 2; s += MRC_NT) v.slot[s] = s == 0 ? off : 0.0;
  if (SMCP_TID == 0) {
    const int notpd = a.pencil ? v.state[CW_NOTPD] : 0;
    const int bad = !notpd && !(fro < INFINITY);
    v.st[0] = fro;
    v.st[1] = DBL_EPSILON * fro;
    for (int s = 0; s < CW_STATE; ++s) v.state[s] = 0;
    v.state[CW_DONE] = bad | notpd;
    v.state[CW_NOCONV] = bad;
    v.state[CW_NOTPD] = notpd;
  }
}

// The start of a block sweep, one workgroup over all cliques of the group.
__global__ void __launch_bounds__(MRC_NT) k_ceigw_check(CeigwArgs a) {
  __shared__ double red[MRC_NT];
  int run = 0;
  for (int wi = 0; wi < a.nw; ++wi) {
    const CeigwDesc w = a.wd[wi];
    const CeigwView v = ceigw_view(w, a.ws);
    if (v.state[CW_DONE]) continue;                    // (uniform: written by thread 0 of an earlier launch only)
    double off = 0.0;
    for (int s = SMCP_TID; s < w.h * (w.h + 1) / 2; s += MRC_NT) off = ceigw_nanmax(off, v.slot[s]);
    off = ceig_reduce(off, true, red);
    if (SMCP_TID == 0) {
      if (off <= v.st[1]) v.state[CW_DONE] = 1;
      else if (v.state[CW_SWEEPS] == CEIG_MAX_SWEEPS) { v.state[CW_DONE] = 1; v.state[CW_NOCONV] = 1; }
      else { v.state[CW_SWEEPS] += 1; ++run; }
    }
  }
  if (SMCP_TID == 0) *a.nrun = run;
}

// Step r, pair blockIdx.x of clique blockIdx.y: see the head of the file.
__global__ void __launch_bounds__(MRC_NT) k_ceigw_pivot(CeigwArgs a, int r) {
  extern __shared__ double mrc_lds[];
  __shared__ double red[MRC_NT];
  __shared__ double tab[5 * (CW_T / 2)];
  __shared__ int rk[CW_T];
  const CeigwDesc w = a.wd[blockIdx.y];
  const int t = blockIdx.x, nf = w.nf;
  if (t >= w.h || r >= w.nb + (w.nb & 1) - 1) return;
  const CeigwView v = ceigw_view(w, a.ws);
  if (v.state[CW_DONE]) return;
  const CeigwPair P = ceigw_pair(nf, w.nb, r, t);
  const int m = P.n0 + P.n1;
  double* Fp = mrc_lds;
  double* Vp = Fp + m * m;
  for (int e = SMCP_TID; e < m * m; e += MRC_NT) {
    const int i = e % m, j = e / m;
    Fp[e] = v.F[ceigw_row(P, i) + (int64_t)ceigw_row(P, j) * nf];
    Vp[e] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  int noconv;
  const int sweeps = ceig_jacobi<true>(m, Fp, tab, red, &noconv, Vp);
  // the rank sort of k_ceig_vec on the pivot's diagonal: column i of the rotations goes to column rk[i] of U_P
  double* dg = tab;
  for (int i = SMCP_TID; i < m; i += MRC_NT) dg[i] = Fp[i + i * m];
  __syncthreads();
  double moved = 0.0;
  for (int i = SMCP_TID; i < m; i += MRC_NT) {
    const double x = dg[i];
    int rr = 0;
    for (int j = 0; j < m; ++j) rr += (dg[j] < x || (dg[j] == x && j < i)) ? 1 : 0;
    rk[i] = rr;
    v.ev[t * CW_T + rr] = x;
    if (rr != i) moved = 1.0;
  }
  moved = ceig_reduce(moved, false, red);
  double* U = v.U + (int64_t)t * CW_T * CW_T;
  for (int e = SMCP_TID; e < m * m; e += MRC_NT) U[e % m + rk[e / m] * CW_T] = Vp[e];
  if (SMCP_TID == 0) v.uflag[t] = (sweeps == 0 && !noconv && moved == 0.0) ? 1 : 0;
}

// Step r, clique blockIdx.y; blockIdx.x < hmax (hmax + 1) / 2: tile (P, Q), P >= Q, of F; then (row tile, Q) of V.
__global__ void __launch_bounds__(MRC_NT) k_ceigw_apply(CeigwArgs a, int r, int hmax) {
  extern __shared__ double mrc_lds[];
  __shared__ double red[MRC_NT];
  const CeigwDesc w = a.wd[blockIdx.y];
  const int nf = w.nf;
  if (r >= w.nb + (w.nb & 1) - 1) return;
  const CeigwView v = ceigw_view(w, a.ws);
  if (v.state[CW_DONE]) return;
  double* T = mrc_lds;
  double* Ub = T + CW_T * CW_LD;
  double* W = Ub + CW_T * CW_LD;
  const int ntf = hmax * (hmax + 1) / 2;
  int x = blockIdx.x;
  if (x < ntf) {
    int Pi = 0;
    while (x > Pi) { x -= Pi + 1; ++Pi; }
    const int Qi = x;
    if (Pi >= w.h) return;
    double* slot = v.slot + Pi * (Pi + 1) / 2 + Qi;
    const CeigwPair P = ceigw_pair(nf, w.nb, r, Pi), Q = ceigw_pair(nf, w.nb, r, Qi);
    const int mP = P.n0 + P.n1, mQ = Q.n0 + Q.n1;
    if (Pi == Qi) {
      for (int e = SMCP_TID; e < mP * mP; e += MRC_NT) {
        const int i = e % mP, j = e / mP;
        v.F[ceigw_row(P, i) + (int64_t)ceigw_row(P, j) * nf] = i == j ? v.ev[Pi * CW_T + i] : 0.0;
      }
      if (SMCP_TID == 0) *slot = 0.0;
      return;
    }
    double mx = 0.0;
    for (int e = SMCP_TID; e < mP * mQ; e += MRC_NT) {
      const int i = e % mP, j = e / mP;
      T[i + j * CW_LD] = v.F[ceigw_row(P, i) + (int64_t)ceigw_row(Q, j) * nf];
    }
    if (v.uflag[Pi] && v.uflag[Qi]) {                   // nothing rotates this tile: its maximum alone
      __syncthreads();
      for (int e = SMCP_TID; e < mP * mQ; e += MRC_NT) mx = ceigw_nanmax(mx, fabs(T[e % mP + (e / mP) * CW_LD]));
      mx = ceig_reduce(mx, true, red);
      if (SMCP_TID == 0) *slot = mx;
      return;
    }
    const double* UP = v.U + (int64_t)Pi * CW_T * CW_T;
    const double* UQ = v.U + (int64_t)Qi * CW_T * CW_T;
    for (int e = SMCP_TID; e < mP * mP; e += MRC_NT) Ub[e % mP + (e / mP) * CW_LD] = UP[e % mP + (e / mP) * CW_T];
    __syncthreads();
    wg_mma(mP, mQ, mP, [=](int i, int kk) { return Ub[kk + i * CW_LD]; }, [=](int kk, int j) { return T[kk + j * CW_LD]; },
           [=](int i, int j, double c) { W[i + j * CW_LD] = c; });                        // W = U_P^T T
    __syncthreads();
    for (int e = SMCP_TID; e < mQ * mQ; e += MRC_NT) Ub[e % mQ + (e / mQ) * CW_LD] = UQ[e % mQ + (e / mQ) * CW_T];
    __syncthreads();
    double* F = v.F;
    wg_mma(mP, mQ, mQ, [=](int i, int kk) { return W[i + kk * CW_LD]; }, [=](int kk, int j) { return Ub[kk + j * CW_LD]; },
           [=, &mx](int i, int j, double c) {                                              // T = W U_Q, in place and mirrored
             const int gi = ceigw_row(P, i), gj = ceigw_row(Q, j);
             F[gi + (int64_t)gj * nf] = c;
             F[gj + (int64_t)gi * nf] = c;
             mx = ceigw_nanmax(mx, fabs(c));
           });
    mx = ceig_reduce(mx, true, red);
    if (SMCP_TID == 0) *slot = mx;
    return;
  }
  x -= ntf;
  const int Qi = x % hmax, i0 = (x / hmax) * CW_T;
  if (!a.vec || Qi >= w.h || i0 >= nf || v.uflag[Qi]) return;
  const CeigwPair Q = ceigw_pair(nf, w.nb, r, Qi);
  const int mQ = Q.n0 + Q.n1, mr = min(CW_T, nf - i0);
  const double* UQ = v.U + (int64_t)Qi * CW_T * CW_T;
  for (int e = SMCP_TID; e < mr * mQ; e += MRC_NT) {
    const int i = e % mr, j = e / mr;
    T[i + j * CW_LD] = v.V[(i0 + i) + (int64_t)ceigw_row(Q, j) * nf];
  }
  for (int e = SMCP_TID; e < mQ * mQ; e += MRC_NT) Ub[e % mQ + (e / mQ) * CW_LD] = UQ[e % mQ + (e / mQ) * CW_T];
  __syncthreads();
  double* V = v.V;
  wg_mma(mr, mQ, mQ, [=](int i, int kk) { return T[i + kk * CW_LD]; }, [=](int kk, int j) { return Ub[kk + j * CW_LD]; },
         [=](int i, int j, double c) { V[(i0 + i) + (int64_t)ceigw_row(Q, j) * nf] = c; });
}

// The end of a clique, one workgroup each: the rank sort of the diagonal into w (and sw, rk, col for k_ceigw_out), with
// vmode 1 the counts of the eigenvalues outside [lo, hi] and pinfo as k_ceig_vec leaves it; the block sweeps into rank, the
// status into flag.  A clique that did not converge: NaN in w and pinfo.  The cone pass (vmode CW_VMODE_CONE): the number of
// eigenvalues < 0 into the status words, and pinfo, rank and flag are left to k_ceigw_cone_finish.  Pencil mode: a clique
// whose B_gg is not positive definite (CW_NOTPD) gets NaN in w and CEIG_NOT_PD in flag, as k_ceig leaves it.
__global__ void __launch_bounds__(MRC_NT) k_ceigw_sort(CeigwArgs a) {
  __shared__ double red[MRC_NT];
  const CeigwDesc w = a.wd[blockIdx.x];
  const CeigwView v = ceigw_view(w, a.ws);
  const int nf = w.nf, k = w.k;
  const CliqueDesc d = a.m.cl[k];
  double* wout = a.m.w + d.rows;
  const int noconv = v.state[CW_NOCONV], notpd = a.pencil ? v.state[CW_NOTPD] : 0;
  if (!noconv && !notpd) {
    double* dg = v.ev;
    for (int i = SMCP_TID; i < nf; i += MRC_NT) dg[i] = v.F[i + (int64_t)i * nf];
    __syncthreads();
    for (int i = SMCP_TID; i < nf; i += MRC_NT) {
      const double x = dg[i];
      int rr = 0;
      for (int j = 0; j < nf; ++j) rr += (dg[j] < x || (dg[j] == x && j < i)) ? 1 : 0;
      wout[rr] = x;
      v.sw[rr] = x;
      v.rk[i] = rr;
      v.col[rr] = i;
    }
    __syncthreads();
    if (a.m.vmode == CW_VMODE_CONE) {
      double cn = 0.0;
      for (int rr = SMCP_TID; rr < nf; rr += MRC_NT) cn += v.sw[rr] < 0.0 ? 1.0 : 0.0;
      const int nneg = (int)ceig_reduce(cn, false, red);
      if (SMCP_TID == 0) v.state[CW_NNEG] = nneg;
    } else if (a.vec && a.m.vmode) {
      const double lo = a.m.lo, hi = a.m.hi;
      double cl = 0.0, ch = 0.0, sq = 0.0;
      for (int rr = SMCP_TID; rr < nf; rr += MRC_NT) {
        const double x = v.sw[rr];
        if (x < lo) { cl += 1.0; sq += (lo - x) * (lo - x); }
        else if (x > hi) { ch += 1.0; sq += (hi - x) * (hi - x); }
      }
      const int nlo = (int)ceig_reduce(cl, false, red), nhi = (int)ceig_reduce(ch, false, red);
      sq = ceig_reduce(sq, false, red);
      if (SMCP_TID == 0) {
        v.state[CW_NLO] = nlo;
        v.state[CW_NHI] = nhi;
        a.m.pinfo[2 * k] = (double)(nlo + nhi);
        a.m.pinfo[2 * k + 1] = sq;
      }
    }
  } else {
    for (int i = SMCP_TID; i < nf; i += MRC_NT) wout[i] = NAN;
    if (a.vec && a.m.vmode == 1 && SMCP_TID == 0) a.m.pinfo[2 * k] = a.m.pinfo[2 * k + 1] = NAN;
  }
  if (SMCP_TID == 0 && a.m.vmode != CW_VMODE_CONE) {     // (the cone pass: k_ceigw_cone_finish)
    a.m.rank[k] = v.state[CW_SWEEPS];
    a.m.flag[k] = notpd ? CEIG_NOT_PD : noconv ? CEIG_NO_CONV : 0;
  }
}

// Block k of Q on gridDim.x workgroups per clique: the columns of V by rank (vmode 0), or A_gg formed again plus the
// corrections of the eigenvalues outside [lo, hi], ascending, per entry of the lower triangle, mirrored on store (vmode 1:
// the expression of k_ceig_vec).  NaN for a clique that did not converge.
__global__ void __launch_bounds__(MRC_NT) k_ceigw_out(CeigwArgs a) {
  const CeigwDesc w = a.wd[blockIdx.y];
  const CeigwView v = ceigw_view(w, a.ws);
  const int nf = w.nf, k = w.k;
  const CliqueDesc d = a.m.cl[k];
  double* Zk = a.m.Q + a.m.qptr[k];
  const int first = blockIdx.x * MRC_NT + SMCP_TID, stride = gridDim.x * MRC_NT;
  if (v.state[CW_NOCONV]) {
    for (int t = first; t < nf * nf; t += stride) Zk[t] = NAN;
    return;
  }
  if (a.m.vmode == 0) {
    for (int t = first; t < nf * nf; t += stride) Zk[t % nf + (int64_t)v.rk[t / nf] * nf] = v.V[t];
    return;
  }
  const double* P = a.m.x + d.blk;
  const double* S = a.m.upd + d.upd;
  const double lo = a.m.lo, hi = a.m.hi;
  const int nlo = v.state[CW_NLO], nhi = v.state[CW_NHI];
  for (int t = first; t < nf * nf; t += stride) {
    const int i = t % nf, j = t / nf;
    if (i >= j) {
      double z = cone_x(d, P, S, i, j);
      for (int rr = 0; rr < nlo; ++rr) {
        const double* q = v.V + (int64_t)v.col[rr] * nf;
        z += (lo - v.sw[rr]) * (q[i] * q[j]);
      }
      for (int rr = nf - nhi; rr < nf; ++rr) {
        const double* q = v.V + (int64_t)v.col[rr] * nf;
        z += (hi - v.sw[rr]) * (q[i] * q[j]);
      }
      Zk[i + (int64_t)j * nf] = z;
      Zk[j + (int64_t)i * nf] = z;
    }
  }
}

// ---- the clique step of csp_cone_project_steps on the wide cliques (k_cone_split of front_ceig.hip, its Jacobi replaced) ----
// MrcArgs as k_cone_split reads them (Q = U, pw = W, lo = relax, pinfo), vmode = CW_VMODE_CONE, w = a buffer of the context.
// The chain of an iteration is fixed: k_ceigw_cone_form, k_ceigw_begin, CEIG_MAX_SWEEPS times
// (k_ceigw_check, the steps of a block sweep), one more k_ceigw_check, k_ceigw_sort, k_ceigw_cone_split, k_ceigw_cone_finish.
// Nothing looks at the host: the launches behind the check that ended a clique return at their top.

// workgroups of k_ceigw_cone_form / _split that share a clique of order nf, and so the partial sums of its r_k^2: a function
// of nf alone, whatever else the launch group holds
__host__ __device__ inline int ceigw_parts(int64_t nf) { return (int)(nf * nf / (MRC_NT * 32) < 1 ? 1 : nf * nf / (MRC_NT * 32) > 64 ? 64 : nf * nf / (MRC_NT * 32)); }

// F = T_k in full (cone_form on the clique's workgroups), V = I
__global__ void __launch_bounds__(MRC_NT) k_ceigw_cone_form(CeigwArgs a) {
  const CeigwDesc w = a.wd[blockIdx.y];
  const int np = ceigw_parts(w.nf);
  if ((int)blockIdx.x >= np) return;
  const CeigwView v = ceigw_view(w, a.ws);
  const CliqueDesc d = a.m.cl[w.k];
  const int64_t q = a.m.qptr[w.k];
  cone_form(d, a.m.x + d.blk, a.m.upd + d.upd, a.m.Q + q, a.m.pw + q, a.m.lo, v.F, blockIdx.x, np);
  for (int e = blockIdx.x * MRC_NT + SMCP_TID; e < w.nf * w.nf; e += np * MRC_NT) v.V[e] = (e % (w.nf + 1) == 0) ? 1.0 : 0.0;
}

// The part of k_cone_split behind its Jacobi.  Every entry i >= j of the lower triangle is one thread's: T_k formed again
// (the bits of the form step: x, U_k and W_k are as they were), u = the sum over the nneg negative eigenvalues, ascending,
// with the columns of V taken by rank, then U_k and W_k stored mirrored.  A thread reads U_k and W_k in its own lower-triangle
// entries only and is the only writer of those and of their mirror images, which nobody reads: no hazard between the
// workgroups of a launch.  Workgroup p leaves its share of r_k^2 in word p of the clique's U region, which the sweeps are
// done with.  A clique that did not converge: NaN in U_k and W_k.
__global__ void __launch_bounds__(MRC_NT) k_ceigw_cone_split(CeigwArgs a) {
  __shared__ double red[MRC_NT];
  const CeigwDesc w = a.wd[blockIdx.y];
  const int nf = w.nf, k = w.k, np = ceigw_parts(nf);
  if ((int)blockIdx.x >= np) return;
  const CeigwView v = ceigw_view(w, a.ws);
  const CliqueDesc d = a.m.cl[k];
  double* Uk = a.m.Q + a.m.qptr[k];
  double* Wk = a.m.pw + a.m.qptr[k];
  const int first = blockIdx.x * MRC_NT + SMCP_TID, stride = np * MRC_NT;
  if (v.state[CW_NOCONV]) {
    for (int t = first; t < nf * nf; t += stride) Uk[t] = Wk[t] = NAN;
    return;
  }
  const double* P = a.m.x + d.blk;
  const double* S = a.m.upd + d.upd;
  const double relax = a.m.lo;
  const int nneg = v.state[CW_NNEG];
  double rs = 0.0;
  for (int t = first; t < nf * nf; t += stride) {
    const int i = t % nf, j = t / nf;
    if (i >= j) {
      double u = 0.0;
      for (int rr = 0; rr < nneg; ++rr) {
        const double* q = v.V + (int64_t)v.col[rr] * nf;
        u += v.sw[rr] * (q[i] * q[j]);
      }
      const double tk = cone_t(d, P, S, Uk, Wk, relax, i, j, t), wk = tk - 2.0 * u;
      const double dz = cone_x(d, P, S, i, j) - (tk - u);
      rs += i == j ? dz * dz : 2.0 * (dz * dz);
      Uk[t] = u;
      Uk[j + (int64_t)i * nf] = u;
      Wk[t] = wk;
      Wk[j + (int64_t)i * nf] = wk;
    }
  }
  rs = ceig_reduce(rs, false, red);
  if (SMCP_TID == 0) v.U[blockIdx.x] = rs;
}

// One workgroup per clique: pinfo as k_cone_split leaves it (the partial sums of r_k^2 added in index order), the block
// sweeps into rank, the status into flag; NaN in pinfo for a clique that did not converge.
__global__ void __launch_bounds__(MRC_NT) k_ceigw_cone_finish(CeigwArgs a) {
  if (SMCP_TID != 0) return;
  const CeigwDesc w = a.wd[blockIdx.x];
  const CeigwView v = ceigw_view(w, a.ws);
  const int k = w.k, noconv = v.state[CW_NOCONV];
  if (!noconv) {
    double rs = 0.0;
    for (int p = 0; p < ceigw_parts(w.nf); ++p) rs += v.U[p];
    a.m.pinfo[2 * k] = (double)v.state[CW_NNEG];
    a.m.pinfo[2 * k + 1] = rs;
  } else {
    a.m.pinfo[2 * k] = a.m.pinfo[2 * k + 1] = NAN;
  }
  a.m.rank[k] = v.state[CW_SWEEPS];
  a.m.flag[k] = noconv ? CEIG_NO_CONV : 0;
}

}  // namespace smcp
