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
constexpr int CW_VMODE_CONE = 2;                      // MrcArgs::vmode of the cone pass (k_ceigw_cone_*)
constexpr size_t CW_APPLY_LDS = (size_t)3 * CW_T * CW_LD * sizeof(double);
constexpr size_t CW_PIVOT_LDS = (size_t)2 * CW_T * CW_T * sizeof(double);

// One wide clique of a call: offsets in doubles into the workspace.  h: pairs of a step.  V: -1 without eigenvectors.
struct CeigwDesc {
  int32_t k, nf, nb, h;
  int64_t F, V, U, ev, slot, sw, st, ints;
};
// doubles of the workspace of one clique and its layout from `base` on
__host__ inline int64_t ceigw_layout(CeigwDesc& w, int32_t k, int64_t nf, bool vec, int64_t base) {
  w.k = k;
  w.nf = (int32_t)nf;
  w.nb = (int32_t)((nf + CW_B - 1) / CW_B);
  w.h = (w.nb + 1) / 2;
  int64_t o = base;
  w.F = o; o += nf * nf;
  w.V = vec ? o : -1; o += vec ? nf * nf : 0;
  w.U = o; o += (int64_t)w.h * CW_T * CW_T;
  w.ev = o; o += (int64_t)w.h * CW_T;                  // (>= nf doubles: k_ceigw_sort keeps the diagonal here)
  w.slot = o; o += (int64_t)w.h * (w.h + 1) / 2;
  w.sw = o; o += nf;
  w.st = o; o += 2;
  w.ints = o; o += (2 * nf + w.h + CW_STATE + 1) / 2;
  return (o - base + 31) / 32 * 32;
}

struct CeigwView {
  double *F, *V, *U, *ev, *slot, *sw, *st;
  int32_t *rk, *col, *uflag, *state;
};
__device__ inline CeigwView ceigw_view(const CeigwDesc& w, double* ws) {
  CeigwView v;
  v.F = ws + w.F; v.V = w.V >= 0 ? ws + w.V : nullptr; v.U = ws + w.U; v.ev = ws + w.ev; v.slot = ws + w.slot;
  v.sw = ws + w.sw; v.st = ws + w.st;
  v.rk = (int32_t*)(ws + w.ints); v.col = v.rk + w.nf; v.uflag = v.col + w.nf; v.state = v.uflag + w.h;
  return v;
}

// MrcArgs m as k_ceig_vec reads them (standard form); wd / nw: the wide cliques of this launch group, ws: their workspace,
// vec: eigenvectors are accumulated; nrun: the cliques still running (k_ceigw_check)
struct CeigwArgs {
  MrcArgs m;
  const CeigwDesc* wd;
  double* ws;
  int nw, vec;
  int32_t* nrun;
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

// F = A_gg in full (ceig_form on gridDim.x workgroups per clique), V = I
__global__ void __launch_bounds__(MRC_NT) k_ceigw_form(CeigwArgs a) {
  const CeigwDesc w = a.wd[blockIdx.y];
  const CeigwView v = ceigw_view(w, a.ws);
  const CliqueDesc d = a.m.cl[w.k];
  ceig_form(d, a.m.x + d.blk, a.m.upd + d.upd, v.F, blockIdx.x, gridDim.x);
  if (a.vec)
    for (int e = blockIdx.x * MRC_NT + SMCP_TID; e < w.nf * w.nf; e += gridDim.x * MRC_NT) v.V[e] = (e % (w.nf + 1) == 0) ? 1.0 : 0.0;
}

// |F|_F and the stop threshold, the largest |off-diagonal entry| of F into slot 0 (zeros into the others), the status: one
// workgroup per clique; a non-finite |F|_F flags the clique at once
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
    const int bad = !(fro < INFINITY);
    v.st[0] = fro;
    v.st[1] = DBL_EPSILON * fro;
    for (int s = 0; s < CW_STATE; ++s) v.state[s] = 0;
    v.state[CW_DONE] = bad;
    v.state[CW_NOCONV] = bad;
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
// eigenvalues < 0 into the status words, and pinfo, rank and flag are left to k_ceigw_cone_finish.
__global__ void __launch_bounds__(MRC_NT) k_ceigw_sort(CeigwArgs a) {
  __shared__ double red[MRC_NT];
  const CeigwDesc w = a.wd[blockIdx.x];
  const CeigwView v = ceigw_view(w, a.ws);
  const int nf = w.nf, k = w.k;
  const CliqueDesc d = a.m.cl[k];
  double* wout = a.m.w + d.rows;
  const int noconv = v.state[CW_NOCONV];
  if (!noconv) {
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
    a.m.flag[k] = noconv ? CEIG_NO_CONV : 0;
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
