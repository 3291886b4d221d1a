// Spectra of the clique blocks (csp_clique_eigvalsh): for every clique g the eigenvalues of A_gg, or of the pencil
// (A_gg, B_gg) with B_gg positive definite.  X lies in the interior of the cone C_V of PSD-completable matrices exactly
// when every X_gg is positive definite (Grone et al.), so membership in C_V, the distance to its boundary and the step to
// its boundary along a direction are minima over these independent small dense eigenproblems.
//
// k_ceig: one workgroup per clique (workgroups loop over the cliques of a launch when there are more of them than slots),
// operands in one slot -- LDS when it fits, HBM otherwise -- as k_mrc_rank (front_mrc.hip):
//   1. F = A_gg in full: own columns from the panel, the separator block from the top-down gather, lower triangle mirrored;
//   2. pencil form: G = B_gg the same way, G = R R^T in place (a non-positive pivot flags the clique), then
//      F <- R^-1 F R^-T by two triangular solves in the slot and F <- (F + F^T) / 2;
//   3. two-sided cyclic Jacobi on F in the round-robin tournament order: nf - 1 steps of nf / 2 disjoint pairs for even nf,
//      nf steps with one bye for odd nf.  A step: every pair's rotation from the current (a_pp, a_qq, a_pq) by Rutishauser's
//      formulas; barrier; rows; barrier; columns.  A pair with |a_pq| <= eps |F|_F / nf is skipped; the sweeps end at the
//      start of the first one with max |off-diagonal| <= eps |F|_F, or after CEIG_MAX_SWEEPS with the clique flagged;
//   4. a rank sort of the diagonal (ties by index) into w[rowptr[k] .. rowptr[k + 1]), ascending.
// No eigenvectors are accumulated.  Every entry of a step is one expression of entries of the step before and every
// reduction is a fixed tree: the same input gives the same bits.
// k_ceig_reduce: the smallest and largest eigenvalue over all cliques with the lowest clique attaining each, and the status.
//
// With eigenvectors (csp_clique_eigh, csp_clique_project): k_ceig_vec, the standard form of k_ceig in the slot of the pencil
// form with V where that keeps G.  V starts as I; every Jacobi step rotates columns p, q of V by the step's (s, tau) tables in
// one more pass shaped as the column pass on F (ceig_jacobi<true>: the arithmetic on F is that of k_ceig, so are the bits of
// w).  The rank sort of the diagonal sends column i of V to column rank(i) of block k of Q (vmode 0).  vmode 1, the
// projection of the block on {lo I <= Z <= hi I}: the sorted spectrum stays in the slot, A_gg is formed again over F, and
// Z = A_gg + sum over the eigenvalues outside [lo, hi], ascending, of (clip(w_j) - w_j) q_j q_j^T, one thread per entry of the
// lower triangle, mirrored on store: a block whose spectrum lies inside [lo, hi] comes back as the bits of A_gg, and the work
// grows with the number of eigenvalues clipped.
// k_clique_gather / k_clique_scatter: the packed clique blocks (block k: nf x nf, column-major, at qptr[k]) from a blkval
// with its separator blocks gathered, and back: x = P_V(sum_k E_k Z_k E_k^T), one launch per level, leaves first, a clique's
// panel and update block from the lower triangle of Z_k, then its children's update blocks by add_children (front_generic.hip).
//
// The projection onto the cone itself (csp_cone_project_steps): k_cone_split, the clique step of a
// clique-splitting ADMM on top of ceig_jacobi<true>, k_cone_update, the step on the pattern, and k_cone_resid, the row of
// residuals of an iteration; k_cone_mult makes the multiplicities once per context.  See above each of them.  Under
// CSP_TUNE_CEIG_WIDE the wide cliques leave k_cone_split for the block Jacobi of front_ceigw.hip (k_ceigw_cone_*), which
// forms T_k by the cone_t below and fills pinfo, rank and flag as k_cone_split does: k_cone_resid sees no difference.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "context.hpp"
#include "wgblas.hpp"

namespace smcp {

constexpr int CEIG_MAX_SWEEPS = 30;
constexpr int CEIG_NOT_PD = 1, CEIG_NO_CONV = 2;     // per-clique flag
constexpr int CEIG_TAB_H = 320;                      // pairs per step whose tables fit the static LDS of k_ceig (orders to 640)

// doubles of one slot: standard form (F, five tables of the pairs of a step) and pencil form (G as well)
__host__ __device__ inline int64_t ceig_slot1(int64_t nf) { return nf * nf + 3 * nf + 3; }
__host__ __device__ inline int64_t ceig_slot2(int64_t nf) { return 2 * nf * nf + 3 * nf + 3; }

// sum (is_max false) or NaN-propagating maximum of v over the workgroup, in a fixed tree; the result reaches every thread
__device__ inline double ceig_reduce(double v, bool is_max, double* red) {
  red[SMCP_TID] = v;
  __syncthreads();
  for (int s = MRC_NT / 2; s > 0; s >>= 1) {
    if (SMCP_TID < s) {
      const double x = red[SMCP_TID], y = red[SMCP_TID + s];
      red[SMCP_TID] = is_max ? ((y > x || y != y) ? y : x) : x + y;
    }
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// pair t of step r of the round-robin tournament on m players (m even): (p, q) with p < q; player m - 1 stays in place
__device__ inline void ceig_pair(int m, int r, int t, int& p, int& q) {
  int x, y;
  if (t == 0) { x = m - 1; y = r; }
  else { x = (r + t) % (m - 1); y = (r - t + m - 1) % (m - 1); }
  p = x < y ? x : y;
  q = x < y ? y : x;
}

// The cyclic Jacobi of the symmetric nf x nf matrix F (full storage, column-major, overwritten; its diagonal ends as the
// eigenvalues).  tab: 5 * ((nf + 1) / 2) doubles.  Returns the sweeps taken; *noconv = 1 when F holds a non-finite entry or
// CEIG_MAX_SWEEPS did not reach the stopping rule.
// VEC: V (nf x nf, the identity on entry) <- V J for every rotation J: its columns end as the eigenvectors, column i for F_ii.
template <bool VEC = false>
__device__ inline int ceig_jacobi(int nf, double* F, double* tab, double* red, int* noconv, double* V = nullptr) {
  const int m = nf + (nf & 1), h = m / 2, steps = m - 1;
  double* tc = tab;            // per pair of the step: s (0: skipped), tau = s / (1 + c), the new a_pp, the new a_qq, (p, q)
  double* tt = tab + h;
  double* tp = tab + 2 * h;
  double* tq = tab + 3 * h;
  int* pq = (int*)(tab + 4 * h);
  double acc = 0.0;
  for (int e = SMCP_TID; e < nf * nf; e += MRC_NT) acc += F[e] * F[e];
  const double fro = sqrt(ceig_reduce(acc, false, red));
  *noconv = 0;
  if (!(fro < INFINITY)) { *noconv = 1; return 0; }
  const double stop = DBL_EPSILON * fro, skip = stop / nf;
  // Item e of a pass is (pair e % h, column e / h) for the rows and (row e % nf, pair e / nf) for the columns; a thread
  // walks e = tid, tid + MRC_NT, ... and keeps both coordinates by addition: a division per item costs more than the item.
  const int rt0 = SMCP_TID % h, rj0 = SMCP_TID / h, rdt = MRC_NT % h, rdj = MRC_NT / h;
  const int ci0 = SMCP_TID % nf, ct0 = SMCP_TID / nf, cdi = MRC_NT % nf, cdt = MRC_NT / nf;
  int sweeps = 0;
  for (;; ++sweeps) {
    double off = 0.0;
    for (int j = 0; j < nf; ++j)
      for (int i = SMCP_TID; i < nf; i += MRC_NT) {
        const double v = fabs(F[i + (int64_t)j * nf]);
        if (i != j && (v > off || v != v)) off = v;
      }
    off = ceig_reduce(off, true, red);
    if (off <= stop) break;
    if (sweeps == CEIG_MAX_SWEEPS) { *noconv = 1; break; }
    for (int r = 0; r < steps; ++r) {
      for (int t = SMCP_TID; t < h; t += MRC_NT) {
        int p, q;
        ceig_pair(m, r, t, p, q);
        double s = 0.0, tau = 0.0, npp = 0.0, nqq = 0.0;
        if (q < nf) {
          const double app = F[p + (int64_t)p * nf], aqq = F[q + (int64_t)q * nf], apq = F[q + (int64_t)p * nf];
          if (fabs(apq) > skip) {
            const double theta = 0.5 * (aqq - app) / apq;
            double tn = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
            if (theta < 0.0) tn = -tn;
            const double c = 1.0 / sqrt(tn * tn + 1.0);
            s = tn * c;
            tau = s / (1.0 + c);
            npp = app - tn * apq;
            nqq = aqq + tn * apq;
          }
        }
        tc[t] = s; tt[t] = tau; tp[t] = npp; tq[t] = nqq;
        pq[2 * t] = p; pq[2 * t + 1] = q;
      }
      __syncthreads();
      for (int t = rt0, j = rj0; j < nf;) {                       // rows p, q of every pair: F <- J^T F
        const double s = tc[t];
        if (s != 0.0) {
          const double tau = tt[t];
          double* Fp = F + pq[2 * t] + (int64_t)j * nf;
          double* Fq = F + pq[2 * t + 1] + (int64_t)j * nf;
          const double g = *Fp, hh = *Fq;
          *Fp = g - s * (hh + g * tau);
          *Fq = hh + s * (g - hh * tau);
        }
        t += rdt; j += rdj;
        if (t >= h) { t -= h; ++j; }
      }
      __syncthreads();
      for (int i = ci0, t = ct0; t < h;) {                        // columns p, q: F <- F J, the 2 x 2 block set exactly
        const double s = tc[t];
        if (s != 0.0) {
          const int p = pq[2 * t], q = pq[2 * t + 1];
          const double tau = tt[t];
          double* Fp = F + i + (int64_t)p * nf;
          double* Fq = F + i + (int64_t)q * nf;
          const double g = *Fp, hh = *Fq;
          double vp = g - s * (hh + g * tau), vq = hh + s * (g - hh * tau);
          if (i == p) { vp = tp[t]; vq = 0.0; }
          if (i == q) { vp = 0.0; vq = tq[t]; }
          *Fp = vp;
          *Fq = vq;
        }
        i += cdi; t += cdt;
        if (i >= nf) { i -= nf; ++t; }
      }
      if constexpr (VEC) {
        for (int i = ci0, t = ct0; t < h;) {                      // columns p, q of V: V <- V J (nothing of F is read or written)
          const double s = tc[t];
          if (s != 0.0) {
            const double tau = tt[t];
            double* Vp = V + i + (int64_t)pq[2 * t] * nf;
            double* Vq = V + i + (int64_t)pq[2 * t + 1] * nf;
            const double g = *Vp, hh = *Vq;
            *Vp = g - s * (hh + g * tau);
            *Vq = hh + s * (g - hh * tau);
          }
          i += cdi; t += cdt;
          if (i >= nf) { i -= nf; ++t; }
        }
      }
      __syncthreads();
    }
  }
  return sweeps;
}

// the full symmetric block of clique d of the matrix with panel P (nf x nn) and gathered separator block U (na x na);
// workgroup `part` of `nparts` that share the block
__device__ inline void ceig_form(const CliqueDesc& d, const double* P, const double* U, double* F, int part = 0, int nparts = 1) {
  const int nn = d.nn, na = d.na, nf = nn + na;
  for (int e = part * MRC_NT + SMCP_TID; e < nf * nf; e += nparts * MRC_NT) {
    const int i = e % nf, j = e / nf;
    if (i >= j) {
      const double v = j < nn ? P[i + (int64_t)j * nf] : U[(i - nn) + (int64_t)(j - nn) * na];
      F[i + (int64_t)j * nf] = v;
      F[j + (int64_t)i * nf] = v;
    }
  }
  __syncthreads();
}

// MrcArgs: x / upd = A and its gathered separator blocks, x2 / upd2 = B and its (x2 null: standard form), w = the
// eigenvalues, rank = sweeps per clique, flag = CEIG_NOT_PD / CEIG_NO_CONV per clique
__global__ void __launch_bounds__(MRC_NT) k_ceig(MrcArgs a) {
  extern __shared__ double mrc_lds[];
  __shared__ double red[MRC_NT];
  // the tables of the pairs of a step: every entry update begins by reading them, so from an HBM slot they would put two
  // more dependent round trips to memory in front of each one; wider cliques than these 12.5 KiB serve keep them in the slot
  __shared__ double stab[5 * CEIG_TAB_H];
  double* ws = a.ws ? a.ws + (int64_t)blockIdx.x * a.slot : mrc_lds;
  for (int e = blockIdx.x; e < a.cnt; e += gridDim.x) {
    const int k = a.lev[e];
    const CliqueDesc d = a.cl[k];
    const int nf = d.nn + d.na;
    double* F = ws;
    double* G = F + (int64_t)nf * nf;
    double* tab = a.x2 ? G + (int64_t)nf * nf : G;
    double* w = a.w + d.rows;
    ceig_form(d, a.x + d.blk, a.upd + d.upd, F);
    int flag = 0, sweeps = 0;
    if (a.x2) {
      ceig_form(d, a.x2 + d.blk, a.upd2 + d.upd, G);
      if (wg::potrf(nf, G, nf)) flag = CEIG_NOT_PD;
      __syncthreads();
      if (!flag) {
        wg::trsm_llN(nf, nf, G, nf, F, nf);
        wg::trsm_rlT(nf, nf, G, nf, F, nf);
        for (int t = SMCP_TID; t < nf * nf; t += MRC_NT) {
          const int i = t % nf, j = t / nf;
          if (i > j) {
            const double v = 0.5 * (F[i + (int64_t)j * nf] + F[j + (int64_t)i * nf]);
            F[i + (int64_t)j * nf] = v;
            F[j + (int64_t)i * nf] = v;
          }
        }
        __syncthreads();
      }
    }
    if (!flag) {
      int noconv;
      sweeps = ceig_jacobi(nf, F, (nf + 1) / 2 <= CEIG_TAB_H ? stab : tab, red, &noconv);
      if (noconv) flag = CEIG_NO_CONV;
      for (int i = SMCP_TID; i < nf; i += MRC_NT) tab[i] = F[i + (int64_t)i * nf];
      __syncthreads();
      for (int i = SMCP_TID; i < nf; i += MRC_NT) {
        const double v = tab[i];
        int rk = 0;
        for (int j = 0; j < nf; ++j) rk += (tab[j] < v || (tab[j] == v && j < i)) ? 1 : 0;
        w[rk] = v;
      }
    } else {
      for (int i = SMCP_TID; i < nf; i += MRC_NT) w[i] = NAN;
    }
    if (SMCP_TID == 0) {
      a.rank[k] = sweeps;
      a.flag[k] = flag;
    }
    __syncthreads();
  }
}

// MrcArgs: as k_ceig in standard form; Q, qptr, lo, hi, pinfo, vmode: see there.  A clique that did not converge leaves NaN
// in its w, its block of Q and (vmode 1) its two entries of pinfo.
__global__ void __launch_bounds__(MRC_NT) k_ceig_vec(MrcArgs a) {
  extern __shared__ double mrc_lds[];
  __shared__ double red[MRC_NT];
  __shared__ double stab[5 * CEIG_TAB_H];      // as in k_ceig
  double* ws = a.ws ? a.ws + (int64_t)blockIdx.x * a.slot : mrc_lds;
  for (int e = blockIdx.x; e < a.cnt; e += gridDim.x) {
    const int k = a.lev[e];
    const CliqueDesc d = a.cl[k];
    const int nf = d.nn + d.na;
    double* F = ws;
    double* V = F + (int64_t)nf * nf;
    double* tab = V + (int64_t)nf * nf;
    double* dg = tab;                          // the diagonal; behind it the rank of every column and the column of every
    int* rk = (int*)(tab + nf);                // rank (2 nf ints), then the sorted spectrum
    int* col = rk + nf;
    double* sw = tab + 2 * nf;
    double* w = a.w + d.rows;
    double* Zk = a.Q + a.qptr[k];
    ceig_form(d, a.x + d.blk, a.upd + d.upd, F);
    for (int t = SMCP_TID; t < nf * nf; t += MRC_NT) V[t] = (t % (nf + 1) == 0) ? 1.0 : 0.0;
    __syncthreads();
    int noconv;
    const int sweeps = ceig_jacobi<true>(nf, F, (nf + 1) / 2 <= CEIG_TAB_H ? stab : tab, red, &noconv, V);
    if (!noconv) {
      for (int i = SMCP_TID; i < nf; i += MRC_NT) dg[i] = F[i + (int64_t)i * nf];
      __syncthreads();
      for (int i = SMCP_TID; i < nf; i += MRC_NT) {
        const double v = dg[i];
        int r = 0;
        for (int j = 0; j < nf; ++j) r += (dg[j] < v || (dg[j] == v && j < i)) ? 1 : 0;
        w[r] = v;
        sw[r] = v;
        rk[i] = r;
        col[r] = i;
      }
      __syncthreads();
      if (a.vmode == 0) {
        for (int t = SMCP_TID; t < nf * nf; t += MRC_NT) Zk[t % nf + (int64_t)rk[t / nf] * nf] = V[t];
      } else {
        ceig_form(d, a.x + d.blk, a.upd + d.upd, F);
        const double lo = a.lo, hi = a.hi;
        double cl = 0.0, ch = 0.0, sq = 0.0;
        for (int r = SMCP_TID; r < nf; r += MRC_NT) {
          const double v = sw[r];
          if (v < lo) { cl += 1.0; sq += (lo - v) * (lo - v); }
          else if (v > hi) { ch += 1.0; sq += (hi - v) * (hi - v); }
        }
        const int nlo = (int)ceig_reduce(cl, false, red), nhi = (int)ceig_reduce(ch, false, red);
        sq = ceig_reduce(sq, false, red);
        for (int t = SMCP_TID; t < nf * nf; t += MRC_NT) {
          const int i = t % nf, j = t / nf;
          if (i >= j) {
            double z = F[t];
            for (int r = 0; r < nlo; ++r) {
              const double* q = V + (int64_t)col[r] * nf;
              z += (lo - sw[r]) * (q[i] * q[j]);
            }
            for (int r = nf - nhi; r < nf; ++r) {
              const double* q = V + (int64_t)col[r] * nf;
              z += (hi - sw[r]) * (q[i] * q[j]);
            }
            Zk[i + (int64_t)j * nf] = z;
            Zk[j + (int64_t)i * nf] = z;
          }
        }
        if (SMCP_TID == 0) {
          a.pinfo[2 * k] = (double)(nlo + nhi);
          a.pinfo[2 * k + 1] = sq;
        }
      }
    } else {
      for (int i = SMCP_TID; i < nf; i += MRC_NT) w[i] = NAN;
      for (int t = SMCP_TID; t < nf * nf; t += MRC_NT) Zk[t] = NAN;
      if (a.vmode && SMCP_TID == 0) a.pinfo[2 * k] = a.pinfo[2 * k + 1] = NAN;
    }
    if (SMCP_TID == 0) {
      a.rank[k] = sweeps;
      a.flag[k] = noconv ? CEIG_NO_CONV : 0;
    }
    __syncthreads();
  }
}

// ---- clique-splitting ADMM for the projection onto the cone of PSD-completable matrices (csp_cone_project_steps) --------
// The clique step (k_cone_split), per clique k with the packed blocks U_k (the scaled dual, negative semidefinite) and
// W_k = Z_k - U_k of the iteration before:
//   T_k = Z'_k + relax (X_gg - Z'_k) + U_k,  Z'_k = W_k + U_k;   U_k <- P_-(T_k),  Z_k = T_k - U_k,  W_k <- T_k - 2 U_k.
// The entry (i >= j) of T_k: x from the panel or the gathered separator block (the indexing of ceig_form), u and w from the
// lower triangles of the blocks; the fused multiply-add is spelled out so that both formations of T_k give the same bits.
__device__ inline double cone_x(const CliqueDesc& d, const double* P, const double* S, int i, int j) {
  return j < d.nn ? P[i + (int64_t)j * (d.nn + d.na)] : S[(i - d.nn) + (int64_t)(j - d.nn) * d.na];
}
// the entry (i >= j, at e = i + j nf) of T_k
__device__ inline double cone_t(const CliqueDesc& d, const double* P, const double* S, const double* Uk, const double* Wk,
                                double relax, int i, int j, int e) {
  const double u = Uk[e], z = Wk[e] + u;
  return fma(relax, cone_x(d, P, S, i, j) - z, z) + u;
}
// workgroup `part` of `nparts` that share the block, as in ceig_form
__device__ inline void cone_form(const CliqueDesc& d, const double* P, const double* S, const double* Uk, const double* Wk,
                                 double relax, double* F, int part = 0, int nparts = 1) {
  const int nf = d.nn + d.na;
  for (int e = part * MRC_NT + SMCP_TID; e < nf * nf; e += nparts * MRC_NT) {
    const int i = e % nf, j = e / nf;
    if (i >= j) {
      const double v = cone_t(d, P, S, Uk, Wk, relax, i, j, e);
      F[e] = v;
      F[j + (int64_t)i * nf] = v;
    }
  }
  __syncthreads();
}

// MrcArgs: x / upd = X and its gathered separator blocks, Q = U and pw = W (packed clique blocks at qptr[k], both
// rewritten in place), lo = relax, pinfo + 2 k = the number of negative eigenvalues of T_k and r_k^2 = |X_gg - Z_k|_F^2,
// rank = sweeps, flag = CEIG_NO_CONV per clique.  The slot and the Jacobi are those of k_ceig_vec; then T_k is formed again
// over F (the last reads of the old U_k and W_k, a barrier behind them) and every entry of the lower triangle is one
// thread's sum over the negative eigenvalues, ascending, mirrored on store: a block without a negative eigenvalue leaves
// U_k exactly 0 and W_k the bits of T_k.  A clique that did not converge leaves NaN in U_k, W_k and its two entries of pinfo.
__global__ void __launch_bounds__(MRC_NT) k_cone_split(MrcArgs a) {
  extern __shared__ double mrc_lds[];
  __shared__ double red[MRC_NT];
  __shared__ double stab[5 * CEIG_TAB_H];      // as in k_ceig
  double* ws = a.ws ? a.ws + (int64_t)blockIdx.x * a.slot : mrc_lds;
  for (int e = blockIdx.x; e < a.cnt; e += gridDim.x) {
    const int k = a.lev[e];
    const CliqueDesc d = a.cl[k];
    const int nf = d.nn + d.na;
    double* F = ws;
    double* V = F + (int64_t)nf * nf;
    double* tab = V + (int64_t)nf * nf;
    double* dg = tab;                          // the diagonal; behind it the column of every rank (nf ints of the 2 nf of
    int* col = (int*)(tab + nf);               // k_ceig_vec), then the sorted spectrum
    double* sw = tab + 2 * nf;
    const double* P = a.x + d.blk;
    const double* S = a.upd + d.upd;
    double* Uk = a.Q + a.qptr[k];
    double* Wk = a.pw + a.qptr[k];
    const double relax = a.lo;
    cone_form(d, P, S, Uk, Wk, relax, F);
    for (int t = SMCP_TID; t < nf * nf; t += MRC_NT) V[t] = (t % (nf + 1) == 0) ? 1.0 : 0.0;
    __syncthreads();
    int noconv;
    const int sweeps = ceig_jacobi<true>(nf, F, (nf + 1) / 2 <= CEIG_TAB_H ? stab : tab, red, &noconv, V);
    if (!noconv) {
      for (int i = SMCP_TID; i < nf; i += MRC_NT) dg[i] = F[i + (int64_t)i * nf];
      __syncthreads();
      for (int i = SMCP_TID; i < nf; i += MRC_NT) {
        const double v = dg[i];
        int r = 0;
        for (int j = 0; j < nf; ++j) r += (dg[j] < v || (dg[j] == v && j < i)) ? 1 : 0;
        sw[r] = v;
        col[r] = i;
      }
      __syncthreads();
      cone_form(d, P, S, Uk, Wk, relax, F);
      double cn = 0.0;
      for (int r = SMCP_TID; r < nf; r += MRC_NT) cn += sw[r] < 0.0 ? 1.0 : 0.0;
      const int nneg = (int)ceig_reduce(cn, false, red);
      double rs = 0.0;
      for (int t = SMCP_TID; t < nf * nf; t += MRC_NT) {
        const int i = t % nf, j = t / nf;
        if (i >= j) {
          double u = 0.0;
          for (int r = 0; r < nneg; ++r) {
            const double* q = V + (int64_t)col[r] * nf;
            u += sw[r] * (q[i] * q[j]);
          }
          const double tk = F[t], w = tk - 2.0 * u;
          const double dz = cone_x(d, P, S, i, j) - (tk - u);
          rs += i == j ? dz * dz : 2.0 * (dz * dz);
          Uk[t] = u;
          Uk[j + (int64_t)i * nf] = u;
          Wk[t] = w;
          Wk[j + (int64_t)i * nf] = w;
        }
      }
      rs = ceig_reduce(rs, false, red);
      if (SMCP_TID == 0) {
        a.pinfo[2 * k] = (double)nneg;
        a.pinfo[2 * k + 1] = rs;
      }
    } else {
      for (int t = SMCP_TID; t < nf * nf; t += MRC_NT) Uk[t] = Wk[t] = NAN;
      if (SMCP_TID == 0) a.pinfo[2 * k] = a.pinfo[2 * k + 1] = NAN;
    }
    if (SMCP_TID == 0) {
      a.rank[k] = sweeps;
      a.flag[k] = noconv ? CEIG_NO_CONV : 0;
    }
    __syncthreads();
  }
}

// mw, the signed multiplicities: per slot of blkval the number of cliques that hold the entry, negative on the diagonal
// of the matrix, 0 on the unused slots above the diagonal of a diagonal block.  One level of the scatter of all-ones
// blocks (k_clique_scatter with Z = 1), the diagonal negated once the children's counts are in.
__global__ void __launch_bounds__(MRC_NT) k_cone_mult(TreeArgs a, double* mw) {
  const int k = a.lev[blockIdx.x];
  const CliqueDesc d = a.cl[k];
  const int nn = d.nn, na = d.na, nf = nn + na;
  double* P = mw + d.blk;
  double* Uk = a.upd + d.upd;
  for (int e = SMCP_TID; e < nf * nn; e += MRC_NT) P[e] = e % nf >= e / nf ? 1.0 : 0.0;
  for (int e = SMCP_TID; e < na * na; e += MRC_NT) Uk[e] = e % na >= e / na ? 1.0 : 0.0;
  __syncthreads();
  add_children(a, d, a.upd, P, Uk, 1.0, 1.0);
  for (int j = SMCP_TID; j < nn; j += MRC_NT) P[j + (int64_t)j * nf] = -P[j + (int64_t)j * nf];
}

// The update on the pattern: x <- (a + rho sw) / (1 + rho |mw|) with sw = the scatter of the W_k, zeros on the unused slots
// whatever a and x hold there; part[blockIdx.x] = this workgroup's share of |x_new - x_old|^2 in the norm of csp_dot (1 on
// the diagonal, 2 off it), summed in a fixed tree.  The grid is a function of len alone.
__global__ void __launch_bounds__(MRC_NT) k_cone_update(int64_t len, const double* a, const double* sw, const double* mw, double rho,
                                                         double* x, double* part) {
  __shared__ double red[MRC_NT];
  double acc = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * MRC_NT + SMCP_TID; e < len; e += (int64_t)gridDim.x * MRC_NT) {
    const double m = mw[e];
    double v = 0.0;
    if (m != 0.0) {
      v = (a[e] + rho * sw[e]) / (1.0 + rho * fabs(m));
      const double dx = v - x[e];
      acc += m < 0.0 ? dx * dx : 2.0 * (dx * dx);
    }
    x[e] = v;
  }
  acc = ceig_reduce(acc, false, red);
  if (SMCP_TID == 0) part[blockIdx.x] = acc;
}

// One row of the history: hist[0] = sum_k r_k^2, hist[1] = the sum of the npart partial sums of k_cone_update,
// hist[2] = the negative eigenvalues over all cliques, hist[3] = 1 + the lowest clique that did not converge (0: none);
// every sum one thread's strided loop and the tree of ceig_reduce.  msw: the most sweeps of a clique since the call with
// reset set.
__global__ void __launch_bounds__(MRC_NT) k_cone_resid(const double* pinfo, const int32_t* sweeps, const int32_t* flag, int nsn,
                                                        const double* part, int npart, double* hist, int32_t* msw, int reset) {
  __shared__ double red[MRC_NT];
  double r2 = 0.0, ng = 0.0, s2 = 0.0, best;
  for (int k = SMCP_TID; k < nsn; k += MRC_NT) { ng += pinfo[2 * k]; r2 += pinfo[2 * k + 1]; }
  for (int p = SMCP_TID; p < npart; p += MRC_NT) s2 += part[p];
  r2 = ceig_reduce(r2, false, red);
  ng = ceig_reduce(ng, false, red);
  s2 = ceig_reduce(s2, false, red);
  const int ncv = mrc_argmax(nsn, [&](int k) { return flag[k] == CEIG_NO_CONV ? -(double)k : -INFINITY; }, best);
  const int sw = mrc_argmax(nsn, [&](int k) { return (double)sweeps[k]; }, best);
  if (SMCP_TID == 0) {
    hist[0] = r2;
    hist[1] = s2;
    hist[2] = ng;
    hist[3] = ncv >= 0 ? (double)(ncv + 1) : 0.0;
    const int most = sw >= 0 ? sweeps[sw] : 0, before = reset ? 0 : *msw;
    *msw = most > before ? most : before;
  }
}

// Z_k = the full symmetric block of clique k = blockIdx.x of the matrix with blkval x and gathered separator blocks upd:
// ceig_form straight to global memory, gridDim.y workgroups per clique
__global__ void __launch_bounds__(MRC_NT) k_clique_gather(const CliqueDesc* cl, const double* x, const double* upd, const int64_t* qptr,
                                                           double* Z) {
  const CliqueDesc d = cl[blockIdx.x];
  ceig_form(d, x + d.blk, upd + d.upd, Z + qptr[blockIdx.x], blockIdx.y, gridDim.y);
}

// One level of x = P_V(sum_k E_k Z_k E_k^T), a workgroup per clique: the panel (zeros above the diagonal of the diagonal
// block) and the update block from the lower triangle of Z_k, then the children's update blocks on top in the order of chidx
__global__ void __launch_bounds__(MRC_NT) k_clique_scatter(TreeArgs a, const double* Z, const int64_t* qptr, double* x) {
  const int k = a.lev[blockIdx.x];
  const CliqueDesc d = a.cl[k];
  const int nn = d.nn, na = d.na, nf = nn + na;
  const double* Zk = Z + qptr[k];
  double* P = x + d.blk;
  double* Uk = a.upd + d.upd;
  for (int e = SMCP_TID; e < nf * nn; e += MRC_NT) P[e] = e % nf >= e / nf ? Zk[e] : 0.0;
  for (int e = SMCP_TID; e < na * na; e += MRC_NT) {
    const int i = e % na, j = e / na;
    Uk[e] = i >= j ? Zk[(nn + i) + (int64_t)(nn + j) * nf] : 0.0;
  }
  __syncthreads();
  add_children(a, d, a.upd, P, Uk, 1.0, 1.0);
}

// ext[0] = the smallest eigenvalue over all cliques, ext[1] = the lowest clique attaining it, ext[2] = the largest,
// ext[3] = the lowest clique attaining that; out[0] = 1 + the lowest clique whose B block is not positive definite (0: none),
// out[1] = 1 + the lowest clique that did not converge (0: none), out[2] = the most sweeps of a clique
__global__ void __launch_bounds__(MRC_NT) k_ceig_reduce(const CliqueDesc* cl, const double* w, const int32_t* sweeps,
                                                         const int32_t* flag, int nsn, double* ext, int32_t* out) {
  double vmin, vmax, best;
  const int kmin = mrc_argmax(nsn, [&](int k) { return -w[cl[k].rows]; }, vmin);
  const int kmax = mrc_argmax(nsn, [&](int k) { return w[cl[k].rows + cl[k].nn + cl[k].na - 1]; }, vmax);
  const int bad = mrc_argmax(nsn, [&](int k) { return flag[k] == CEIG_NOT_PD ? -(double)k : -INFINITY; }, best);
  const int ncv = mrc_argmax(nsn, [&](int k) { return flag[k] == CEIG_NO_CONV ? -(double)k : -INFINITY; }, best);
  const int sw = mrc_argmax(nsn, [&](int k) { return (double)sweeps[k]; }, best);
  if (SMCP_TID == 0) {
    ext[0] = kmin >= 0 ? -vmin : NAN;
    ext[1] = (double)kmin;
    ext[2] = kmax >= 0 ? vmax : NAN;
    ext[3] = (double)kmax;
    out[0] = bad >= 0 ? bad + 1 : 0;
    out[1] = ncv >= 0 ? ncv + 1 : 0;
    out[2] = sw >= 0 ? sweeps[sw] : 0;
  }
}

}  // namespace smcp
