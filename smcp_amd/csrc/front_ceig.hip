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
__device__ inline int ceig_jacobi(int nf, double* F, double* tab, double* red, int* noconv) {
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
      __syncthreads();
    }
  }
  return sweeps;
}

// the full symmetric block of clique d of the matrix with panel P (nf x nn) and gathered separator block U (na x na)
__device__ inline void ceig_form(const CliqueDesc& d, const double* P, const double* U, double* F) {
  const int nn = d.nn, na = d.na, nf = nn + na;
  for (int e = SMCP_TID; e < nf * nf; e += MRC_NT) {
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
