// Minimum-rank positive semidefinite completion (csp_mrcompletion_rank / csp_mrcompletion): Y (n x r) with
// P_V(Y Y^T) = X, r = the largest numerical rank of a clique block X_gg -- CHOMPACK's mrcompletion.
//
// Pass 1 (k_mrc_rank): every clique k forms its whole block F = X_gg (own columns from the panel, the separator block
// X_AA from the top-down gather of front_generic.hip) and runs a diagonally pivoted Cholesky (LAPACK pstrf semantics):
// pivots are taken while the largest remaining diagonal entry exceeds thr = tol * max diag F; rank_k = their number.  A
// remaining diagonal entry below -thr means F is not positive semidefinite: X has no such completion.
// Pass 2 (k_mrc_factor, one launch per level, root first): with Y_A (the separator rows, written by the ancestors),
//   Y_A^T P = Q R         column-pivoted Householder QR, ra steps (the pivoted Cholesky of Y_A Y_A^T = F_AA)
//   Z1 = (F_NA P)[:, :ra] R11^-1
//   Z2 = pivoted Cholesky factor of F_NN - Z1 Z1^T, rn <= r - ra columns (more would be dropped: recorded per clique)
//   Y_N = [Z1 Z2 0] Q^T   (the reflectors applied from the right, no explicit Q)
// so that Y_N Y_A^T = F_NA and Y_N Y_N^T = F_NN.  A root is the case na = 0: Y_N = the pivoted factor of F_NN.
//
// One workgroup per clique (workgroups loop over the cliques of a launch when there are more of them than slots); its
// operands live in one slot of scratch -- LDS when the largest clique of the launch fits, HBM otherwise -- through the
// workgroup routines below, which take any pointer.  Every sum is a fixed-order loop of one thread or a fixed tree:
// the same input gives the same Y bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>

#include "context.hpp"
#include "wgblas.hpp"

namespace smcp {

constexpr int MRC_NT = 256;     // threads per workgroup of every kernel below (the reductions assume it)

struct MrcArgs {
  const CliqueDesc* cl;
  const int32_t* rowidx;
  const int32_t* lev;       // cliques of this launch
  int cnt;
  const double* x;          // blkval of X
  const double* upd;        // X_AA of every clique at cl[k].upd (pass 1)
  const double* xdiag;      // diagonal of X, permuted order (k_mrc_diag)
  double tol;
  double* ws;               // HBM slots (nullptr: the slot is the workgroup's dynamic LDS)
  int64_t slot;             // doubles per HBM slot
  int32_t* rank;            // per clique: numerical rank of X_gg (pass 1)
  int32_t* flag;            // per clique: pass 1: 1 = not positive semidefinite; pass 2: columns the clamp dropped
  double* Y;                // pass 2: n x r, row i at Y + i * ldY (permuted order)
  int64_t ldY;
  int r;
  double* pw;               // k_psd_solve (front_psd.hip): W_k[rho] of every clique, A[rho], |rho|
  int32_t* pidx;
  int32_t* pra;
  const double* x2;         // k_ceig (front_ceig.hip): blkval of B and B_AA of every clique (null: standard form), the
  const double* upd2;       // eigenvalues of clique k at w + cl[k].rows
  double* w;
  double* Q;                // k_ceig_vec: the packed clique blocks it writes (block k at Q + qptr[k]): the eigenvectors
  const int64_t* qptr;      // (vmode 0) or the block with its spectrum clipped to [lo, hi] (vmode 1), then per clique the
  double lo, hi;            // eigenvalues changed and the squared distance at pinfo + 2 k
  double* pinfo;
  int vmode;
  // k_cone_split reads these differently: Q = U and pw = W (packed clique blocks, rewritten in place), lo = the
  // over-relaxation, pinfo + 2 k = the negative eigenvalues and the squared primal residual of clique k
};

// (value, index) of the largest val(i), i < n; ties go to the lowest index, -1 when every value is -inf / NaN.  The
// result reaches every thread.
template <class F>
__device__ inline int mrc_argmax(int n, F val, double& best) {
  __shared__ double sv[MRC_NT];
  __shared__ int si[MRC_NT];
  double bv = -INFINITY;
  int bi = -1;
  for (int i = SMCP_TID; i < n; i += MRC_NT) {
    const double v = val(i);
    if (v > bv) { bv = v; bi = i; }
  }
  sv[SMCP_TID] = bv;
  si[SMCP_TID] = bi;
  __syncthreads();
  for (int s = MRC_NT / 2; s > 0; s >>= 1) {
    if (SMCP_TID < s) {
      const double v = sv[SMCP_TID + s];
      const int j = si[SMCP_TID + s];
      if (j >= 0 && (si[SMCP_TID] < 0 || v > sv[SMCP_TID] || (v == sv[SMCP_TID] && j < si[SMCP_TID]))) {
        sv[SMCP_TID] = v;
        si[SMCP_TID] = j;
      }
    }
    __syncthreads();
  }
  best = sv[0];
  const int r = si[0];
  __syncthreads();
  return r;
}

// Diagonally pivoted Cholesky of the symmetric n x n matrix A (lower triangle, column-major, lda; overwritten).  Pivots
// are taken while the largest remaining diagonal entry exceeds thr, at most maxcols of them.  Column j of the factor, in
// A's row order (zero in the rows pivoted before), goes to L + j * ldl when L is given.  lv: n doubles, done: n ints of
// scratch.  Returns the number of pivots; *neg = 1 when the factorisation ran to the threshold and a remaining diagonal
// entry is below -thr (A is not positive semidefinite), *more = 1 when it stopped at maxcols with a pivot above thr left.
// piv (optional, n ints): piv[j] = the row pivot j took.
__device__ inline int mrc_pchol(int n, double* A, int64_t lda, double thr, int maxcols, double* L, int64_t ldl,
                                double* lv, int* done, int* neg, int* more, int* piv = nullptr) {
  for (int i = SMCP_TID; i < n; i += MRC_NT) done[i] = 0;
  __syncthreads();
  *neg = 0;
  *more = 0;
  int j = 0;
  for (;; ++j) {
    double d;
    const int p = mrc_argmax(n, [&](int i) { return done[i] ? -INFINITY : A[i + i * lda]; }, d);
    if (p < 0 || !(d > thr)) break;
    if (j == maxcols) { *more = 1; break; }
    const double s = sqrt(d), rs = 1.0 / s;
    for (int i = SMCP_TID; i < n; i += MRC_NT) {
      const double v = (done[i] || i == p) ? 0.0 : (i > p ? A[i + p * lda] : A[p + i * lda]) * rs;
      lv[i] = v;
      if (L) L[i + j * ldl] = i == p ? s : v;
    }
    __syncthreads();
    if (SMCP_TID == 0) {
      done[p] = 1;
      if (piv) piv[j] = p;
    }
    for (int e = SMCP_TID; e < n * n; e += MRC_NT) {       // trailing update; pivoted rows have lv = 0
      const int i = e % n, k = e / n;
      if (i >= k) A[i + (int64_t)k * lda] -= lv[i] * lv[k];
    }
    __syncthreads();
  }
  if (!*more) {
    double dmin;
    const int q = mrc_argmax(n, [&](int i) { return done[i] ? -INFINITY : -A[i + i * lda]; }, dmin);
    if (q >= 0 && -dmin < -thr) *neg = 1;
  }
  return j;
}

// Householder QR with column pivoting of the m x nc matrix M (column-major, ldm): M P = Q R.  Steps are taken while
// the largest remaining column norm squared exceeds thr.  On return the leading rows of M hold R (on and above the
// diagonal), the Householder vectors lie below the diagonal (unit leading entry implied), tau[j] are their scalars and
// perm[j] the original column of pivot j.  cn: nc doubles of scratch.  Returns the number of steps.
__device__ inline int mrc_qrp(int m, int nc, double* M, int64_t ldm, double thr, double* tau, int* perm, double* cn) {
  for (int q = SMCP_TID; q < nc; q += MRC_NT) perm[q] = q;
  __syncthreads();
  const int kmax = m < nc ? m : nc;
  int j = 0;
  for (; j < kmax; ++j) {
    for (int q = j + SMCP_TID; q < nc; q += MRC_NT) {
      double s = 0.0;
      for (int i = j; i < m; ++i) s += M[i + q * ldm] * M[i + q * ldm];
      cn[q] = s;
    }
    __syncthreads();
    double d;
    int p = mrc_argmax(nc - j, [&](int t) { return cn[j + t]; }, d);
    if (p < 0 || !(d > thr)) break;
    p += j;
    if (p != j) {
      for (int i = SMCP_TID; i < m; i += MRC_NT) {
        const double t = M[i + j * ldm];
        M[i + j * ldm] = M[i + p * ldm];
        M[i + p * ldm] = t;
      }
      if (SMCP_TID == 0) { const int t = perm[j]; perm[j] = perm[p]; perm[p] = t; }
      __syncthreads();
    }
    const double alpha = M[j + j * ldm], nrm = sqrt(d);
    const double beta = alpha >= 0.0 ? -nrm : nrm;
    const double sc = 1.0 / (alpha - beta);
    __syncthreads();
    for (int i = j + 1 + SMCP_TID; i < m; i += MRC_NT) M[i + j * ldm] *= sc;
    if (SMCP_TID == 0) {
      M[j + j * ldm] = beta;
      tau[j] = (beta - alpha) / beta;
    }
    __syncthreads();
    const double t = tau[j];
    for (int q = j + 1 + SMCP_TID; q < nc; q += MRC_NT) {      // H = I - t v v^T on the remaining columns
      double w = M[j + q * ldm];
      for (int i = j + 1; i < m; ++i) w += M[i + j * ldm] * M[i + q * ldm];
      w *= t;
      M[j + q * ldm] -= w;
      for (int i = j + 1; i < m; ++i) M[i + q * ldm] -= w * M[i + j * ldm];
    }
    __syncthreads();
  }
  return j;
}

// largest diagonal entry of X over the rows of clique k (the scale of its rank threshold), at least 0
__device__ inline double mrc_maxdiag(const MrcArgs& a, const CliqueDesc& d, const int32_t* rows) {
  double md;
  mrc_argmax(d.nn + d.na, [&](int i) { return a.xdiag[rows[i]]; }, md);
  return md > 0.0 ? md : 0.0;
}

// xdiag[j] = X_jj (permuted order): one workgroup per clique
__global__ void __launch_bounds__(MRC_NT) k_mrc_diag(const CliqueDesc* cl, const double* x, double* xdiag) {
  const CliqueDesc d = cl[blockIdx.x];
  const int nf = d.nn + d.na;
  for (int t = SMCP_TID; t < d.nn; t += MRC_NT) xdiag[d.first + t] = x[d.blk + (int64_t)t * nf + t];
}

// doubles of one slot: pass 1 (front order nf), pass 2 (supernode nn, separator na, r columns)
__host__ __device__ inline int64_t mrc_slot1(int64_t nf) { return nf * nf + 2 * nf + 2; }
__host__ __device__ inline int64_t mrc_slot2(int64_t nn, int64_t na, int64_t r) {
  return r * na + nn * r + nn * nn + 3 * na + 2 * nn + 4;
}

__global__ void __launch_bounds__(MRC_NT) k_mrc_rank(MrcArgs a) {
  extern __shared__ double mrc_lds[];
  double* ws = a.ws ? a.ws + (int64_t)blockIdx.x * a.slot : mrc_lds;
  for (int e = blockIdx.x; e < a.cnt; e += gridDim.x) {
    const int k = a.lev[e];
    const CliqueDesc d = a.cl[k];
    const int nn = d.nn, na = d.na, nf = nn + na;
    const double* P = a.x + d.blk;
    const double* U = a.upd + d.upd;
    double* F = ws;
    double* lv = F + (int64_t)nf * nf;
    int* done = (int*)(lv + nf);
    for (int t = SMCP_TID; t < nf * nf; t += MRC_NT) {
      const int i = t % nf, j = t / nf;
      if (i >= j) F[t] = j < nn ? P[i + (int64_t)j * nf] : U[(i - nn) + (int64_t)(j - nn) * na];
    }
    __syncthreads();
    const double thr = a.tol * mrc_maxdiag(a, d, a.rowidx + d.rows);
    int neg, more;
    const int rk = mrc_pchol(nf, F, nf, thr, nf, nullptr, 0, lv, done, &neg, &more);
    if (SMCP_TID == 0) {
      a.rank[k] = rk;
      a.flag[k] = neg;
    }
    __syncthreads();
  }
}

// out[0] = max rank, out[1] = 1 + the lowest clique that is not positive semidefinite (0: none)
__global__ void __launch_bounds__(MRC_NT) k_mrc_reduce(const int32_t* rank, const int32_t* flag, int nsn, int32_t* out) {
  double best;
  const int q = mrc_argmax(nsn, [&](int k) { return (double)rank[k]; }, best);
  const int b = mrc_argmax(nsn, [&](int k) { return flag[k] ? -(double)k : -INFINITY; }, best);
  int clamped = 0;
  if (SMCP_TID == 0) {
    for (int k = 0; k < nsn; ++k) clamped += flag[k];
    out[0] = q >= 0 ? rank[q] : 0;
    out[1] = b >= 0 ? b + 1 : 0;
    out[2] = clamped;
  }
}

__global__ void __launch_bounds__(MRC_NT) k_mrc_factor(MrcArgs a) {
  extern __shared__ double mrc_lds[];
  double* ws = a.ws ? a.ws + (int64_t)blockIdx.x * a.slot : mrc_lds;
  const int r = a.r;
  for (int e = blockIdx.x; e < a.cnt; e += gridDim.x) {
    const int k = a.lev[e];
    const CliqueDesc d = a.cl[k];
    const int nn = d.nn, na = d.na, nf = nn + na;
    const double* P = a.x + d.blk;
    const int32_t* rows = a.rowidx + d.rows;
    double* M = ws;                                  // r x na : Y_A^T, then its QR
    double* W = M + (int64_t)r * na;                 // nn x r : [Z1 Z2 0], then Y_N
    double* S = W + (int64_t)nn * r;                 // nn x nn: F_NN - Z1 Z1^T
    double* tau = S + (int64_t)nn * nn;              // na
    double* cn = tau + na;                           // na
    double* lv = cn + na;                            // nn
    int* perm = (int*)(lv + nn);                     // na
    int* done = perm + na + (na & 1);                // nn
    for (int t = SMCP_TID; t < r * na; t += MRC_NT) {
      const int c = t % r, i = t / r;
      M[t] = a.Y[(int64_t)rows[nn + i] * a.ldY + c];
    }
    for (int t = SMCP_TID; t < nn * r; t += MRC_NT) W[t] = 0.0;
    __syncthreads();
    const double thr = a.tol * mrc_maxdiag(a, d, rows);
    const int ra = na ? mrc_qrp(r, na, M, r, thr, tau, perm, cn) : 0;
    for (int i = SMCP_TID; i < nn; i += MRC_NT)      // Z1 R11 = (F_NA P)[:, :ra], row by row
      for (int j = 0; j < ra; ++j) {
        double z = P[(int64_t)i * nf + nn + perm[j]];
        for (int l = 0; l < j; ++l) z -= W[i + (int64_t)l * nn] * M[l + (int64_t)j * r];
        W[i + (int64_t)j * nn] = z / M[j + (int64_t)j * r];
      }
    __syncthreads();
    for (int t = SMCP_TID; t < nn * nn; t += MRC_NT) {
      const int i = t % nn, j = t / nn;
      if (i < j) continue;
      double s = P[i + (int64_t)j * nf];
      for (int l = 0; l < ra; ++l) s -= W[i + (int64_t)l * nn] * W[j + (int64_t)l * nn];
      S[t] = s;
    }
    __syncthreads();
    int neg, more;
    const int rn = mrc_pchol(nn, S, nn, thr, r - ra, W + (int64_t)ra * nn, nn, lv, done, &neg, &more);
    (void)rn;
    // Y_N = W Q^T = W H_{ra-1} ... H_0: every thread owns rows of W
    for (int i = SMCP_TID; i < nn; i += MRC_NT)
      for (int j = ra - 1; j >= 0; --j) {
        double w = W[i + (int64_t)j * nn];
        for (int c = j + 1; c < r; ++c) w += W[i + (int64_t)c * nn] * M[c + (int64_t)j * r];
        w *= tau[j];
        W[i + (int64_t)j * nn] -= w;
        for (int c = j + 1; c < r; ++c) W[i + (int64_t)c * nn] -= w * M[c + (int64_t)j * r];
      }
    __syncthreads();
    for (int t = SMCP_TID; t < nn * r; t += MRC_NT) {
      const int c = t % r, i = t / r;
      a.Y[(int64_t)(d.first + i) * a.ldY + c] = W[i + (int64_t)c * nn];
    }
    if (SMCP_TID == 0) a.flag[k] = more;
    __syncthreads();
  }
}

// ---- max-cut rounding (csp_maxcut_cuts) ---------------------------------------------------
// s[t * n + i] = sign(Y_i . g_t) with 0 -> +1; Y row i at Y + i * ldY (r columns), g_t at G + t * r
__global__ void __launch_bounds__(MRC_NT) k_cut_signs(int64_t n, int r, const double* Y, int64_t ldY, const double* G,
                                                       int8_t* s) {
  const int64_t i = (int64_t)blockIdx.x * MRC_NT + SMCP_TID;
  if (i >= n) return;
  const double* g = G + (int64_t)blockIdx.y * r;
  const double* y = Y + i * ldY;
  double v = 0.0;
  for (int c = 0; c < r; ++c) v += y[c] * g[c];
  s[(int64_t)blockIdx.y * n + i] = v < 0.0 ? -1 : 1;
}

// cut[t] = sum over edges e of w_e [s_t(ei_e) != s_t(ej_e)]: one workgroup per trial, fixed-order partial sums per
// thread and a fixed tree
__global__ void __launch_bounds__(MRC_NT) k_cut_weights(int64_t n, int64_t nedges, const int64_t* ei, const int64_t* ej,
                                                         const double* w, const int8_t* s, double* cut) {
  __shared__ double red[MRC_NT];
  const int8_t* st = s + (int64_t)blockIdx.x * n;
  double acc = 0.0;
  for (int64_t e = SMCP_TID; e < nedges; e += MRC_NT)
    if (st[ei[e]] != st[ej[e]]) acc += w[e];
  red[SMCP_TID] = acc;
  __syncthreads();
  for (int h = MRC_NT / 2; h > 0; h >>= 1) {
    if (SMCP_TID < h) red[SMCP_TID] += red[SMCP_TID + h];
    __syncthreads();
  }
  if (SMCP_TID == 0) cut[blockIdx.x] = red[0];
}

}  // namespace smcp
