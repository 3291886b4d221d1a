// Dense maximum-determinant positive semidefinite completion (csp_psdcompletion): the n x n matrix Xh with Xh = X on V
// whose inverse vanishes off V when X is positive definite on V, and the limit of that matrix when X is only positive
// semidefinite on every clique -- CHOMPACK's psdcompletion.
//
// Per clique k with columns N and separator A (|A| > 0):  W_k = the basic solution of X_AA W = X_AN from the diagonally
// pivoted Cholesky of X_AA (mrc_pchol: pivots rho above tol * max diag X_AA), W_k[rho] = X[rho, rho]^-1 X[rho, N], the other
// rows zero (k_psd_solve; everything it reads lies on V, so ONE launch does the whole tree).  The fill walks the levels of
// the clique tree root first; with U the columns of the levels already done,
//   step 1   Xh[U \ A, N] = Xh[U \ A, A[rho]] W_k[rho]          for every clique of the level
//   step 2   Xh[N_s, N]   = Xh[N_s, A[rho]]   W_k[rho]          for the cliques s > k of the same level
// (two launches of k_psd_fill per level: step 2 reads rows step 1 wrote).  Every product is a 64-row tile on
// v_mfma_f64_16x16x4 (gemm_tile64 of front_large.hip) whose gathered operand is read as Xh[A[rho]_j, R] -- Xh is symmetric,
// and the rows R of a tile are consecutive entries of `ulist`, the columns in the order the levels complete them -- and
// each tile is written twice, as computed and transposed, both from LDS with consecutive lanes on consecutive addresses.
// Entries on V are never rewritten: the only rows of U that meet N on V are those of A, and they are masked.
// Every sum is a fixed-order loop: the same input gives the same Xh bit for bit.
#include <hip/hip_runtime.h>

#include "context.hpp"
#include "wgblas.hpp"

namespace smcp {

// doubles of one slot of k_psd_solve: X_AA, its factor, lv; done and piv (ints)
__host__ __device__ inline int64_t psd_slot(int64_t na) { return 2 * na * na + 2 * na + 2; }

// Xd[i * ld + j] = 0, i, j < n
__global__ void __launch_bounds__(MRC_NT) k_psd_zero(int64_t n, double* Xd, int64_t ld) {
  const int64_t j = (int64_t)blockIdx.x * MRC_NT + SMCP_TID;
  if (j >= n) return;
  for (int64_t i = blockIdx.y; i < n; i += gridDim.y) Xd[i * ld + j] = 0.0;
}

// both triangles of X on V: one workgroup per clique (the part of a panel above the diagonal of its N x N block is not X)
__global__ void __launch_bounds__(MRC_NT) k_psd_scatter(const CliqueDesc* cl, const int32_t* rowidx, const double* x,
                                                         double* Xd, int64_t ld) {
  const CliqueDesc d = cl[blockIdx.x];
  const int nn = d.nn, nf = d.nn + d.na;
  const int32_t* rows = rowidx + d.rows;
  const double* P = x + d.blk;
  for (int t = SMCP_TID; t < nf * nn; t += MRC_NT) {
    const int i = t % nf, j = t / nf;
    if (i < j) continue;
    const double v = P[t];
    const int64_t r = rows[i], c = d.first + j;
    Xd[c * ld + r] = v;
    Xd[r * ld + c] = v;
  }
}

// W_k of every clique of the launch (MrcArgs: pw, pidx, pra).  The ra x nn block W_k[rho] goes to pw + blk (column c at
// + c * na: it fits the clique's panel), the global rows A[rho] to pidx + rel, ra to pra[k].
__global__ void __launch_bounds__(MRC_NT) k_psd_solve(MrcArgs a) {
  extern __shared__ double psd_lds[];
  double* ws = a.ws ? a.ws + (int64_t)blockIdx.x * a.slot : psd_lds;
  for (int e = blockIdx.x; e < a.cnt; e += gridDim.x) {
    const int k = a.lev[e];
    const CliqueDesc d = a.cl[k];
    const int nn = d.nn, na = d.na, nf = nn + na;
    const double* P = a.x + d.blk;
    const double* U = a.upd + d.upd;
    const int32_t* sep = a.rowidx + d.rows + nn;
    double* A = ws;
    double* L = A + (int64_t)na * na;
    double* lv = L + (int64_t)na * na;
    int* done = (int*)(lv + na);
    int* piv = done + na;
    for (int t = SMCP_TID; t < na * na; t += MRC_NT)
      if (t % na >= t / na) A[t] = U[t];
    __syncthreads();
    double md;
    mrc_argmax(na, [&](int i) { return a.xdiag[sep[i]]; }, md);
    const double thr = a.tol * (md > 0.0 ? md : 0.0);
    int neg, more;
    const int ra = mrc_pchol(na, A, na, thr, na, L, na, lv, done, &neg, &more, piv);
    __syncthreads();
    double* W = a.pw + d.blk;
    for (int t = SMCP_TID; t < ra * nn; t += MRC_NT) {
      const int i = t % ra, c = t / ra;
      W[i + (int64_t)c * na] = P[nn + piv[i] + (int64_t)c * nf];
    }
    for (int i = SMCP_TID; i < ra; i += MRC_NT) a.pidx[d.rel + i] = sep[piv[i]];
    if (SMCP_TID == 0) a.pra[k] = ra;
    __syncthreads();
    // X[rho, rho] = Lp Lp^T with Lp[i, j] = L[piv[i] + j * na] lower triangular: Lp Z = B, then Lp^T W = Z, in place
    for (int j = 0; j < ra; ++j) {
      const double r = 1.0 / L[piv[j] + (int64_t)j * na];
      for (int c = SMCP_TID; c < nn; c += MRC_NT) W[j + (int64_t)c * na] *= r;
      __syncthreads();
      const int rem = ra - j - 1;
      for (int t = SMCP_TID; t < rem * nn; t += MRC_NT) {
        const int i = j + 1 + t % rem, c = t / rem;
        W[i + (int64_t)c * na] -= L[piv[i] + (int64_t)j * na] * W[j + (int64_t)c * na];
      }
      __syncthreads();
    }
    for (int j = ra - 1; j >= 0; --j) {
      const double r = 1.0 / L[piv[j] + (int64_t)j * na];
      for (int c = SMCP_TID; c < nn; c += MRC_NT) W[j + (int64_t)c * na] *= r;
      __syncthreads();
      for (int t = SMCP_TID; t < j * nn; t += MRC_NT) {
        const int i = t % j, c = t / j;
        W[i + (int64_t)c * na] -= L[piv[j] + (int64_t)i * na] * W[j + (int64_t)c * na];
      }
      __syncthreads();
    }
  }
}

// one 64-row tile of a fill product: clique k, rows ulist[off .. off + cnt), columns n0 .. n0 + 64 of N_k
struct PsdTask { int32_t k, off, cnt, n0; };

struct PsdFillArgs {
  const CliqueDesc* cl;
  const int32_t* rowidx;
  const PsdTask* tasks;
  const int32_t* ulist;
  const double* w;          // W_k[rho] at cl[k].blk, leading dimension na
  const int32_t* idx;       // A[rho] at cl[k].rel
  const int32_t* ra;
  double* X;
  int64_t ld;
};

constexpr int PSD_LST = LT + 1;     // leading dimension of the staged output tile

__global__ void __launch_bounds__(256) k_psd_fill(PsdFillArgs a) {
  __shared__ double sA[LKC * LSA];
  __shared__ double sB[LT * LSB];
  __shared__ double sT[LT * PSD_LST];
  __shared__ int sR[LT];            // the rows of the tile; -1: none, or a row of the separator (on V: not written)
  const PsdTask t = a.tasks[blockIdx.x];
  const CliqueDesc d = a.cl[t.k];
  const int nn = d.nn, na = d.na, ra = a.ra[t.k];
  const int tid = threadIdx.x;
  const int32_t* ul = a.ulist + t.off;
  if (tid < LT) {
    int r = -1;
    if (tid < t.cnt) {
      r = ul[tid];
      const int32_t* sep = a.rowidx + d.rows + nn;
      int lo = 0, hi = na;            // first position with sep[pos] >= r
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sep[mid] < r) lo = mid + 1; else hi = mid;
      }
      if (lo < na && sep[lo] == r) r = -1;
    }
    sR[tid] = r;
  }
  __syncthreads();
  const double* W = a.w + d.blk;
  const int32_t* idx = a.idx + d.rel;
  double* X = a.X;
  const int64_t ld = a.ld;
  d4 acc[2][2];
  tile64_zero(acc);
  gemm_tile64<1>(acc, t.cnt, nn, ra, 0, t.n0, [=](int m, int kk) { return X[(int64_t)idx[kk] * ld + ul[m]]; },
                 [=](int kk, int n) { return W[kk + (int64_t)n * na]; }, sA, sB);
  tile64_foreach(acc, 0, 0, LT, LT, [&](int m, int n, double v) { sT[m + n * PSD_LST] = v; });
  __syncthreads();
  const int ncol = min(LT, nn - t.n0);
  const int64_t c0 = d.first + t.n0;
  const int q = tid & 63, p0 = tid >> 6;
  {                                   // Xh[N, R]: lanes along the rows of the tile
    const int r = sR[q];
    if (r >= 0)
      for (int n = p0; n < ncol; n += 4) X[(c0 + n) * ld + r] = sT[q + n * PSD_LST];
  }
  if (q < ncol)                       // Xh[R, N]: lanes along the columns
    for (int m = p0; m < LT; m += 4) {
      const int r = sR[m];
      if (r >= 0) X[(int64_t)r * ld + c0 + q] = sT[m + q * PSD_LST];
    }
}

}  // namespace smcp
