// Rank-k update and downdate of the supernodal factor: L L^T <- L L^T + V diag(a) V^T in place, for columns of V whose
// support lies inside one clique each.  With w = sqrt|a_j| v_j the rank-one step on panel column c is
//     x = w_c (0: nothing to do),  r^2 = d^2 + x^2 (update) or (d - x)(d + x) (downdate; <= 0: not positive definite)
//     rc = d / r, cc = r / d, ss = x / d, d <- r
//     every row i below:  l <- (l +- ss w_i) rc,  w_i <- cc w_i - ss l        (the new l: the mixed form)
// and a panel column takes the steps of the active columns of V one after the other, so the arithmetic is that of successive
// rank-one updates of the whole factor.  The support condition keeps w inside the rows of the clique it has reached: what is
// left of it after the columns N_s lies on A_s, which are rows of the parent.
//
//   k_cu_plan   a workgroup per column of V: finite check, first nonzero (min-reduction), its supernode (bisection over the
//               first columns of the cliques), every nonzero looked up in the sorted rows of that clique, the scaled copy into
//               the workspace, and one bit per pass in the visit byte of the supernode and of its ancestors.  L is not read.
//   k_cu_walk   ONE workgroup of 1024 threads.  It returns at once when a column was refused.  Otherwise, per pass of CU_KC
//               columns, it visits the marked supernodes in ascending number (children before parents, so every w it meets is
//               final), the panel in blocks of CU_CB columns: the triangle of the block and its w in LDS, a barrier per column,
//               the (rc, cc, ss) of every (panel column, V column) pair left in a table; then the rows below the block with a
//               thread per row (the panel is column-major: coalesced), w of the row in registers, no barrier.  The home of w is
//               the workspace in device memory (k x n): a row of w belongs to one thread at a time, and the barrier between
//               the phases orders the hand-over inside the workgroup.  It clears the visit bytes before it ends.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

namespace smcp {

constexpr int CU_KMAX = 64;          // columns of V per call
constexpr int CU_KC = 16;            // columns of V per pass of the walk (w of a row: 16 doubles in registers)
constexpr int CU_CB = 32;            // panel columns per block of the walk
constexpr int CU_NT = 1024;          // threads of the walk
constexpr int CU_HDR = 40;           // doubles of flags ahead of the visit bytes: CU_KMAX ints, then status and column
enum { CU_OK = 0, CU_BAD_SUPPORT = 1, CU_BAD_VALUE = 2 };

// the columns in the order they are taken: a_j > 0 first, then a_j < 0 (a_j = 0: no slot)
struct CuCols {
  double scale[CU_KMAX];             // by caller's column: sqrt|a_j|
  signed char slot[CU_KMAX];         // caller's column -> place in the order, -1: left out
  signed char col[CU_KMAX];          // place -> caller's column
  signed char sign[CU_KMAX];         // place -> +1 / -1
  int nact;
};

__host__ __device__ inline int64_t cu_visit_doubles(int64_t nsn) { return (nsn + 7) / 8; }
__host__ __device__ inline int64_t cu_ws_len(int64_t nsn, int64_t n, int64_t k) { return CU_HDR + cu_visit_doubles(nsn) + k * n; }

// grid (k), 256 threads
__global__ void __launch_bounds__(256) k_cu_plan(const CliqueDesc* cl, const int32_t* rowidx, int nsn, int n, const double* V, int64_t ldv,
                                                 CuCols cols, double* W, int64_t ldw, unsigned* visit, int* flags) {
  __shared__ int red[8];
  __shared__ int sn;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = blockIdx.x;
  const double* v = V + (int64_t)j * ldv;
  const int slot = cols.slot[j];
  if (slot < 0) {                                      // a_j = 0: the column is left out, unread
    if (tid == 0) flags[j] = CU_OK;
    return;
  }
  const double scale = cols.scale[j];
  double* w = W + (int64_t)slot * ldw;
  int first = INT_MAX, bad = 0;
  for (int r = tid; r < n; r += 256) {
    const double x = v[r];
    if (!(fabs(x) <= DBL_MAX)) bad = 1;                // NaN or infinite
    if (x != 0.0 && first == INT_MAX) first = r;
    w[r] = scale * x;
  }
  for (int s = 32; s >= 1; s >>= 1) {
    first = min(first, __shfl_xor(first, s, 64));
    bad |= __shfl_xor(bad, s, 64);
  }
  if (lane == 0) { red[wave] = first; red[4 + wave] = bad; }
  __syncthreads();
  first = min(min(red[0], red[1]), min(red[2], red[3]));
  bad = red[4] | red[5] | red[6] | red[7];
  if (bad || first == INT_MAX) {                       // (a column of zeros is inside every clique and marks nothing)
    if (tid == 0) flags[j] = bad ? CU_BAD_VALUE : CU_OK;
    return;
  }
  if (tid == 0) {                                      // the last clique whose first column is not beyond the first nonzero
    int lo = 0, hi = nsn - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (cl[mid].first <= first) lo = mid; else hi = mid - 1;
    }
    sn = lo;
  }
  __syncthreads();
  const int s = sn;
  const CliqueDesc d = cl[s];
  const int32_t* A = rowidx + d.rows + d.nn;           // the separator rows, ascending
  const int nend = d.first + d.nn;
  int out = 0;
  for (int r = tid; r < n; r += 256) {
    if (v[r] == 0.0 || r < nend) continue;             // (r >= first >= d.first: a column of the supernode itself)
    int lo = 0, hi = d.na;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (A[mid] < r) lo = mid + 1; else hi = mid;
    }
    if (lo >= d.na || A[lo] != r) out = 1;
  }
  __syncthreads();                                     // (red is read above)
  for (int sft = 32; sft >= 1; sft >>= 1) out |= __shfl_xor(out, sft, 64);
  if (lane == 0) red[wave] = out;
  __syncthreads();
  if (tid != 0) return;
  out = red[0] | red[1] | red[2] | red[3];
  flags[j] = out ? CU_BAD_SUPPORT : CU_OK;
  if (out) return;
  // the path to the root: whoever finds the bit of this pass already set leaves the rest to the one who set it
  const unsigned bit = 1u << (slot / CU_KC);
  for (int q = s; q >= 0; q = cl[q].parent) {
    const unsigned m = bit << (8 * (q & 3));
    if (atomicOr(visit + (q >> 2), m) & m) break;
  }
}

struct CuWalkArgs {
  const CliqueDesc* cl; const int32_t* rowidx; int nsn;
  double* L; double* W; int64_t ldw;
  unsigned* visit; const int* flags; int* status;      // status[0]: what the call returns, status[1]: the column it names
  int k; int e_support, e_value;                       // the codes of a refused column
};

// One supernode of one pass (columns [m0, m0 + kcp) of the order); returns 0 or 1 + the caller's column of a failed downdate,
// the same value in every thread.
__device__ inline int cu_visit(const CuWalkArgs& a, const CuCols& cols, int s, int m0, int kcp, double* tri, double* wt, double* P, int* act,
                               int* sfail) {
  const int tid = threadIdx.x;
  const CliqueDesc d = a.cl[s];
  const int nn = d.nn, nf = d.nn + d.na;
  double* Lp = a.L + d.blk;
  const int32_t* rows = a.rowidx + d.rows;
  for (int c0 = 0; c0 < nn; c0 += CU_CB) {
    const int cb = min(CU_CB, nn - c0);
    for (int e = tid; e < cb * cb; e += CU_NT) {
      const int c = e / cb, t = e - c * cb;
      if (t >= c) tri[c * (CU_CB + 1) + t] = Lp[(int64_t)(c0 + c) * nf + c0 + t];
    }
    for (int e = tid; e < kcp * cb; e += CU_NT) {
      const int jj = e / cb, t = e - jj * cb;
      wt[jj * CU_CB + t] = a.W[(int64_t)(m0 + jj) * a.ldw + d.first + c0 + t];
    }
    if (tid == 0) *sfail = 0;
    __syncthreads();
    // the triangle: thread t owns row c0 + t; every owner of a row at or below the diagonal repeats the chain of the diagonal
    for (int c = 0; c < cb; ++c) {
      if (tid >= c && tid < cb) {
        double dd = tri[c * (CU_CB + 1) + c];
        double lv = tri[c * (CU_CB + 1) + tid];
        int any = 0;
        for (int jj = 0; jj < kcp; ++jj) {
          const double x = wt[jj * CU_CB + c];
          double rc = 1.0, cc = 1.0, ss = 0.0;
          if (x != 0.0) {
            const double sg = (double)cols.sign[m0 + jj];
            const double t2 = sg > 0.0 ? fma(x, x, dd * dd) : (dd - x) * (dd + x);
            if (!(t2 > 0.0)) {
              if (tid == c && !*sfail) *sfail = 1 + cols.col[m0 + jj];
            } else {
              const double r = sqrt(t2);
              rc = dd / r; cc = r / dd; ss = x / dd;
              dd = r;
              any = 1;
              if (tid > c) {
                const double w = wt[jj * CU_CB + tid];
                lv = fma(sg * ss, w, lv) * rc;
                wt[jj * CU_CB + tid] = fma(-ss, lv, cc * w);
              }
            }
          }
          if (tid == c) {
            double* p = P + (c * CU_KC + jj) * 3;
            p[0] = rc; p[1] = cc; p[2] = ss;
          }
        }
        tri[c * (CU_CB + 1) + tid] = tid == c ? dd : lv;
        if (tid == c) act[c] = any;
      }
      __syncthreads();
    }
    const int fail = *sfail;
    if (fail) return fail;
    int anyact = 0;
    for (int c = 0; c < cb; ++c) anyact |= act[c];
    if (anyact) {
      for (int e = tid; e < cb * cb; e += CU_NT) {
        const int c = e / cb, t = e - c * cb;
        if (t >= c && act[c]) Lp[(int64_t)(c0 + c) * nf + c0 + t] = tri[c * (CU_CB + 1) + t];
      }
      // the rows below the block: a thread per row
      for (int i = c0 + cb + tid; i < nf; i += CU_NT) {
        const int r = i < nn ? d.first + i : rows[i];
        double* wr = a.W + (int64_t)m0 * a.ldw + r;
        double w[CU_KC];
#pragma unroll
        for (int jj = 0; jj < CU_KC; ++jj) w[jj] = jj < kcp ? wr[(int64_t)jj * a.ldw] : 0.0;
        for (int c = 0; c < cb; ++c) {
          if (!act[c]) continue;
          double* lp = Lp + (int64_t)(c0 + c) * nf + i;
          double l = *lp;
#pragma unroll
          for (int jj = 0; jj < CU_KC; ++jj) {
            if (jj >= kcp) continue;
            const double* p = P + (c * CU_KC + jj) * 3;
            const double ss = p[2];
            if (ss == 0.0) continue;
            l = fma((double)cols.sign[m0 + jj] * ss, w[jj], l) * p[0];
            w[jj] = fma(-ss, l, p[1] * w[jj]);
          }
          *lp = l;
        }
#pragma unroll
        for (int jj = 0; jj < CU_KC; ++jj) if (jj < kcp) wr[(int64_t)jj * a.ldw] = w[jj];
      }
    }
    __syncthreads();             // w of the rows below is in the workspace before the next block, or the parent, gathers it
  }
  return 0;
}

// grid (1), CU_NT threads
__global__ void __launch_bounds__(CU_NT) k_cu_walk(CuWalkArgs a, CuCols cols) {
  __shared__ double tri[CU_CB * (CU_CB + 1)], wt[CU_KC * CU_CB], P[CU_CB * CU_KC * 3];
  __shared__ int act[CU_CB];
  __shared__ unsigned long long mask[CU_NT / 64];
  __shared__ int sfail, sbad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nwords = (a.nsn + 3) >> 2;
  if (tid == 0) sbad = INT_MAX;
  __syncthreads();
  if (tid < a.k && a.flags[tid] != CU_OK) atomicMin(&sbad, tid);     // the first refused column, in the caller's numbering
  __syncthreads();
  const int bad = sbad;
  int fail = 0;
  if (bad == INT_MAX) {
    const int npass = (cols.nact + CU_KC - 1) / CU_KC;
    for (int p = 0; p < npass && !fail; ++p) {
      const int m0 = p * CU_KC, kcp = min(CU_KC, cols.nact - m0);
      for (int base = 0; base < a.nsn && !fail; base += CU_NT) {
        const int s = base + tid;
        const unsigned byte = s < a.nsn ? (a.visit[s >> 2] >> (8 * (s & 3))) & 0xffu : 0u;
        const unsigned long long b = __ballot((byte >> p) & 1u);
        if (lane == 0) mask[wave] = b;
        __syncthreads();
        for (int w = 0; w < CU_NT / 64 && !fail; ++w) {
          unsigned long long m = mask[w];
          while (m && !fail) {
            const int bit = __ffsll((long long)m) - 1;
            m &= m - 1;
            fail = cu_visit(a, cols, base + 64 * w + bit, m0, kcp, tri, wt, P, act, &sfail);
          }
        }
        __syncthreads();         // (mask is rewritten by the next chunk)
      }
    }
  }
  for (int w = tid; w < nwords; w += CU_NT) a.visit[w] = 0u;          // ready for the next call, whatever happened in this one
  if (tid == 0) {
    if (bad != INT_MAX) {
      a.status[0] = a.flags[bad] == CU_BAD_SUPPORT ? a.e_support : a.e_value;
      a.status[1] = bad;
    } else {
      a.status[0] = fail;
      a.status[1] = fail ? fail - 1 : 0;
    }
  }
}

}  // namespace smcp
