// Products with the supernodal Cholesky factor (chompack.trmm): B <- alpha L B or alpha L^T B for a dense n x nrhs block B
// (column-major, rows in the permuted order).  A product has no dependency chain along the clique tree once it is written
// in two phases, so a call is two or three launches whatever the depth of the tree:
//
//   phase 1, products (every clique at once; reads B, never writes it).  Clique k with columns N, separator rows A and
//   panel [L_NN; L_AN] (nf x nn, ld nf):
//     N:  X_N = L_NN B_N  (lower triangle of L_NN only)  -> X, a scratch image of B
//         U_k = L_AN B_N  (na x nrhs)                    -> update workspace, entry (q, c) at pos[sepptr[k] + q] + c ntot
//     T:  X_N = L_NN^T B_N + L_AN^T B[A]                 -> X (a pure gather through rowidx)
//   phase 2, combine:
//     N:  B[i, c] = alpha (X[i, c] + sum U_k[q, c]) over the separator entries (k, q) with rowidx = i, in ascending k.  The
//         host lays the transposed separator index out once per context (products.hip: trmm_setup): row i owns the positions
//         [tptr[i], tptr[i + 1]) of a list of all ntot = sepptr[nsn] separator entries, its own in ascending k, and
//         pos[sepptr[k] + q] is the position of entry (k, q).  Phase 1 stores U_k through pos, so the contributions to one
//         entry of B are CONTIGUOUS in the workspace, already in the order of the sum: the combine pass reads no index but
//         tptr.  One thread per entry of B walks its run; a row with more than TRMM_HEAVY contributors (a row of a top front
//         is in the separator of every clique below it: thousands on a wide tree) gets a wave per entry instead, lane l
//         taking positions l, l + 64, ... and the lanes meeting in a fixed shuffle tree.  Either way the order of the sum
//         is fixed by the index alone: the result is deterministic, and there are no floating-point atomics on any route.
//     T:  B = alpha X
//
// Two kernels form the products.  k_trmm_n / k_trmm_t: plain FMA, one wave per item (64 panel rows of a clique for N, four
// panel columns for T), four items per workgroup, lanes along the rows of a panel column (coalesced; every entry of L is
// read once per block of CB <= 8 columns of B).  They take any front size: the whole tree on the generic / deterministic
// route and for fewer than eight columns.  The row chunks of a wide supernode (nn >= TRMM_SPLIT_NN) are items of a whole
// workgroup in k_trmm_n: its four waves share the k range and meet in LDS in a fixed order (64 waves cannot pull a
// 4096-row front through at memory speed).  k_trmm_mm: 64 x 64 tiles on v_mfma_f64_16x16x4 (gemm_tile64) over
// (row tile of a front, column tile), the row tiles listed by the host, those of the large fronts first: the large fronts
// when B has at least eight columns, every front from TRMM_MM_ALL columns on.
#include <hip/hip_runtime.h>

namespace smcp {

struct TrmmArgs {
  const CliqueDesc* cl;
  const int32_t* rowidx;
  const int32_t* items;    // k_trmm_n / k_trmm_t: (clique, chunk) pairs
  int nitems;
  const int32_t* tiles;    // k_trmm_mm: (clique, row tile) pairs
  const double* L;
  const double* B;         // phase 1 only reads B
  double* X;               // scratch image of B (ldb x nrhs)
  double* U;               // update workspace (N only): ntot x nrhs, ld ntot
  const int32_t* pos;      // separator entry sepptr[k] + q -> its position in the transposed separator index
  int64_t ntot;
  int nrhs;
  int64_t ldb;
};

constexpr int TRMM_WAVES = 4;        // items per workgroup
constexpr int TRMM_JC = 4;           // panel columns per item of the transposed product
constexpr int TRMM_SPLIT_NN = 256;   // k_trmm_n: supernodes from this width on share the k range of a row chunk among the waves of a workgroup
constexpr int TRMM_HEAVY = 32;       // k_trmm_combine: rows with more contributors take a wave per entry
constexpr int TRMM_MM_ALL = 32;      // columns of B from which every front, not only the large ones, takes the tile products
// item code of k_trmm_n: chunk | part << 20 | split << 30 (a split row chunk is four consecutive items, parts 0 .. 3, of ONE workgroup)
__host__ __device__ inline int trmm_code(int chunk, int part, int split) { return chunk | part << 20 | split << 30; }

// N: rows [64 chunk, 64 chunk + 64) of the panel of one clique times CB columns of B; lane = panel row.  Items whose
// clique is -1 pad a group of unsplit items to a whole workgroup.
template <int CB>
__global__ void __launch_bounds__(64 * TRMM_WAVES) k_trmm_n(TrmmArgs a) {
  __shared__ double red[(TRMM_WAVES - 1) * CB * 64];
  const int lane = threadIdx.x & 63;
  const int it = blockIdx.x * TRMM_WAVES + (threadIdx.x >> 6);
  if (it >= a.nitems) return;
  const int k = a.items[2 * it], code = a.items[2 * it + 1];
  if (k < 0) return;                          // (never in a workgroup of split items: no barrier is left waiting)
  const int split = code >> 30, part = (code >> 20) & 1023, m0 = 64 * (code & 0xFFFFF);
  const CliqueDesc d = a.cl[k];
  const int nn = d.nn, nf = nn + d.na;
  const int m = m0 + lane;
  const int c0 = blockIdx.y * CB, nc = min(CB, a.nrhs - c0);
  const int kend = min(nn, m0 + 64);          // L_NN(m, kk) = 0 for kk > m
  const int kpart = (kend + TRMM_WAVES - 1) / TRMM_WAVES;
  const int k0 = split ? min(kend, part * kpart) : 0, k1 = split ? min(kend, k0 + kpart) : kend;
  const double* Lp = a.L + d.blk + min(m, nf - 1);
  const double* Bp = a.B + d.first + (int64_t)c0 * a.ldb;
  int64_t coff[CB];
#pragma unroll
  for (int c = 0; c < CB; ++c) coff[c] = (int64_t)min(c, nc - 1) * a.ldb;
  double acc[CB];
#pragma unroll
  for (int c = 0; c < CB; ++c) acc[c] = 0.0;
#pragma unroll 8
  for (int kk = k0; kk < k1; ++kk) {
    const double lv = Lp[(int64_t)kk * nf];
    const double l = (kk <= m) ? lv : 0.0;    // what is stored above the diagonal of L_NN is not part of L
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[c] = fma(l, Bp[kk + coff[c]], acc[c]);
  }
  if (split) {                                // workgroup-uniform: the four items of a split chunk share a workgroup
    if (part > 0) {
#pragma unroll
      for (int c = 0; c < CB; ++c) red[((part - 1) * CB + c) * 64 + lane] = acc[c];
    }
    __syncthreads();
    if (part > 0) return;
    for (int p = 0; p < TRMM_WAVES - 1; ++p)
#pragma unroll
      for (int c = 0; c < CB; ++c) acc[c] += red[(p * CB + c) * 64 + lane];
  }
  if (m >= nf) return;
  if (m < nn) {
    double* Xp = a.X + d.first + m + (int64_t)c0 * a.ldb;
#pragma unroll
    for (int c = 0; c < CB; ++c) if (c < nc) Xp[(int64_t)c * a.ldb] = acc[c];
  } else {
    double* Up = a.U + a.pos[d.rel + (m - nn)] + (int64_t)c0 * a.ntot;    // d.rel == sepptr[k]
#pragma unroll
    for (int c = 0; c < CB; ++c) if (c < nc) Up[(int64_t)c * a.ntot] = acc[c];
  }
}

// T: columns [JC chunk, JC chunk + JC) of the panel of one clique (entries of X_N) times CB columns of B; lanes run
// down the panel columns, each row's entries of B are fetched once for the JC columns, wave reduction in a fixed order
template <int CB>
__global__ void __launch_bounds__(64 * TRMM_WAVES) k_trmm_t(TrmmArgs a) {
  const int lane = threadIdx.x & 63;
  const int it = blockIdx.x * TRMM_WAVES + (threadIdx.x >> 6);
  if (it >= a.nitems) return;
  const int k = a.items[2 * it], j0 = TRMM_JC * a.items[2 * it + 1];
  const CliqueDesc d = a.cl[k];
  const int nn = d.nn, nf = nn + d.na;
  const int nj = min(TRMM_JC, nn - j0);
  const int c0 = blockIdx.y * CB, nc = min(CB, a.nrhs - c0);
  const int32_t* rows = a.rowidx + d.rows;
  const double* Lk = a.L + d.blk;
  const double* Bc = a.B + (int64_t)c0 * a.ldb;
  int64_t coff[CB];
#pragma unroll
  for (int c = 0; c < CB; ++c) coff[c] = (int64_t)min(c, nc - 1) * a.ldb;
  double acc[TRMM_JC][CB];
#pragma unroll
  for (int jj = 0; jj < TRMM_JC; ++jj)
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[jj][c] = 0.0;
  for (int mb = j0; mb < nf; mb += 64) {
    const int m = mb + lane, mc = min(m, nf - 1);
    const int64_t row = mc < nn ? (int64_t)d.first + mc : (int64_t)rows[mc];
    double bv[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) bv[c] = Bc[row + coff[c]];
#pragma unroll
    for (int jj = 0; jj < TRMM_JC; ++jj) {
      const int j = j0 + jj;
      const double lv = Lk[mc + (int64_t)min(j, nn - 1) * nf];
      const double l = (jj < nj && m >= j && m < nf) ? lv : 0.0;
#pragma unroll
      for (int c = 0; c < CB; ++c) acc[jj][c] = fma(l, bv[c], acc[jj][c]);
    }
  }
#pragma unroll
  for (int jj = 0; jj < TRMM_JC; ++jj)
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      double v = acc[jj][c];
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
      acc[jj][c] = v;
    }
  if (lane == 0) {
#pragma unroll
    for (int jj = 0; jj < TRMM_JC; ++jj)
#pragma unroll
      for (int c = 0; c < CB; ++c)
        if (jj < nj && c < nc) a.X[d.first + j0 + jj + (int64_t)(c0 + c) * a.ldb] = acc[jj][c];
  }
}

// tile products: one workgroup per (64 rows of the result of one front: an entry of the tile list, 64 columns of B)
template <bool TRANS>
__global__ void __launch_bounds__(256, 4) k_trmm_mm(TrmmArgs a) {
  __shared__ double sA[LKC * LSA], sB[LT * LSB];
  const CliqueDesc d = a.cl[a.tiles[2 * blockIdx.x]];
  const int nn = d.nn, nf = nn + d.na;
  const int m0 = a.tiles[2 * blockIdx.x + 1] * LT, n0 = blockIdx.y * LT;
  const double* Lk = a.L + d.blk;
  const double* Bc = a.B;
  const int64_t ldb = a.ldb;
  const int first = d.first, nrhs = a.nrhs;
  double* Xn = a.X + d.first;
  d4 acc[2][2];
  tile64_zero(acc);
  if constexpr (!TRANS) {
    const int kend = (m0 < nn) ? min(nn, m0 + LT) : nn;      // the k range of a row tile stops at its diagonal
    gemm_tile64(acc, nf, nrhs, kend, m0, n0, [=](int m, int kk) { return kk <= m ? Lk[m + (int64_t)kk * nf] : 0.0; },
                [=](int kk, int n) { return Bc[first + kk + (int64_t)n * ldb]; }, sA, sB);
    double* Uw = a.U;
    const int32_t* pos = a.pos + d.rel;
    const int64_t ntot = a.ntot;
    tile64_foreach(acc, m0, n0, nf, nrhs, [=](int m, int n, double v) {
      if (m < nn) Xn[m + (int64_t)n * ldb] = v;
      else Uw[pos[m - nn] + (int64_t)n * ntot] = v;
    });
  } else {
    const int32_t* rows = a.rowidx + d.rows;
    // [L_NN^T | L_AN^T](m, kk) = L[kk + m nf], zero for kk < m
    gemm_tile64(acc, nn, nrhs, nf, m0, n0, [=](int m, int kk) { return kk >= m ? Lk[kk + (int64_t)m * nf] : 0.0; },
                [=](int kk, int n) { return Bc[(kk < nn ? first + kk : rows[kk]) + (int64_t)n * ldb]; }, sA, sB, m0);
    tile64_foreach(acc, m0, n0, nn, nrhs, [=](int m, int n, double v) { Xn[m + (int64_t)n * ldb] = v; });
  }
}

// phase 2: row i sums the run [tptr[i], tptr[i + 1]) of every column of the update workspace (ld ntot) in ascending
// position; tptr null: B = alpha X.  Workgroups [0, light): one thread per entry of B (rows with more than TRMM_HEAVY
// contributors left out); the others: one wave per entry of the nheavy rows of `heavy`.
__global__ void __launch_bounds__(256) k_trmm_combine(const int64_t* tptr, const int32_t* heavy, int nheavy, int light, const double* X,
                                                      const double* U, int64_t ntot, double* B, int64_t n, int nrhs, int64_t ldb,
                                                      double alpha) {
  if ((int)blockIdx.x < light) {
    const int64_t tot = n * nrhs;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (int64_t)light * blockDim.x) {
      const int64_t i = e % n, c = e / n;
      double v = X[i + c * ldb];
      if (tptr) {
        const int64_t pb = tptr[i], pe = tptr[i + 1];
        if (pe - pb > TRMM_HEAVY) continue;
        const double* Uc = U + c * ntot;
        for (int64_t p = pb; p < pe; ++p) v += Uc[p];
      }
      B[i + c * ldb] = alpha * v;
    }
    return;
  }
  const int lane = threadIdx.x & 63;
  const int64_t tot = (int64_t)nheavy * nrhs, nw = (int64_t)(gridDim.x - light) * (blockDim.x >> 6);
  for (int64_t e = (int64_t)(blockIdx.x - light) * (blockDim.x >> 6) + (threadIdx.x >> 6); e < tot; e += nw) {
    const int64_t i = heavy[e % nheavy], c = e / nheavy;
    const int64_t pe = tptr[i + 1];
    const double* Uc = U + c * ntot;
    double v = 0.0;
    for (int64_t p = tptr[i] + lane; p < pe; p += 64) v += Uc[p];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    if (lane == 0) B[i + c * ldb] = alpha * (X[i + c * ldb] + v);
  }
}

}  // namespace smcp
