// Products of a chordal symmetric matrix with a dense block: C <- alpha X B + beta C for X stored on the pattern (blkval; of
// the N N block of a supernode only the lower triangle counts) and dense n x nrhs blocks B, C (column-major, rows in the
// permuted order).  Like the products with the factor (front_trmm.hip) there is no dependency along the clique tree, so a
// call is two or three launches whatever the tree; unlike them every stored entry X_ij serves TWO outputs, row i and row j,
// and the kernels here read it once for both.
//
// Clique k has columns N, front rows F = [N; A] (its rowidx list) and the nf x nn panel P (ld nf) at blkptr[k].  An ITEM is
// (k, r, p): the rows 64 r .. 64 r + 63 of the panel (a row chunk) and the columns p KP .. p KP + KP - 1, clipped to nn (a
// column part, KP = SYMM_KP).  With `last` the last panel row of the chunk, an item is listed when p KP <= last: otherwise
// all of it lies above the diagonal of the N N block.  An item has
//   a ROW partial for each of its rows m:  sum over the columns kk of the part of P[m, kk] B[N_kk, :] (for m < nn only
//     kk <= m: the diagonal is taken here), target row F_m of C;
//   a COLUMN partial for each column kk < last of its part:  sum over the rows m > kk of the chunk of P[m, kk] B[F_m, :],
//     target row N_kk of C.
// Every partial has one position in a list of ntot: row i of C owns the positions [tptr[i], tptr[i + 1]), its partials in
// ascending (k, side, r, p), side 0 = row partial, 1 = column partial (products.hip: symm_setup; specified by the numpy
// restatement of tests/symm_ref.py).  Phase 1 stores the value of the partial at position q for column c at U[q + c ntot]
// in the update workspace, so phase 2 reads no index but tptr:
//   C[i, c] = beta C[i, c] + alpha (the run of row i summed in ascending position),
// a thread per entry, a wave per entry with a fixed shuffle tree for the rows with more than SYMM_HEAVY partials.  A term
// whose factor is zero is left out, not multiplied by zero.  The order of every sum is fixed by an index: no atomics.
//
// The device list holds an item as (k, r, p, base): pos[base + j], j < rows of the chunk, is the position of the row
// partial of row 64 r + j, and pos[base + rows + j] that of the column partial of column p KP + j.
//
// k_symm_fma<CB>: plain FMA, one wave per item, four items per workgroup, lane = panel row, CB columns of B.  The panel
// streams coalesced in slabs of SYMM_SLAB columns whose loads are all issued up front at clamped indices.  The row partial
// is a register accumulator per lane; the entries of B it needs are loaded once by the wave, one per lane, and read from
// the lanes as wave-uniform operands (k_syr2k_fma).  For the column partials the wave stages the slab, masked to the rows
// strictly below the diagonal, in LDS with an odd leading dimension, next to its own 64 x CB values of B[F_m, :] (staged
// once per item); lane l then runs down a quarter (l >> 4) of column l & 15 and the quarters meet in two shuffles.
// k_symm_mm: 64 x 64 tiles on v_mfma_f64_16x16x4 (gemm_tile64), one workgroup per (item, 64 columns of B): the row
// partials accumulated over the column tiles of the part, then one product per column tile with the transposed,
// strictly-lower-masked loader.  gemm_tile64 is called once per product: the second read of a tile comes from L2.
#include <hip/hip_runtime.h>

namespace smcp {

struct SymmArgs {
  const CliqueDesc* cl;
  const int32_t* rowidx;
  const int32_t* items;    // (clique, row chunk, column part, base in pos) quadruples, the large fronts first
  int item0, nitems;       // the items [item0, item0 + nitems) of the list
  const int32_t* pos;
  const double* X;
  const double* B;
  double* U;               // update workspace: ntot x nrhs, ld ntot
  int64_t ntot;
  int nrhs;
  int64_t ldb;
};

constexpr int SYMM_WAVES = 4;        // items per workgroup of k_symm_fma
constexpr int SYMM_ROWS = 64;        // panel rows of an item
constexpr int SYMM_KP = 256;         // panel columns of an item (TRMM_SPLIT_NN: the width at which trmm had to split; not swept)
constexpr int SYMM_SLAB = 16;        // panel columns staged at a time by k_symm_fma
constexpr int SYMM_LDS = 65;         // leading dimension of the staged slab, in doubles: odd
constexpr int SYMM_HEAVY = 32;       // k_symm_combine: rows with more partials take a wave per entry (TRMM_HEAVY)
constexpr int SYMM_MM_ALL = 32;      // columns of B from which every front, not only the large ones, takes the tile products

#define SYMM_WAVE_FENCE() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                               __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

template <int CB>
__global__ void __launch_bounds__(64 * SYMM_WAVES) k_symm_fma(SymmArgs a) {
  constexpr int NG = (CB + 3) / 4;            // groups of four columns of B
  __shared__ double sS[SYMM_WAVES][SYMM_SLAB * SYMM_LDS];
  __shared__ double sB[SYMM_WAVES][64 * CB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int it = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SYMM_WAVES + wave));
  if (it >= a.nitems) return;
  const int4 item = reinterpret_cast<const int4*>(a.items)[a.item0 + it];
  const CliqueDesc d = a.cl[item.x];
  const int nn = d.nn, nf = nn + d.na;
  const int m0 = SYMM_ROWS * item.y, m = m0 + lane, mc = min(m, nf - 1);
  const int last = min(m0 + SYMM_ROWS, nf) - 1;
  const int j0 = SYMM_KP * item.z, j1 = min(nn, j0 + SYMM_KP);
  const int jend = min(j1, last + 1);         // columns with an entry that counts in this chunk
  const int jcol = min(j1, last);             // columns with a column partial
  const bool live = m < nf;
  const int c0 = blockIdx.y * CB, nc = min(CB, a.nrhs - c0);
  const double* P = a.X + d.blk + mc;
  const double* Bc = a.B + (int64_t)c0 * a.ldb;
  double* S = sS[wave];
  double* Bf = sB[wave];
  {                                           // the lane's own row of B, for the column partials: Bf[lane][c]
    const int64_t row = mc < nn ? (int64_t)d.first + mc : (int64_t)a.rowidx[d.rows + mc];
    double bf[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) bf[c] = Bc[row + (int64_t)min(c, nc - 1) * a.ldb];
#pragma unroll
    for (int c = 0; c < CB; ++c) Bf[lane * CB + c] = bf[c];
  }
  double acc[CB];
#pragma unroll
  for (int c = 0; c < CB; ++c) acc[c] = 0.0;
  const int col = lane & 15, q = lane >> 4;   // the column and the quarter of the rows this lane sums
  const int32_t* pos = a.pos + item.w;
  const int nrows = last - m0 + 1;
  for (int s0 = j0; s0 < jend; s0 += SYMM_SLAB) {
    double pv[SYMM_SLAB], cb[NG];
#pragma unroll
    for (int j = 0; j < SYMM_SLAB; ++j) pv[j] = P[(int64_t)min(s0 + j, nn - 1) * nf];
#pragma unroll
    for (int g = 0; g < NG; ++g)
      cb[g] = Bc[d.first + min(s0 + col, nn - 1) + (int64_t)min(4 * g + q, nc - 1) * a.ldb];
    SYMM_WAVE_FENCE();                        // (the reads of the previous slab are done; first slab: Bf is in place)
#pragma unroll
    for (int j = 0; j < SYMM_SLAB; ++j) {
      const int kk = s0 + j;
      S[j * SYMM_LDS + lane] = (live && kk < jend && m > kk) ? pv[j] : 0.0;
      if (kk < jend) {                        // (wave-uniform)
        const double x = (live && (m >= nn || kk <= m)) ? pv[j] : 0.0;
#pragma unroll
        for (int c = 0; c < CB; ++c) acc[c] = fma(x, syr2k_lane(cb[c >> 2], 16 * (c & 3) + j), acc[c]);
      }
    }
    SYMM_WAVE_FENCE();
    double cs[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) cs[c] = 0.0;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const double x = S[col * SYMM_LDS + 16 * q + t];
#pragma unroll
      for (int c = 0; c < CB; ++c) cs[c] = fma(x, Bf[(16 * q + t) * CB + c], cs[c]);
    }
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      cs[c] += __shfl_xor(cs[c], 16, 64);
      cs[c] += __shfl_xor(cs[c], 32, 64);
    }
    if (q == 0 && s0 + col < jcol) {
      double* Up = a.U + pos[nrows + (s0 + col - j0)] + (int64_t)c0 * a.ntot;
#pragma unroll
      for (int c = 0; c < CB; ++c) if (c < nc) Up[(int64_t)c * a.ntot] = cs[c];
    }
  }
  if (live) {
    double* Up = a.U + pos[lane] + (int64_t)c0 * a.ntot;
#pragma unroll
    for (int c = 0; c < CB; ++c) if (c < nc) Up[(int64_t)c * a.ntot] = acc[c];
  }
}

// tile products: one workgroup per (item, 64 columns of B)
__global__ void __launch_bounds__(256, 4) k_symm_mm(SymmArgs a) {
  __shared__ double sA[LKC * LSA], sB[LT * LSB];
  const int4 item = reinterpret_cast<const int4*>(a.items)[a.item0 + blockIdx.x];
  const CliqueDesc d = a.cl[item.x];
  const int nn = d.nn, nf = nn + d.na;
  const int m0 = SYMM_ROWS * item.y, n0 = blockIdx.y * LT;
  const int mend = min(m0 + SYMM_ROWS, nf), last = mend - 1;
  const int j0 = SYMM_KP * item.z, j1 = min(nn, j0 + SYMM_KP);
  const int jend = min(j1, last + 1), jcol = min(j1, last);
  const double* P = a.X + d.blk;
  const double* Bc = a.B;
  const int32_t* rows = a.rowidx + d.rows;
  const int32_t* pos = a.pos + item.w;
  const int64_t ldb = a.ldb, ntot = a.ntot;
  const int first = d.first, nrhs = a.nrhs, nrows = mend - m0;
  double* Uw = a.U;
  d4 acc[2][2];
  tile64_zero(acc);
  // row partials: P[chunk, part] B[N_part, :], of the N N block the lower triangle with its diagonal
  gemm_tile64(acc, mend, nrhs, jend, m0, n0, [=](int m, int kk) { return (m >= nn || kk <= m) ? P[m + (int64_t)kk * nf] : 0.0; },
              [=](int kk, int n) { return Bc[first + kk + (int64_t)n * ldb]; }, sA, sB, j0);
  tile64_foreach(acc, m0, n0, mend, nrhs, [=](int m, int n, double v) { Uw[pos[m - m0] + (int64_t)n * ntot] = v; });
  // column partials: P[chunk, column tile]^T B[F_chunk, :], the rows strictly below the diagonal
  for (int t0 = j0; t0 < jcol; t0 += LT) {
    tile64_zero(acc);
    gemm_tile64(acc, jcol, nrhs, mend, t0, n0, [=](int j, int m) { return m > j ? P[m + (int64_t)j * nf] : 0.0; },
                [=](int m, int n) { return Bc[(m < nn ? first + m : rows[m]) + (int64_t)n * ldb]; }, sA, sB, m0);
    tile64_foreach(acc, t0, n0, jcol, nrhs, [=](int j, int n, double v) { Uw[pos[nrows + (j - j0)] + (int64_t)n * ntot] = v; });
  }
}

// phase 2: row i sums the run [tptr[i], tptr[i + 1]) of every column of the update workspace (ld ntot) in ascending
// position and C = beta C + alpha sum, a term with a zero factor left out (alpha == 0: U is not read; beta == 0: C is
// not).  Workgroups [0, light): one thread per entry of C (rows with more than SYMM_HEAVY partials left out); the others:
// one wave per entry of the nheavy rows of `heavy`.
__global__ void __launch_bounds__(256) k_symm_combine(const int64_t* tptr, const int32_t* heavy, int nheavy, int light, const double* U,
                                                      int64_t ntot, double* C, int64_t n, int nrhs, int64_t ldc, double alpha, double beta) {
  if ((int)blockIdx.x < light) {
    const int64_t tot = n * nrhs;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (int64_t)light * blockDim.x) {
      const int64_t i = e % n, c = e / n;
      double v = 0.0;
      if (alpha != 0.0) {
        const int64_t pb = tptr[i], pe = tptr[i + 1];
        if (pe - pb > SYMM_HEAVY) continue;
        const double* Uc = U + c * ntot;
        for (int64_t p = pb; p < pe; ++p) v += Uc[p];
      }
      double* Cp = C + i + c * ldc;
      *Cp = syr2k_combine(beta != 0.0 ? *Cp : 0.0, v, alpha, beta);
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
    if (lane == 0) {
      double* Cp = C + i + c * ldc;
      *Cp = syr2k_combine(beta != 0.0 ? *Cp : 0.0, v, alpha, beta);
    }
  }
}

}  // namespace smcp
