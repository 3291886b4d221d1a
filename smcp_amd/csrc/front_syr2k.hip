// Symmetric rank-2k updates projected on the chordal pattern (chompack.syr2 for a block of k columns):
//   X <- beta X + alpha P_V(U V^T + V U^T)    (syr2k)        X <- beta X + alpha P_V(U U^T)    (syrk: V absent)
// U and V are dense n x k blocks (column-major, rows in the permuted order).  For clique c with columns N, front rows
// F = [N; A] (its rowidx list) and the panel (nf x nn, ld nf) at blkptr[c]
//   panel[m, j] = beta panel[m, j] + alpha sum_r (U[F_m, r] V[N_j, r] + V[F_m, r] U[N_j, r]),   r ascending,
// on the rows m >= j of the N N part and all rows of the A N part.  Every entry of blkval belongs to one clique: no
// dependency along the tree, no reduction across cliques, no atomics -- one launch per route, two when a call uses both.
// The slots of blkval outside the pattern (the strict upper triangles of the N N blocks) are never read and are stored as
// exactly 0.0; X is read once (not at all for beta == 0) and written once; U and V are read only when alpha != 0.
//
// k_syr2k_fma: plain FMA, one wave per item (clique, 64 panel rows, SYR2K_JC panel columns), four items per workgroup,
// lanes along the rows of a panel column (X streams coalesced).  A lane gathers the U / V values of its own row once
// through rowidx, RB <= 8 ranks at a time, into registers; the values of the column are wave-uniform (loaded once by the wave,
// one per lane, and read from the lanes).  Any front size and
// any k: the whole tree on the generic / deterministic route and at small k.  The column chunk is capped, so a 4096-wide
// front is thousands of items and not 64 waves walking 4096 columns each (front_trmm.hip, TRMM_SPLIT_NN, needed a
// reduction for that; here the outputs are disjoint).
// k_syr2k_mm: 64 x 64 tiles on v_mfma_f64_16x16x4 (gemm_tile64) over a host-built list of (clique, row tile, column
// tile), the tiles of the large fronts first.  syr2k runs ONE product over the inner dimension 2k with concatenated
// operands, A(m, kk) = kk < k ? U[F_m, kk] : V[F_m, kk - k], B(kk, j) = kk < k ? V[N_j, kk] : U[N_j, kk - k]; syrk runs
// over k.
// An item or tile whose rows all lie above the diagonal of the N N block is listed with its `zero` flag set: it reads
// nothing, computes nothing and stores the zeros the contract asks for.
#include <hip/hip_runtime.h>

namespace smcp {

struct Syr2kArgs {
  const CliqueDesc* cl;
  const int32_t* rowidx;
  const int32_t* items;    // k_syr2k_fma: (clique, row chunk, column chunk, zero) quadruples
  int nitems;
  const int32_t* tiles;    // k_syr2k_mm: (clique, row tile, column tile, zero) quadruples
  double* X;
  const double* U;
  const double* V;         // syrk: not read
  int k;
  int64_t ldu, ldv;
  double alpha, beta;
};

constexpr int SYR2K_WAVES = 4;       // items per workgroup
constexpr int SYR2K_JC = 16;         // panel columns per item of k_syr2k_fma
constexpr int SYR2K_MM_LARGE = 8;    // ranks from which the large fronts take the tile products
constexpr int SYR2K_MM_ALL = 32;     // ranks from which every front does

// beta x + alpha s, a term left out (not multiplied by zero) when its factor is zero: NaN / Inf behind a zero factor
// do not propagate, and alpha == 0, beta == 1 returns x bit for bit
__device__ inline double syr2k_combine(double x, double s, double alpha, double beta) {
  if (alpha != 0.0 && beta != 0.0) return fma(alpha, s, beta * x);
  if (alpha != 0.0) return alpha * s;
  if (beta != 0.0) return beta * x;
  return 0.0;
}

// the value lane `l` (a constant) holds, as a wave-uniform operand
__device__ inline double syr2k_lane(double x, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

// Rows [64 chunk, 64 chunk + 64) x columns [JC cchunk, JC cchunk + JC) of the panel of one clique; lane = panel row.  Per
// block of RB ranks every load is issued up front and unconditionally, at indices clamped into the operands: the lane's own
// U / V values, and the column's values spread over the wave (lane l: column l & 15, rank l >> 4 of each group of four),
// from where the products take them as wave-uniform operands.  No lane leaves before the end: all 64 hold column values.
template <int RB, bool TWO>
__global__ void __launch_bounds__(64 * SYR2K_WAVES) k_syr2k_fma(Syr2kArgs a) {
  constexpr int NG = (RB + 3) / 4;            // groups of four ranks
  const int lane = threadIdx.x & 63;
  const int it = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SYR2K_WAVES + (threadIdx.x >> 6)));
  if (it >= a.nitems) return;
  const int4 item = reinterpret_cast<const int4*>(a.items)[it];
  const CliqueDesc d = a.cl[item.x];
  const int nn = d.nn, nf = nn + d.na;
  const int m = 64 * item.y + lane, j0 = SYR2K_JC * item.z;
  const int nj = min(SYR2K_JC, nn - j0);
  const bool live = m < nf;
  const int mc = min(m, nf - 1);
  double* P = a.X + d.blk + mc + (int64_t)j0 * nf;
  if (item.w) {                               // every row of the chunk lies above the diagonal
    if (live)
      for (int jj = 0; jj < nj; ++jj) P[(int64_t)jj * nf] = 0.0;
    return;
  }
  const bool rd = a.beta != 0.0;
  double x[SYR2K_JC], acc[SYR2K_JC];
#pragma unroll
  for (int jj = 0; jj < SYR2K_JC; ++jj) {
    x[jj] = (rd && live && jj < nj && m >= j0 + jj) ? P[(int64_t)jj * nf] : 0.0;
    acc[jj] = 0.0;
  }
  if (a.alpha != 0.0) {
    const int k = a.k;
    const int64_t ldu = a.ldu, ldv = TWO ? a.ldv : a.ldu;
    const int64_t row = mc < nn ? (int64_t)d.first + mc : (int64_t)a.rowidx[d.rows + mc];
    const double* Ur = a.U + row;
    const double* Vr = (TWO ? a.V : a.U) + row;
    const double* Uc = a.U + d.first + j0 + min(lane & 15, nj - 1);
    const double* Vc = (TWO ? a.V : a.U) + d.first + j0 + min(lane & 15, nj - 1);
    for (int r0 = 0; r0 < k; r0 += RB) {
      double u[RB], v[RB], cu[NG], cv[NG];
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int rr = min(r0 + r, k - 1);
        u[r] = Ur[(int64_t)rr * ldu];
        if (TWO) v[r] = Vr[(int64_t)rr * ldv];
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int rr = min(r0 + 4 * g + (lane >> 4), k - 1);
        cu[g] = Uc[(int64_t)rr * ldu];
        if (TWO) cv[g] = Vc[(int64_t)rr * ldv];
      }
#pragma unroll
      for (int jj = 0; jj < SYR2K_JC; ++jj) {
        if (jj < nj) {
          double s = acc[jj];
#pragma unroll
          for (int r = 0; r < RB; ++r) {
            if (r0 + r < k) {                 // (wave-uniform: a rank past the last one is left out, not multiplied by zero)
              const int src = 16 * (r & 3) + jj;
              if (TWO) {
                s = fma(u[r], syr2k_lane(cv[r >> 2], src), s);
                s = fma(v[r], syr2k_lane(cu[r >> 2], src), s);
              } else {
                s = fma(u[r], syr2k_lane(cu[r >> 2], src), s);
              }
            }
          }
          acc[jj] = s;
        }
      }
    }
  }
#pragma unroll
  for (int jj = 0; jj < SYR2K_JC; ++jj)
    if (live && jj < nj) P[(int64_t)jj * nf] = (m >= j0 + jj) ? syr2k_combine(x[jj], acc[jj], a.alpha, a.beta) : 0.0;
}

template <bool TWO>
__global__ void __launch_bounds__(256, 4) k_syr2k_mm(Syr2kArgs a) {
  __shared__ double sA[LKC * LSA], sB[LT * LSB];
  const int4 t = reinterpret_cast<const int4*>(a.tiles)[blockIdx.x];
  const CliqueDesc d = a.cl[t.x];
  const int nn = d.nn, nf = nn + d.na;
  const int m0 = t.y * LT, n0 = t.z * LT;
  double* P = a.X + d.blk;
  if (t.w) {                                  // a tile strictly above the diagonal
    for (int e = threadIdx.x; e < LT * LT; e += 256) {
      const int m = m0 + (e & 63), n = n0 + (e >> 6);
      if (m < nf && n < nn) P[m + (int64_t)n * nf] = 0.0;
    }
    return;
  }
  d4 acc[2][2];
  tile64_zero(acc);
  const double alpha = a.alpha, beta = a.beta;
  if (alpha != 0.0) {
    const int k = a.k, first = d.first;
    const int32_t* rows = a.rowidx + d.rows;
    const double* U = a.U;
    const double* V = a.V;
    const int64_t ldu = a.ldu, ldv = a.ldv;
    if constexpr (TWO) {
      gemm_tile64(acc, nf, nn, 2 * k, m0, n0,
                  [=](int m, int kk) { const int64_t r = m < nn ? first + m : rows[m]; return kk < k ? U[r + (int64_t)kk * ldu] : V[r + (int64_t)(kk - k) * ldv]; },
                  [=](int kk, int n) { return kk < k ? V[first + n + (int64_t)kk * ldv] : U[first + n + (int64_t)(kk - k) * ldu]; }, sA, sB);
    } else {
      gemm_tile64(acc, nf, nn, k, m0, n0,
                  [=](int m, int kk) { return U[(m < nn ? first + m : rows[m]) + (int64_t)kk * ldu]; },
                  [=](int kk, int n) { return U[first + n + (int64_t)kk * ldu]; }, sA, sB);
    }
  }
  // (the load of an element above the diagonal is redirected to the owned slot (n, n) of its column and not used)
  tile64_rmw(acc, m0, n0, nf, nn, [=](int m, int n) { return beta != 0.0 ? P[max(m, n) + (int64_t)n * nf] : 0.0; },
             [=](int m, int n, double v, double old) { P[m + (int64_t)n * nf] = (m >= n) ? syr2k_combine(old, v, alpha, beta) : 0.0; });
}

}  // namespace smcp
