// ---------------------------------------------------------------------------------------------
// Fronts of at most TOP_MAXROWS rows: the Cholesky of one front in ONE workgroup with the front held in REGISTERS
// (k_top_chol).  k_mid_chol (front_large.hip) works on one 64-column block column in LDS and updates everything to its
// right -- the other block columns and the update block -- in global memory, a read-modify-write through L2 from a single
// CU after every block column; the triangular inverse the scaling point needs next was five more launches
// (k_lf_diag_inv, 4 x k_lf_trtri), although wave_potrf_inv16 had already produced every 16 x 16 diagonal inverse they start from.
//
// Here the lower triangle of the front [panel | update block], in 16 x 16 tiles, is dealt cyclically over fifteen TILE
// waves (tile t = i (i + 1) / 2 + j  ->  wave t % 15, slot t / 15) and stays in the accumulator layout of v_mfma_f64_16x16x4
// (lane (l15, kq), register q <-> entry (l15, kq + 4 q)) from the one load to the one store.  The sixteenth wave holds no
// tile: it runs wave_potrf_inv16, which needs most of the 128 registers a wave of a 1024-thread workgroup has (with the
// routine on the tile's owner the compiler reported 212 spilled registers, 133 with the owner's tiles parked in LDS by
// hand; this way none).  Column step r:
//   A1 the owner of (r, r) applies the previous step's update to it and puts it to LDS                            -- barrier
//   A2 the factor wave factors and inverts it there; the tile waves apply the previous step's update to the rest   -- barrier
//   B  the owners of (i, r), i > r, multiply by the transposed block inverse (4 MFMAs), write the tile to the LDS panel
//      buffer and to L                                                                                             -- barrier
// and the update T(i, j) -= P_i P_j^T takes both operands from the panel buffer: no global traffic inside the loop.
// A partial last column tile (nn not a multiple of 16) holds panel columns and update-block columns side by side: the rows
// of tile (r, r) beyond the bw x bw block are rows below as well, and the last update then covers tile column r too (its
// panel columns receive zeros: rows < bw of P_r are zero).
// INV: Li = L_NN^-1 goes to LK (the layout of k_lf_diag_inv / k_lf_trtri: zeros above the diagonal) after the factorisation,
// one wave per tile column c by forward substitution down the column, X_rc = -D_r^-1 sum_{c <= k < r} L_rk X_kc, from
// the L tiles just written and the block inverses kept in LDS; the columns do not depend on each other.  The wave works on
// the transposes Z = X^T: in the accumulator layout a tile is at once the A operand of the next product, so a finished tile goes
// from the registers straight into the sums of the tile rows below it and is never read back.
// ---------------------------------------------------------------------------------------------
#pragma once

namespace smcp {

constexpr int TOP_MAXT = 13;                                               // tiles per side
constexpr int TOP_MAXROWS = 16 * TOP_MAXT;                                 // 208: the root of synth50k
constexpr int TOP_TW = 15;                                                 // tile waves (wave 15 factors the diagonal tiles)
constexpr int TOP_SLOTS = (TOP_MAXT * (TOP_MAXT + 1) / 2 + TOP_TW - 1) / TOP_TW;   // tiles per tile wave

#define TOP_WAVE_FENCE() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

template <bool INV>
__global__ void __launch_bounds__(1024) k_top_chol(MfmaArgs a, double* x, double* LK) {
  __shared__ __attribute__((aligned(16))) double s_d[256];                 // the diagonal tile being factored
  __shared__ __attribute__((aligned(16))) double s_inv[TOP_MAXT * 256];    // block inverses, X(n, k) at [n + 16 k]
  __shared__ __attribute__((aligned(16))) double s_pan[TOP_MAXT * 256];    // panel of the step, tile i at 256 i, P(m, k) at [m + 16 k]
  __shared__ int s_fail;
  const int k = a.t.lev[blockIdx.x];
  if (*info_of(a.t, k)) return;
  const CliqueDesc d = a.t.cl[k];
  const int nn = d.nn, na = d.na, nf = nn + na;
  if (nf > TOP_MAXROWS) return;                                            // (the host routes such fronts to k_mid_chol)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, kq = lane >> 4;
  const int nt = (nf + 15) >> 4, nct = (nn + 15) >> 4, ntile = nt * (nt + 1) / 2;
  double* const P = x + d.blk;                                             // nf x nn, ld nf
  if (tid == 0) s_fail = 0;
  __syncthreads();

  if (wave == TOP_TW) {
    // ---- the factor wave: same barriers as the tile waves below
    for (int r = 0; r < nct; ++r) {
      __syncthreads();
      const bool ok = wave_potrf_inv16(s_d, 16, min(16, nn - 16 * r), s_inv + 256 * r);
      if (!ok && lane == 0) s_fail = 1;
      __syncthreads();
      if (!ok) { if (lane == 0) atomicCAS(info_of(a.t, k), 0, info_val(a.t, k)); return; }
      __syncthreads();
    }
  } else {
    // ---- the wave's tiles
    const double* const U = a.t.upd + d.upd;                               // na x na, ld na (lower triangle assembled)
    // (addresses: a wave-uniform part that stays in scalar registers + ONE per-lane offset for the panel, one for the update block
    // -- per-slot 64-bit lane addresses are loop invariants the compiler hoists out of the column loop and then spills)
    unsigned vo[4], vu[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { vo[q] = l15 + (kq + 4 * q) * nf; vu[q] = l15 + (kq + 4 * q) * na; }
    int ti[TOP_SLOTS], tj[TOP_SLOTS];
    bool valid[TOP_SLOTS];
    d4 T[TOP_SLOTS];
#pragma unroll
    for (int s = 0; s < TOP_SLOTS; ++s) {
      const int t = TOP_TW * s + wave;
      int i = 0;
      while ((i + 1) * (i + 2) / 2 <= t) ++i;
      ti[s] = i; tj[s] = t - i * (i + 1) / 2;
      valid[s] = t < ntile;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = 16 * i + l15, col = 16 * tj[s] + kq + 4 * q;
        // (every lane loads -- the padding lanes the front's first entry -- and selects afterwards: a load under a per-lane
        // branch is waited for before the next one is issued, 28 round trips one after the other)
        const bool ok = valid[s] && row < nf && col <= row;
        const double* src = !ok ? P : (col < nn ? &(P + (16 * i + 16 * tj[s] * nf))[vo[q]] : &(U + ((16 * i - nn) + (16 * tj[s] - nn) * na))[vu[q]]);
        const double v = *src;
        T[s][q] = ok ? v : 0.0;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // T(i, j) -= P_i P_j^T, both operands from the panel buffer
    auto update = [&](d4& t, int i, int j) {
      const double* Pi = s_pan + 256 * i;
      const double* Pj = s_pan + 256 * j;
#pragma unroll
      for (int q = 0; q < 4; ++q) t = __builtin_amdgcn_mfma_f64_16x16x4f64(Pj[l15 + 16 * (4 * q + kq)], -Pi[l15 + 16 * (4 * q + kq)], t, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);      // (one tile's operands in flight at a time: scheduled side by side the slots' loads spill)
    };
    for (int r = 0; r < nct; ++r) {
      const int bw = min(16, nn - 16 * r);
      const bool part = bw < 16;
      // ---- A1: the diagonal tile first
#pragma unroll
      for (int s = 0; s < TOP_SLOTS; ++s)
        if (valid[s] && ti[s] == r && tj[s] == r) {
          if (r > 0) update(T[s], r, r);
#pragma unroll
          for (int q = 0; q < 4; ++q) s_d[l15 + 16 * (kq + 4 * q)] = T[s][q];
        }
      __syncthreads();
      // ---- A2: the rest of the previous step's update beside the factor wave
      if (r > 0) {
#pragma unroll
        for (int s = 0; s < TOP_SLOTS; ++s)
          if (valid[s] && tj[s] >= r && ti[s] > r) update(T[s], ti[s], tj[s]);
      }
      __syncthreads();
      if (s_fail) return;
      // ---- B: the factored block comes back and goes to L; rows below x the block's inverse (transposed) -> panel buffer, L
      int l15b = l15, kqb = kq;      // (as for the last update below)
      asm volatile("" : "+v"(l15b), "+v"(kqb));
      const double* Xr = s_inv + 256 * r;
#pragma unroll
      for (int s = 0; s < TOP_SLOTS; ++s) {
        if (!valid[s] || tj[s] != r) continue;
        const bool diag = ti[s] == r;
        if (diag) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int col = kqb + 4 * q;
            if (l15b < bw && col <= l15b) {
              T[s][q] = s_d[l15b + 16 * col];
              (P + (16 * r + 16 * r * nf))[vo[q]] = T[s][q];
            }
          }
          if (!part) continue;
        }
        d4 p = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // (a partial tile: its columns beyond bw belong to the update block and meet zeros of the inverse -- masked, a stray
          // NaN times zero would still be a NaN)
          const double av = (!part || 4 * q + kqb < bw) ? T[s][q] : 0.0;
          p = __builtin_amdgcn_mfma_f64_16x16x4f64(Xr[l15b + 16 * (4 * q + kqb)], av, p, 0, 0, 0);
        }
        double* Ps = s_pan + 256 * ti[s];
        const int row = 16 * ti[s] + l15b;
        const bool below = !diag || l15b >= bw;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int col = kqb + 4 * q;
          const double v = below ? p[q] : 0.0;
          Ps[l15b + 16 * col] = v;
          if (below && col < bw) {
            T[s][q] = v;
            if (row < nf) (P + (16 * ti[s] + 16 * r * nf))[vo[q]] = v;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
    }
    // ---- the last step's update: what remains is the update block, published once as packed lower triangle
    if (na > 0) {
      const int j0 = (nn & 15) ? nct - 1 : nct;
      double* UP = a.t.updp + d.updp;
      // (lane coordinates the optimiser cannot tie to those of the load above: shared, the loads' per-lane predicates and
      // offsets stay live through the column loop and the kernel spills)
      int l15f = l15, kqf = kq;
      asm volatile("" : "+v"(l15f), "+v"(kqf));
#pragma unroll
      for (int s = 0; s < TOP_SLOTS; ++s) {
        if (!valid[s] || tj[s] < j0) continue;
        update(T[s], ti[s], tj[s]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = 16 * ti[s] + l15f, col = 16 * tj[s] + kqf + 4 * q;
          if (row < nf && col >= nn && col <= row) UP[pk_idx(row - nn, col - nn, na)] = T[s][q];
        }
      }
    }
  }
  if (!INV) return;
  // ---- Li = L_NN^-1 by tile columns (L and the block inverses are complete: the loop ended with a barrier)
  for (int c = wave; c < nct; c += 16) {
    const int cw = min(16, nn - 16 * c);
    double* Xc = LK + d.blk + (int64_t)(16 * c) * nf;           // columns 16 c .. of Li: X(row, 16 c + m) at Xc[row + m nf]
    const bool mok = l15 < cw;
    for (int e = lane; e < 16 * c * cw; e += 64) Xc[e % (16 * c) + (int64_t)(e / (16 * c)) * nf] = 0.0;
    d4 z;                                                       // Z(m, n) = X(16 r + n, 16 c + m) of the newest tile row r
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = kq + 4 * q;
      z[q] = n >= l15 ? s_inv[256 * c + n + 16 * l15] : 0.0;
      if (mok && n < cw) Xc[(16 * c + n) + (int64_t)l15 * nf] = z[q];
    }
    // right-looking: as soon as Z of tile row kt is final it goes -- from the registers, as the A operand -- into the sums S of all
    // the tile rows below, whose L operands do not depend on the chain and can be in flight ahead of it; the chain itself is one
    // such product and the product with the block inverse per tile row.  (Left-looking, Z_rc = sum over ALL earlier tile rows read
    // back from LK, was up to eleven dependent round trips to L2 per tile row: 70 us for the root of synth50k.)
    const double* __restrict__ Lp = P;
    double* __restrict__ Xw = Xc;
    const bool lastok = 16 * (nct - 1) + l15 < nn;
    const unsigned lo = l15 + kq * nf, lo_last = (lastok ? l15 : 0) + kq * nf;
    d4 S[TOP_MAXT - 1];                                         // S[j] <-> tile row c + 1 + j
#pragma unroll
    for (int j = 0; j < TOP_MAXT - 1; ++j) S[j] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < TOP_MAXT - 1; ++ks) {
      const int kt = c + ks;
      if (kt + 1 < nct) {           // (guards, not breaks: the loops must unroll for S to stay in registers)
#pragma unroll
        for (int j = ks; j < TOP_MAXT - 1; ++j) {
          // (no branch per product -- its loads would be waited for one product at a time: tile rows beyond the front's take the
          // last row's address and a zero operand.  Rows beyond nn, in the last tile row only, are separator rows: masked, such a
          // lane loads row 16 r.  Scalar base + one of two per-lane offsets: no 64-bit lane addresses)
          const int r = min(c + 1 + j, nct - 1);
          const bool last = r == nct - 1;
          const bool rok = c + 1 + j < nct && (!last || lastok);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double b0 = (Lp + (16 * r + (16 * kt + 4 * q) * nf))[last ? lo_last : lo];
            S[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(rok ? b0 : 0.0, z[q], S[j], 0, 0, 0);
          }
        }
        const int r = kt + 1, rw = min(16, nn - 16 * r);
        d4 zn = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 4; ++q) zn = __builtin_amdgcn_mfma_f64_16x16x4f64(s_inv[256 * r + l15 + 16 * (4 * q + kq)], S[ks][q], zn, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = kq + 4 * q;
          z[q] = -zn[q];
          if (mok && n < rw) Xw[(16 * r + n) + (int64_t)l15 * nf] = z[q];
        }
      }
    }
  }
}
#undef TOP_WAVE_FENCE

}  // namespace smcp
