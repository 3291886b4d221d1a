// Cholesky of whole FAMILIES at the scaling point: one workgroup of four waves per family (a parent with nn <= 16, na <= 64 and its
// 1 .. 8 childless children with nn <= 16, 1 <= na <= 32), every family of the level resident at once.  The per-level route
// (k_chol_mfma<true, true> on the leaves, then on their parents) sends every child's packed update block through HBM -- written
// by the first launch, read by the second, by nobody else -- and is two dependent launches of gather / potrf_inv16 / small MFMA
// products / store.  Here
//   * the four waves copy the parent's panel into the first nn columns of the parent's front in LDS (lower triangle packed by
//     columns, as in k_hess_up_fam1) and clear the rest of it;
//   * the children are shared by the four waves (children w and w + 4 for wave w).  A child's panel comes in by consecutive lanes
//     over consecutive addresses into the wave's staging area; its diagonal block is factored and inverted there by the wave
//     (wave_potrf_inv16), L_AN = S_AN Li^T and K = L_AN Li are MFMA products whose accumulators are the next product's operands,
//     and the update -L_AN L_AN^T is added straight into the parent's front through relidx (ds_add_f64): the packed update block
//     of a family child is never written.  The child's panel goes to x, its inverse-form factor [Li; K] to lkout;
//   * behind one barrier wave 0 factors the parent's diagonal block, behind a second one wave gw forms row tile gw of L_AN, of K
//     and of the parent's update, which go to HBM where k_chol_mfma puts them (panel, lkout, packed update);
//   * childless cliques of the level below that belong to no family (lone) ride along as workgroups without children.
// A non-positive pivot raises the failure flag of its clique (child or parent) and ends the workgroup: a parent whose child
// failed is not factored.  LDS: front + 2 + 4 x (child panel + 256 + 32 ints) doubles = 39.8 KB on synth50k ((15, 64) parents,
// (5, 31) children): four workgroups per CU.
#include <hip/hip_runtime.h>

namespace smcp {

// dynamic LDS of k_chol_fam / k_pinv_fam: the parent's front (order <= nfmax), a flag word, and per wave a child's panel or LK
// block (<= cpan doubles), a 16 x 16 block and the child's relidx (32 ints)
__host__ __device__ inline int sfam_wave_doubles(int cpan) { return cpan + 256 + 16; }
__host__ inline size_t sfam_lds_bytes(int nfmax, int cpan) { return (size_t)(nfmax * (nfmax + 1) / 2 + 2 + 4 * sfam_wave_doubles(cpan)) * sizeof(double); }
struct SfamStage { double* P; double* D; int32_t* rel; };
__device__ inline SfamStage sfam_stage_of(double* zs, int nfmax, int wave, int cpan) {
  double* w = zs + nfmax * (nfmax + 1) / 2 + 2 + (size_t)wave * sfam_wave_doubles(cpan);
  return SfamStage{w, w + cpan, (int32_t*)(w + cpan + 256)};
}
// pan consecutive doubles from src into the staging area, by consecutive lanes; the relidx of clique d (na <= 32)
__device__ inline void sfam_stage(const SfamStage& st, const double* src, int pan, int lane) {
  for (int e0 = 0; e0 < pan; e0 += 256) {
    double v[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int e = e0 + 64 * h + lane;
      v[h] = e < pan ? src[(unsigned)e] : 0.0;
    }
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int e = e0 + 64 * h + lane;
      if (e < pan) st.P[e] = v[h];
    }
  }
}
__device__ inline void sfam_stage_rel(const SfamStage& st, const TreeArgs& t, const CliqueDesc& d, int lane) {
  if (lane < d.na) st.rel[lane] = t.relidx[d.rel + lane];
}
// the same for a block of at most 256 doubles in two halves: on its way into registers while the wave works on something else,
// from there into the staging area
struct SfamPre { double v[4]; int rel; };
__device__ inline void sfam_fetch(SfamPre& p, const double* src, int pan, const TreeArgs& t, const CliqueDesc& d, int lane) {
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int e = 64 * h + lane;
    p.v[h] = e < pan ? src[(unsigned)e] : 0.0;
  }
  p.rel = lane < d.na ? t.relidx[d.rel + lane] : 0;
}
__device__ inline void sfam_commit(const SfamStage& st, const SfamPre& p, int pan, const CliqueDesc& d, int lane) {
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int e = 64 * h + lane;
    if (e < pan) st.P[e] = p.v[h];
  }
  if (lane < d.na) st.rel[lane] = p.rel;
}

// one childless child from its staging area (st.P: its panel, nfc x nnc).  Returns false on a non-positive pivot.
template <int NATC, bool PREP>
__device__ inline bool chol_fam_child(const SfamStage& st, const CliqueDesc& cd, double* Pc, double* lkc, double* zs, int nfz, int lane) {
  const int l15 = lane & 15, kq = lane >> 4;
  const int nnc = cd.nn, nac = cd.na, nfc = nnc + nac;
  const int ksnc = (nnc + 3) >> 2;
  const d4 zero4 = {0.0, 0.0, 0.0, 0.0};
  wave_sync();                  // the staging area as the wave's other lanes wrote it
  const bool ok = wave_potrf_inv16(st.P, nfc, nnc, st.D);
  if (!ok) return false;
  wave_sync();
  double lir[4], lic[4], san[NATC][4];
  int rm[NATC];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int kk = kq + 4 * s;
    lir[s] = (l15 < nnc && kk <= l15) ? st.D[l15 + kk * 16] : 0.0;            // Li[l15][kk]
    lic[s] = (kk < nnc && l15 <= kk) ? st.D[kk + l15 * 16] : 0.0;             // Li[kk][l15]
    if (l15 < nnc && kk <= l15) Pc[l15 + kk * nfc] = st.P[l15 + kk * nfc];    // L_NN (lower)
    if (PREP && l15 < nnc && kk < nnc) lkc[l15 + kk * nfc] = lir[s];          // Li, zeros above the diagonal
#pragma unroll
    for (int t = 0; t < NATC; ++t) {
      const int m = 16 * t + l15;
      san[t][s] = (m < nac && kk < nnc) ? st.P[nnc + m + kk * nfc] : 0.0;     // S_AN[m][kk]
    }
  }
#pragma unroll
  for (int t = 0; t < NATC; ++t) {
    const int m = 16 * t + l15;
    rm[t] = m < nac ? st.rel[m] : -1;
  }
  d4 accL[NATC];
#pragma unroll
  for (int t = 0; t < NATC; ++t) {
    accL[t] = zero4;
    if (16 * t >= nac) continue;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s < ksnc) fmma(accL[t], san[t][s], lir[s]);                          // L_AN = S_AN Li^T
    d4 accK = zero4;
    if (PREP) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (s < ksnc) fmma(accK, accL[t][s], lic[s]);                          // K = L_AN Li
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int m = 16 * t + l15, n = kq + 4 * rr;
      if (m < nac && n < nnc) {
        Pc[(nnc + m) + n * nfc] = accL[t][rr];
        if (PREP) lkc[(nnc + m) + n * nfc] = accK[rr];
      }
    }
  }
  // update -L_AN L_AN^T into the parent's front
#pragma unroll
  for (int tm = 0; tm < NATC; ++tm)
#pragma unroll
    for (int tn = 0; tn <= tm; ++tn) {
      if (16 * tm >= nac) continue;
      d4 acc = zero4;
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (s < ksnc) fmma(acc, accL[tm][s], accL[tn][s]);
      const int ri = rm[tm];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int n = 16 * tn + kq + 4 * rr;          // (relidx ascends: ri >= rj below the diagonal)
        if (ri >= 0 && n < nac && 16 * tm + l15 >= n) unsafeAtomicAdd(&zs[pk_low(ri, st.rel[n], nfz)], -acc[rr]);
      }
    }
  wave_sync();                  // the staging area is read before the next child is staged
  return true;
}

// PNAT / CNAT: separator row tiles of the widest parent / child of the launch.  Grid: families + lone cliques.
// PREP: the inverse-form factor [Li; K] of every clique of the launch goes to lkout (as k_chol_mfma<true, true>).
template <int PNAT, int CNAT, bool PREP>
__global__ void __launch_bounds__(256, 4) k_chol_fam(MfmaArgs a, double* x, double* lkout, int nfmax, int cpan, int nfam, const int32_t* lone) {
  extern __shared__ double zs[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, l15 = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int k = (int)blockIdx.x < nfam ? a.t.lev[blockIdx.x] : lone[(int)blockIdx.x - nfam];
  const CliqueDesc d = a.t.cl[k];
  const int nn = d.nn, na = d.na, nf = nn + na;
  const int nch = (int)blockIdx.x < nfam ? d.chend - d.chbeg : 0;      // <= 8 (host guarantee)
  int* const sflag = (int*)(zs + nfmax * (nfmax + 1) / 2);              // failure seen by this workgroup (or before this launch)
  if (tid == 0) {           // [0]: a failure before this launch, [1]: of a child, [2]: of the parent
    sflag[0] = *info_of(a.t, k); sflag[1] = 0; sflag[2] = 0;
    if (nch > 8) { atomicCAS(info_of(a.t, k), 0, -7); sflag[0] = 1; }   // (a ninth child would go unfactored: a failed call, never a silent one)
  }
  double* const P = x + d.blk;
  double* const UkP = a.t.updp + d.updp;
  const int ksn = (nn + 3) >> 2;
  const d4 zero4 = {0.0, 0.0, 0.0, 0.0};
  // children `wave` and `wave + 4` of this wave; both descriptors are fetched now (two dependent round trips each)
  const bool has0 = wave < nch, has1 = wave + 4 < nch;
  const int kc0 = has0 ? a.t.chidx[d.chbeg + wave] : k, kc1 = has1 ? a.t.chidx[d.chbeg + wave + 4] : k;
  const CliqueDesc dc0 = a.t.cl[kc0];
  const CliqueDesc dc1 = a.t.cl[kc1];
  const SfamStage st = sfam_stage_of(zs, nfmax, wave, cpan);
  if (has0) { sfam_stage(st, x + dc0.blk, (dc0.nn + dc0.na) * dc0.nn, lane); sfam_stage_rel(st, a.t, dc0, lane); }
  // the parent's panel into the first nn columns of the front (a column per wave and step, rows by lanes), zeros behind them
  {
    double v[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = wave + 4 * c;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = j + lane + 64 * h;
        v[2 * c + h] = (j < nn && i < nf) ? P[i + j * nf] : 0.0;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = wave + 4 * c;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = j + lane + 64 * h;
        if (j < nn && i < nf) zs[pk_low(i, j, nf)] = v[2 * c + h];
      }
    }
    for (int e = pk_low(nn, nn, nf) + tid; e < nf * (nf + 1) / 2; e += 256) zs[e] = 0.0;
  }
  __syncthreads();
  if (sflag[0]) return;         // (a failure before this launch: nothing is factored, as on the per-level route)
  if (has0) {
    // the second child's panel is fetched beside the first one's factorisation
    const int pan1 = (dc1.nn + dc1.na) * dc1.nn;
    const bool pre1 = has1 && pan1 <= 256;
    SfamPre pre;
    if (pre1) sfam_fetch(pre, x + dc1.blk, pan1, a.t, dc1, lane);
    bool ok = chol_fam_child<CNAT, PREP>(st, dc0, x + dc0.blk, lkout + dc0.blk, zs, nf, lane);
    int kf = kc0;
    if (ok && has1) {
      if (pre1) sfam_commit(st, pre, pan1, dc1, lane);
      else { sfam_stage(st, x + dc1.blk, pan1, lane); sfam_stage_rel(st, a.t, dc1, lane); }
      ok = chol_fam_child<CNAT, PREP>(st, dc1, x + dc1.blk, lkout + dc1.blk, zs, nf, lane);
      kf = kc1;
    }
    if (!ok && lane == 0) { atomicCAS(info_of(a.t, kf), 0, info_val(a.t, kf)); sflag[1] = 1; }
  }
  __syncthreads();
  if (sflag[1]) return;
  // ---- the parent.  Wave 0: its diagonal block through a 16 x 16 scratch (the staging areas are free now), factor and inverse
  double* const Sd = sfam_stage_of(zs, nfmax, 1, cpan).D;     // diagonal block, leading dimension 16
  double* const Dv = sfam_stage_of(zs, nfmax, 0, cpan).D;     // its inverse
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = kq + 4 * r;
      if (l15 < nn && c <= l15) Sd[l15 + c * 16] = zs[pk_low(l15, c, nf)];
    }
    wave_sync();
    const bool ok = wave_potrf_inv16(Sd, 16, nn, Dv);
    if (!ok) { if (lane == 0) { atomicCAS(info_of(a.t, k), 0, info_val(a.t, k)); sflag[2] = 1; } }
    else {
      wave_sync();
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = kq + 4 * r;
        if (l15 < nn && c <= l15) P[l15 + c * nf] = Sd[l15 + c * 16];                                             // L_NN (lower)
        if (PREP && l15 < nn && c < nn) (lkout + d.blk)[l15 + c * nf] = c <= l15 ? Dv[l15 + c * 16] : 0.0;        // Li
      }
    }
  }
  __syncthreads();
  if (sflag[2]) return;
  // wave gw owns row tile gw of L_AN, of K and of the update matrix; it forms the L_AN tiles 0 .. gw itself (the result
  // register rr of a tile is the operand of k-step rr of the next product)
  const int gw = wave;
  if (gw >= PNAT || 16 * gw >= na) return;
  double lir[4], lic[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int kk = kq + 4 * s;
    lir[s] = (l15 < nn && kk <= l15) ? Dv[l15 + kk * 16] : 0.0;                // Li[l15][kk]
    lic[s] = (kk < nn && l15 <= kk) ? Dv[kk + l15 * 16] : 0.0;                 // Li[kk][l15]
  }
  d4 accL[PNAT];
#pragma unroll
  for (int t = 0; t < PNAT; ++t) {
    accL[t] = zero4;
    if (t > gw) continue;
    const int m = 16 * t + l15;
    double san[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) san[s] = (m < na && kq + 4 * s < nn) ? zs[pk_low(nn + m, kq + 4 * s, nf)] : 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s < ksn) fmma(accL[t], san[s], lir[s]);
  }
  d4 accM = zero4, accK = zero4;
#pragma unroll
  for (int t = 0; t < PNAT; ++t) if (t == gw) accM = accL[t];
  if (PREP) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s < ksn) fmma(accK, accM[s], lic[s]);
  }
  const int m = 16 * gw + l15;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int n = kq + 4 * rr;
    if (m < na && n < nn) {
      P[(nn + m) + n * nf] = accM[rr];
      if (PREP) (lkout + d.blk)[(nn + m) + n * nf] = accK[rr];
    }
  }
  // update tiles (gw, tn), tn <= gw: U_out = U_assembled - L_AN L_AN^T, packed, straight to HBM
#pragma unroll
  for (int tn = 0; tn < PNAT; ++tn) {
    if (tn > gw) continue;
    d4 acc = zero4;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s < ksn) fmma(acc, accM[s], accL[tn][s]);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int n = 16 * tn + kq + 4 * rr;
      if (m >= n && m < na) UkP[n * na - ((n * (n - 1)) >> 1) + (m - n)] = zs[pk_low(nn + m, nn + n, nf)] - acc[rr];
    }
  }
}

}  // namespace smcp
