// Projected inverse of whole FAMILIES at the scaling point: one workgroup of four waves per family, parent -> children (the
// families and the LDS layout of k_chol_fam, front_cholfam.hip).  The per-level route (k_pinv_mfma<true> on the parents, then on
// the leaves) has every child gather its Y_AA element by element from the parent's panel and the parent's Y_AA block in HBM,
// in a launch of its own.  Here
//   * the four waves gather the parent's Y_AA from the grandparent (its panel and its Y_AA block in the separator workspace: a
//     column per wave and step, a row per lane) into the parent's front in LDS (lower triangle packed by columns) and store it to
//     the separator workspace, where k_factor_yaa_lds and the sweeps look for it;
//   * nothing of a child but its Y_AA depends on the parent: every wave has the [Li; K] block and the relidx of its first child
//     staged in LDS before the parent is done;
//   * wave gw forms row tile gw of E^T = K^T Y_AA (the accumulator is the right operand of the next product), Y_AN = -E goes to the
//     panel and into the front, and the tile's share of Y_NN = Li^T Li + K^T E to a 16 x 16 block of its own in LDS; behind a
//     barrier the four shares are summed in a fixed order, Y_NN goes to the panel and into the front;
//   * behind one more barrier the four waves share the children (w and w + 4 for wave w): a child takes its Y_AA from the front in
//     LDS through relidx, stores it to the separator workspace and forms its panel by the same products;
//   * childless cliques of the level below that belong to no family (lone) ride along as workgroups without children.
// A family parent that is a root (na = 0) has nothing to gather: Y_NN = Li^T Li.  Every sum has a fixed order: the results do not
// change from run to run.
#include <hip/hip_runtime.h>

namespace smcp {

// E^T = K^T Y_AA by row tiles, Y_AN = -E to the panel P, and the share of the tiles t0 .. t1 - 1 in Y_NN = Li^T Li + K^T E
// (with_li: the Li^T Li term is part of this share).  li / kk: operands of down_fam_load_lk.  OWN: zs is the clique's own front
// (order nfz = nn + na; Y_AN is kept there as well); otherwise Y_AA is taken from zs, its parent's front, through rel and
// stored to yaa (lower triangle, leading dimension na).
template <int NAT, bool OWN, int M>
__device__ inline d4 pinv_fam_tiles(const double (&li)[4], const double (&kk)[4 * M], const CliqueDesc& d, double* P, double* yaa,
                                    double* zs, int nfz, const int32_t* rel, int t0, int t1, bool with_li, int lane) {
  const int l15 = lane & 15, kq = lane >> 4;
  const int nn = d.nn, na = d.na, nf = nn + na;
  const int ksn = (nn + 3) >> 2, ksa = (na + 3) >> 2;
  const d4 zero4 = {0.0, 0.0, 0.0, 0.0};
  d4 accN = zero4;
  if (with_li) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s < ksn) fmma(accN, li[s], li[s]);                      // (Li^T Li)[l15][n] = sum_kk Li[kk][l15] Li[kk][n]
  }
#pragma unroll
  for (int t = 0; t < NAT; ++t) {
    if (t < t0 || t >= t1 || 16 * t >= na) continue;
    const int m = 16 * t + l15;
    int ri = 0;
    if (!OWN) ri = rel[min(m, na - 1)];
    d4 accE = zero4;
#pragma unroll
    for (int s0 = 0; s0 < 4 * NAT; s0 += 8) {
      double y[8];
#pragma unroll
      for (int s = s0; s < s0 + 8 && s < 4 * NAT; ++s) {
        const int j = kq + 4 * s;
        const int i1 = OWN ? nn + min(m, na - 1) : ri, j1 = OWN ? nn + min(j, na - 1) : rel[min(j, na - 1)];
        const double v = zs[pk_low(max(i1, j1), min(i1, j1), nfz)];
        y[s - s0] = (m < na && j < na) ? v : 0.0;                 // Y_AA[m][j]
        if (!OWN && m < na && j <= m) yaa[m + j * na] = v;
      }
#pragma unroll
      for (int s = s0; s < s0 + 8 && s < 4 * NAT; ++s)
        if (s < ksa) fmma(accE, kk[s], y[s - s0]);                // E^T[l15][16 t + n] = sum_j K[j][l15] Y_AA[j][16 t + n]
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int mm = 16 * t + kq + 4 * rr;
      if (mm < na && l15 < nn) {
        P[nn + mm + l15 * nf] = -accE[rr];                        // Y_AN[mm][l15]
        if (OWN) zs[pk_low(nn + mm, l15, nfz)] = -accE[rr];
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) fmma(accN, kk[4 * t + s], accE[s]);           // (K^T E)[l15][n]: K[16 t + kq + 4 s][l15] is K^T in left-operand layout, the accumulator E^T[l15][16 t + kq + 4 s] is E in right-operand layout
  }
  return accN;
}

// PNAT / CNAT: separator row tiles of the widest parent / child of the launch.  Grid: families + lone cliques.
template <int PNAT, int CNAT>
__global__ void __launch_bounds__(256, 4) k_pinv_fam(MfmaArgs a, double* x, int nfmax, int cpan, int nfam, const int32_t* lone) {
  extern __shared__ double zs[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, l15 = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int k = (int)blockIdx.x < nfam ? a.t.lev[blockIdx.x] : lone[(int)blockIdx.x - nfam];
  const CliqueDesc d = a.t.cl[k];
  const int nn = d.nn, na = d.na, nf = nn + na;
  const int nch = (int)blockIdx.x < nfam ? d.chend - d.chbeg : 0;      // <= 8 (host guarantee: the factorisation has checked it)
  double* const P = x + d.blk;
  const bool has0 = wave < nch, has1 = wave + 4 < nch;
  const CliqueDesc dc0 = a.t.cl[has0 ? a.t.chidx[d.chbeg + wave] : k];
  const CliqueDesc dc1 = a.t.cl[has1 ? a.t.chidx[d.chbeg + wave + 4] : k];
  const SfamStage st = sfam_stage_of(zs, nfmax, wave, cpan);
  if (has0) { sfam_stage(st, a.LK + dc0.blk, (dc0.nn + dc0.na) * dc0.nn, lane); sfam_stage_rel(st, a.t, dc0, lane); }
  constexpr int M = PNAT > CNAT ? PNAT : CNAT;
  double li[4], kk[4 * M];
  down_fam_load_lk<PNAT, M>(li, kk, a.LK + d.blk, d, lane);             // (of the parent, from global memory in operand layout)
  // the parent's Y_AA from the grandparent's front (its panel and its Y_AA block): a column per wave and step, a row per lane
  if (na > 0) {
    const bool haspar = d.parent >= 0;
    const CliqueDesc par = a.t.cl[haspar ? d.parent : k];
    const int nng = par.nn, nag = par.na, nfg = nng + nag;
    const double* Pg = x + par.blk;
    const double* Ug = a.t.upd + par.upd;
    double* const UkG = a.t.upd + d.upd;
    const int32_t* rel = a.t.relidx + d.rel;
    const int gi = rel[min(lane, na - 1)];
    double v[4 * PNAT];
#pragma unroll
    for (int c = 0; c < 4 * PNAT; ++c) {
      const int j = wave + 4 * c;
      v[c] = 0.0;
      if (haspar && j < na && lane >= j && lane < na) {
        const int gj = rel[j];
        const int hi = max(gi, gj), lo = min(gi, gj);
        v[c] = lo < nng ? Pg[hi + (int64_t)lo * nfg] : Ug[(hi - nng) + (int64_t)(lo - nng) * nag];
      }
    }
#pragma unroll
    for (int c = 0; c < 4 * PNAT; ++c) {
      const int j = wave + 4 * c;
      if (j < na && lane >= j && lane < na) {
        zs[pk_low(nn + lane, nn + j, nf)] = v[c];
        if (haspar) UkG[lane + j * na] = v[c];
      }
    }
  }
  __syncthreads();
  // ---- the parent: wave gw forms row tile gw and its share of Y_NN (wave 0: with the Li^T Li term)
  {
    const d4 accN = pinv_fam_tiles<PNAT, true, M>(li, kk, d, P, nullptr, zs, nf, nullptr, wave, wave + 1, wave == 0, lane);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) st.D[l15 + 16 * (kq + 4 * rr)] = accN[rr];
  }
  __syncthreads();
  {
    const int i = tid & 15, j = tid >> 4;
    if (i < nn && j <= i) {
      double v = sfam_stage_of(zs, nfmax, 0, cpan).D[tid];
#pragma unroll
      for (int w = 1; w < 4; ++w)
        if (w < PNAT && 16 * w < na) v += sfam_stage_of(zs, nfmax, w, cpan).D[tid];
      zs[pk_low(i, j, nf)] = v;                                   // Y_NN (lower)
      P[i + j * nf] = v;
    }
  }
  if (nch == 0) return;
  __syncthreads();
  // ---- the children, from the front in LDS
  const int pan1 = (dc1.nn + dc1.na) * dc1.nn;
  const bool pre1 = has1 && pan1 <= 256;       // the second child's LK block and relidx are fetched beside the first one's products
  SfamPre pre;
  if (has0) {
    down_fam_load_lk<CNAT, M>(li, kk, st.P, dc0, lane);
    if (pre1) sfam_fetch(pre, a.LK + dc1.blk, pan1, a.t, dc1, lane);
  }
  auto child = [&](const CliqueDesc& dc) {
    double* const Pc = x + dc.blk;
    const d4 accN = pinv_fam_tiles<CNAT, false, M>(li, kk, dc, Pc, a.t.upd + dc.upd, zs, nf, st.rel, 0, CNAT, true, lane);
    const int nfc = dc.nn + dc.na;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int c = kq + 4 * rr;
      if (l15 < dc.nn && c <= l15) Pc[l15 + c * nfc] = accN[rr];  // Y_NN (lower; the accumulator holds the symmetric block)
    }
  };
  if (has0) child(dc0);
  if (has1) {
    wave_sync();                // the first child's LK block and relidx have been read
    if (pre1) sfam_commit(st, pre, pan1, dc1, lane);
    else { sfam_stage(st, a.LK + dc1.blk, pan1, lane); sfam_stage_rel(st, a.t, dc1, lane); }
    wave_sync();
    down_fam_load_lk<CNAT, M>(li, kk, st.P, dc1, lane);
    child(dc1);
  }
}

}  // namespace smcp
