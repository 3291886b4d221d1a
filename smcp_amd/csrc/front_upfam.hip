// Leaves -> root Hessian sweep of whole FAMILIES for few dense right-hand sides: one workgroup of four waves per (family parent,
// right-hand side), every family of the level resident at once.  k_hess_up_fam (front_fam.hip) was built for the Schur sweeps,
// where one workgroup of twelve waves pushes many right-hand sides through a double-buffered pipeline out of 155 KB of LDS: for
// ONE right-hand side that is one workgroup per CU (3.5 rounds of the 896 families of synth50k on 256 CUs), a set-up (clear the
// LDS, offset table, constants into operand layouts) that is used once, and a child group and a parent group that run strictly
// one after the other.  Here
//   * the four waves copy the parent's input panel into the first nn columns of the parent's front in LDS (lower triangle packed
//     by columns, as in k_hess_down_fam: at most 80 x 81 / 2 doubles) and clear the rest of it;
//   * the children are shared by the four waves (children w and w + 4 for wave w).  A child's input panel, its LK block and its
//     relidx come in by consecutive lanes over consecutive addresses into the wave's staging area (down_fam_stage) and are read
//     from there in MFMA layout; the products are those of the child group of k_hess_up_fam with the same accumulator-to-operand
//     reuse, the update -(K E^T + E K^T) is added into the front through relidx (ds_add_f64), the output panel goes to HBM;
//   * after one barrier wave gw runs row tile gw of the parent's products as the parent group of k_hess_up_fam does, out of the
//     one front; output panel and packed update straight to HBM;
//   * childless cliques of the level below that belong to no family (lone) ride along as workgroups without children.
// No workgroup waits for another.  LDS: that of k_hess_down_fam (front + 4 x (2 child panels + 32 ints) = 37.6 KB on synth50k),
// four workgroups per CU.  The scaling operands (Y_AA blocks or their factors) and the parent's K are read from global memory
// in operand layout: staging them would cost the fourth workgroup per CU (8 KB for K, 16 KB for the children's blocks).
#include <hip/hip_runtime.h>

namespace smcp {

// operand [m][kk] of the scaling product from the block ys (order na, lower triangle stored in full-matrix layout)
__device__ inline double up_fam_ysc(const double* ys, int ymode, int m, int kk, int na) {
  if (m >= na || kk >= na) return 0.0;
  if (ymode == 1) return m >= kk ? ys[m + kk * na] : ys[kk + m * na];
  if (ymode == 2) return kk >= m ? ys[kk + m * na] : 0.0;       // R^T
  return m >= kk ? ys[m + kk * na] : 0.0;                       // R
}

// panel, LK block and relidx entry of a child with at most 256 panel entries on their way into registers / from there into the
// staging area: the second child of a wave is fetched while its first one is being multiplied
struct UpPre { double vp[4], vl[4]; int rel; };
__device__ inline void up_fam_fetch(UpPre& p, const MfmaArgs& a, const CliqueDesc& d, const double* U, int lane) {
  const int pan = (d.nn + d.na) * d.nn;
  const double* P = U + d.blk;
  const double* LK = a.LK + d.blk;
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int e = 64 * h + lane;
    p.vp[h] = e < pan ? P[(unsigned)e] : 0.0;
    p.vl[h] = e < pan ? LK[(unsigned)e] : 0.0;
  }
  p.rel = lane < d.na ? a.t.relidx[d.rel + lane] : 0;
}
__device__ inline void up_fam_commit(const DownStage& st, const UpPre& p, const CliqueDesc& d, int lane) {
  const int pan = (d.nn + d.na) * d.nn;
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int e = 64 * h + lane;
    if (e < pan) { st.P[e] = p.vp[h]; st.LK[e] = p.vl[h]; }
  }
  if (lane < d.na) st.rel[lane] = p.rel;
}

// one childless child from its staging area: E = F_AN - K F_NN / 2, X = F_AN - K F_NN, T = Li F_NN; update -(K E^T + E K^T) into
// the parent's front zs (order nfz); G = X Li^T, G_NN = T Li^T and, with a scaling operand, Q = Ysc G to the child's panel Pc
// (loaded(): called once the child's operands are in registers -- the staging area's panel and LK block are free from there on)
template <int NATC, class F>
__device__ inline void up_fam_child(const MfmaArgs& a, const DownStage& st, const CliqueDesc& cd, double* Pc, double* zs, int nfz, int lane, F loaded) {
  const int l15 = lane & 15, kq = lane >> 4;
  const int nnc = cd.nn, nac = cd.na, nfc = nnc + nac;
  const int ksnc = (nnc + 3) >> 2, ksac = (nac + 3) >> 2;
  const int ymode = a.ymode;
  const d4 zero4 = {0.0, 0.0, 0.0, 0.0};
  double kreg[NATC][4], bdreg[4], fnn[4], fan[NATC][4];
  int rm[NATC];
  wave_sync();                  // the staging area as the wave's other lanes wrote it
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int kk = kq + 4 * s;
    bdreg[s] = (l15 < nnc && kk <= l15) ? st.LK[l15 + kk * nfc] : 0.0;                                     // Li[l15][kk]
    fnn[s] = (l15 < nnc && kk < nnc) ? st.P[max(l15, kk) + min(l15, kk) * nfc] : 0.0;                      // F_NN (symmetric)
#pragma unroll
    for (int t = 0; t < NATC; ++t) {
      const int m = 16 * t + l15;
      const bool in = m < nac && kk < nnc;
      kreg[t][s] = in ? st.LK[nnc + m + kk * nfc] : 0.0;                                                    // K[m][kk]
      fan[t][s] = in ? st.P[nnc + m + kk * nfc] : 0.0;                                                      // F_AN[m][kk]
    }
  }
#pragma unroll
  for (int t = 0; t < NATC; ++t) {
    const int m = 16 * t + l15;
    rm[t] = m < nac ? st.rel[m] : -1;
  }
  wave_sync();                  // panel and LK block of the staging area are free from here on (G goes through it below)
  loaded();
  d4 accE[NATC], accT = zero4;
#pragma unroll
  for (int t = 0; t < NATC; ++t) {
    accE[t] = zero4;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s < ksnc) fmma(accE[t], kreg[t][s], fnn[s]);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s < ksnc) fmma(accT, bdreg[s], fnn[s]);
  double ev[NATC][4], xv[NATC][4];
#pragma unroll
  for (int t = 0; t < NATC; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      ev[t][rr] = fan[t][rr] - 0.5 * accE[t][rr];
      xv[t][rr] = fan[t][rr] - accE[t][rr];
    }
#pragma unroll
  for (int tm = 0; tm < NATC; ++tm)
#pragma unroll
    for (int tn = 0; tn <= tm; ++tn) {
      if (16 * tm >= nac) continue;
      d4 acc = zero4;
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (s < ksnc) {
          fmma(acc, kreg[tm][s], ev[tn][s]);
          fmma(acc, ev[tm][s], kreg[tn][s]);
        }
      const int ri = rm[tm];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int n = 16 * tn + kq + 4 * rr;          // (relidx ascends: ri >= rj below the diagonal)
        if (ri >= 0 && n < nac && 16 * tm + l15 >= n) unsafeAtomicAdd(&zs[pk_low(ri, st.rel[n], nfz)], -acc[rr]);
      }
    }
  d4 accG[NATC], accN = zero4;
#pragma unroll
  for (int t = 0; t < NATC; ++t) {
    accG[t] = zero4;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s < ksnc) fmma(accG[t], xv[t][s], bdreg[s]);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s < ksnc) fmma(accN, accT[s], bdreg[s]);
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int jn = kq + 4 * rr;
    if (l15 < nnc && jn <= l15) Pc[l15 + jn * nfc] = accN[rr];                    // G_NN (lower)
  }
  if (!ymode) {
#pragma unroll
    for (int t = 0; t < NATC; ++t)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int m = 16 * t + l15, n = kq + 4 * rr;
        if (m < nac && n < nnc) Pc[(nnc + m) + n * nfc] = accG[t][rr];
      }
    return;
  }
  // Q = Ysc G: G is transposed through the staging area (G[m][n] at m + n * nac: nac * nnc doubles, no more than a panel)
#pragma unroll
  for (int t = 0; t < NATC; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int m = 16 * t + l15, n = kq + 4 * rr;
      if (m < nac && n < nnc) st.P[m + n * nac] = accG[t][rr];
    }
  wave_sync();
  double gv[4 * NATC];
#pragma unroll
  for (int s2 = 0; s2 < 4 * NATC; ++s2) {
    const int kk = kq + 4 * s2;
    gv[s2] = (kk < nac && l15 < nnc) ? st.P[kk + l15 * nac] : 0.0;
  }
  const double* ys = a.ysc + cd.upd;
#pragma unroll
  for (int t = 0; t < NATC; ++t) {
    if (16 * t >= nac) continue;
    double yc[4 * NATC];
#pragma unroll
    for (int s2 = 0; s2 < 4 * NATC; ++s2) yc[s2] = up_fam_ysc(ys, ymode, 16 * t + l15, kq + 4 * s2, nac);
    d4 acc = zero4;
#pragma unroll
    for (int s2 = 0; s2 < 4 * NATC; ++s2)     // R^T (ymode 2) is zero left of the diagonal block, R (3) right of it
      if (s2 < ksac && !(ymode == 2 && s2 < 4 * t) && !(ymode == 3 && s2 >= 4 * (t + 1)))
        fmma(acc, yc[s2], gv[s2]);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int m = 16 * t + l15, n = kq + 4 * rr;
      if (m < nac && n < nnc) Pc[(nnc + m) + n * nfc] = acc[rr];
    }
  }
  wave_sync();                  // G is consumed before the next child is staged
}

// PNAT / CNAT: separator row tiles of the widest parent / child of the launch.  Grid (families + lone cliques, right-hand sides).
template <int PNAT, int CNAT>
__global__ void __launch_bounds__(256, 4) k_hess_up_fam1(MfmaArgs a, double* u, int64_t ldu, int nfmax, int cpan, int nfam, const int32_t* lone) {
  extern __shared__ double zs[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, l15 = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int k = (int)blockIdx.x < nfam ? a.t.lev[blockIdx.x] : lone[(int)blockIdx.x - nfam];
  const CliqueDesc d = a.t.cl[k];
  const int nn = d.nn, na = d.na, nf = nn + na;
  const int nch = (int)blockIdx.x < nfam ? d.chend - d.chbeg : 0;      // <= 8 (host guarantee)
  if (nch > 8 && tid == 0) atomicCAS(a.t.info, 0, -7);                 // (a ninth child would go unswept: a failed call, never a silent one)
  double* const U = u + (int64_t)blockIdx.y * ldu;
  double* const P = U + d.blk;
  double* const UkP = a.t.updp + (int64_t)blockIdx.y * a.t.updplen + d.updp;
  const int ymode = a.ymode;
  const int ksn = (nn + 3) >> 2, ksa = (na + 3) >> 2;
  const d4 zero4 = {0.0, 0.0, 0.0, 0.0};
  // children `wave` and `wave + 4` of this wave; both descriptors are fetched now (two dependent round trips each)
  const bool has0 = wave < nch, has1 = wave + 4 < nch;
  const CliqueDesc dc0 = a.t.cl[has0 ? a.t.chidx[d.chbeg + wave] : k];
  const CliqueDesc dc1 = a.t.cl[has1 ? a.t.chidx[d.chbeg + wave + 4] : k];
  const DownStage st = down_fam_stage_of(zs + nfmax * (nfmax + 1) / 2, wave, cpan);
  if (has0) down_fam_stage(st, a, dc0, U, lane);
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
  const bool pre1 = has1 && (dc1.nn + dc1.na) * dc1.nn <= 256;      // the second child is fetched beside the first one's products
  UpPre pre;
  if (has0) up_fam_child<CNAT>(a, st, dc0, U + dc0.blk, zs, nf, lane, [&]() { if (pre1) up_fam_fetch(pre, a, dc1, U, lane); });
  if (has1) {
    if (pre1) up_fam_commit(st, pre, dc1, lane);
    else down_fam_stage(st, a, dc1, U, lane);
    up_fam_child<CNAT>(a, st, dc1, U + dc1.blk, zs, nf, lane, []() {});
  }
  __syncthreads();
  // ---- the parent: wave gw owns row tile gw of the update matrix, of G and of Q; it forms the E tiles 0 .. gw itself (the result
  // register rr of a tile is the operand of k-step rr of the next product); wave 0 also forms T and G_NN
  const int gw = wave;
  const double* const lk = a.LK + d.blk;
  double bdP[4], kt[PNAT][4], kPm[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int kk = kq + 4 * s;
    bdP[s] = (l15 < nn && kk <= l15) ? lk[l15 + kk * nf] : 0.0;                  // Li[l15][kk]
#pragma unroll
    for (int t = 0; t < PNAT; ++t) {
      const int m = 16 * t + l15;
      kt[t][s] = (t <= gw && m < na && kk < nn) ? lk[(nn + m) + kk * nf] : 0.0;  // K[m][kk]
      if (t == gw) kPm[s] = kt[t][s];
    }
  }
  double ev[PNAT][4], evm[4] = {0.0, 0.0, 0.0, 0.0}, xvm[4] = {0.0, 0.0, 0.0, 0.0};
  d4 accT = zero4;
  {
    double fnn[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int kr = kq + 4 * s;
      fnn[s] = (kr < nn && l15 < nn) ? zs[pk_low(max(kr, l15), min(kr, l15), nf)] : 0.0;
    }
#pragma unroll
    for (int t = 0; t < PNAT; ++t) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) ev[t][rr] = 0.0;
      if (t <= gw && 16 * t < na) {
        double fan[4];
        const int m = 16 * t + l15;
#pragma unroll
        for (int s = 0; s < 4; ++s) fan[s] = (m < na && kq + 4 * s < nn) ? zs[pk_low(nn + m, kq + 4 * s, nf)] : 0.0;
        d4 acc = zero4;
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (s < ksn) fmma(acc, kt[t][s], fnn[s]);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) ev[t][rr] = fan[rr] - 0.5 * acc[rr];       // E = F_AN - K F_NN / 2
        if (t == gw) {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) { evm[rr] = ev[t][rr]; xvm[rr] = fan[rr] - acc[rr]; }   // X = F_AN - K F_NN
        }
      }
    }
    if (gw == 0) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (s < ksn) fmma(accT, bdP[s], fnn[s]);
    }
  }
  __syncthreads();              // every wave has read F_NN / F_AN: G may take the place of F_AN
  if (gw < PNAT && 16 * gw < na) {
    const int m = 16 * gw + l15;
    // update tiles (gw, tn), tn <= gw: U_out = U_assembled - K E^T - E K^T, packed, straight to HBM
#pragma unroll
    for (int tn = 0; tn < PNAT; ++tn) {
      if (tn > gw) continue;
      d4 acc = zero4;
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (s < ksn) {
          fmma(acc, kPm[s], ev[tn][s]);
          fmma(acc, evm[s], kt[tn][s]);
        }
      double uv[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int n = 16 * tn + kq + 4 * rr;
        uv[rr] = (m >= n && m < na) ? zs[pk_low(nn + m, nn + n, nf)] : 0.0;
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int n = 16 * tn + kq + 4 * rr;
        if (m >= n && m < na) UkP[n * na - ((n * (n - 1)) >> 1) + (m - n)] = uv[rr] - acc[rr];
      }
    }
    // G = X Li^T: row tile gw
    d4 acc = zero4;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s < ksn) fmma(acc, xvm[s], bdP[s]);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int n = kq + 4 * rr;
      if (m < na && n < nn) {
        if (ymode) zs[pk_low(nn + m, n, nf)] = acc[rr];
        else P[(nn + m) + n * nf] = acc[rr];
      }
    }
  }
  // G_NN = T Li^T (lower), straight to HBM
  if (gw == 0) {
    d4 acc = zero4;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s < ksn) fmma(acc, accT[s], bdP[s]);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int jn = kq + 4 * rr;
      if (l15 < nn && jn <= l15) P[l15 + jn * nf] = acc[rr];
    }
  }
  if (!ymode) return;
  __syncthreads();              // G complete
  // Q = Ysc G (row tile gw), straight to HBM
  if (gw < PNAT && 16 * gw < na) {
    const double* ys = a.ysc + d.upd;
    const int m = 16 * gw + l15;
    d4 acc = zero4;
#pragma unroll
    for (int s0 = 0; s0 < 4 * PNAT; s0 += 8) {
      double yv[8], gv[8];
#pragma unroll
      for (int s2 = s0; s2 < s0 + 8 && s2 < 4 * PNAT; ++s2) {
        const int kk = kq + 4 * s2;
        yv[s2 - s0] = up_fam_ysc(ys, ymode, m, kk, na);
        gv[s2 - s0] = (kk < na && l15 < nn) ? zs[pk_low(nn + kk, l15, nf)] : 0.0;
      }
#pragma unroll
      for (int s2 = s0; s2 < s0 + 8 && s2 < 4 * PNAT; ++s2)     // R^T (ymode 2) is zero left of the diagonal block, R (3) right of it
        if (s2 < ksa && !(ymode == 2 && s2 < 4 * gw) && !(ymode == 3 && s2 >= 4 * (gw + 1)))
          fmma(acc, yv[s2 - s0], gv[s2 - s0]);
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int n = kq + 4 * rr;
      if (m < na && n < nn) P[(nn + m) + n * nf] = acc[rr];
    }
  }
}

}  // namespace smcp
