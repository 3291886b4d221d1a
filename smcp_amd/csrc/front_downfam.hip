// Root -> leaves Hessian sweep (no scaling operand) of whole FAMILIES: one workgroup of four waves per (family parent,
// right-hand side).  A family (capi.hip classify_levels) is a front with nn <= 16, na <= 64 and its 1 .. 8 childless
// children with nn <= 16, 1 <= na <= 32.  k_hess_down_w (front_n16.hip) sweeps parents and children in two launches: every
// parent wave gathers its Z_AA from the grandparent tile by tile (four dependent rounds of 16 scattered loads per lane at
// na = 64), writes a mirror copy of it to global memory, and the next launch's children gather their Z_AA element by
// element from the parent's panel and that mirror.  Here
//   * the four waves load the parent's panel and gather its Z_AA from the grandparent in ONE round (a column per wave and
//     step, a row per lane) into the parent's front Z in LDS (lower triangle, packed by columns: at most 80 x 81 / 2 doubles);
//   * wave 0 runs the products of k_hess_down_w on the parent with every operand but Li and K read from LDS and leaves Z_NN and
//     Z_AN in LDS in place of the panel (and in the panel in global memory, the result);
//   * the children's panels, LK blocks and relidx come in by consecutive lanes over consecutive addresses into a staging area
//     per wave; nothing of them depends on the parent, so waves 1 .. 3 have their first child in registers and their second one
//     staged before the parent is done;
//   * after one barrier the four waves share the children (two each at eight children) and take the children's Z_AA from the
//     front in LDS through relidx.  The mirror copy and one launch per sweep are gone.
// LDS: front + 4 x (2 child panels + 32 ints) = 37.6 KB for (15, 64) parents with (5, 31) children: four workgroups per CU.
// The products, their order and every operand value are those of k_hess_down_w: the results are bitwise the same.
#include <hip/hip_runtime.h>

namespace smcp {

// position of (hi, lo), hi >= lo, in the lower triangle of a symmetric matrix of order n packed by columns
__device__ inline int pk_low(int hi, int lo, int n) { return hi + ((lo * (2 * n - lo - 1)) >> 1); }
// dynamic LDS: the parent's front (order <= nfmax) and the four waves' staging areas (children's panels of <= cpan doubles)
__host__ inline size_t down_fam_lds_bytes(int nfmax, int cpan) { return (size_t)(nfmax * (nfmax + 1) / 2 + 4 * (2 * cpan + 16)) * sizeof(double); }

// operands of one child in the lanes that need them as MFMA operands (layouts of k_hess_down_w)
// (M row tiles of storage; the functions below use the first NAT <= M: ONE object serves wave 0 for the parent's Li and K and
// then for its children -- two objects would both stay allocated across the barriers)
template <int M>
struct DownOps {
  double li[4], kk[4 * M], g[4], q[4 * M];
  int ri[M], rj[4 * M];     // rows of the parent's front that the separator rows 16 t + l15 / kq + 4 s map to (relidx)
};

// Li and K of clique d from its block LK of the inverse-form factor (global memory, or a copy in LDS)
template <int NAT, int M>
__device__ inline void down_fam_load_lk(double (&li)[4], double (&kk)[4 * M], const double* LK, const CliqueDesc& d, int lane) {
  const int l15 = lane & 15, kq = lane >> 4;
  const int nn = d.nn, na = d.na, nf = nn + na;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int r = kq + 4 * s;
    const double v = LK[(unsigned)(min(r, nn - 1) + min(l15, nn - 1) * nf)];
    li[s] = (r < nn && l15 < nn && r >= l15) ? v : 0.0;                         // Li[r][l15], lower triangular
  }
#pragma unroll
  for (int s = 0; s < 4 * NAT; ++s) {
    const int j = kq + 4 * s;
    // (a front without separator has no K rows: the clamped row index falls back into the supernode block)
    const double v = LK[(unsigned)((na > 0 ? nn + min(j, na - 1) : 0) + min(l15, nn - 1) * nf)];
    kk[s] = (j < na && l15 < nn) ? v : 0.0;                                      // K[j][l15]
  }
}

// LDS staging area of one wave for one child: its panel, its LK block (cpan doubles each) and its relidx (32 ints)
struct DownStage { double* P; double* LK; int32_t* rel; };
__device__ inline DownStage down_fam_stage_of(double* base, int wave, int cpan) {
  double* w = base + (size_t)wave * (2 * cpan + 16);
  return DownStage{w, w + cpan, (int32_t*)(w + 2 * cpan)};
}
// child d -> staging area, by consecutive lanes over consecutive addresses (the operand layouts below take 4-row pieces of
// 16 columns per load instruction: the same panels cost five times the load instructions when they are read from global memory)
__device__ inline void down_fam_stage(const DownStage& st, const MfmaArgs& a, const CliqueDesc& d, const double* U, int lane) {
  const int pan = (d.nn + d.na) * d.nn;
  const double* P = U + d.blk;
  const double* LK = a.LK + d.blk;
  for (int e0 = 0; e0 < pan; e0 += 256) {
    double vp[4], vl[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int e = e0 + 64 * h + lane;
      vp[h] = e < pan ? P[(unsigned)e] : 0.0;
      vl[h] = e < pan ? LK[(unsigned)e] : 0.0;
    }
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int e = e0 + 64 * h + lane;
      if (e < pan) { st.P[e] = vp[h]; st.LK[e] = vl[h]; }
    }
  }
  if (lane < d.na) st.rel[lane] = a.t.relidx[d.rel + lane];       // (na <= 32)
  __builtin_amdgcn_wave_barrier();
}

// operands of child d from its staging area
template <int NAT, int M>
__device__ inline void down_fam_load(DownOps<M>& o, const DownStage& st, const CliqueDesc& d, int lane) {
  const int l15 = lane & 15, kq = lane >> 4;
  const int nn = d.nn, na = d.na, nf = nn + na;       // (na >= 1: a family child)
  down_fam_load_lk<NAT, M>(o.li, o.kk, st.LK, d, lane);
#pragma unroll
  for (int t = 0; t < NAT; ++t) o.ri[t] = st.rel[min(16 * t + l15, na - 1)];
#pragma unroll
  for (int s = 0; s < 4 * NAT; ++s) o.rj[s] = st.rel[min(kq + 4 * s, na - 1)];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int c = kq + 4 * s;
    const int hi = min(max(l15, c), nn - 1), lo = min(min(l15, c), nn - 1);
    const double v = st.P[hi + lo * nf];
    o.g[s] = (l15 < nn && c < nn) ? v : 0.0;                                    // G_NN[c][l15] (symmetric, lower stored)
  }
#pragma unroll
  for (int t = 0; t < NAT; ++t) {
    const int m = 16 * t + l15;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int c = kq + 4 * s;
      const double v = st.P[nn + min(m, na - 1) + min(c, nn - 1) * nf];
      o.q[4 * t + s] = (m < na && c < nn) ? v : 0.0;                            // Q[m][c]
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// The products of k_hess_down_w on one front.  zs: a front of order nfz in LDS (lower, packed by columns).
// OWN = false (a child): G_NN, Q in o; Z_AA is gathered from zs, its parent's front, through o.ri / o.rj.
// OWN = true (the parent): zs is its own front; it holds G_NN and Q where Z_NN and Z_AN go (the lower part of the first nn
// columns IS the panel) and Z_AA behind them; Z_NN and Z_AN overwrite their inputs in LDS and go to the panel P as well.
// (one wave works on the front: its LDS reads and writes are served in program order, so a tile's results, written by other
// lanes than those that read its inputs, cannot overtake those reads)
template <int NAT, bool OWN, int M>
__device__ inline void down_fam_sweep(const DownOps<M>& o, const CliqueDesc& d, double* P, double* zs, int nfz, int lane) {
  const int l15 = lane & 15, kq = lane >> 4;
  const int nn = d.nn, na = d.na, nf = nn + na;
  const d4 zero4 = {0.0, 0.0, 0.0, 0.0};
  // Tt = Li^T G_NN, Z1 = Tt Li
  d4 tt = zero4, z1 = zero4;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    double g = o.g[s];
    if (OWN) {
      const int c = kq + 4 * s;
      const int hi = min(max(l15, c), nn - 1), lo = min(min(l15, c), nn - 1);
      const double v = zs[pk_low(hi, lo, nfz)];
      g = (l15 < nn && c < nn) ? v : 0.0;
    }
    tt = __builtin_amdgcn_mfma_f64_16x16x4f64(g, o.li[s], tt, 0, 0, 0);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) z1 = __builtin_amdgcn_mfma_f64_16x16x4f64(o.li[s], tt[s], z1, 0, 0, 0);
  d4 w = zero4;
#pragma unroll
  for (int t = 0; t < NAT; ++t) {
    if (16 * t < na) {
      double q[4];
      const int m = 16 * t + l15, mc = min(m, na - 1);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        q[s] = o.q[OWN ? s : 4 * t + s];
        if (OWN) {
          const int c = kq + 4 * s;
          const double v = zs[pk_low(nn + mc, min(c, nn - 1), nfz)];
          q[s] = (m < na && c < nn) ? v : 0.0;                                  // Q[m][c]
        }
      }
      d4 qlt = zero4, zkt = zero4;
#pragma unroll
      for (int s = 0; s < 4; ++s) qlt = __builtin_amdgcn_mfma_f64_16x16x4f64(q[s], o.li[s], qlt, 0, 0, 0);
      // Z_AA K in k-steps of eight (16 doubles of Z_AA in registers at a time)
#pragma unroll
      for (int s0 = 0; s0 < 4 * NAT; s0 += 8) {
        double z[8];
#pragma unroll
        for (int s = s0; s < s0 + 8 && s < 4 * NAT; ++s) {
          const int j = kq + 4 * s;
          const int i1 = OWN ? nn + mc : o.ri[t], j1 = OWN ? nn + min(j, na - 1) : o.rj[s];
          const double v = zs[pk_low(max(i1, j1), min(i1, j1), nfz)];
          z[s - s0] = (m < na && j < na) ? v : 0.0;                             // Z_AA[m][j]
        }
#pragma unroll
        for (int s = s0; s < s0 + 8 && s < 4 * NAT; ++s) zkt = __builtin_amdgcn_mfma_f64_16x16x4f64(z[s - s0], o.kk[s], zkt, 0, 0, 0);
        if (4 * NAT > 8) __builtin_amdgcn_sched_barrier(0);
      }
      d4 dt;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        dt[rr] = qlt[rr] - 0.5 * zkt[rr];                                       // D^T[l15][16 t + kq + 4 rr]
        const int mm = 16 * t + kq + 4 * rr;
        if (mm < na && l15 < nn) {
          const double v = qlt[rr] - zkt[rr];                                   // Z_AN[mm][l15]
          P[nn + mm + l15 * nf] = v;
          if (OWN) zs[pk_low(nn + mm, l15, nfz)] = v;
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        w = __builtin_amdgcn_mfma_f64_16x16x4f64(dt[s], o.kk[4 * t + s], w, 0, 0, 0);       // K^T D
        w = __builtin_amdgcn_mfma_f64_16x16x4f64(o.kk[4 * t + s], dt[s], w, 0, 0, 0);       // D^T K
      }
      __builtin_amdgcn_sched_barrier(0);     // (one tile's operands at a time in registers)
    }
  }
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int c = kq + 4 * rr;
    if (l15 < nn && c <= l15) {
      const double v = z1[rr] - w[rr];                                          // Z_NN, lower
      P[l15 + (int64_t)c * nf] = v;
      if (OWN) zs[pk_low(l15, c, nfz)] = v;
    }
  }
}

// PNAT / CNAT: separator row tiles of the widest parent / child of the launch.  Grid (families + lone cliques, right-hand sides).
// (four waves per SIMD = four workgroups per CU at 128 registers, <4, 2> with 12 of them spilled: the 896 families of synth50k
// are resident at once on 256 CUs.  The kernel is a chain of dependent memory round trips and MFMA chains that only other
// workgroups hide: 72 us at three workgroups per CU without spills, 54 us at four, measured on an earlier version)
template <int PNAT, int CNAT>
__global__ void __launch_bounds__(256, 4) k_hess_down_fam(MfmaArgs a, double* u, int64_t ldu, int nfmax, int cpan, int nfam, const int32_t* lone) {
  extern __shared__ double zs[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // workgroups beyond the nfam families: the childless cliques of the level below that belong to no family (lone), each swept as
  // a parent without children (they would otherwise be a launch of their own behind this one: 12 us for the one such leaf of synth50k)
  const int k = (int)blockIdx.x < nfam ? a.t.lev[blockIdx.x] : lone[(int)blockIdx.x - nfam];
  const CliqueDesc d = a.t.cl[k];
  const int nn = d.nn, na = d.na, nf = nn + na;
  const int nch = (int)blockIdx.x < nfam ? d.chend - d.chbeg : 0;
  double* U = u + (int64_t)blockIdx.y * ldu;
  double* P = U + d.blk;
  // children q0 and q0 + 4 of this wave: wave 0, busy with the parent first, takes 3 and 7.  Both descriptors are fetched now:
  // behind the barriers they would be two more dependent round trips each (child list, descriptor) in front of the operands
  const int q0 = (wave + 3) & 3;
  const bool has0 = q0 < nch, has1 = q0 + 4 < nch;
  const CliqueDesc dc0 = a.t.cl[has0 ? a.t.chidx[d.chbeg + q0] : k];
  const CliqueDesc dc1 = a.t.cl[has1 ? a.t.chidx[d.chbeg + q0 + 4] : k];
  const DownStage st = down_fam_stage_of(zs + nfmax * (nfmax + 1) / 2, wave, cpan);
  constexpr int M = PNAT > CNAT ? PNAT : CNAT;
  DownOps<M> o;
  // nothing of the children depends on the parent: waves 1 .. 3 have their first child in registers and their second one staged
  // before the parent is done, wave 0 its first one staged
  if (has0) down_fam_stage(st, a, dc0, U, lane);
  if (wave == 0) down_fam_load_lk<PNAT, M>(o.li, o.kk, a.LK + d.blk, d, lane);      // (of the parent: Li and K only, the rest comes from LDS)
  else if (has0) {
    down_fam_load<CNAT, M>(o, st, dc0, lane);
    if (has1) down_fam_stage(st, a, dc1, U, lane);
  }
  // the parent's panel (G_NN lower, Q) into the first nn columns of the front: a column per wave and step, rows by lanes
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
  }
  __builtin_amdgcn_sched_barrier(0);
  // the parent's Z_AA from the grandparent's front (its panel and the copy of its Z_AA in the update workspace): a column per
  // wave and step, a row per lane
  if (na > 0) {
    const bool haspar = d.parent >= 0;
    const CliqueDesc par = a.t.cl[haspar ? d.parent : k];
    const int nng = par.nn, nag = par.na, nfg = nng + nag;
    const double* Pg = U + par.blk;
    const double* Ug = a.t.upd + (int64_t)blockIdx.y * a.t.updlen + par.upd;
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
        v[c] = lo < nng ? Pg[hi + lo * nfg] : Ug[(hi - nng) + (lo - nng) * nag];
      }
    }
#pragma unroll
    for (int c = 0; c < 4 * PNAT; ++c) {
      const int j = wave + 4 * c;
      if (j < na && lane >= j && lane < na) zs[pk_low(nn + lane, nn + j, nf)] = v[c];
    }
  }
  __syncthreads();
  if (wave == 0) down_fam_sweep<PNAT, true, M>(o, d, P, zs, nf, lane);
  __syncthreads();
  if (has0) {
    if (wave == 0) {
      down_fam_load<CNAT, M>(o, st, dc0, lane);
      if (has1) down_fam_stage(st, a, dc1, U, lane);
    }
    down_fam_sweep<CNAT, false, M>(o, dc0, U + dc0.blk, zs, nf, lane);
  }
  if (has1) {
    down_fam_load<CNAT, M>(o, st, dc1, lane);
    down_fam_sweep<CNAT, false, M>(o, dc1, U + dc1.blk, zs, nf, lane);
  }
}

}  // namespace smcp
