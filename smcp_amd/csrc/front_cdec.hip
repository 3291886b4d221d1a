// The factor as a sum of PSD clique blocks (Agler's decomposition of L L^T; no CHOMPACK counterpart).
// Clique k has nn own columns and nf = nn + na rows; its panel P is nf x nn, column-major with leading dimension nf, at
// blkptr[k] of L.blkval.  With Pt[m, c] = P[m, c] for m >= c and 0 otherwise (the slots m < c < nn are NEVER READ: after
// cholesky they hold whatever they hold)
//   Z_k[i, j] = sum_{c = 0}^{min(i, j, nn - 1)} Pt[i, c] Pt[j, c],        0 <= i, j < nf,        c ascending,
// stored at Z + qptr[k] + i + j nf: the full symmetric block, both triangles, as clique_gather returns it.  Z_k[i, j] and
// Z_k[j, i] carry the same bits, and every entry of Z has exactly one writer.  Every column of L belongs to one supernode
// and its nonzeros lie in that clique's rows, hence L L^T = sum_k E_k Z_k E_k^T with Z_k = Pt Pt^T PSD of rank <= nn.
// No dependency along the tree, no reduction across cliques, no atomics, no flags between workgroups, no inline assembly:
// one launch per route, two when a call uses both.  L is only read; the same L gives the same bits from call to call.
//
// k_cdec_fma: plain FMA, one wave per item (clique, 64 output rows, CDEC_JC output columns), four items per workgroup,
// lane = output row i.  Pt[i, c] streams coalesced down panel column c; the Pt[j, c] of the item's columns are loaded
// once by the wave (lane l: column l & 15, inner index l >> 4 of each group of four) and read from the lanes as
// wave-uniform operands.  c ascends, so the summation order is that of the definition; both triangles are computed by the
// same chain of FMAs (a product commutes), which is why Z_k[i, j] and Z_k[j, i] agree bit for bit.  Any nf and nn: the
// 1 x 1 cliques of an LP and a 152 x 152 block from an inner dimension of 2 alike.  The column chunk is capped, so a wide
// front is hundreds of items and not a few waves walking every column.
// k_cdec_mm: 64 x 64 tiles on v_mfma_f64_16x16x4 (gemm_tile64) over a host-built list of (clique, row tile, column tile)
// with row tile >= column tile, the tiles of the large fronts first.  The loaders apply the mask m >= c under the
// condition of the load; the inner dimension of column tile ct stops at min(nn, 64 (ct + 1)), beyond which Pt[j, c] is
// zero for every j of the tile.  An element m >= n of a tile is stored in place and, for m > n, transposed: the strict
// upper half that a diagonal tile computes is dropped, so the two triangles hold the same bits here too.
// Both kernels are launched under borrowed kernel ids (KID_syr2k_fma, KID_syr2k_mm): the profile hooks time them as
// k_syr2k_fma and k_syr2k_mm; the launch census (csp_census_*) and SMCP_TRACE=1 name them k_cdec_fma and k_cdec_mm.
#include <hip/hip_runtime.h>

namespace smcp {

struct CdecArgs {
  const CliqueDesc* cl;
  const int64_t* qptr;
  const int32_t* items;    // k_cdec_fma: (clique, row chunk, column chunk, 0) quadruples
  int nitems;
  const int32_t* tiles;    // k_cdec_mm: (clique, row tile, column tile, 0) quadruples, row tile >= column tile
  const double* L;
  double* Z;
};

constexpr int CDEC_WAVES = 4;        // items per workgroup
constexpr int CDEC_JC = 16;          // output columns per item of k_cdec_fma

// Rows [64 chunk, 64 chunk + 64) x columns [JC cchunk, JC cchunk + JC) of the block of one clique; lane = output row.  Per
// group of four inner indices every load is issued up front and unconditionally, at indices clamped into the owned part of
// the panel (row max(m, c) of column c), and masked afterwards.  No lane leaves before the end: all 64 hold column values.
__global__ void __launch_bounds__(64 * CDEC_WAVES) k_cdec_fma(CdecArgs a) {
  const int lane = threadIdx.x & 63;
  const int it = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * CDEC_WAVES + (threadIdx.x >> 6)));
  if (it >= a.nitems) return;
  const int4 item = reinterpret_cast<const int4*>(a.items)[it];
  const CliqueDesc d = a.cl[item.x];
  const int nn = d.nn, nf = nn + d.na;
  const int i = 64 * item.y + lane, j0 = CDEC_JC * item.z;
  const int nj = min(CDEC_JC, nf - j0);
  const bool live = i < nf;
  const int ic = min(i, nf - 1);
  // the last inner index any entry of the item takes, plus one: min(i, j, nn - 1) over its rows and columns
  const int cend = min(nn, min(min(64 * item.y + 63, nf - 1), j0 + nj - 1) + 1);
  const double* P = a.L + d.blk;
  const int j = j0 + (lane & 15), jc = min(j, nf - 1);
  double acc[CDEC_JC];
#pragma unroll
  for (int jj = 0; jj < CDEC_JC; ++jj) acc[jj] = 0.0;
  for (int c0 = 0; c0 < cend; c0 += 4) {
    double pi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = min(c0 + r, nn - 1);
      const double v = P[max(ic, c) + (int64_t)c * nf];
      pi[r] = (live && i >= c0 + r) ? v : 0.0;
    }
    const int cq = c0 + (lane >> 4), cqc = min(cq, nn - 1);
    const double w = P[max(jc, cqc) + (int64_t)cqc * nf];
    const double pj = (j < nf && j >= cq) ? w : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (c0 + r < cend) {                    // (wave-uniform: an index past the last one is left out, not multiplied by zero)
#pragma unroll
        for (int jj = 0; jj < CDEC_JC; ++jj) acc[jj] = fma(pi[r], syr2k_lane(pj, 16 * r + jj), acc[jj]);
      }
    }
  }
  double* Zk = a.Z + a.qptr[item.x] + ic + (int64_t)j0 * nf;
#pragma unroll
  for (int jj = 0; jj < CDEC_JC; ++jj)
    if (live && jj < nj) Zk[(int64_t)jj * nf] = acc[jj];
}

__global__ void __launch_bounds__(256, 4) k_cdec_mm(CdecArgs a) {
  __shared__ double sA[LKC * LSA], sB[LT * LSB];
  const int4 t = reinterpret_cast<const int4*>(a.tiles)[blockIdx.x];
  const CliqueDesc d = a.cl[t.x];
  const int nn = d.nn, nf = nn + d.na;
  const int m0 = t.y * LT, n0 = t.z * LT;
  const double* P = a.L + d.blk;
  d4 acc[2][2];
  tile64_zero(acc);
  // (a load above the diagonal of the N N block is not issued: the condition is the loader's own)
  gemm_tile64(acc, nf, nf, min(nn, n0 + LT), m0, n0, [=](int m, int kk) { return kk <= m ? P[m + (int64_t)kk * nf] : 0.0; },
              [=](int kk, int n) { return kk <= n ? P[n + (int64_t)kk * nf] : 0.0; }, sA, sB);
  double* Zk = a.Z + a.qptr[t.x];
  tile64_foreach(acc, m0, n0, nf, nf, [=](int m, int n, double v) {
    if (m >= n) {
      Zk[m + (int64_t)n * nf] = v;
      if (m > n) Zk[n + (int64_t)m * nf] = v;
    }
  });
}

}  // namespace smcp
