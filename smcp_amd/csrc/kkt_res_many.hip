// The KKT residual for a block of iterates: kkt_residual_many / kkt_update_many; included by capi.hip after kkt_many.hip.
// Row r of the block is the kkt_res of the reference (src/python/solvers.py:401-411) with the four norms of its DEBUG check
// (534-538):
//   RX_r = -kk * W^-1(XS_r) + Aadj(YS_r) - BX_r,   RY_r = Amap(XS_r) - BY_r,
//   norms[4 r ..] = ||RX_r||, ||RY_r||, ||BX_r||, ||BY_r||    (trace inner product of csp_dot on the blkvals),
// every stage ONE launch sequence for all rows of a chunk: a strided copy XS -> RX, the inverse Hessian in place (hessian_impl, which
// already carries a right-hand-side grid dimension), ONE pass over the rows that forms RX and the weighted squares of RX and BX,
// k_amap with the row dimension, one small kernel for RY and its two sums, one fixed-order final pass that takes the square roots.
// Aadj touches rnnz << blklen positions: the pass finds them through an inverse position table (blkval position -> index into
// rpos, -1 elsewhere; 4 bytes per position, built once per constraint set), so that the rows are passed over ONCE after the
// Hessian and nothing is read back.

namespace {

using namespace smcp;

constexpr int RES_NT = 256;          // threads of every kernel of this file
constexpr int RES_MAXWG = 512;       // most workgroups per row of the combine pass (= most partial sums per row and quantity)

typedef double res_d2 __attribute__((ext_vector_type(2)));
typedef int32_t res_i2 __attribute__((ext_vector_type(2)));

// workgroups per row of the flat combine pass: a function of blklen alone (the partition of the positions is fixed by the shape);
// a thread takes pairs of positions, four of them where the row is long enough
int res_flat_wgs(int64_t bl) {
  const int64_t pairs = (bl + 1) / 2;
  return (int)std::max<int64_t>(1, std::min<int64_t>(RES_MAXWG, (pairs + 4 * RES_NT - 1) / (4 * RES_NT)));
}
// doubles of the partial-sum buffer of a context: per row of a chunk two quantities (RX, BX) of RES_MAXWG partial sums and the two
// sums of the RY kernel
int64_t res_ws_doubles(int64_t rows) { return rows * (2 * RES_MAXWG + 2); }

// rinv[rpos[q]] = q (the table is -1 everywhere else: memset before the launch)
__global__ void __launch_bounds__(RES_NT) k_res_inv_table(int64_t rnnz, const int64_t* rpos, int32_t* rinv) {
  const int64_t q = (int64_t)blockIdx.x * RES_NT + threadIdx.x;
  if (q < rnnz) rinv[rpos[q]] = (int32_t)q;
}

// entry q of Aadj(y): the sum of k_aadj, in its order
__device__ inline double res_aadj(int32_t q, const int64_t* rptr, const int32_t* rcon, const double* rval, const double* y) {
  double acc = 0.0;
  for (int64_t e = rptr[q]; e < rptr[q + 1]; ++e) acc += rval[e] * y[rcon[e]];
  return acc;
}
// one position: r = (-kk w + Aadj(y)) - b; the weighted squares of r and b go to ax / ab (wt: 1 diagonal, 2 below it, 0 for the
// slots above the diagonal, which are not summed whatever they hold).  Explicit fma: the vector and the scalar form of the pass
// must round alike.
__device__ inline double res_elem(double w, double b, double wt, int32_t q, double kk, const int64_t* rptr, const int32_t* rcon,
                                  const double* rval, const double* y, double& ax, double& ab) {
  const double a = q >= 0 ? res_aadj(q, rptr, rcon, rval, y) : 0.0;
  const double r = fma(-kk, w, a) - b;
  if (wt != 0.0) {
    ax = fma(wt * r, r, ax);
    ab = fma(wt * b, b, ab);
  }
  return r;
}
__device__ inline double res_weight(double s) { return s == 0.0 ? 0.0 : (s == 1.0 ? 1.0 : 2.0); }      // from sw = sqrt(weight)

// sum of v over the workgroup in a fixed order (lanes by halving, then the wavefronts in ascending order); valid in thread 0.
// sh: RES_NT / 64 doubles.  Ends with a barrier: sh may be used again.
__device__ inline double res_block_sum(double v, double* sh) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < RES_NT / 64; ++w) s += sh[w];
  __syncthreads();
  return s;
}

// The fused combine over the flat blkval, row r = blockIdx.y: RX_r <- -kk RX_r + Aadj(YS_r) - BX_r (RX_r holds W^-1(XS_r)), weights
// from sw.  A thread takes the positions 2 p, 2 p + 1 with one 16-byte access per array where the row's two pointers are
// 16-byte aligned (sw and rinv always are), two 8-byte ones otherwise -- the same positions, the same order, the same bits.
// part (null: no sums): workgroup b's sums of row r at part[(2 r) * gridDim.x + b] (RX) and part[(2 r + 1) * gridDim.x + b] (BX).
__global__ void __launch_bounds__(RES_NT) k_res_combine(int64_t bl, const double* sw, const int32_t* rinv, const int64_t* rptr,
                                                        const int32_t* rcon, const double* rval, const double* YS, int64_t ldys,
                                                        const double* BX, int64_t ldbx, double* RX, int64_t ldrx, double kk, double* part) {
  __shared__ double sh[RES_NT / 64];
  const int r = blockIdx.y;
  double* const rx = RX + (int64_t)r * ldrx;
  const double* const bx = BX + (int64_t)r * ldbx;
  const double* const y = YS + (int64_t)r * ldys;
  const bool vec = ((((uintptr_t)rx) | ((uintptr_t)bx)) & 15) == 0;
  const int64_t npair = (bl + 1) >> 1;
  double ax = 0.0, ab = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * RES_NT + threadIdx.x; p < npair; p += (int64_t)gridDim.x * RES_NT) {
    const int64_t e = 2 * p;
    if (e + 1 < bl) {
      const res_d2 s = *reinterpret_cast<const res_d2*>(sw + e);
      const res_i2 q = *reinterpret_cast<const res_i2*>(rinv + e);
      res_d2 w, b;
      if (vec) {
        w = *reinterpret_cast<const res_d2*>(rx + e);
        b = *reinterpret_cast<const res_d2*>(bx + e);
      } else {
        w.x = rx[e]; w.y = rx[e + 1];
        b.x = bx[e]; b.y = bx[e + 1];
      }
      res_d2 o;
      o.x = res_elem(w.x, b.x, res_weight(s.x), q.x, kk, rptr, rcon, rval, y, ax, ab);
      o.y = res_elem(w.y, b.y, res_weight(s.y), q.y, kk, rptr, rcon, rval, y, ax, ab);
      if (vec) *reinterpret_cast<res_d2*>(rx + e) = o;
      else { rx[e] = o.x; rx[e + 1] = o.y; }
    } else {
      rx[e] = res_elem(rx[e], bx[e], res_weight(sw[e]), rinv[e], kk, rptr, rcon, rval, y, ax, ab);
    }
  }
  if (!part) return;
  const double sx = res_block_sum(ax, sh);
  const double sb = res_block_sum(ab, sh);
  if (threadIdx.x == 0) {
    part[(int64_t)(2 * r) * gridDim.x + blockIdx.x] = sx;
    part[(int64_t)(2 * r + 1) * gridDim.x + blockIdx.x] = sb;
  }
}
// The same pass clique by clique with the weights from the clique descriptors (the any-size route, where reduce_impl takes
// k_reduce_cliques): workgroup b takes the cliques b, b + gridDim.x, ...
__global__ void __launch_bounds__(RES_NT) k_res_combine_cliques(const CliqueDesc* cl, int nsn, const int32_t* rinv, const int64_t* rptr,
                                                                const int32_t* rcon, const double* rval, const double* YS, int64_t ldys,
                                                                const double* BX, int64_t ldbx, double* RX, int64_t ldrx, double kk,
                                                                double* part) {
  __shared__ double sh[RES_NT / 64];
  const int r = blockIdx.y;
  double* const rx = RX + (int64_t)r * ldrx;
  const double* const bx = BX + (int64_t)r * ldbx;
  const double* const y = YS + (int64_t)r * ldys;
  double ax = 0.0, ab = 0.0;
  for (int k = blockIdx.x; k < nsn; k += gridDim.x) {
    const CliqueDesc d = cl[k];
    const int nn = d.nn, nf = d.nn + d.na;
    for (int e = threadIdx.x; e < nf * nn; e += RES_NT) {
      const int i = e % nf, j = e / nf;
      const int64_t pos = d.blk + e;
      rx[pos] = res_elem(rx[pos], bx[pos], i == j ? 1.0 : (i > j ? 2.0 : 0.0), rinv[pos], kk, rptr, rcon, rval, y, ax, ab);
    }
  }
  if (!part) return;
  const double sx = res_block_sum(ax, sh);
  const double sb = res_block_sum(ab, sh);
  if (threadIdx.x == 0) {
    part[(int64_t)(2 * r) * gridDim.x + blockIdx.x] = sx;
    part[(int64_t)(2 * r + 1) * gridDim.x + blockIdx.x] = sb;
  }
}

// RY_r <- RY_r - BY_r (RY_r holds Amap(XS_r)), r = blockIdx.x, with the sums of squares of the result and of BY_r at ysum[2 r],
// ysum[2 r + 1] (null: no sums)
__global__ void __launch_bounds__(RES_NT) k_res_y(int64_t m, const double* BY, int64_t ldby, double* RY, int64_t ldry, double* ysum) {
  __shared__ double sh[RES_NT / 64];
  const int r = blockIdx.x;
  double* const ry = RY + (int64_t)r * ldry;
  const double* const by = BY + (int64_t)r * ldby;
  double ay = 0.0, ab = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += RES_NT) {
    const double b = by[i], t = ry[i] - b;
    ry[i] = t;
    ay = fma(t, t, ay);
    ab = fma(b, b, ab);
  }
  if (!ysum) return;
  const double sy = res_block_sum(ay, sh);
  const double sb = res_block_sum(ab, sh);
  if (threadIdx.x == 0) { ysum[2 * r] = sy; ysum[2 * r + 1] = sb; }
}

// norms[4 r + 0 .. 3] = sqrt of: the nwg partial sums of RX_r, the sum of RY_r, the partial sums of BX_r, the sum of BY_r;
// r = blockIdx.x, one wavefront per quantity, lane l adds the partial sums l, l + 64, ... in ascending order, then the lanes
// by halving: the same partial sums give the same norm bit for bit
__global__ void __launch_bounds__(RES_NT) k_res_norms(const double* part, int nwg, const double* ysum, double* norms) {
  const int r = blockIdx.x, lane = threadIdx.x & 63, v = threadIdx.x >> 6;
  double s = 0.0;
  if (v == 0 || v == 2) {
    const double* p = part + (int64_t)(2 * r + (v >> 1)) * nwg;
    for (int i = lane; i < nwg; i += 64) s += p[i];
  } else if (lane == 0) {
    s = ysum[2 * r + (v >> 1)];
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) norms[4 * r + v] = sqrt(s);
}

// XS_r <- XS_r - DX_r over the blkval (workgroups x < nbx, pairs of positions as in k_res_combine) and YS_r <- YS_r - DY_r over
// the m entries of the vector (the workgroups behind them), r = blockIdx.y: the update of a refinement round in one launch
__global__ void __launch_bounds__(RES_NT) k_kkt_many_sub(int64_t bl, int64_t m, int nbx, double* XS, int64_t ldxs, const double* DX,
                                                         int64_t lddx, double* YS, int64_t ldys, const double* DY, int64_t lddy) {
  const int r = blockIdx.y;
  if ((int)blockIdx.x >= nbx) {
    double* const y = YS + (int64_t)r * ldys;
    const double* const d = DY + (int64_t)r * lddy;
    for (int64_t i = (int64_t)(blockIdx.x - nbx) * RES_NT + threadIdx.x; i < m; i += (int64_t)(gridDim.x - nbx) * RES_NT) y[i] -= d[i];
    return;
  }
  double* const x = XS + (int64_t)r * ldxs;
  const double* const d = DX + (int64_t)r * lddx;
  const bool vec = ((((uintptr_t)x) | ((uintptr_t)d)) & 15) == 0;
  const int64_t npair = (bl + 1) >> 1;
  for (int64_t p = (int64_t)blockIdx.x * RES_NT + threadIdx.x; p < npair; p += (int64_t)nbx * RES_NT) {
    const int64_t e = 2 * p;
    if (vec && e + 1 < bl) {
      res_d2 a = *reinterpret_cast<const res_d2*>(x + e);
      const res_d2 b = *reinterpret_cast<const res_d2*>(d + e);
      a.x -= b.x; a.y -= b.y;
      *reinterpret_cast<res_d2*>(x + e) = a;
    } else {
      x[e] -= d[e];
      if (e + 1 < bl) x[e + 1] -= d[e + 1];
    }
  }
}

// the inverse position table of the installed constraint set (ConstraintBufs::rinv), built at the first call after
// kkt_set_constraints and released with the constraint buffers
int res_inverse_table(csp_ctx* c, hipStream_t st) {
  DeviceCtx& D = c->D;
  const int64_t bl = c->S.blklen();
  if (D.rinv && D.rinv_len >= bl) return 0;
  if (D.rnnz > (int64_t)0x7fffffff) return SMCP_ENOMEM;
  if (int rc = dev_grow(&D.rinv, &D.rinv_len, bl, D.mem, st)) return rc;
  HIPCHK(hipMemsetAsync(D.rinv, 0xFF, sizeof(int32_t) * bl, st));
  if (D.rnnz)
    launch(c, KID_res_inv_table, k_res_inv_table, dim3((unsigned)((D.rnnz + RES_NT - 1) / RES_NT)), dim3(RES_NT), st, D.rnnz, (const int64_t*)D.rpos, D.rinv);
  // later calls may come on another stream: the table is complete before this one goes on (once per constraint set)
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

}  // namespace

extern "C" {

int kkt_residual_many(csp_ctx* c, const double* L, const double* Y, double kk, const double* XS, int64_t ldxs, const double* YS,
                      int64_t ldys, const double* BX, int64_t ldbx, const double* BY, int64_t ldby, double* RX, int64_t ldrx,
                      double* RY, int64_t ldry, double* norms, int64_t nrhs, void* stream) {
  if (int rc = ready(c)) return rc;
  DeviceCtx& D = c->D;
  const int64_t m = D.m, bl = c->S.blklen();
  if (!m || !L || !Y || !XS || !YS || !BX || !BY || !RX || !RY || nrhs < 1) return SMCP_EINVAL;
  if (nrhs > 1 && (ldxs < bl || ldbx < bl || ldrx < bl || ldys < m || ldby < m || ldry < m)) return SMCP_EINVAL;
  if (c->xr_world > 1) return SMCP_EINVAL;      // a partitioned context holds the factors of its own cliques only
  {
    const int64_t n1 = nrhs - 1;
    const double* const in[6] = {XS, YS, BX, BY, L, Y};
    const int64_t inlen[6] = {ldxs * n1 + bl, ldys * n1 + m, ldbx * n1 + bl, ldby * n1 + m, bl, bl};
    const int64_t rxlen = ldrx * n1 + bl, rylen = ldry * n1 + m;
    if (ranges_overlap(RX, rxlen, RY, rylen)) return SMCP_EINVAL;
    for (int i = 0; i < 6; ++i)
      if (ranges_overlap(RX, rxlen, in[i], inlen[i]) || ranges_overlap(RY, rylen, in[i], inlen[i]) ||
          (norms && ranges_overlap(norms, 4 * nrhs, in[i], inlen[i])))
        return SMCP_EINVAL;
    if (norms && (ranges_overlap(RX, rxlen, norms, 4 * nrhs) || ranges_overlap(RY, rylen, norms, 4 * nrhs))) return SMCP_EINVAL;
  }
  if (D.max_rhs < 1) return SMCP_ENOMEM;
  hipStream_t st = (hipStream_t)stream;
  const int64_t cmax = std::min<int64_t>(D.max_rhs, 65535);      // rows of a chunk: what the Hessian sweeps take (csp_hessian)
  if (int rc = res_inverse_table(c, st)) return rc;
  if (int rc = dev_grow(&D.res_ws, &D.res_len, res_ws_doubles(cmax), D.mem, st)) return rc;
  for (int64_t r = 0; r < nrhs; ++r) invalidate_tags(c, RX + r * ldrx);
  // chol(Y_AA) and the inverse-form factors, as csp_hessian(inv = 1) prepares them: formed only when the cache holds another
  // matrix's, and only then is a verdict read back (or latched, csp_lazy_status)
  HIPCHK(zero_flag(c, st));
  const bool refactor = cache_off() || D.fac_tag != Y;
  if (int rc = prepare_yaa(c, Y, true, st, !use_generic(c))) return rc;
  const bool flat = D.sw && !use_generic(c);                       // the weights: as reduce_impl chooses
  const int nwg = flat ? res_flat_wgs(bl) : (int)std::min<int64_t>(c->S.nsn, RES_MAXWG);
  for (int64_t r0 = 0; r0 < nrhs; r0 += cmax) {
    const int64_t k = std::min(cmax, nrhs - r0);
    const double* const xs = XS + r0 * ldxs;
    const double* const ys = YS + r0 * ldys;
    double* const rx = RX + r0 * ldrx;
    double* const ry = RY + r0 * ldry;
    double* const part = norms ? D.res_ws : nullptr;
    double* const ysum = norms ? D.res_ws + 2 * RES_MAXWG * k : nullptr;
    if (k == 1) HIPCHK(hipMemcpyAsync(rx, xs, sizeof(double) * bl, hipMemcpyDeviceToDevice, st));      // (one row: the leading dimensions may be anything)
    else HIPCHK(hipMemcpy2DAsync(rx, sizeof(double) * ldrx, xs, sizeof(double) * ldxs, sizeof(double) * bl, (size_t)k, hipMemcpyDeviceToDevice, st));
    hessian_impl(c, L, rx, k, ldrx, 2, 1, st);                                                          // W^-1(x)          (403-404)
    if (flat)
      launch(c, KID_res_combine, k_res_combine, dim3((unsigned)nwg, (unsigned)k), dim3(RES_NT), st, bl, (const double*)D.sw, (const int32_t*)D.rinv,
             (const int64_t*)D.rptr, (const int32_t*)D.rcon, (const double*)D.rval, ys, ldys, BX + r0 * ldbx, ldbx, rx, ldrx, kk, part);   // (405-408)
    else
      launch(c, KID_res_combine, k_res_combine_cliques, dim3((unsigned)nwg, (unsigned)k), dim3(RES_NT), st, (const CliqueDesc*)D.cl, (int)c->S.nsn,
             (const int32_t*)D.rinv, (const int64_t*)D.rptr, (const int32_t*)D.rcon, (const double*)D.rval, ys, ldys, BX + r0 * ldbx, ldbx, rx, ldrx, kk, part);
    amap_impl(c, xs, ldxs, (int)k, ry, ldry, st);                                                       // Amap(x)          (410)
    launch(c, KID_res_y, k_res_y, dim3((unsigned)k), dim3(RES_NT), st, m, BY + r0 * ldby, ldby, ry, ldry, ysum);
    if (norms)
      launch(c, KID_res_norms, k_res_norms, dim3((unsigned)k), dim3(RES_NT), st, (const double*)part, nwg, (const double*)ysum, norms + 4 * r0);   // (534-538)
  }
  HIPCHK(end_call(c));
  if (refactor) {
    const int rc = fetch_info(c, st);
    if (rc) D.fac_tag = D.faci_tag = nullptr;
    return rc;
  }
  return 0;
}

int kkt_update_many(csp_ctx* c, double* XS, int64_t ldxs, double* YS, int64_t ldys, const double* DX, int64_t lddx, const double* DY,
                    int64_t lddy, int64_t nrhs, void* stream) {
  if (int rc = ready(c)) return rc;
  const int64_t m = c->D.m, bl = c->S.blklen();
  if (!m || !XS || !YS || !DX || !DY || nrhs < 1) return SMCP_EINVAL;
  if (nrhs > 1 && (ldxs < bl || lddx < bl || ldys < m || lddy < m)) return SMCP_EINVAL;
  {
    const int64_t n1 = nrhs - 1;
    const double* const blk[4] = {XS, YS, DX, DY};
    const int64_t len[4] = {ldxs * n1 + bl, ldys * n1 + m, lddx * n1 + bl, lddy * n1 + m};
    for (int i = 0; i < 2; ++i)
      for (int j = i + 1; j < 4; ++j)
        if (ranges_overlap(blk[i], len[i], blk[j], len[j])) return SMCP_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nbx = res_flat_wgs(bl), nby = (int)std::max<int64_t>(1, std::min<int64_t>(64, (m + RES_NT - 1) / RES_NT));
  for (int64_t r0 = 0; r0 < nrhs; r0 += 65535) {
    const int64_t k = std::min<int64_t>(65535, nrhs - r0);
    launch(c, KID_kkt_many_sub, k_kkt_many_sub, dim3((unsigned)(nbx + nby), (unsigned)k), dim3(RES_NT), st, bl, m, nbx, XS + r0 * ldxs, ldxs,
           DX + r0 * lddx, lddx, YS + r0 * ldys, ldys, DY + r0 * lddy, lddy);
  }
  HIPCHK(end_call(c));
  return 0;
}

}  // extern "C"
