// The Newton-KKT solve for a block of right-hand sides: kkt_solve_many; included by capi.hip after kkt.hip.
// Row r of the block is the system of the solve_ closure of kkt_chol (src/python/solvers.py:506-541, the solve itself at 526):
//   W(bx) -> y = kk * by + Amap(.) -> potrs -> x = -W(bx - Aadj(y)) / kk,
// every stage ONE launch sequence for all rows of a chunk (the Hessian sweeps and k_amap already carry a right-hand-side grid
// dimension; dense_chol.hip has the dense block solve, the kernels below are the three small updates).

namespace {

using namespace smcp;

// X_r[rpos[q]] -= sum over the constraints touching that position of y_r[con] * val  (k_aadj_sub, right-hand side r = blockIdx.y)
__global__ void k_aadj_sub_many(int64_t rnnz, const int64_t* rpos, const int64_t* rptr, const int32_t* rcon, const double* rval,
                                const double* Y, int64_t ldy, double* X, int64_t ldx) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= rnnz) return;
  const double* y = Y + (int64_t)blockIdx.y * ldy;
  double acc = 0.0;
  for (int64_t e = rptr[q]; e < rptr[q + 1]; ++e) acc += rval[e] * y[rcon[e]];
  X[(int64_t)blockIdx.y * ldx + rpos[q]] -= acc;
}
// by_r = kk * by_r + t_r (length m; t_r = Amap(W(bx_r)) at t + r * m), r = blockIdx.y
__global__ void k_kkt_many_y(int64_t m, const double* t, double kk, double* BY, int64_t ldby) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double* y = BY + (int64_t)blockIdx.y * ldby;
  y[i] = 1.0 * t[(int64_t)blockIdx.y * m + i] + kk * y[i];
}
// bx_r *= s over the blkval only (the entries of a row beyond blklen are the caller's), r = blockIdx.y
__global__ void k_kkt_many_scale(int64_t bl, double s, double* BX, int64_t ldbx) {
  double* x = BX + (int64_t)blockIdx.y * ldbx;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < bl; i += (int64_t)gridDim.x * blockDim.x) x[i] = s * x[i];
}

// the largest number c of right-hand sides whose W(bx) (c rows of the stack) and y temporaries (c * m doubles behind them) fit in
// max_rhs rows of blklen doubles: c + ceil(c m / blklen) <= max_rhs; 0: none does
int64_t solve_many_chunk(int64_t m, int64_t bl, int64_t max_rhs) {
  if (m < 1 || bl < 1 || max_rhs < 2) return 0;
  int64_t c = 0;
  while ((c + 1) + ((c + 1) * m + bl - 1) / bl <= max_rhs) ++c;
  return c;
}

}  // namespace

extern "C" {

int64_t kkt_solve_many_chunk(int64_t m, int64_t blklen, int64_t max_rhs) { return solve_many_chunk(m, blklen, max_rhs); }

int kkt_solve_many(csp_ctx* c, const double* L, const double* Y, const double* H, int64_t ldh, double kk, double* BX, int64_t ldbx,
                   double* BY, int64_t ldby, int64_t nrhs, void* stream) {
  if (int rc = ready(c)) return rc;
  DeviceCtx& D = c->D;
  const int64_t m = D.m, bl = c->S.blklen();
  if (!m || !L || !Y || !H || !BX || !BY || nrhs < 1 || ldh < m || (nrhs > 1 && (ldbx < bl || ldby < m))) return SMCP_EINVAL;
  if (c->xr_world > 1) return SMCP_EINVAL;      // a partitioned context holds the factor of its own cliques only (the sharded solve_ is the drivers')
  {
    const int64_t xlen = ldbx * (nrhs - 1) + bl, ylen = ldby * (nrhs - 1) + m, hlen = ldh * (m - 1) + m;
    if (ranges_overlap(BX, xlen, BY, ylen) || ranges_overlap(BX, xlen, H, hlen) || ranges_overlap(BY, ylen, H, hlen)) return SMCP_EINVAL;
  }
  if (D.max_rhs < 2) return SMCP_ENOMEM;
  const int64_t cmax = solve_many_chunk(m, bl, D.max_rhs);
  if (cmax < 1) return SMCP_ENOMEM;
  hipStream_t st = (hipStream_t)stream;
  D.qr_valid = false;          // the rows of the stack are overwritten below
  // a Schur complement that kkt_schur_factor left unfactored (deferred status) is factored where it stands, on this stream
  if (int rc = chol_flush(c, st)) return rc;
  HIPCHK(zero_flag(c, st));
  if (!(c->D.yaa_tag == Y && c->D.yaa_tag)) prepare_yaa(c, Y, false, st);
  if (!use_generic(c)) { if (int rc = prep_lk_cached(c, L, Y, st)) return rc; }
  for (int64_t r0 = 0; r0 < nrhs; r0 += cmax) {
    const int64_t k = std::min(cmax, nrhs - r0);
    double* const U = D.ustack;                  // k rows: W(bx_r)
    double* const ytmp = D.ustack + k * bl;      // k x m: Amap of them
    double* const bx = BX + r0 * ldbx;
    double* const by = BY + r0 * ldby;
    if (k == 1) HIPCHK(hipMemcpyAsync(U, bx, sizeof(double) * bl, hipMemcpyDeviceToDevice, st));      // (one row: ldbx may be anything)
    else HIPCHK(hipMemcpy2DAsync(U, sizeof(double) * bl, bx, sizeof(double) * ldbx, sizeof(double) * bl, (size_t)k, hipMemcpyDeviceToDevice, st));
    hessian_impl(c, L, U, k, bl, 2, 0, st);
    amap_impl(c, U, bl, (int)k, ytmp, m, st);
    launch(c, KID_kkt_many_y, k_kkt_many_y, dim3((unsigned)((m + 255) / 256), (unsigned)k), dim3(256), st, m, (const double*)ytmp, kk, by, ldby);
    if (int rc = potrs_many_impl(c, H, m, ldh, by, k, ldby, st)) return rc;
    if (D.rnnz)
      launch(c, KID_aadj_sub_many, k_aadj_sub_many, dim3((unsigned)((D.rnnz + 255) / 256), (unsigned)k), dim3(256), st, D.rnnz, D.rpos, D.rptr, D.rcon,
             D.rval, (const double*)by, ldby, bx, ldbx);
    hessian_impl(c, L, bx, k, ldbx, 2, 0, st);
    launch(c, KID_kkt_many_scale, k_kkt_many_scale, dim3((unsigned)std::min<int64_t>(1024, (bl + 255) / 256), (unsigned)k), dim3(256), st, bl, -1.0 / kk,
           bx, ldbx);
  }
  HIPCHK(end_call(c));
  return 0;
}

}  // extern "C"
