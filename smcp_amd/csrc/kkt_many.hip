// The Newton-KKT solve for a block of right-hand sides: kkt_solve_many / dense_potrs_many; included by capi.hip after kkt.hip.
// Row r of the block is the system of the solve_ closure of kkt_chol (src/python/solvers.py:506-541, the solve itself at 526):
//   W(bx) -> y = kk * by + Amap(.) -> potrs -> x = -W(bx - Aadj(y)) / kk,
// every stage ONE launch sequence for all rows of a chunk (the Hessian sweeps and k_amap already carry a right-hand-side grid
// dimension; the kernels below add the dense solve and the three small updates).

namespace {

using namespace smcp;

constexpr int PM_CB = 32;        // columns of B per workgroup of the step kernel (blockIdx.y: column block)
constexpr int PM_CBS = 16;       // ... of the one-workgroup kernel, whose LDS holds the whole factor beside them
constexpr int PM_LD = 65;        // leading dimension of the 64 x 64 blocks in LDS

// Row (trans 0: L y = t) or column (trans 1: L^T x = t) `lane` of the bw x bw diagonal block at (jb, jb) of the lower triangular
// A into registers, identity beyond bw -- the operand of wave_trsv16, loaded ONCE for all the columns a wavefront solves
__device__ inline void pm_load_row16(const double* A, int lda, int jb, int bw, int trans, double (&Lr)[16], double& rdii) {
  const int i = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const bool in = i < bw && j < bw && (trans ? j >= i : j <= i);
    Lr[j] = in ? (trans ? A[(jb + j) + (jb + i) * lda] : A[(jb + i) + (jb + j) * lda]) : (i == j ? 1.0 : 0.0);
  }
  double dii = 1.0;
#pragma unroll
  for (int j = 0; j < 16; ++j) if (j == i) dii = Lr[j];
  rdii = 1.0 / dii;
}
// the substitution chain of wave_trsv16 (the same arithmetic in the same order: the single solve_ and a row of the block differ
// in the order of the updates BETWEEN diagonal blocks only); returns entry `lane` of the solution
__device__ inline double pm_chain16(const double (&Lr)[16], double rdii, double ti, int trans) {
  const int i = threadIdx.x & 63;
  double xi = 0.0;
  if (!trans) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const double xj = __shfl(ti * rdii, j, 64);
      if (i == j) xi = xj;
      if (i > j) ti -= Lr[j] * xj;
    }
  } else {
#pragma unroll
    for (int j = 15; j >= 0; --j) {
      const double xj = __shfl(ti * rdii, j, 64);
      if (i == j) xi = xj;
      if (i < j) ti -= Lr[j] * xj;
    }
  }
  return xi;
}

// T (nb x kc, column c at T + c * ldt, in LDS) <- solution of L T' = T (trans 0) or L^T T' = T (trans 1) with the lower
// triangular nb x nb block Ls (LDS, leading dimension ld), by the whole workgroup (256 threads): 16-wide sub-blocks, the
// diagonal sub-block by substitution (wavefront v takes the columns v, v + 4, ... -- a column never meets another one's
// numbers), then the other rows of the block, one (row, column) pair per thread, sixteen products in ascending order.
// Ends with a barrier.  The caller has synchronised after filling Ls and T.
__device__ inline void pm_block_solve(const double* Ls, int ld, int nb, double* T, int ldt, int kc, int trans) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nsb = (nb + 15) >> 4;
  for (int q = 0; q < nsb; ++q) {
    const int sb = trans ? nsb - 1 - q : q;            // forward: top sub-block first; transposed: bottom first
    const int s0 = 16 * sb, bw = min(16, nb - s0);
    if (wave < kc) {
      double Lr[16], rdii;
      pm_load_row16(Ls, ld, s0, bw, trans, Lr, rdii);
      for (int cc = wave; cc < kc; cc += 4) {
        const double v = pm_chain16(Lr, rdii, lane < bw ? T[s0 + lane + cc * ldt] : 0.0, trans);
        if (lane < bw) T[s0 + lane + cc * ldt] = v;
      }
    }
    __syncthreads();
    const int base = trans ? 0 : s0 + bw, nrem = trans ? s0 : nb - s0 - bw;
    for (int e = tid; e < nrem * kc; e += 256) {
      const int i = base + e % nrem, cc = e / nrem;
      const double* x = T + s0 + cc * ldt;
      double acc = 0.0;
      if (!trans) for (int j = 0; j < bw; ++j) acc += Ls[i + (s0 + j) * ld] * x[j];
      else for (int j = 0; j < bw; ++j) acc += Ls[(s0 + j) + i * ld] * x[j];
      T[i + cc * ldt] -= acc;
    }
    __syncthreads();
  }
}

// A Z = B for nrhs columns with the Cholesky factor A (lower, n <= 128) in ONE launch: workgroup g takes the columns
// 16 g .. 16 g + 15 with the lower triangle of the factor in LDS (n (n | 1) doubles, the layout of k_dense_potrs_small) beside them
// (16 x n doubles).  Only the lower triangle of A is read; A and the entries of B beyond n are not written.
__global__ void __launch_bounds__(256) k_potrs_many_small(const double* Ag, int n, int64_t ldag, double* B, int nrhs, int64_t ldb) {
  extern __shared__ __attribute__((aligned(16))) double pms[];
  const int tid = threadIdx.x, ld = n | 1;
  double* const A = pms;
  double* const T = pms + n * ld;
  const int c0 = blockIdx.x * PM_CBS, kc = min(PM_CBS, nrhs - c0);
  for (int e = tid; e < n * n; e += 256) {
    const int i = e % n, j = e / n;
    if (i >= j) A[i + j * ld] = Ag[i + (int64_t)j * ldag];
  }
  for (int e = tid; e < n * kc; e += 256) T[e] = B[e % n + (int64_t)(c0 + e / n) * ldb];
  __syncthreads();
  pm_block_solve(A, ld, n, T, n, kc, 0);
  pm_block_solve(A, ld, n, T, n, kc, 1);
  for (int e = tid; e < n * kc; e += 256) B[e % n + (int64_t)(c0 + e / n) * ldb] = T[e];
}

// One block step of the blocked triangular solves for a BLOCK of right-hand sides (k_dense_trsv_step generalised): the 64-wide
// block column jb of the factor A (lower, n x n), w = min(64, n - jb) of it.  Workgroup (x, y) takes the columns 32 y .. of
// the right-hand sides.  Every workgroup solves the diagonal block for its columns redundantly (pm_block_solve on a copy in
// LDS); the workgroups x = 0 store the solved block to dst; then workgroup x updates ITS 64 rows of the other rows of src
// with its 64 x 64 tile of the factor, fetched to registers before the solve and passed through LDS, so that every entry of
// the factor is read once per triangle and column block:
//   trans 0 (L Y = B):    src[i, :] -= A[i, jb : jb + w] Z,      i = jb + 64 + 64 x ..    (w = 64 whenever rows remain)
//   trans 1 (L^T Z = Y):  src[i, :] -= A[jb : jb + w, i]^T Z,    i = 64 x ..  < jb
// One thread per (row, column) pair, 64 products in ascending order -- or, with mm and eight columns or more, one 16 x 16 tile
// of the result per wavefront and sixteen columns on the matrix cores: a fixed summation order either way.  The steps are separate launches
// (the block below needs every update of this one): no workgroup waits for another.
// src / dst: columns at multiples of lds_ / ldd.  Forward: src = B, dst = the scratch; backward: src = the scratch, dst = B.
__global__ void __launch_bounds__(256) k_potrs_many_step(const double* A, int n, int64_t lda, int jb, int w, double* src, int64_t lds_,
                                                         double* dst, int64_t ldd, int nrhs, int trans, int mm) {
  __shared__ double Ds[64 * PM_LD];          // the diagonal block; after the solve this workgroup's tile of the factor:
  double* const As = Ds;                     // As[r + 65 j] multiplies Z[j] for row r (pm_block_solve ends with a barrier)
  __shared__ double T[PM_CB * 64];           // the right-hand sides of the block, then its solution
  const int tid = threadIdx.x;
  const int c0 = blockIdx.y * PM_CB, kc = min(PM_CB, nrhs - c0);
  const int r0 = trans ? 64 * (int)blockIdx.x : jb + w + 64 * (int)blockIdx.x;     // first row of the tile
  const bool tile = trans ? r0 < jb : r0 < n;
  double pre[16];
  if (tile) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int e = tid + 256 * q, a = e & 63, b = e >> 6;
      // forward: a = row of the tile, b = column of the block; transposed: a = row of the block, b = row (column of A) of the tile
      if (!trans) pre[q] = (r0 + a < n && b < w) ? A[(r0 + a) + (int64_t)(jb + b) * lda] : 0.0;
      else pre[q] = (a < w) ? A[(jb + a) + (int64_t)(r0 + b) * lda] : 0.0;
    }
  }
  for (int e = tid; e < 64 * 64; e += 256) {
    const int i = e & 63, j = e >> 6;
    Ds[i + j * PM_LD] = (i < w && j < w && i >= j) ? A[(jb + i) + (int64_t)(jb + j) * lda] : (i == j ? 1.0 : 0.0);
  }
  for (int e = tid; e < 64 * kc; e += 256) {
    const int i = e & 63, cc = e >> 6;
    T[e] = i < w ? src[(jb + i) + (int64_t)(c0 + cc) * lds_] : 0.0;
  }
  __syncthreads();
  pm_block_solve(Ds, PM_LD, w, T, 64, kc, trans);
  if (blockIdx.x == 0)
    for (int e = tid; e < 64 * kc; e += 256) {
      const int i = e & 63, cc = e >> 6;
      if (i < w) dst[(jb + i) + (int64_t)(c0 + cc) * ldd] = T[e];
    }
  if (!tile) return;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int e = tid + 256 * q, a = e & 63, b = e >> 6;
    if (!trans) As[a + b * PM_LD] = pre[q];
    else As[b + a * PM_LD] = pre[q];
  }
  __syncthreads();
  if (mm && kc >= 8) {
    // tile products (v_mfma_f64_16x16x4, operand map of fmma in front_fam.hip): wavefront v takes the rows 16 v .. 16 v + 15 of the
    // tile, one 16 x 16 result tile per sixteen columns of Z, sixteen k-steps in ascending order.  A column of the result is a
    // function of its own column of Z only (the columns >= kc of T are never stored).
    const int lane = tid & 63, l15 = lane & 15, kq = lane >> 4, v = tid >> 6;
    double av[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) av[s] = As[(16 * v + l15) + (kq + 4 * s) * PM_LD];
    for (int cb = 0; 16 * cb < kc; ++cb) {
      d4 acc = {0.0, 0.0, 0.0, 0.0};
      const double* z = T + 64 * (16 * cb + l15) + kq;
#pragma unroll
      for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(z[4 * s], av[s], acc, 0, 0, 0);
      const int i = r0 + 16 * v + l15;
      if (trans ? i < jb : i < n) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int cc = 16 * cb + kq + 4 * rr;
          if (cc < kc) src[i + (int64_t)(c0 + cc) * lds_] -= acc[rr];
        }
      }
    }
    return;
  }
  const int r = tid & 63, i = r0 + r;
  if (trans ? i < jb : i < n)
    for (int cc = tid >> 6; cc < kc; cc += 4) {
      const double* z = T + 64 * cc;
      double acc = 0.0;
#pragma unroll 8
      for (int j = 0; j < 64; ++j) acc += As[r + j * PM_LD] * z[j];
      src[i + (int64_t)(c0 + cc) * lds_] -= acc;
    }
}

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

bool ranges_overlap(const double* a, int64_t alen, const double* b, int64_t blen) {
  const uintptr_t a0 = (uintptr_t)a, a1 = (uintptr_t)(a + alen), b0 = (uintptr_t)b, b1 = (uintptr_t)(b + blen);
  return a0 < b1 && b0 < a1;
}

// The two halves of the blocked solve beyond n = 128, ceil(n / 64) block steps each (potrs_many_impl runs one after the other;
// kkt_qr_solve_many puts its update of the forward solution between them).  Yw: n x nrhs, leading dimension n.
// forward: Yw <- L^-1 B (the rows of B below each solved block are updated in place)
void potrs_many_fwd(csp_ctx* c, const double* A, int64_t n, int64_t lda, double* B, int64_t nrhs, int64_t ldb, double* Yw, int mm, hipStream_t st) {
  const unsigned ncb = (unsigned)((nrhs + PM_CB - 1) / PM_CB);
  for (int jb = 0; jb < (int)n; jb += LB) {
    const int w = (int)std::min<int64_t>(LB, n - jb);
    const int rest = (int)n - jb - w;
    launch(c, KID_potrs_many_step, k_potrs_many_step, dim3((unsigned)std::max(1, (rest + 63) / 64), ncb), dim3(256), st, A, (int)n, lda, jb, w, B, ldb,
           Yw, n, (int)nrhs, 0, mm);
  }
}
// backward: B <- L^-T Yw (the rows of Yw above each solved block are updated in place)
void potrs_many_bwd(csp_ctx* c, const double* A, int64_t n, int64_t lda, double* B, int64_t nrhs, int64_t ldb, double* Yw, int mm, hipStream_t st) {
  const unsigned ncb = (unsigned)((nrhs + PM_CB - 1) / PM_CB);
  const int64_t nblocks = (n + LB - 1) / LB;
  for (int jb = (int)((nblocks - 1) * LB); jb >= 0; jb -= LB) {
    const int w = (int)std::min<int64_t>(LB, n - jb);
    launch(c, KID_potrs_many_step, k_potrs_many_step, dim3((unsigned)std::max(1, jb / 64), ncb), dim3(256), st, A, (int)n, lda, jb, w, Yw, n,
           B, ldb, (int)nrhs, 1, mm);
  }
}

// L L^T Z = B for a block: n <= 128 one launch, beyond 2 ceil(n / 64) block steps over the chip -- whatever nrhs is.
int potrs_many_impl(csp_ctx* c, const double* A, int64_t n, int64_t lda, double* B, int64_t nrhs, int64_t ldb, hipStream_t st) {
  DeviceCtx& D = c->D;
  if (n <= 2 * LB) {
    static bool attr = false;
    if (!attr) attr = hipFuncSetAttribute((const void*)k_potrs_many_small, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024) == hipSuccess;
    const size_t lds = ((size_t)n * (n | 1) + (size_t)PM_CBS * n) * sizeof(double);
    launch_lds(c, KID_potrs_many_small, k_potrs_many_small, dim3((unsigned)((nrhs + PM_CBS - 1) / PM_CBS)), dim3(256), lds, st, A, (int)n, lda, B,
               (int)nrhs, ldb);
    return 0;
  }
  // the forward solution lives in the scratch image of csp_trsm / csp_trmm (no call keeps it): n x nrhs, leading dimension n
  if (int rc = dev_grow(&D.trsm_x, &D.trsm_x_len, n * nrhs, D.mem, st)) return rc;
  double* const Yw = D.trsm_x;
  // the updates of the other rows: FMA below eight columns of a workgroup's block, tile products on the matrix cores from eight on
  // (the gate of csp_trmm / csp_symm); SMCP_POTRS_MANY_MM=0: FMA only.  Read on every call: tools/solve_many_time.py alternates the two
  const int mm = (sw_int("SMCP_POTRS_MANY_MM", 1) && !use_generic(c)) ? 1 : 0;
  potrs_many_fwd(c, A, n, lda, B, nrhs, ldb, Yw, mm, st);
  potrs_many_bwd(c, A, n, lda, B, nrhs, ldb, Yw, mm, st);
  return 0;
}

}  // namespace

extern "C" {

int64_t kkt_solve_many_chunk(int64_t m, int64_t blklen, int64_t max_rhs) { return solve_many_chunk(m, blklen, max_rhs); }

int dense_potrs_many(csp_ctx* c, const double* A, int64_t n, int64_t lda, double* B, int64_t nrhs, int64_t ldb, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!A || !B || n < 1 || n > (int64_t)0x7fffffff || lda < n || nrhs < 1 || nrhs > (int64_t)PM_CB * 65535 || (nrhs > 1 && ldb < n)) return SMCP_EINVAL;
  if (ranges_overlap(A, lda * (n - 1) + n, B, ldb * (nrhs - 1) + n)) return SMCP_EINVAL;
  if (int rc = flush_pending_potrf(c, (hipStream_t)stream, A, false)) return rc;
  if (int rc = potrs_many_impl(c, A, n, lda, B, nrhs, ldb, (hipStream_t)stream)) return rc;
  HIPCHK(end_call(c));
  return 0;
}

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
  if (int rc = flush_pending_potrf(c, st, nullptr, false)) return rc;
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
