// Dense Cholesky of the Schur complement H: potrf / potrs (lapack.potrf / potrs of kkt_chol, src/python/solvers.py:501, 526) --
// every kernel, the host drivers, the C-ABI entry points dense_potrf / dense_potrs / dense_potrs_many, and the ONLY code that
// touches DeviceCtx::chol (context.hpp: which matrix waits for its factorisation, which factor was made here).  Included by
// capi.hip ahead of its extern "C" part; kkt.hip, kkt_many.hip and kkt_qr_many.hip call in here.

namespace {

using namespace smcp;

// single-workgroup dense Cholesky / triangular solves (generic path)
__global__ void k_dense_potrf(double* A, int n, int64_t lda, int* info) {
  int f = wg::potrf(n, A, lda);
  if (f && threadIdx.x == 0) *info = f;
}
__global__ void k_dense_potrs(const double* A, int n, int64_t lda, double* B, int nrhs, int64_t ldb) {
  wg::trsm_llN(n, nrhs, A, lda, B, ldb);
  wg::trsm_llT(n, nrhs, A, lda, B, ldb);
}
// threads of the one-workgroup factorisation of H (SMCP_POTRF_THREADS, timing studies)
static dim3 potrf_blk() {
  static int t = 0;
  if (!t) { const char* e = sw_str("SMCP_POTRF_THREADS"); t = e ? atoi(e) : 1024; if (t < 64 || t > 1024 || (t & 63)) t = 1024; }
  return dim3(t);
}
// m <= 128: the whole factorisation in the LDS of one workgroup -- 16-wide block columns, diagonal blocks factored
// and inverted by one wavefront (potrf_inv16), panel and trailing updates on MFMA (the scheme of k_factor_yaa_lds).
// The inverse of a diagonal block (D16) is the operand of its panel update and lives in LDS only: the solves substitute.
__global__ void __launch_bounds__(1024) k_dense_potrf_small(double* A, int n, int64_t lda, int* info) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int ld = n | 1;
  double* const M = smem;
  double* const D16 = smem + (int64_t)ld * n;
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
    const int i = e % n, j = e / n;
    M[i + j * ld] = (i >= j) ? A[i + (int64_t)j * lda] : 0.0;
  }
  for (int jb = 0; jb < n; jb += 16) {
    const int bw = min(16, n - jb);
    const int f = potrf_inv16(M + jb + jb * ld, ld, bw, D16);
    if (f) { if (threadIdx.x == 0) *info = jb + f; return; }
    const int mrem = n - jb - bw;
    if (mrem > 0) {
      double* Pj = M + (jb + bw) + jb * ld;
      wg_mma(mrem, bw, bw, [=](int m, int kk) { return Pj[m + kk * ld]; },
             [=](int kk, int nn_) { return D16[nn_ + kk * 16]; },
             [=](int m, int nn_, double acc) { Pj[m + nn_ * ld] = acc; });
      __syncthreads();
      double* Tr = M + (jb + bw) + (jb + bw) * ld;
      wg_mma(mrem, mrem, bw, [=](int m, int kk) { return Pj[m + kk * ld]; },
             [=](int kk, int nn_) { return Pj[nn_ + kk * ld]; },
             [=](int m, int nn_, double acc) { if (m >= nn_) Tr[m + nn_ * ld] -= acc; }, true);
      __syncthreads();
    }
  }
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
    const int i = e % n, j = e / n;
    if (i >= j) A[i + (int64_t)j * lda] = M[i + j * ld];
  }
}
// Triangular solve with one 16 x 16 (bw x bw) diagonal block of the factor by ONE wavefront, by substitution
// (backward stable; multiplying by the explicit block inverse costs the interior-point endgame several digits), in two parts
// so that a wavefront that solves several columns loads the block once.
// trsv16_load: row (trans 0: L y = t) or column (trans 1: L^T x = t) `lane` of the block at (jb, jb) of the lower triangular A
// into registers, identity beyond bw, and the reciprocal of its diagonal entry.  LD: int for a factor in LDS, int64_t in global
// memory (the index arithmetic is LD's).
template <typename LD>
__device__ inline void trsv16_load(const double* A, LD lda, int jb, int bw, int trans, double (&Lr)[16], double& rdii) {
  const int i = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const bool in = i < bw && j < bw && (trans ? j >= i : j <= i);
    Lr[j] = in ? (trans ? A[(jb + j) + (jb + i) * lda] : A[(jb + i) + (jb + j) * lda]) : (i == j ? 1.0 : 0.0);
  }
  double dii = 1.0;
#pragma unroll
  for (int j = 0; j < 16; ++j) if (j == i) dii = Lr[j];
  // one division per lane and block: a division inside each of the sixteen dependent steps was most of the chain
  // (k_dense_potrs_small: 41 us at m = 100 whether the factor came from LDS or from global memory)
  rdii = 1.0 / dii;
}
// trsv16_chain: the substitution; lane i holds entry i of the right-hand side (ti), the solved entries are broadcast with shuffles.
// Returns entry `lane` of the solution.  (A single solve_ and a row of a block differ in the order of the updates BETWEEN blocks only.)
__device__ inline double trsv16_chain(const double (&Lr)[16], double rdii, double ti, int trans) {
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
// ... and one column: load and chain
__device__ inline double wave_trsv16(const double* A, int64_t lda, int jb, int bw, double ti, int trans) {
  double Lr[16], rdii;
  trsv16_load(A, lda, jb, bw, trans, Lr, rdii);
  return trsv16_chain(Lr, rdii, ti, trans);
}
// A x = b with the factor of k_dense_potrf_small (one right-hand side, one workgroup, n <= 128).  The factor is copied to
// LDS first (dynamic: n (n | 1) doubles): the 2 ceil(n / 16) block steps each read their diagonal block and the columns
// below / beside it, and from global memory every step was two dependent round trips (41 us at m = 100, twice per solve_
// of the interior-point iteration ... once per solve_); from LDS the steps are the substitution chains alone.
__global__ void __launch_bounds__(256) k_dense_potrs_small(const double* Ag, int n, int64_t ldag, double* b) {
  extern __shared__ __attribute__((aligned(16))) double sAf[];
  __shared__ double x[128], t[16];
  const int tid = threadIdx.x;
  const int lda = n | 1;
  double* const A = sAf;
  for (int e = tid; e < n * n; e += 256) {
    const int i = e % n, j = e / n;
    if (i >= j) A[i + j * lda] = Ag[i + (int64_t)j * ldag];
  }
  if (tid < n) x[tid] = b[tid];
  __syncthreads();
  for (int jb = 0; jb < n; jb += 16) {            // L y = b
    const int bw = min(16, n - jb);
    if (tid < 64) {
      const double v = wave_trsv16(A, lda, jb, bw, tid < bw ? x[jb + tid] : 0.0, 0);
      if (tid < bw) t[tid] = v;
    }
    __syncthreads();
    if (tid < bw) x[jb + tid] = t[tid];
    const int i = jb + bw + tid;
    if (i < n) { double acc = 0.0; for (int j = 0; j < bw; ++j) acc += A[i + (int64_t)(jb + j) * lda] * t[j]; x[i] -= acc; }
    __syncthreads();
  }
  for (int jb = ((n - 1) >> 4) << 4; jb >= 0; jb -= 16) {   // L^T x = y
    const int bw = min(16, n - jb);
    if (tid < 64) {
      const double v = wave_trsv16(A, lda, jb, bw, tid < bw ? x[jb + tid] : 0.0, 1);
      if (tid < bw) t[tid] = v;
    }
    __syncthreads();
    if (tid < bw) x[jb + tid] = t[tid];
    if (tid < jb) { double acc = 0.0; for (int j = 0; j < bw; ++j) acc += A[(jb + j) + (int64_t)tid * lda] * t[j]; x[tid] -= acc; }
    __syncthreads();
  }
  if (tid < n) b[tid] = x[tid];
}

// One block step of the blocked triangular solves with the Cholesky factor A (lower, n x n).  Every workgroup
// solves the 64-wide diagonal block redundantly (four 16-wide substitutions by wavefront 0, see wave_trsv16);
// workgroup 0 publishes x_blk to xout; then the workgroups update their slice of the remaining rows:
//   trans 0 (L y = b):    b[i] -= sum_j A[i, jb + j] x[j],  i >= jb + w   (one thread per row, coalesced)
//   trans 1 (L^T x = y):  b[i] -= sum_j A[jb + j, i] x[j],  i <  jb       (one wave per row, lanes over j)
__global__ void __launch_bounds__(256) k_dense_trsv_step(const double* A, int n, int64_t lda, int jb, int w, double* b, double* xout, int trans) {
  __shared__ double t[64], x[64];
  const int tid = threadIdx.x;
  if (tid < 64) t[tid] = tid < w ? b[jb + tid] : 0.0;
  __syncthreads();
  if (tid < 64) {
    const int nsb = (w + 15) >> 4;
    for (int q = 0; q < nsb; ++q) {
      const int sb = trans ? nsb - 1 - q : q;          // forward: top sub-block first; transposed: bottom first
      const int s0 = 16 * sb, bw = min(16, w - s0);
      const double v = wave_trsv16(A, lda, jb + s0, bw, tid < bw ? t[s0 + tid] : 0.0, trans);
      if (tid < bw) x[s0 + tid] = v;
      // remaining sub-blocks of this diagonal block (same wavefront: LDS traffic is program-ordered)
      if (!trans) {
        const int i = s0 + bw + tid;
        if (i < w) { double acc = 0.0; for (int j = 0; j < bw; ++j) acc += A[(jb + i) + (int64_t)(jb + s0 + j) * lda] * x[s0 + j]; t[i] -= acc; }
      } else {
        if (tid < s0) { double acc = 0.0; for (int j = 0; j < bw; ++j) acc += A[(jb + s0 + j) + (int64_t)(jb + tid) * lda] * x[s0 + j]; t[tid] -= acc; }
      }
    }
    if (blockIdx.x == 0 && tid < w) xout[jb + tid] = x[tid];
  }
  __syncthreads();
  if (!trans) {
    const int i = jb + w + blockIdx.x * 256 + tid;
    if (i < n) {
      double acc = 0.0;
      const double* Ai = A + i + (int64_t)jb * lda;
      for (int j = 0; j < w; ++j) acc += Ai[(int64_t)j * lda] * x[j];
      b[i] -= acc;
    }
  } else {
    const int lane = tid & 63, wave = tid >> 6;
    for (int i = blockIdx.x * 4 + wave; i < jb; i += gridDim.x * 4) {
      double acc = (lane < w) ? A[(jb + lane) + (int64_t)i * lda] * x[lane] : 0.0;
      for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
      if (lane == 0) b[i] -= acc;
    }
  }
}

// A x = b with the Cholesky factor A (lower, n x n, 128 < n <= 1024), ONE right-hand side, in ONE launch of one workgroup:
// the step kernel above is 2 ceil(n / 64) dependent launches of ~21 us (m = 1000, config 4: 32 launches, 0.76 ms per solve_ for
// 8 MB of factor).  Here the chain is 2 ceil(n / 16) steps of one 16-wide substitution by wavefront 0 (wave_trsv16 on the
// diagonal blocks, all of them staged in LDS up front: the same arithmetic, so the same backward-stable solve) followed by
// the update of the other rows, one thread per row, whose sixteen factor entries were fetched a step ahead: the factor is
// static, so its stream never waits for the chain.  x lives in LDS; barriers wait for LDS traffic only.
// (Round 4 tried 64-wide steps through the diagonal blocks' cached inverses, x_blk = Dinv r_blk, the other rows updated in
// four sub-steps of sixteen prefetched columns: 0.62 ms against 0.37 here -- a sub-step is 16 multiply-adds, far shorter
// than the ~2.4 us a request to the 8 MB factor takes, and 128 registers per thread hold only one sub-step ahead, so the
// kernel ran 256 exposed round trips where this one hides its 126 behind the one-wave substitutions.)
constexpr int POTRS1_MAXN = 1024;
__host__ __device__ inline size_t potrs_one_lds(int n) { return ((size_t)((n + 15) & ~15) * 17 + 16) * sizeof(double); }
__global__ void __launch_bounds__(1024) k_dense_potrs_one(const double* A, int n, int64_t lda, double* b) {
  extern __shared__ __attribute__((aligned(16))) double sm1[];
  const int tid = threadIdx.x, npad = (n + 15) & ~15, nblk = npad >> 4;
  double* const x = sm1;
  double* const t = sm1 + npad;              // 16
  double* const dg = t + 16;                 // nblk x 256: the diagonal 16 x 16 blocks (ld 16), identity beyond n
  for (int e = tid; e < nblk * 256; e += 1024) {
    const int blk = e >> 8, r = e & 15, cc = (e >> 4) & 15, i = 16 * blk + r, j = 16 * blk + cc;
    dg[e] = (i < n && j < n && i >= j) ? A[i + (int64_t)j * lda] : (r == cc ? 1.0 : 0.0);
  }
  for (int e = tid; e < npad; e += 1024) x[e] = e < n ? b[e] : 0.0;
  const int i = tid;                         // this thread's row (forward) / column (backward)
  double va[16], vb[16];
  // ---- L y = b
  auto fetch_f = [&](int jb, double (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = (i < n && i >= jb + 16 && jb + j < n) ? A[i + (int64_t)(jb + j) * lda] : 0.0;
  };
  auto step_f = [&](int blk, const double (&cur)[16]) {
    const int jb = 16 * blk;
    if (tid < 64) {
      const double v = wave_trsv16(dg + 256 * blk, 16, 0, 16, tid < 16 ? x[jb + tid] : 0.0, 0);
      if (tid < 16) t[tid] = v;
    }
    lds_barrier();
    if (tid < 16) x[jb + tid] = t[tid];
    if (i >= jb + 16 && i < n) {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < 16; ++j) acc += cur[j] * t[j];
      x[i] -= acc;
    }
    lds_barrier();
  };
  fetch_f(0, va);
  __syncthreads();
  for (int blk = 0; blk < nblk; blk += 2) {
    if (blk + 1 < nblk) fetch_f(16 * (blk + 1), vb);
    step_f(blk, va);
    if (blk + 1 < nblk) {
      if (blk + 2 < nblk) fetch_f(16 * (blk + 2), va);
      step_f(blk + 1, vb);
    }
  }
  // ---- L^T x = y
  auto fetch_b = [&](int jb, double (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = (i < jb && jb + j < n) ? A[(jb + j) + (int64_t)i * lda] : 0.0;
  };
  auto step_b = [&](int blk, const double (&cur)[16]) {
    const int jb = 16 * blk;
    if (tid < 64) {
      const double v = wave_trsv16(dg + 256 * blk, 16, 0, 16, tid < 16 ? x[jb + tid] : 0.0, 1);
      if (tid < 16) t[tid] = v;
    }
    lds_barrier();
    if (tid < 16) x[jb + tid] = t[tid];
    if (i < jb) {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < 16; ++j) acc += cur[j] * t[j];
      x[i] -= acc;
    }
    lds_barrier();
  };
  fetch_b(16 * (nblk - 1), va);
  for (int blk = nblk - 1; blk >= 0; blk -= 2) {
    if (blk >= 1) fetch_b(16 * (blk - 1), vb);
    step_b(blk, va);
    if (blk >= 1) {
      if (blk >= 2) fetch_b(16 * (blk - 2), va);
      step_b(blk - 1, vb);
    }
  }
  if (tid < n) b[tid] = x[tid];
}
// ---- blocks of right-hand sides --------------------------------------------------------------------------------------------
constexpr int PM_CB = 32;        // columns of B per workgroup of the step kernel (blockIdx.y: column block)
constexpr int PM_CBS = 16;       // ... of the one-workgroup kernel, whose LDS holds the whole factor beside them
constexpr int PM_LD = 65;        // leading dimension of the 64 x 64 blocks in LDS
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
      trsv16_load(Ls, ld, s0, bw, trans, Lr, rdii);
      for (int cc = wave; cc < kc; cc += 4) {
        const double v = trsv16_chain(Lr, rdii, lane < bw ? T[s0 + lane + cc * ldt] : 0.0, trans);
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
bool ranges_overlap(const double* a, int64_t alen, const double* b, int64_t blen) {
  const uintptr_t a0 = (uintptr_t)a, a1 = (uintptr_t)(a + alen), b0 = (uintptr_t)b, b1 = (uintptr_t)(b + blen);
  return a0 < b1 && b0 < a1;
}

// ---- DeviceCtx::chol: the functions below and potrf_launch are the only code that reads or writes it -------------------------
// Was the factor at A (order n) made by a factorisation of this context, and is it still its latest?  The gate of the fast
// single-right-hand-side solves: it is what guarantees that the workspace of the step solve exists.
bool chol_made_here(const csp_ctx* c, const void* A, int64_t n) { return c->D.chol.factored.A == A && c->D.chol.factored.n == n; }
// (never in generic mode, whose factors take the generic solve)
void chol_mark_factored(csp_ctx* c, const void* A, int64_t n) { if (!use_generic(c)) c->D.chol.factored = {A, n}; }
// A Schur complement built by kkt_schur_factor under csp_lazy_status is left UNFACTORED until its first use: kkt_solve then
// factors it on a side stream beside its first Hessian sweep, which does not read H (chol_take_pending); any other reader
// factors it where it stands (chol_flush).  ONE matrix can wait; st: the stream it was built on.
void chol_defer(csp_ctx* c, double* H, int64_t n, int64_t ld, hipStream_t st) { c->D.chol.pending = {H, n, ld, st}; c->D.chol.factored = {}; }
// H if it is the matrix that waits, which then waits no longer: the caller factors it (potrf_launch, chol_mark_factored), or is
// about to factor or rebuild it anyway (chol_drop_pending)
double* chol_take_pending(csp_ctx* c, const void* H) {
  double* const P = c->D.chol.pending.H;
  if (!P || (const void*)P != H) return nullptr;
  c->D.chol.pending.H = nullptr;
  return P;
}
void chol_drop_pending(csp_ctx* c, const void* H) { (void)chol_take_pending(c, H); }
// The caller is about to free or reuse the memory of H
void chol_forget(csp_ctx* c, const void* H) { chol_drop_pending(c, H); if (c->D.chol.factored.A == H) c->D.chol.factored = {}; }

// launches of the dense Cholesky of A (no status read-back); info: the failure flag the kernels set (the context's flag, or
// a slot of its own when the factorisation runs on a side stream beside kernels that use the context's flag)
int potrf_launch(csp_ctx* c, double* A, int64_t n, int64_t lda, hipStream_t st, int* info) {
  DenseChol& C = c->D.chol;
  HIPCHK(hipMemsetAsync(info, 0, sizeof(int), st));
  C.factored = {};
  if (use_generic(c)) {
    launch(c, KID_dense_potrf, k_dense_potrf, dim3(1), dim3(1024), st, A, (int)n, lda, info);
    return 0;
  }
  if (n <= 2 * LB) {
    const size_t lds = ((size_t)((n | 1) * n) + 256 + 8) * sizeof(double);
    static bool attr_set = false;
    if (!attr_set) { HIPCHK(hipFuncSetAttribute((const void*)k_dense_potrf_small, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024)); attr_set = true; }
    launch_lds(c, KID_dense_potrf, k_dense_potrf_small, dim3(1), potrf_blk(), lds, st, A, (int)n, lda, info);
    return 0;
  }
  // blocked right-looking Cholesky, 64-wide block columns: diagonal block by one workgroup, panel and
  // trailing update as 64 x 64 MFMA tiles over the chip (the kernels of the large fronts, dense view)
  MfmaArgs a = mfma_args(c, nullptr, 0, 1);
  a.t.lev = c->D.lev3idx;
  a.t.info = info;
  a.lfd = c->D.lfd_dense;
  a.dn = (int)n; a.dld = lda;
  dim3 blk(256);
  const int64_t nblocks = (n + LB - 1) / LB, need = nblocks * LB * LB + 2 * n;
  if (int rc = dev_grow(&C.ws, &C.cap, need, c->D.mem, st)) return rc;
  // the whole blocked factorisation in ONE launch (front_flow.hip: tile dataflow inside the launch, the diagonal blocks' inverses
  // straight to their slots); SMCP_FLOW=0 or beyond 4096: three launches per block column
  if (flow_chol(c, st, A, lda, (int)n, C.ws, nullptr, 5, info, 1)) return 0;
  for (int jb = 0; jb < (int)n; jb += LB) {
    a.lfd = C.ws + (int64_t)(jb / LB) * LB * LB;      // the diagonal block's inverse goes straight to its slot (the panel kernel's operand)
    launch_lds(c, KID_lf_diag, k_lf_diag, dim3(1), dim3(512), LF_DIAG_LDS, st, a, A, (double*)nullptr, 5, jb, 1);
    const int mrem = (int)n - jb - LB;
    if (mrem > 0) {
      const int mt = tiles64(mrem);
      launch(c, KID_lf_chol_panel, k_lf_chol_panel, dim3(mt, 1), blk, st, a, A, (double*)nullptr, 5, jb);
      launch(c, KID_lf_chol_trail, k_lf_chol_trail, dim3(mt * (mt + 1) / 2, 1), blk, st, a, A, (double*)nullptr, 5, jb);
    }
  }
  return 0;
}
// The matrix that waits for its factorisation, if any, is factored where it stands, on st, and its verdict returned.
// only: nothing is done unless it is this matrix; except: ... if it is this one (the caller is about to rebuild it).
int chol_flush(csp_ctx* c, hipStream_t st, const void* only = nullptr, const void* except = nullptr) {
  const auto p = c->D.chol.pending;
  if (!p.H || (only && only != (const void*)p.H) || except == (const void*)p.H) return 0;
  c->D.chol.pending.H = nullptr;
  if (int rc = potrf_launch(c, p.H, p.n, p.ld, st, c->D.info)) return rc;
  HIPCHK(end_call(c));
  const int rc = fetch_info(c, st);
  if (!rc) chol_mark_factored(c, p.H, p.n);
  return rc;
}
// ... on the stream it was built on (kkt_set_constraints has no stream of its own)
int chol_flush_own_stream(csp_ctx* c) { return chol_flush(c, c->D.chol.pending.stream); }

// potrs with a Cholesky factor from anywhere, by route: one right-hand side of a factor made here takes k_dense_potrs_small
// (n <= 128) or, beyond POTRS1_MAXN, 2 ceil(n / 64) block steps over the chip, whose two work vectors are the tail of the
// workspace of the blocked factorisation; one right-hand side of any factor in between takes k_dense_potrs_one; everything else
// (generic mode, several right-hand sides, a factor from elsewhere outside that range) the one-workgroup generic solve.
int potrs_impl(csp_ctx* c, const double* A, int64_t n, int64_t lda, double* B, int64_t nrhs, int64_t ldb, hipStream_t st) {
  const bool fast = nrhs == 1 && chol_made_here(c, A, n);
  if (fast && n <= 2 * LB) {
    static bool attr = false;
    if (!attr) attr = hipFuncSetAttribute((const void*)k_dense_potrs_small, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024) == hipSuccess;
    launch_lds(c, KID_dense_potrs, k_dense_potrs_small, dim3(1), dim3(256), (size_t)n * (n | 1) * sizeof(double), st, A, (int)n, lda, B);
    return 0;
  }
  if (nrhs == 1 && n > 2 * LB && n <= POTRS1_MAXN && !use_generic(c)) {
    // one launch of one workgroup: the whole substitution chain with the factor streamed a step ahead (k_dense_potrs_one)
    static bool attr1 = false;
    if (!attr1) attr1 = hipFuncSetAttribute((const void*)k_dense_potrs_one, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024) == hipSuccess;
    if (attr1 && potrs_one_lds((int)n) <= (size_t)(160 * 1024 - 1024)) {
      launch_lds(c, KID_dense_potrs, k_dense_potrs_one, dim3(1), dim3(1024), potrs_one_lds((int)n), st, A, (int)n, lda, B);
      return 0;
    }
  }
  if (fast && n > 2 * LB) {
    const int64_t nblocks = (n + LB - 1) / LB;
    double* y = c->D.chol.ws + nblocks * LB * LB;      // forward solution
    double* z = y + n;                                  // backward solution
    for (int jb = 0; jb < (int)n; jb += LB) {
      const int w = (int)std::min<int64_t>(LB, n - jb);
      const int rest = (int)n - jb - w;
      launch(c, KID_dense_potrs, k_dense_trsv_step, dim3((unsigned)std::max(1, (rest + 255) / 256)), dim3(256), st, A, (int)n, lda, jb, w, B, y, 0);
    }
    for (int jb = (int)((nblocks - 1) * LB); jb >= 0; jb -= LB) {
      const int w = (int)std::min<int64_t>(LB, n - jb);
      launch(c, KID_dense_potrs, k_dense_trsv_step, dim3((unsigned)std::max(1, std::min(256, (jb + 3) / 4))), dim3(256), st, A, (int)n, lda, jb, w, y,
             z, 1);
    }
    HIPCHK(hipMemcpyAsync(B, z, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    return 0;
  }
  launch(c, KID_dense_potrs, k_dense_potrs, dim3(1), dim3(1024), st, A, (int)n, lda, B, (int)nrhs, ldb);
  return 0;
}
// dynamic LDS of the one-launch kernels (k_potrs_many_small, k_qr_many_small): the whole factor and sixteen columns beside it
size_t potrs_many_small_lds(int64_t n) { return ((size_t)n * (n | 1) + (size_t)PM_CBS * n) * sizeof(double); }
// the updates of the other rows in the block steps: FMA below eight columns of a workgroup's block, tile products on the matrix
// cores from eight on (the gate of csp_trmm / csp_symm); SMCP_POTRS_MANY_MM=0: FMA only; never in generic mode.  Read on every
// call: tools/solve_many_time.py alternates the two
int potrs_many_mm(const csp_ctx* c) { return (sw_int("SMCP_POTRS_MANY_MM", 1) && !use_generic(c)) ? 1 : 0; }
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
    launch_lds(c, KID_potrs_many_small, k_potrs_many_small, dim3((unsigned)((nrhs + PM_CBS - 1) / PM_CBS)), dim3(256), potrs_many_small_lds(n), st, A,
               (int)n, lda, B, (int)nrhs, ldb);
    return 0;
  }
  // the forward solution lives in the scratch image of csp_trsm / csp_trmm (no call keeps it): n x nrhs, leading dimension n
  if (int rc = dev_grow(&D.trsm_x, &D.trsm_x_len, n * nrhs, D.mem, st)) return rc;
  double* const Yw = D.trsm_x;
  const int mm = potrs_many_mm(c);
  potrs_many_fwd(c, A, n, lda, B, nrhs, ldb, Yw, mm, st);
  potrs_many_bwd(c, A, n, lda, B, nrhs, ldb, Yw, mm, st);
  return 0;
}

}  // namespace

extern "C" {

int dense_potrf(csp_ctx* c, double* A, int64_t n, int64_t lda, void* stream) {
  if (int rc = ready(c)) return rc;
  hipStream_t st = (hipStream_t)stream;
  chol_drop_pending(c, A);
  if (int rc = potrf_launch(c, A, n, lda, st, c->D.info)) return rc;
  HIPCHK(end_call(c));
  const int rc = fetch_info(c, st);
  if (!rc) chol_mark_factored(c, A, n);
  return rc;
}
int dense_potrs(csp_ctx* c, const double* A, int64_t n, int64_t lda, double* B, int64_t nrhs, int64_t ldb, void* stream) {
  if (int rc = ready(c)) return rc;
  if (int rc = chol_flush(c, (hipStream_t)stream, A)) return rc;
  if (int rc = potrs_impl(c, A, n, lda, B, nrhs, ldb, (hipStream_t)stream)) return rc;
  HIPCHK(end_call(c));
  return 0;
}

int dense_potrs_many(csp_ctx* c, const double* A, int64_t n, int64_t lda, double* B, int64_t nrhs, int64_t ldb, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!A || !B || n < 1 || n > (int64_t)0x7fffffff || lda < n || nrhs < 1 || nrhs > (int64_t)PM_CB * 65535 || (nrhs > 1 && ldb < n)) return SMCP_EINVAL;
  if (ranges_overlap(A, lda * (n - 1) + n, B, ldb * (nrhs - 1) + n)) return SMCP_EINVAL;
  if (int rc = chol_flush(c, (hipStream_t)stream, A)) return rc;
  if (int rc = potrs_many_impl(c, A, n, lda, B, nrhs, ldb, (hipStream_t)stream)) return rc;
  HIPCHK(end_call(c));
  return 0;
}

}  // extern "C"
