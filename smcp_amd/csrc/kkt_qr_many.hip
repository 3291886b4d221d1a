// The kkt_qr solve for a block of right-hand sides: kkt_qr_solve_many; included by capi.hip after kkt_qr.hip; the triangular block
// solves are dense_chol.hip's.
// Row r of the block is the system of kkt_qr_solve, statement for statement (src/python/solvers.py:444-465), in the device's
// normalisation (weights 1 on the diagonal and 2 below it, R stored as the lower Lc = R^T, no 0.5 factor):
//   r1 = G(bx) -> xm = Q^T r1 (weighted) -> t = Lc^-1 by -> x = xm + kk t -> y = Lc^-T x -> bx = G^adj(Q x - r1) / kk.
// Q is the whole constraint stack (m x blklen doubles) and kkt_qr_solve reads it twice per right-hand side; here the two tall
// products take all the rows of a chunk at once on v_mfma_f64_16x16x4, so that Q is read twice per CHUNK of up to QM_CT rows.
// Both products are bound by the bytes of Q whatever the number of rows (2 m blklen 16 flops against m blklen 8 bytes): there is
// one route, with the block padded to sixteen columns.

namespace {

constexpr int QM_CT = 16;                 // rows of the block per chunk: one column tile of the two products (the cap of the chunk)
// positions per workgroup of k_stack_dots_many, one set of partial sums each: 2048, and a multiple of that once the stack is longer
// than 2^22 positions, so that the sum over the chunks stays at most 2048 terms long (a function of blklen only)
int64_t qr_many_positions(int64_t bl) { return 2048 * std::max<int64_t>(1, (bl + (((int64_t)1 << 22) - 1)) >> 22); }
constexpr int QM_NT = 2;                  // tiles of sixteen rows of Q per wavefront of k_stack_dots_many (128 rows per workgroup)

typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));      // two consecutive doubles, no more aligned than one

// part[(chunk * QM_CT + r) * m + j] = sum over the positions p of chunk blockIdx.x of Q[j][p] sw[p]^2 BX_r[p]
// One workgroup = `chunk` positions (a multiple of 32) x 128 rows of Q (blockIdx.y) x the c <= 16 rows of the block; wavefront w takes the tiles
// w and w + 4 of sixteen rows of Q.  MFMA operands: A[M = row of Q][k], B[k][N = row of the block], K = positions.  The sum over
// the positions has no prescribed order, so a group of 32 positions is dealt as position = base + 8 i + 2 kq + e <-> k-step
// 2 i + e, k-slot kq, for A and B alike: lane (l15, kq) fetches two consecutive doubles of ITS row per load, the four lanes of a
// row 64 contiguous bytes, and no operand passes through LDS.  The weighted block operand is formed once per wavefront and
// shared by its tiles of Q; the rows of Q are read once per launch.  A column of the result depends on its own row of the block
// only (rows >= c and rows of Q >= m enter as zeros by selection, never by multiplication).
__global__ void __launch_bounds__(256) k_stack_dots_many(const double* __restrict__ Q, int64_t ldq, int64_t len, int m,
                                                         const double* __restrict__ sw, const double* __restrict__ BX, int64_t ldbx, int c,
                                                         int64_t chunk, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile0 = (int)blockIdx.y * 4 * QM_NT + wave;
  if (16 * tile0 >= m) return;                                   // (wave-uniform; the kernel has no barrier)
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(len, lo + chunk);
  const double* qrow[QM_NT];
  bool qin[QM_NT];
#pragma unroll
  for (int t = 0; t < QM_NT; ++t) {
    const int row = 16 * (tile0 + 4 * t) + l15;
    qin[t] = row < m;
    qrow[t] = Q + (int64_t)(qin[t] ? row : 0) * ldq;
  }
  const bool bin = l15 < c;
  const double* brow = BX + (int64_t)(bin ? l15 : 0) * ldbx;
  d4 acc[QM_NT];
#pragma unroll
  for (int t = 0; t < QM_NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  for (int64_t pb = lo; pb < hi; pb += 32) {
    double a[QM_NT][8], b[8];
    if (pb + 32 <= hi) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t off = pb + 8 * i + 2 * kq;
        const d2u w = *reinterpret_cast<const d2u*>(sw + off);
        const d2u x = *reinterpret_cast<const d2u*>(brow + off);
        b[2 * i] = bin ? x.x * (w.x * w.x) : 0.0;
        b[2 * i + 1] = bin ? x.y * (w.y * w.y) : 0.0;
#pragma unroll
        for (int t = 0; t < QM_NT; ++t) {
          const d2u q = *reinterpret_cast<const d2u*>(qrow[t] + off);
          a[t][2 * i] = qin[t] ? q.x : 0.0;
          a[t][2 * i + 1] = qin[t] ? q.y : 0.0;
        }
      }
    } else {                                                     // the ragged end of the stack: position by position
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int64_t p = pb + 8 * (s >> 1) + 2 * kq + (s & 1);
        const bool in = p < hi;
        const double w = in ? sw[p] : 0.0;
        b[s] = (in && bin) ? brow[p] * (w * w) : 0.0;
#pragma unroll
        for (int t = 0; t < QM_NT; ++t) a[t][s] = (in && qin[t]) ? qrow[t][p] : 0.0;
      }
    }
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int t = 0; t < QM_NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t][s], b[s], acc[t], 0, 0, 0);
  }
  if (!bin) return;
  double* out = part + ((int64_t)blockIdx.x * QM_CT + l15) * m;
#pragma unroll
  for (int t = 0; t < QM_NT; ++t)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int j = 16 * (tile0 + 4 * t) + kq + 4 * x;
      if (j < m) out[j] = acc[t][x];
    }
}
// XM[r * m + j] = sum over the chunks of part[(chunk * QM_CT + r) * m + j], r = blockIdx.y: sixteen interleaved runs of the chunks in
// ascending order, then a binary tree over the sixteen -- an order that depends on the shapes only
__global__ void __launch_bounds__(1024) k_qr_many_sum(const double* __restrict__ part, int nchunk, int m, double* XM) {
  __shared__ double red[16][64];
  const int jl = threadIdx.x & 63, g = threadIdx.x >> 6, j = (int)blockIdx.x * 64 + jl, r = blockIdx.y;
  double acc = 0.0;
  if (j < m) {
#pragma unroll 4
    for (int ch = g; ch < nchunk; ch += 16) acc += part[((int64_t)ch * QM_CT + r) * m + j];
  }
  red[g][jl] = acc;
  __syncthreads();
  if (g == 0 && j < m) {
    double t[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = red[i][jl];
#pragma unroll
    for (int w = 1; w < 16; w *= 2)
#pragma unroll
      for (int i = 0; i < 16; i += 2 * w) t[i] += t[i + w];
    XM[(int64_t)r * m + j] = t[0];
  }
}

// The m x m step for m <= 128 in one launch (the two halves of k_potrs_many_small with the update between them): workgroup g
// takes the columns 16 g .. with the lower triangle of Lc in LDS.  T = Lc^-1 BY;  X <- X + kk T (in place on XM: the x of
// solvers.py:453, kept for the second product);  BY <- Lc^-T X.
__global__ void __launch_bounds__(256) k_qr_many_small(const double* Ag, int n, int64_t ldag, double* XM, double kk, double* BY, int nrhs, int64_t ldby) {
  extern __shared__ __attribute__((aligned(16))) double pms[];
  const int tid = threadIdx.x, ld = n | 1;
  double* const A = pms;
  double* const T = pms + n * ld;
  const int c0 = blockIdx.x * PM_CBS, kc = min(PM_CBS, nrhs - c0);
  for (int e = tid; e < n * n; e += 256) {
    const int i = e % n, j = e / n;
    if (i >= j) A[i + j * ld] = Ag[i + (int64_t)j * ldag];
  }
  for (int e = tid; e < n * kc; e += 256) T[e] = BY[e % n + (int64_t)(c0 + e / n) * ldby];
  __syncthreads();
  pm_block_solve(A, ld, n, T, n, kc, 0);
  for (int e = tid; e < n * kc; e += 256) {
    double* x = XM + e % n + (int64_t)(c0 + e / n) * n;
    const double v = kk * T[e] + 1.0 * x[0];
    T[e] = v;
    x[0] = v;
  }
  __syncthreads();
  pm_block_solve(A, ld, n, T, n, kc, 1);
  for (int e = tid; e < n * kc; e += 256) BY[e % n + (int64_t)(c0 + e / n) * ldby] = T[e];
}
// ... and beyond 128, between the forward and the backward block steps of k_potrs_many_step: X <- X + kk T in place on XM, and a
// copy of it in T (the backward steps update their source in place)
__global__ void k_qr_many_mid(int64_t n, double kk, double* T, double* XM) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = kk * T[i] + 1.0 * XM[i];
  T[i] = v;
  XM[i] = v;
}

// BX_r[p] <- sum_j X[r][j] Q[j][p] - BX_r[p]  for the c <= 16 rows of the block (X: c x m, row r at X + r * m), in place.
// MFMA operands: A[M = row r of the block][k = j], B[k = j][N = position], K = j: a wavefront takes 64 positions as four groups
// of sixteen, group (h, e) the positions p0 + 32 h + 2 l15 + e, so that the operand of two groups is ONE load of two consecutive
// doubles of a row of Q (four rows x 256 contiguous bytes per load) and the result of two groups one store of two doubles.
// Q is read once per launch; a row of the result depends on its own row of X and of the block only.
__global__ void __launch_bounds__(256) k_stack_comb_many(const double* __restrict__ Q, int64_t ldq, int64_t len, int m,
                                                         const double* __restrict__ X, double* BX, int64_t ldbx, int c) {
  const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t p0 = ((int64_t)blockIdx.x * 4 + wave) * 64;
  if (p0 >= len) return;
  const bool full = p0 + 64 <= len;                              // (wave-uniform)
  const bool ain = l15 < c;
  const double* xrow = X + (int64_t)(ain ? l15 : 0) * m;
  d4 acc[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int e = 0; e < 2; ++e) acc[h][e] = d4{0.0, 0.0, 0.0, 0.0};
  const int64_t pl = p0 + 2 * l15;
  for (int j0 = 0; j0 < m; j0 += 8) {                            // two k-steps per trip: four loads of Q in flight
    double a[2], b[2][2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int j = j0 + 4 * s + kq;
      const bool jin = j < m;
      a[s] = (jin && ain) ? xrow[j] : 0.0;
      const double* q = Q + (int64_t)(jin ? j : 0) * ldq + pl;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (full) {
          const d2u v = *reinterpret_cast<const d2u*>(q + 32 * h);
          b[s][h][0] = jin ? v.x : 0.0;
          b[s][h][1] = jin ? v.y : 0.0;
        } else {
#pragma unroll
          for (int e = 0; e < 2; ++e) b[s][h][e] = (jin && pl + 32 * h + e < len) ? q[32 * h + e] : 0.0;
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 2; ++e) acc[h][e] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[s][h][e], acc[h][e], 0, 0, 0);
  }
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int r = kq + 4 * x;
    if (r >= c) continue;
    double* o = BX + (int64_t)r * ldbx + pl;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (full) {
        d2u v = *reinterpret_cast<const d2u*>(o + 32 * h);
        v.x = acc[h][0][x] - v.x;
        v.y = acc[h][1][x] - v.y;
        *reinterpret_cast<d2u*>(o + 32 * h) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 2; ++e)
          if (pl + 32 * h + e < len) o[32 * h + e] = acc[h][e][x] - o[32 * h + e];
      }
    }
  }
}

int64_t qr_many_chunk(int64_t max_rhs) { return max_rhs < 1 ? 0 : std::min<int64_t>(max_rhs, QM_CT); }
// doubles of the workspace of a chunk: the partial sums of every position chunk, XM and T (sixteen rows of m each)
int64_t qr_many_ws_doubles(int64_t m, int64_t bl) { const int64_t ch = qr_many_positions(bl); return ((bl + ch - 1) / ch + 2) * QM_CT * m; }

}  // namespace

extern "C" {

int64_t kkt_qr_solve_many_chunk(int64_t max_rhs) { return qr_many_chunk(max_rhs); }

int kkt_qr_solve_many(csp_ctx* c, const double* L, const double* Y, double kk, double* BX, int64_t ldbx, double* BY, int64_t ldby,
                      int64_t nrhs, void* stream) {
  if (int rc = ready(c)) return rc;
  DeviceCtx& D = c->D;
  const int64_t m = D.m, bl = c->S.blklen();
  if (!m || !L || !Y || !BX || !BY || nrhs < 1 || (nrhs > 1 && (ldbx < bl || ldby < m))) return SMCP_EINVAL;
  if (!D.qr_valid || D.qr_L != L || D.qr_Y != Y) return SMCP_EINVAL;
  if (c->xr_world > 1) return SMCP_EINVAL;                        // as kkt_qr_factor: one device holds the whole Q
  // (the any-size route, CSP_TUNE_DETERMINISTIC / SMCP_GENERIC, is accepted as kkt_qr_solve accepts it: the Hessian sweeps then take
  // the fixed-order kernels -- the LDS classes of the fast sweeps add the children's updates with atomics, in whatever order they
  // arrive -- and every kernel of this file sums in a fixed order anyway, so that "the same call gives the same bits" has a route
  // on which it holds for every pattern)
  {
    const int64_t xlen = ldbx * (nrhs - 1) + bl, ylen = ldby * (nrhs - 1) + m;
    if (ranges_overlap(BX, xlen, BY, ylen)) return SMCP_EINVAL;
    for (const double* B : {(const double*)BX, (const double*)BY}) {
      const int64_t blen = B == BX ? xlen : ylen;
      if (ranges_overlap(B, blen, D.ustack, D.ustack_cols * bl) || ranges_overlap(B, blen, D.qr_ws, D.qr_len)) return SMCP_EINVAL;
      if (D.qrm_ws && ranges_overlap(B, blen, D.qrm_ws, D.qrm_len)) return SMCP_EINVAL;
    }
  }
  const int64_t cmax = qr_many_chunk(D.max_rhs);
  if (cmax < 1) return SMCP_ENOMEM;
  hipStream_t st = (hipStream_t)stream;
  // a buffer of its own (qr_ws holds R and must not move): grown at the first call of a larger shape, never in steady state
  if (int rc = dev_grow(&D.qrm_ws, &D.qrm_len, qr_many_ws_doubles(m, bl), D.mem, st)) return rc;
  const int64_t chunk = qr_many_positions(bl);
  const int nchunk = (int)((bl + chunk - 1) / chunk);
  double* const part = D.qrm_ws;
  double* const XM = part + (int64_t)nchunk * QM_CT * m;
  double* const T = XM + QM_CT * m;
  const double* Lc = D.qr_ws + 2 * m * m;
  // the half-Hessians need chol(Y_AA) of THIS Y (kkt_qr_solve): another factorisation since kkt_qr_factor has left its own
  HIPCHK(zero_flag(c, st));
  prepare_yaa(c, Y, true, st);
  if (int rc = prep_lk_cached(c, L, Y, st)) return rc;
  const int mm = potrs_many_mm(c);
  for (int64_t r0 = 0; r0 < nrhs; r0 += cmax) {
    const int k = (int)std::min(cmax, nrhs - r0);
    double* const bx = BX + r0 * ldbx;
    double* const by = BY + r0 * ldby;
    hessian_impl(c, L, bx, k, ldbx, 0, 0, st);                                               // BX_r = G(bx_r), in place   (444-447)
    launch(c, KID_qr_dots_many, k_stack_dots_many, dim3((unsigned)nchunk, (unsigned)((m + 64 * QM_NT - 1) / (64 * QM_NT))), dim3(256), st,
           (const double*)D.ustack, bl, bl, (int)m, (const double*)D.sw, (const double*)bx, ldbx, k, chunk, part);
    launch(c, KID_qr_many_sum, k_qr_many_sum, dim3((unsigned)((m + 63) / 64), (unsigned)k), dim3(1024), st, (const double*)part, nchunk, (int)m, XM);   // (449-450)
    if (m <= 2 * LB) {
      static bool attr = false;
      if (!attr) attr = hipFuncSetAttribute((const void*)k_qr_many_small, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024) == hipSuccess;
      launch_lds(c, KID_qr_many_small, k_qr_many_small, dim3((unsigned)((k + PM_CBS - 1) / PM_CBS)), dim3(256), potrs_many_small_lds(m), st, Lc, (int)m, m, XM,
                 kk, by, k, ldby);
    } else {
      potrs_many_fwd(c, Lc, m, m, by, k, ldby, T, mm, st);                                   // T = R^-T by                (452)
      launch(c, KID_qr_many_mid, k_qr_many_mid, dim3((unsigned)((m * k + 255) / 256)), dim3(256), st, m * k, kk, T, XM);   // x          (453)
      potrs_many_bwd(c, Lc, m, m, by, k, ldby, T, mm, st);                                   // y = R^-1 x                 (454-455)
    }
    launch(c, KID_qr_comb_many, k_stack_comb_many, dim3((unsigned)((bl + 255) / 256)), dim3(256), st, (const double*)D.ustack, bl, bl, (int)m,
           (const double*)XM, bx, ldbx, k);                                                  // Q x - r1                   (457-458)
    hessian_impl(c, L, bx, k, ldbx, 1, 0, st);                                               // G^adj                      (461)
    launch(c, KID_kkt_many_scale, k_kkt_many_scale, dim3((unsigned)std::min<int64_t>(1024, (bl + 255) / 256), (unsigned)k), dim3(256), st, bl, 1.0 / kk,
           bx, ldbx);
  }
  HIPCHK(end_call(c));
  // kkt_qr_solve reads no verdict of chol(Y_AA) back (its Y is the one kkt_qr_factor accepted) and neither does this call; with
  // deferred status a failure is moved to the latch, where csp_status finds it -- a launch, no wait
  if (c->lazy_status) return fetch_info(c, st);
  return 0;
}

}  // extern "C"
