// Lanczos on the dual cone: the extreme Ritz values of L^-1 D L^-T (the step to the boundary of the
// dual cone along D) or of L^-T L^-1 (the smallest eigenvalue of S = L L^T).  The operator is the library's own csp_trsm /
// csp_symm on one column; the kernels here are everything around it, and nothing of it comes back to the host per step:
//
//   k_lz_copy     the scratch row <- v_j (the operator works in place on the scratch rows, the basis is never written twice).
//   k_lz_dots     the partial products v_i . w, i <= j, over the row slabs of lr_slab_rows (front_lowrank.hip): lanes along n,
//                 sixteen basis rows per workgroup, the basis read once.  Nobody adds into anybody's result: the partial of
//                 (slab, i) is stored at P[slab jmax + i] and every consumer sums the slabs in ascending order.
//   k_lz_update   every workgroup sums the partials into the coefficients c_i in LDS (ascending slab) and subtracts
//                 sum_i c_i v_i from its 256 rows of w, i ascending; the second pass leaves the partial |w|^2 of its rows.
//   k_lz_finish   one workgroup: alpha_j = c_j of pass one + c_j of pass two, beta_{j+1} = sqrt(sum of the partials), the
//                 breakdown test, and the scale 1 / beta_{j+1} (0 after a breakdown) for
//   k_lz_scale    v_{j+1} <- scale w, exact zeros when the scale is 0.
//   k_lz_ritz     one workgroup: the extreme eigenvalues of the tridiagonal T_m by multisection with Sturm counts, and the
//                 bottom components of their eigenvectors by two steps of inverse iteration.
//
// Classical Gram-Schmidt twice = dots, update, dots, update: separate launches order the passes, barriers order the phases
// inside a workgroup, and there is no floating-point atomic anywhere, so the same input gives the same bits.
//
// The workspace belongs to the caller (lz_work_len doubles):
//   [0, lz_state_len)     the state block: [0] status (0 running, 1 broke down: the Krylov space is invariant, 2 a non-finite
//                         alpha or beta), [1] steps done m, [2] the step count at which it broke down (-1: never), [3] the
//                         scale of the pending k_lz_scale, [4 .. 7] theta_min, resid_min, theta_max, resid_max (k_lz_ritz),
//                         [8] max(|alpha|, beta) seen so far, [16 + j] alpha_j, [16 + jmax + j] beta_j (beta_0 = |v0|)
//   then P1, P2           the partials of the two passes, LR_NSLAB_MAX x jmax each
//   then PN               the partials of |w|^2, one per 256 rows
//   then the basis        rows v_0 .. v_jmax of lz_ld(n) doubles each (entries n .. lz_ld(n) of a row are never touched)
//   then two scratch rows (csp_symm's C must not overlap its B)
#include <hip/hip_runtime.h>

namespace smcp {

constexpr int LZ_JMAX = 128;         // largest Krylov dimension: T and the pivoted solves of k_lz_ritz live in LDS
constexpr int LZ_HDR = 16;           // doubles ahead of alpha in the state block
constexpr int LZ_RB = 16;            // k_lz_dots: basis rows per workgroup
constexpr int LZ_UROWS = 256;        // k_lz_update / k_lz_scale / k_lz_copy: rows per workgroup (one per thread)
constexpr int LZ_ROUNDS = 8;         // k_lz_ritz: multisection rounds of 128 shifts per end (129^8 > 2^53 (2 |T| / |T|))
enum { LZ_ST_STATUS = 0, LZ_ST_STEPS, LZ_ST_BRK, LZ_ST_SCALE, LZ_ST_TMIN, LZ_ST_RMIN, LZ_ST_TMAX, LZ_ST_RMAX, LZ_ST_SEEN };

__host__ __device__ inline int64_t lz_up8(int64_t x) { return (x + 7) & ~(int64_t)7; }
__host__ __device__ inline int64_t lz_ld(int64_t n) { return lz_up8(n); }
__host__ __device__ inline int64_t lz_state_len(int64_t jmax) { return lz_up8(LZ_HDR + 2 * jmax + 1); }
__host__ __device__ inline int64_t lz_nnorm(int64_t n) { return (n + LZ_UROWS - 1) / LZ_UROWS; }
__host__ __device__ inline int64_t lz_off_p(int64_t jmax, int pass) { return lz_state_len(jmax) + pass * lz_up8((int64_t)LR_NSLAB_MAX * jmax); }
__host__ __device__ inline int64_t lz_off_pn(int64_t jmax) { return lz_off_p(jmax, 2); }
__host__ __device__ inline int64_t lz_off_basis(int64_t n, int64_t jmax) { return lz_off_pn(jmax) + lz_up8(lz_nnorm(n)); }
__host__ __device__ inline int64_t lz_off_scratch(int64_t n, int64_t jmax) { return lz_off_basis(n, jmax) + (jmax + 1) * lz_ld(n); }
__host__ __device__ inline int64_t lz_work_len(int64_t n, int64_t jmax) { return lz_off_scratch(n, jmax) + 2 * lz_ld(n); }

// grid ceil(n / LZ_UROWS)
__global__ void __launch_bounds__(256) k_lz_copy(const double* src, double* dst, int64_t n) {
  const int64_t r = (int64_t)blockIdx.x * LZ_UROWS + threadIdx.x;
  if (r < n) dst[r] = src[r];
}

struct LzDotsArgs {
  const double* V; int64_t ld;   // basis rows 0 .. nrow - 1
  const double* w;
  int nrow, jmax;
  int64_t n, slab;
  double* P;                     // (slab, i) at slab jmax + i
};

// grid (slabs, ceil(nrow / LZ_RB))
__global__ void __launch_bounds__(256) k_lz_dots(LzDotsArgs a) {
  __shared__ double red[3 * LZ_RB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * a.slab, r1 = r0 + a.slab < a.n ? r0 + a.slab : a.n;
  const int i0 = blockIdx.y * LZ_RB;
  const double* Vp[LZ_RB];
#pragma unroll
  for (int ii = 0; ii < LZ_RB; ++ii) Vp[ii] = a.V + (int64_t)min(i0 + ii, a.nrow - 1) * a.ld;
  double acc[LZ_RB];
#pragma unroll
  for (int ii = 0; ii < LZ_RB; ++ii) acc[ii] = 0.0;
  for (int64_t r = r0 + tid; r < r1; r += 256) {
    const double wv = a.w[r];
    double v[LZ_RB];
#pragma unroll
    for (int ii = 0; ii < LZ_RB; ++ii) v[ii] = Vp[ii][r];
#pragma unroll
    for (int ii = 0; ii < LZ_RB; ++ii) acc[ii] = fma(v[ii], wv, acc[ii]);
  }
#pragma unroll
  for (int ii = 0; ii < LZ_RB; ++ii) {
    double v = acc[ii];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    acc[ii] = v;
  }
  if (wave > 0 && lane == 0) {
#pragma unroll
    for (int ii = 0; ii < LZ_RB; ++ii) red[(wave - 1) * LZ_RB + ii] = acc[ii];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int ii = 0; ii < LZ_RB; ++ii) {
      double v = acc[ii];
      for (int w = 0; w < 3; ++w) v += red[w * LZ_RB + ii];
      if (i0 + ii < a.nrow) a.P[(int64_t)blockIdx.x * a.jmax + i0 + ii] = v;
    }
  }
}

struct LzUpdateArgs {
  const double* V; int64_t ld;
  double* w;
  int nrow, jmax, nslab;
  int64_t n;
  const double* P;
  double* PN;                    // null: pass one
};

// grid ceil(n / LZ_UROWS)
__global__ void __launch_bounds__(256) k_lz_update(LzUpdateArgs a) {
  __shared__ double cs[LZ_JMAX + 1];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  for (int i = tid; i < a.nrow; i += 256) {
    double v = 0.0;
    for (int s = 0; s < a.nslab; ++s) v += a.P[(int64_t)s * a.jmax + i];
    cs[i] = v;
  }
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * LZ_UROWS + tid;
  const bool live = r < a.n;
  const int64_t rc = live ? r : a.n - 1;
  double acc = a.w[rc];
  const double* Vr = a.V + rc;
  int i = 0;
  for (; i + 8 <= a.nrow; i += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = Vr[(int64_t)(i + u) * a.ld];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = fma(-cs[i + u], v[u], acc);
  }
  for (; i < a.nrow; ++i) acc = fma(-cs[i], Vr[(int64_t)i * a.ld], acc);
  if (live) a.w[r] = acc;
  if (a.PN) {
    double q = live ? acc * acc : 0.0;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) q += __shfl_xor(q, s, 64);
    if ((tid & 63) == 0) red[tid >> 6] = q;
    __syncthreads();
    if (tid == 0) a.PN[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

struct LzFinishArgs {
  double* state;
  const double* P1; const double* P2; const double* PN;
  int j;                         // the step; -1: the start vector (beta_0 = |v0| from P1[slab jmax], the state is reset)
  int jmax, nslab;
  int64_t nnorm;
  double brk;                    // breakdown when beta_{j+1} <= brk max(|alpha|, beta seen so far)
};

// one workgroup
__global__ void __launch_bounds__(256) k_lz_finish(LzFinishArgs a) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double* st = a.state;
  double* alpha = st + LZ_HDR;
  double* beta = alpha + a.jmax;
  if (a.j < 0) {
    if (tid == 0) {
      double s = 0.0;
      for (int k = 0; k < a.nslab; ++k) s += a.P1[(int64_t)k * a.jmax];
      const double b0 = sqrt(s);
      const bool ok = b0 > 0.0 && b0 < INFINITY;
      st[LZ_ST_STATUS] = ok ? 0.0 : (b0 == 0.0 ? 1.0 : 2.0);     // v0 = 0 spans an invariant space of dimension 0
      st[LZ_ST_STEPS] = 0.0;
      st[LZ_ST_BRK] = ok ? -1.0 : 0.0;
      st[LZ_ST_SCALE] = ok ? 1.0 / b0 : 0.0;
      for (int k = LZ_ST_TMIN; k < LZ_HDR; ++k) st[k] = 0.0;
      beta[0] = b0;
    }
    return;
  }
  double q = 0.0;
  for (int64_t k = tid; k < a.nnorm; k += 256) q += a.PN[k];
  red[tid] = q;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    if (st[LZ_ST_STATUS] != 0.0) { st[LZ_ST_SCALE] = 0.0; return; }      // after a breakdown: zeros stay zeros, nothing is counted
    double c1 = 0.0, c2 = 0.0;
    for (int k = 0; k < a.nslab; ++k) c1 += a.P1[(int64_t)k * a.jmax + a.j];
    for (int k = 0; k < a.nslab; ++k) c2 += a.P2[(int64_t)k * a.jmax + a.j];
    const double al = c1 + c2, be = sqrt(red[0]);
    alpha[a.j] = al;
    beta[a.j + 1] = be;
    st[LZ_ST_STEPS] = (double)(a.j + 1);
    const double seen = fmax(st[LZ_ST_SEEN], fabs(al));
    if (!(fabs(al) < INFINITY) || !(be < INFINITY)) {
      st[LZ_ST_STATUS] = 2.0; st[LZ_ST_BRK] = (double)(a.j + 1); st[LZ_ST_SCALE] = 0.0;
    } else if (be <= a.brk * seen) {
      st[LZ_ST_STATUS] = 1.0; st[LZ_ST_BRK] = (double)(a.j + 1); st[LZ_ST_SCALE] = 0.0;
    } else {
      st[LZ_ST_SCALE] = 1.0 / be;
    }
    st[LZ_ST_SEEN] = fmax(seen, be < INFINITY ? be : 0.0);
  }
}

// grid ceil(n / LZ_UROWS); dst may be w itself
__global__ void __launch_bounds__(256) k_lz_scale(const double* state, const double* w, double* dst, int64_t n) {
  const int64_t r = (int64_t)blockIdx.x * LZ_UROWS + threadIdx.x;
  const double s = state[LZ_ST_SCALE];
  if (r < n) dst[r] = s != 0.0 ? w[r] * s : 0.0;
}

// ---- the tridiagonal eigenproblem ------------------------------------------------------------------------------------------
// eigenvalues of T (diagonal al[0 .. m), squares of the off-diagonal b2[1 .. m)) below x: the recurrence of LAPACK's dlaebz
__device__ inline int lz_sturm(const double* al, const double* b2, int m, double x, double pivmin) {
  double q = al[0] - x;
  if (fabs(q) < pivmin) q = -pivmin;
  int cnt = q < 0.0 ? 1 : 0;
  for (int i = 1; i < m; ++i) {
    q = al[i] - x - b2[i] / q;
    if (fabs(q) < pivmin) q = -pivmin;
    cnt += q < 0.0 ? 1 : 0;
  }
  return cnt;
}

// |bottom component| of the normalised eigenvector of T for the eigenvalue theta: T - theta I = P L U by elimination with
// partial pivoting (LAPACK's dgttrf), two steps of inverse iteration from a fixed generic vector.  One lane; d, du, du2, l, x
// are its LDS arrays of LZ_JMAX doubles, pv its row-swap flags.
__device__ inline double lz_bottom(const double* al, const double* be, int m, double theta, double tiny, double* d, double* du,
                                   double* du2, double* l, double* x, int* pv) {
  for (int i = 0; i < m; ++i) { d[i] = al[i] - theta; du[i] = i + 1 < m ? be[i + 1] : 0.0; du2[i] = 0.0; }
  for (int i = 0; i + 1 < m; ++i) {
    const double dl = be[i + 1];
    if (fabs(d[i]) >= fabs(dl)) {
      const double f = d[i] != 0.0 ? dl / d[i] : 0.0;
      l[i] = f; pv[i] = 0;
      d[i + 1] -= f * du[i];
    } else {
      const double f = d[i] / dl;
      d[i] = dl; l[i] = f; pv[i] = 1;
      const double t = du[i];
      du[i] = d[i + 1];
      d[i + 1] = t - f * d[i + 1];
      if (i + 2 < m) { du2[i] = du[i + 1]; du[i + 1] = -f * du[i + 1]; }
    }
  }
  for (int i = 0; i < m; ++i) {
    if (fabs(d[i]) < tiny) d[i] = d[i] < 0.0 ? -tiny : tiny;
    const double t = (i + 1) * 0.6180339887498949;
    x[i] = 0.5 + (t - floor(t));
  }
  double bottom = 0.0;
  for (int it = 0; it < 2; ++it) {
    for (int i = 0; i + 1 < m; ++i) {
      if (!pv[i]) x[i + 1] -= l[i] * x[i];
      else { const double t = x[i]; x[i] = x[i + 1]; x[i + 1] = t - l[i] * x[i + 1]; }
    }
    x[m - 1] /= d[m - 1];
    if (m > 1) x[m - 2] = (x[m - 2] - du[m - 2] * x[m - 1]) / d[m - 2];
    for (int i = m - 3; i >= 0; --i) x[i] = (x[i] - du[i] * x[i + 1] - du2[i] * x[i + 2]) / d[i];
    double big = 0.0;
    for (int i = 0; i < m; ++i) big = fmax(big, fabs(x[i]));
    if (!(big > 0.0) || !(big < INFINITY)) return 0.0;
    double s = 0.0;
    for (int i = 0; i < m; ++i) { x[i] /= big; s = fma(x[i], x[i], s); }
    const double nrm = sqrt(s);
    for (int i = 0; i < m; ++i) x[i] /= nrm;
    bottom = fabs(x[m - 1]);
  }
  return bottom;
}

// one workgroup of 256 threads: threads 0 .. 127 work on the lower end of the spectrum, 128 .. 255 on the upper end
__global__ void __launch_bounds__(256) k_lz_ritz(double* state, int jmax) {
  __shared__ double al[LZ_JMAX], be[LZ_JMAX + 1], b2[LZ_JMAX];
  __shared__ double iv[2][2];                 // [end][lo, hi]
  __shared__ int cnt[256];
  __shared__ double xs[256];                  // the shifts of a round: the new interval ends are shifts, bit for bit
  __shared__ double fac[2][5][LZ_JMAX];
  __shared__ int piv[2][LZ_JMAX];
  const int tid = threadIdx.x, end = tid >> 7, t = tid & 127;
  const double steps = state[LZ_ST_STEPS];
  const int m = steps >= 1.0 ? (int)fmin(steps, (double)min(jmax, LZ_JMAX)) : 0;     // (whatever the block holds: T fits the LDS)
  const double* ga = state + LZ_HDR;
  const double* gb = ga + jmax;
  if (m < 1) {
    if (tid < 4) state[LZ_ST_TMIN + tid] = 0.0;
    return;
  }
  if (m == 1) {
    if (tid == 0) {
      state[LZ_ST_TMIN] = state[LZ_ST_TMAX] = ga[0];
      state[LZ_ST_RMIN] = state[LZ_ST_RMAX] = gb[1];
    }
    return;
  }
  if (tid < m) { al[tid] = ga[tid]; be[tid] = tid ? gb[tid] : 0.0; b2[tid] = tid ? gb[tid] * gb[tid] : 0.0; }
  if (tid == 0) be[m] = gb[m];
  __syncthreads();
  if (tid == 0) {
    double lo = INFINITY, hi = -INFINITY, bmax = 0.0;
    for (int i = 0; i < m; ++i) {
      const double r = fabs(be[i]) + (i + 1 < m ? fabs(be[i + 1]) : 0.0);
      lo = fmin(lo, al[i] - r); hi = fmax(hi, al[i] + r);
      bmax = fmax(bmax, b2[i]);
    }
    const double tn = fmax(fabs(lo), fabs(hi));
    const double pad = 2.0 * 2.220446049250313e-16 * tn * m + 2.0 * 2.2250738585072014e-308;   // the discs hold the spectrum strictly
    iv[0][0] = iv[1][0] = lo - pad;
    iv[0][1] = iv[1][1] = hi + pad;
    fac[0][0][0] = tn;
    fac[0][0][1] = 2.2250738585072014e-308 * fmax(1.0, bmax);
  }
  __syncthreads();
  const double tnorm = fac[0][0][0], pivmin = fac[0][0][1];
  __syncthreads();
  // count(x) = eigenvalues below x is monotone in x (the recurrence is, in IEEE arithmetic).  Lower end: the smallest
  // eigenvalue lies between the last shift with count 0 and the first with count >= 1; upper end: between the last with
  // count < m and the first with count m.
  const int want = end ? m : 1;
  for (int round = 0; round < LZ_ROUNDS; ++round) {
    const double lo = iv[end][0], hi = iv[end][1];
    const double x = fmin(lo + (hi - lo) * ((double)(t + 1) / 129.0), hi);
    xs[tid] = x;
    cnt[tid] = lz_sturm(al, b2, m, x, pivmin);
    __syncthreads();
    if (t == 0) {
      int f = 0;
      while (f < 128 && cnt[128 * end + f] < want) ++f;
      if (f < 128) iv[end][1] = xs[128 * end + f];
      if (f > 0) iv[end][0] = xs[128 * end + f - 1];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double theta = 0.5 * (iv[end][0] + iv[end][1]);
    const double tiny = fmax(2.220446049250313e-16 * tnorm, 2.2250738585072014e-308);
    const double bot = lz_bottom(al, be, m, theta, tiny, fac[end][0], fac[end][1], fac[end][2], fac[end][3], fac[end][4], piv[end]);
    state[end ? LZ_ST_TMAX : LZ_ST_TMIN] = theta;
    state[end ? LZ_ST_RMAX : LZ_ST_RMIN] = fabs(be[m]) * bot;
  }
}

}  // namespace smcp
