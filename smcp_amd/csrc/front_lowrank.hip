// Chordal plus low rank: M = L L^T + V diag(a) V^T = L (I + W A W^T) L^T with W = L^-1 V (n x k, k <= 64).  Everything
// beside the products with L is tall-skinny or k x k:
//
//   k_lr_gram    Z = W^T B (k x kb) for W and B in the layout of csp_trsm (column j of W at W + j ldw).  The n rows are cut
//                into slabs whose size depends on n alone (lr_slab_rows); a workgroup forms the partial product of one slab
//                and stores it at P[(slab k + j) kb + c].  Nobody adds into anybody's result: the consumers sum the partials
//                in ascending slab, so the bits do not depend on the order in which the workgroups ran.  Two routes: plain
//                FMA (any shape; 4 x 4 results per workgroup, a thread per row, a fixed shuffle tree and a fixed order of
//                the four waves) and v_mfma_f64_16x16x4 tiles (16 columns of W against up to 64 of B per workgroup, sixteen
//                rows per wave and step).
//   k_lr_small   one workgroup: K = W^T W from its partials, then the k x k construction of C and D in LDS, one column of V
//                at a time (the columns with a_j > 0 first, then those with a_j < 0; a_j = 0 is skipped):
//                    c = e_j + D K e_j,  s = c^T K c,  t = 1 + a_j s   (t <= 0: M is not positive definite, status 1 + j)
//                    sigma = a_j / (1 + sqrt t),  tau = sigma / sqrt t
//                    C += sigma (c + C K c) c^T,   D -= tau c (c + D^T K c)^T
//                so that (I + W C W^T)(I + W C W^T)^T = I + W A W^T and (I + W C W^T)^-1 = I + W D W^T after every column.
//                Nothing is divided by a quantity that dependent columns make small.  Then S = D + D^T + D^T K D.
//                The state block (lr_state_len doubles): [0] status, [1] sum of log t_j, [2] k, then a, K, C, D, S (k x k,
//                row-major).
//   k_lr_apply   B <- B + W (T Z) for T one of C, C^T, D, D^T, S, diag(a): a workgroup sums the partials of Z for its (at
//                most 16) columns, forms T Z in LDS and streams its 512 rows of W and of B once.
#include <hip/hip_runtime.h>

namespace smcp {

constexpr int LR_KMAX = 64;          // largest rank: the k x k blocks of k_lr_small live in LDS
constexpr int LR_SLAB_UNIT = 256;    // slabs are multiples of this many rows ...
constexpr int LR_NSLAB_MAX = 128;    // ... and there are at most this many of them
constexpr int LR_JB = 4, LR_CB = 4;  // FMA route: columns of W and of B per workgroup
constexpr int LR_ACB = 16;           // k_lr_apply: columns of B per workgroup
constexpr int LR_AROWS = 512;        // k_lr_apply: rows per workgroup (two per thread)
constexpr int LR_HDR = 8;            // doubles ahead of a in the state block
enum { LR_T_C = 0, LR_T_CT, LR_T_D, LR_T_DT, LR_T_S, LR_T_A };

__host__ __device__ inline int64_t lr_slab_rows(int64_t n) {
  const int64_t span = (int64_t)LR_SLAB_UNIT * LR_NSLAB_MAX;
  return LR_SLAB_UNIT * ((n + span - 1) / span);
}
__host__ __device__ inline int64_t lr_state_len(int64_t k) { return LR_HDR + k + 4 * k * k; }
// offsets into the state block
__host__ __device__ inline int64_t lr_off_a() { return LR_HDR; }
__host__ __device__ inline int64_t lr_off_mat(int64_t k, int which) { return LR_HDR + k + which * k * k; }   // 0 K, 1 C, 2 D, 3 S
__host__ __device__ inline size_t lr_small_lds(int k) { return ((size_t)3 * k * (k | 1) + 4 * LR_KMAX + 8 + LR_KMAX) * sizeof(double); }

struct LrGramArgs {
  const double* W; int64_t ldw; int k;
  const double* B; int64_t ldb; int kb;
  int64_t n, slab;
  double* P;               // partials: (slab, j, c) at (slab k + j) kb + c
};

// MM = false: grid (slabs, ceil(k / 4), ceil(kb / 4)); MM = true: grid (slabs, ceil(k / 16), ceil(kb / (16 NT)))
template <bool MM, int NT>
__global__ void __launch_bounds__(256) k_lr_gram(LrGramArgs a) {
  __shared__ double red[3 * (MM ? NT * 4 : LR_JB * LR_CB) * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * a.slab, r1 = r0 + a.slab < a.n ? r0 + a.slab : a.n;
  double* Ps = a.P + (int64_t)blockIdx.x * a.k * a.kb;
  if constexpr (!MM) {
    const int j0 = blockIdx.y * LR_JB, c0 = blockIdx.z * LR_CB;
    const double* Wp[LR_JB];
    const double* Bp[LR_CB];
#pragma unroll
    for (int jj = 0; jj < LR_JB; ++jj) Wp[jj] = a.W + (int64_t)min(j0 + jj, a.k - 1) * a.ldw;
#pragma unroll
    for (int cc = 0; cc < LR_CB; ++cc) Bp[cc] = a.B + (int64_t)min(c0 + cc, a.kb - 1) * a.ldb;
    double acc[LR_JB][LR_CB];
#pragma unroll
    for (int jj = 0; jj < LR_JB; ++jj)
#pragma unroll
      for (int cc = 0; cc < LR_CB; ++cc) acc[jj][cc] = 0.0;
    for (int64_t r = r0 + tid; r < r1; r += 256) {
      double w[LR_JB], b[LR_CB];
#pragma unroll
      for (int jj = 0; jj < LR_JB; ++jj) w[jj] = Wp[jj][r];
#pragma unroll
      for (int cc = 0; cc < LR_CB; ++cc) b[cc] = Bp[cc][r];
#pragma unroll
      for (int jj = 0; jj < LR_JB; ++jj)
#pragma unroll
        for (int cc = 0; cc < LR_CB; ++cc) acc[jj][cc] = fma(w[jj], b[cc], acc[jj][cc]);
    }
#pragma unroll
    for (int jj = 0; jj < LR_JB; ++jj)
#pragma unroll
      for (int cc = 0; cc < LR_CB; ++cc) {
        double v = acc[jj][cc];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
        acc[jj][cc] = v;
      }
    if (wave > 0 && lane == 0) {
#pragma unroll
      for (int jj = 0; jj < LR_JB; ++jj)
#pragma unroll
        for (int cc = 0; cc < LR_CB; ++cc) red[(wave - 1) * LR_JB * LR_CB + jj * LR_CB + cc] = acc[jj][cc];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int jj = 0; jj < LR_JB; ++jj)
#pragma unroll
        for (int cc = 0; cc < LR_CB; ++cc) {
          double v = acc[jj][cc];
          for (int w = 0; w < 3; ++w) v += red[w * LR_JB * LR_CB + jj * LR_CB + cc];
          if (j0 + jj < a.k && c0 + cc < a.kb) Ps[(int64_t)(j0 + jj) * a.kb + c0 + cc] = v;
        }
    }
  } else {
    const int l15 = lane & 15, kq = lane >> 4;
    const int j0 = blockIdx.y * 16, c0 = blockIdx.z * 16 * NT;
    const bool jok = j0 + l15 < a.k;
    const double* Wj = a.W + (int64_t)min(j0 + l15, a.k - 1) * a.ldw;
    const double* Bc[NT];
    bool cok[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      cok[t] = c0 + 16 * t + l15 < a.kb;
      Bc[t] = a.B + (int64_t)min(c0 + 16 * t + l15, a.kb - 1) * a.ldb;
    }
    d4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    // sixteen rows per wave and step: lane (l15, kq) takes the rows g + 4 kq + u, u < 4, of its column of W and of B (32
    // contiguous bytes each); MFMA number u sums over the rows g + 4 kq' + u, kq' < 4 -- the order of the inner index is free
    for (int64_t g = r0 + 16 * wave; g < r1; g += 64) {
      double av[4], bv[NT][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t rr = g + 4 * kq + u;
        const bool ok = rr < r1;
        const int64_t rc = ok ? rr : r1 - 1;       // loads at an index clamped into the slab, masked afterwards
        const double wv = Wj[rc];
        av[u] = (ok && jok) ? wv : 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const double b = Bc[t][rc];
          bv[t][u] = (ok && cok[t]) ? b : 0.0;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(bv[t][u], av[u], acc[t], 0, 0, 0);
    }
    // acc[t][r] = Z[j0 + l15][c0 + 16 t + kq + 4 r]; the four waves meet in LDS in ascending wave
    if (wave > 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[((wave - 1) * NT * 4 + t * 4 + r) * 64 + lane] = acc[t][r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double v = acc[t][r];
          for (int w = 0; w < 3; ++w) v += red[(w * NT * 4 + t * 4 + r) * 64 + lane];
          const int c = c0 + 16 * t + kq + 4 * r;
          if (jok && c < a.kb) Ps[(int64_t)(j0 + l15) * a.kb + c] = v;
        }
    }
  }
}

struct LrCoef { double a[LR_KMAX]; };

// one workgroup of 256 threads, lr_small_lds(k) bytes of dynamic LDS
__global__ void __launch_bounds__(256) k_lr_small(const double* P, int nslab, int k, LrCoef coef, double* state) {
  extern __shared__ double lr_sm[];
  const int ld = k | 1;                // odd: a column walk meets every bank
  double* Ks = lr_sm;
  double* Cs = Ks + k * ld;
  double* Ds = Cs + k * ld;
  double* cv = Ds + k * ld;            // c
  double* kc = cv + LR_KMAX;           // K c
  double* pv = kc + LR_KMAX;           // c + C K c
  double* qv = pv + LR_KMAX;           // c + D^T K c
  double* sc = qv + LR_KMAX;           // [0] t (<= 0: stop), [1] sigma, [2] tau
  int* ord = (int*)(sc + 8);           // the columns in the order they are taken, [LR_KMAX]: their number
  const int tid = threadIdx.x;
  const int row = tid >> 2, part = tid & 3;
  for (int e = tid; e < k * k; e += 256) {
    const int i = e / k, j = e - i * k;
    const int hi = max(i, j), lo = min(i, j);          // K from its lower triangle: exactly symmetric
    double v = 0.0;
    for (int s = 0; s < nslab; ++s) v += P[((int64_t)s * k + hi) * k + lo];
    Ks[i * ld + j] = v;
    Cs[i * ld + j] = 0.0;
    Ds[i * ld + j] = 0.0;
  }
  if (tid == 0) {
    int m = 0;
    for (int j = 0; j < k; ++j) if (coef.a[j] > 0.0) ord[m++] = j;
    for (int j = 0; j < k; ++j) if (coef.a[j] < 0.0) ord[m++] = j;
    ord[LR_KMAX] = m;
  }
  __syncthreads();
  const int nord = ord[LR_KMAX];
  // a dot product per row, four threads each (entries part, part + 4, ...), joined by a fixed butterfly
  auto rowdot = [&](auto term) {
    double v = 0.0;
    if (row < k) for (int m = part; m < k; m += 4) v += term(m);
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    return v;
  };
  double logsum = 0.0;
  int status = 0;
  for (int x = 0; x < nord; ++x) {
    const int j = ord[x];
    const double aj = coef.a[j];
    {
      const double v = rowdot([&](int m) { return Ds[row * ld + m] * Ks[m * ld + j]; });
      if (part == 0 && row < k) cv[row] = v + (row == j ? 1.0 : 0.0);
    }
    __syncthreads();
    {
      const double v = rowdot([&](int m) { return Ks[row * ld + m] * cv[m]; });
      if (part == 0 && row < k) kc[row] = v;
    }
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int m = 0; m < k; ++m) s = fma(cv[m], kc[m], s);
      const double t = 1.0 + aj * s;
      sc[0] = t;
      if (t > 0.0) {
        const double rt = sqrt(t);
        sc[1] = aj / (1.0 + rt);
        sc[2] = sc[1] / rt;
      }
    }
    {
      const double vp = rowdot([&](int m) { return Cs[row * ld + m] * kc[m]; });
      const double vq = rowdot([&](int m) { return Ds[m * ld + row] * kc[m]; });
      if (part == 0 && row < k) { pv[row] = cv[row] + vp; qv[row] = cv[row] + vq; }
    }
    __syncthreads();
    const double t = sc[0];
    if (!(t > 0.0)) { status = 1 + j; break; }         // (the same value in every thread: no barrier is left waiting)
    logsum += log(t);
    const double sigma = sc[1], tau = sc[2];
    for (int e = tid; e < k * k; e += 256) {
      const int i = e / k, jj = e - i * k;
      Cs[i * ld + jj] = fma(sigma * pv[i], cv[jj], Cs[i * ld + jj]);
      Ds[i * ld + jj] = fma(-tau * cv[i], qv[jj], Ds[i * ld + jj]);
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid == 0) {
    state[0] = (double)status;
    state[1] = logsum;
    state[2] = (double)k;
    for (int i = 3; i < LR_HDR; ++i) state[i] = 0.0;
  }
  for (int e = tid; e < k; e += 256) state[lr_off_a() + e] = coef.a[e];
  for (int e = tid; e < k * k; e += 256) {
    const int i = e / k, j = e - i * k;
    state[lr_off_mat(k, 0) + e] = Ks[i * ld + j];
    state[lr_off_mat(k, 1) + e] = Cs[i * ld + j];
    state[lr_off_mat(k, 2) + e] = Ds[i * ld + j];
  }
  __syncthreads();
  // S = D + D^T + D^T (K D); K D takes the place of C
  for (int e = tid; e < k * k; e += 256) {
    const int i = e / k, j = e - i * k;
    double v = 0.0;
    for (int m = 0; m < k; ++m) v = fma(Ks[i * ld + m], Ds[m * ld + j], v);
    Cs[i * ld + j] = v;
  }
  __syncthreads();
  for (int e = tid; e < k * k; e += 256) {
    const int i = e / k, j = e - i * k;
    double v = 0.0;
    for (int m = 0; m < k; ++m) v = fma(Ds[m * ld + i], Cs[m * ld + j], v);
    state[lr_off_mat(k, 3) + e] = Ds[i * ld + j] + Ds[j * ld + i] + v;
  }
}

struct LrApplyArgs {
  const double* W; int64_t ldw; int k;
  double* B; int64_t ldb; int kb;
  int64_t n;
  const double* P; int nslab;          // partials of Z = W^T B (k_lr_gram)
  const double* state; int mode;       // LR_T_*
};

// grid (ceil(n / LR_AROWS), ceil(kb / LR_ACB))
__global__ void __launch_bounds__(256) k_lr_apply(LrApplyArgs a) {
  __shared__ double Zs[LR_KMAX * LR_ACB], Ys[LR_KMAX * LR_ACB];
  const int tid = threadIdx.x;
  const int k = a.k;
  const int c0 = blockIdx.y * LR_ACB, nc = min(LR_ACB, a.kb - c0);
  for (int e = tid; e < k * LR_ACB; e += 256) {
    const int j = e / LR_ACB, cc = e % LR_ACB;
    double v = 0.0;
    if (cc < nc) for (int s = 0; s < a.nslab; ++s) v += a.P[((int64_t)s * k + j) * a.kb + c0 + cc];
    Zs[e] = v;
  }
  __syncthreads();
  if (a.mode == LR_T_A) {
    const double* av = a.state + lr_off_a();
    for (int e = tid; e < k * LR_ACB; e += 256) Ys[e] = av[e / LR_ACB] * Zs[e];
  } else {
    const int which = a.mode == LR_T_S ? 3 : (a.mode == LR_T_C || a.mode == LR_T_CT) ? 1 : 2;
    const bool tr = a.mode == LR_T_CT || a.mode == LR_T_DT;
    const double* T = a.state + lr_off_mat(k, which);
    const int si = tr ? 1 : k, sj = tr ? k : 1;        // T(i, j) = T[i si + j sj]
    for (int e = tid; e < k * LR_ACB; e += 256) {
      const int i = e / LR_ACB, cc = e % LR_ACB;
      double v = 0.0;
      for (int j = 0; j < k; ++j) v = fma(T[i * si + j * sj], Zs[j * LR_ACB + cc], v);
      Ys[e] = v;
    }
  }
  __syncthreads();
  const int64_t rbase = (int64_t)blockIdx.x * LR_AROWS + tid;
  const int64_t ra = rbase < a.n ? rbase : a.n - 1, rb = rbase + 256 < a.n ? rbase + 256 : a.n - 1;
  double acc[2][LR_ACB];
#pragma unroll
  for (int cc = 0; cc < LR_ACB; ++cc) acc[0][cc] = acc[1][cc] = 0.0;
  for (int j = 0; j < k; ++j) {
    const double* Wj = a.W + (int64_t)j * a.ldw;
    const double w0 = Wj[ra], w1 = Wj[rb];
#pragma unroll
    for (int cc = 0; cc < LR_ACB; ++cc) {
      const double y = Ys[j * LR_ACB + cc];
      acc[0][cc] = fma(w0, y, acc[0][cc]);
      acc[1][cc] = fma(w1, y, acc[1][cc]);
    }
  }
#pragma unroll
  for (int cc = 0; cc < LR_ACB; ++cc) {
    if (cc >= nc) continue;
    double* Bc = a.B + (int64_t)(c0 + cc) * a.ldb;
    if (rbase < a.n) Bc[rbase] += acc[0][cc];
    if (rbase + 256 < a.n) Bc[rbase + 256] += acc[1][cc];
  }
}

}  // namespace smcp
