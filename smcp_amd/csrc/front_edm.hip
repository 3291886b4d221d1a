// Euclidean distance matrix completion on a chordal pattern (csp_edmcompletion_rank / csp_edmcompletion / csp_edm_dense):
// points Y (n x r) with |Y_i - Y_j|^2 = D_ij on V, r = the largest numerical affine dimension of a clique -- CHOMPACK's
// edmcompletion.  A partial EDM on a chordal pattern is completable iff every clique block D_gg is an EDM (Bakonyi and
// Johnson), and D_gg is an EDM iff a centred Gram matrix of it is positive semidefinite (Schoenberg, Gower); its rank is the
// affine dimension of the clique.
//
// Per clique g = N u A (own columns N, separator A) the Gram matrix is taken about the centroid of the separator points:
//   G_ij = -1/2 (D_ij - rho_i - rho_j + sigma),  rho_i = mean_{a in A} D_ia,  sigma = mean_{a,b in A} D_ab,
// a root (na = 0) about the centroid of its own clique (rho, sigma over g: classical MDS).  Then G_ij = <Y_i - c, Y_j - c>
// for any points Y of the clique, c the centroid of Y_A, and the step of k_mrc_factor applies unchanged to G:
// Pass 1 (k_edm_rank): D_gg from the panel and the separator block D_AA (top-down gather), turned into G in the slot, then
//   mrc_pchol with thr = tol * max diag G: rank_k = its pivots; a remaining pivot below -thr: D_gg is not an EDM.  G times
//   the indicator of the centring set is zero, so the factorisation runs on G without its last row and column (a vertex
//   of that set): same rank, same semidefiniteness, and no pivot that is zero by construction to be judged by its
//   rounding.  A nonzero stored diagonal entry of the clique's own columns is flagged (2) and makes the call return
//   SMCP_EINVAL.
// Pass 2 (k_edm_factor, one launch per level, root first): c = column mean of Y_A (the rows the ancestors wrote, summed in
//   a fixed order), W_A = Y_A - 1 c^T.  sigma is taken from the placed rows, sigma = (2/na) sum_a |W_a|^2, and likewise
//   rho_a = |W_a|^2 + sigma/2, so that G_NA is consistent with the W_A it is solved against and no D_AA is needed; rho_i
//   (i in N) comes from the panel.  Then pivoted QR of W_A^T, Z1 = (G_NA P)[:, :ra] R11^-1, pivoted Cholesky of
//   G_NN - Z1 Z1^T (at most r - ra columns, more are recorded as in k_mrc_factor), the reflectors from the right, and
//   Y_N = W_N + 1 c^T.  A root has c = 0 and ra = 0.  The threshold is tol * max diag G_gg, the diagonal taken as |W_a|^2
//   on A and rho_i - sigma/2 on N.
// k_edm_dense: D^[i, j] = sum_c (Y[p_i, c] - Y[p_j, c])^2 over 64 x 64 output tiles, the two sets of Y rows staged in LDS;
//   the sum runs over c in a fixed order and (x - y)^2 = (y - x)^2 exactly, so D^ is exactly symmetric with a zero diagonal.
//
// Slots, launches and the workgroup routines (mrc_pchol, mrc_qrp, mrc_argmax, MrcArgs) are those of front_mrc.hip, which
// capi.hip includes before this file.
#include <hip/hip_runtime.h>

#include <cmath>

#include "context.hpp"

namespace smcp {

// doubles of one pass-2 slot: the pass-2 slot of mrcompletion plus the centroid (r) and |W_a|^2 (na)
__host__ __device__ inline int64_t edm_slot2(int64_t nn, int64_t na, int64_t r) { return mrc_slot2(nn, na, r) + r + na + 2; }

// pass 1: see the head of the file.  Slot: mrc_slot1(nf) -- F (nf x nf), rho then pchol scratch (nf), done (nf ints)
__global__ void __launch_bounds__(MRC_NT) k_edm_rank(MrcArgs a) {
  extern __shared__ double mrc_lds[];
  __shared__ double s_sigma;
  __shared__ int s_baddiag;
  double* ws = a.ws ? a.ws + (int64_t)blockIdx.x * a.slot : mrc_lds;
  for (int e = blockIdx.x; e < a.cnt; e += gridDim.x) {
    const int k = a.lev[e];
    const CliqueDesc d = a.cl[k];
    const int nn = d.nn, na = d.na, nf = nn + na;
    const double* P = a.x + d.blk;
    const double* U = a.upd + d.upd;
    double* F = ws;
    double* rho = F + (int64_t)nf * nf;
    int* done = (int*)(rho + nf);
    if (SMCP_TID == 0) s_baddiag = 0;
    __syncthreads();
    for (int t = SMCP_TID; t < nf * nf; t += MRC_NT) {
      const int i = t % nf, j = t / nf;
      if (i >= j) F[t] = j < nn ? P[i + (int64_t)j * nf] : U[(i - nn) + (int64_t)(j - nn) * na];
    }
    for (int t = SMCP_TID; t < nn; t += MRC_NT)
      if (P[t + (int64_t)t * nf] != 0.0) s_baddiag = 1;
    __syncthreads();
    // centre: the separator points, or (root) the clique's own
    const int c0 = na ? nn : 0, nc = na ? na : nf;
    for (int i = SMCP_TID; i < nf; i += MRC_NT) {
      double s = 0.0;
      for (int b = c0; b < c0 + nc; ++b) s += i >= b ? F[i + (int64_t)b * nf] : F[b + (int64_t)i * nf];
      rho[i] = s / nc;
    }
    __syncthreads();
    if (SMCP_TID == 0) {
      double s = 0.0;
      for (int b = c0; b < c0 + nc; ++b) s += rho[b];
      s_sigma = s / nc;
    }
    __syncthreads();
    const double sigma = s_sigma;
    for (int t = SMCP_TID; t < nf * nf; t += MRC_NT) {
      const int i = t % nf, j = t / nf;
      if (i >= j) F[t] = -0.5 * (F[t] - rho[i] - rho[j] + sigma);
    }
    __syncthreads();
    double md;
    mrc_argmax(nf, [&](int i) { return F[i + (int64_t)i * nf]; }, md);
    const double thr = a.tol * (md > 0.0 ? md : 0.0);
    // the rows of G over the centring set sum to zero: the last of them (vertex nf - 1, in that set in both cases) is left
    // out, which keeps the rank and the sign of G and drops the one pivot that is zero by construction (rounding only)
    int neg, more;
    const int rk = mrc_pchol(nf - 1, F, nf, thr, nf - 1, nullptr, 0, rho, done, &neg, &more);
    if (SMCP_TID == 0) {
      a.rank[k] = rk;
      a.flag[k] = s_baddiag ? 2 : neg;
    }
    __syncthreads();
  }
}

// out[0] = max rank, out[1] = 1 + the lowest clique whose block is not an EDM (0: none), out[2] = cliques with a nonzero
// diagonal entry
__global__ void __launch_bounds__(MRC_NT) k_edm_reduce(const int32_t* rank, const int32_t* flag, int nsn, int32_t* out) {
  double best;
  const int q = mrc_argmax(nsn, [&](int k) { return (double)rank[k]; }, best);
  const int b = mrc_argmax(nsn, [&](int k) { return flag[k] == 1 ? -(double)k : -INFINITY; }, best);
  int bad = 0;
  if (SMCP_TID == 0) {
    for (int k = 0; k < nsn; ++k) bad += flag[k] == 2;
    out[0] = q >= 0 ? rank[q] : 0;
    out[1] = b >= 0 ? b + 1 : 0;
    out[2] = bad;
  }
}

// pass 2: see the head of the file.  Slot: edm_slot2(nn, na, r)
__global__ void __launch_bounds__(MRC_NT) k_edm_factor(MrcArgs a) {
  extern __shared__ double mrc_lds[];
  __shared__ double s_half;          // sigma / 2
  double* ws = a.ws ? a.ws + (int64_t)blockIdx.x * a.slot : mrc_lds;
  const int r = a.r;
  for (int e = blockIdx.x; e < a.cnt; e += gridDim.x) {
    const int k = a.lev[e];
    const CliqueDesc d = a.cl[k];
    const int nn = d.nn, na = d.na, nf = nn + na;
    const double* P = a.x + d.blk;
    const int32_t* rows = a.rowidx + d.rows;
    double* M = ws;                                  // r x na : W_A^T, then its QR
    double* W = M + (int64_t)r * na;                 // nn x r : [Z1 Z2 0], then W_N
    double* S = W + (int64_t)nn * r;                 // nn x nn: G_NN - Z1 Z1^T
    double* tau = S + (int64_t)nn * nn;              // na
    double* cn = tau + na;                           // na
    double* lv = cn + na;                            // nn: rho_N, then pchol scratch
    double* cv = lv + nn;                            // r : centroid of Y_A
    double* wn = cv + r;                             // na: |W_a|^2
    int* perm = (int*)(wn + na);                     // na
    int* done = perm + na + (na & 1);                // nn
    for (int t = SMCP_TID; t < r * na; t += MRC_NT) {
      const int c = t % r, i = t / r;
      M[t] = a.Y[(int64_t)rows[nn + i] * a.ldY + c];
    }
    for (int t = SMCP_TID; t < nn * r; t += MRC_NT) W[t] = 0.0;
    __syncthreads();
    for (int c = SMCP_TID; c < r; c += MRC_NT) {
      double s = 0.0;
      for (int i = 0; i < na; ++i) s += M[c + (int64_t)i * r];
      cv[c] = na ? s / na : 0.0;
    }
    __syncthreads();
    for (int t = SMCP_TID; t < r * na; t += MRC_NT) M[t] -= cv[t % r];
    __syncthreads();
    for (int i = SMCP_TID; i < na; i += MRC_NT) {
      double s = 0.0;
      for (int c = 0; c < r; ++c) s += M[c + (int64_t)i * r] * M[c + (int64_t)i * r];
      wn[i] = s;
    }
    // rho_i, i in N: the mean of D_ia over the separator, or (root) of D_ij over the clique
    for (int i = SMCP_TID; i < nn; i += MRC_NT) {
      double s = 0.0;
      if (na)
        for (int b = 0; b < na; ++b) s += P[(nn + b) + (int64_t)i * nf];
      else
        for (int b = 0; b < nn; ++b) s += i >= b ? P[i + (int64_t)b * nf] : P[b + (int64_t)i * nf];
      lv[i] = s / (na ? na : nn);
    }
    __syncthreads();
    if (SMCP_TID == 0) {
      double s = 0.0;
      if (na)
        for (int b = 0; b < na; ++b) s += wn[b];
      else
        for (int b = 0; b < nn; ++b) s += lv[b];
      s_half = na ? s / na : 0.5 * (s / nn);
    }
    __syncthreads();
    const double h = s_half;
    double md;
    mrc_argmax(nf, [&](int i) { return i < nn ? lv[i] - h : wn[i - nn]; }, md);
    const double thr = a.tol * (md > 0.0 ? md : 0.0);
    const int ra = na ? mrc_qrp(r, na, M, r, thr, tau, perm, cn) : 0;
    // G_ia = -1/2 (D_ia - rho_i - rho_a + sigma) with rho_a = |W_a|^2 + sigma/2: -1/2 (D_ia - rho_i - |W_a|^2 + sigma/2)
    for (int i = SMCP_TID; i < nn; i += MRC_NT)      // Z1 R11 = (G_NA P)[:, :ra], row by row
      for (int j = 0; j < ra; ++j) {
        const int b = perm[j];
        double z = -0.5 * (P[(int64_t)i * nf + nn + b] - lv[i] - wn[b] + h);
        for (int l = 0; l < j; ++l) z -= W[i + (int64_t)l * nn] * M[l + (int64_t)j * r];
        W[i + (int64_t)j * nn] = z / M[j + (int64_t)j * r];
      }
    __syncthreads();
    for (int t = SMCP_TID; t < nn * nn; t += MRC_NT) {
      const int i = t % nn, j = t / nn;
      if (i < j) continue;
      double s = -0.5 * (P[i + (int64_t)j * nf] - lv[i] - lv[j] + 2.0 * h);
      for (int l = 0; l < ra; ++l) s -= W[i + (int64_t)l * nn] * W[j + (int64_t)l * nn];
      S[t] = s;
    }
    __syncthreads();
    int neg, more;
    mrc_pchol(nn, S, nn, thr, r - ra, W + (int64_t)ra * nn, nn, lv, done, &neg, &more);
    // W_N = W Q^T = W H_{ra-1} ... H_0: every thread owns rows of W
    for (int i = SMCP_TID; i < nn; i += MRC_NT)
      for (int j = ra - 1; j >= 0; --j) {
        double w = W[i + (int64_t)j * nn];
        for (int c = j + 1; c < r; ++c) w += W[i + (int64_t)c * nn] * M[c + (int64_t)j * r];
        w *= tau[j];
        W[i + (int64_t)j * nn] -= w;
        for (int c = j + 1; c < r; ++c) W[i + (int64_t)c * nn] -= w * M[c + (int64_t)j * r];
      }
    __syncthreads();
    for (int t = SMCP_TID; t < nn * r; t += MRC_NT) {
      const int c = t % r, i = t / r;
      a.Y[(int64_t)(d.first + i) * a.ldY + c] = W[i + (int64_t)c * nn] + cv[c];
    }
    if (SMCP_TID == 0) a.flag[k] = more;
    __syncthreads();
  }
}

// ---- dense form (csp_edm_dense) ------------------------------------------------------------------------------------
constexpr int EDM_TILE = 64;       // output tile edge
constexpr int EDM_KC = 16;         // columns of Y staged per step

// D[i * ldD + j] = sum_c (Y[p_i, c] - Y[p_j, c])^2, p = perm (nullptr: identity), i, j < n.  One 64 x 64 tile per
// workgroup, a 4 x 4 block of it per thread.
__global__ void __launch_bounds__(MRC_NT) k_edm_dense(int64_t n, int r, const double* Y, int64_t ldY, const int64_t* perm,
                                                       double* D, int64_t ldD) {
  __shared__ double yi[EDM_TILE][EDM_KC + 1];
  __shared__ double yj[EDM_TILE][EDM_KC + 1];
  const int64_t i0 = (int64_t)blockIdx.y * EDM_TILE, j0 = (int64_t)blockIdx.x * EDM_TILE;
  const int ti = SMCP_TID / 16, tj = SMCP_TID % 16;      // rows ti + 16 u, columns tj + 16 v of the tile
  double acc[4][4] = {};
  for (int c0 = 0; c0 < r; c0 += EDM_KC) {
    for (int t = SMCP_TID; t < EDM_TILE * EDM_KC; t += MRC_NT) {
      const int q = t / EDM_KC, c = t % EDM_KC;
      const int64_t gi = i0 + q, gj = j0 + q;
      const bool cin = c0 + c < r;
      yi[q][c] = (cin && gi < n) ? Y[(perm ? perm[gi] : gi) * ldY + c0 + c] : 0.0;
      yj[q][c] = (cin && gj < n) ? Y[(perm ? perm[gj] : gj) * ldY + c0 + c] : 0.0;
    }
    __syncthreads();
    for (int c = 0; c < EDM_KC; ++c)
      for (int u = 0; u < 4; ++u)
        for (int v = 0; v < 4; ++v) {
          const double x = yi[ti + 16 * u][c] - yj[tj + 16 * v][c];
          acc[u][v] += x * x;
        }
    __syncthreads();
  }
  for (int u = 0; u < 4; ++u)
    for (int v = 0; v < 4; ++v) {
      const int64_t gi = i0 + ti + 16 * u, gj = j0 + tj + 16 * v;
      if (gi < n && gj < n) D[gi * ldD + gj] = acc[u][v];
    }
}

}  // namespace smcp
