// KKT layer on device: Amap / Aadj, Schur-complement build, solve_ closure (the dense Cholesky of H: dense_chol.hip).
// Mirrors kkt_chol of src/python/solvers.py:477-541 (and Amap/Aadj 369-386); included by capi.hip.

namespace {

using namespace smcp;

// y[i] = sum_e w_e a_e X[idx_e], one workgroup per (constraint i, rhs r) with four gathers in flight per thread (a
// constraint of synth50k has 11 k entries: one wave per constraint walked them in 178 dependent steps);
// X_r = X + r*ldx; y_r = y + r*ldy.  The partial sums are combined in a fixed order (deterministic).
// gridDim.z > 1: workgroup z takes the z-th share of the constraint's entries and writes its partial sum to y + z * pstride (the
// caller adds the shares in order: k_vec_axpby_parts)
__global__ void __launch_bounds__(1024) k_amap(int64_t m, const int64_t* cptr, const int64_t* cidx, const double* cwval,
                                               const double* X, int64_t ldx, double* y, int64_t ldy, int64_t pstride) {
  __shared__ double part[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nthr = blockDim.x;
  const int64_t i = blockIdx.x;
  const int r = blockIdx.y;
  const double* x = X + (int64_t)r * ldx;
  const int64_t c0 = cptr[i], c1 = cptr[i + 1], share = (c1 - c0 + gridDim.z - 1) / gridDim.z;
  const int64_t e0 = c0 + (int64_t)blockIdx.z * share, e1 = e0 + share < c1 ? e0 + share : c1;
  y += (int64_t)blockIdx.z * pstride;
  double acc = 0.0;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += 4 * nthr) {
    double w[4], v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t ee = e + (int64_t)q * nthr;
      w[q] = ee < e1 ? cwval[ee] : 0.0;
      v[q] = ee < e1 ? x[cidx[ee]] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc += w[q] * v[q];
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int q = 0; q < (nthr >> 6); ++q) s += part[q];
    y[i + (int64_t)r * ldy] = s;
  }
}

// X[rpos[q]] = sum over constraints touching that position of y[con] * val   (X pre-zeroed)
__global__ void k_aadj(int64_t rnnz, const int64_t* rpos, const int64_t* rptr, const int32_t* rcon,
                       const double* rval, const double* y, double* X) {
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= rnnz) return;
  double acc = 0.0;
  for (int64_t e = rptr[q]; e < rptr[q + 1]; ++e) acc += rval[e] * y[rcon[e]];
  X[rpos[q]] = acc;
}

// X[rpos[q]] -= the same sum: X <- X - Aadj(y) touching only the positions that carry constraint entries (solve_ forms
// bx - Aadj(y) in place this way: no cleared scratch vector, no pass over the whole of blkval)
__global__ void k_aadj_sub(int64_t rnnz, const int64_t* rpos, const int64_t* rptr, const int32_t* rcon,
                           const double* rval, const double* y, double* X) {
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= rnnz) return;
  double acc = 0.0;
  for (int64_t e = rptr[q]; e < rptr[q + 1]; ++e) acc += rval[e] * y[rcon[e]];
  X[rpos[q]] -= acc;
}

// U_r (pre-zeroed) <- A_{j0+r} scattered into blkval coordinates
__global__ void k_scatter_constraints(int64_t j0, const int64_t* cptr, const int64_t* cidx,
                                      const double* cval, double* U, int64_t ldu) {
  const int r = blockIdx.y;
  const int64_t j = j0 + r;
  double* u = U + (int64_t)r * ldu;
  for (int64_t e = cptr[j] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < cptr[j + 1];
       e += (int64_t)gridDim.x * blockDim.x)
    u[cidx[e]] = cval[e];
}

// U_q (pre-zeroed) <- A_{ids[q]} scattered into blkval coordinates
__global__ void k_scatter_constraints_ids(const int32_t* ids, const int64_t* cptr, const int64_t* cidx,
                                          const double* cval, double* U, int64_t ldu) {
  const int64_t j = ids[blockIdx.y];
  double* u = U + (int64_t)blockIdx.y * ldu;
  for (int64_t e = cptr[j] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < cptr[j + 1];
       e += (int64_t)gridDim.x * blockDim.x)
    u[cidx[e]] = cval[e];
}
// H[ids[i], ids[j]] <- Hd[i, j]  (md x md, both triangles)
__global__ void k_scatter_hd(const int32_t* ids, int md, const double* Hd, double* H, int64_t ldh) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < (int64_t)md * md; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e % md), j = (int)(e / md);
    H[ids[i] + (int64_t)ids[j] * ldh] = Hd[e];
  }
}
// V (n x ncols, zeroed) <- unit vectors: column q has a one in row kidx[q]
__global__ void k_unit_columns(const int32_t* kidx, int64_t ncols, double* V, int64_t n) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < ncols) V[kidx[q] + q * n] = 1.0;
}
// misc.SCMcolumn2 (misc.c:620-663): H[i, s] = tr(A_i S^-1 A_s S^-1) from V_s = S^-1[:, K_s], for every
// constraint i and the column-sparse constraints s of this chunk (one wave per pair; H is symmetric, both
// triangles are written).  voff[q]: first column of V_s inside V for the q-th sparse constraint of the chunk.
// owner / me (sharded over ranks by sparse constraint, kkt_schur_gram_part): owner[i] = the rank that computes the columns of
// constraint i, -1 for the swept (dense-class) constraints.  The partial matrices of the ranks are SUMMED, so a pair of
// sparse constraints owned by two different ranks must be written by one of them only: the owner of the smaller index.
__global__ void k_scm_columns(int64_t m, const int64_t* cptr, const int32_t* a_r, const int32_t* a_c, const double* cval,
                              const int32_t* slist, const int64_t* voff, const int32_t* rloc, const int32_t* cloc,
                              const double* V, int64_t n, double* H, int64_t ldh, const int32_t* owner = nullptr, int me = 0) {
  const int lane = threadIdx.x & 63;
  const int64_t i = blockIdx.x;
  const int64_t s = slist[blockIdx.y];
  if (owner && owner[i] >= 0 && owner[i] != me && i < s) return;
  const double* Vs = V + voff[blockIdx.y] * n;
  double acc = 0.0;
  for (int64_t q = cptr[i] + lane; q < cptr[i + 1]; q += 64) {
    const int r1 = a_r[q], c1 = a_c[q];
    const double beta = cval[q];
    double t = 0.0;
    for (int64_t p = cptr[s]; p < cptr[s + 1]; ++p) {
      const double alpha = (a_r[p] != a_c[p]) ? 2.0 * cval[p] : cval[p];
      const double* Vr = Vs + (int64_t)rloc[p] * n;
      const double* Vc = Vs + (int64_t)cloc[p] * n;
      double w = Vr[r1] * Vc[c1];
      if (r1 != c1) w += Vr[c1] * Vc[r1];
      t += alpha * w;
    }
    acc += beta * t;
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) { H[i + s * ldh] = acc; H[s + i * ldh] = acc; }
}

// y = a*y + x (length m), small
__global__ void k_vec_axpby(int64_t m, double a, const double* x, double b, double* y) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) y[i] = a * x[i] + b * y[i];
}
// y = b*y + a*(x_0 + x_1 + ... in order), x_z = x + z * pstride: the shares of a split k_amap
__global__ void k_vec_axpby_parts(int64_t m, double a, const double* x, int parts, int64_t pstride, double b, double* y) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double s = 0.0;
  for (int z = 0; z < parts; ++z) s += x[i + (int64_t)z * pstride];
  y[i] = a * s + b * y[i];
}

int amap_impl(csp_ctx* c, const double* X, int64_t ldx, int nrhs, double* y, int64_t ldy, hipStream_t st) {
  const DeviceCtx& D = c->D;
  // workgroup size by the average list length (short lists: LP / max-cut constraints have a handful of entries)
  const int64_t avg = D.m ? D.cnnz / D.m : 0;
  const int thr = avg > 4096 ? 1024 : (avg > 512 ? 256 : 64);
  launch(c, KID_amap, k_amap, dim3((unsigned)D.m, nrhs), dim3(thr), st, D.m,
                     D.cptr, D.cidx, D.cwval, X, ldx, y, ldy, (int64_t)0);
  return 0;
}
int aadj_impl(csp_ctx* c, const double* y, double* X, hipStream_t st) {
  const DeviceCtx& D = c->D;
  if (hipMemsetAsync(X, 0, sizeof(double) * c->S.blklen(), st) != hipSuccess) return SMCP_EHIP;
  if (D.rnnz)
    launch(c, KID_aadj, k_aadj, dim3((unsigned)((D.rnnz + 255) / 256)), dim3(256), st, D.rnnz, D.rpos,
                       D.rptr, D.rcon, D.rval, y, X);
  return 0;
}

// Uploads and allocations of a built constraint set.  Their order is part of the contract: the placement of the large
// buffers (ustack last) is what the measured step times were taken with.
int upload_constraint_tables(csp_ctx* c, const ConstraintTables& T, int64_t m, const int64_t* cptr, const int64_t* cidx,
                             const double* cval, SetupClock& clk) {
  DeviceCtx& D = c->D;
  const int64_t nnz = cptr[m], blklen = c->S.blklen();
  int rc = 0;                    // the first failure; nothing is uploaded or allocated after it
  auto up = [&](auto** dst, const auto& src) { if (!rc) rc = dev_upload(dst, src, D.mem); };
  auto upn = [&](auto** dst, const auto* src, int64_t n) { if (!rc) rc = dev_upload(dst, src, (size_t)n, D.mem); };
  auto alloc = [&](auto** dst, int64_t n) { if (!rc) rc = dev_alloc(dst, n, D.mem); };
  upn(&D.cptr, cptr, m + 1); upn(&D.cidx, cidx, nnz); upn(&D.cval, cval, nnz);
  up(&D.cwval, T.w);
  up(&D.rpos, T.rpos); up(&D.rptr, T.rptr); up(&D.rcon, T.rcon); up(&D.rval, T.rval);
  up(&D.a_r, T.ar); up(&D.a_c, T.ac); up(&D.s_rloc, T.rloc); up(&D.s_cloc, T.cloc);
  up(&D.dlist, T.dl); up(&D.slist, T.sl); up(&D.kidx, T.kidx);
  if (!T.sl.empty()) {
    alloc(&D.vbuf, T.vcols * c->S.n);
    if (!T.dl.empty()) alloc(&D.hd, (int64_t)(T.dl.size() * T.dl.size()));
  }
  if (T.has_leafgram) {
    up(&D.lg_eptr, T.lg_eptr); up(&D.lg_epk, T.epk); up(&D.lg_ew, T.ewv); up(&D.lg_remap, T.remap);
    alloc(&D.lg_tab, T.lg_children * T.lg_rec);
  }
  if (T.has_fam_terms) {
    up(&D.fz_no, T.fno); up(&D.fz_ptr, T.fptr); up(&D.fz_pk, T.fpk); up(&D.fz_s, T.fsv);
    alloc(&D.fz_slot, T.fz_nfam + 8);                                  // (+ the eight task counters of k_lf_assemble_fz)
    if (rc) return rc;
    HIPCHK(hipMemset(D.fz_slot, 0, sizeof(int32_t) * (T.fz_nfam + 8)));
  }
  if (T.has_entry_tables) { up(&D.kc_ij, T.kij); up(&D.kc_ptr, T.kptr); up(&D.kc_off, T.koff); up(&D.kc_val, T.kval); }
  if (rc) return rc;
  clk.mark("uploads");
  const int64_t ustack_cols = std::max(D.max_rhs, m);
  if ((rc = dev_alloc(&D.ustack, ustack_cols * blklen, D.mem))) return rc;
  // entries the sweeps never write (strict upper triangles of the NN blocks) must stay finite
  HIPCHK(hipMemset(D.ustack, 0, sizeof(double) * ustack_cols * blklen));
  clk.mark("swept stack");
  return 0;
}

}  // namespace

extern "C" {

int kkt_set_constraints(csp_ctx* c, int64_t m, const int64_t* cptr, const int64_t* cidx, const double* cval) {
  if (int rc = ready(c)) return rc;
  if (m < 1 || !cptr || !cidx || !cval) return SMCP_EINVAL;
  DeviceCtx& D = c->D;
  HIPCHK(hipSetDevice(D.device));
  // a Schur complement of the OUTGOING constraint set still waiting for its factorisation (deferred status): it is complete
  // and does not depend on what is replaced here -- factor it where it stands, on the stream it was built on
  if (int rc = chol_flush_own_stream(c)) return rc;
  D.ConstraintBufs::release(D.mem);
  c->gsl_key.clear();
  SetupClock clk("kkt_set_constraints");
  static int scm_off = -1;
  if (scm_off < 0) { const char* e = sw_str("SMCP_SCM"); scm_off = (e && e[0] == '0') ? 1 : 0; }
  ConstraintParams P;
  P.tnzcols = c->tnzcols;
  P.max_rhs = D.max_rhs;
  P.tmplen = D.tmplen;
  P.scm_on = !scm_off && !use_generic(c);
  P.fam = &c->fam;
  P.large_mask = &c->large_mask;
  P.famt_terms_ok = famt_terms_ok;
  P.lf_alds_maxnf = LF_ALDS_MAXNF;
  P.famt_child = FAMT_CHILD;
  // every host table first (constraints.cpp; an invalid entry leaves the context without constraints, its host lists untouched)
  ConstraintTables T;
  if (int rc = build_constraint_tables(c->S, P, m, cptr, cidx, cval, T, [&](const char* step, int) { clk.mark(step); })) return rc;
  c->h_kptr = std::move(T.h_kptr);
  c->h_slist = T.sl;
  if (int rc = upload_constraint_tables(c, T, m, cptr, cidx, cval, clk)) return rc;
  D.md = (int64_t)T.dl.size();
  D.ns = (int64_t)T.sl.size();
  if (D.ns) D.vcols = T.vcols;
  if (T.has_entry_tables) {
    D.kc_maxlist = T.kc_maxlist;
    D.fam_maxterms = T.fam_maxterms;
    D.fam_meanterms = T.fam_meanterms;
    D.kc_maxlist_large = T.kc_maxlist_large;
    D.kc_sorted = T.kc_sorted;
    D.lg_children = T.lg_children; D.lg_maxent = T.lg_maxent; D.lg_pairs = T.lg_pairs; D.lg_rows = T.lg_rows; D.lg_rec = T.lg_rec;
    c->lg_slot_of = std::move(T.lg_slot_of);
  }
  if (T.has_fz_levels) c->fz_levels = std::move(T.fz_levels);
  if (T.has_fam_terms) { D.fz_nfam = T.fz_nfam; D.fz_ok = true; }
  D.ustack_cols = std::max(D.max_rhs, m);
  D.m = m;
  D.cnnz = cptr[m];
  D.rnnz = (int64_t)T.rpos.size();
  return 0;
}

int kkt_set_tnzcols(csp_ctx* c, double tnzcols) {
  if (!c || !(tnzcols >= 0.0 && tnzcols <= 1.0)) return SMCP_EINVAL;
  c->tnzcols = tnzcols;
  return 0;
}

int kkt_amap(csp_ctx* c, const double* X, double* y, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!c->D.m) return SMCP_EINVAL;
  amap_impl(c, X, 0, 1, y, 0, (hipStream_t)stream);
  HIPCHK(end_call(c));
  return 0;
}

int kkt_aadj(csp_ctx* c, const double* y, double* X, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!c->D.m) return SMCP_EINVAL;
  if (int rc = aadj_impl(c, y, X, (hipStream_t)stream)) return rc;
  HIPCHK(end_call(c));
  return 0;
}

static bool use_gram(const csp_ctx* c) {
  static int g = -1;
  if (g < 0) { const char* e = sw_str("SMCP_GRAM"); g = (e && e[0] == '0') ? 0 : 1; }
  return g == 1 && !use_generic(c);
}

// Gram formulation of the whole Schur complement (what kkt_qr implies, solvers.py:414-420):
// H = G(A)^T G(A) with ONE leaves->root sweep per constraint, then one tall-skinny SYRK.
// ---- Gram formulation, in steps so that the multi-GPU driver can interleave the boundary exchange
static bool leafgram_ok(csp_ctx* c, int64_t mcols);
static int gram_prepare(csp_ctx* c, const double* L, const double* Y, hipStream_t st, bool allow_partial_fac = false) {
  DeviceCtx& D = c->D;
  const int64_t m = D.m, bl = c->S.blklen();
  D.qr_valid = false;      // the stack is about to be rewritten
  D.lg_nochild = false;    // ... by sweeps that decide anew whether the family children's panels are formed
  // the flag read after the sweeps must be theirs: a failed dense_potrf (Schur complement not positive definite) or
  // kkt_qr_factor leaves its own behind
  HIPCHK(zero_flag(c, st));
  prepare_yaa(c, Y, true, st, false, allow_partial_fac);
  if (int rc = prep_lk_cached(c, L, Y, st)) return rc;
  if (!D.kc_ptr) {   // the sweeps read their input from the stack: clear it and scatter the constraints into it
    HIPCHK(hipMemsetAsync(D.ustack, 0, sizeof(double) * m * bl, st));
    for (int64_t jb = 0; jb < m; jb += 65535)
      launch(c, KID_scatter_constraints, k_scatter_constraints, dim3(8, (unsigned)std::min<int64_t>(65535, m - jb)),
             dim3(256), st, jb, D.cptr, D.cidx, D.cval, D.ustack + jb * bl, bl);
  }
  HIPCHK(end_call(c));
  return 0;
}
// sorted blkval ranges with touching ones merged
static std::vector<std::pair<int64_t, int64_t>> gram_merge_ranges(int64_t nranges, const int64_t* ranges) {
  std::vector<std::pair<int64_t, int64_t>> rs;
  for (int64_t q = 0; q < nranges; ++q)
    if (ranges[2 * q + 1] > ranges[2 * q]) rs.push_back({ranges[2 * q], ranges[2 * q + 1]});
  std::sort(rs.begin(), rs.end());
  size_t w = 0;
  for (size_t q = 0; q < rs.size(); ++q) {
    if (w && rs[q].first <= rs[w - 1].second) rs[w - 1].second = std::max(rs[w - 1].second, rs[q].second);
    else rs[w++] = rs[q];
  }
  rs.resize(w);
  return rs;
}
// chunking of a Gram accumulation over `total` rows: ~one resident wave of workgroups (2 per CU) over all ranges
static int64_t gram_chunk_rows(int64_t total) {
  static int64_t minrows = 0;     // SMCP_GRAM_MINCHUNK (timing studies): smallest chunk of rows per workgroup
  if (!minrows) { const char* e = sw_str("SMCP_GRAM_MINCHUNK"); minrows = e ? atoll(e) : 512; if (minrows < GRAM_KS) minrows = GRAM_KS; }   // 512: one rank's share of an 8-rank job 0.202 -> 0.173 ms (with 2048 rows per workgroup two thirds of the chip idle); large problems are chunked by the second term
  return std::max<int64_t>(minrows, ((total / 512 + GRAM_KS - 1) / GRAM_KS) * GRAM_KS);
}
static int gram_count_chunks(const std::vector<std::pair<int64_t, int64_t>>& rs, int64_t chunk) {
  int n = 0;
  for (auto& r : rs) n += (int)((r.second - r.first + chunk - 1) / chunk);
  return n;
}
static int gram_reserve(csp_ctx* c, int64_t m, int nchunk, hipStream_t st) {
  DeviceCtx& D = c->D;
  const int nb = (int)((m + GRAM_BLK - 1) / GRAM_BLK), nblk = nb * (nb + 1) / 2;
  const int64_t need = (int64_t)nblk * nchunk * 64 * 256;
  return dev_grow(&D.gpart, &D.gpart_len, need, D.mem, st);
}
// ---- slice table of a set of blkval ranges (k_gram_diag128) and the family children inside them (k_leaf_gram) ----------
// Built on the host when the ranges (or the leaf switch) differ from the cached ones: a rank's ranges are the same at
// every step.  leaf: the panels of the family children are not in the stack -- their rows are left out of the slices and
// the cliques are listed for k_leaf_gram.
static int64_t gram_chunk_rows(int64_t total);
// early_first (leaf tables only): the rows of the cliques of levels 0 and 1 first, padded with empty slices to whole chunks, then
// the rest -- D.gsl_spw / D.gsl_early tell the consumers (the early part can be accumulated while the sweep is still above)
static int gram_tables(csp_ctx* c, const std::vector<std::pair<int64_t, int64_t>>& rs, bool leaf, hipStream_t st, bool early_first = false) {
  DeviceCtx& D = c->D;
  const Symbolic& S = c->S;
  std::vector<int64_t> key;
  key.reserve(2 * rs.size() + 1);
  for (auto& r : rs) { key.push_back(r.first); key.push_back(r.second); }
  key.push_back((leaf ? 1 : 0) | (early_first ? 2 : 0));
  if (key == c->gsl_key && D.gsl_start) return 0;
  std::vector<int64_t> start, late_start;
  std::vector<int32_t> len, late_len, list, slot;
  int nf = 0, nn = 0, na = 0;
  auto add_segment = [&](int64_t lo, int64_t hi) {
    // (early_first: a segment is cut at clique boundaries and each piece goes to the part its clique's level says)
    if (!early_first) {
      for (int64_t e = lo; e < hi; e += GRAM_KS) { start.push_back(e); len.push_back((int32_t)std::min<int64_t>(GRAM_KS, hi - e)); }
      return;
    }
    int64_t k = (int64_t)(std::upper_bound(S.blkptr.begin(), S.blkptr.end(), lo) - S.blkptr.begin()) - 1;
    for (int64_t p = lo; p < hi; ++k) {
      const int64_t q = std::min(hi, S.blkptr[k + 1]);
      const bool late = S.level[(size_t)k] >= 2;
      for (int64_t e = p; e < q; e += GRAM_KS) {
        (late ? late_start : start).push_back(e);
        (late ? late_len : len).push_back((int32_t)std::min<int64_t>(GRAM_KS, q - e));
      }
      p = q;
    }
  };
  for (auto& r : rs) {
    if (!leaf) { add_segment(r.first, r.second); continue; }
    int64_t k = (int64_t)(std::upper_bound(S.blkptr.begin(), S.blkptr.end(), r.first) - S.blkptr.begin()) - 1;
    int64_t seg_lo = r.first;
    for (; k < S.nsn && S.blkptr[k] < r.second; ++k) {
      if (c->fam[k] != 1) continue;
      const int64_t b = std::max(S.blkptr[k], r.first), e = std::min(S.blkptr[k + 1], r.second);
      if (b != S.blkptr[k] || e != S.blkptr[k + 1]) return SMCP_EINVAL;     // ranges are unions of whole cliques
      if (b > seg_lo) add_segment(seg_lo, b);
      seg_lo = e;
      list.push_back((int32_t)k);
      slot.push_back(c->lg_slot_of[(size_t)k]);
      nf = std::max(nf, (int)S.nf(k)); nn = std::max(nn, (int)S.nn(k)); na = std::max(na, (int)S.na(k));
    }
    if (r.second > seg_lo) add_segment(seg_lo, r.second);
  }
  D.gsl_spw = 0; D.gsl_early = 0;
  if (early_first) {
    const int64_t chunk = gram_chunk_rows((int64_t)(start.size() + late_start.size()) * GRAM_KS);
    const int spw = (int)(chunk / GRAM_KS);
    while (start.size() % (size_t)spw) { start.push_back(0); len.push_back(0); }       // whole chunks of early rows
    D.gsl_spw = spw;
    D.gsl_early = late_start.empty() ? 0 : (int)(start.size() / (size_t)spw);
    start.insert(start.end(), late_start.begin(), late_start.end());
    len.insert(len.end(), late_len.begin(), late_len.end());
  }
  // (two tables share each capacity; at least one element, so that a built table is never a null pointer)
  const int64_t nslice = std::max<int64_t>((int64_t)start.size(), 1), nlist = std::max<int64_t>((int64_t)list.size(), 1);
  int64_t cap_len = D.gsl_cap, cap_slot = D.lg_cap;
  if (int rc = dev_grow(&D.gsl_start, &D.gsl_cap, nslice, D.mem, st)) return rc;
  if (int rc = dev_grow(&D.gsl_len, &cap_len, nslice, D.mem, st)) return rc;
  if (int rc = dev_grow(&D.lg_list, &D.lg_cap, nlist, D.mem, st)) return rc;
  if (int rc = dev_grow(&D.lg_slot, &cap_slot, nlist, D.mem, st)) return rc;
  HIPCHK(hipStreamSynchronize(st));             // the tables may be in use by launches still queued
  if (!start.empty()) {
    HIPCHK(hipMemcpy(D.gsl_start, start.data(), start.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.gsl_len, len.data(), len.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  if (!list.empty()) {
    HIPCHK(hipMemcpy(D.lg_list, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.lg_slot, slot.data(), slot.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  D.gsl_n = (int)start.size();
  D.lg_cnt = (int)list.size();
  D.lg_nf = nf; D.lg_nn = nn; D.lg_na = na;
  c->gsl_key = key;
  return 0;
}

// may the Schur sweep of mcols constraints leave the panels of the family children to k_leaf_gram?  (SMCP_LEAFGRAM=0: no)
constexpr int LG_ECAP_MAX = 1024;
static bool leafgram_ok(csp_ctx* c, int64_t mcols) {
  static int on = -1;
  if (on < 0) { const char* e = sw_str("SMCP_LEAFGRAM"); on = (e && e[0] == '0') ? 0 : 1; }
  const DeviceCtx& D = c->D;
  if (!on || !c->leafgram_policy || use_generic(c) || !D.kc_ptr || !D.kc_ij || mcols > GRAM_BLK || mcols < 1 || D.lg_children <= 0) return false;
  if (D.lg_maxent > LG_ECAP_MAX) return false;
  // the pairs of entries cost ~ as much as half as many (row, constraint) pairs moved through HBM twice
  if (c->leafgram_policy < 2 && D.lg_pairs > D.lg_rows * mcols) return false;
  if (!D.lg_eptr || !D.lg_tab) return false;
  const int64_t np = mcols * (mcols + 1) / 2 + 1;
  const int ecap = (int)((std::max<int64_t>(D.lg_maxent, 2) + 1) & ~1);
  return np + leafgram_wave_doubles(D.lg_rec, ecap) <= (int64_t)(LDS_LIMIT / 8);
}

// partial tiles of the listed family children (gram_tables) -> the slots part[0 .. *nl) (at most leafgram_slots())
static int leafgram_slots(csp_ctx* c) {
  return c->D.ncu;
}
static int leafgram_partials(csp_ctx* c, int64_t mcols, const int32_t* ids, hipStream_t st, double* part, int* nl) {
  DeviceCtx& D = c->D;
  *nl = 0;
  if (!D.lg_cnt) return 0;
  const int ncu = leafgram_slots(c);
  const int64_t np = mcols * (mcols + 1) / 2;
  const int ecap = (int)((std::max<int64_t>(D.lg_maxent, 2) + 1) & ~1);
  const int wd = leafgram_wave_doubles(D.lg_rec, ecap);
  const int64_t lim = (int64_t)(LDS_LIMIT / 8);
  const int nw = (int)std::max<int64_t>(1, std::min<int64_t>(8, (lim - ((np + 1) & ~1)) / wd));
  const int nwg = (int)std::max<int64_t>(1, std::min<int64_t>(ncu, (D.lg_cnt + nw - 1) / nw));
  LeafGramArgs a;
  a.cl = D.cl; a.list = D.lg_list; a.slot = D.lg_slot; a.cnt = D.lg_cnt; a.LK = D.lk; a.yaa = D.yaa;
  a.tab = D.lg_tab; a.rec = D.lg_rec;
  a.eptr = D.lg_eptr; a.epk = D.lg_epk; a.ew = D.lg_ew; a.remap = ids ? D.lg_remap : nullptr;
  a.nr = (int)mcols; a.ecap = ecap;
  a.part = part; a.info = D.info;
  { static int sk = -1; if (sk < 0) { const char* e = sw_str("SMCP_LGSKIP"); sk = e ? atoi(e) : 0; } a.skip = sk; }
  launch_lds(c, KID_leaf_tables, k_leaf_tables, dim3(D.lg_cnt), dim3(64), (size_t)leaftab_doubles(D.lg_nf, D.lg_nn, D.lg_na) * sizeof(double), st,
             a, D.lg_nf, D.lg_nn, D.lg_na);
  const size_t lds = (size_t)(((np + 1) & ~1) + (int64_t)nw * wd) * sizeof(double);
  const int rt = (D.lg_rec + 63) / 64, et = (ecap + 63) / 64;
  bool ok = false;
#define SMCP_LG_CASE(RT, ET) \
  if (!ok && rt <= RT && et <= ET) { \
    static bool attr = false; \
    if (!attr) attr = hipFuncSetAttribute((const void*)k_leaf_pairs<RT, ET>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024) == hipSuccess; \
    if (!attr) return SMCP_EHIP; \
    launch_lds(c, KID_leaf_gram, k_leaf_pairs<RT, ET>, dim3(nwg), dim3(64 * nw), lds, st, a); \
    ok = true; \
  }
  SMCP_LG_CASE(12, 2) SMCP_LG_CASE(12, 4) SMCP_LG_CASE(24, 2) SMCP_LG_CASE(24, 4) SMCP_LG_CASE(24, 16)
  SMCP_LG_CASE(48, 4) SMCP_LG_CASE(48, 16)
#undef SMCP_LG_CASE
  if (!ok) return SMCP_EINVAL;
  *nl = nwg;
  return 0;
}

// k_gram_diag128 over the chunks c0 .. c1 - 1 of the slice table (spw slices each) into the partial slots of the same numbers
static void gram_launch_chunks(csp_ctx* c, int64_t m, int spw, int c0, int c1, int nchunk_total, hipStream_t st) {
  DeviceCtx& D = c->D;
  const int64_t bl = c->S.blklen();
  static int nw = -1;
  if (nw < 0) { const char* e = sw_str("SMCP_GRAM_NW"); nw = (e && e[0] == '4') ? 4 : ((e && e[0] == '8') ? 8 : 16); }
  const int mti = (int)((m + 15) / 16), npw = (mti * (mti + 1) / 2 + nw - 1) / nw;   // lower tiles per wave
  static int gskip = -1;     // ablation switch for timing studies only (SMCP_GSKIP: 1 = no MFMA phase, 2 = no global loads)
  if (gskip < 0) { const char* e = sw_str("SMCP_GSKIP"); gskip = e ? atoi(e) : 0; }
  const size_t lds = (size_t)GRAM_BLK * GRAM_LDK * sizeof(double);
  const int64_t* ss = D.gsl_start + (int64_t)c0 * spw;
  const int32_t* sl = D.gsl_len + (int64_t)c0 * spw;
  const int nsl = std::min<int>(D.gsl_n - c0 * spw, (c1 - c0) * spw);
  const dim3 grid((unsigned)(c1 - c0), 1);
#define SMCP_GRAM_CASE(N) case N: if (nw == 16) launch_lds(c, KID_gram_diag128, k_gram_diag128<(N <= 3 ? N : 3), 16>, grid, dim3(1024), lds, st, \
               (const double*)D.ustack, bl, (int)m, ss, sl, nsl, spw, (const double*)D.sw, D.gpart, c0, nchunk_total, gskip); \
             else if (nw == 8) launch_lds(c, KID_gram_diag128, k_gram_diag128<(N <= 5 ? N : 5), 8>, grid, dim3(512), lds, st, \
               (const double*)D.ustack, bl, (int)m, ss, sl, nsl, spw, (const double*)D.sw, D.gpart, c0, nchunk_total, gskip); \
             else launch_lds(c, KID_gram_diag128, k_gram_diag128<N, 4>, grid, dim3(256), lds, st, \
               (const double*)D.ustack, bl, (int)m, ss, sl, nsl, spw, (const double*)D.sw, D.gpart, c0, nchunk_total, gskip); break;
  switch (npw) {
    SMCP_GRAM_CASE(1) SMCP_GRAM_CASE(2) SMCP_GRAM_CASE(3) SMCP_GRAM_CASE(4) SMCP_GRAM_CASE(5)
    SMCP_GRAM_CASE(6) SMCP_GRAM_CASE(7) SMCP_GRAM_CASE(8) SMCP_GRAM_CASE(9)
  }
#undef SMCP_GRAM_CASE
}

// H = sum over the given blkval ranges of G^T W G (ranges: host array of nranges (begin, end) pairs); leaf: the stack
// lacks the panels of the family children (D.lg_nochild), whose Gram block k_leaf_gram supplies
static int gram_accumulate(csp_ctx* c, int64_t nranges, const int64_t* ranges, double* H, int64_t ldh, hipStream_t st,
                           int64_t mcols = -1, bool leaf = false, const int32_t* ids = nullptr) {
  DeviceCtx& D = c->D;
  const int64_t m = mcols < 0 ? D.m : mcols, bl = c->S.blklen();
  const std::vector<std::pair<int64_t, int64_t>> rs = gram_merge_ranges(nranges, ranges);
  int64_t total = 0;
  for (auto& r : rs) total += r.second - r.first;
  if (total <= 0) {
    HIPCHK(hipMemset2DAsync(H, ldh * sizeof(double), 0, m * sizeof(double), m, st));
    return 0;
  }
  const int nb = (int)((m + GRAM_BLK - 1) / GRAM_BLK);
  const int nblk = nb * (nb + 1) / 2;
  if (nblk == 1) {
    int spw, nchunk, ngram, nl = 0;
    Fork* side = (Fork*)c->side_fork;
    c->side_fork = nullptr;
    bool early_done = false;
    int early = 0;
    if (c->gpre.valid && leaf) {        // planned, and the leaf partials started, beside the large-front stage of the sweep (schur_gram)
      spw = c->gpre.spw; nchunk = c->gpre.nchunk; ngram = c->gpre.ngram; nl = c->gpre.nl;
      early_done = c->gpre.early_done; early = c->gpre.early;
    } else {
      if (side) { side->join(); delete side; side = nullptr; }
      if (int rc = gram_tables(c, rs, leaf, st)) return rc;
      const int64_t chunk = gram_chunk_rows((int64_t)D.gsl_n * GRAM_KS);
      spw = (int)(chunk / GRAM_KS);
      nchunk = std::max(1, (D.gsl_n + spw - 1) / spw);
      ngram = D.gsl_n > 0 ? nchunk : 0;
      if (int rc = gram_reserve(c, m, nchunk + (leaf ? leafgram_slots(c) : 0) + GRAM_RZ, st)) return rc;
      if (leaf) { if (int rc = leafgram_partials(c, m, ids, st, D.gpart + (int64_t)ngram * (64 * 256), &nl)) return rc; }
    }
    c->gpre.valid = false; c->gpre.early_done = false;
    // sixteen waves per workgroup (two workgroups per CU: eight waves per SIMD hide the staging and operand latency:
    // 0.96 ms with four waves, 0.75 with eight, 0.72 with sixteen; SMCP_GRAM_NW=4 / 8 select the smaller variants)
    static int nw = -1;
    if (nw < 0) { const char* e = sw_str("SMCP_GRAM_NW"); nw = (e && e[0] == '4') ? 4 : ((e && e[0] == '8') ? 8 : 16); }
    const int mti = (int)((m + 15) / 16), npw = (mti * (mti + 1) / 2 + nw - 1) / nw;   // lower tiles per wave
    static int gskip = -1;     // ablation switch for timing studies only (SMCP_GSKIP: 1 = no MFMA phase, 2 = no global loads)
    if (gskip < 0) { const char* e = sw_str("SMCP_GSKIP"); gskip = e ? atoi(e) : 0; }
    const size_t lds = (size_t)GRAM_BLK * GRAM_LDK * sizeof(double);
    (void)nw; (void)npw; (void)gskip; (void)lds;
    // (the chunks before c0 were accumulated beside the large-front stage of the sweep: gpre.early_done)
    const int c0 = early_done ? early : 0;
    if (D.gsl_n > 0 && nchunk > c0) gram_launch_chunks(c, m, spw, c0, nchunk, nchunk, st);
    if (side) { side->join(); delete side; }      // the leaf partials of the side branch
    if (ngram + nl >= 256 && D.gpart_len >= (int64_t)(ngram + nl + GRAM_RZ) * (64 * 256)) {
      // two stages: GRAM_RZ workgroups per tile, then their GRAM_RZ sums (slots behind the partial tiles: gram_reserve)
      double* const stage = D.gpart + (int64_t)(ngram + nl) * (64 * 256);
      launch(c, KID_gram_reduce, k_gram_reduce, dim3(64, 1, GRAM_RZ), dim3(1024), st, (const double*)D.gpart, ngram + nl, (int)m, H, ldh, stage);
      launch(c, KID_gram_reduce, k_gram_reduce, dim3(64, 1), dim3(256), st, (const double*)stage, GRAM_RZ, (int)m, H, ldh, (double*)nullptr);
    } else
    launch(c, KID_gram_reduce, k_gram_reduce, dim3(64, 1), dim3(ngram + nl >= 64 ? 1024 : 256), st, (const double*)D.gpart, ngram + nl, (int)m, H, ldh, (double*)nullptr);
    HIPCHK(end_call(c));
    return 0;
  }
  if (c->side_fork) { Fork* f = (Fork*)c->side_fork; c->side_fork = nullptr; f->join(); delete f; }
  c->gpre.valid = false;
  if (leaf) return SMCP_EINVAL;                 // leafgram_ok admits one block only
  const int64_t chunk = gram_chunk_rows(total);
  const int nchunk = gram_count_chunks(rs, chunk);
  if (int rc = gram_reserve(c, m, nchunk, st)) return rc;
  int coff = 0;
  for (auto& r : rs) {
    const int64_t lo = r.first, hi = r.second;
    const int nc = (int)((hi - lo + chunk - 1) / chunk);
    for (int bi = 0; bi < nb; ++bi)
      for (int bj = 0; bj <= bi; ++bj) {
        if (bi == bj)
          launch_lds(c, KID_gram_partial, k_gram_partial<true>, dim3(nc), dim3(256), (size_t)GRAM_KS * GRAM_LD * sizeof(double), st,
                     (const double*)D.ustack, bl, (int)m, lo, hi, (const double*)D.sw, chunk, D.gpart, coff, nchunk, bi, bj);
        else
          launch_lds(c, KID_gram_partial, k_gram_partial<false>, dim3(nc), dim3(256), (size_t)2 * GRAM_KS * GRAM_LD * sizeof(double), st,
                     (const double*)D.ustack, bl, (int)m, lo, hi, (const double*)D.sw, chunk, D.gpart, coff, nchunk, bi, bj);
      }
    coff += nc;
  }
  launch(c, KID_gram_reduce, k_gram_reduce, dim3(64, nblk), dim3(nchunk >= 64 ? 1024 : 256), st, (const double*)D.gpart, nchunk, (int)m, H, ldh, (double*)nullptr);
  HIPCHK(end_call(c));
  return 0;
}

// Gram formulation of the whole Schur complement (what kkt_qr implies, solvers.py:414-420):
// H = G(A)^T G(A) with ONE leaves->root sweep per constraint, then one tall-skinny SYRK.
// part / nparts (kkt_schur_gram_part): this caller's share of the column-sparse constraints -- a contiguous range of the
// sparse list -- and, for part 0, the Gram block of the swept ones; H must have been cleared, the parts are summed
static int schur_gram(csp_ctx* c, const double* L, const double* Y, double* H, int64_t ldh, hipStream_t st, int64_t part = 0,
                      int64_t nparts = 1) {
  DeviceCtx& D = c->D;
  const int64_t m = D.m, bl = c->S.blklen();
  if (!D.ns) {
    if (part) return 0;
    // (sweeps that take the family children's Gram block from k_leaf_pairs do not read those children's chol(Y_AA))
    if (int rc = gram_prepare(c, L, Y, st, leafgram_ok(c, m) && m <= D.max_rhs)) return rc;
    // (Accumulating the Gram tiles of the lower levels on a side stream while the large fronts are still swept was
    // measured in round 2 and dropped: 5.92 against 5.61 ms per step -- the two stages only take CUs from each other.)
    D.lg_request = leafgram_ok(c, m);
    // The closed-form Gram blocks of the family children depend on the factors only, not on the sweep: with one chunk of
    // right-hand sides they start on a side stream as soon as the extend-add of the first large level has been launched and
    // run beside the phase kernels of the top fronts (MFMA at a few workgroups per CU against VALU / LDS work: they share
    // the CUs instead of taking them from each other).  SMCP_LG_SIDE=0: after the sweep, on the caller's stream.
    static int lgside = -1;
    if (lgside < 0) {
      const char* e = sw_str("SMCP_LG_SIDE");
      const char* d0 = sw_str("SMCP_ALDS_DYN");
      const char* d1 = sw_str("SMCP_RHS_SPLIT_DYN");
      // (the two-stream split of the right-hand sides -- the plain extend-add launch, hess_up_fast -- uses the same side streams)
      lgside = ((e && e[0] == '0') || (d0 && d0[0] == '0') || (d1 && d1[0] == '1')) ? 0 : 1;
    }
    c->gpre.valid = false;
    if (lgside && D.lg_request && m <= D.max_rhs && Fork::enabled() && (m + GRAM_BLK - 1) / GRAM_BLK == 1) {
      c->side_work = [c, m, bl](hipStream_t side) {
        DeviceCtx& D = c->D;
        // (started before the family launch has decided -- SMCP_LG_EARLY -- the work is discarded by gram_accumulate when that launch
        // kept the children's panels after all: D.lg_nochild false)
        if (!D.lg_nochild && !D.lg_request) return;  // the family launch kept the children's panels: the Gram kernel takes them
        const int64_t range[2] = {0, bl};
        const std::vector<std::pair<int64_t, int64_t>> rs = gram_merge_ranges(1, range);
        // (round 5, measured and NOT the default: the Gram chunks of the rows of levels 0 / 1 -- 88 % of them on synth50k -- on the side
        // branch beside the phase kernels of the top fronts: k_gram_diag128 0.36 -> 0.66 ms, k_lf_up2 0.24 -> 0.50, the step 3.22 ->
        // 3.37 ms; started earlier still, beside the fused extend-add, that kernel goes 0.45 -> 0.75.  As in round 2: the stages take
        // CUs, LDS and L2 from each other.  SMCP_GRAM_EARLY=1 runs it.)
        static const int gearly = sw_on("SMCP_GRAM_EARLY", 0);
        if (gram_tables(c, rs, true, side, gearly != 0)) return;
        const int64_t chunk = gram_chunk_rows((int64_t)D.gsl_n * GRAM_KS);
        const int spw = D.gsl_spw ? D.gsl_spw : (int)(chunk / GRAM_KS);
        const int nchunk = std::max(1, (D.gsl_n + spw - 1) / spw);
        const int ngram = D.gsl_n > 0 ? nchunk : 0;
        if (gram_reserve(c, m, nchunk + leafgram_slots(c) + GRAM_RZ, side)) return;
        int nl = 0;
        if (leafgram_partials(c, m, nullptr, side, D.gpart + (int64_t)ngram * (64 * 256), &nl)) return;
        c->gpre.valid = true; c->gpre.ngram = ngram; c->gpre.nchunk = nchunk; c->gpre.spw = spw; c->gpre.nl = nl;
        c->gpre.early = D.gsl_early; c->gpre.early_done = false;
      };
      // behind level 1 of the sweep (hess_up_fast): the panels of the levels 0 and 1 are final -- their chunks of the Gram
      // accumulation go to the side branch (after the leaf partials already queued there), beside the large fronts above
      c->mid_work = [c, m](hipStream_t mainst) {
        Fork* f = (Fork*)c->side_fork;
        if (!f || !f->on || !c->gpre.valid || c->gpre.early <= 0 || !c->D.lg_nochild) return;
        if (hipEventRecord(c->aux_fork, mainst) != hipSuccess || hipStreamWaitEvent(f->s, c->aux_fork, 0) != hipSuccess) return;
        gram_launch_chunks(c, m, c->gpre.spw, 0, c->gpre.early, c->gpre.nchunk, f->s);
        c->gpre.early_done = true;
      };
    }
    // The closed-form leaf blocks start at once (SMCP_LG_EARLY=0: beside the phase kernels of the top fronts, as in round 3), beside the first launches of the sweep (the stray leaves, the
    // families' tables), instead of beside the phase kernels of the top fronts
    static int lgearly = -1;
    if (lgearly < 0) lgearly = sw_on("SMCP_LG_EARLY", 1);
    if (lgearly && c->side_work) {
      std::function<void(hipStream_t)> w = std::move(c->side_work);
      c->side_work = nullptr;
      Fork* f = new Fork(c, st, 1);
      c->side_fork = f;
      w(f->s);
    }
    for (int64_t jb = 0; jb < m; jb += D.max_rhs) {
      int nr = (int)std::min(D.max_rhs, m - jb);
      hess_up_fast(c, D.ustack + jb * bl, nr, bl, D.fac, 2, st, 0, D.kc_ptr ? jb : -1);     // G(A_j) = (G_NN, R^T G_AN)
    }
    c->side_work = nullptr;
    c->mid_work = nullptr;
    D.lg_request = false;
    const int64_t range[2] = {0, bl};
    if (int rc = gram_accumulate(c, 1, range, H, ldh, st, -1, D.lg_nochild)) return rc;
    if (int f = fetch_info(c, st)) return f;   // chol(Y_AA) failure
    return 0;
  }
  // ---- hybrid (solvers.py:479-497): Gram block of the swept constraints + SCMcolumn2 columns of the sparse ones
  const int64_t md = part == 0 ? D.md : 0, n = c->S.n;
  const int64_t qlo = D.ns * part / nparts, qhi = D.ns * (part + 1) / nparts;
  const int32_t* owner = nullptr;
  if (nparts > 1) {
    std::vector<int32_t> ow((size_t)m, -1);
    for (int64_t p = 0; p < nparts; ++p)
      for (int64_t q = D.ns * p / nparts; q < D.ns * (p + 1) / nparts; ++q) ow[(size_t)c->h_slist[(size_t)q]] = (int32_t)p;
    if (!D.scm_owner) { if (int rc = dev_alloc(&D.scm_owner, m, D.mem)) return rc; }
    HIPCHK(hipMemcpyAsync(D.scm_owner, ow.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));      // ow is a local
    owner = D.scm_owner;
  }
  if (md) {
    prepare_yaa(c, Y, true, st);
    if (int rc = prep_lk_cached(c, L, Y, st)) return rc;
    if (!D.kc_ptr) {
      HIPCHK(hipMemsetAsync(D.ustack, 0, sizeof(double) * md * bl, st));
      for (int64_t jb = 0; jb < md; jb += 65535)
        launch(c, KID_scatter_constraints, k_scatter_constraints_ids, dim3(8, (unsigned)std::min<int64_t>(65535, md - jb)),
               dim3(256), st, (const int32_t*)D.dlist + jb, D.cptr, D.cidx, D.cval, D.ustack + jb * bl, bl);
    }
    D.lg_nochild = false;
    D.lg_request = leafgram_ok(c, md);
    for (int64_t jb = 0; jb < md; jb += D.max_rhs) {
      int nr = (int)std::min(D.max_rhs, md - jb);
      hess_up_fast(c, D.ustack + jb * bl, nr, bl, D.fac, 2, st, 0, D.kc_ptr ? jb : -1, D.kc_ptr ? D.dlist : nullptr);
    }
    D.lg_request = false;
    const int64_t range[2] = {0, bl};
    if (int rc = gram_accumulate(c, 1, range, D.hd, md, st, md, D.lg_nochild, D.kc_ptr ? D.dlist : nullptr)) return rc;
    launch(c, KID_scatter_constraints, k_scatter_hd, dim3((unsigned)std::min<int64_t>(1024, (md * md + 255) / 256)), dim3(256), st,
           (const int32_t*)D.dlist, (int)md, (const double*)D.hd, H, ldh);
  }
  // sparse constraints in chunks of at most vcols columns of S^-1
  std::vector<int64_t> voff;
  for (int64_t q0 = qlo; q0 < qhi;) {
    int64_t q1 = q0, cols = 0;
    voff.clear();
    while (q1 < qhi && cols + (c->h_kptr[q1 + 1] - c->h_kptr[q1]) <= D.vcols && q1 - q0 < 65535) {
      voff.push_back(cols);
      cols += c->h_kptr[q1 + 1] - c->h_kptr[q1];
      ++q1;
    }
    if (q1 == q0) return SMCP_ENOMEM;   // cannot happen: vcols >= max |K_s|
    HIPCHK(hipMemsetAsync(D.vbuf, 0, sizeof(double) * cols * n, st));
    launch(c, KID_scatter_constraints, k_unit_columns, dim3((unsigned)((cols + 255) / 256)), dim3(256), st,
           (const int32_t*)D.kidx + c->h_kptr[q0], cols, D.vbuf, n);
    if (int rc = trsm_impl(c, L, Y, D.vbuf, cols, n, 0, st)) return rc;      // V = L^-T L^-1 E_K  (solvers.py:491-492)
    if (int rc = trsm_impl(c, L, Y, D.vbuf, cols, n, 1, st)) return rc;
    // chunk offsets: a small device array behind the reduction scratch would not fit 65535 entries; use tmp's head
    int64_t* dvoff = reinterpret_cast<int64_t*>(D.tmp);
    HIPCHK(hipMemcpyAsync(dvoff, voff.data(), sizeof(int64_t) * voff.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));    // voff is reused by the next chunk
    launch(c, KID_scatter_constraints, k_scm_columns, dim3((unsigned)m, (unsigned)(q1 - q0)), dim3(64), st, m, D.cptr,
           (const int32_t*)D.a_r, (const int32_t*)D.a_c, (const double*)D.cval, (const int32_t*)D.slist + q0,
           (const int64_t*)dvoff, (const int32_t*)D.s_rloc, (const int32_t*)D.s_cloc, (const double*)D.vbuf, n, H, ldh, owner, (int)part);
    q0 = q1;
  }
  HIPCHK(end_call(c));
  if (md) { if (int f = fetch_info(c, st)) return f; }
  return 0;
}

int kkt_schur_columns(csp_ctx* c, const double* L, const double* Y, double* H, int64_t ldh, int64_t j0,
                      int64_t j1, void* stream) {
  if (int rc = ready(c)) return rc;
  DeviceCtx& D = c->D;
  const int64_t m = D.m, bl = c->S.blklen();
  if (!m || ldh < m || j0 < 0 || j1 > m || j0 > j1) return SMCP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  D.qr_valid = false;
  chol_drop_pending(c, H);
  HIPCHK(zero_flag(c, st));
  if (j0 == 0 && j1 == m && use_gram(c)) return schur_gram(c, L, Y, H, ldh, st);
  prepare_yaa(c, Y, false, st);
  if (!use_generic(c)) { if (int rc = prep_lk_cached(c, L, Y, st)) return rc; }
  for (int64_t jb = j0; jb < j1; jb += D.max_rhs) {
    int nr = (int)std::min(D.max_rhs, j1 - jb);
    HIPCHK(hipMemsetAsync(D.ustack, 0, sizeof(double) * nr * bl, st));
    launch(c, KID_scatter_constraints, k_scatter_constraints, dim3(8, nr), dim3(256), st, jb, D.cptr, D.cidx,
           D.cval, D.ustack, bl);
    hessian_impl(c, L, D.ustack, nr, bl, 2, 0, st);
    // H[:, jb+r] = Amap(W(A_{jb+r}))  (full column; H is symmetric)
    amap_impl(c, D.ustack, bl, nr, H + jb * ldh, ldh, st);
  }
  HIPCHK(end_call(c));
  return 0;
}

// The hybrid Schur complement (Gram block of the swept constraints + SCMcolumn2 columns of the column-sparse ones,
// solvers.py:479-497, misc.c:620-663) sharded over `nparts` callers by sparse constraint: this one computes the columns of
// its contiguous share of the sparse list (trsm x 2 + k_scm_columns per chunk) and, as part 0, the Gram block.  H (cleared
// by the caller) receives this part only; the sum of the parts over all callers is the Schur complement (both triangles).
int kkt_schur_gram_part(csp_ctx* c, const double* L, const double* Y, double* H, int64_t ldh, int64_t part, int64_t nparts,
                        void* stream) {
  if (int rc = ready(c)) return rc;
  DeviceCtx& D = c->D;
  if (!D.m || ldh < D.m || nparts < 1 || part < 0 || part >= nparts || !use_gram(c)) return SMCP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  D.qr_valid = false;
  chol_drop_pending(c, H);
  HIPCHK(zero_flag(c, st));
  return schur_gram(c, L, Y, H, ldh, st, part, nparts);
}
// how kkt_set_constraints classified the constraints (misc.nzcolumns / matperm, misc.c:682-773): counts[0] = swept through the
// Hessian (dense class), counts[1] = column-sparse (SCMcolumn2 route)
int kkt_constraint_classes(csp_ctx* c, int64_t* counts) {
  if (!c || !counts) return SMCP_EINVAL;
  counts[0] = c->D.ns ? c->D.md : c->D.m;
  counts[1] = c->D.ns;
  return 0;
}
static bool potrf_defer_on() {
  static int on = -1;
  if (on < 0) { const char* e = sw_str("SMCP_POTRF_DEFER"); on = (e && e[0] == '0') ? 0 : 1; }
  return on == 1;
}
int kkt_schur_factor(csp_ctx* c, const double* L, const double* Y, double* H, int64_t ldh, void* stream) {
  // ONE matrix can wait for its factorisation: a pending Schur complement of another system on this context (two KKT systems
  // may share a Symbolic) is factored where it stands before this one takes the slot, so its solve_ never meets a raw H
  if (c) { if (int rc = chol_flush(c, (hipStream_t)stream, nullptr, H)) return rc; }
  if (int rc = kkt_schur_columns(c, L, Y, H, ldh, 0, c ? c->D.m : 0, stream)) return rc;
  if (c->lazy_status && !use_generic(c) && potrf_defer_on() && Fork::enabled()) {
    // deferred status: nobody waits for potrf's verdict here, so the factorisation itself can wait for the first solve_
    // (kkt_solve runs it beside its first Hessian sweep) or for whoever reads H first (chol_flush)
    chol_defer(c, H, c->D.m, ldh, (hipStream_t)stream);
    return 0;
  }
  return dense_potrf(c, H, c->D.m, ldh, stream);
}
// The caller is about to free (or reuse) the memory of H: whatever the context still remembers about it -- the mark of a
// factorisation that kkt_schur_factor deferred, the mark of a factor made here -- is dropped, nothing is launched.
int kkt_schur_forget(csp_ctx* c, const double* H) {
  if (!c || !H) return SMCP_EINVAL;
  chol_forget(c, H);
  return 0;
}

int kkt_solve(csp_ctx* c, const double* L, const double* Y, const double* H, int64_t ldh, double kk,
              double* bx, double* by, void* stream) {
  if (int rc = ready(c)) return rc;
  DeviceCtx& D = c->D;
  const int64_t m = D.m, bl = c->S.blklen();
  if (!m) return SMCP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  D.qr_valid = false;          // r1 below overwrites the first row of the stack
  double* r1 = D.ustack;       // blkval-sized temporaries
  double* ytmp = D.red + 600;  // (m <= 400 fits; larger m uses the tail of ustack)
  if (m > 400) {
    if (D.max_rhs < 2) return SMCP_ENOMEM;
    ytmp = D.ustack + bl;
  }
  HIPCHK(zero_flag(c, st));
  // a Schur complement that kkt_schur_factor left unfactored (deferred status): its Cholesky on a side stream beside the first
  // Hessian sweep, which does not read H -- with a failure flag of its own, latched by the branch itself
  std::unique_ptr<Fork> hf;
  if (double* Hw = chol_take_pending(c, H)) {
    // (only under deferred status: an eager caller -- the status regime may have been switched since kkt_schur_factor -- gets
    // the verdict of this factorisation as the return value, through the in-stream branch)
    hf.reset(c->lazy_status ? new Fork(c, st, 0) : nullptr);
    if (hf && hf->on) {
      int* pinfo = c->D.info + 20;
      if (int rc = potrf_launch(c, Hw, m, ldh, hf->s, pinfo)) return rc;
      census_note(c, k_latch_status);
      hipLaunchKernelGGL(k_latch_status, dim3(1), dim3(64), 0, hf->s, pinfo, 1, c->D.info + 16);
    } else {                                    // no side stream: where it stands, status latched as after dense_potrf
      hf.reset();
      if (int rc = potrf_launch(c, Hw, m, ldh, st, c->D.info)) return rc;
      if (int rc = fetch_info(c, st)) return rc;
      HIPCHK(zero_flag(c, st));
    }
    chol_mark_factored(c, H, m);
  } else if (int rc = chol_flush(c, st)) return rc;    // (another matrix is pending: factor it where it stands)
  // the Y_AA cache must correspond to (L, Y): recompute (cheap, one gather sweep)
  if (!(c->D.yaa_tag == Y && c->D.yaa_tag)) prepare_yaa(c, Y, false, st);
  if (!use_generic(c)) { if (int rc = prep_lk_cached(c, L, Y, st)) return rc; }
  HIPCHK(hipMemcpyAsync(r1, bx, sizeof(double) * bl, hipMemcpyDeviceToDevice, st));
  hessian_impl(c, L, r1, 1, bl, 2, 0, st);                      // r1 = W(bx)
  {
    // Amap(r1), then y = kk*by + Amap(r1).  Few long constraints (synth50k: 100 of 11 k entries each) leave most of the chip idle
    // with one workgroup per constraint, each thread walking three rounds of dependent gathers: the entries are dealt over
    // `parts` workgroups per constraint and the shares added in order by the update of y (deterministic)
    const int64_t avg = D.m ? D.cnnz / D.m : 0;
    int parts = 1;
    if (avg > 4096 && m <= 400) parts = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)8, (2 * (int64_t)D.ncu) / std::max<int64_t>(m, 1), avg / 2048, (int64_t)3072 / std::max<int64_t>(m, 1)}));
    if (parts <= 1) {
      amap_impl(c, r1, 0, 1, ytmp, 0, st);
      launch(c, KID_vec_axpby, k_vec_axpby, dim3((unsigned)((m + 255) / 256)), dim3(256), st, m, 1.0, ytmp, kk, by);
    } else {
      double* const ypart = D.red + 1024;
      launch(c, KID_amap, k_amap, dim3((unsigned)m, 1, (unsigned)parts), dim3(1024), st, m, D.cptr, D.cidx, D.cwval, (const double*)r1, (int64_t)0,
             ypart, (int64_t)0, m);
      launch(c, KID_vec_axpby, k_vec_axpby_parts, dim3((unsigned)((m + 255) / 256)), dim3(256), st, m, 1.0, (const double*)ypart, parts, m, kk, by);
    }
  }
  if (hf) hf->join();                                           // H is factored from here on
  if (int rc = potrs_impl(c, H, m, ldh, by, 1, m, st)) return rc;
  // x = W(Aadj(y) - bx) / kk = -W(bx - Aadj(y)) / kk: the subtraction touches the constraint entries' positions only (no cleared
  // blkval-sized vector, no axpby over the whole of it: 28 us of three launches on synth50k), the sign rides on the final scaling
  if (D.rnnz)
    launch(c, KID_aadj, k_aadj_sub, dim3((unsigned)((D.rnnz + 255) / 256)), dim3(256), st, D.rnnz, D.rpos, D.rptr, D.rcon, D.rval,
           (const double*)by, bx);
  hessian_impl(c, L, bx, 1, bl, 2, 0, st);
  launch(c, KID_axpby, k_axpby, dim3(1024), dim3(256), st, bl, 0.0, (const double*)nullptr, -1.0 / kk, bx);
  HIPCHK(end_call(c));
  return 0;
}


// ---- subtree-sharded Gram path (multi-GPU; orchestrated by smcp_amd/kkt.py ShardedSchur) ----------
int csp_set_partition(csp_ctx* c, const int32_t* owner, int rank) {
  if (int rc = ready(c)) return rc;
  const Symbolic& S = c->S;
  HIPCHK(hipSetDevice(c->D.device));
  c->PartitionTables::release(c->D.mem);
  for (int set = 1; set <= 2; ++set) {
    LevelSet& LS = c->sets[set];
    std::vector<int32_t> lev2;
    const int want = (set == 1) ? rank : -1;
    classify_levels(S, [&](int64_t k) { return owner[k] == want; }, LS.lvl, lev2, LS.off);
    if (int rc = dev_upload(&LS.lev2, lev2, c->D.mem)) return rc;
  }
  // subtree roots (owned clique whose parent lies in the replicated top), rank by rank in ascending clique order
  int world = 0;
  for (int64_t k = 0; k < S.nsn; ++k) world = std::max(world, owner[k] + 1);
  std::vector<int32_t> roots, own;
  std::vector<int64_t> bptr;
  c->xr_size.assign(std::max(world, rank + 1), 0);
  c->xr_npmax = 1;
  for (int r = 0; r < world; ++r)
    for (int64_t k = 0; k < S.nsn; ++k)
      if (owner[k] == r && S.snpar[k] >= 0 && owner[S.snpar[k]] == -1) {
        const int64_t np = S.na(k) * (S.na(k) + 1) / 2;
        roots.push_back((int32_t)k); own.push_back(r); bptr.push_back(c->xr_size[r]);
        c->xr_size[r] += np;
        c->xr_npmax = std::max(c->xr_npmax, np);
      }
  c->xr_n = (int64_t)roots.size(); c->xr_me = rank; c->xr_world = world;
  // may the owned sweeps leave the family parents' updates to the extend-add above (fz_on)?  Only when no family parent of this
  // rank is a subtree root: a root's update is what the boundary exchange packs, so it has to exist in the exchange buffer
  c->fz_set1_ok = true;
  for (int64_t k = 0; k < S.nsn; ++k)
    if (k < (int64_t)c->fam.size() && c->fam[(size_t)k] == 2 && owner[k] == rank && (S.snpar[k] < 0 || owner[S.snpar[k]] != rank)) c->fz_set1_ok = false;
  if (int rc = dev_upload(&c->xr_roots, roots, c->D.mem)) return rc;
  if (int rc = dev_upload(&c->xr_owner, own, c->D.mem)) return rc;
  if (int rc = dev_upload(&c->xr_bptr, bptr, c->D.mem)) return rc;
  return 0;
}
int kkt_gram_prepare(csp_ctx* c, const double* L, const double* Y, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!c->D.m || use_generic(c)) return SMCP_EINVAL;
  return gram_prepare(c, L, Y, (hipStream_t)stream);
}
// the same when the factor (L, Y) is valid on the owned cliques and the top only: kkt_prepare_part has been called
// for both sets; this clears the failure flag and rewrites the input stack if the sweeps read their input from it
int kkt_gram_prepare_part(csp_ctx* c, void* stream) {
  if (int rc = ready(c)) return rc;
  DeviceCtx& D = c->D;
  if (!D.m || use_generic(c)) return SMCP_EINVAL;
  if (!D.part_valid) return SMCP_ESTALE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t m = D.m, bl = c->S.blklen();
  D.qr_valid = false;
  D.lg_nochild = false;
  if (!D.kc_ptr) {
    HIPCHK(hipMemsetAsync(D.ustack, 0, sizeof(double) * m * bl, st));
    for (int64_t jb = 0; jb < m; jb += 65535)
      launch(c, KID_scatter_constraints, k_scatter_constraints, dim3(8, (unsigned)std::min<int64_t>(65535, m - jb)),
             dim3(256), st, jb, D.cptr, D.cidx, D.cval, D.ustack + jb * bl, bl);
  }
  HIPCHK(end_call(c));
  return 0;
}
int kkt_gram_sweep(csp_ctx* c, int set, int64_t j0, int64_t j1, void* stream) {
  if (int rc = ready(c)) return rc;
  DeviceCtx& D = c->D;
  if (set < 0 || set > 2 || j0 < 0 || j1 > D.m || j1 <= j0 || j1 - j0 > D.max_rhs) return SMCP_EINVAL;
  if (set && !c->sets[set].lev2) return SMCP_EINVAL;
  const int64_t bl = c->S.blklen();
  D.lg_request = leafgram_ok(c, D.m);
  hess_up_fast(c, D.ustack + j0 * bl, (int)(j1 - j0), bl, D.fac, 2, (hipStream_t)stream, set, D.kc_ptr ? j0 : -1);
  D.lg_request = false;
  HIPCHK(end_call(c));
  return 0;
}
int kkt_gram_accumulate(csp_ctx* c, int64_t nranges, const int64_t* ranges, double* H, int64_t ldh, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!c->D.m || ldh < c->D.m || nranges < 0) return SMCP_EINVAL;
  if (int rc = gram_accumulate(c, nranges, ranges, H, ldh, (hipStream_t)stream, -1, c->D.lg_nochild)) return rc;
  return fetch_info(c, (hipStream_t)stream);
}
// ---- sharded factorisation and solve (every leaves->root / root->leaves sweep shards by subtree) ----
// Y_AA blocks and their Cholesky factors of the cliques of one set (1 = owned, 2 = replicated top; call 2 before 1:
// a subtree root gathers from its parent's panel, which lies in the top); with_lk: also the inverse-form factor of L.
int kkt_prepare_part(csp_ctx* c, const double* L, const double* Y, int set, int with_lk, void* stream) {
  if (int rc = ready(c)) return rc;
  if (set < 1 || set > 2 || !c->sets[set].lev2 || use_generic(c) || !use_large()) return SMCP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  DeviceCtx& D = c->D;
  D.yaa_tag = D.fac_tag = D.faci_tag = nullptr;        // partial content: nothing to claim for the caches
  D.lk_tag_L = D.lk_tag_Y = nullptr;
  D.part_valid = false;
  D.part_Y = nullptr;
  D.fac_gen++;
  if (set == 2) HIPCHK(zero_flag(c, st));
  if (with_lk) prep_lk_set(c, set, L, st);
  gather_set(c, set, Y, 0, 1, D.yaa, st);
  {
    // fac <- yaa on the blocks of THIS set only: the other set's blocks may already hold their factors (a copy of the
    // whole array for set 1 used to put the unfactored Y_AA back over the factors of the top, set 2 -- unnoticed as long
    // as the top was a root without separator)
    TreeArgs t = tree_args(c);
    const LevelSet& LS = c->sets[set];
    for (int64_t l = 0; l < c->S.nlev; ++l) {
      const int cnt = (int)(LS.lvl[l].nI + LS.lvl[l].nII);
      if (!cnt) continue;
      t.lev = LS.lev2 + LS.off[l];
      const int namax = std::max(LS.lvl[l].namaxI, LS.lvl[l].namaxII);
      if (!namax) continue;
      launch(c, KID_axpby, k_copy_upd_blocks, dim3(cnt, umax1(std::min(64, (namax * namax + 1023) / 1024))), dim3(256), st, t,
             (const double*)D.yaa, D.fac);
    }
  }
  MfmaArgs a0 = mfma_args(c, nullptr, 0, 1);
  for (int64_t l = 0; l < c->S.nlev; ++l)
    for_level_classes(c, l, a0, [&](bool lds, MfmaArgs am, int cnt, size_t, int) {
      if (!am.namax) return;
      if (lds) {
        size_t bytes = ((size_t)padld(am.namax) * am.namax + 256 + 8) * sizeof(double);
        launch_lds(c, KID_factor_yaa_lds, k_factor_yaa_lds, dim3(cnt), dim3(fact_threads(am, 256, 2)), bytes, st, am, (const double*)D.yaa, D.fac);
      } else lf_factor_yaa(c, am, cnt, D.fac, st);
    }, set);
  HIPCHK(end_call(c));
  if (set == 2) return 0;
  if (int rc = fetch_info(c, st)) return rc;
  D.part_valid = true;
  D.part_Y = Y;          // (the root blocks of Y serve the fronts without separator in csp_hessian_sweep_part: Z_NN = Y_NN F_NN Y_NN)
  return 0;
}
// one half of the Hessian hessian(L, Y, U, adj=None) over the cliques of a set: dir 0 = leaves->root (with the Y_AA
// scaling of the separator rows), dir 1 = root->leaves.  The caller exchanges the packed updates of the subtree roots
// between the owned and the top pass of dir 0 (csp_exchange_pack / unpack); dir 1 needs no exchange.
int csp_hessian_sweep_part(csp_ctx* c, double* U, int64_t nrhs, int64_t ldu, int set, int dir, void* stream) {
  if (int rc = ready(c)) return rc;
  if (set < 1 || set > 2 || !c->sets[set].lev2 || use_generic(c) || nrhs < 1 || nrhs > c->D.max_rhs) return SMCP_EINVAL;
  if (!c->D.part_valid) return SMCP_ESTALE;
  hipStream_t st = (hipStream_t)stream;
  // (the two halves of a set always come as a pair -- the caller runs dir 1 of every set after dir 0 of every set -- so the
  // fronts without separator take both together, as in hessian_impl)
  if (dir == 0) hess_up_fast(c, U, (int)nrhs, ldu, c->D.yaa, 1, st, set, -1, nullptr, 0, -1, c->D.part_Y);
  else hess_down_fast(c, U, (int)nrhs, ldu, nullptr, 0, st, set, c->D.part_Y);
  HIPCHK(end_call(c));
  return 0;
}
// boundary exchange of the subtree partition: doubles per right-hand side that every rank contributes (host array of
// `world` entries), pack of this rank's subtree roots into buf ([root][rhs][packed block]) and unpack of all OTHER ranks'
// roots from the all-gathered buffers (`width` doubles per rank).  One launch each; nothing is allocated or waited for.
int csp_exchange_sizes(csp_ctx* c, int64_t world, int64_t* sizes) {
  if (!c || !sizes || world < 1) return SMCP_EINVAL;
  for (int64_t r = 0; r < world; ++r) sizes[r] = r < (int64_t)c->xr_size.size() ? c->xr_size[r] : 0;
  return 0;
}
static int exchange_roots(csp_ctx* c, int64_t nrhs, double* buf, int64_t width, int unpack, void* stream, int64_t r0 = 0) {
  if (int rc = ready(c)) return rc;
  if (c->xr_me < 0 || nrhs < 1 || r0 < 0 || r0 + nrhs > c->D.max_rhs || !buf) return SMCP_EINVAL;
  if (!c->xr_n) return 0;
  launch(c, KID_axpby, k_exchange_roots, dim3((unsigned)std::min<int64_t>(32, (c->xr_npmax + 255) / 256), (unsigned)c->xr_n, (unsigned)nrhs),
         dim3(256), (hipStream_t)stream, (const CliqueDesc*)c->D.cl, (const int32_t*)c->xr_roots, (const int32_t*)c->xr_owner,
         (const int64_t*)c->xr_bptr, c->xr_me, (int)nrhs, c->D.updp, c->D.updp_stride ? c->D.updp_stride : c->S.updplen(), buf, width, unpack, (int)r0);
  HIPCHK(end_call(c));
  return 0;
}
int csp_exchange_combine(csp_ctx* c, int64_t nrhs, const double* y, const double* gbuf, int64_t gwidth, double* out, int64_t owidth,
                         int mode, void* stream) {
  if (int rc = ready(c)) return rc;
  if (c->xr_me < 0 || nrhs < 1 || !y || !gbuf || !out || mode < 0 || mode > 1) return SMCP_EINVAL;
  if (!c->xr_n) return 0;
  launch(c, KID_axpby, k_exchange_combine, dim3((unsigned)std::min<int64_t>(32, (c->xr_npmax + 255) / 256), (unsigned)c->xr_n),
         dim3(256), (hipStream_t)stream, (const CliqueDesc*)c->D.cl, (const int32_t*)c->xr_roots, (const int32_t*)c->xr_owner,
         (const int64_t*)c->xr_bptr, c->xr_me, (int)nrhs, y, gbuf, gwidth, out, owidth, mode);
  HIPCHK(end_call(c));
  return 0;
}
int csp_exchange_pack(csp_ctx* c, int64_t nrhs, double* buf, void* stream) { return exchange_roots(c, nrhs, buf, 0, 0, stream); }
// The exchange BY CONSTRAINT SHARE (round 5: the top of the tree sharded by constraint instead of replicated for all of them):
// pack the right-hand sides r0 .. r0 + nrhs - 1 of the sweep that just ran (the share of ONE destination rank) as
// [root][rhs][packed block]; unpack the roots of EVERY rank -- this one's too -- from the all-to-all's receive buffer (`width`
// doubles per source rank) into the slots 0 .. nrhs - 1, where the top sweep of this rank's own share reads them.
int csp_exchange_pack_range(csp_ctx* c, int64_t r0, int64_t nrhs, double* buf, void* stream) { return exchange_roots(c, nrhs, buf, 0, 0, stream, r0); }
int csp_exchange_unpack_all(csp_ctx* c, int64_t nrhs, const double* buf, int64_t width, void* stream) {
  return exchange_roots(c, nrhs, const_cast<double*>(buf), width, 2, stream);
}
// rows [a, b) of the swept stack of the constraints j0 .. j1 - 1 <-> buf[(j - j0) * (b - a) + (row - a)]   (dir 0: stack -> buf,
// 1: buf -> stack): the top's panels of a rank's constraint share travel to the rank that accumulates the top's Gram block
__global__ void k_stack_rows(double* ustack, int64_t bl, int64_t j0, int64_t a, int64_t len, double* buf, int dir) {
  double* row = ustack + (j0 + blockIdx.y) * bl + a;
  double* b = buf + (int64_t)blockIdx.y * len;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += (int64_t)gridDim.x * blockDim.x) {
    if (dir) row[e] = b[e]; else b[e] = row[e];
  }
}
int kkt_stack_rows(csp_ctx* c, int dir, int64_t j0, int64_t j1, int64_t a, int64_t b, double* buf, void* stream) {
  if (int rc = ready(c)) return rc;
  DeviceCtx& D = c->D;
  if (!D.ustack || j0 < 0 || j1 > D.m || j1 < j0 || a < 0 || b > c->S.blklen() || b < a || !buf || dir < 0 || dir > 1) return SMCP_EINVAL;
  if (j1 == j0 || b == a) return 0;
  launch(c, KID_axpby, k_stack_rows, dim3((unsigned)std::min<int64_t>(256, (b - a + 255) / 256), (unsigned)(j1 - j0)), dim3(256), (hipStream_t)stream,
         D.ustack, c->S.blklen(), j0, a, b - a, buf, dir);
  HIPCHK(end_call(c));
  return 0;
}
int csp_exchange_unpack(csp_ctx* c, int64_t nrhs, const double* buf, int64_t width, void* stream) {
  return exchange_roots(c, nrhs, const_cast<double*>(buf), width, 1, stream);
}

}  // extern "C"
