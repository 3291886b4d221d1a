// Host driver of the chordal-plus-low-rank factor (front_lowrank.hip): M = L L^T + V diag(a) V^T = F F^T with
// F = L (I + W C W^T), W = L^-1 V.  Included by capi.hip.  W and the state block belong to the caller; the only buffer of
// the context is the workspace of the partial Gram products.  Every application of F, F^T, their inverses, M^-1 or M is
// the existing csp_trsm / csp_trmm launches around exactly two launches of the kernels here: k_lr_gram (the partials of
// Z = W^T B) and k_lr_apply (B += W (T Z)); csp_lowrank_factor is one csp_trsm, k_lr_gram (K = W^T W) and k_lr_small.

namespace {

constexpr int64_t LR_CHUNK = 512;      // columns of B per pass (the partials of one pass: at most 128 slabs x 64 x 512 doubles)

// tile products from eight columns on both sides (the gate of csp_trmm / csp_trsm); FMA on the generic / deterministic route
bool lr_tiles(csp_ctx* c, int64_t k, int64_t kb) {
  static const int mm = sw_int("SMCP_LOWRANK_MM", 1);     // read once per process
  return mm && !use_generic(c) && use_large() && k >= 8 && kb >= 8;
}

// the partials of Z = W^T B into the workspace of the context; returns the number of slabs through *nslab
int lr_gram(csp_ctx* c, const double* W, int64_t ldw, int64_t k, const double* B, int64_t ldb, int64_t kb, int* nslab, hipStream_t st) {
  DeviceCtx& D = c->D;
  const int64_t n = c->S.n;
  LrGramArgs a;
  a.W = W; a.ldw = ldw; a.k = (int)k; a.B = B; a.ldb = ldb; a.kb = (int)kb; a.n = n; a.slab = lr_slab_rows(n);
  const int64_t ns = (n + a.slab - 1) / a.slab;
  if (int rc = dev_grow(&D.lr_ws, &D.lr_ws_len, ns * k * kb, D.mem, st)) return rc;
  a.P = D.lr_ws;
  *nslab = (int)ns;
  if (!lr_tiles(c, k, kb))
    launch(c, KID_lr_gram, k_lr_gram<false, 1>, dim3((unsigned)ns, (unsigned)((k + LR_JB - 1) / LR_JB), (unsigned)((kb + LR_CB - 1) / LR_CB)), dim3(256), st, a);
  else if (kb <= 16)
    launch(c, KID_lr_gram, k_lr_gram<true, 1>, dim3((unsigned)ns, (unsigned)((k + 15) / 16), 1), dim3(256), st, a);
  else
    launch(c, KID_lr_gram, k_lr_gram<true, 4>, dim3((unsigned)ns, (unsigned)((k + 15) / 16), (unsigned)((kb + 63) / 64)), dim3(256), st, a);
  return 0;
}

// B <- B + W T (W^T B): the two launches
int lr_middle(csp_ctx* c, const double* W, int64_t ldw, int64_t k, const double* state, double* B, int64_t ldb, int64_t kb, int mode,
              hipStream_t st) {
  int nslab = 0;
  if (int rc = lr_gram(c, W, ldw, k, B, ldb, kb, &nslab, st)) return rc;
  LrApplyArgs a;
  a.W = W; a.ldw = ldw; a.k = (int)k; a.B = B; a.ldb = ldb; a.kb = (int)kb; a.n = c->S.n;
  a.P = c->D.lr_ws; a.nslab = nslab; a.state = state; a.mode = mode;
  launch(c, KID_lr_apply, k_lr_apply, dim3((unsigned)((a.n + LR_AROWS - 1) / LR_AROWS), (unsigned)((kb + LR_ACB - 1) / LR_ACB)), dim3(256), st, a);
  return 0;
}

int lr_check(csp_ctx* c, int64_t k, int64_t ld) {
  if (int rc = ready(c)) return rc;
  // (a partitioned context holds valid factors on its own cliques only)
  if (k < 1 || k > LR_KMAX || ld < c->S.n || c->xr_world > 1) return SMCP_EINVAL;
  return 0;
}

}  // namespace

extern "C" {

int64_t csp_lowrank_state_len(int64_t k) { return (k < 1 || k > LR_KMAX) ? SMCP_EINVAL : lr_state_len(k); }

int csp_lowrank_factor(csp_ctx* c, const double* L, double* W, int64_t ldw, int64_t k, const double* a_host, double* state, void* stream) {
  if (int rc = lr_check(c, k, ldw)) return rc;
  if (!L || !W || !state) return SMCP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  static bool attr = false;
  if (!attr) attr = hipFuncSetAttribute((const void*)k_lr_small, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lr_small_lds(LR_KMAX)) == hipSuccess;
  if (!attr) return SMCP_EHIP;
  if (int rc = trsm_impl(c, L, nullptr, W, k, ldw, 0, st, true)) return rc;
  int nslab = 0;
  if (int rc = lr_gram(c, W, ldw, k, W, ldw, k, &nslab, st)) return rc;
  LrCoef coef;
  for (int64_t j = 0; j < LR_KMAX; ++j) coef.a[j] = j < k ? (a_host ? a_host[j] : 1.0) : 0.0;
  launch_lds(c, KID_lr_small, k_lr_small, dim3(1), dim3(256), lr_small_lds((int)k), st, (const double*)c->D.lr_ws, nslab, (int)k, coef, state);
  HIPCHK(end_call(c));
  double* h = (double*)(c->D.info_host + 24);          // the pinned scalar of the reductions
  HIPCHK(hipMemcpyAsync(h, state, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return (int)*h;
}

int csp_lowrank_apply(csp_ctx* c, const double* L, const double* W, int64_t ldw, int64_t k, const double* state, double* B, int64_t ldb,
                      int64_t nrhs, int op, void* stream) {
  if (int rc = lr_check(c, k, ldw)) return rc;
  if (!L || !W || !state || !B || nrhs < 1 || ldb < c->S.n || op < 0 || op > CSP_LR_M) return SMCP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  for (int64_t c0 = 0; c0 < nrhs; c0 += LR_CHUNK) {
    double* Bc = B + c0 * ldb;
    const int64_t nc = std::min(LR_CHUNK, nrhs - c0);
    int before = -1, mode = 0, after = -1;           // csp_trsm (0 / 1) or csp_trmm (2 / 3) with trans = code & 1, or nothing
    switch (op) {
      case CSP_LR_F: mode = LR_T_C; after = 2; break;                      // L (I + W C W^T)
      case CSP_LR_FT: before = 3; mode = LR_T_CT; break;                   // (I + W C^T W^T) L^T
      case CSP_LR_FINV: before = 0; mode = LR_T_D; break;                  // (I + W D W^T) L^-1
      case CSP_LR_FINVT: mode = LR_T_DT; after = 1; break;                 // L^-T (I + W D^T W^T)
      case CSP_LR_MINV: before = 0; mode = LR_T_S; after = 1; break;       // L^-T (I + W S W^T) L^-1
      default: before = 3; mode = LR_T_A; after = 2; break;                // L (I + W A W^T) L^T
    }
    auto tri = [&](int code) -> int {
      if (code < 0) return 0;
      return code < 2 ? trsm_impl(c, L, nullptr, Bc, nc, ldb, code & 1, st, true) : csp_trmm(c, L, Bc, nc, ldb, 1.0, code & 1, stream);
    };
    if (int rc = tri(before)) return rc;
    if (int rc = lr_middle(c, W, ldw, k, state, Bc, ldb, nc, mode, st)) return rc;
    HIPCHK(end_call(c));
    if (int rc = tri(after)) return rc;
  }
  return 0;
}

int csp_lowrank_logdet(csp_ctx* c, const double* L, const double* state, double* out, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!L || !state || !out || c->xr_world > 1) return SMCP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  double lds = 0.0;
  if (int rc = reduce_impl(c, L, nullptr, 1, &lds, st)) return rc;
  double* h = (double*)(c->D.info_host + 24);
  HIPCHK(hipMemcpyAsync(h, state + 1, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  *out = 2.0 * lds + *h;
  return 0;
}

}  // extern "C"
