// Host driver of the Lanczos iteration on the dual cone (front_lanczos.hip).  Included by capi.hip.
// The workspace, the basis and the state block in it belong to the caller; the context lends only what csp_trsm and
// csp_symm use anyway.  A step is: the copy of v_j, the operator (csp_trsm / csp_symm / csp_trsm on one column, or csp_trsm
// twice), dots, update, dots, update, finish, scale -- every one queued on the caller's stream, nothing read back.

namespace {

struct LzPlan {
  int64_t n, ld, slab;
  int nslab;
  double *state, *P1, *P2, *PN, *V, *A, *B;
};

LzPlan lz_plan(csp_ctx* c, double* work, int64_t jmax) {
  LzPlan p;
  p.n = c->S.n; p.ld = lz_ld(p.n); p.slab = lr_slab_rows(p.n);
  p.nslab = (int)((p.n + p.slab - 1) / p.slab);
  p.state = work;
  p.P1 = work + lz_off_p(jmax, 0); p.P2 = work + lz_off_p(jmax, 1); p.PN = work + lz_off_pn(jmax);
  p.V = work + lz_off_basis(p.n, jmax);
  p.A = work + lz_off_scratch(p.n, jmax); p.B = p.A + p.ld;
  return p;
}

void lz_dots(csp_ctx* c, const LzPlan& p, const double* w, int nrow, int64_t jmax, double* P, hipStream_t st) {
  LzDotsArgs a;
  a.V = p.V; a.ld = p.ld; a.w = w; a.nrow = nrow; a.jmax = (int)jmax; a.n = p.n; a.slab = p.slab; a.P = P;
  launch(c, KID_vec_axpby, k_lz_dots, dim3((unsigned)p.nslab, (unsigned)((nrow + LZ_RB - 1) / LZ_RB)), dim3(256), st, a);
}

void lz_update(csp_ctx* c, const LzPlan& p, double* w, int nrow, int64_t jmax, const double* P, double* PN, hipStream_t st) {
  LzUpdateArgs a;
  a.V = p.V; a.ld = p.ld; a.w = w; a.nrow = nrow; a.jmax = (int)jmax; a.nslab = p.nslab; a.n = p.n; a.P = P; a.PN = PN;
  launch(c, KID_vec_axpby, k_lz_update, dim3((unsigned)lz_nnorm(p.n)), dim3(256), st, a);
}

void lz_finish(csp_ctx* c, const LzPlan& p, int j, int64_t jmax, hipStream_t st) {
  LzFinishArgs a;
  a.state = p.state; a.P1 = p.P1; a.P2 = p.P2; a.PN = p.PN; a.j = j; a.jmax = (int)jmax; a.nslab = p.nslab; a.nnorm = lz_nnorm(p.n);
  // below n eps |T| a norm cannot be told from the rounding of the operator itself: the Krylov space counts as invariant
  a.brk = 2.220446049250313e-16 * (double)p.n;
  launch(c, KID_vec_axpby, k_lz_finish, dim3(1), dim3(256), st, a);
}

int lz_check(csp_ctx* c, const double* work, int64_t jmax) {
  if (int rc = ready(c)) return rc;
  // (a partitioned context holds valid factors on its own cliques only; a replicated one has no single L)
  if (!work || jmax < 1 || jmax > LZ_JMAX || c->xr_world > 1 || c->ntrial != 1) return SMCP_EINVAL;
  return 0;
}

}  // namespace

extern "C" {

int64_t csp_lanczos_work_len(int64_t n, int64_t jmax) { return (n < 1 || jmax < 1 || jmax > LZ_JMAX) ? SMCP_EINVAL : lz_work_len(n, jmax); }

int csp_lanczos_steps(csp_ctx* c, const double* L, const double* Dm, double* work, int64_t jmax, int64_t j0, int64_t nsteps, void* stream) {
  if (int rc = lz_check(c, work, jmax)) return rc;
  if (!L || j0 < 0 || nsteps < 1 || j0 + nsteps > jmax) return SMCP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const LzPlan p = lz_plan(c, work, jmax);
  const dim3 rows((unsigned)lz_nnorm(p.n));
  if (j0 == 0) {                                   // v_0 <- v_0 / |v_0|; the state block starts afresh
    lz_dots(c, p, p.V, 1, jmax, p.P1, st);
    lz_finish(c, p, -1, jmax, st);
    launch(c, KID_vec_axpby, k_lz_scale, rows, dim3(256), st, (const double*)p.state, (const double*)p.V, p.V, p.n);
  }
  for (int64_t j = j0; j < j0 + nsteps; ++j) {
    double* w = p.A;
    launch(c, KID_vec_axpby, k_lz_copy, rows, dim3(256), st, (const double*)(p.V + j * p.ld), p.A, p.n);
    if (Dm) {                                      // w = L^-1 D L^-T v_j
      if (int rc = trsm_impl(c, L, nullptr, p.A, 1, p.ld, 1, st, true)) return rc;
      if (int rc = csp_symm(c, Dm, p.A, p.ld, p.B, p.ld, 1, 1.0, 0.0, stream)) return rc;
      if (int rc = trsm_impl(c, L, nullptr, p.B, 1, p.ld, 0, st, true)) return rc;
      w = p.B;
    } else {                                       // w = L^-T L^-1 v_j
      if (int rc = trsm_impl(c, L, nullptr, p.A, 1, p.ld, 0, st, true)) return rc;
      if (int rc = trsm_impl(c, L, nullptr, p.A, 1, p.ld, 1, st, true)) return rc;
    }
    const int nrow = (int)j + 1;
    lz_dots(c, p, w, nrow, jmax, p.P1, st);
    lz_update(c, p, w, nrow, jmax, p.P1, nullptr, st);
    lz_dots(c, p, w, nrow, jmax, p.P2, st);
    lz_update(c, p, w, nrow, jmax, p.P2, p.PN, st);
    lz_finish(c, p, (int)j, jmax, st);
    launch(c, KID_vec_axpby, k_lz_scale, rows, dim3(256), st, (const double*)p.state, (const double*)w, p.V + (j + 1) * p.ld, p.n);
  }
  HIPCHK(end_call(c));
  return 0;
}

int csp_lanczos_ritz(csp_ctx* c, double* work, int64_t jmax, void* stream) {
  if (int rc = lz_check(c, work, jmax)) return rc;
  launch(c, KID_qr_small, k_lz_ritz, dim3(1), dim3(256), (hipStream_t)stream, work, (int)jmax);
  HIPCHK(end_call(c));
  return 0;
}

}  // extern "C"
