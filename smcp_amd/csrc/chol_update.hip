// Host driver of the rank-k update / downdate of the supernodal factor (front_update.hip).  Included by capi.hip.
// csp_chol_update is two launches whatever the tree and whatever k: k_cu_plan (under KID_lr_apply: a workgroup per column
// streams it once) and k_cu_walk (under KID_lr_small: one workgroup).  The walk reads the flags of k_cu_plan on the device
// and returns at once when a column was refused, so the host waits once, for the two status words.  The workspace (flags,
// visit bytes, then the k x n image of V that becomes w) belongs to the context.  The two ids are borrowed: the profile hooks
// time the launches as k_lr_apply and k_lr_small; the launch census (csp_census_*) and SMCP_TRACE=1 name k_cu_plan and k_cu_walk.

namespace {

int cu_host_check(const csp_ctx* c, int64_t cnt, const int64_t* idx) {
  const Symbolic& S = c->S;
  int64_t lo = S.n;
  for (int64_t q = 0; q < cnt; ++q) {
    if (idx[q] < 0 || idx[q] >= S.n) return -1;
    lo = std::min(lo, idx[q]);
  }
  if (cnt < 1) return -1;
  const int64_t s = S.snode[lo];
  const int32_t* r0 = S.rowidx.data() + S.rowptr[s];
  const int32_t* r1 = S.rowidx.data() + S.rowptr[s + 1];
  for (int64_t q = 0; q < cnt; ++q)
    if (!std::binary_search(r0, r1, (int32_t)idx[q])) return -1;
  return (int)s;
}

}  // namespace

extern "C" {

int64_t csp_clique_support(const csp_ctx* c, int64_t cnt, const int64_t* idx) {
  if (!c || cnt < 1 || !idx || c->ntrial != 1) return -1;
  return cu_host_check(c, cnt, idx);
}

int csp_chol_update_info(const csp_ctx* c, int64_t* column) {
  if (!c || !column) return SMCP_EINVAL;
  *column = c->cu_column;
  return 0;
}

int csp_chol_update(csp_ctx* c, double* L, const double* V, int64_t ldv, int64_t k, const double* a_host, void* stream) {
  if (int rc = ready(c)) return rc;
  // (a partitioned context holds valid factors on its own cliques only; the copies of a replicated one are separate matrices)
  if (!L || !V || k < 1 || k > CU_KMAX || ldv < c->S.n || c->xr_world > 1 || c->ntrial != 1) return SMCP_EINVAL;
  c->cu_column = -1;
  CuCols cols;
  int m = 0;
  for (int sgn = 1; sgn >= -1; sgn -= 2)
    for (int64_t j = 0; j < k; ++j) {
      const double aj = a_host ? a_host[j] : 1.0;
      if (!(std::fabs(aj) <= DBL_MAX)) { c->cu_column = j; return SMCP_EVALUE; }
      if (sgn * aj > 0.0) { cols.col[m] = (signed char)j; cols.sign[m] = (signed char)sgn; cols.slot[j] = (signed char)m; ++m; }
    }
  for (int64_t j = 0; j < CU_KMAX; ++j) {
    const double aj = j < k ? (a_host ? a_host[j] : 1.0) : 0.0;
    cols.scale[j] = std::sqrt(std::fabs(aj));
    if (aj == 0.0) cols.slot[j] = -1;
  }
  for (int q = m; q < CU_KMAX; ++q) { cols.col[q] = 0; cols.sign[q] = 1; }
  cols.nact = m;
  hipStream_t st = (hipStream_t)stream;
  DeviceCtx& D = c->D;
  const int64_t n = c->S.n, nsn = c->S.nsn;
  const int64_t hdr = CU_HDR + cu_visit_doubles(nsn);
  if (D.cu_ws_len < cu_ws_len(nsn, n, k)) {
    if (int rc = dev_grow(&D.cu_ws, &D.cu_ws_len, cu_ws_len(nsn, n, k), D.mem, st)) return rc;
    HIPCHK(hipMemsetAsync(D.cu_ws, 0, hdr * sizeof(double), st));       // the walk leaves the visit bytes clear; a new buffer starts so
  }
  int* flags = (int*)D.cu_ws;
  unsigned* visit = (unsigned*)(D.cu_ws + CU_HDR);
  double* W = D.cu_ws + hdr;
  invalidate_tags(c, L);
  launch(c, KID_lr_apply, k_cu_plan, dim3((unsigned)k), dim3(256), st, (const CliqueDesc*)D.cl, (const int32_t*)D.rowidx, (int)nsn, (int)n, V, ldv,
         cols, W, n, visit, flags);
  CuWalkArgs a;
  a.cl = D.cl; a.rowidx = D.rowidx; a.nsn = (int)nsn; a.L = L; a.W = W; a.ldw = n; a.visit = visit; a.flags = flags;
  a.status = flags + CU_KMAX; a.k = (int)k; a.e_support = SMCP_ESUPPORT; a.e_value = SMCP_EVALUE;
  launch(c, KID_lr_small, k_cu_walk, dim3(1), dim3(CU_NT), st, a, cols);
  HIPCHK(end_call(c));
  int* h = D.info_host + 26;                           // (24, 25: the pinned scalar of the reductions)
  HIPCHK(hipMemcpyAsync(h, a.status, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (h[0]) c->cu_column = h[1];
  return h[0];
}

}  // extern "C"
