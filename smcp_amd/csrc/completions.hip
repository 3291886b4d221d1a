// Host drivers of the completions: minimum-rank (front_mrc.hip, with the cut rounding of csp_maxcut_cuts), Euclidean
// distance matrix (front_edm.hip, with csp_edm_dense) and dense maximum-determinant PSD (front_psd.hip), and of the
// spectra of the clique blocks (front_ceig.hip), which run in the same slots.  Included by capi.hip.  All three share the launches, slots and per-clique buffers of D.mrc (CompletionWs, context.hpp): a rank pass
// over all cliques at once, then either a factor pass, one launch group per level from the root down (mrc, edm), or the
// solves and fills of the dense completion (psd).

namespace {

constexpr int64_t MRC_LDS = 128 * 1024;     // bytes of dynamic LDS a slot may take (the rest: the reduction buffers, one
                                            // pair per instantiation of mrc_argmax)
constexpr int64_t MRC_HBM_DOUBLES = (int64_t)1 << 25;  // HBM slots of one launch: 256 MiB at most (always at least one slot)
// the same under this context's CSP_TUNE_SLOT_DOUBLES (0: the default above)
int64_t hbm_doubles(const csp_ctx* c) { return c->slot_doubles > 0 ? c->slot_doubles : MRC_HBM_DOUBLES; }

int mrc_setup(csp_ctx* c) {
  DeviceCtx& D = c->D;
  if (D.mrc.ints) return 0;
  if (int rc = dev_alloc(&D.mrc.ints, 2 * c->S.nsn + 4, D.mem)) return rc;
  if (int rc = dev_alloc(&D.mrc.xdiag, c->S.n, D.mem)) return rc;
  return dev_alloc(&D.mrc.list, c->S.nsn, D.mem);
}

// bytes of dynamic LDS a launch of Kern may ask for: MRC_LDS once the device has granted it to this kernel (asked on
// its first launch), the default limit otherwise
template <auto Kern>
int64_t lds_ceiling() {
  static const bool granted = hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MRC_LDS) == hipSuccess;
  return granted ? MRC_LDS : 65536;
}

// Runs Kern over the cliques list[b, e) (host copy; the device copy is D.mrc.list), which ascend in slot size need[]
// (doubles): those whose slot fits in LDS one workgroup each, in launches by size class, the rest over HBM slots.
// list: another device list than D.mrc.list (one that outlives the call)
template <auto Kern>
int mrc_launch(csp_ctx* c, int kid, MrcArgs a, const std::vector<int64_t>& need, int64_t b, int64_t e, hipStream_t st,
               const int32_t* list = nullptr) {
  DeviceCtx& D = c->D;
  if (!list) list = D.mrc.list;
  const int64_t lds_max = lds_ceiling<Kern>();
  int64_t q = b;
  for (int64_t cap : {(int64_t)8192, (int64_t)16384, (int64_t)32768, (int64_t)65536, MRC_LDS}) {
    int64_t q2 = q;
    while (q2 < e && need[q2] * (int64_t)sizeof(double) <= std::min(cap, lds_max)) ++q2;
    if (q2 > q) {
      a.lev = list + q;
      a.cnt = (int)(q2 - q);
      a.ws = nullptr;
      launch_lds(c, kid, Kern, dim3((unsigned)(q2 - q)), dim3(MRC_NT), (size_t)need[q2 - 1] * sizeof(double), st, a);
    }
    q = q2;
  }
  if (q < e) {
    const int64_t slot = (need[e - 1] + 31) / 32 * 32;
    const int64_t G = std::min<int64_t>(std::min<int64_t>(e - q, 4 * D.ncu), std::max<int64_t>(1, hbm_doubles(c) / slot));
    c->slot_share = std::max<int64_t>(c->slot_share, (e - q + G - 1) / G);      // CSP_Q_SLOT_SHARE
    if (int rc = dev_grow(&D.mrc.ws, &D.mrc.cap, G * slot, D.mem, st)) return rc;
    a.lev = list + q;
    a.cnt = (int)(e - q);
    a.ws = D.mrc.ws;
    a.slot = slot;
    launch(c, kid, Kern, dim3((unsigned)G), dim3(MRC_NT), st, a);
  }
  return 0;
}

// The cliques of every launch group of a pass, uploaded to D.mrc.list: group l is launches[l] (a range of clique numbers)
// without the cliques whose slot(k) is negative, in ascending slot size (doubles; ties keep their order), and occupies
// ranges[l] .. ranges[l + 1] of the list and of need[]
using CliqueRange = std::pair<const int64_t*, const int64_t*>;
template <class Slot>
int slot_sorted_lists(csp_ctx* c, const std::vector<CliqueRange>& launches, Slot slot, std::vector<int64_t>& need,
                      std::vector<int64_t>& ranges, hipStream_t st) {
  std::vector<int32_t> list;
  std::vector<std::pair<int64_t, int32_t>> tmp;
  need.clear();
  ranges.assign(1, 0);
  for (const CliqueRange& L : launches) {
    tmp.clear();
    for (const int64_t* k = L.first; k != L.second; ++k)
      if (slot(*k) >= 0) tmp.push_back({slot(*k), (int32_t)*k});
    std::stable_sort(tmp.begin(), tmp.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    for (auto& t : tmp) { need.push_back(t.first); list.push_back(t.second); }
    ranges.push_back((int64_t)list.size());
  }
  if (!list.empty()) HIPCHK(hipMemcpyAsync(c->D.mrc.list, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));      // (list is a host temporary)
  return 0;
}
// pass 1: one launch group over all cliques
std::vector<CliqueRange> all_cliques(const Symbolic& S) { return {{S.levidx.data(), S.levidx.data() + S.nsn}}; }
// pass 2: one launch group per level, root first
std::vector<CliqueRange> levels_root_first(const Symbolic& S) {
  std::vector<CliqueRange> v;
  for (int64_t l = S.nlev - 1; l >= 0; --l) v.push_back({S.levidx.data() + S.levptr[l], S.levidx.data() + S.levptr[l + 1]});
  return v;
}

MrcArgs mrc_args(csp_ctx* c, const double* x, double tol) {
  MrcArgs a{};
  a.cl = c->D.cl;
  a.rowidx = c->D.rowidx;
  a.x = x;
  a.upd = c->D.upd;
  a.xdiag = c->D.mrc.xdiag;
  a.tol = tol;
  a.rank = c->D.mrc.ints;
  a.flag = c->D.mrc.ints + c->S.nsn;
  return a;
}

// a reduce kernel (k_mrc_reduce, k_edm_reduce) over the per-clique ranks and flags, and the read-back of its three integers
template <class K>
int reduce_flags(csp_ctx* c, int kid, K kern, hipStream_t st, int32_t* out) {
  int32_t* ints = c->D.mrc.ints;
  int32_t* dout = ints + 2 * c->S.nsn;
  launch(c, kid, kern, dim3(1), dim3(MRC_NT), st, (const int32_t*)ints, (const int32_t*)(ints + c->S.nsn), (int)c->S.nsn, dout);
  HIPCHK(end_call(c));
  HIPCHK(hipMemcpyAsync(out, dout, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// Pass 1 of a completion: Rank over every clique block in one launch group (their separator blocks gathered first), then
// Reduce.  *r = the largest rank; a clique that fails the test of Rank returns its status.  with_diag: k_mrc_diag leaves
// diag(X) for the thresholds (mrc, psd); out2_is_error: the third integer of Reduce flags invalid input (edm: a nonzero
// diagonal entry).
template <auto Rank, class R>
int rank_pass(csp_ctx* c, const double* x, double tol, int kid_rank, int kid_reduce, R reduce, bool with_diag, bool out2_is_error,
              int64_t* r, hipStream_t st) {
  c->slot_share = 0;
  if (int rc = mrc_setup(c)) return rc;
  std::vector<int64_t> need, ranges;
  if (int rc = slot_sorted_lists(c, all_cliques(c->S), [&](int64_t k) { return mrc_slot1(c->S.nf(k)); }, need, ranges, st)) return rc;
  if (with_diag) launch(c, KID_mrc_diag, k_mrc_diag, dim3((unsigned)c->S.nsn), dim3(MRC_NT), st, (const CliqueDesc*)c->D.cl, x, c->D.mrc.xdiag);
  gather_all(c, x, 0, 1, c->D.upd, st);          // X_AA of every clique
  if (int rc = mrc_launch<Rank>(c, kid_rank, mrc_args(c, x, tol), need, 0, c->S.nsn, st)) return rc;
  int32_t out[3];
  if (int rc = reduce_flags(c, kid_reduce, reduce, st, out)) return rc;
  if (out2_is_error && out[2]) return SMCP_EINVAL;
  if (out[1]) return out[1];
  if (r) *r = out[0];
  return 0;
}

// Pass 2 of a completion: Factor over the levels, root first, writing the r rows of Y; *clamped = the cliques whose Schur
// factor lost columns to the r-column cap.  slot2(nn, na, r): the slot of a clique in doubles.
template <auto Factor, class Slot2>
int factor_pass(csp_ctx* c, const double* x, double tol, int64_t r, double* Y, int64_t ldY, int kid, Slot2 slot2, bool with_diag,
                int64_t* clamped, hipStream_t st) {
  const Symbolic& S = c->S;
  c->slot_share = 0;
  if (int rc = mrc_setup(c)) return rc;
  std::vector<int64_t> need, ranges;
  if (int rc = slot_sorted_lists(c, levels_root_first(S), [&](int64_t k) { return slot2(S.nn(k), S.na(k), r); }, need, ranges, st)) return rc;
  if (with_diag) launch(c, KID_mrc_diag, k_mrc_diag, dim3((unsigned)S.nsn), dim3(MRC_NT), st, (const CliqueDesc*)c->D.cl, x, c->D.mrc.xdiag);
  MrcArgs a = mrc_args(c, x, tol);
  a.Y = Y;
  a.ldY = ldY;
  a.r = (int)r;
  for (size_t l = 0; l + 1 < ranges.size(); ++l)
    if (int rc = mrc_launch<Factor>(c, kid, a, need, ranges[l], ranges[l + 1], st)) return rc;
  // the clamped count is the third integer of k_mrc_reduce for both completions (k_edm_reduce counts nonzero diagonal
  // entries there); its ranks are unused here
  HIPCHK(hipMemsetAsync(c->D.mrc.ints, 0, S.nsn * sizeof(int32_t), st));
  int32_t out[3];
  if (int rc = reduce_flags(c, KID_mrc_reduce, k_mrc_reduce, st, out)) return rc;
  *clamped = out[2];
  return 0;
}

// what csp_mrcompletion and csp_edmcompletion refuse
int factor_args_check(csp_ctx* c, const double* x, double tol, int64_t r, const double* Y, int64_t ldY) {
  if (int rc = ready(c)) return rc;
  if (!x || !(tol >= 0.0) || r < 0 || r > c->S.max_front || (r > 0 && (!Y || ldY < r)) || c->ntrial != 1) return SMCP_EINVAL;
  return 0;
}

// ---- dense maximum-determinant PSD completion (front_psd.hip) -------------------------------------------------------
// ulist (the columns in the order the levels complete them, root level first, cliques ascending inside a level), the tile
// tasks of the two fill launches of every level and the W workspace: built on the first call
int psd_setup(csp_ctx* c) {
  DeviceCtx& D = c->D;
  PsdPlan& P = D.psd;
  if (P.ulist) return 0;
  const Symbolic& S = c->S;
  std::vector<int32_t> ulist;
  std::vector<PsdTask> tasks;
  std::vector<int64_t> end_of(S.nsn, 0);
  c->psd_lev.clear();
  const int64_t max_tasks = (int64_t)1 << 26;
  for (int64_t l = S.nlev - 1; l >= 0; --l) {
    std::vector<int64_t> ks(S.levidx.begin() + S.levptr[l], S.levidx.begin() + S.levptr[l + 1]);
    std::sort(ks.begin(), ks.end());
    const int64_t before = (int64_t)ulist.size();
    for (int64_t k : ks) {
      for (int64_t j = S.snptr[k]; j < S.snptr[k + 1]; ++j) ulist.push_back((int32_t)j);
      end_of[k] = (int64_t)ulist.size();
    }
    const int64_t after = (int64_t)ulist.size();
    csp_ctx::PsdLevel L;
    auto add = [&](int64_t k, int64_t b, int64_t e) {
      for (int64_t off = b; off < e; off += LT)
        for (int64_t n0 = 0; n0 < S.nn(k); n0 += LT)
          tasks.push_back({(int32_t)k, (int32_t)off, (int32_t)std::min<int64_t>(LT, e - off), (int32_t)n0});
    };
    L.b1 = (int64_t)tasks.size();
    for (int64_t k : ks) if (S.na(k) > 0) add(k, 0, before);                 // step 1: the rows of the levels done
    L.b2 = (int64_t)tasks.size();
    for (int64_t k : ks) if (S.na(k) > 0) add(k, end_of[k], after);          // step 2: the later cliques of the level
    L.e2 = (int64_t)tasks.size();
    if (L.e2 > max_tasks) return SMCP_ENOMEM;
    if (L.e2 > L.b1) c->psd_lev.push_back(L);
  }
  if (int rc = dev_upload(&P.tasks, tasks, D.mem)) return rc;
  if (int rc = dev_alloc(&P.w, S.blklen(), D.mem)) return rc;
  if (int rc = dev_alloc(&P.idx, S.sepptr[S.nsn], D.mem)) return rc;
  if (int rc = dev_alloc(&P.ra, S.nsn, D.mem)) return rc;
  return dev_upload(&P.ulist, ulist, D.mem);      // last: ulist marks the plan as built
}

// ---- packed clique blocks (front_ceig.hip) --------------------------------------------------------------------------
// block k (nf x nf, column-major, rows and columns in the order of the clique's rowidx) lies at [q[k], q[k + 1])
std::vector<int64_t> clique_ptr_of(const Symbolic& S) {
  std::vector<int64_t> q(S.nsn + 1, 0);
  for (int64_t k = 0; k < S.nsn; ++k) q[k + 1] = q[k] + S.nf(k) * S.nf(k);
  return q;
}
// the device copy of these offsets, made by the first call that needs it
int qptr_setup(csp_ctx* c) {
  if (c->D.mrc.qptr) return 0;
  const std::vector<int64_t> q = clique_ptr_of(c->S);
  c->qlen = q.back();
  return dev_upload(&c->D.mrc.qptr, q, c->D.mem);
}

// some output range overlaps an input range or another output range (a null range overlaps nothing)
using DRange = std::pair<const double*, int64_t>;
bool ranges_overlap(std::initializer_list<DRange> outs, std::initializer_list<DRange> ins) {
  auto overlap = [](const DRange& p, const DRange& q) { return p.first && q.first && p.first < q.first + q.second && q.first < p.first + p.second; };
  for (const DRange* o = outs.begin(); o != outs.end(); ++o) {
    for (const DRange& i : ins) if (overlap(*o, i)) return true;
    for (const DRange* o2 = o + 1; o2 != outs.end(); ++o2) if (overlap(*o, *o2)) return true;
  }
  return false;
}

// ---- wide cliques on the whole chip (front_ceigw.hip) ---------------------------------------------------------------
// the clique takes the block Jacobi under this context's CSP_TUNE_CEIG_WIDE
bool ceig_is_wide(const csp_ctx* c, int64_t k) { return c->ceig_wide > 0 && c->S.nf(k) >= c->ceig_wide; }

// One launch group of wide cliques: form, then block sweeps until no clique of the group runs (one integer read back per
// sweep), then the rank sort and the output blocks.  m.rank / m.flag of these cliques are filled as k_ceig fills them.
// Pencil mode (a.pencil): behind the form the reduction to standard form, 3 ntmax + 1 launches for the most 64-row tiles
// ntmax of a clique of the group (front_ceigw.hip), whatever the data.
int ceigw_group(csp_ctx* c, CeigwArgs a, const std::vector<CeigwDesc>& desc, int64_t doubles, hipStream_t st) {
  DeviceCtx& D = c->D;
  if (lds_ceiling<k_ceigw_pivot>() < (int64_t)CW_PIVOT_LDS + 4096 || lds_ceiling<k_ceigw_apply>() < (int64_t)CW_APPLY_LDS + 4096) return SMCP_EHIP;
  if (a.pencil && (lds_ceiling<k_ceigw_panel>() < (int64_t)CW_APPLY_LDS + 4096 || lds_ceiling<k_ceigw_trail>() < (int64_t)CW_APPLY_LDS + 4096 ||
                   lds_ceiling<k_ceigw_solve<true>>() < (int64_t)CW_APPLY_LDS + 4096 || lds_ceiling<k_ceigw_solve<false>>() < (int64_t)CW_APPLY_LDS + 4096))
    return SMCP_EHIP;
  const int nw = (int)desc.size();
  if (int rc = dev_grow(&D.mrc.wws, &D.mrc.wcap, doubles, D.mem, st)) return rc;
  if (int rc = dev_grow(&D.mrc.wdesc, &D.mrc.wdesc_cap, (int64_t)nw, D.mem, st)) return rc;
  HIPCHK(hipMemcpyAsync(D.mrc.wdesc, desc.data(), nw * sizeof(CeigwDesc), hipMemcpyHostToDevice, st));
  a.wd = D.mrc.wdesc;
  a.ws = D.mrc.wws;
  a.nw = nw;
  a.nrun = D.mrc.ints + 2 * c->S.nsn + 3;
  int hmax = 0, nbmax = 0;
  int64_t nfmax = 0;
  for (const CeigwDesc& w : desc) { hmax = std::max(hmax, (int)w.h); nbmax = std::max(nbmax, (int)w.nb); nfmax = std::max<int64_t>(nfmax, w.nf); }
  const int steps = nbmax + (nbmax & 1) - 1;
  const unsigned parts = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, nfmax * nfmax / (MRC_NT * 32)));
  const unsigned tiles = (unsigned)(hmax * (hmax + 1) / 2 + (a.vec ? (int)((nfmax + CW_T - 1) / CW_T) * hmax : 0));
  launch(c, KID_ceig, k_ceigw_form, dim3(parts, (unsigned)nw), dim3(MRC_NT), st, a);
  if (a.pencil) {
    const int ntmax = (int)((nfmax + CW_T - 1) / CW_T);
    const size_t tile = (size_t)CW_T * CW_LD * sizeof(double);
    for (int j = 0; j < ntmax; ++j) {
      launch_lds(c, KID_ceig, k_ceigw_potrf, dim3((unsigned)nw), dim3(MRC_NT), tile, st, a, j);
      const unsigned rem = (unsigned)(ntmax - 1 - j);
      if (rem == 0) break;
      launch_lds(c, KID_ceig, k_ceigw_panel, dim3(rem, (unsigned)nw), dim3(MRC_NT), 2 * tile, st, a, j);
      launch_lds(c, KID_ceig, k_ceigw_trail, dim3(rem * (rem + 1) / 2, (unsigned)nw), dim3(MRC_NT), 2 * tile, st, a, j);
    }
    launch_lds(c, KID_ceig, k_ceigw_solve<true>, dim3((unsigned)ntmax, (unsigned)nw), dim3(MRC_NT), CW_APPLY_LDS, st, a);
    launch_lds(c, KID_ceig, k_ceigw_solve<false>, dim3((unsigned)ntmax, (unsigned)nw), dim3(MRC_NT), CW_APPLY_LDS, st, a);
    launch(c, KID_ceig, k_ceigw_symm, dim3(parts, (unsigned)nw), dim3(MRC_NT), st, a);
  }
  launch(c, KID_ceig, k_ceigw_begin, dim3((unsigned)nw), dim3(MRC_NT), st, a);
  for (;;) {
    launch(c, KID_ceig_reduce, k_ceigw_check, dim3(1), dim3(MRC_NT), st, a);
    int32_t nrun = 0;
    HIPCHK(hipMemcpyAsync(&nrun, a.nrun, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nrun <= 0) break;
    for (int r = 0; r < steps; ++r) {
      launch_lds(c, KID_ceig, k_ceigw_pivot, dim3((unsigned)hmax, (unsigned)nw), dim3(MRC_NT), CW_PIVOT_LDS, st, a, r);
      launch_lds(c, KID_ceig, k_ceigw_apply, dim3(tiles, (unsigned)nw), dim3(MRC_NT), CW_APPLY_LDS, st, a, r, hmax);
    }
  }
  launch(c, KID_ceig, k_ceigw_sort, dim3((unsigned)nw), dim3(MRC_NT), st, a);
  if (a.vec) launch(c, KID_ceig, k_ceigw_out, dim3(parts, (unsigned)nw), dim3(MRC_NT), st, a);
  return 0;
}

// The wide cliques of a call (ascending), in groups whose workspace stays within hbm_doubles (always at least one clique);
// pencil: m.x2 / m.upd2 hold B, and the workspace of a clique holds G as well
int ceigw_pass(csp_ctx* c, const MrcArgs& m, bool vec, bool pencil, hipStream_t st) {
  const Symbolic& S = c->S;
  CeigwArgs a{};
  a.m = m;
  a.vec = vec ? 1 : 0;
  a.pencil = pencil ? 1 : 0;
  std::vector<CeigwDesc> desc;
  int64_t doubles = 0;
  c->ceig_wide_count = 0;
  c->ceig_groups = 0;
  for (int64_t k = 0; k < S.nsn; ++k) {
    if (!ceig_is_wide(c, k)) continue;
    ++c->ceig_wide_count;
    CeigwDesc w;
    int64_t len = ceigw_layout(w, (int32_t)k, S.nf(k), vec, doubles, pencil);
    if (!desc.empty() && doubles + len > hbm_doubles(c)) {
      ++c->ceig_groups;
      if (int rc = ceigw_group(c, a, desc, doubles, st)) return rc;
      desc.clear();
      doubles = 0;
      len = ceigw_layout(w, (int32_t)k, S.nf(k), vec, 0, pencil);
    }
    desc.push_back(w);
    doubles += len;
  }
  if (desc.empty()) return 0;
  ++c->ceig_groups;
  return ceigw_group(c, a, desc, doubles, st);
}

// csp_clique_eigh (vmode 0) and csp_clique_project (vmode 1): the launches of csp_clique_eigvalsh in standard form with
// k_ceig_vec in the slots of the pencil form, under the same kernel ids; ext null: the context's own four doubles
int ceig_vec_pass(csp_ctx* c, const double* a, int vmode, double lo, double hi, double* Q, double* w, double* ext, double* info,
                  hipStream_t st) {
  const Symbolic& S = c->S;
  DeviceCtx& D = c->D;
  const int64_t nsn = S.nsn;
  c->slot_share = 0;
  if (int rc = mrc_setup(c)) return rc;
  if (!ext && !D.mrc.ext)
    if (int rc = dev_alloc(&D.mrc.ext, 4, D.mem)) return rc;
  std::vector<int64_t> need, ranges;
  if (int rc = slot_sorted_lists(c, all_cliques(S), [&](int64_t k) { return ceig_is_wide(c, k) ? (int64_t)-1 : ceig_slot2(S.nf(k)); }, need, ranges, st))
    return rc;
  gather_all(c, a, 0, 1, D.upd, st);
  MrcArgs m = mrc_args(c, a, 0.0);
  m.w = w;
  m.Q = Q;
  m.qptr = D.mrc.qptr;
  m.lo = lo;
  m.hi = hi;
  m.pinfo = info;
  m.vmode = vmode;
  if (int rc = mrc_launch<k_ceig_vec>(c, KID_ceig, m, need, 0, (int64_t)need.size(), st)) return rc;
  if (int rc = ceigw_pass(c, m, true, false, st)) return rc;
  int32_t* dout = D.mrc.ints + 2 * nsn;
  launch(c, KID_ceig_reduce, k_ceig_reduce, dim3(1), dim3(MRC_NT), st, (const CliqueDesc*)D.cl, (const double*)w, (const int32_t*)m.rank,
         (const int32_t*)m.flag, (int)nsn, ext ? ext : D.mrc.ext, dout);
  HIPCHK(end_call(c));
  int32_t out[3];
  HIPCHK(hipMemcpyAsync(out, dout, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  c->ceig_sweeps = out[2];
  if (out[1]) return SMCP_ENOCONV;
  return 0;
}

// workgroups of k_cone_update, which is also the number of its partial sums: a function of blklen alone
int64_t cone_parts(const Symbolic& S) { return std::max<int64_t>(1, std::min<int64_t>(1024, (S.blklen() + 4 * MRC_NT - 1) / (4 * MRC_NT))); }

// What csp_cone_project_steps keeps for the life of the context, made by its first call: the workspace of CompletionWs,
// room for its list of cliques (a list of its own: D.mrc.list belongs to whichever call runs; filled by cone_route) and
// the signed multiplicities, by one launch of k_cone_mult per level, leaves first
int cone_setup(csp_ctx* c, hipStream_t st) {
  const Symbolic& S = c->S;
  DeviceCtx& D = c->D;
  if (int rc = mrc_setup(c)) return rc;
  if (int rc = qptr_setup(c)) return rc;
  if (D.mrc.cone_mw) return 0;
  if (int rc = dev_alloc(&D.mrc.cone_list, S.nsn, D.mem)) return rc;
  if (int rc = dev_alloc(&D.mrc.cone_sw, S.blklen(), D.mem)) return rc;
  if (int rc = dev_alloc(&D.mrc.cone_info, 2 * S.nsn, D.mem)) return rc;
  if (int rc = dev_alloc(&D.mrc.cone_part, cone_parts(S), D.mem)) return rc;
  if (int rc = dev_alloc(&D.mrc.cone_sweeps, 1, D.mem)) return rc;
  double* mw = nullptr;
  if (int rc = dev_alloc(&mw, S.blklen(), D.mem)) return rc;
  TreeArgs a = tree_args(c);
  for_levels_up(c, [&](const int32_t* lev, int cnt) {
    a.lev = lev;
    launch(c, KID_gather_level, k_cone_mult, dim3((unsigned)cnt), dim3(MRC_NT), st, a, mw);
  });
  HIPCHK(hipMemsetAsync(D.mrc.cone_sweeps, 0, sizeof(int32_t), st));
  D.mrc.cone_mw = mw;                    // last: marks the workspace as made
  return 0;
}

// Which clique takes which route in csp_cone_project_steps, made by the first call under a value of CSP_TUNE_CEIG_WIDE and
// again when a call sees another value (c->cone_wide; it waits for the device and uploads synchronously): the slot-sorted
// list of the cliques of k_cone_split with its slot sizes -- all cliques at 0, which is the list of a context never tuned --
// and, for the wide ones, their descriptors (with V) in launch groups within hbm_doubles, kept on the device, the
// workspace of the largest group and the buffer of their eigenvalues.  The lists are made again as well when
// CSP_TUNE_SLOT_DOUBLES has changed (c->cone_limit).  SMCP_EHIP without the 128 KiB LDS class.
int cone_route(csp_ctx* c, hipStream_t st) {
  const Symbolic& S = c->S;
  DeviceCtx& D = c->D;
  // keyed on both tunes, also at CSP_TUNE_CEIG_WIDE 0, where there are no groups and the lists do not depend on the limit:
  // one rule, and the remake (with its wait) costs only the call after the limit was changed
  if (c->cone_wide == c->ceig_wide && c->cone_limit == hbm_doubles(c)) return 0;
  c->cone_wide = -1;
  HIPCHK(hipDeviceSynchronize());        // launches of earlier calls, on whatever stream, may still read the lists
  std::vector<std::pair<int64_t, int32_t>> tmp;
  for (int64_t k : S.levidx)
    if (!ceig_is_wide(c, k)) tmp.push_back({ceig_slot2(S.nf(k)), (int32_t)k});
  std::stable_sort(tmp.begin(), tmp.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
  std::vector<int32_t> list;
  c->cone_need.clear();
  for (auto& t : tmp) { c->cone_need.push_back(t.first); list.push_back(t.second); }
  if (!list.empty()) HIPCHK(hipMemcpy(D.mrc.cone_list, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  std::vector<CeigwDesc> desc;
  c->cone_groups.clear();
  int64_t doubles = 0, most = 0;
  for (int64_t k = 0; k < S.nsn; ++k) {
    if (!ceig_is_wide(c, k)) continue;
    CeigwDesc w;
    int64_t len = ceigw_layout(w, (int32_t)k, S.nf(k), true, doubles);
    if (c->cone_groups.empty() || (c->cone_groups.back().nw > 0 && doubles + len > hbm_doubles(c))) {
      csp_ctx::ConeGroup g;
      g.first = (int)desc.size();
      c->cone_groups.push_back(g);
      doubles = 0;
      len = ceigw_layout(w, (int32_t)k, S.nf(k), true, 0);
    }
    csp_ctx::ConeGroup& g = c->cone_groups.back();
    ++g.nw;
    g.hmax = std::max(g.hmax, (int)w.h);
    g.nbmax = std::max(g.nbmax, (int)w.nb);
    g.nfmax = std::max<int64_t>(g.nfmax, w.nf);
    desc.push_back(w);
    doubles += len;
    most = std::max(most, doubles);
  }
  if (!desc.empty()) {
    if (lds_ceiling<k_ceigw_pivot>() < (int64_t)CW_PIVOT_LDS + 4096 || lds_ceiling<k_ceigw_apply>() < (int64_t)CW_APPLY_LDS + 4096) return SMCP_EHIP;
    if (int rc = dev_grow(&D.mrc.cone_wdesc, &D.mrc.cone_wdesc_cap, (int64_t)desc.size(), D.mem, st)) return rc;
    HIPCHK(hipMemcpy(D.mrc.cone_wdesc, desc.data(), desc.size() * sizeof(CeigwDesc), hipMemcpyHostToDevice));
    if (int rc = dev_grow(&D.mrc.wws, &D.mrc.wcap, most, D.mem, st)) return rc;
    if (!D.mrc.wbuf)
      if (int rc = dev_alloc(&D.mrc.wbuf, S.rowptr[S.nsn], D.mem)) return rc;
  }
  c->cone_limit = hbm_doubles(c);
  c->cone_wide = c->ceig_wide;           // last: marks the lists as made for these values
  return 0;
}

// The clique step of the wide cliques of an iteration of csp_cone_project_steps, group by group in the one workspace: the
// launches of ceigw_group with the cone kernels at both ends and its stopping rule without its read-back -- every block
// sweep the rule allows is enqueued, and the launches behind the check that ended a clique return at their top (section 23).
// The number of launches depends on the pattern and the tune alone.
void cone_wide_pass(csp_ctx* c, const MrcArgs& m, hipStream_t st) {
  DeviceCtx& D = c->D;
  CeigwArgs a{};
  a.m = m;
  a.m.vmode = CW_VMODE_CONE;
  a.m.w = D.mrc.wbuf;
  a.vec = 1;
  a.ws = D.mrc.wws;
  a.nrun = D.mrc.ints + 2 * c->S.nsn + 3;
  for (const csp_ctx::ConeGroup& g : c->cone_groups) {
    a.wd = D.mrc.cone_wdesc + g.first;
    a.nw = g.nw;
    const unsigned nw = (unsigned)g.nw, parts = (unsigned)ceigw_parts(g.nfmax);
    const int steps = g.nbmax + (g.nbmax & 1) - 1;
    const unsigned tiles = (unsigned)(g.hmax * (g.hmax + 1) / 2 + (int)((g.nfmax + CW_T - 1) / CW_T) * g.hmax);
    launch(c, KID_ceig, k_ceigw_cone_form, dim3(parts, nw), dim3(MRC_NT), st, a);
    launch(c, KID_ceig, k_ceigw_begin, dim3(nw), dim3(MRC_NT), st, a);
    for (int s = 0; s < CEIG_MAX_SWEEPS; ++s) {
      launch(c, KID_ceig_reduce, k_ceigw_check, dim3(1), dim3(MRC_NT), st, a);
      for (int r = 0; r < steps; ++r) {
        launch_lds(c, KID_ceig, k_ceigw_pivot, dim3((unsigned)g.hmax, nw), dim3(MRC_NT), CW_PIVOT_LDS, st, a, r);
        launch_lds(c, KID_ceig, k_ceigw_apply, dim3(tiles, nw), dim3(MRC_NT), CW_APPLY_LDS, st, a, r, g.hmax);
      }
    }
    launch(c, KID_ceig_reduce, k_ceigw_check, dim3(1), dim3(MRC_NT), st, a);
    launch(c, KID_ceig, k_ceigw_sort, dim3(nw), dim3(MRC_NT), st, a);
    launch(c, KID_ceig, k_ceigw_cone_split, dim3(parts, nw), dim3(MRC_NT), st, a);
    launch(c, KID_ceig, k_ceigw_cone_finish, dim3(nw), dim3(MRC_NT), st, a);
  }
}

}  // namespace

extern "C" {

// ---- minimum-rank completion (front_mrc.hip) ----------------------------------------------------------------------
int csp_mrcompletion_rank(csp_ctx* c, const double* x, double tol, int64_t* r, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!x || !r || !(tol >= 0.0) || c->ntrial != 1) return SMCP_EINVAL;
  return rank_pass<k_mrc_rank>(c, x, tol, KID_mrc_rank, KID_mrc_reduce, k_mrc_reduce, true, false, r, (hipStream_t)stream);
}

int csp_mrcompletion(csp_ctx* c, const double* x, double tol, int64_t r, double* Y, int64_t ldY, void* stream) {
  if (int rc = factor_args_check(c, x, tol, r, Y, ldY)) return rc;
  if (r == 0) return 0;
  return factor_pass<k_mrc_factor>(c, x, tol, r, Y, ldY, KID_mrc_factor, mrc_slot2, true, &c->mrc_clamped, (hipStream_t)stream);
}

int csp_maxcut_cuts(csp_ctx* c, const double* Y, int64_t ldY, int64_t r, int64_t trials, const double* G, int64_t nedges,
                    const int64_t* ei, const int64_t* ej, const double* w, int8_t* s, double* cut, void* stream) {
  if (int rc = ready(c)) return rc;
  const int64_t n = c->S.n;
  if (r < 1 || ldY < r || trials < 1 || trials > 65535 || nedges < 0 || !Y || !G || !s || !cut || (nedges && (!ei || !ej || !w)))
    return SMCP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  launch(c, KID_cut_signs, k_cut_signs, dim3((unsigned)((n + MRC_NT - 1) / MRC_NT), (unsigned)trials), dim3(MRC_NT), st, n, (int)r,
         Y, ldY, G, s);
  launch(c, KID_cut_weights, k_cut_weights, dim3((unsigned)trials), dim3(MRC_NT), st, n, nedges, ei, ej, w, (const int8_t*)s, cut);
  HIPCHK(end_call(c));
  return 0;
}

// ---- spectra of the clique blocks (front_ceig.hip) ------------------------------------------------------------------
// One launch group over all cliques, as pass 1 of the completions: the separator blocks of A (and of B, into the second
// gather buffer) gathered top-down, k_ceig by slot size, the wide cliques of CSP_TUNE_CEIG_WIDE in ceigw_pass (standard
// and pencil form), k_ceig_reduce, and the read-back of its three integers.
int csp_clique_eigvalsh(csp_ctx* c, const double* a, const double* b, double* w, double* ext, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!a || !w || c->ntrial != 1) return SMCP_EINVAL;
  const Symbolic& S = c->S;
  DeviceCtx& D = c->D;
  const int64_t nsn = S.nsn, wlen = S.rowptr[nsn];
  auto overlap = [](const double* p, int64_t np, const double* q, int64_t nq) { return p && q && p < q + nq && q < p + np; };
  for (const double* in : {a, b})
    if (overlap(w, wlen, in, S.blklen()) || overlap(ext, 4, in, S.blklen())) return SMCP_EINVAL;
  if (overlap(w, wlen, ext, 4)) return SMCP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  c->slot_share = 0;
  if (int rc = mrc_setup(c)) return rc;
  if (b && !D.mrc.upd2)
    if (int rc = dev_alloc(&D.mrc.upd2, S.updlen(), D.mem)) return rc;
  if (!ext && !D.mrc.ext)
    if (int rc = dev_alloc(&D.mrc.ext, 4, D.mem)) return rc;
  std::vector<int64_t> need, ranges;
  // the wide cliques leave the list for the block Jacobi of front_ceigw.hip, in both forms
  if (int rc = slot_sorted_lists(c, all_cliques(S), [&](int64_t k) { return ceig_is_wide(c, k) ? (int64_t)-1 : b ? ceig_slot2(S.nf(k)) : ceig_slot1(S.nf(k)); },
                                 need, ranges, st))
    return rc;
  gather_all(c, a, 0, 1, D.upd, st);
  if (b) gather_all(c, b, 0, 1, D.mrc.upd2, st);
  MrcArgs m = mrc_args(c, a, 0.0);
  m.x2 = b;
  m.upd2 = D.mrc.upd2;
  m.w = w;
  if (int rc = mrc_launch<k_ceig>(c, KID_ceig, m, need, 0, (int64_t)need.size(), st)) return rc;
  if (int rc = ceigw_pass(c, m, false, b != nullptr, st)) return rc;
  int32_t* dout = D.mrc.ints + 2 * nsn;
  launch(c, KID_ceig_reduce, k_ceig_reduce, dim3(1), dim3(MRC_NT), st, (const CliqueDesc*)D.cl, (const double*)w, (const int32_t*)m.rank,
         (const int32_t*)m.flag, (int)nsn, ext ? ext : D.mrc.ext, dout);
  HIPCHK(end_call(c));
  int32_t out[3];
  HIPCHK(hipMemcpyAsync(out, dout, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  c->ceig_sweeps = out[2];
  if (out[0]) return out[0];
  if (out[1]) return SMCP_ENOCONV;
  return 0;
}

// ---- packed clique blocks: gather, scatter, eigenvectors, projection (front_ceig.hip) -------------------------------
int csp_clique_ptr(csp_ctx* c, int64_t* qptr_host) {
  if (!c || !qptr_host) return SMCP_EINVAL;
  const std::vector<int64_t> q = clique_ptr_of(c->S);
  std::copy(q.begin(), q.end(), qptr_host);
  return 0;
}

// One launch over all cliques behind the top-down gathers of the separator blocks.
int csp_clique_gather(csp_ctx* c, const double* x, double* Z, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!x || !Z || c->ntrial != 1) return SMCP_EINVAL;
  const Symbolic& S = c->S;
  DeviceCtx& D = c->D;
  if (int rc = qptr_setup(c)) return rc;
  if (ranges_overlap({{Z, c->qlen}}, {{x, S.blklen()}})) return SMCP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  gather_all(c, x, 0, 1, D.upd, st);
  const unsigned parts = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, S.max_front * S.max_front / (MRC_NT * 32)));
  launch(c, KID_gather_level, k_clique_gather, dim3((unsigned)S.nsn, parts), dim3(MRC_NT), st, (const CliqueDesc*)D.cl, x, (const double*)D.upd,
         (const int64_t*)D.mrc.qptr, Z);
  HIPCHK(end_call(c));
  return 0;
}

// One launch per level, leaves first; D.upd is the update stack, as in csp_cholesky.
int csp_clique_scatter(csp_ctx* c, const double* Z, double* x, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!x || !Z || c->ntrial != 1 || c->xr_world > 1) return SMCP_EINVAL;
  if (int rc = qptr_setup(c)) return rc;
  if (ranges_overlap({{x, c->S.blklen()}}, {{Z, c->qlen}})) return SMCP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  invalidate_tags(c, x);
  TreeArgs a = tree_args(c);
  for_levels_up(c, [&](const int32_t* lev, int cnt) {
    a.lev = lev;
    launch(c, KID_gather_level, k_clique_scatter, dim3((unsigned)cnt), dim3(MRC_NT), st, a, Z, (const int64_t*)c->D.mrc.qptr, x);
  });
  HIPCHK(end_call(c));
  return 0;
}

int csp_clique_eigh(csp_ctx* c, const double* a, double* w, double* Q, double* ext, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!a || !w || !Q || c->ntrial != 1) return SMCP_EINVAL;
  if (int rc = qptr_setup(c)) return rc;
  const int64_t wlen = c->S.rowptr[c->S.nsn];
  if (ranges_overlap({{w, wlen}, {Q, c->qlen}, {ext, 4}}, {{a, c->S.blklen()}})) return SMCP_EINVAL;
  return ceig_vec_pass(c, a, 0, 0.0, 0.0, Q, w, ext, nullptr, (hipStream_t)stream);
}

int csp_clique_project(csp_ctx* c, const double* a, double lo, double hi, double* Z, double* w, double* info, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!a || !Z || !info || !(lo <= hi) || c->ntrial != 1) return SMCP_EINVAL;
  if (int rc = qptr_setup(c)) return rc;
  const int64_t wlen = c->S.rowptr[c->S.nsn];
  if (ranges_overlap({{Z, c->qlen}, {w, wlen}, {info, 2 * c->S.nsn}}, {{a, c->S.blklen()}})) return SMCP_EINVAL;
  if (!w) {
    if (!c->D.mrc.wbuf)
      if (int rc = dev_alloc(&c->D.mrc.wbuf, wlen, c->D.mem)) return rc;
    w = c->D.mrc.wbuf;
  }
  return ceig_vec_pass(c, a, 1, lo, hi, Z, w, nullptr, info, (hipStream_t)stream);
}

// Iterations it0 .. it0 + nsteps - 1 of the clique-splitting ADMM for the projection of a onto the cone of PSD-completable
// matrices, on the state (x, U, W) in place.  An iteration: gather_all of x into D.upd, k_cone_split by slot class,
// the fixed chain of cone_wide_pass for the cliques that CSP_TUNE_CEIG_WIDE sends to the block Jacobi (none at 0),
// k_clique_scatter of W per level into cone_sw (it uses D.upd as its stack, so it comes behind both), k_cone_update,
// k_cone_resid into row it of hist.  Nothing is read back, nothing waits, no buffer grows and nothing is uploaded, after
// the first call on the context under a value of the tune (cone_setup, cone_route).
int csp_cone_project_steps(csp_ctx* c, const double* a, double* x, double* U, double* W, double rho, double relax, int64_t it0,
                           int64_t nsteps, double* hist, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!a || !x || !U || !W || !hist || !(rho > 0.0) || !(relax > 0.0 && relax < 2.0) || it0 < 0 || nsteps < 1 || c->ntrial != 1 ||
      c->xr_world > 1)
    return SMCP_EINVAL;
  const Symbolic& S = c->S;
  DeviceCtx& D = c->D;
  hipStream_t st = (hipStream_t)stream;
  c->slot_share = 0;
  if (int rc = cone_setup(c, st)) return rc;
  if (ranges_overlap({{x, S.blklen()}, {U, c->qlen}, {W, c->qlen}, {hist, 4 * (it0 + nsteps)}}, {{a, S.blklen()}})) return SMCP_EINVAL;
  if (int rc = cone_route(c, st)) return rc;
  c->ceig_wide_count = S.nsn - (int64_t)c->cone_need.size();   // the cliques that left the list of k_cone_split
  c->ceig_groups = (int64_t)c->cone_groups.size();
  invalidate_tags(c, x);
  const int64_t nsn = S.nsn;
  const int npart = (int)cone_parts(S);
  MrcArgs m = mrc_args(c, x, 0.0);
  m.Q = U;
  m.pw = W;
  m.qptr = D.mrc.qptr;
  m.lo = relax;
  m.pinfo = D.mrc.cone_info;
  TreeArgs t = tree_args(c);
  for (int64_t it = it0; it < it0 + nsteps; ++it) {
    gather_all(c, x, 0, 1, D.upd, st);
    if (int rc = mrc_launch<k_cone_split>(c, KID_ceig, m, c->cone_need, 0, (int64_t)c->cone_need.size(), st, D.mrc.cone_list)) return rc;
    cone_wide_pass(c, m, st);
    for_levels_up(c, [&](const int32_t* lev, int cnt) {
      t.lev = lev;
      launch(c, KID_gather_level, k_clique_scatter, dim3((unsigned)cnt), dim3(MRC_NT), st, t, (const double*)W, (const int64_t*)D.mrc.qptr,
             D.mrc.cone_sw);
    });
    launch(c, KID_axpby, k_cone_update, dim3((unsigned)npart), dim3(MRC_NT), st, S.blklen(), a, (const double*)D.mrc.cone_sw,
           (const double*)D.mrc.cone_mw, rho, x, D.mrc.cone_part);
    launch(c, KID_ceig_reduce, k_cone_resid, dim3(1), dim3(MRC_NT), st, (const double*)D.mrc.cone_info, (const int32_t*)m.rank,
           (const int32_t*)m.flag, (int)nsn, (const double*)D.mrc.cone_part, npart, hist + 4 * it, D.mrc.cone_sweeps, it == 0 ? 1 : 0);
  }
  HIPCHK(end_call(c));
  return 0;
}

// the most Jacobi sweeps of a clique in any iteration since the csp_cone_project_steps that began at it0 = 0 (waits for the
// stream: one integer is read back)
int csp_cone_project_sweeps(csp_ctx* c, int64_t* out, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!out || !c->D.mrc.cone_sweeps) return SMCP_EINVAL;
  int32_t v = 0;
  HIPCHK(hipMemcpyAsync(&v, c->D.mrc.cone_sweeps, sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  *out = v;
  return 0;
}

// ---- Euclidean distance matrix completion (front_edm.hip) -----------------------------------------------------------
// Only the kernels and the pass-2 slot (edm_slot2, larger) differ from the minimum-rank completion; diag(D) = 0 is checked
// by the reduce kernel, not read by the thresholds.
int csp_edmcompletion_rank(csp_ctx* c, const double* x, double tol, int64_t* r, void* stream) {
  if (int rc = ready(c)) return rc;
  if (!x || !r || !(tol >= 0.0) || c->ntrial != 1) return SMCP_EINVAL;
  return rank_pass<k_edm_rank>(c, x, tol, KID_edm_rank, KID_edm_reduce, k_edm_reduce, false, true, r, (hipStream_t)stream);
}

int csp_edmcompletion(csp_ctx* c, const double* x, double tol, int64_t r, double* Y, int64_t ldY, void* stream) {
  if (int rc = factor_args_check(c, x, tol, r, Y, ldY)) return rc;
  c->edm_clamped = 0;
  if (r == 0) return 0;
  return factor_pass<k_edm_factor>(c, x, tol, r, Y, ldY, KID_edm_factor, edm_slot2, false, &c->edm_clamped, (hipStream_t)stream);
}

int csp_edm_dense(csp_ctx* c, const double* Y, int64_t ldY, int64_t r, const int64_t* perm, double* D, int64_t ldD,
                  void* stream) {
  if (int rc = ready(c)) return rc;
  const int64_t n = c->S.n;
  if (r < 0 || r > INT32_MAX || (r > 0 && (!Y || ldY < r)) || !D || ldD < n) return SMCP_EINVAL;
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nt = (unsigned)((n + EDM_TILE - 1) / EDM_TILE);
  if (nt > 65535) return SMCP_EINVAL;
  launch(c, KID_edm_dense, k_edm_dense, dim3(nt, nt), dim3(MRC_NT), st, n, (int)r, Y, ldY, perm, D, ldD);
  HIPCHK(end_call(c));
  return 0;
}

// ---- dense maximum-determinant PSD completion (front_psd.hip) -------------------------------------------------------
int csp_psdcompletion(csp_ctx* c, const double* x, double tol, double* Xd, int64_t ldX, void* stream) {
  if (int rc = ready(c)) return rc;
  const Symbolic& S = c->S;
  const int64_t n = S.n, nsn = S.nsn;
  if (!x || !Xd || !(tol >= 0.0) || ldX < n || c->ntrial != 1) return SMCP_EINVAL;
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  DeviceCtx& D = c->D;
  if (int rc = mrc_setup(c)) return rc;
  if (int rc = psd_setup(c)) return rc;
  const PsdPlan& P = D.psd;
  // is every clique block positive semidefinite?  (pass 1 of the minimum-rank completion)
  if (int rc = rank_pass<k_mrc_rank>(c, x, tol, KID_mrc_rank, KID_mrc_reduce, k_mrc_reduce, true, false, nullptr, st)) return rc;
  launch(c, KID_psd_zero, k_psd_zero, dim3((unsigned)((n + MRC_NT - 1) / MRC_NT), (unsigned)std::min<int64_t>(n, 1024)), dim3(MRC_NT), st,
         n, Xd, ldX);
  launch(c, KID_psd_scatter, k_psd_scatter, dim3((unsigned)nsn), dim3(MRC_NT), st, (const CliqueDesc*)D.cl, (const int32_t*)D.rowidx, x,
         Xd, ldX);
  // the solves: the cliques with a separator (ascending, then by slot size)
  std::vector<int64_t> ks((size_t)nsn), need, ranges;
  for (int64_t k = 0; k < nsn; ++k) ks[(size_t)k] = k;
  if (int rc = slot_sorted_lists(c, {{ks.data(), ks.data() + nsn}}, [&](int64_t k) { return S.na(k) > 0 ? psd_slot(S.na(k)) : (int64_t)-1; }, need, ranges, st))
    return rc;
  MrcArgs a = mrc_args(c, x, tol);
  a.pw = P.w;
  a.pidx = P.idx;
  a.pra = P.ra;
  if (int rc = mrc_launch<k_psd_solve>(c, KID_psd_solve, a, need, 0, (int64_t)need.size(), st)) return rc;
  PsdFillArgs f{D.cl, D.rowidx, nullptr, P.ulist, P.w, P.idx, P.ra, Xd, ldX};
  for (const csp_ctx::PsdLevel& L : c->psd_lev) {
    if (L.b2 > L.b1) {
      f.tasks = P.tasks + L.b1;
      launch(c, KID_psd_fill, k_psd_fill, dim3((unsigned)(L.b2 - L.b1)), dim3(256), st, f);
    }
    if (L.e2 > L.b2) {
      f.tasks = P.tasks + L.b2;
      launch(c, KID_psd_fill, k_psd_fill, dim3((unsigned)(L.e2 - L.b2)), dim3(256), st, f);
    }
  }
  HIPCHK(end_call(c));
  return 0;
}

}  // extern "C"
