// Host drivers of the products with dense blocks: trmm (front_trmm.hip), syr2k / syrk (front_syr2k.hip) and symm
// (front_symm.hip), and of the factor as a sum of clique blocks (front_cdec.hip).  Included by capi.hip.  Each operation
// builds its plan (context.hpp) once per context and then runs in a fixed number of launches: the products of all cliques
// at once and, for trmm and symm, one combining pass over a transposed row index.

namespace {

// The cliques with the large fronts first, the widest front first among them (the long tiles start first), then the rest
// in ascending order.  The first D.nII_total entries are the large fronts.
std::vector<int64_t> large_fronts_first(const csp_ctx* c) {
  const Symbolic& S = c->S;
  std::vector<int64_t> order;
  for (int pass = 1; pass >= 0; --pass)
    for (int64_t k = 0; k < S.nsn; ++k) if ((c->large_mask[(size_t)k] != 0) == (pass == 1)) order.push_back(k);
  std::stable_sort(order.begin(), order.begin() + c->D.nII_total, [&](int64_t x, int64_t y) { return S.nf(x) > S.nf(y); });
  return order;
}

// Builds a transposed row index (RowIndex, context.hpp) over n rows and ntot contributions and uploads it.  each(f) calls
// f(row, slot) once per contribution IN THE ORDER OF THE ROW SUMS of the combine kernel: the contribution stored by its
// producer at `slot` gets the next position of `row`.  That order decides the bits of the results.
template <class Each>
int build_row_index(RowIndex* R, int64_t n, int64_t ntot, int heavy_from, Each each, DevLedger& mem) {
  std::vector<int64_t> tptr((size_t)n + 1, 0);
  each([&](int64_t row, int64_t) { ++tptr[(size_t)row + 1]; });
  for (int64_t i = 0; i < n; ++i) tptr[(size_t)i + 1] += tptr[(size_t)i];
  std::vector<int32_t> pos((size_t)ntot);
  {
    std::vector<int64_t> fill(tptr.begin(), tptr.end() - 1);
    each([&](int64_t row, int64_t slot) { pos[(size_t)slot] = (int32_t)fill[(size_t)row]++; });
  }
  std::vector<int32_t> heavy;
  for (int64_t i = 0; i < n; ++i) if (tptr[(size_t)i + 1] - tptr[(size_t)i] > heavy_from) heavy.push_back((int32_t)i);
  R->nheavy = (int64_t)heavy.size();
  if (int rc = dev_upload(&R->pos, pos, mem)) return rc;
  if (int rc = dev_upload(&R->heavy, heavy, mem)) return rc;
  return dev_upload(&R->tptr, tptr, mem);      // last: tptr marks the index (and its owner's plan) as built
}

// Which kernels take the fronts of a product: the FMA kernels only, tile products for the large fronts, or tile products
// for every front.
enum class Route { fma, tiles_large, tiles_all };
// sw: the operation's SMCP_*_MM switch (0: FMA only, 2: tile products for the large fronts at most); cols: columns of the
// dense block or ranks of the update; tile products take the large fronts from min_large on and every front from min_all
// on.  sw2_forces_large: the switch value 2 sends the large fronts to the tile products whatever cols is.  Everything on
// the generic / deterministic route stays on the FMA kernels.
Route product_route(csp_ctx* c, int sw, int64_t cols, int64_t min_large, int64_t min_all, bool has_large, bool sw2_forces_large) {
  if (!sw || use_generic(c) || !use_large()) return Route::fma;
  if (sw != 2 && cols >= min_all) return Route::tiles_all;
  if ((cols >= min_large || (sw == 2 && sw2_forces_large)) && has_large) return Route::tiles_large;
  return Route::fma;
}

// f(integral_constant<int, CB>) for the column block CB of an FMA kernel: 1, up to 4, or wider (8)
template <class F>
void with_column_block(int64_t cols, F f) {
  if (cols == 1) f(std::integral_constant<int, 1>{});
  else if (cols <= 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

// Grid of a combining pass over n rows and nrhs columns: `light` workgroups sum a thread per entry, `heavy` more a wave
// per entry of the nheavy rows with long sums
struct CombineGrid { int light, heavy; };
CombineGrid combine_grid(const DeviceCtx& D, int64_t n, int64_t nrhs, int64_t nheavy) {
  const int64_t cap = 16 * (int64_t)D.ncu;
  return {(int)std::min<int64_t>((n * nrhs + 255) / 256, cap), (int)std::min<int64_t>((nheavy * nrhs + 3) / 4, cap)};
}

// ---- products with the factor (front_trmm.hip) ----------------------------------------------------------------------
// Once per context: the transposed separator index (specified by the numpy restatement of tests/trmm_ref.py: position p
// of its lists (tk, tq) is pos[sepptr[tk[p]] + tq[p]] here), the item lists of the FMA kernels and the row tiles of the
// tile products.
int trmm_setup(csp_ctx* c) {
  DeviceCtx& D = c->D;
  TrmmPlan& P = D.trmm;
  if (P.idx.tptr) return 0;
  const Symbolic& S = c->S;
  if (S.sepptr[S.nsn] >= ((int64_t)1 << 31)) return SMCP_EINVAL;      // positions are 32-bit
  // items: the cliques outside the large class, then the large fronts; for N every group is padded to whole workgroups
  // (clique -1) and the row chunks of wide supernodes come last, four items (the parts of the k range) each
  std::vector<int32_t> items[2];
  int64_t nsmall[2] = {0, 0};
  auto pad = [&]() { while ((items[0].size() / 2) % TRMM_WAVES) { items[0].push_back(-1); items[0].push_back(0); } };
  for (int pass = 0; pass < 3; ++pass) {          // N: small, large, split
    for (int64_t k = 0; k < S.nsn; ++k) {
      const bool large = c->large_mask[(size_t)k] != 0, split = large && S.nn(k) >= TRMM_SPLIT_NN;
      if (pass != (split ? 2 : large ? 1 : 0)) continue;
      for (int64_t ch = 0; ch < (S.nf(k) + 63) / 64; ++ch)
        for (int part = 0; part < (split ? TRMM_WAVES : 1); ++part) { items[0].push_back((int32_t)k); items[0].push_back(trmm_code((int)ch, part, split ? 1 : 0)); }
    }
    pad();
    if (pass == 0) nsmall[0] = (int64_t)items[0].size() / 2;
  }
  for (int pass = 0; pass < 2; ++pass) {          // T: small, large
    for (int64_t k = 0; k < S.nsn; ++k) {
      if ((c->large_mask[(size_t)k] != 0) != (pass == 1)) continue;
      for (int64_t ch = 0; ch < (S.nn(k) + TRMM_JC - 1) / TRMM_JC; ++ch) { items[1].push_back((int32_t)k); items[1].push_back((int32_t)ch); }
    }
    if (pass == 0) nsmall[1] = (int64_t)items[1].size() / 2;
  }
  // row tiles of the tile products: the large fronts first
  std::vector<int32_t> tiles[2];
  int64_t nlarge[2] = {0, 0};
  const std::vector<int64_t> order = large_fronts_first(c);
  for (size_t x = 0; x < order.size(); ++x) {
    const int64_t k = order[x];
    for (int t = 0; t < 2; ++t) {
      for (int64_t rt = 0; rt < tiles64((int)(t ? S.nn(k) : S.nf(k))); ++rt) { tiles[t].push_back((int32_t)k); tiles[t].push_back((int32_t)rt); }
      if ((int64_t)x + 1 == D.nII_total) nlarge[t] = (int64_t)tiles[t].size() / 2;
    }
  }
  for (int t = 0; t < 2; ++t) {
    if (int rc = dev_upload(&P.tiles[t], tiles[t], D.mem)) return rc;
    P.ntiles[t][0] = nlarge[t];
    P.ntiles[t][1] = (int64_t)tiles[t].size() / 2;
    if (int rc = dev_upload(&P.items[t], items[t], D.mem)) return rc;
    P.nitems[t][0] = nsmall[t];
    P.nitems[t][1] = (int64_t)items[t].size() / 2;
  }
  auto each = [&](auto f) {                       // ascending k: the order of the sums of k_trmm_combine
    for (int64_t k = 0; k < S.nsn; ++k)
      for (int64_t q = 0; q < S.na(k); ++q) f(S.rowidx[S.rowptr[k] + S.nn(k) + q], S.sepptr[k] + q);
  };
  return build_row_index(&P.idx, S.n, S.sepptr[S.nsn], TRMM_HEAVY, each, D.mem);
}

// ---- rank-k updates projected on the pattern (front_syr2k.hip) ------------------------------------------------------
// Once per context: the item list of the FMA kernel and the tile list of the tile products.
int syr2k_setup(csp_ctx* c) {
  DeviceCtx& D = c->D;
  Syr2kPlan& P = D.syr2k;
  if (P.ready) return 0;
  const Symbolic& S = c->S;
  std::vector<int32_t> items, tiles;
  auto list = [&](std::vector<int32_t>& out, int64_t k, int rows, int cols) {       // computing entries, then the zero-only ones
    const int64_t nf = S.nf(k), nn = S.nn(k);
    for (int zero = 0; zero < 2; ++zero)
      for (int64_t r = 0; r < (nf + rows - 1) / rows; ++r)
        for (int64_t j = 0; j < (nn + cols - 1) / cols; ++j) {
          const bool above = std::min<int64_t>(r * rows + rows, nf) - 1 < j * cols;   // the last row lies above the first column
          if (above == (zero == 1)) { out.push_back((int32_t)k); out.push_back((int32_t)r); out.push_back((int32_t)j); out.push_back(zero); }
        }
  };
  for (int pass = 0; pass < 2; ++pass) {          // items: small, large
    for (int64_t k = 0; k < S.nsn; ++k) if ((c->large_mask[(size_t)k] != 0) == (pass == 1)) list(items, k, 64, SYR2K_JC);
    P.nitems[pass] = (int64_t)items.size() / 4;
  }
  const std::vector<int64_t> order = large_fronts_first(c);      // tiles: large, small
  for (size_t x = 0; x < order.size(); ++x) {
    list(tiles, order[x], LT, LT);
    if ((int64_t)x + 1 == D.nII_total) P.ntiles[0] = (int64_t)tiles.size() / 4;
  }
  P.ntiles[1] = (int64_t)tiles.size() / 4;
  if (P.nitems[1] >= ((int64_t)1 << 31) || P.ntiles[1] >= ((int64_t)1 << 31)) return SMCP_EINVAL;     // grid dimension
  if (int rc = dev_upload(&P.items, items, D.mem)) return rc;
  if (int rc = dev_upload(&P.tiles, tiles, D.mem)) return rc;
  P.ready = true;
  return 0;
}

// ---- the factor as a sum of clique blocks (front_cdec.hip) -----------------------------------------------------------
// Once per context: the item list of the FMA kernel over the full nf x nf blocks and the lower tile pairs of the tile
// products.
int cdec_setup(csp_ctx* c) {
  DeviceCtx& D = c->D;
  CdecPlan& P = D.cdec;
  if (P.ready) return 0;
  const Symbolic& S = c->S;
  std::vector<int32_t> items, tiles;
  for (int pass = 0; pass < 2; ++pass) {          // items: small, large
    for (int64_t k = 0; k < S.nsn; ++k) {
      if ((c->large_mask[(size_t)k] != 0) != (pass == 1)) continue;
      for (int64_t r = 0; r < (S.nf(k) + 63) / 64; ++r)
        for (int64_t j = 0; j < (S.nf(k) + CDEC_JC - 1) / CDEC_JC; ++j) { items.push_back((int32_t)k); items.push_back((int32_t)r); items.push_back((int32_t)j); items.push_back(0); }
    }
    P.nitems[pass] = (int64_t)items.size() / 4;
  }
  const std::vector<int64_t> order = large_fronts_first(c);      // tiles: the large fronts, the only ones that take them
  for (int64_t x = 0; x < D.nII_total; ++x)
    for (int64_t r = 0; r < tiles64((int)S.nf(order[(size_t)x])); ++r)
      for (int64_t j = 0; j <= r; ++j) { tiles.push_back((int32_t)order[(size_t)x]); tiles.push_back((int32_t)r); tiles.push_back((int32_t)j); tiles.push_back(0); }
  P.ntiles = (int64_t)tiles.size() / 4;
  if (P.nitems[1] >= ((int64_t)1 << 31) || P.ntiles >= ((int64_t)1 << 31)) return SMCP_EINVAL;     // grid dimension
  if (int rc = dev_upload(&P.items, items, D.mem)) return rc;
  if (int rc = dev_upload(&P.tiles, tiles, D.mem)) return rc;
  P.ready = true;
  return 0;
}

int qptr_setup(csp_ctx* c);      // (completions.hip, which follows this file in capi.hip)

// ---- products of the matrix itself with a dense block (front_symm.hip) -----------------------------------------------
// rows of chunk r of clique k that part p of its columns multiplies, and the columns of that part with a column partial
// (false: the chunk lies above the diagonal of the part, no item)
bool symm_extent(const Symbolic& S, int64_t k, int64_t r, int64_t p, int64_t* nrows, int64_t* ncol) {
  const int64_t last = std::min<int64_t>(r * SYMM_ROWS + SYMM_ROWS, S.nf(k)) - 1;
  if (p * SYMM_KP > last) return false;
  *nrows = last - r * SYMM_ROWS + 1;
  *ncol = std::max<int64_t>(0, std::min(std::min<int64_t>(S.nn(k), p * SYMM_KP + SYMM_KP), last) - p * SYMM_KP);
  return true;
}

// The items (k, r, p, base in pos) in ascending order (specified by the numpy restatement of tests/symm_ref.py); returns
// the number of positions.  Host only; with items == nullptr it counts the positions and builds nothing, and no item is
// listed beyond 2^31 positions (positions are 32-bit: symm_setup refuses).
int64_t symm_items(const Symbolic& S, std::vector<int32_t>* items) {
  int64_t ntot = 0, nrows, ncol;
  for (int64_t k = 0; k < S.nsn; ++k)
    for (int64_t r = 0; r < (S.nf(k) + SYMM_ROWS - 1) / SYMM_ROWS; ++r)
      for (int64_t p = 0; p < (S.nn(k) + SYMM_KP - 1) / SYMM_KP; ++p) {
        if (!symm_extent(S, k, r, p, &nrows, &ncol)) continue;
        if (items && ntot < ((int64_t)1 << 31)) { items->push_back((int32_t)k); items->push_back((int32_t)r); items->push_back((int32_t)p); items->push_back((int32_t)ntot); }
        ntot += nrows + ncol;
      }
  return ntot;
}

// Once per context: the contribution index on the device (row i of C owning its partials in ascending (k, side, r, p)),
// and the item list with the large fronts first.
int symm_setup(csp_ctx* c) {
  DeviceCtx& D = c->D;
  SymmPlan& P = D.symm;
  if (P.idx.tptr) return 0;
  const Symbolic& S = c->S;
  std::vector<int32_t> byk;
  const int64_t ntot = symm_items(S, &byk);
  if (ntot >= ((int64_t)1 << 31)) return SMCP_EINVAL;                 // positions are 32-bit
  P.ntot = ntot;
  const size_t nitems = byk.size() / 4;
  std::vector<size_t> kfirst((size_t)S.nsn + 1, nitems);
  for (size_t it = nitems; it-- > 0;) kfirst[(size_t)byk[4 * it]] = it;
  for (int64_t k = S.nsn - 1; k >= 0; --k) kfirst[(size_t)k] = std::min(kfirst[(size_t)k], kfirst[(size_t)k + 1]);
  const std::vector<int64_t> order = large_fronts_first(c);
  std::vector<int32_t> items;
  items.reserve(byk.size());
  for (size_t x = 0; x < order.size(); ++x) {
    const size_t k = (size_t)order[x];
    items.insert(items.end(), byk.begin() + 4 * kfirst[k], byk.begin() + 4 * kfirst[k + 1]);
    if ((int64_t)x + 1 == D.nII_total) P.nitems[0] = (int64_t)items.size() / 4;
  }
  P.nitems[1] = (int64_t)items.size() / 4;
  if (int rc = dev_upload(&P.items, items, D.mem)) return rc;
  auto each = [&](auto f) {                       // ascending (k, side, r, p): the order of the sums of k_symm_combine
    int64_t nrows, ncol;
    for (int64_t k = 0; k < S.nsn; ++k)
      for (int side = 0; side < 2; ++side)
        for (size_t it = kfirst[(size_t)k]; it < kfirst[(size_t)k + 1]; ++it) {
          const int64_t r = byk[4 * it + 1], p = byk[4 * it + 2], base = byk[4 * it + 3];
          symm_extent(S, k, r, p, &nrows, &ncol);
          if (side == 0) for (int64_t j = 0; j < nrows; ++j) f(S.rowidx[S.rowptr[k] + r * SYMM_ROWS + j], base + j);
          else for (int64_t j = 0; j < ncol; ++j) f(S.snptr[k] + p * SYMM_KP + j, base + nrows + j);
        }
  };
  return build_row_index(&P.idx, S.n, ntot, SYMM_HEAVY, each, D.mem);
}

}  // namespace

extern "C" {

int csp_trmm(csp_ctx* c, const double* L, double* B, int64_t nrhs, int64_t ldb, double alpha, int trans, void* stream) {
  static const int mm = sw_int("SMCP_TRMM_MM", 1);     // read once per process
  if (int rc = ready(c)) return rc;
  // (grid limits of the column-block dimension; a partitioned context holds valid factors on its own cliques only)
  if (nrhs < 1 || nrhs > ((int64_t)1 << 18) || ldb < c->S.n || c->xr_world > 1) return SMCP_EINVAL;
  trans = trans ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  DeviceCtx& D = c->D;
  const TrmmPlan& P = D.trmm;
  const Symbolic& S = c->S;
  if (int rc = trmm_setup(c)) return rc;
  if (!trans && S.sepptr[S.nsn] * nrhs > D.max_rhs * D.tmplen) return SMCP_ENOMEM;
  // the scratch image of B is csp_trsm's: neither call keeps it
  if (int rc = dev_grow(&D.trsm_x, &D.trsm_x_len, ldb * nrhs, D.mem, st)) return rc;
  // tile products: the large fronts from eight columns on (the gate of csp_trsm), every front from TRMM_MM_ALL on
  const Route route = product_route(c, mm, nrhs, 8, TRMM_MM_ALL, D.nII_total > 0, false);
  TrmmArgs a;
  a.cl = D.cl; a.rowidx = D.rowidx; a.items = P.items[trans];
  a.nitems = route == Route::tiles_all ? 0 : (int)P.nitems[trans][route == Route::tiles_large ? 0 : 1];
  a.tiles = P.tiles[trans];
  a.L = L; a.B = B; a.X = D.trsm_x; a.U = D.tmp; a.pos = P.idx.pos; a.ntot = S.sepptr[S.nsn]; a.nrhs = (int)nrhs; a.ldb = ldb;
  if (a.nitems)
    with_column_block(nrhs, [&](auto cb) {        // CB columns of B per wave: L is read once per block of CB columns
      constexpr int CB = decltype(cb)::value;
      const dim3 grid((unsigned)((a.nitems + TRMM_WAVES - 1) / TRMM_WAVES), (unsigned)((a.nrhs + CB - 1) / CB));
      if (!trans) launch(c, KID_trmm_n, k_trmm_n<CB>, grid, dim3(64 * TRMM_WAVES), st, a);
      else launch(c, KID_trmm_t, k_trmm_t<CB>, grid, dim3(64 * TRMM_WAVES), st, a);
    });
  if (route != Route::fma) {
    const dim3 grid((unsigned)P.ntiles[trans][route == Route::tiles_all ? 1 : 0], (unsigned)tiles64((int)nrhs));
    if (!trans) launch(c, KID_trmm_mm, k_trmm_mm<false>, grid, dim3(256), st, a);
    else launch(c, KID_trmm_mm, k_trmm_mm<true>, grid, dim3(256), st, a);
  }
  const int64_t nheavy = trans ? 0 : P.idx.nheavy;
  const CombineGrid g = combine_grid(D, S.n, nrhs, nheavy);
  launch(c, KID_trmm_combine, k_trmm_combine, dim3((unsigned)(g.light + g.heavy)), dim3(256), st, (const int64_t*)(trans ? nullptr : P.idx.tptr),
         (const int32_t*)P.idx.heavy, (int)nheavy, g.light, (const double*)D.trsm_x, (const double*)D.tmp, a.ntot, B, S.n, (int)nrhs, ldb, alpha);
  HIPCHK(end_call(c));
  return 0;
}

int csp_syr2k(csp_ctx* c, double* X, const double* U, const double* V, int64_t k, int64_t ldu, int64_t ldv, double alpha, double beta,
              void* stream) {
  if (int rc = ready(c)) return rc;
  const int mm = sw_int("SMCP_SYR2K_MM", 1);      // read on every call: tools/syr2k_time.py alternates the settings in one process
  // (the inner dimension 2k is an int; a partitioned context keeps valid panels on its own cliques only)
  if (k < 1 || k > ((int64_t)1 << 18) || ldu < c->S.n || (V && ldv < c->S.n) || c->xr_world > 1) return SMCP_EINVAL;
  if (int rc = syr2k_setup(c)) return rc;
  DeviceCtx& D = c->D;
  const Syr2kPlan& P = D.syr2k;
  hipStream_t st = (hipStream_t)stream;
  invalidate_tags(c, X);
  // tile products for the large fronts from SYR2K_MM_LARGE ranks on and for every front from SYR2K_MM_ALL ranks on
  const Route route = product_route(c, mm, k, SYR2K_MM_LARGE, SYR2K_MM_ALL, D.nII_total > 0, false);
  Syr2kArgs a;
  a.cl = D.cl; a.rowidx = D.rowidx; a.items = P.items; a.tiles = P.tiles;
  a.nitems = route == Route::tiles_all ? 0 : (int)P.nitems[route == Route::tiles_large ? 0 : 1];
  a.X = X; a.U = U; a.V = V; a.k = (int)k; a.ldu = ldu; a.ldv = V ? ldv : ldu; a.alpha = alpha; a.beta = beta;
  if (a.nitems)
    with_column_block(k, [&](auto rb) {
      constexpr int RB = decltype(rb)::value;
      const dim3 grid((unsigned)((a.nitems + SYR2K_WAVES - 1) / SYR2K_WAVES));
      if (V) launch(c, KID_syr2k_fma, k_syr2k_fma<RB, true>, grid, dim3(64 * SYR2K_WAVES), st, a);
      else launch(c, KID_syr2k_fma, k_syr2k_fma<RB, false>, grid, dim3(64 * SYR2K_WAVES), st, a);
    });
  const int64_t ntiles = route == Route::fma ? 0 : P.ntiles[route == Route::tiles_all ? 1 : 0];
  if (ntiles) {
    if (V) launch(c, KID_syr2k_mm, k_syr2k_mm<true>, dim3((unsigned)ntiles), dim3(256), st, a);
    else launch(c, KID_syr2k_mm, k_syr2k_mm<false>, dim3((unsigned)ntiles), dim3(256), st, a);
  }
  HIPCHK(end_call(c));
  return 0;
}

// Z_k = P_k P_k^T for every clique (front_cdec.hip): one launch per route, two when the large fronts take the tile products.
// L is only read and nothing cached for it is touched.
int csp_clique_decompose(csp_ctx* c, const double* L, double* Z, void* stream) {
  if (int rc = ready(c)) return rc;
  // (a partitioned context holds valid factors on its own cliques only)
  if (!L || !Z || c->ntrial != 1 || c->xr_world > 1) return SMCP_EINVAL;
  if (int rc = qptr_setup(c)) return rc;
  if (ranges_overlap(Z, c->qlen, L, c->S.blklen())) return SMCP_EINVAL;
  if (int rc = cdec_setup(c)) return rc;
  DeviceCtx& D = c->D;
  const CdecPlan& P = D.cdec;
  hipStream_t st = (hipStream_t)stream;
  // tile products for the large fronts; everything on the FMA kernel on the generic / deterministic route
  const bool tiled = !use_generic(c) && use_large() && P.ntiles > 0;
  CdecArgs a;
  a.cl = D.cl; a.qptr = D.mrc.qptr; a.items = P.items; a.tiles = P.tiles; a.L = L; a.Z = Z;
  a.nitems = (int)P.nitems[tiled ? 0 : 1];
  if (a.nitems) launch(c, KID_syr2k_fma, k_cdec_fma, dim3((unsigned)((a.nitems + CDEC_WAVES - 1) / CDEC_WAVES)), dim3(64 * CDEC_WAVES), st, a);
  if (tiled) launch(c, KID_syr2k_mm, k_cdec_mm, dim3((unsigned)P.ntiles), dim3(256), st, a);
  HIPCHK(end_call(c));
  return 0;
}

int64_t csp_symm_positions(csp_ctx* c) {
  if (!c) return SMCP_EINVAL;
  if (c->D.symm.ntot < 0) c->D.symm.ntot = symm_items(c->S, nullptr);
  return c->D.symm.ntot;
}

int csp_symm(csp_ctx* c, const double* X, const double* B, int64_t ldb, double* C, int64_t ldc, int64_t nrhs, double alpha, double beta,
             void* stream) {
  if (int rc = ready(c)) return rc;
  const int mm = sw_int("SMCP_SYMM_MM", 1);       // read on every call: tools/symm_time.py alternates the settings in one process
  DeviceCtx& D = c->D;
  const SymmPlan& P = D.symm;
  const Symbolic& S = c->S;
  // (grid limits of the column-block dimension; a partitioned context holds valid panels on its own cliques only)
  if (nrhs < 1 || nrhs > ((int64_t)1 << 18) || ldb < S.n || ldc < S.n || c->xr_world > 1) return SMCP_EINVAL;
  {
    const uintptr_t b0 = (uintptr_t)B, b1 = (uintptr_t)(B + ldb * (nrhs - 1) + S.n);
    const uintptr_t c0 = (uintptr_t)C, c1 = (uintptr_t)(C + ldc * (nrhs - 1) + S.n);
    if (c0 < b1 && b0 < c1) return SMCP_EINVAL;   // phase 2 would write what phase 1 of a later column block still reads
  }
  if (int rc = symm_setup(c)) return rc;
  if (P.ntot * nrhs > D.max_rhs * D.tmplen) return SMCP_ENOMEM;
  hipStream_t st = (hipStream_t)stream;
  // tile products: the gates of csp_trmm, but SMCP_SYMM_MM=2 sends the large fronts there at any column count
  const Route route = product_route(c, mm, nrhs, 8, SYMM_MM_ALL, P.nitems[0] > 0, true);
  SymmArgs a;
  a.cl = D.cl; a.rowidx = D.rowidx; a.items = P.items; a.pos = P.idx.pos;
  a.X = X; a.B = B; a.U = D.tmp; a.ntot = P.ntot; a.nrhs = (int)nrhs; a.ldb = ldb;
  if (alpha != 0.0) {                             // alpha == 0: neither X nor B is read
    a.item0 = route == Route::tiles_large ? (int)P.nitems[0] : 0;
    a.nitems = route == Route::tiles_all ? 0 : (int)P.nitems[1] - a.item0;
    if (a.nitems)
      with_column_block(nrhs, [&](auto cb) {      // CB columns of B per wave: X is read once per block of CB columns
        constexpr int CB = decltype(cb)::value;
        const dim3 grid((unsigned)((a.nitems + SYMM_WAVES - 1) / SYMM_WAVES), (unsigned)((a.nrhs + CB - 1) / CB));
        launch(c, KID_symm_fma, k_symm_fma<CB>, grid, dim3(64 * SYMM_WAVES), st, a);
      });
    if (route != Route::fma) {
      a.item0 = 0;
      a.nitems = (int)P.nitems[route == Route::tiles_all ? 1 : 0];
      launch(c, KID_symm_mm, k_symm_mm, dim3((unsigned)a.nitems, (unsigned)tiles64((int)nrhs)), dim3(256), st, a);
    }
  }
  const int64_t nheavy = alpha != 0.0 ? P.idx.nheavy : 0;
  const CombineGrid g = combine_grid(D, S.n, nrhs, nheavy);
  launch(c, KID_symm_combine, k_symm_combine, dim3((unsigned)(g.light + g.heavy)), dim3(256), st, (const int64_t*)P.idx.tptr,
         (const int32_t*)P.idx.heavy, (int)nheavy, g.light, (const double*)D.tmp, a.ntot, C, S.n, (int)nrhs, ldc, alpha, beta);
  HIPCHK(end_call(c));
  return 0;
}

}  // extern "C"
