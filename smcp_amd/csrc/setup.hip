// Set-up and teardown of the device context (included by capi.hip): csp_device_init builds and uploads every tree-resident
// table as a sequence of named steps; csp_symbolic_destroy frees whatever the context's ledger (devmem.hpp) holds.

namespace {

bool fam_off() {
  static int off = -1;
  if (off < 0) { const char* e = sw_str("SMCP_FAM"); off = (e && e[0] == '0') ? 1 : 0; }
  return off == 1;
}
// dynamic LDS of the family kernel instantiation that serves (parent separator famna, child separator famcna)
size_t fam_bytes_for(int famna, int famcna, int fampan, int fampk) {
  const int nat = std::max(1, (famna + 15) / 16), natc = std::max(1, (famcna + 15) / 16);
  switch (nat * 2 + natc - 1) {
    case 2: return fam_lds_bytes<1, 1>(fampan, fampk);
    case 3: return fam_lds_bytes<1, 2>(fampan, fampk);
    case 4: return fam_lds_bytes<2, 1>(fampan, fampk);
    case 5: return fam_lds_bytes<2, 2>(fampan, fampk);
    case 6: return fam_lds_bytes<3, 1>(fampan, fampk);
    case 7: return fam_lds_bytes<3, 2>(fampan, fampk);
    case 8: return fam_lds_bytes<4, 1>(fampan, fampk);
    case 9: return fam_lds_bytes<4, 2>(fampan, fampk);
  }
  return (size_t)1 << 30;
}

// Splits the cliques selected by `keep` into per-level lists (LDS-class first -- its family tail last --, large
// fronts after) and records the sizing maxima of each class.  lev2 is the concatenation of the lists, off[l] its start.
template <class Keep>
void classify_levels(const Symbolic& S, Keep keep, std::vector<LevelClass>& lvl, std::vector<int32_t>& lev2,
                     std::vector<int64_t>& off) {
  lvl.assign(S.nlev, LevelClass());
  lev2.clear();
  off.assign(S.nlev + 1, 0);
  auto fits = [&](int64_t k) { return (size_t)mfma_lds_doubles((int)S.nn(k), (int)S.na(k)) * sizeof(double) <= LDS_LIMIT; };
  // pass 1: sizing of the LDS class of every level; the joint maxima may not fit even if every clique does: the
  // level's LDS class is demoted to the large-front class then
  std::vector<uint8_t> demoted(S.nlev, 0);
  for (int64_t l = 0; l < S.nlev; ++l) {
    int nnm = 0, nam = 0;
    bool any = false;
    for (int64_t q = S.levptr[l]; q < S.levptr[l + 1]; ++q) {
      const int64_t k = S.levidx[q];
      if (!keep(k) || !fits(k)) continue;
      any = true;
      nnm = std::max<int>(nnm, (int)S.nn(k));
      nam = std::max<int>(nam, (int)S.na(k));
    }
    if (any && (size_t)mfma_lds_doubles(nnm, nam) * sizeof(double) > LDS_LIMIT) demoted[l] = 1;
  }
  auto small = [&](int64_t k) { return fits(k) && !demoted[S.level[k]]; };
  // pass 2: families.  Parent: small front, nn <= 16, na <= 64, 1..8 children, every child kept, childless, small,
  // nn <= 16, na <= 32; all candidates of a level or none (one launch geometry per level).
  std::vector<uint8_t> special(S.nsn, 0);
  if (!fam_off())
    for (int64_t l = 1; l < S.nlev; ++l) {
      std::vector<int64_t> cand;
      int famna = 0, fampan = 0, fampk = 0, famcna = 0, famnn = 0, famcnn = 0;
      for (int64_t q = S.levptr[l]; q < S.levptr[l + 1]; ++q) {
        const int64_t k = S.levidx[q];
        if (!keep(k) || !small(k) || S.nn(k) > 16 || S.na(k) > 64) continue;
        const int64_t nch = S.chptr[k + 1] - S.chptr[k];
        if (nch < 1 || nch > 8) continue;
        bool ok = true;
        int cna = 0, cnn = 0;
        for (int64_t q2 = S.chptr[k]; q2 < S.chptr[k + 1] && ok; ++q2) {
          const int64_t ch = S.chidx[q2];
          ok = keep(ch) && S.chptr[ch + 1] == S.chptr[ch] && small(ch) && S.nn(ch) <= 16 && S.na(ch) <= 32 && S.na(ch) >= 1;
          cna = std::max<int>(cna, (int)S.na(ch));
          cnn = std::max<int>(cnn, (int)S.nn(ch));
        }
        if (!ok) continue;
        cand.push_back(k);
        famnn = std::max<int>(famnn, (int)S.nn(k));
        famcnn = std::max(famcnn, cnn);
        famna = std::max<int>(famna, (int)S.na(k));
        fampan = std::max<int>(fampan, (int)(S.nf(k) * S.nn(k)));
        fampk = std::max<int>(fampk, (int)(S.na(k) * (S.na(k) + 1) / 2));
        famcna = std::max(famcna, cna);
      }
      if (cand.empty() || fam_bytes_for(famna, famcna, fampan, fampk) > LDS_LIMIT) continue;
      LevelClass& L = lvl[l];
      L.famna = famna; L.fampan = fampan; L.fampk = fampk; L.famcna = famcna; L.famnn = famnn; L.famcnn = famcnn;
      for (int64_t k : cand) {
        special[k] = 1;
        for (int64_t q2 = S.chptr[k]; q2 < S.chptr[k + 1]; ++q2) special[S.chidx[q2]] = 1;
      }
    }
  // pass 3: the lists
  for (int64_t l = 0; l < S.nlev; ++l) {
    LevelClass& L = lvl[l];
    off[l] = (int64_t)lev2.size();
    int64_t b = S.levptr[l], e = S.levptr[l + 1];
    for (int pass = 0; pass < 3; ++pass)
      for (int64_t q = b; q < e; ++q) {
        int64_t k = S.levidx[q];
        if (!keep(k)) continue;
        const bool sm = small(k);
        const int cls = sm ? (special[k] ? 1 : 0) : 2;
        if (cls != pass) continue;
        lev2.push_back((int32_t)k);
        if (sm) {
          L.nI++;
          if (special[k]) L.nS++;
          L.nnmaxI = std::max<int>(L.nnmaxI, (int)S.nn(k));
          L.namaxI = std::max<int>(L.namaxI, (int)S.na(k));
          int64_t rs = 0;
          for (int64_t q2 = S.chptr[k]; q2 < S.chptr[k + 1]; ++q2) rs += S.na(S.chidx[q2]) * (S.na(S.chidx[q2]) + 1) / 2;
          L.plansumI = (int)std::max<int64_t>(L.plansumI, rs);
          L.nchmaxI = std::max<int>(L.nchmaxI, (int)(S.chptr[k + 1] - S.chptr[k]));
          L.panmaxI = std::max<int>(L.panmaxI, (int)(S.nf(k) * S.nn(k)));
          L.pkmaxI = std::max<int>(L.pkmaxI, (int)(S.na(k) * (S.na(k) + 1) / 2));
        } else {
          L.nII++;
          L.nnmaxII = std::max<int>(L.nnmaxII, (int)S.nn(k));
          L.nnminII = std::min<int>(L.nnminII, (int)S.nn(k));
          L.namaxII = std::max<int>(L.namaxII, (int)S.na(k));
          L.nchmaxII = std::max<int>(L.nchmaxII, (int)(S.chptr[k + 1] - S.chptr[k]));
        }
      }
  }
  off[S.nlev] = (int64_t)lev2.size();
}


// ---- the steps of csp_device_init, in call order.  InitTables: the host tables the steps hand to each other.
struct InitTables {
  std::vector<CliqueDesc> cl;
  std::vector<int32_t> lev2;          // classify_levels: per level LDS-class cliques, then large fronts
  std::vector<int32_t> lev3, large;   // all LDS-class cliques / all large fronts, by level
  int32_t nslots = 0;                 // large fronts (64 x 64 scratch slots in lfd; one more for the dense Cholesky)
};

// clique descriptors, per-clique scratch offsets, level classes, and what follows from them: family roles, the slots and the
// mask of the large fronts, the flat lists for clique-local kernels
void init_descriptors(csp_ctx* c, InitTables& T) {
  DeviceCtx& D = c->D;
  const Symbolic& S = c->S;
  T.cl.resize((size_t)S.nsn);
  for (int64_t k = 0; k < S.nsn; ++k) {
    CliqueDesc& d = T.cl[k];
    d.blk = S.blkptr[k];
    d.upd = S.updptr[k];
    d.updp = S.updpptr[k];
    d.rows = S.rowptr[k];
    d.rel = S.sepptr[k];
    d.nn = (int32_t)S.nn(k);
    d.na = (int32_t)S.na(k);
    d.parent = (int32_t)S.snpar[k];
    d.chbeg = (int32_t)S.chptr[k];
    d.chend = (int32_t)S.chptr[k + 1];
    d.first = (int32_t)S.snptr[k];
    d.pad = -1;
  }
  c->h_tmpptr.resize(S.nsn + 1);
  for (int64_t k = 0; k <= S.nsn; ++k) c->h_tmpptr[k] = 2 * S.blkptr[k] + 256 * k;
  D.tmplen = 2 * S.blklen() + 256 * S.nsn;
  std::vector<int64_t> lev2off;
  classify_levels(S, [](int64_t) { return true; }, c->lvl, T.lev2, lev2off);
  const std::vector<int32_t>& lev2 = T.lev2;
  c->lev_namax.assign(S.nlev, 0);
  c->fam.assign(S.nsn, 0);
  for (int64_t l = 0; l < S.nlev; ++l) {
    const LevelClass& L = c->lvl[l];
    int64_t b = S.levptr[l];
    for (int64_t q = L.nI - L.nS; q < L.nI; ++q) c->fam[lev2[b + q]] = l ? 2 : 1;
    for (int64_t q = 0; q < L.nI; ++q) T.lev3.push_back(lev2[b + q]);
    for (int64_t q = L.nI; q < L.nI + L.nII; ++q) { T.cl[lev2[b + q]].pad = T.nslots++; T.large.push_back(lev2[b + q]); }
    c->lev_namax[l] = std::max(L.namaxI, L.namaxII);
    if (L.nII) { D.nnmaxII_all = std::max(D.nnmaxII_all, L.nnmaxII); D.namaxII_all = std::max(D.namaxII_all, L.namaxII); }
  }
  c->large_mask.assign((size_t)S.nsn, 0);
  for (int32_t k : T.large) c->large_mask[(size_t)k] = 1;
  D.nI_total = (int64_t)T.lev3.size();
  D.nII_total = (int64_t)T.large.size();
}

// childless large fronts the sparse-input sweep can take (front_lfsp.hip)
int init_sparse_sweep(csp_ctx* c, const InitTables& T) {
  DeviceCtx& D = c->D;
  const Symbolic& S = c->S;
  std::vector<int32_t> sp;
  for (int32_t k : T.large)
    if (S.chptr[k + 1] == S.chptr[k] && S.nn(k) <= 64 && S.na(k) <= 128 && S.na(k) > 0) sp.push_back(k);
  D.lfsp_cnt = (int64_t)sp.size();
  D.lfsp_exact = !sp.empty();
  for (int32_t k : sp) if (S.nn(k) != 64 || S.na(k) != 128) D.lfsp_exact = false;
  return sp.empty() ? 0 : dev_upload(&D.lfsp_list, sp, D.mem);
}

// Sibling groups of the n cliques list[0 .. n) of one level: cliques under one LARGE parent with equal na and equal relative
// indices share a group, at most `cap` per group, in list order; every clique is in exactly one group (singletons included).
// glist: the groups as positions in the list, gptr: their starts.  Returns whether some group has more than one member.
bool sibling_groups(const csp_ctx* c, const int32_t* list, int64_t n, int cap, std::vector<int32_t>& gptr, std::vector<int32_t>& glist) {
  const Symbolic& S = c->S;
  gptr.assign(1, 0);
  glist.clear();
  std::vector<uint8_t> taken((size_t)n, 0);
  bool shared = false;
  // the members by parent, in list order: a clique is only ever compared with its own siblings
  std::unordered_map<int64_t, std::vector<int64_t>> sibs;
  for (int64_t q = 0; q < n; ++q) sibs[S.snpar[list[q]]].push_back(q);
  for (int64_t q = 0; q < n; ++q) {
    if (taken[(size_t)q]) continue;
    const int32_t k = list[q];
    taken[(size_t)q] = 1;
    glist.push_back((int32_t)q);
    int size = 1;
    const int64_t par = S.snpar[k];
    if (par >= 0 && c->large_mask[(size_t)par]) {
      const std::vector<int64_t>& sb = sibs[par];
      for (auto it = std::upper_bound(sb.begin(), sb.end(), q); it != sb.end() && size < cap; ++it) {
        const int64_t q2 = *it;
        const int32_t k2 = list[q2];
        if (taken[(size_t)q2] || S.na(k2) != S.na(k)) continue;
        if (!std::equal(S.relidx.begin() + S.sepptr[k], S.relidx.begin() + S.sepptr[k + 1], S.relidx.begin() + S.sepptr[k2])) continue;
        taken[(size_t)q2] = 1;
        glist.push_back((int32_t)q2);
        ++size;
      }
    }
    gptr.push_back((int32_t)glist.size());
    if (size > 1) shared = true;
  }
  return shared;
}

int init_sibling_groups(csp_ctx* c, const InitTables& T) {
  DeviceCtx& D = c->D;
  const Symbolic& S = c->S;
  const std::vector<int32_t>& lev2 = T.lev2;
  int rc = 0;
  std::vector<int32_t> gptr, glist;
  // sibling groups for the sparse-input sweep (front_lfsp.hip, k_lfsp_up<..., GRP>): members of a large-front class all
  // of whose fronts that sweep can take (childless, nn <= 64, 0 < na <= 128); at most eight per group; the lists hold
  // cliques.  SMCP_LFSP_GROUP=0: none.
  const char* ge = sw_str("SMCP_LFSP_GROUP");
  const bool gon = !(ge && ge[0] == '0');
  std::vector<uint8_t> skip((size_t)S.nsn, 0);
  c->lfsp_grp.assign((size_t)S.nlev, csp_ctx::LfspGroups());
  c->lfsp_any_groups = false;
  for (int64_t l = 0; l < S.nlev && gon; ++l) {
    const LevelClass& L = c->lvl[l];
    if (!L.nII || L.nchmaxII != 0 || L.nnmaxII > 64 || L.namaxII > 128) continue;
    const int32_t* list = lev2.data() + S.levptr[l] + L.nI;
    bool ok = true;
    for (int64_t q = 0; q < L.nII; ++q) ok = ok && S.na(list[q]) > 0;
    if (!ok || !sibling_groups(c, list, L.nII, 8, gptr, glist)) continue;
    for (int32_t& q : glist) q = list[q];
    // (the member that writes the summed update rotates with the group number; the others' slots stay unwritten)
    const int ng = (int)gptr.size() - 1;
    for (int g = 0; g < ng; ++g) {
      const int sz = gptr[(size_t)g + 1] - gptr[(size_t)g];
      for (int q = 0; q < sz; ++q)
        if (q != g % sz) skip[(size_t)glist[(size_t)gptr[(size_t)g] + q]] = 1;
    }
    csp_ctx::LfspGroups& G = c->lfsp_grp[(size_t)l];
    if ((rc = dev_upload(&G.ptr, gptr, D.mem))) return rc;
    if ((rc = dev_upload(&G.list, glist, D.mem))) return rc;
    G.ngroups = ng;
    c->lfsp_any_groups = true;
  }
  if (c->lfsp_any_groups && (rc = dev_upload(&D.lfsp_skip, skip, D.mem))) return rc;
  // sibling groups of FAMILY PARENTS for the entry-driven family sweep (front_famt.hip, k_fam_terms_grp): the family parents
  // of a level; at most FAMT_GMAX per group; the lists hold positions in the level's family list (= record indices of
  // k_famt_prep).  SMCP_FAMT_GROUP=0: none.
  const char* fe = sw_str("SMCP_FAMT_GROUP");
  const bool fon = !(fe && fe[0] == '0');
  std::vector<uint8_t> fskip((size_t)S.nsn, 0);
  c->famt_grp.assign((size_t)S.nlev, csp_ctx::LfspGroups());
  c->famt_any_groups = false;
  for (int64_t l = 1; l < S.nlev && fon; ++l) {
    const LevelClass& L = c->lvl[l];
    if (!L.nS) continue;
    const int nat = std::max(1, (L.famna + 15) / 16);
    if (nat > 4 || !famt_grp_fits(nat, std::max(1, L.famcnn))) continue;
    const int32_t* list = lev2.data() + S.levptr[l] + (L.nI - L.nS);
    if (!sibling_groups(c, list, L.nS, FAMT_GMAX, gptr, glist)) continue;
    // (a group's first member leads: the updates of the others are summed into its)
    for (size_t g = 0; g + 1 < gptr.size(); ++g)
      for (int32_t e = gptr[g] + 1; e < gptr[g + 1]; ++e) fskip[(size_t)list[glist[(size_t)e]]] = 1;
    csp_ctx::LfspGroups& G = c->famt_grp[(size_t)l];
    if ((rc = dev_upload(&G.ptr, gptr, D.mem))) return rc;
    if ((rc = dev_upload(&G.list, glist, D.mem))) return rc;
    G.ngroups = (int)gptr.size() - 1;
    c->famt_any_groups = true;
  }
  if (c->famt_any_groups) {
    if ((rc = dev_upload(&D.famt_skip, fskip, D.mem))) return rc;
    std::vector<uint8_t> both(fskip);
    if (c->lfsp_any_groups) for (size_t i = 0; i < both.size(); ++i) both[i] |= skip[i];
    if ((rc = dev_upload(&D.both_skip, both, D.mem))) return rc;
  }
  return 0;
}

// the flat clique list, the 64 x 64 slots of the large fronts, descriptors and index arrays
int init_index_uploads(csp_ctx* c, InitTables& T) {
  DeviceCtx& D = c->D;
  const Symbolic& S = c->S;
  int rc = 0;
  T.lev3.insert(T.lev3.end(), T.large.begin(), T.large.end());
  if ((rc = dev_upload(&D.lev3idx, T.lev3, D.mem))) return rc;
  D.lfd_len = (int64_t)(T.nslots + 1) * 64 * 64;
  if ((rc = dev_alloc(&D.lfd, D.lfd_len, D.mem))) return rc;
  D.lfd_dense = D.lfd + (int64_t)T.nslots * 64 * 64;
  std::vector<int32_t> ch(S.chidx.begin(), S.chidx.end()), lev(S.levidx.begin(), S.levidx.end());
  if ((rc = dev_upload(&D.cl, T.cl, D.mem))) return rc;
  if ((rc = dev_upload(&D.rowidx, S.rowidx, D.mem))) return rc;
  if ((rc = dev_upload(&D.relidx, S.relidx, D.mem))) return rc;
  if ((rc = dev_upload(&D.chidx, ch, D.mem))) return rc;
  if ((rc = dev_upload(&D.levidx, lev, D.mem))) return rc;
  return dev_upload(&D.lev2idx, T.lev2, D.mem);
}

}  // namespace

extern "C" {

// copies 1 .. K-1 of the extend-add gather plan of a K-fold replicated pattern: targets repeat, sources shift by the
// packed update length of one copy, the source ranges by the source count of one copy
__global__ void k_replicate_plan(int32_t* tgt, int64_t* cptr, int32_t* src, int64_t nt1, int64_t ns1, int64_t up1, int64_t K) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t e = g; e < nt1 * (K - 1); e += stride) {
    const int64_t t = 1 + e / nt1, q = e % nt1;
    tgt[t * nt1 + q] = tgt[q];
    cptr[t * nt1 + q + 1] = cptr[q + 1] + t * ns1;
  }
  for (int64_t e = g; e < ns1 * (K - 1); e += stride) {
    const int64_t t = 1 + e / ns1, q = e % ns1;
    src[t * ns1 + q] = (int32_t)(src[q] + t * up1);
  }
}

}  // extern "C"

namespace {

// gather plans for the extend-add
int init_gather_plan(csp_ctx* c, const InitTables& T, SetupClock& clk) {
  DeviceCtx& D = c->D;
  const Symbolic& S = c->S;
  const std::vector<CliqueDesc>& cl = T.cl;
  int rc = 0;
  if (S.updplen() < (int64_t)1 << 31) {
    std::vector<int64_t> tptr(S.nsn + 1, 0), cptr;
    std::vector<int32_t> tgt, src;
    const int64_t nsn1 = S.nsn / c->ntrial;       // a replicated pattern: plan of the first copy, shifted for the others
    // (target code, src offset) pairs of every clique with children, sorted per clique: the cliques are independent,
    // so host threads take them round-robin (5.5 M pairs on synth50k: 0.2 s of the set-up on one thread)
    std::vector<int64_t> par;
    for (int64_t k = 0; k < nsn1; ++k) if (S.chptr[k + 1] > S.chptr[k] || (cl[(size_t)k].pad >= 0 && S.na(k) > 0)) par.push_back(k);
    std::vector<std::vector<std::pair<int32_t, int32_t>>> prs(par.size());
    std::vector<int64_t> ntg(par.size(), 0);     // distinct targets per clique
    // Large fronts list EVERY position of the lower triangle of their update block as a target, with or without
    // contributions (marker pairs, dropped again when the sources are laid out): the plan kernels then assign the whole block
    // and the clear pass before them (k_lf_clear_upd: a 5 us launch in every chain over the top fronts) is not needed
    constexpr int32_t PLAN_MARK = INT32_MIN;
    std::vector<int64_t> nmark(par.size(), 0);
    {
      const int nth = host_threads(16, par.size() / 64 + 1);
      auto work = [&](int tix) {
        for (size_t x = (size_t)tix; x < par.size(); x += (size_t)nth) {
          const int64_t k = par[x];
          auto& pr = prs[x];
          const int64_t nnp = S.nn(k);
          size_t tot = 0;
          for (int64_t q = S.chptr[k]; q < S.chptr[k + 1]; ++q) { const int64_t nac = S.na(S.chidx[q]); tot += (size_t)(nac * (nac + 1) / 2); }
          pr.reserve(tot);
          for (int64_t q = S.chptr[k]; q < S.chptr[k + 1]; ++q) {
            const int64_t cc = S.chidx[q], nac = S.na(cc);
            const int32_t* rel = &S.relidx[S.sepptr[cc]];
            for (int64_t j = 0; j < nac; ++j)
              for (int64_t i = j; i < nac; ++i) {
                int32_t ri = rel[i], rj = rel[j];
                int32_t code = rj < nnp ? (ri | (rj << 15)) : ((1 << 30) | (ri - (int32_t)nnp) | ((rj - (int32_t)nnp) << 15));
                pr.emplace_back(code, (int32_t)(S.updpptr[cc] + j * nac - j * (j - 1) / 2 + (i - j)));
              }
          }
          if (cl[(size_t)k].pad >= 0) {
            const int64_t nak = S.na(k);
            for (int64_t j = 0; j < nak; ++j)
              for (int64_t i = j; i < nak; ++i) pr.emplace_back((int32_t)((1 << 30) | (int32_t)i | ((int32_t)j << 15)), PLAN_MARK);
            nmark[x] = nak * (nak + 1) / 2;
          }
          std::sort(pr.begin(), pr.end());
          int64_t nd = 0;
          for (size_t e = 0; e < pr.size(); ++e) if (e == 0 || pr[e].first != pr[e - 1].first) ++nd;
          ntg[x] = nd;
        }
      };
      run_threads(nth, work);
    }
    clk.mark("plan: sorted pairs");
    // targets (distinct codes) per clique were counted by the workers: the serial part only lays the pieces out
    std::vector<int64_t> tbase(par.size() + 1, 0), sbase(par.size() + 1, 0);
    for (size_t x = 0; x < par.size(); ++x) { tbase[x + 1] = tbase[x] + ntg[x]; sbase[x + 1] = sbase[x] + (int64_t)prs[x].size() - nmark[x]; }
    const int64_t nt1 = tbase[par.size()], ns1 = sbase[par.size()];
    tgt.resize((size_t)nt1);
    src.resize((size_t)ns1);
    cptr.assign((size_t)nt1 + 1, 0);
    {
      const int nth2 = (int)std::max<int64_t>(1, std::min<int64_t>(16, (int64_t)par.size() / 64 + 1));
      auto fill = [&](int tix) {
        for (size_t x = (size_t)tix; x < par.size(); x += (size_t)nth2) {
          const auto& pr = prs[x];
          int64_t tq = tbase[x];
          const int64_t s0 = sbase[x];
          int64_t w = 0;
          for (size_t e = 0; e < pr.size(); ++e) {
            if (e == 0 || pr[e].first != pr[e - 1].first) { tgt[(size_t)tq] = pr[e].first; cptr[(size_t)tq] = s0 + w; ++tq; }
            if (pr[e].second != PLAN_MARK) src[(size_t)(s0 + w++)] = pr[e].second;
          }
        }
      };
      run_threads(nth2, fill);
    }
    cptr[(size_t)nt1] = ns1;
    {
      size_t x = 0;
      for (int64_t k = 0; k < nsn1; ++k) {
        if (x < par.size() && par[x] == k) ++x;
        tptr[k + 1] = tbase[x];
      }
    }
    prs.clear();
    clk.mark("plan: merge");
    if (c->ntrial > 1) {
      // a replicated pattern: the copies' plans are the first one shifted -- laid out on the device by one kernel
      // (K = 8 on synth50k: 44 M indices; building them on the host and uploading 176 MB took 0.12 s)
      const int64_t K = c->ntrial, up1 = S.updplen() / K;
      for (int64_t t = 1; t < K; ++t)
        for (int64_t k = 0; k < nsn1; ++k) tptr[t * nsn1 + k + 1] = tptr[k + 1] + t * nt1;
      if ((rc = dev_upload(&D.gp_tptr, tptr, D.mem))) return rc;
      if ((rc = dev_alloc(&D.gp_tgt, nt1 * K, D.mem))) return rc;
      if ((rc = dev_alloc(&D.gp_cptr, nt1 * K + 1, D.mem))) return rc;
      if ((rc = dev_alloc(&D.gp_src, ns1 * K, D.mem))) return rc;
      if (nt1) HIPCHK(hipMemcpy(D.gp_tgt, tgt.data(), sizeof(int32_t) * nt1, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(D.gp_cptr, cptr.data(), sizeof(int64_t) * (nt1 + 1), hipMemcpyHostToDevice));
      if (ns1) HIPCHK(hipMemcpy(D.gp_src, src.data(), sizeof(int32_t) * ns1, hipMemcpyHostToDevice));
      c->census.note((const void*)k_replicate_plan);
      hipLaunchKernelGGL(k_replicate_plan, dim3(2048), dim3(256), 0, 0, D.gp_tgt, D.gp_cptr, D.gp_src, nt1, ns1, up1, K);
      HIPCHK(hipGetLastError());
      HIPCHK(hipDeviceSynchronize());
      clk.mark("plan: replicate (device)");
    } else {
      if ((rc = dev_upload(&D.gp_tptr, tptr, D.mem))) return rc;
      if ((rc = dev_upload(&D.gp_tgt, tgt, D.mem))) return rc;
      if ((rc = dev_upload(&D.gp_cptr, cptr, D.mem))) return rc;
      if ((rc = dev_upload(&D.gp_src, src, D.mem))) return rc;
    }
  }
  c->plan_full_upd = true;
  clk.mark("plan: upload");
  return 0;
}

// dynamic LDS beyond 64 KB for the kernels of the sweeps.  Function attributes are per process (one device per process): set once
int init_kernel_attributes() {
  static bool attrs_done = false;
  if (attrs_done) return 0;
  attrs_done = true;
  const int mx = 160 * 1024 - 1024;
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_up_mfma<true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_up_pad, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_up_n16<1, false>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_up_n16<1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_up_n16<2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_up_n16<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_up_n16<3, false>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_up_n16<3, true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_up_n16<4, false>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_up_n16<4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_partial<true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_partial<false>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<1, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<2, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<3, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<1, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<1, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<2, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<2, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<3, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<3, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<4, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<4, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<5, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<5, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<6, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<7, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<8, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_gram_diag128<9, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_lf_diag, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_factor_yaa_lds, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_down_mfma<true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_down_mfma<true, WK_DOWN0>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_chol_mfma<true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_chol_mfma<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_pinv_mfma<true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_down_inv_mfma<true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_hess_up_inv_mfma<true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_llt_mfma<true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  HIPCHK(hipFuncSetAttribute((const void*)k_completion_mfma<true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx));
  return 0;
}

// caches of what is derived from the factors (lk, yaa, fac, faci), the weights, reduction scratch and the failure flags
int init_caches(csp_ctx* c) {
  DeviceCtx& D = c->D;
  const Symbolic& S = c->S;
  int rc = 0;
  if ((rc = dev_alloc(&D.lk, S.blklen(), D.mem))) return rc;
  HIPCHK(hipMemset(D.lk, 0, sizeof(double) * std::max<int64_t>(S.blklen(), 1)));
  if ((rc = dev_upload(&D.tmpptr, c->h_tmpptr, D.mem))) return rc;
  if ((rc = dev_alloc(&D.yaa, S.updlen(), D.mem))) return rc;
  if ((rc = dev_alloc(&D.fac, S.updlen(), D.mem))) return rc;
  HIPCHK(hipMemset(D.fac, 0, sizeof(double) * std::max<int64_t>(S.updlen(), 1)));     // strict upper triangles stay zero (prepare_yaa)
  if ((rc = dev_alloc(&D.sw, S.blklen(), D.mem))) return rc;
  c->census.note((const void*)k_fill_sqrt_weights);
  hipLaunchKernelGGL(k_fill_sqrt_weights, dim3((unsigned)std::min<int64_t>(S.nsn, 4096)), dim3(256), 0, 0, D.cl, (int)S.nsn, D.sw);
  if ((rc = dev_alloc(&D.faci, S.updlen(), D.mem))) return rc;
  if ((rc = dev_alloc(&D.red, 4096, D.mem))) return rc;      // [0, 1024): reduction scratch, [1024, 4096): shares of a split Amap (kkt_solve)
  if ((rc = dev_alloc(&D.info, 32, D.mem))) return rc;      // [0, 16): failure flags of the copies; [16]: status latch
  HIPCHK(hipMemset(D.info, 0, sizeof(int) * 32));
  // pinned mirror: ints [0, 16) the trial flags (csp_trial_flags), [16] the status latch (csp_status), bytes [96, 104) the
  // scalar of the reductions (csp_dot / csp_logdiagsum): separate slots, so that no call overwrites another's result
  HIPCHK(hipHostMalloc((void**)&D.info_host, 128));
  return 0;
}

// update matrices, packed exchange buffer and per-clique scratch for max_rhs right-hand sides (replacing smaller ones)
int init_rhs_workspaces(csp_ctx* c, int64_t max_rhs) {
  DeviceCtx& D = c->D;
  const Symbolic& S = c->S;
  int rc = 0;
  D.RhsWorkspaces::release(D.mem);
  if ((rc = dev_alloc(&D.upd, max_rhs * S.updlen(), D.mem))) return rc;
  { const char* e = sw_str("SMCP_UPDP_PAD"); D.updp_stride = S.updplen() + (e ? std::max(0, atoi(e)) : 0); }
  if ((rc = dev_alloc(&D.updp, max_rhs * D.updp_stride, D.mem))) return rc;
  if ((rc = dev_alloc(&D.tmp, max_rhs * D.tmplen, D.mem))) return rc;
  D.max_rhs = max_rhs;
  return 0;
}

}  // namespace

extern "C" {

int csp_device_init(csp_ctx* c, int device, int64_t max_rhs) {
  if (!c || max_rhs < 1) return SMCP_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return SMCP_ENODEV;
  if (device < 0 || device >= ndev) return SMCP_EINVAL;
  DeviceCtx& D = c->D;
  if (D.device == device && D.max_rhs >= max_rhs) return 0;
  // One process drives one GPU (one rank per GPU under torch.distributed): the launch helpers cache function
  // attributes, occupancy and the CU count per process, and a context's buffers live on the device it was
  // first initialised on.  A second device -- for this context or for another one of this process -- is refused.
  static int bound_device = -1;
  if (D.device >= 0 && D.device != device) return SMCP_EINVAL;
  if (bound_device >= 0 && bound_device != device) return SMCP_EINVAL;
  bound_device = device;
  HIPCHK(hipSetDevice(device));
  SetupClock clk("csp_device_init");
  int rc = 0;
  if (D.device < 0) {
    InitTables T;
    init_descriptors(c, T);
    if ((rc = init_sparse_sweep(c, T))) return rc;
    if ((rc = init_sibling_groups(c, T))) return rc;
    if ((rc = init_index_uploads(c, T))) return rc;
    clk.mark("descriptors + uploads");
    if ((rc = init_gather_plan(c, T, clk))) return rc;
    if ((rc = init_kernel_attributes())) return rc;
    if ((rc = init_caches(c))) return rc;
    clk.mark("attributes + buffers");
    { hipDeviceProp_t p; D.ncu = (hipGetDeviceProperties(&p, device) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256; }
    D.device = device;
  }
  if ((rc = init_rhs_workspaces(c, max_rhs))) return rc;
  clk.mark("per-rhs workspaces");
  return 0;
}

void csp_symbolic_destroy(csp_ctx* c) {
  if (!c) return;
  DeviceCtx& D = c->D;
  if (D.device >= 0) {
    hipSetDevice(D.device);
    if (c->side_fork) { Fork* f = (Fork*)c->side_fork; c->side_fork = nullptr; f->join(); delete f; }
    for (int q = 0; q < 2; ++q) {
      if (c->aux_stream[q]) { (void)hipStreamSynchronize(c->aux_stream[q]); (void)hipStreamDestroy(c->aux_stream[q]); }
      if (c->aux_join[q]) (void)hipEventDestroy(c->aux_join[q]);
    }
    if (c->aux_fork) (void)hipEventDestroy(c->aux_fork);
    for (hipEvent_t e : c->prof.ev) (void)hipEventDestroy(e);
    dev_free_all(D.mem);
    if (D.info_host) hipHostFree(D.info_host);
  }
  delete c;
}

}  // extern "C"
