// Host tables of a constraint set (constraints.hpp): six steps, each a function below, run in order by
// build_constraint_tables.  Steps that split their work over host threads write disjoint index ranges of shared vectors and
// lay the pieces out serially, so the tables are the same for every thread count.
#include "constraints.hpp"

#include <algorithm>
#include <atomic>

#include "../../include/smcp_amd.h"
#include "hostpar.hpp"

namespace smcp {
namespace {

// what the steps share: the input, the tables, and per entry its clique and its position inside that clique's panel
struct Build {
  const Symbolic& S;
  const ConstraintParams& P;
  const int64_t m, nnz;
  const int64_t* cptr;
  const int64_t* cidx;
  const double* cval;
  ConstraintTables& T;
  std::vector<int32_t> ek, eoff;
  int threads = 1;               // host threads of the step that ran last
};

// 1. locate entries: clique by binary search on blkptr (the entry ranges split over host threads), matrix coordinates,
// Amap weights.  False for a position outside blkval or in the strict upper triangle of an NN block.
bool locate_entries(Build& B) {
  const Symbolic& S = B.S;
  ConstraintTables& T = B.T;
  const int64_t nnz = B.nnz;
  const int64_t* cidx = B.cidx;
  const double* cval = B.cval;
  T.w.resize(nnz); T.ar.resize(nnz); T.ac.resize(nnz);
  B.ek.resize(nnz); B.eoff.resize(nnz);
  const int nth = B.threads = host_threads(B.P.max_threads, nnz / 65536 + 1);
  std::atomic<int> bad{0};
  auto work = [&](int tix) {
    const int64_t e0 = nnz * tix / nth, e1 = nnz * (tix + 1) / nth;
    int64_t k = 0;
    for (int64_t e = e0; e < e1; ++e) {
      int64_t pos = cidx[e];
      if (pos < 0 || pos >= S.blklen()) { bad = 1; return; }
      if (pos < S.blkptr[k] || pos >= S.blkptr[k + 1])      // (runs of entries share their clique)
        k = (int64_t)(std::upper_bound(S.blkptr.begin(), S.blkptr.end(), pos) - S.blkptr.begin()) - 1;
      int64_t nf = S.nf(k), off = pos - S.blkptr[k];
      int64_t col = off / nf, row = off % nf;
      if (row < col) { bad = 1; return; }  // upper triangle of the NN block is not part of V
      T.w[e] = (row == col) ? cval[e] : 2.0 * cval[e];
      T.ar[e] = (int32_t)S.rowidx[S.rowptr[k] + row];
      T.ac[e] = (int32_t)(S.snptr[k] + col);
      B.ek[e] = (int32_t)k;
      B.eoff[e] = (int32_t)off;
    }
  };
  run_threads(nth, work);
  return !bad;
}

// 2. classify columns.  Column-sparse constraints (misc.nzcolumns / misc.matperm, misc.c:682-773, solvers.py:246-268): a
// constraint whose entries touch at most int(n * tnzcols) distinct rows/columns takes the SCMcolumn2 path (two sparse
// triangular solves for S^-1[:, K_s], then pairwise contractions) instead of a Hessian sweep.
void classify_columns(Build& B) {
  const Symbolic& S = B.S;
  const ConstraintParams& P = B.P;
  ConstraintTables& T = B.T;
  const int64_t m = B.m, nnz = B.nnz;
  const int64_t* cptr = B.cptr;
  T.rloc.assign(nnz, 0); T.cloc.assign(nnz, 0);
  T.h_kptr.assign(1, 0);
  const int64_t tnz = (int64_t)((double)S.n * P.tnzcols);
  // at most this many columns of S^-1 are formed per constraint (n x |K| doubles of workspace)
  const int64_t colcap = ((int64_t)256 << 20) / std::max<int64_t>(1, S.n * 8);
  const int64_t kcap = std::min<int64_t>(tnz, std::max<int64_t>(1, colcap));
  const int64_t sepsum = std::max<int64_t>(1, S.sepptr[S.nsn]);
  const int64_t trsm_cap = std::max<int64_t>(1, (P.max_rhs * P.tmplen) / sepsum);
  // the distinct rows / columns of every constraint: independent per constraint, host threads take them round-robin
  // (synth50k: 100 sorts of 23 k indices, 65 ms on one thread); the lists are then joined in constraint order
  std::vector<std::vector<int32_t>> kss((size_t)m);
  std::vector<char> is_sparse((size_t)m, 0);
  const int64_t cap = std::min(kcap, trsm_cap);
  const int nth = B.threads = host_threads(P.max_threads, m, nnz / 4096 + 1);
  auto work = [&](int tix) {
    for (int64_t j = tix; j < m; j += nth) {
      std::vector<int32_t>& ks = kss[(size_t)j];
      ks.reserve((size_t)(2 * (cptr[j + 1] - cptr[j])));
      for (int64_t e = cptr[j]; e < cptr[j + 1]; ++e) { ks.push_back(T.ar[e]); ks.push_back(T.ac[e]); }
      std::sort(ks.begin(), ks.end());
      ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
      const int64_t nz = (int64_t)ks.size();
      const bool sparse = P.scm_on && nz > 0 && nz <= cap;
      is_sparse[(size_t)j] = sparse ? 1 : 0;
      if (!sparse) { std::vector<int32_t>().swap(ks); continue; }
      for (int64_t e = cptr[j]; e < cptr[j + 1]; ++e) {
        T.rloc[e] = (int32_t)(std::lower_bound(ks.begin(), ks.end(), T.ar[e]) - ks.begin());
        T.cloc[e] = (int32_t)(std::lower_bound(ks.begin(), ks.end(), T.ac[e]) - ks.begin());
      }
    }
  };
  run_threads(nth, work);
  int64_t kmax = 1;
  for (int64_t j = 0; j < m; ++j) {
    if (!is_sparse[(size_t)j]) { T.dl.push_back((int32_t)j); continue; }
    T.sl.push_back((int32_t)j);
    T.kidx.insert(T.kidx.end(), kss[(size_t)j].begin(), kss[(size_t)j].end());
    T.h_kptr.push_back((int64_t)T.kidx.size());
    kmax = std::max(kmax, (int64_t)kss[(size_t)j].size());
  }
  if (!T.sl.empty()) T.vcols = std::min(trsm_cap, std::max(kmax, std::min<int64_t>((int64_t)T.kidx.size(), colcap)));
}

// 3. CSR by position.  Entries ordered by position, ties in constraint order: a counting sort over the positions of V (a
// comparison sort of the 1.1 M entries of synth50k took 74 ms), split by position range over host threads: every thread
// walks the entry list for the positions of its range (counts, then places), so the pieces come out in global order and
// only their offsets are laid out serially.
void csr_by_position(Build& B) {
  ConstraintTables& T = B.T;
  const int64_t m = B.m, nnz = B.nnz;
  const int64_t* cptr = B.cptr;
  const int64_t* cidx = B.cidx;
  const double* cval = B.cval;
  T.rcon.resize(nnz); T.rval.resize(nnz);
  std::vector<int32_t> con(nnz);
  for (int64_t j = 0; j < m; ++j)
    for (int64_t e = cptr[j]; e < cptr[j + 1]; ++e) con[e] = (int32_t)j;
  const int nth = B.threads = host_threads(B.P.max_threads, nnz / 65536 + 1);
  const int64_t P = B.S.blklen();
  std::vector<std::vector<int64_t>> start((size_t)nth);          // per thread: first slot of every position of its range
  std::vector<int64_t> ecount((size_t)nth + 1, 0), dcount((size_t)nth + 1, 0);
  auto count = [&](int tix) {
    const int64_t p0 = P * tix / nth, p1 = P * (tix + 1) / nth;
    std::vector<int64_t>& st = start[(size_t)tix];
    st.assign((size_t)(p1 - p0) + 1, 0);
    for (int64_t e = 0; e < nnz; ++e) { const int64_t p = cidx[e]; if (p >= p0 && p < p1) ++st[(size_t)(p - p0) + 1]; }
    int64_t distinct = 0;
    for (int64_t p = 0; p < p1 - p0; ++p) { distinct += st[(size_t)p + 1] != 0; st[(size_t)p + 1] += st[(size_t)p]; }
    ecount[(size_t)tix + 1] = st[(size_t)(p1 - p0)];
    dcount[(size_t)tix + 1] = distinct;
  };
  run_threads(nth, count);
  for (int t = 0; t < nth; ++t) { ecount[(size_t)t + 1] += ecount[(size_t)t]; dcount[(size_t)t + 1] += dcount[(size_t)t]; }
  T.rpos.resize((size_t)dcount[(size_t)nth]);
  T.rptr.resize((size_t)dcount[(size_t)nth] + 1);
  auto place = [&](int tix) {
    const int64_t p0 = P * tix / nth, p1 = P * (tix + 1) / nth, q0 = ecount[(size_t)tix];
    std::vector<int64_t>& st = start[(size_t)tix];
    int64_t d = dcount[(size_t)tix];
    for (int64_t p = 0; p < p1 - p0; ++p)
      if (st[(size_t)p + 1] != st[(size_t)p]) { T.rpos[(size_t)d] = p0 + p; T.rptr[(size_t)d] = q0 + st[(size_t)p]; ++d; }
    for (int64_t e = 0; e < nnz; ++e) {                          // e ascending: ties stay in constraint order
      const int64_t p = cidx[e];
      if (p < p0 || p >= p1) continue;
      const int64_t q = q0 + st[(size_t)(p - p0)]++;
      T.rcon[(size_t)q] = con[e];
      T.rval[(size_t)q] = cval[e];
    }
  };
  run_threads(nth, place);
  T.rptr[(size_t)dcount[(size_t)nth]] = nnz;
}

// 4a. entries grouped by (clique, constraint): the sweeps of the Schur complement build their input panels from these.
// kptr[k * (m + 1) + j] is the first entry of constraint j in clique k; slot (k, m) doubles as the start of clique k + 1.
void group_entries(Build& B) {
  const Symbolic& S = B.S;
  ConstraintTables& T = B.T;
  const int64_t m = B.m, nnz = B.nnz;
  const int64_t* cptr = B.cptr;
  const std::vector<int32_t>& ek = B.ek;
  const std::vector<int32_t>& eoff = B.eoff;
  std::vector<int32_t>& kptr = T.kptr;
  kptr.assign((size_t)(S.nsn * (m + 1)) + 1, 0);
  T.koff.resize(nnz); T.kval.resize(nnz); T.kij.resize(nnz);
  // (a slot belongs to one constraint: counting and filling run over the constraints on host threads)
  const int nth = B.threads = host_threads(B.P.max_threads, m, nnz / 65536 + 1);
  auto over_constraints = [&](auto body) {
    run_threads(nth, [&](int tix) { for (int64_t j = tix; j < m; j += nth) body(j); });
  };
  over_constraints([&](int64_t j) {
    for (int64_t e = cptr[j]; e < cptr[j + 1]; ++e) kptr[(size_t)ek[e] * (m + 1) + j + 1]++;
  });
  // exclusive scan over (clique, constraint)
  int64_t run = 0;
  for (int64_t k = 0; k < S.nsn; ++k) {
    for (int64_t j = 0; j <= m; ++j) {
      const size_t idx = (size_t)k * (m + 1) + j;
      const int32_t cnt = (j < m) ? kptr[idx + 1] : 0;
      kptr[idx] = (int32_t)run;
      if (j < m) run += cnt;
    }
  }
  // positions inside the panel, and the same as (row | column << 16), for k_fam_sparse (its members have < 2^16 rows)
  std::vector<int32_t> fill(kptr.begin(), kptr.end() - 1);
  over_constraints([&](int64_t j) {
    for (int64_t e = cptr[j]; e < cptr[j + 1]; ++e) {
      const int64_t nf = S.nf(ek[e]);
      const int32_t q = fill[(size_t)ek[e] * (m + 1) + j]++;
      T.koff[q] = eoff[e];
      T.kval[q] = B.cval[e];
      T.kij[q] = (int32_t)((eoff[e] % nf) & 0xffff) | (int32_t)((eoff[e] / nf) << 16);
    }
  });
  kptr.pop_back();
  T.kc_sorted = true;           // (CCS columns with ascending rows give ascending panel positions per clique)
  for (size_t q = 0; q + 1 < kptr.size() && T.kc_sorted; ++q)
    for (int32_t e = kptr[q] + 1; e < kptr[q + 1]; ++e)
      if (T.koff[(size_t)e] <= T.koff[(size_t)e - 1]) { T.kc_sorted = false; break; }
}

// 4b. what the routes of the Schur sweeps decide on: list lengths per class of front, and the family children
void entry_statistics(Build& B) {
  const Symbolic& S = B.S;
  ConstraintTables& T = B.T;
  const int64_t m = B.m;
  const std::vector<int64_t>& fam = *B.P.fam;
  auto len = [&](int64_t k, int64_t j) { const size_t q = (size_t)k * (m + 1) + j; return (int64_t)(T.kptr[q + 1] - T.kptr[q]); };
  T.kc_maxlist = 0;             // over the cliques that can be members of a family (nn <= 16, na <= 64)
  for (int64_t k = 0; k < S.nsn; ++k)
    if (S.nn(k) <= 16 && S.na(k) <= 64)
      for (int64_t j = 0; j < m; ++j) T.kc_maxlist = std::max(T.kc_maxlist, len(k, j));
  // most entries of a (family, constraint) pair: the parent's own + its children's (the entry-driven family sweep of
  // front_famt.hip turns every entry into one term of a rank-T product)
  int64_t sum = 0, pairs = 0;
  for (int64_t k = 0; k < S.nsn; ++k)
    if (k < (int64_t)fam.size() && fam[k] == 2)
      for (int64_t j = 0; j < m; ++j) {
        int64_t tot = len(k, j);
        for (int64_t q2 = S.chptr[k]; q2 < S.chptr[k + 1]; ++q2) tot += len(S.chidx[q2], j);
        T.fam_maxterms = std::max(T.fam_maxterms, tot);
        sum += tot;
        ++pairs;
      }
  if (pairs) T.fam_meanterms = (double)sum / (double)pairs;
  T.kc_maxlist_large = 0;       // over the childless fronts beyond the small classes (sparse-input sweep of large fronts)
  for (int64_t k = 0; k < S.nsn; ++k)
    if ((S.nn(k) > 16 || S.na(k) > 64) && S.nn(k) <= 64 && S.na(k) <= 128 && S.chptr[k + 1] == S.chptr[k])
      for (int64_t j = 0; j < m; ++j) T.kc_maxlist_large = std::max(T.kc_maxlist_large, len(k, j));
  // closed-form Gram blocks of the family children (front_leafgram.hip): their slots, entry counts over all constraints,
  // and the record size of the per-step tables
  T.lg_slot_of.assign((size_t)S.nsn, -1);
  T.lg_eptr.assign(1, 0);
  for (int64_t k = 0; k < S.nsn; ++k)
    if (k < (int64_t)fam.size() && fam[k] == 1) {
      const int64_t E = T.kptr[(size_t)k * (m + 1) + m] - T.kptr[(size_t)k * (m + 1)];
      T.lg_slot_of[(size_t)k] = (int32_t)T.lg_children++;
      T.lg_maxent = std::max(T.lg_maxent, E);
      T.lg_pairs += E * (E + 1) / 2;
      T.lg_rows += S.nf(k) * S.nn(k);
      T.lg_rec = std::max<int>(T.lg_rec, (int)(S.nf(k) * S.nf(k) + S.nf(k) * S.nn(k)));
      T.lg_eptr.push_back(T.lg_eptr.back() + (int32_t)E);
    }
}

// 5. leaf-Gram lists: per family child its entries over all constraints in constraint order (row | column << 8 |
// constraint << 16, value halved on the diagonal) -- static, so the pair kernel reads them with one coalesced load -- and
// the place of every swept constraint in the dense list
void leafgram_lists(Build& B) {
  ConstraintTables& T = B.T;
  const int64_t m = B.m;
  T.epk.resize((size_t)T.lg_eptr.back());
  T.ewv.resize((size_t)T.lg_eptr.back());
  T.remap.assign((size_t)m, -1);
  for (int64_t k = 0; k < B.S.nsn; ++k) {
    const int32_t g = T.lg_slot_of[(size_t)k];
    if (g < 0) continue;
    int32_t o = T.lg_eptr[(size_t)g];
    for (int64_t j = 0; j < m; ++j)
      for (int32_t q = T.kptr[(size_t)k * (m + 1) + j]; q < T.kptr[(size_t)k * (m + 1) + j + 1]; ++q, ++o) {
        const int32_t i = T.kij[q] & 0xffff, jc = T.kij[q] >> 16;
        T.epk[(size_t)o] = i | (jc << 8) | ((int32_t)j << 16);
        T.ewv[(size_t)o] = i == jc ? 0.5 * T.kval[q] : T.kval[q];
      }
  }
  for (size_t q = 0; q < T.dl.size(); ++q) T.remap[(size_t)T.dl[q]] = (int32_t)q;
  T.has_leafgram = true;
}

// 6a. number the family parents and mark the levels of their parent fronts.  False unless every family parent hangs under a
// large front whose packed triangle fits LDS, and the counts fit the int32 tables.
bool number_families(Build& B) {
  const Symbolic& S = B.S;
  const ConstraintParams& P = B.P;
  ConstraintTables& T = B.T;
  T.fno.assign((size_t)S.nsn, -1);
  T.fz_levels.assign((size_t)S.nlev, 0);
  T.has_fz_levels = true;
  int64_t nfam = 0;
  bool ok = true;
  for (int64_t k = 0; k < S.nsn; ++k)
    if ((*P.fam)[(size_t)k] == 2) {
      T.fno[(size_t)k] = (int32_t)nfam++;
      const int64_t par = S.snpar[k];
      if (par < 0 || (size_t)par >= P.large_mask->size() || !(*P.large_mask)[(size_t)par] || S.nf(par) > P.lf_alds_maxnf) ok = false;
      else T.fz_levels[(size_t)S.level[(size_t)par]] = 1;
    }
  T.fz_nfam = nfam;
  return ok && nfam > 0 && nfam < ((int64_t)1 << 19) && nfam * (B.m + 1) < ((int64_t)1 << 31);
}

// 6b. family term lists (fused extend-add, front_famt.hip lf_add_family): every entry of constraint j inside family f -- the
// parent's own, then its children's in chidx order -- as (vector ids vx | vy << 16, scale), the mapping k_fam_terms does per
// launch from the entry lists (front_famt.hip, header): own entry v at (i, j): e_i, e_j, v (v / 2 on the diagonal); child
// entry at (separator row a, column j): q~_{c,j}, e_{rel_c[a]}, -v; child entry at (i, j) of its supernode block: q~_{c,i},
// q~_{c,j}, v (v / 2).  Sizes first, then the lists themselves, the families spread over host threads.
// A term with exactly one unit vector of the parent's separator part (id < famt_child and >= nn of the parent: an own entry in a
// separator row, a child's separator-row entry whose row lands there) is a UNIT term: a(e_i) is a unit vector, so the term adds
// s a(d) to one row and column of the update and needs no matrix product.  Every list holds its dense terms first, then its
// unit terms, each class in the entry order above; a unit term carries FAM_UNIT_TERM, its dense vector in the low half and
// its unit vector in the high half (ids are below 256).  The same constant is FAMT_UNIT of front_famt.hip.
constexpr int32_t FAM_UNIT_TERM = 1 << 30;
void family_term_lists(Build& B) {
  const Symbolic& S = B.S;
  ConstraintTables& T = B.T;
  const int64_t m = B.m, nfam = T.fz_nfam;
  const int32_t CHILD = B.P.famt_child;
  const std::vector<int32_t>& kptr = T.kptr;
  const std::vector<int32_t>& kij = T.kij;
  const std::vector<double>& kval = T.kval;
  std::vector<int32_t>& fptr = T.fptr;
  fptr.assign((size_t)(nfam * (m + 1)) + 1, 0);
  std::vector<int64_t> fam_k((size_t)nfam);
  int64_t run = 0;
  for (int64_t k = 0; k < S.nsn; ++k) {
    const int32_t f = T.fno[(size_t)k];
    if (f < 0) continue;
    fam_k[(size_t)f] = k;
    for (int64_t j = 0; j < m; ++j) {
      fptr[(size_t)f * (m + 1) + j] = (int32_t)run;
      run += kptr[(size_t)k * (m + 1) + j + 1] - kptr[(size_t)k * (m + 1) + j];
      for (int64_t q2 = S.chptr[k]; q2 < S.chptr[k + 1]; ++q2) {
        const size_t q = (size_t)S.chidx[q2] * (m + 1) + j;
        run += kptr[q + 1] - kptr[q];
      }
    }
    fptr[(size_t)f * (m + 1) + m] = (int32_t)run;
  }
  fptr[(size_t)(nfam * (m + 1))] = (int32_t)run;
  T.fpk.resize((size_t)run);
  T.fsv.resize((size_t)run);
  const int nth = B.threads = host_threads(B.P.max_threads, nfam / 16 + 1);
  run_threads(nth, [&](int tix) {
    std::vector<int32_t> upk;          // the unit terms of the list being written, in entry order
    std::vector<double> usv;
    for (int64_t f = tix; f < nfam; f += nth) {
      const int64_t k = fam_k[(size_t)f];
      const int32_t nnp = (int32_t)S.nn(k);
      for (int64_t j = 0; j < m; ++j) {
        size_t o = (size_t)fptr[(size_t)f * (m + 1) + j];
        upk.clear();
        usv.clear();
        // vx, vy as the mapping above gives them: dense terms go to the list at once, unit terms behind them
        auto put = [&](int32_t vx, int32_t vy, double s) {
          const bool ux = vx < CHILD && vx >= nnp, uy = vy < CHILD && vy >= nnp;
          if (ux != uy) {
            upk.push_back((ux ? vy | (vx << 16) : vx | (vy << 16)) | FAM_UNIT_TERM);
            usv.push_back(s);
          } else {
            T.fpk[o] = vx | (vy << 16);
            T.fsv[o++] = s;
          }
        };
        for (int32_t q = kptr[(size_t)k * (m + 1) + j]; q < kptr[(size_t)k * (m + 1) + j + 1]; ++q) {
          const int32_t i = kij[q] & 0xffff, jc = kij[q] >> 16;
          put(i, jc, i == jc ? 0.5 * kval[q] : kval[q]);
        }
        int32_t colbase = 0;
        for (int64_t q2 = S.chptr[k]; q2 < S.chptr[k + 1]; ++q2) {
          const int64_t cc = S.chidx[q2];
          const int32_t nnc = (int32_t)S.nn(cc);
          const int32_t* rel = &S.relidx[S.sepptr[cc]];
          for (int32_t q = kptr[(size_t)cc * (m + 1) + j]; q < kptr[(size_t)cc * (m + 1) + j + 1]; ++q) {
            const int32_t i = kij[q] & 0xffff, jc = kij[q] >> 16;
            if (i >= nnc) put(CHILD + colbase + jc, rel[i - nnc], -kval[q]);
            else put(CHILD + colbase + i, CHILD + colbase + jc, i == jc ? 0.5 * kval[q] : kval[q]);
          }
          colbase += nnc;
        }
        for (size_t x = 0; x < upk.size(); ++x, ++o) { T.fpk[o] = upk[x]; T.fsv[o] = usv[x]; }
      }
    }
  });
  T.has_fam_terms = true;
}

}  // namespace

int build_constraint_tables(const Symbolic& S, const ConstraintParams& P, int64_t m, const int64_t* cptr, const int64_t* cidx,
                            const double* cval, ConstraintTables& T, const ConstraintStepMark& mark) {
  T = ConstraintTables();
  Build B{S, P, m, cptr[m], cptr, cidx, cval, T, {}, {}};
  auto done = [&](const char* step) { if (mark) mark(step, B.threads); B.threads = 1; };
  if (!locate_entries(B)) return SMCP_EINVAL;
  done("locate entries");
  classify_columns(B);
  done("classify");
  csr_by_position(B);
  done("CSR by position");
  if (B.nnz < ((int64_t)1 << 31) && S.nsn * (m + 1) <= ((int64_t)1 << 28)) {
    group_entries(B);
    entry_statistics(B);
    T.has_entry_tables = true;
    done("entry tables");
    if (T.lg_children > 0 && m < 32768) leafgram_lists(B);
    done("leaf Gram tables");
    if (T.fam_maxterms > 0 && P.famt_terms_ok(T.fam_maxterms, T.fam_meanterms) && !P.fam->empty() && number_families(B))
      family_term_lists(B);
    done("family term lists");
  }
  return 0;
}

}  // namespace smcp
