// Stand-alone check of the host tables of a constraint set (smcp_amd/csrc/constraints.cpp); tests/test_constraint_tables_host.py
// compiles it with constraints.cpp and symbolic.cpp and expects exit status 0.  No device, no Python.
//
// Two patterns, generated here: a band (n = 60, half-bandwidth 3) and a block arrow whose clique tree has 40 families (a
// parent of 4 columns with two childless children of 3 columns) under one root front, labelled as csp_device_init labels
// them (the band's chain has one family, not under a large front: no term lists).  m = 5 constraints with repeated
// entries, nnz >= 131072, so that every step of the builder takes more than one host thread; tnzcols 0 (every constraint
// swept) and 0.5 (constraints 0 and 1 column-sparse).  Checked:
//   (a) the tables built on 1 and on up to 16 host threads are equal byte for byte -- and the second build did use more than
//       one thread in every parallel step (on a machine with one hardware thread this program fails: it cannot tell);
//   (b) the CSR by position against a stable sort of the entries by position;
//   (c) every entry is in the (clique, constraint) lists once, under its clique and constraint, kij agreeing with koff;
//   (d) a position out of range and one in the strict upper triangle of an NN block are SMCP_EINVAL.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/smcp_amd.h"
#include "../../smcp_amd/csrc/constraints.hpp"

using namespace smcp;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Pattern { int64_t n; std::vector<int64_t> colptr, rowind; };

static Pattern from_columns(const std::vector<std::vector<int64_t>>& cols) {
  Pattern p;
  p.n = (int64_t)cols.size();
  p.colptr.push_back(0);
  for (const auto& c : cols) { p.rowind.insert(p.rowind.end(), c.begin(), c.end()); p.colptr.push_back((int64_t)p.rowind.size()); }
  return p;
}
static Pattern band(int64_t n, int64_t hb) {
  std::vector<std::vector<int64_t>> cols((size_t)n);
  for (int64_t j = 0; j < n; ++j) for (int64_t i = j; i < std::min(n, j + hb + 1); ++i) cols[(size_t)j].push_back(i);
  return from_columns(cols);
}
// per family: child (3 columns), child (3), parent (4); then the root (24 columns).  A child's columns see the parent's, the
// parent's see three columns of the root: a perfect elimination order without fill.
static Pattern block_arrow(int64_t nfam) {
  const int64_t NL = 3, NP = 4, NR = 24, per = 2 * NL + NP, n = nfam * per + NR;
  std::vector<std::vector<int64_t>> cols((size_t)n);
  for (int64_t f = 0; f < nfam; ++f) {
    const int64_t b = f * per, pb = b + 2 * NL;
    for (int64_t c = 0; c < 2; ++c)
      for (int64_t j = 0; j < NL; ++j) {
        auto& col = cols[(size_t)(b + c * NL + j)];
        for (int64_t i = j; i < NL; ++i) col.push_back(b + c * NL + i);
        for (int64_t i = 0; i < NP; ++i) col.push_back(pb + i);
      }
    std::vector<int64_t> sep = {nfam * per + f % NR, nfam * per + (f + 5) % NR, nfam * per + (f + 11) % NR};
    std::sort(sep.begin(), sep.end());
    for (int64_t j = 0; j < NP; ++j) {
      auto& col = cols[(size_t)(pb + j)];
      for (int64_t i = j; i < NP; ++i) col.push_back(pb + i);
      col.insert(col.end(), sep.begin(), sep.end());
    }
  }
  for (int64_t j = 0; j < NR; ++j) for (int64_t i = j; i < NR; ++i) cols[(size_t)(nfam * per + j)].push_back(nfam * per + i);
  return from_columns(cols);
}

struct Problem {
  Symbolic S;
  std::vector<int64_t> fam;
  std::vector<uint8_t> large_mask;
  int64_t m = 5;
  std::vector<int64_t> cptr, cidx;
  std::vector<double> cval;
};

static bool gate_open(int64_t, double) { return true; }    // (the lists here are longer than the library's gate lets through)

// the labelling of csp_device_init for this tree: childless cliques under a small non-root parent are family children,
// their parents family parents; the root is the one large front
static void make_problem(const Pattern& pat, Problem& pr) {
  CHECK(symbolic_build(pat.n, pat.colptr.data(), pat.rowind.data(), nullptr, pr.S) == 0, "symbolic_build");
  const Symbolic& S = pr.S;
  pr.fam.assign((size_t)S.nsn, 0);
  pr.large_mask.assign((size_t)S.nsn, 0);
  for (int64_t k = 0; k < S.nsn; ++k) {
    const int64_t p = S.snpar[k];
    if (p < 0) { pr.large_mask[(size_t)k] = 1; continue; }
    if (S.chptr[k + 1] == S.chptr[k] && S.snpar[p] >= 0 && S.nn(p) <= 16 && S.na(p) <= 64) { pr.fam[(size_t)k] = 1; pr.fam[(size_t)p] = 2; }
  }
  // the positions of V: lower triangle of every NN block, all of every AN block
  std::vector<int64_t> all, head;
  for (int64_t k = 0; k < S.nsn; ++k)
    for (int64_t col = 0; col < S.nn(k); ++col)
      for (int64_t row = col; row < S.nf(k); ++row) {
        all.push_back(S.blkptr[k] + col * S.nf(k) + row);
        if (k < S.nsn / 4) head.push_back(all.back());
      }
  // constraints 0 and 1 draw from the first quarter of the cliques (few distinct columns), the others from everywhere; 27 000
  // draws each with repeats, in no order
  uint64_t state = 12345;
  auto next = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
  pr.cptr.assign(1, 0);
  for (int64_t j = 0; j < pr.m; ++j) {
    const std::vector<int64_t>& from = j < 2 ? head : all;
    for (int e = 0; e < 27000; ++e) {
      pr.cidx.push_back(from[next() % from.size()]);
      pr.cval.push_back((double)((int)(next() % 2001) - 1000) / 64.0);
    }
    pr.cptr.push_back((int64_t)pr.cidx.size());
  }
}

static ConstraintParams params(const Problem& pr, double tnzcols, int max_threads) {
  ConstraintParams P;
  P.tnzcols = tnzcols;
  P.max_rhs = 4;
  P.tmplen = 2 * pr.S.blklen() + 256 * pr.S.nsn;
  P.scm_on = true;
  P.fam = &pr.fam;
  P.large_mask = &pr.large_mask;
  P.famt_terms_ok = gate_open;
  P.lf_alds_maxnf = 198;
  P.famt_child = 128;
  P.max_threads = max_threads;
  return P;
}

template <class V>
static bool same_bytes(const std::vector<V>& a, const std::vector<V>& b) {
  return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(V)));
}
static void compare(const ConstraintTables& A, const ConstraintTables& B, const char* what) {
#define VEC(f) CHECK(same_bytes(A.f, B.f), "%s: " #f " depends on the thread count", what)
#define SCA(f) CHECK(!memcmp(&A.f, &B.f, sizeof(A.f)), "%s: " #f " depends on the thread count", what)
  VEC(w); VEC(ar); VEC(ac); VEC(rloc); VEC(cloc); VEC(dl); VEC(sl); VEC(kidx); VEC(h_kptr);
  VEC(rpos); VEC(rptr); VEC(rcon); VEC(rval); VEC(kptr); VEC(koff); VEC(kval); VEC(kij);
  VEC(lg_eptr); VEC(epk); VEC(ewv); VEC(remap); VEC(lg_slot_of); VEC(fno); VEC(fptr); VEC(fpk); VEC(fsv); VEC(fz_levels);
  SCA(kc_maxlist); SCA(kc_maxlist_large); SCA(fam_maxterms); SCA(fam_meanterms); SCA(kc_sorted);
  SCA(lg_children); SCA(lg_maxent); SCA(lg_pairs); SCA(lg_rows); SCA(lg_rec); SCA(fz_nfam); SCA(vcols);
  SCA(has_entry_tables); SCA(has_leafgram); SCA(has_fz_levels); SCA(has_fam_terms);
#undef VEC
#undef SCA
}

static int64_t clique_of(const Symbolic& S, int64_t pos) {
  return (int64_t)(std::upper_bound(S.blkptr.begin(), S.blkptr.end(), pos) - S.blkptr.begin()) - 1;
}

// (b)
static void check_csr(const Problem& pr, const ConstraintTables& T, const char* what) {
  const int64_t nnz = pr.cptr[pr.m];
  CHECK(T.rptr.size() == T.rpos.size() + 1 && T.rptr.front() == 0 && T.rptr.back() == nnz, "%s: rptr ends", what);
  for (size_t d = 0; d + 1 < T.rpos.size(); ++d) CHECK(T.rpos[d] < T.rpos[d + 1], "%s: rpos not strictly ascending at %zu", what, d);
  for (size_t d = 0; d < T.rpos.size(); ++d) {
    CHECK(T.rptr[d] < T.rptr[d + 1], "%s: empty run at %zu", what, d);
    for (int64_t q = T.rptr[d] + 1; q < T.rptr[d + 1]; ++q) CHECK(T.rcon[(size_t)q - 1] <= T.rcon[(size_t)q], "%s: constraint ids descend in run %zu", what, d);
  }
  std::vector<int64_t> order((size_t)nnz);
  std::iota(order.begin(), order.end(), (int64_t)0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return pr.cidx[(size_t)a] < pr.cidx[(size_t)b]; });
  int64_t bad = 0;
  size_t d = 0;
  for (int64_t q = 0; q < nnz; ++q) {
    const int64_t e = order[(size_t)q];
    while (d + 1 < T.rpos.size() && T.rptr[d + 1] <= q) ++d;
    const int64_t j = (int64_t)(std::upper_bound(pr.cptr.begin(), pr.cptr.end(), e) - pr.cptr.begin()) - 1;
    bad += !(T.rpos[d] == pr.cidx[(size_t)e] && T.rcon[(size_t)q] == j && !memcmp(&T.rval[(size_t)q], &pr.cval[(size_t)e], sizeof(double)));
  }
  CHECK(bad == 0, "%s: %lld entries of the CSR differ from a stable sort by position", what, (long long)bad);
}

// (c)
static void check_entry_lists(const Problem& pr, const ConstraintTables& T, const char* what) {
  const Symbolic& S = pr.S;
  const int64_t m = pr.m, nnz = pr.cptr[m];
  CHECK(T.has_entry_tables && (int64_t)T.kptr.size() == S.nsn * (m + 1), "%s: entry tables", what);
  if (failures) return;
  auto slot_end = [&](size_t s) { return s + 1 < T.kptr.size() ? (int64_t)T.kptr[s + 1] : nnz; };
  std::vector<int32_t> cursor(T.kptr);
  int64_t bad = 0;
  for (int64_t j = 0; j < m; ++j)
    for (int64_t e = pr.cptr[j]; e < pr.cptr[j + 1]; ++e) {
      const int64_t k = clique_of(S, pr.cidx[(size_t)e]), off = pr.cidx[(size_t)e] - S.blkptr[k], nf = S.nf(k);
      const size_t s = (size_t)(k * (m + 1) + j);
      const int64_t q = cursor[s]++;
      if (q >= slot_end(s)) { ++bad; continue; }
      bad += !(T.koff[(size_t)q] == off && !memcmp(&T.kval[(size_t)q], &pr.cval[(size_t)e], sizeof(double)) &&
               T.kij[(size_t)q] == (int32_t)((off % nf) | ((off / nf) << 16)));
    }
  CHECK(bad == 0, "%s: %lld entries misplaced in the (clique, constraint) lists", what, (long long)bad);
  for (size_t s = 0; s < T.kptr.size(); ++s) {
    CHECK(cursor[s] == slot_end(s), "%s: list %zu holds entries that are not its own", what, s);
    if (s % (size_t)(m + 1) == (size_t)m) CHECK(T.kptr[s] == slot_end(s), "%s: slot (k, m) is not empty", what);
  }
}

// (d)
static void check_invalid(const Problem& pr, const char* what) {
  const Symbolic& S = pr.S;
  ConstraintTables T;
  for (int64_t badpos : {S.blklen(), (int64_t)-1}) {
    std::vector<int64_t> cidx(pr.cidx);
    cidx[cidx.size() / 2] = badpos;
    CHECK(build_constraint_tables(S, params(pr, 0.5, 16), pr.m, pr.cptr.data(), cidx.data(), pr.cval.data(), T) == SMCP_EINVAL,
          "%s: position %lld accepted", what, (long long)badpos);
  }
  int64_t k = 0;
  while (k < S.nsn && S.nn(k) < 2) ++k;
  CHECK(k < S.nsn, "%s: no clique with two columns", what);
  if (k == S.nsn) return;
  std::vector<int64_t> cidx(pr.cidx);
  cidx.back() = S.blkptr[k] + S.nf(k);          // row 0, column 1 of the NN block
  CHECK(build_constraint_tables(S, params(pr, 0.5, 16), pr.m, pr.cptr.data(), cidx.data(), pr.cval.data(), T) == SMCP_EINVAL,
        "%s: upper-triangle position accepted", what);
}

static void run(const char* name, const Pattern& pat, bool families) {
  Problem pr;
  make_problem(pat, pr);
  CHECK(pr.cptr[pr.m] >= 131072, "%s: nnz", name);
  for (double tnzcols : {0.0, 0.5}) {
    const std::string what = std::string(name) + (tnzcols ? " tnzcols 0.5" : " tnzcols 0");
    ConstraintTables T1, T16;
    std::map<std::string, int> th1, th16;
    const int rc1 = build_constraint_tables(pr.S, params(pr, tnzcols, 1), pr.m, pr.cptr.data(), pr.cidx.data(), pr.cval.data(), T1,
                                            [&](const char* step, int threads) { th1[step] = threads; });
    const int rc16 = build_constraint_tables(pr.S, params(pr, tnzcols, 16), pr.m, pr.cptr.data(), pr.cidx.data(), pr.cval.data(), T16,
                                             [&](const char* step, int threads) { th16[step] = threads; });
    CHECK(rc1 == 0 && rc16 == 0, "%s: status %d, %d", what.c_str(), rc1, rc16);
    for (const auto& kv : th1) CHECK(kv.second == 1, "%s: %s ran on %d threads with max_threads = 1", what.c_str(), kv.first.c_str(), kv.second);
    std::vector<const char*> parallel = {"locate entries", "classify", "CSR by position", "entry tables"};
    if (families) parallel.push_back("family term lists");
    for (const char* step : parallel)
      CHECK(th16[step] > 1, "%s: %s ran on %d thread(s) with max_threads = 16: nothing compared", what.c_str(), step, th16[step]);
    compare(T1, T16, what.c_str());
    check_csr(pr, T16, what.c_str());
    check_entry_lists(pr, T16, what.c_str());
    CHECK(tnzcols ? (!T16.dl.empty() && !T16.sl.empty() && T16.vcols > 0) : (T16.sl.empty() && (int64_t)T16.dl.size() == pr.m),
          "%s: %zu swept and %zu column-sparse constraints", what.c_str(), T16.dl.size(), T16.sl.size());
    CHECK(T16.h_kptr.size() == T16.sl.size() + 1 && T16.h_kptr.back() == (int64_t)T16.kidx.size(), "%s: h_kptr", what.c_str());
    if (families) {
      CHECK(T16.has_leafgram && T16.lg_children >= 32 && T16.lg_eptr.back() == (int32_t)T16.epk.size(), "%s: leaf-Gram lists", what.c_str());
      CHECK(T16.has_fam_terms && T16.fz_nfam >= 16 && T16.fptr.back() == (int32_t)T16.fpk.size() && T16.fpk.size() == T16.fsv.size(),
            "%s: family term lists (%lld families)", what.c_str(), (long long)T16.fz_nfam);
    } else {        // the chain's first two cliques form a family, but not under a large front: numbered, levels marked, no lists
      CHECK(T16.lg_children == 1 && T16.has_fz_levels && !T16.has_fam_terms && T16.fpk.empty(), "%s: term lists outside a large front", what.c_str());
    }
  }
  check_invalid(pr, name);
}

int main() {
  run("band", band(60, 3), false);
  run("block arrow", block_arrow(40), true);
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("constraint tables: ok\n");
  return 0;
}
