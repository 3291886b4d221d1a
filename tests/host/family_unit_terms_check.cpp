// Stand-alone check of the static term lists of the family parents (smcp_amd/csrc/constraints.cpp, family_term_lists);
// tests/test_family_unit_terms_host.py compiles it with constraints.cpp and symbolic.cpp and expects exit status 0.
//
// Two block arrows of 64 families (a parent of 4 columns with two childless children of 3 columns, three separator rows in
// one root front), generated here.  In the first the children see the parent's columns only, so a child's separator-row
// entry is always a dense term; in the second they also see two of the parent's separator rows, so that such an entry is a
// unit term whenever its row is one of those.  Four hand-made constraints: every lower position of V once (all classes in
// one list); the parents' separator-row entries only (unit terms only); the supernode blocks only (dense terms only); and a
// few repeated positions in every other family (empty lists, duplicates).  Checked for every (family, constraint) list:
//   (a) its dense terms, in order, are the dense terms the mapping of front_famt.hip's header gives for the entries of
//       kij / kval / relidx in entry order (ids and scale, bit for bit), and its unit terms likewise -- so the list is a
//       permutation of that mapping's list which keeps the order inside each class;
//   (b) no dense term follows a unit term;
//   (c) the flag is set exactly on the terms with one unit vector of the parent's separator part, the dense vector in the
//       low half and the unit vector in the high half;
//   (d) fptr, fpk, fsv are equal byte for byte on 1 and on 4 host threads (and the second build did use more than one).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/smcp_amd.h"
#include "../../smcp_amd/csrc/constraints.hpp"

using namespace smcp;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const int32_t CHILD = 128, UNIT = 1 << 30;

struct Pattern { int64_t n; std::vector<int64_t> colptr, rowind; };

static Pattern block_arrow(int64_t nfam, bool children_see_separator) {
  const int64_t NL = 3, NP = 4, NR = 24, per = 2 * NL + NP, n = nfam * per + NR;
  std::vector<std::vector<int64_t>> cols((size_t)n);
  for (int64_t f = 0; f < nfam; ++f) {
    const int64_t b = f * per, pb = b + 2 * NL;
    std::vector<int64_t> sep = {nfam * per + f % NR, nfam * per + (f + 5) % NR, nfam * per + (f + 11) % NR};
    std::sort(sep.begin(), sep.end());
    for (int64_t c = 0; c < 2; ++c)
      for (int64_t j = 0; j < NL; ++j) {
        auto& col = cols[(size_t)(b + c * NL + j)];
        for (int64_t i = j; i < NL; ++i) col.push_back(b + c * NL + i);
        for (int64_t i = (children_see_separator && c == 0) ? 1 : 0; i < NP; ++i) col.push_back(pb + i);
        if (children_see_separator) { col.push_back(sep[0]); col.push_back(sep[2]); }
      }
    for (int64_t j = 0; j < NP; ++j) {
      auto& col = cols[(size_t)(pb + j)];
      for (int64_t i = j; i < NP; ++i) col.push_back(pb + i);
      col.insert(col.end(), sep.begin(), sep.end());
    }
  }
  for (int64_t j = 0; j < NR; ++j) for (int64_t i = j; i < NR; ++i) cols[(size_t)(nfam * per + j)].push_back(nfam * per + i);
  Pattern p;
  p.n = n;
  p.colptr.push_back(0);
  for (const auto& c : cols) { p.rowind.insert(p.rowind.end(), c.begin(), c.end()); p.colptr.push_back((int64_t)p.rowind.size()); }
  return p;
}

struct Problem {
  Symbolic S;
  std::vector<int64_t> fam;
  std::vector<uint8_t> large_mask;
  int64_t m = 4;
  std::vector<int64_t> cptr, cidx;
  std::vector<double> cval;
};

static bool gate_open(int64_t, double) { return true; }

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
  pr.cptr.assign(1, 0);
  auto add = [&](int64_t pos) { pr.cidx.push_back(pos); pr.cval.push_back(1.0 + (double)(pos % 977) / 16.0 + (double)pr.cidx.size() / 4096.0); };
  for (int64_t j = 0; j < pr.m; ++j) {
    for (int64_t k = 0; k < S.nsn; ++k)
      for (int64_t col = 0; col < S.nn(k); ++col)
        for (int64_t row = col; row < S.nf(k); ++row) {
          const int64_t pos = S.blkptr[k] + col * S.nf(k) + row;
          const bool parent = pr.fam[(size_t)k] == 2;
          if (j == 0) add(pos);
          else if (j == 1) { if (parent && row >= S.nn(k)) add(pos); }
          else if (j == 2) { if (row < S.nn(k)) add(pos); }
          // (the cliques come child, child, parent: every other family)
          else if ((k / 3) % 2 == 0 && (row + col) % 3 == 0) { add(pos); add(pos); if (row == col) add(pos); }
        }
    pr.cptr.push_back((int64_t)pr.cidx.size());
  }
}

static ConstraintParams params(const Problem& pr, int max_threads) {
  ConstraintParams P;
  P.tnzcols = 0.0;
  P.max_rhs = 4;
  P.tmplen = 2 * pr.S.blklen() + 256 * pr.S.nsn;
  P.scm_on = true;
  P.fam = &pr.fam;
  P.large_mask = &pr.large_mask;
  P.famt_terms_ok = gate_open;
  P.lf_alds_maxnf = 198;
  P.famt_child = CHILD;
  P.max_threads = max_threads;
  return P;
}

struct Term { int32_t vx, vy; double s; };

// the mapping of front_famt.hip's header for (family parent k, constraint j), in entry order: the parent's own entries,
// then its children's in chidx order
static std::vector<Term> mapped(const Symbolic& S, const ConstraintTables& T, int64_t m, int64_t k, int64_t j) {
  std::vector<Term> out;
  for (int32_t q = T.kptr[(size_t)(k * (m + 1) + j)]; q < T.kptr[(size_t)(k * (m + 1) + j + 1)]; ++q) {
    const int32_t i = T.kij[(size_t)q] & 0xffff, jc = T.kij[(size_t)q] >> 16;
    out.push_back({i, jc, i == jc ? 0.5 * T.kval[(size_t)q] : T.kval[(size_t)q]});
  }
  int32_t colbase = 0;
  for (int64_t q2 = S.chptr[k]; q2 < S.chptr[k + 1]; ++q2) {
    const int64_t cc = S.chidx[q2];
    const int32_t nnc = (int32_t)S.nn(cc);
    const int32_t* rel = &S.relidx[S.sepptr[cc]];
    for (int32_t q = T.kptr[(size_t)(cc * (m + 1) + j)]; q < T.kptr[(size_t)(cc * (m + 1) + j + 1)]; ++q) {
      const int32_t i = T.kij[(size_t)q] & 0xffff, jc = T.kij[(size_t)q] >> 16;
      if (i >= nnc) out.push_back({CHILD + colbase + jc, rel[i - nnc], -T.kval[(size_t)q]});
      else out.push_back({CHILD + colbase + i, CHILD + colbase + jc, i == jc ? 0.5 * T.kval[(size_t)q] : T.kval[(size_t)q]});
    }
    colbase += nnc;
  }
  return out;
}

struct Counts { int64_t lists = 0, empty = 0, dense = 0, unit = 0, unit_child = 0, unit_own = 0, mixed = 0, only_unit = 0, only_dense = 0; };

static void check_lists(const Problem& pr, const ConstraintTables& T, const char* what, Counts& cn) {
  const Symbolic& S = pr.S;
  const int64_t m = pr.m;
  CHECK(T.has_fam_terms && T.fz_nfam == 64 && (int64_t)T.fptr.size() == T.fz_nfam * (m + 1) + 1 && T.fptr.back() == (int32_t)T.fpk.size() &&
        T.fpk.size() == T.fsv.size(), "%s: no term lists (%lld families)", what, (long long)T.fz_nfam);
  if (failures) return;
  for (int64_t k = 0; k < S.nsn; ++k) {
    const int32_t f = T.fno[(size_t)k];
    if (f < 0) continue;
    const int32_t nnp = (int32_t)S.nn(k);
    auto is_unit = [&](int32_t v) { return v < CHILD && v >= nnp; };
    for (int64_t j = 0; j < m; ++j) {
      const std::vector<Term> want = mapped(S, T, m, k, j);
      const int32_t p0 = T.fptr[(size_t)(f * (m + 1) + j)], p1 = T.fptr[(size_t)(f * (m + 1) + j + 1)];
      CHECK(p1 - p0 == (int32_t)want.size(), "%s: list (%d, %lld) holds %d terms, the entries give %zu", what, f, (long long)j, p1 - p0, want.size());
      if (p1 - p0 != (int32_t)want.size()) continue;
      std::vector<Term> wd, wu;
      for (const Term& t : want) (is_unit(t.vx) != is_unit(t.vy) ? wu : wd).push_back(t);
      ++cn.lists;
      cn.empty += want.empty();
      cn.dense += (int64_t)wd.size();
      cn.unit += (int64_t)wu.size();
      cn.mixed += !wd.empty() && !wu.empty();
      cn.only_unit += wd.empty() && !wu.empty();
      cn.only_dense += !wd.empty() && wu.empty();
      size_t nd = 0, nu = 0;
      bool seen_unit = false;
      for (int32_t p = p0; p < p1; ++p) {
        const int32_t pk = T.fpk[(size_t)p], lo = pk & 0xff, hi = (pk >> 16) & 0xff;
        const bool flag = (pk & UNIT) != 0;
        CHECK((pk & ~(UNIT | 0x00ff00ff)) == 0, "%s: term %d of (%d, %lld) has stray bits: %08x", what, p - p0, f, (long long)j, (unsigned)pk);
        CHECK(flag == (is_unit(lo) != is_unit(hi)), "%s: flag of term %d of (%d, %lld): ids %d, %d, nn %d", what, p - p0, f, (long long)j, lo, hi, nnp);
        if (flag) {
          seen_unit = true;
          CHECK(!is_unit(lo) && is_unit(hi), "%s: unit term %d of (%d, %lld) is not normalised: ids %d, %d", what, p - p0, f, (long long)j, lo, hi);
          if (nu < wu.size()) {
            const Term& w = wu[nu];
            const int32_t wdv = is_unit(w.vx) ? w.vy : w.vx, wuv = is_unit(w.vx) ? w.vx : w.vy;
            CHECK(lo == wdv && hi == wuv && !memcmp(&T.fsv[(size_t)p], &w.s, sizeof(double)), "%s: unit term %zu of (%d, %lld) differs from the mapping", what, nu, f, (long long)j);
            (wdv >= CHILD ? cn.unit_child : cn.unit_own) += 1;
          }
          ++nu;
        } else {
          CHECK(!seen_unit, "%s: dense term %d of (%d, %lld) behind a unit term", what, p - p0, f, (long long)j);
          if (nd < wd.size()) {
            const Term& w = wd[nd];
            CHECK(lo == w.vx && hi == w.vy && !memcmp(&T.fsv[(size_t)p], &w.s, sizeof(double)), "%s: dense term %zu of (%d, %lld) differs from the mapping", what, nd, f, (long long)j);
          }
          ++nd;
        }
      }
      CHECK(nd == wd.size() && nu == wu.size(), "%s: (%d, %lld) has %zu dense and %zu unit terms, the mapping %zu and %zu", what, f, (long long)j, nd, nu, wd.size(), wu.size());
    }
  }
}

static Counts run(const char* name, const Pattern& pat) {
  Problem pr;
  make_problem(pat, pr);
  ConstraintTables T1, T4;
  std::map<std::string, int> th4;
  const int rc1 = build_constraint_tables(pr.S, params(pr, 1), pr.m, pr.cptr.data(), pr.cidx.data(), pr.cval.data(), T1);
  const int rc4 = build_constraint_tables(pr.S, params(pr, 4), pr.m, pr.cptr.data(), pr.cidx.data(), pr.cval.data(), T4,
                                          [&](const char* step, int threads) { th4[step] = threads; });
  CHECK(rc1 == 0 && rc4 == 0, "%s: status %d, %d", name, rc1, rc4);
  CHECK(th4["family term lists"] > 1, "%s: the term lists were built on %d thread(s) with max_threads = 4: nothing compared", name, th4["family term lists"]);
  auto same = [](const auto& a, const auto& b) { return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(a[0]))); };
  CHECK(same(T1.fptr, T4.fptr) && same(T1.fpk, T4.fpk) && same(T1.fsv, T4.fsv), "%s: the term lists depend on the thread count", name);
  Counts cn;
  check_lists(pr, T4, name, cn);
  printf("%s: %lld lists (%lld empty, %lld unit only, %lld dense only, %lld mixed), %lld dense and %lld unit terms (%lld on a -K column, %lld on a child column)\n",
         name, (long long)cn.lists, (long long)cn.empty, (long long)cn.only_unit, (long long)cn.only_dense, (long long)cn.mixed,
         (long long)cn.dense, (long long)cn.unit, (long long)cn.unit_own, (long long)cn.unit_child);
  return cn;
}

int main() {
  const Counts a = run("children inside the parent's columns", block_arrow(64, false));
  const Counts b = run("children on the parent's separator", block_arrow(64, true));
  // the cases must have occurred, or nothing was checked
  CHECK(a.unit_own > 0 && a.unit_child == 0 && a.empty > 0 && a.only_unit > 0 && a.only_dense > 0 && a.mixed > 0, "first pattern: a class of lists is missing");
  CHECK(b.unit_own > 0 && b.unit_child > 0 && b.empty > 0 && b.only_unit > 0 && b.only_dense > 0 && b.mixed > 0, "second pattern: a class of lists is missing");
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("family unit terms: ok\n");
  return 0;
}
