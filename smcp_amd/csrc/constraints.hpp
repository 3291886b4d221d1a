// Host tables of a constraint set: everything kkt_set_constraints uploads, built from the symbolic analysis, two masks of
// the device set-up and the caller's arrays.  Plain host C++ like symbolic.cpp: no device header, no environment switch;
// what the builder needs from either arrives in ConstraintParams.  The result does not depend on how many host threads
// built it (tests/host/constraint_tables_check.cpp).
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "symbolic.hpp"

namespace smcp {

struct ConstraintParams {
  double tnzcols = 0.1;          // csp_ctx::tnzcols
  int64_t max_rhs = 0;           // DeviceCtx::max_rhs, tmplen: workspace of the triangular solves of the SCMcolumn2 path
  int64_t tmplen = 0;
  bool scm_on = true;            // column-sparse constraints take the SCMcolumn2 path (SMCP_SCM, and not the generic route)
  const std::vector<int64_t>* fam = nullptr;          // csp_ctx::fam: per clique 1 = family child, 2 = family parent
  const std::vector<uint8_t>* large_mask = nullptr;   // csp_ctx::large_mask: per clique, a large front
  // the gate of the entry-driven family sweeps on the statistics step 4 computes (longest and mean (family, constraint) list)
  bool (*famt_terms_ok)(int64_t fam_maxterms, double fam_meanterms) = nullptr;
  int lf_alds_maxnf = 0;         // LF_ALDS_MAXNF (front_large.hip): rows of the largest front the LDS extend-add takes
  int famt_child = 0;            // FAMT_CHILD (front_famt.hip): first vector id of a child column in a term
  int max_threads = 16;          // most host threads of a step
};

struct ConstraintTables {
  // 1. entries: weights (off-diagonals doubled), matrix coordinates; 2. positions within the column set of a sparse constraint
  std::vector<double> w;
  std::vector<int32_t> ar, ac, rloc, cloc;
  // 2. the dense / sparse split, the column sets of the sparse constraints and their offsets; columns of S^-1 kept at once
  std::vector<int32_t> dl, sl, kidx;
  std::vector<int64_t> h_kptr;
  int64_t vcols = 0;
  // 3. CSR by position
  std::vector<int64_t> rpos, rptr;
  std::vector<int32_t> rcon;
  std::vector<double> rval;
  // 4. entries grouped by (clique, constraint), and what the routes decide on
  bool has_entry_tables = false;
  std::vector<int32_t> kptr, koff, kij;
  std::vector<double> kval;
  int64_t kc_maxlist = 0, kc_maxlist_large = 0, fam_maxterms = 0;
  double fam_meanterms = 0.0;
  bool kc_sorted = false;
  int64_t lg_children = 0, lg_maxent = 0, lg_pairs = 0, lg_rows = 0;
  int lg_rec = 0;
  std::vector<int32_t> lg_slot_of, lg_eptr;
  // 5. entry lists of the family children (closed-form Gram blocks)
  bool has_leafgram = false;
  std::vector<int32_t> epk, remap;
  std::vector<double> ewv;
  // 6. static term lists of the family parents (fused extend-add); fz_levels is filled whenever the gate let the step look
  bool has_fz_levels = false, has_fam_terms = false;
  std::vector<uint8_t> fz_levels;
  std::vector<int32_t> fno, fptr, fpk;
  std::vector<double> fsv;
  int64_t fz_nfam = 0;
};

// called at the end of every step with its name and the host threads it ran on
using ConstraintStepMark = std::function<void(const char* step, int threads)>;

// The constraint set (cptr, cidx, cval): CSC over blkval positions, m columns.  SMCP_EINVAL for a position outside blkval
// or in the strict upper triangle of an NN block (T is then unspecified), 0 otherwise.
int build_constraint_tables(const Symbolic& S, const ConstraintParams& P, int64_t m, const int64_t* cptr, const int64_t* cidx,
                            const double* cval, ConstraintTables& T, const ConstraintStepMark& mark = nullptr);

}  // namespace smcp
