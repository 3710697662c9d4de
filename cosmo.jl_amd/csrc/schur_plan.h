// schur_plan.h -- host analysis of the Schur-complement KKT solver (COSMO_HIP_KKT_SCHUR; schur_plan.cpp, host only, pattern only; the device side is
// schur.hip).  The reduced matrix M = P + sigma I + A' rho A is split by the rows of A: a row with at least `row_threshold` stored entries is LONG and
// belongs to A_d (nd rows), every other row and all of P belong to
//     M_s = P + sigma I + A_s' rho_s A_s,      M = M_s + A_d' rho_d A_d.
// The connected components of pattern(M_s) are the diagonal blocks of M_s under the symmetric permutation `perm`; a block of side s is stored as a full
// s x s square (row-major) at boff[k] of the packed storage.  Every map is in a fixed order: the same input gives the same plan, and the device adds the
// terms of a block entry left to right (no atomics).
#pragma once
#include <stdint.h>
#include <vector>

// limits of the device kernels (schur.hip): the dense capacitance matrix C and its inverse are two (nd rounded up to SCHUR_NB)^2 arrays, which have to fit
// SCHUR_MEM_BUDGET together; a block of M_s is inverted by at most one workgroup of SCHUR_BLOCK_MAX threads, one column of the inverse per thread
#define SCHUR_NB 64                      // block side of the dense Cholesky factorisation of C
#define SCHUR_WAVE_MAX 64                // blocks up to this side are factored by one wave, larger ones by a workgroup
#define SCHUR_SMALL_MAX 3                // blocks up to this side are factored by one thread each
#define SCHUR_BLOCK_MAX_DEFAULT 256
#define SCHUR_ND_MAX_DEFAULT 16384       // 2 * 16384^2 * 8 bytes = 4 GiB
#define SCHUR_MEM_BUDGET (8LL << 30)     // bytes of C plus C^-1 (Float64: nd <= 23170)
#define SCHUR_ROW_THRESHOLD_DEFAULT 3
#define SCHUR_REFINE_STEPS_DEFAULT 2
#define SCHUR_REFINE_STEPS_MAX 8

struct SchurPlan {
  int64_t n = 0, m = 0, nd = 0, ncomp = 0, largest = 0, sumsq = 0, nnz_w = 0;
  int row_threshold = SCHUR_ROW_THRESHOLD_DEFAULT;
  int n_small = 0, n_wave = 0;          // blocks [0, n_small) have side <= SCHUR_SMALL_MAX, [n_small, n_wave) side <= SCHUR_WAVE_MAX, the rest are larger
  std::vector<int> perm;                // position -> variable: the members of block k are perm[comp_ptr[k] .. comp_ptr[k + 1]), ascending
  std::vector<int> pos;                 // variable -> position
  std::vector<int> comp_ptr;            // ncomp + 1
  std::vector<int> blk_of_pos;          // n: position -> block
  std::vector<int64_t> boff;            // ncomp + 1: offset of block k in the packed storage (side^2 entries each)
  // refill: packed entry epos[e] = sum over t in [eptr[e], eptr[e + 1]) of term t, left to right.  Term t: tb[t] == -2: sigma; tb[t] == -1: P.val[ta[t]];
  // else A.val[ta[t]] * A.val[tb[t]] * rho[trow[t]].  Entries without a term are not listed (they are zero).  ta / tb index the CSR arrays handed in.
  std::vector<int64_t> epos;
  std::vector<int64_t> eptr;
  std::vector<int> ta, tb, trow;
  // the long rows, as index lists into the CSR of A (values are read from A.val itself): row kd of A_d is row ad_row[kd] of A
  std::vector<int> ad_row, ad_ptr, ad_col, ad_src;     // CSR of A_d (nd rows)
  std::vector<int> adt_ptr, adt_k, adt_src;            // CSR of A_d' (n rows): adt_k = row of A_d, ascending
};

// P: n x n, A: m x n, both CSR, 0-based (column indices within a row in any order, duplicates allowed).  Returns 0, or -1 with *err set.
int schur_analyze(int64_t n, int64_t m, const std::vector<int>& p_ptr, const std::vector<int>& p_col, const std::vector<int>& a_ptr,
                  const std::vector<int>& a_col, int row_threshold, SchurPlan& S, const char** err);
// bytes of C plus C^-1 for `real_bytes` per value
int64_t schur_dense_bytes(int64_t nd, int real_bytes);
// 0: accepted; 1: nd > nd_max; 2: a block larger than block_max; 3: the dense matrices exceed SCHUR_MEM_BUDGET
int schur_check_limits(const SchurPlan& S, int64_t nd_max, int64_t block_max, int real_bytes);
