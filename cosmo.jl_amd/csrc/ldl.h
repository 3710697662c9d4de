// ldl.h -- the direct KKT solver (COSMO_HIP_KKT_DIRECT): symbolic analysis (ldl_symbolic.cpp, host only, pattern only) and the supernodal
// LDL' factorisation / solve on the device (ldl.hip).
//
// K = [P + sigma I, A'; A, -diag(1 ./ rho)] (the reference's assemble_kkt_triangle, src/linear_solver/kktsolver.jl:175-250) is permuted
// symmetrically, K[perm, perm] = L D L', perm[k] = the original index at position k.  The columns of L are grouped into supernodes: a run of
// consecutive columns f .. l-1 with parent(j) = j + 1 and nnz(L(:, j)) = nnz(L(:, j + 1)) + 1, so all its columns share one row structure
// rows_J = {f .. l-1} u pattern(L(:, l-1)).  Supernode J is stored as a dense column-major panel of nrows_J x ncols_J values: entry (r, c)
// (r = position in rows_J, c = column - f) at poff[J] + c * nrows_J + r; D sits on the diagonal (r = c), L below it, the strict upper part of
// the diagonal block is never read.
#pragma once
#include <stdint.h>
#include <vector>

struct LdlSymbolic {
  int64_t n = 0, m = 0, N = 0;
  std::vector<int64_t> perm, iperm;        // perm[k] = original index at permuted position k; iperm[perm[k]] = k
  // supernodes (ns of them, in column order; a parent always comes after its children)
  int64_t ns = 0;
  std::vector<int64_t> sn_first;           // ns + 1: first permuted column of supernode J; sn_first[ns] = N
  std::vector<int64_t> sn_rp;              // ns + 1: rows_J = sn_rows[sn_rp[J] .. sn_rp[J+1])
  std::vector<int32_t> sn_rows;            // ascending permuted row indices
  std::vector<int64_t> sn_poff;            // ns + 1: panel offsets
  std::vector<int64_t> sn_parent;          // -1 for roots
  std::vector<int32_t> sn_of;              // N: supernode of a permuted column
  // level schedule: level 0 = supernodes without children; level of a parent = 1 + max level of its children
  std::vector<int32_t> lvl_ptr, lvl_sn;
  // left-looking update lists: the descendants K of J (ascending) whose rows [r0, r1) (positions in rows_K) are columns of J; rows [r1, ..)
  // of K lie in the rest of rows_J
  std::vector<int32_t> desc_ptr;           // ns + 1
  std::vector<int32_t> desc;               // 3 per pair: K, r0, r1
  // figures (cosmo_hip_ldl_analyze: out[8])
  int64_t nnz_L = 0;                       // strictly lower nonzeros of L (QDLDL's count), without amalgamation zeros
  int64_t nnz_stored = 0;                  // strictly lower entries held by the panels (nnz_L + amalgamation zeros)
  int64_t height = 0;                      // levels of the supernodal tree
  int64_t max_width = 0;                   // widest supernode
  int64_t amalg_zeros = 0;                 // explicit zeros added by amalgamation (0: maximal supernodes only, no relaxed amalgamation)
  int64_t panel_size = 0;                  // values held by the panels (including the unused upper half of each diagonal block)
  double seconds = 0.0;                    // wall time of the analysis

  // slot of K entry (i, j) (ORIGINAL indices, i != j or i == j) in the panel storage; -1 if the pattern has no such entry
  int64_t slot(int64_t i, int64_t j) const;
};

// Pattern of K given as the upper off-diagonal entries of P (row < col, original indices 0..n-1) and the entries of A (row i of A = node n + i,
// column j).  Duplicates are allowed.  perm: NULL = the default ordering (rows of A with at most one entry first, then approximate minimum degree
// on the rest), otherwise a permutation of n + m in the convention above (checked).  Returns 0, or -1 with *err set.
int ldl_analyze(int64_t n, int64_t m, const std::vector<int64_t>& p_row, const std::vector<int64_t>& p_col, const std::vector<int64_t>& a_row,
                const std::vector<int64_t>& a_col, const int64_t* perm, LdlSymbolic& S, const char** err);
