// Test hook for csrc/value_maps.cpp (compiled by tests/update_matrix_cases.py into its own shared object with g++; the libraries export the C ABI only).
// Input: the Julia CSC patterns (1-based) of P (n x n) and A (m x n).  Output, sized by the caller: the value maps of the CSR copies of A and P and of
// the row-merged [P | A'] with their row pointers and the split positions.  Returns 0, or -1 (P) / -2 (A) for a malformed pattern.
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "value_maps.h"

extern "C" int value_maps_probe(int64_t n, int64_t m, const int64_t* P_colptr, const int64_t* P_rowval, const int64_t* A_colptr, const int64_t* A_rowval,
                                int32_t* A_rowptr /* m+1 */, int32_t* A_map /* nnzA */, int32_t* P_rowptr /* n+1 */, int32_t* P_map /* nnzP */,
                                int32_t* PT_rowptr /* n+1 */, int32_t* PT_split /* n */, int32_t* PT_map /* nnzP+nnzA */) {
  std::vector<int> arp, am, prp, pm, trp, tsp, tm;
  if (value_map_csr(n, n, P_colptr, P_rowval, prp, pm) != 0) return -1;
  if (value_map_csr(m, n, A_colptr, A_rowval, arp, am) != 0) return -2;
  value_map_merged(n, prp, pm, A_colptr, trp, tsp, tm);
  std::copy(arp.begin(), arp.end(), A_rowptr); std::copy(am.begin(), am.end(), A_map);
  std::copy(prp.begin(), prp.end(), P_rowptr); std::copy(pm.begin(), pm.end(), P_map);
  std::copy(trp.begin(), trp.end(), PT_rowptr); std::copy(tsp.begin(), tsp.end(), PT_split); std::copy(tm.begin(), tm.end(), PT_map);
  return 0;
}
