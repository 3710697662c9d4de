// ldl_analysis_probe.cpp -- test-only window onto the symbolic analysis of the direct KKT solver (csrc/ldl_symbolic.cpp, csrc/ldl.h).
//
// The C ABI reports eight figures of an analysis (cosmo_hip_ldl_analyze) but not the ordering it chose, and the structural tests
// (tests/ldl_structures.py) need exactly that: the reference factorisation of their error bound must eliminate in the library's order.
// tests/ldl_structures.py compiles this file together with ldl_symbolic.cpp (host C++, no GPU) into a temporary shared object; the library and
// its ABI stay as they are.
#include "ldl.h"

// P, A: CSC, 0-based (the arguments of cosmo_hip_ldl_analyze).  perm_in: NULL = the default ordering.
// perm_out[N]: the elimination order of the analysis (perm_out[k] = original index at position k; a postorder of the requested ordering's tree).
// figures[7]: {supernodes, most rows below the diagonal block of any supernode, most descendants of any supernode,
//              longest list rows_J[w .. nr) that some descendant's update searches (ldl_rowpos: the descendant has rows beyond J's columns),
//              most columns of a supernode that ONE descendant updates (r1 - r0: the gather loop of ldl_fwd_sn),
//              first column and row count of the widest supernode}.
extern "C" int ldl_probe(int64_t n, int64_t m, const int64_t* P_colptr, const int64_t* P_rowval, const int64_t* A_colptr, const int64_t* A_rowval,
                         const int64_t* perm_in, int64_t* perm_out, int64_t* figures) {
  std::vector<int64_t> pr, pc, ar, ac;
  for (int64_t j = 0; j < n; ++j)
    for (int64_t q = P_colptr[j]; q < P_colptr[j + 1]; ++q)
      if (P_rowval[q] < j) { pr.push_back(P_rowval[q]); pc.push_back(j); }
  for (int64_t j = 0; j < n; ++j)
    for (int64_t q = A_colptr[j]; q < A_colptr[j + 1]; ++q) { ar.push_back(A_rowval[q]); ac.push_back(j); }
  LdlSymbolic S;
  const char* err = nullptr;
  if (ldl_analyze(n, m, pr, pc, ar, ac, perm_in, S, &err) != 0) return -1;
  for (int64_t k = 0; k < S.N; ++k) perm_out[k] = S.perm[k];
  int64_t below = 0, ndesc = 0, searched = 0, gather = 0, wide = 0, wide_first = 0, wide_rows = 0;
  for (int64_t J = 0; J < S.ns; ++J) {
    const int64_t w = S.sn_first[J + 1] - S.sn_first[J], nr = S.sn_rp[J + 1] - S.sn_rp[J];
    if (nr - w > below) below = nr - w;
    if (w > wide) { wide = w; wide_first = S.sn_first[J]; wide_rows = nr; }
    if (S.desc_ptr[J + 1] - S.desc_ptr[J] > ndesc) ndesc = S.desc_ptr[J + 1] - S.desc_ptr[J];
    for (int64_t d = S.desc_ptr[J]; d < S.desc_ptr[J + 1]; ++d) {
      const int64_t K = S.desc[3 * d], r0 = S.desc[3 * d + 1], r1 = S.desc[3 * d + 2];
      if (r1 - r0 > gather) gather = r1 - r0;
      const int64_t tail = (S.sn_rp[K + 1] - S.sn_rp[K]) - r1;          // rows of K past J's columns: each one a search in rows_J[w .. nr)
      if (tail > 0 && nr - w > searched) searched = nr - w;
    }
  }
  figures[0] = S.ns; figures[1] = below; figures[2] = ndesc; figures[3] = searched; figures[4] = gather;
  figures[5] = wide_first; figures[6] = wide_rows;
  return 0;
}
