// schur_plan.cpp -- host analysis of the Schur-complement KKT solver (see schur_plan.h): host only, pattern only.
#include "schur_plan.h"
#include <algorithm>
#include <numeric>
#include "../../include/cosmo_hip.h"

namespace {
int uf_find(std::vector<int>& parent, int i) {
  while (parent[i] != i) { parent[i] = parent[parent[i]]; i = parent[i]; }
  return i;
}
// the smaller index becomes the root: the root of a component is its smallest member, whatever the order of the unions
void uf_union(std::vector<int>& parent, int a, int b) {
  a = uf_find(parent, a); b = uf_find(parent, b);
  if (a == b) return;
  if (a < b) parent[b] = a; else parent[a] = b;
}
struct Term { int64_t e; int ta, tb, trow; };
}  // namespace

int64_t schur_dense_bytes(int64_t nd, int real_bytes) {
  const int64_t ndp = (nd + SCHUR_NB - 1) / SCHUR_NB * SCHUR_NB;
  return 2 * ndp * ndp * (int64_t)real_bytes;
}

int schur_check_limits(const SchurPlan& S, int64_t nd_max, int64_t block_max, int real_bytes) {
  if (S.nd > nd_max) return 1;
  if (S.largest > block_max) return 2;
  if (schur_dense_bytes(S.nd, real_bytes) > SCHUR_MEM_BUDGET) return 3;
  return 0;
}

int schur_analyze(int64_t n, int64_t m, const std::vector<int>& p_ptr, const std::vector<int>& p_col, const std::vector<int>& a_ptr,
                  const std::vector<int>& a_col, int row_threshold, SchurPlan& S, const char** err) {
  static const char* e_shape = "schur analysis: bad row pointers";
  static const char* e_index = "schur analysis: column index out of range";
  static const char* e_size = "schur analysis: the problem is out of int32 range";
  S = SchurPlan();
  if (row_threshold <= 0) row_threshold = SCHUR_ROW_THRESHOLD_DEFAULT;
  if (row_threshold < 2) row_threshold = 2;        // a row with one entry is a diagonal term of M_s and never long
  if (n < 0 || m < 0 || n >= 2147483647LL || m >= 2147483647LL) { if (err) *err = e_size; return -1; }
  if ((int64_t)p_ptr.size() != n + 1 || (int64_t)a_ptr.size() != m + 1 || p_ptr[0] != 0 || a_ptr[0] != 0) { if (err) *err = e_shape; return -1; }
  for (int64_t i = 0; i < n; ++i) if (p_ptr[i + 1] < p_ptr[i]) { if (err) *err = e_shape; return -1; }
  for (int64_t i = 0; i < m; ++i) if (a_ptr[i + 1] < a_ptr[i]) { if (err) *err = e_shape; return -1; }
  if ((int64_t)p_col.size() < p_ptr[n] || (int64_t)a_col.size() < a_ptr[m]) { if (err) *err = e_shape; return -1; }
  for (int k = 0; k < p_ptr[n]; ++k) if (p_col[k] < 0 || p_col[k] >= n) { if (err) *err = e_index; return -1; }
  for (int k = 0; k < a_ptr[m]; ++k) if (a_col[k] < 0 || a_col[k] >= n) { if (err) *err = e_index; return -1; }
  S.n = n; S.m = m; S.row_threshold = row_threshold;

  // 1. the components of pattern(M_s): P's off-diagonals and the short rows with more than one entry
  std::vector<int> parent((size_t)n);
  std::iota(parent.begin(), parent.end(), 0);
  for (int64_t i = 0; i < n; ++i)
    for (int k = p_ptr[i]; k < p_ptr[i + 1]; ++k) if (p_col[k] != i) uf_union(parent, (int)i, p_col[k]);
  for (int64_t i = 0; i < m; ++i) {
    const int len = a_ptr[i + 1] - a_ptr[i];
    if (len >= row_threshold) { S.ad_row.push_back((int)i); continue; }
    for (int k = a_ptr[i] + 1; k < a_ptr[i + 1]; ++k) uf_union(parent, a_col[a_ptr[i]], a_col[k]);
  }
  S.nd = (int64_t)S.ad_row.size();
  // sizes; blocks ordered by (size, smallest member), members ascending
  std::vector<int> root((size_t)n), size((size_t)n, 0);
  for (int64_t i = 0; i < n; ++i) { root[i] = uf_find(parent, (int)i); size[root[i]] += 1; }
  std::vector<int> roots;
  for (int64_t i = 0; i < n; ++i) if (root[i] == i) roots.push_back((int)i);
  std::stable_sort(roots.begin(), roots.end(), [&](int a, int b) { return size[a] != size[b] ? size[a] < size[b] : a < b; });
  S.ncomp = (int64_t)roots.size();
  std::vector<int> blk_of_root((size_t)n, -1);
  S.comp_ptr.assign((size_t)S.ncomp + 1, 0);
  S.boff.assign((size_t)S.ncomp + 1, 0);
  for (int64_t k = 0; k < S.ncomp; ++k) {
    const int s = size[roots[k]];
    blk_of_root[roots[k]] = (int)k;
    S.comp_ptr[k + 1] = S.comp_ptr[k] + s;
    S.boff[k + 1] = S.boff[k] + (int64_t)s * s;
    S.largest = std::max<int64_t>(S.largest, s);
    if (s <= SCHUR_SMALL_MAX) S.n_small = (int)k + 1;
    if (s <= SCHUR_WAVE_MAX) S.n_wave = (int)k + 1;
  }
  S.sumsq = S.boff[S.ncomp];
  S.perm.assign((size_t)n, 0); S.pos.assign((size_t)n, 0); S.blk_of_pos.assign((size_t)n, 0);
  {
    std::vector<int> fill(S.comp_ptr.begin(), S.comp_ptr.end() - 1);
    for (int64_t i = 0; i < n; ++i) {          // ascending i: the members of a block are ascending
      const int k = blk_of_root[root[i]];
      const int p = fill[k]++;
      S.perm[p] = (int)i; S.pos[i] = p; S.blk_of_pos[p] = k;
    }
  }
  auto entry_of = [&](int i, int j) -> int64_t {      // packed position of M_s(i, j); i and j are in the same block by construction
    const int k = S.blk_of_pos[S.pos[i]];
    const int s = S.comp_ptr[k + 1] - S.comp_ptr[k];
    return S.boff[k] + (int64_t)(S.pos[i] - S.comp_ptr[k]) * s + (S.pos[j] - S.comp_ptr[k]);
  };

  // 2. refill terms in a fixed order: sigma, then P by stored index, then the short rows by row and pair of stored entries
  std::vector<Term> terms;
  terms.reserve((size_t)n + (size_t)p_ptr[n] + (size_t)a_ptr[m]);
  for (int64_t i = 0; i < n; ++i) terms.push_back({entry_of((int)i, (int)i), 0, -2, 0});
  for (int64_t i = 0; i < n; ++i)
    for (int k = p_ptr[i]; k < p_ptr[i + 1]; ++k) terms.push_back({entry_of((int)i, p_col[k]), k, -1, 0});
  for (int64_t i = 0; i < m; ++i) {
    if (a_ptr[i + 1] - a_ptr[i] >= row_threshold) continue;
    for (int ka = a_ptr[i]; ka < a_ptr[i + 1]; ++ka)
      for (int kb = a_ptr[i]; kb < a_ptr[i + 1]; ++kb) terms.push_back({entry_of(a_col[ka], a_col[kb]), ka, kb, (int)i});
  }
  std::stable_sort(terms.begin(), terms.end(), [](const Term& a, const Term& b) { return a.e < b.e; });
  S.ta.resize(terms.size()); S.tb.resize(terms.size()); S.trow.resize(terms.size());
  for (size_t t = 0; t < terms.size(); ++t) {
    if (t == 0 || terms[t].e != terms[t - 1].e) { S.epos.push_back(terms[t].e); S.eptr.push_back((int64_t)t); }
    S.ta[t] = terms[t].ta; S.tb[t] = terms[t].tb; S.trow[t] = terms[t].trow;
  }
  S.eptr.push_back((int64_t)terms.size());

  // 3. A_d and A_d' as index lists into A's CSR; nnz(W = M_s^-1 A_d'): a long row fills the blocks it touches
  S.ad_ptr.assign((size_t)S.nd + 1, 0);
  std::vector<int> cnt((size_t)n + 1, 0), mark((size_t)S.ncomp, -1);
  for (int64_t kd = 0; kd < S.nd; ++kd) {
    const int i = S.ad_row[kd];
    for (int k = a_ptr[i]; k < a_ptr[i + 1]; ++k) {
      S.ad_col.push_back(a_col[k]); S.ad_src.push_back(k);
      cnt[a_col[k] + 1] += 1;
      const int b = S.blk_of_pos[S.pos[a_col[k]]];
      if (mark[b] != (int)kd) { mark[b] = (int)kd; S.nnz_w += S.comp_ptr[b + 1] - S.comp_ptr[b]; }
    }
    S.ad_ptr[kd + 1] = (int)S.ad_col.size();
  }
  S.adt_ptr.assign((size_t)n + 1, 0);
  for (int64_t j = 0; j < n; ++j) S.adt_ptr[j + 1] = S.adt_ptr[j] + cnt[j + 1];
  S.adt_k.resize(S.ad_col.size()); S.adt_src.resize(S.ad_col.size());
  {
    std::vector<int> fill(S.adt_ptr.begin(), S.adt_ptr.end() - 1);
    for (int64_t kd = 0; kd < S.nd; ++kd)
      for (int p = S.ad_ptr[kd]; p < S.ad_ptr[kd + 1]; ++p) { const int q = fill[S.ad_col[p]]++; S.adt_k[q] = (int)kd; S.adt_src[q] = S.ad_src[p]; }
  }
  return 0;
}

// out = {nd, components of M_s, largest component, sum of size^2, nnz(M_s^-1 A_d'), bytes of C plus C^-1 in this library's scalar type,
//        1 if the default limits accept the plan (else 0), components of side <= 3}
extern "C" COSMO_HIP_API int32_t cosmo_hip_schur_analyze(int64_t n, int64_t m, const int64_t* P_colptr, const int64_t* P_rowval, const int64_t* A_colptr,
                                                        const int64_t* A_rowval, int32_t row_threshold, int64_t* out) {
  if (n < 0 || m < 0 || n >= 2147483647LL || m >= 2147483647LL || !P_colptr || !A_colptr || !out) return COSMO_HIP_ERR_INVALID;
  if (P_colptr[n] >= 2147483647LL || A_colptr[n] >= 2147483647LL || P_colptr[0] != 0 || A_colptr[0] != 0) return COSMO_HIP_ERR_INVALID;
  // CSC -> CSR (pattern): within a row the columns come out ascending
  std::vector<int> pp((size_t)n + 1, 0), ap((size_t)m + 1, 0), pc((size_t)P_colptr[n]), ac((size_t)A_colptr[n]);
  for (int64_t j = 0; j < n; ++j) {
    if (P_colptr[j + 1] < P_colptr[j] || A_colptr[j + 1] < A_colptr[j]) return COSMO_HIP_ERR_INVALID;
    for (int64_t q = P_colptr[j]; q < P_colptr[j + 1]; ++q) { if (P_rowval[q] < 0 || P_rowval[q] >= n) return COSMO_HIP_ERR_INVALID; pp[P_rowval[q] + 1] += 1; }
    for (int64_t q = A_colptr[j]; q < A_colptr[j + 1]; ++q) { if (A_rowval[q] < 0 || A_rowval[q] >= m) return COSMO_HIP_ERR_INVALID; ap[A_rowval[q] + 1] += 1; }
  }
  for (int64_t i = 0; i < n; ++i) pp[i + 1] += pp[i];
  for (int64_t i = 0; i < m; ++i) ap[i + 1] += ap[i];
  {
    std::vector<int> fp(pp.begin(), pp.end() - 1), fa(ap.begin(), ap.end() - 1);
    for (int64_t j = 0; j < n; ++j) {
      for (int64_t q = P_colptr[j]; q < P_colptr[j + 1]; ++q) pc[fp[P_rowval[q]]++] = (int)j;
      for (int64_t q = A_colptr[j]; q < A_colptr[j + 1]; ++q) ac[fa[A_rowval[q]]++] = (int)j;
    }
  }
  SchurPlan S;
  const char* err = nullptr;
  if (schur_analyze(n, m, pp, pc, ap, ac, row_threshold, S, &err) != 0) return COSMO_HIP_ERR_INVALID;
  out[0] = S.nd; out[1] = S.ncomp; out[2] = S.largest; out[3] = S.sumsq; out[4] = S.nnz_w;
  out[5] = schur_dense_bytes(S.nd, (int)sizeof(cosmo_hip_real));
  out[6] = schur_check_limits(S, SCHUR_ND_MAX_DEFAULT, SCHUR_BLOCK_MAX_DEFAULT, (int)sizeof(cosmo_hip_real)) == 0 ? 1 : 0;
  out[7] = S.n_small;
  return COSMO_HIP_OK;
}
