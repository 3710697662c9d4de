// value_maps.cpp -- see value_maps.h
#include "value_maps.h"

int value_map_csr(int64_t nr, int64_t nc, const int64_t* colptr, const int64_t* rowval, std::vector<int>& rowptr, std::vector<int>& map) {
  if (nr < 0 || nc < 0 || !colptr || colptr[0] != 1) return -1;
  for (int64_t j = 0; j < nc; ++j) if (colptr[j + 1] < colptr[j]) return -1;
  const int64_t nnz = colptr[nc] - 1;
  if (nnz >= (int64_t)2147483647 || (nnz > 0 && !rowval)) return -1;
  std::vector<int> rp((size_t)nr + 1, 0);
  for (int64_t k = 0; k < nnz; ++k) {
    const int64_t i = rowval[k] - 1;
    if (i < 0 || i >= nr) return -1;
    rp[(size_t)i + 1]++;
  }
  for (int64_t i = 0; i < nr; ++i) rp[(size_t)i + 1] += rp[(size_t)i];
  std::vector<int> pos(rp.begin(), rp.end() - 1), mp((size_t)nnz);
  for (int64_t j = 0; j < nc; ++j)
    for (int64_t k = colptr[j] - 1; k < colptr[j + 1] - 1; ++k) mp[(size_t)pos[(size_t)(rowval[k] - 1)]++] = (int)k;
  rowptr.swap(rp);
  map.swap(mp);
  return 0;
}

void value_map_merged(int64_t n, const std::vector<int>& p_rowptr, const std::vector<int>& p_map, const int64_t* a_colptr, std::vector<int>& rowptr,
                      std::vector<int>& split, std::vector<int>& map) {
  rowptr.assign((size_t)n + 1, 0);
  split.assign((size_t)n, 0);
  map.clear();
  map.reserve(p_map.size() + (size_t)(n > 0 ? a_colptr[n] - 1 : 0));
  for (int64_t j = 0; j < n; ++j) {
    rowptr[(size_t)j] = (int)map.size();
    for (int k = p_rowptr[(size_t)j]; k < p_rowptr[(size_t)j + 1]; ++k) map.push_back(p_map[(size_t)k]);
    split[(size_t)j] = (int)map.size();
    for (int64_t k = a_colptr[j] - 1; k < a_colptr[j + 1] - 1; ++k) map.push_back((int)k);
  }
  rowptr[(size_t)n] = (int)map.size();
}
