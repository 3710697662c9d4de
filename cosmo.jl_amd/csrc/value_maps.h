// value_maps.h -- where every stored entry of the resident CSR copies comes from in the caller's CSC value arrays (host code, pattern only; no HIP
// headers, the same object in both libraries).  cosmo_hip_set_problem stages A (m x n), A' (n x m), P (n x n) and the row-merged [P | A'] from the
// Julia CSC arrays it receives; cosmo_hip_update_matrices refills the same four copies from new value arrays of the same pattern through these maps.
// The maps are per STORED entry: duplicate entries and unsorted row indices inside a column (the C ABI passes both through) keep their own slots.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

// CSC (1-based, as cosmo_hip_set_problem takes it) of an (nr x nc) matrix -> rowptr of its CSR copy and, for every CSR entry p, the index map[p] of its
// source in nzval.  The placement is the one of csc_to_csr_pair (api.hip): columns ascending, entries of a column in their stored order.  The CSR of the
// TRANSPOSE shares the CSC arrays, so its map is the identity and is not built.  Returns 0, or -1 for a malformed pattern (nothing is written then).
int value_map_csr(int64_t nr, int64_t nc, const int64_t* colptr, const int64_t* rowval, std::vector<int>& rowptr, std::vector<int>& map);

// Row-merged [P | A'] (n x (n + m)): row j = (row j of the CSR copy of P) ++ (column j of A in its stored order).  map[p] indexes P's value array where
// entry p lies in the P part and A's value array where it lies in the A' part; split[j] = first entry of the A' part of row j.
void value_map_merged(int64_t n, const std::vector<int>& p_rowptr, const std::vector<int>& p_map, const int64_t* a_colptr, std::vector<int>& rowptr,
                      std::vector<int>& split, std::vector<int>& map);
