// update.hip -- cosmo_hip_update_matrices: new VALUES for the stored entries of P and A on a set-up handle (same pattern), without a new set-up.
// The caller's arrays are uploaded once; every resident copy and every value array the host computed at set-up time is then refilled on the device
// through index maps that were recorded when it was built (value_maps.h for the four copies, build_op_split / fold_build for the reduced operator):
//     A, A', P, [P | A']              val[p] = scale(new[src[p]])                                    (k_upd_copy)
//     Am, [P | Am'], Ad               gathers from A.val / P.val / Am.val                            (k_upd_copy, unscaled)
//     op_sc_a2                        a * a of the row's single entry                                (k_upd_square)
//     FoldPlan::tprod, FoldPlan::base a_ki * a_kj ; P entries summed left to right                  (k_upd_tprod, k_upd_base)
// Each pass performs the floating-point operations of the host build in the same order (this file compiles under -ffp-contract=off like the rest), so
// a handle that was updated holds the bits of a handle that was set up with the new values.  One thread per destination entry, coalesced stores,
// gathers inside an nnz-sized array, no atomics; capped grid-stride launches as in scaling.hip.
#include "device_utils.h"
#include <algorithm>
#include <vector>

namespace {

inline int egrid(long long n) { long long g = (n + COSMO_BS - 1) / COSMO_BS; return (int)std::max<long long>(1, std::min<long long>(g, 4096)); }

// row of the CSR entry p: the r with rowptr[r] <= p < rowptr[r + 1] (empty rows share a boundary: the last of them that starts at or before p holds it)
__device__ __forceinline__ int row_of(const int* __restrict__ rowptr, int nrows, int p) {
  int lo = 0, hi = nrows;
  while (hi - lo > 1) { const int mid = lo + ((hi - lo) >> 1); if (rowptr[mid] <= p) lo = mid; else hi = mid; }
  return lo;
}

// val[p] = scale(new[src[p]]) over one CSR array.  Entries with col < split_col take new1 (src indexes it), the others new2 (the A' part of a merged
// operator); a null new1 / new2 leaves its entries alone, a null src is the identity.  scale != 0 (apply_scaling), with (r, c) the entry's row and column:
//     col <  split_col :  v * (rowf[r] * colf[c]) * cs        -- P: (p * (D_i * D_j)) * c ; A: a * (E_i * D_j), cs = 1 ; A': a * (D_r * E_c), cs = 1
//     col >= split_col :  v * (colf2[c - split_col] * rowf[r]) -- the A' part of [P | A']: a * (E_i * D_j)
// the expressions of k_scale_csr (scaling.hip) and of model._scale_csc followed by P.data *= c; products of two factors commute bit for bit.
__global__ __launch_bounds__(COSMO_BS) void k_upd_copy(long long nnz, int nrows, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                       real* __restrict__ val, const int* __restrict__ src, const real* __restrict__ new1,
                                                       const real* __restrict__ new2, int split_col, int scale, const real* __restrict__ rowf,
                                                       const real* __restrict__ colf, const real* __restrict__ colf2, real cs) {
  for (long long p = (long long)blockIdx.x * COSMO_BS + threadIdx.x; p < nnz; p += (long long)gridDim.x * COSMO_BS) {
    const int c = col[p];
    const bool first = c < split_col;
    const real* __restrict__ nv = first ? new1 : new2;
    if (!nv) continue;
    real v = nv[src ? src[p] : (int)p];
    if (scale) {
      const int r = row_of(rowptr, nrows, (int)p);
      if (first) { v = v * (rowf[r] * colf[c]); v = v * cs; }
      else v = v * (colf2[c - split_col] * rowf[r]);
    }
    val[p] = v;
  }
}

// op_sc_a2[p] = a * a, a = the single entry of row sc_row[p] of A: it sits at A.rowptr[row], so this pass needs no map of its own (build_op_split)
__global__ __launch_bounds__(COSMO_BS) void k_upd_square(long long n, const int* __restrict__ sc_row, const int* __restrict__ a_rowptr, const real* __restrict__ a,
                                                         real* __restrict__ out) {
  for (long long p = (long long)blockIdx.x * COSMO_BS + threadIdx.x; p < n; p += (long long)gridDim.x * COSMO_BS) { const real v = a[a_rowptr[sc_row[p]]]; out[p] = v * v; }
}

// tprod[t] = a_ki * a_kj in the operand order of fold_build; the single entry of a factored row where tb[t] < 0
__global__ __launch_bounds__(COSMO_BS) void k_upd_tprod(long long nt, const int* __restrict__ ta, const int* __restrict__ tb, const real* __restrict__ a,
                                                        real* __restrict__ tprod) {
  for (long long t = (long long)blockIdx.x * COSMO_BS + threadIdx.x; t < nt; t += (long long)gridDim.x * COSMO_BS) {
    const real aki = a[ta[t]];
    const int q = tb[t];
    tprod[t] = q < 0 ? aki : aki * a[q];
  }
}

// base[p] = the entries of P at (row, column) of M's entry p, summed left to right from 0 as fold_build does (0 where P has none)
__global__ __launch_bounds__(COSMO_BS) void k_upd_base(long long nnz, const int* __restrict__ bptr, const int* __restrict__ bsrc,
                                                       const real* __restrict__ pval, real* __restrict__ base) {
  for (long long p = (long long)blockIdx.x * COSMO_BS + threadIdx.x; p < nnz; p += (long long)gridDim.x * COSMO_BS) {
    real b = 0.0;
    for (int k = bptr[p]; k < bptr[p + 1]; ++k) b += pval[bsrc[k]];
    base[p] = b;
  }
}

// first use: the device copy of a host map (the host copy stays: kkt_configure may rebuild the operator and with it the maps)
int32_t up_map(cosmo_hip_handle* h, int** dst, const std::vector<int>& v) {
  if (*dst) return COSMO_HIP_OK;
  HIPCHK(h, hipMalloc((void**)dst, std::max<size_t>(v.size(), 1) * sizeof(int)));
  if (!v.empty()) HIPCHK(h, hipMemcpyAsync(*dst, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->upd_last_bytes += (long long)(v.size() * sizeof(int));
  return COSMO_HIP_OK;
}
void drop_map(int** p) { if (*p) { (void)hipFree(*p); *p = nullptr; } }
long long held(const int* dev, const std::vector<int>& v) { return dev ? (long long)(v.size() * sizeof(int)) : 0; }

void copy_pass(cosmo_hip_handle* h, const CsrDev& M, const int* src, const real* new1, const real* new2, int split_col, int scale, const real* rowf,
               const real* colf, const real* colf2, real cs) {
  if (M.nnz <= 0) return;
  hipLaunchKernelGGL(k_upd_copy, dim3(egrid(M.nnz)), dim3(COSMO_BS), 0, h->stream, M.nnz, M.nrows, (const int*)M.rowptr, (const int*)M.col, M.val, src, new1,
                     new2, split_col, scale, rowf, colf, colf2, cs);
}

}  // namespace

void upd_free_split(cosmo_hip_handle* h) {
  drop_map(&h->u_am); drop_map(&h->u_ptm);
  h->vm_am.clear(); h->vm_ptm.clear();
}

void upd_free_fold(FoldPlan* f) { drop_map(&f->u_ta); drop_map(&f->u_tb); drop_map(&f->u_bptr); drop_map(&f->u_bsrc); drop_map(&f->u_ad); }

void upd_free(cosmo_hip_handle* h) {
  upd_free_split(h);
  drop_map(&h->u_A); drop_map(&h->u_P); drop_map(&h->u_PT);
  h->vm_A.clear(); h->vm_P.clear(); h->vm_PT.clear();
  if (h->u_newP) { (void)hipFree(h->u_newP); h->u_newP = nullptr; }
  if (h->u_newA) { (void)hipFree(h->u_newA); h->u_newA = nullptr; }
}

// The value arrays of the reduced operator, from the refreshed A.val / P.val; refresh_op_split (the caller: kkt_update_values) then forms the
// rho-dependent values from them exactly as after set_params.
int32_t upd_refresh_operator(cosmo_hip_handle* h) {
  if (!h->op_split) return COSMO_HIP_OK;               // the unsplit routes apply A and [P | A'] themselves
  hipStream_t st = h->stream;
  CHK(up_map(h, &h->u_am, h->vm_am)); CHK(up_map(h, &h->u_ptm, h->vm_ptm));
  copy_pass(h, h->Am, h->u_am, h->A.val, nullptr, INT32_MAX, 0, nullptr, nullptr, nullptr, R(1.0));
  copy_pass(h, h->PTm, h->u_ptm, h->P.val, h->A.val, (int)h->n, 0, nullptr, nullptr, nullptr, R(1.0));
  if (h->op_nsingle > 0) hipLaunchKernelGGL(k_upd_square, dim3(egrid(h->op_nsingle)), dim3(COSMO_BS), 0, st, h->op_nsingle, (const int*)h->op_sc_row, (const int*)h->A.rowptr, (const real*)h->A.val, h->op_sc_a2);
  h->upd_refreshed += 3;
  FoldPlan* f = (FoldPlan*)h->fold;
  if (h->op_fold && f) {
    CHK(up_map(h, &f->u_ta, f->m_ta)); CHK(up_map(h, &f->u_tb, f->m_tb)); CHK(up_map(h, &f->u_bptr, f->m_bptr)); CHK(up_map(h, &f->u_bsrc, f->m_bsrc));
    CHK(up_map(h, &f->u_ad, f->m_ad));
    if (f->nterms > 0) hipLaunchKernelGGL(k_upd_tprod, dim3(egrid(f->nterms)), dim3(COSMO_BS), 0, st, f->nterms, (const int*)f->u_ta, (const int*)f->u_tb, (const real*)h->Am.val, f->tprod);
    if (f->M.nnz > 0) hipLaunchKernelGGL(k_upd_base, dim3(egrid(f->M.nnz)), dim3(COSMO_BS), 0, st, f->M.nnz, (const int*)f->u_bptr, (const int*)f->u_bsrc, (const real*)h->P.val, f->base);
    h->upd_refreshed += 2;
    if (f->nd > 0) { copy_pass(h, f->Ad, f->u_ad, h->Am.val, nullptr, INT32_MAX, 0, nullptr, nullptr, nullptr, R(1.0)); CHK(fold_ad_image_refresh(h)); h->upd_refreshed += 1; }
  }
  HIPCHK(h, hipGetLastError());
  return COSMO_HIP_OK;
}

// INVARIANT: no device array that existed before the call is freed, moved or resized -- the four copies, the split and the assembled operator, the
// direct solver's panels are all rewritten in place --, so captured launch chains (cg_fold.hip: fold_chain_ready, cg_sr.hip) keep valid pointers.
// The only allocations are the maps and the two staging arrays of the FIRST update.  Like cosmo_hip_update_qb the call leaves rho, the iterates
// (have_iterates), the Krylov warm start, the solve counter and the accelerator alone.
extern "C" int32_t cosmo_hip_update_matrices(cosmo_hip_handle* h, const real* P_nzval, const real* A_nzval, int32_t apply_scaling) {
  if (!h) return COSMO_HIP_ERR_INVALID;
  if (hipSetDevice(h->device) != hipSuccess) return cosmo_fail(h, COSMO_HIP_ERR_HIP, "hipSetDevice failed");
  if (h->row_shard) return cosmo_fail(h, COSMO_HIP_ERR_UNSUPPORTED, "update_matrices: not available on a row-sharded handle");
  if (!h->have_problem) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "set_problem first");
  const long long nnzP = h->P.nnz, nnzA = h->A.nnz;
  if (nnzP == 0) P_nzval = nullptr;
  if (nnzA == 0) A_nzval = nullptr;
  if (!P_nzval && !A_nzval) return COSMO_HIP_OK;
  if ((long long)h->vm_P.size() != nnzP || (long long)h->vm_A.size() != nnzA || (long long)h->vm_PT.size() != nnzP + nnzA)
    return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "update_matrices: the handle has no value maps for its matrices");
  hipStream_t st = h->stream;
  h->upd_last_bytes = 0;
  // maps and staging (first update only), then the new values
  if (P_nzval) {
    CHK(up_map(h, &h->u_P, h->vm_P));
    if (!h->u_newP) HIPCHK(h, hipMalloc((void**)&h->u_newP, sizeof(real) * (size_t)nnzP));
    HIPCHK(h, hipMemcpyAsync(h->u_newP, P_nzval, sizeof(real) * (size_t)nnzP, hipMemcpyHostToDevice, st));
    h->upd_last_bytes += (long long)sizeof(real) * nnzP;
  }
  if (A_nzval) {
    CHK(up_map(h, &h->u_A, h->vm_A));
    if (!h->u_newA) HIPCHK(h, hipMalloc((void**)&h->u_newA, sizeof(real) * (size_t)nnzA));
    HIPCHK(h, hipMemcpyAsync(h->u_newA, A_nzval, sizeof(real) * (size_t)nnzA, hipMemcpyHostToDevice, st));
    h->upd_last_bytes += (long long)sizeof(real) * nnzA;
  }
  CHK(up_map(h, &h->u_PT, h->vm_PT));
  const int sc = (apply_scaling && h->has_scaling) ? 1 : 0;
  const real* D = h->Dscale;
  const real* E = h->Escale;
  const real cs = sc ? (real)h->cscale : R(1.0);
  const real* nP = P_nzval ? h->u_newP : nullptr;
  const real* nA = A_nzval ? h->u_newA : nullptr;
  if (nA) {
    copy_pass(h, h->A, h->u_A, nA, nullptr, INT32_MAX, sc, E, D, nullptr, R(1.0));          // entry (i, j): a * (E_i * D_j)
    copy_pass(h, h->AT, nullptr, nA, nullptr, INT32_MAX, sc, D, E, nullptr, R(1.0));        // A' shares the caller's order; row = j, column = i
  }
  if (nP) copy_pass(h, h->P, h->u_P, nP, nullptr, INT32_MAX, sc, D, D, nullptr, cs);
  copy_pass(h, h->PT, h->u_PT, nP, nA, (int)h->n, sc, D, D, E, cs);
  HIPCHK(h, hipGetLastError());
  // issymmetric(P) of the new values, from the caller's array through the map of the P copy (P' is the caller's order itself)
  if (P_nzval) {
    bool sym = h->P_pattern_symmetric;
    for (long long p = 0; sym && p < nnzP; ++p) sym = P_nzval[h->vm_P[(size_t)p]] == P_nzval[p];
    h->P_symmetric = sym;
  }
  HIPCHK(h, hipStreamSynchronize(st));             // the caller's arrays are not retained
  h->upd_count += 1;
  if (!h->have_params && !h->upd_lost_params) return COSMO_HIP_OK;     // before set_params: the route is built later from the copies, as always
  const bool lost = h->upd_lost_params;
  if (lost) h->have_params = true;
  const int32_t rc = kkt_update_values(h);
  if (rc != COSMO_HIP_OK) { h->have_params = false; h->have_iterates = false; h->upd_lost_params = true; return rc; }
  h->upd_lost_params = false;
  return COSMO_HIP_OK;
}

extern "C" int32_t cosmo_hip_update_matrices_info(cosmo_hip_handle* h, int64_t out[8]) {
  if (!h || !out) return h ? cosmo_fail(h, COSMO_HIP_ERR_INVALID, "update_matrices_info: null output") : COSMO_HIP_ERR_INVALID;
  long long bytes = held(h->u_A, h->vm_A) + held(h->u_P, h->vm_P) + held(h->u_PT, h->vm_PT) + held(h->u_am, h->vm_am) + held(h->u_ptm, h->vm_ptm);
  if (const FoldPlan* f = (const FoldPlan*)h->fold)
    bytes += held(f->u_ta, f->m_ta) + held(f->u_tb, f->m_tb) + held(f->u_bptr, f->m_bptr) + held(f->u_bsrc, f->m_bsrc) + held(f->u_ad, f->m_ad);
  out[0] = h->upd_count; out[1] = h->upd_refreshed; out[2] = h->upd_host_rebuilds; out[3] = h->upd_last_bytes; out[4] = bytes;
  out[5] = h->ldl_analyses; out[6] = 0; out[7] = 0;
  return COSMO_HIP_OK;
}
