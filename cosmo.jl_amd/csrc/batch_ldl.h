// batch_ldl.h -- the direct KKT solver (QdldlKKTSolver, COSMO_HIP_KKT_DIRECT) inside the persistent batch kernels (batch.hip, opt-in through
// cosmo_hip_batch_set_direct).  Host side: batch_ldl.hip.
//
// One symbolic analysis per batch (ldl_analyze of ldl_symbolic.cpp) on the UNION of the members' patterns of K = [P + sigma I, A'; A, -diag(1 ./ rho)]
// (upper triangle of P, A): a member's missing entries are explicit zeros of its panels -- a quasi-definite K factorises under any symmetric
// permutation, so the factor of every member is exact.  Problem k owns one contiguous slab Lx + k * panel of the supernodal panels (ldl.h layout)
// and one permuted work vector y + k * N.  Its persistent workgroup walks the supernodes in postorder (column order: children before parents):
//   refill + factor (bldl_refill_factor): zero the slab, scatter P + sigma I, A and -1 ./ rho (the problem's own rho vector), then ldl_factor_sn of
//     every supernode -- at set-up (k_bldl_setup, the inertia check) and whenever the workgroup's adaptive-rho decision changed its rho (batch.hip);
//   solve (bldl_solve): y = [ls_x; ls_s][perm], ldl_fwd_sn over J = 0 .. ns-1, ldl_bwd_sn over J = ns-1 .. 0, then the unpermutation fused with
//     the full-KKT tail of k_mr_tail_full (x_tl, nu, s_tl, w).
// Parallelism comes from the batch: one problem per workgroup, the supernodes of a problem one after the other.
#pragma once
#include <string>
#include <vector>
#include "ldl_dev.h"

struct BLdlDev {                           // (plain data: a field of BatchDev, passed to kernels by value)
  int ns, N;
  long long panel;                       // reals per problem slab
  const int* sn_first;                   // ns + 1
  const long long* sn_rp;                // ns + 1
  const int* sn_rows;
  const long long* sn_poff;              // ns + 1
  const int* desc_ptr;
  const int* desc;
  const int* perm;                       // N: perm[k] = original index at position k
  const int* dslot;                      // n: slot of K(j, j), j < n (shared: the union pattern)
  const int* rslot;                      // m: slot of K(n + i, n + i)
  const int* pdiag;                      // nprob * n: position of P_jj among problem k's values of [P | A'] (BatchDev::PT), -1 if absent
  const int* pslot;                      // concatenated like BatchDev::PT values: slot of a strictly upper entry of P, -1 for every other entry
  const int* aslot;                      // concatenated like BatchDev::A values: slot of the entry of A
  real* Lx;                              // nprob * panel
  real* y;                               // nprob * N
  int* nfact;                            // nprob: factorisations so far
  int* npos;                             // nprob: positive pivots of the last factorisation
  int* fail;                             // nprob: 1 = a zero or non-finite pivot (the problem stopped)
};

// Refill problem k's slab from its P + sigma I, A and rho, then factorise it.  ptv / pnnz: problem k's values of [P | A'] (BatchDev::PT) and
// their count; av / annz: its values of A.  Returns the pivot error flag (block-uniform); thread 0 records the counters.
template <int BS>
__device__ __forceinline__ int bldl_refill_factor(const BLdlDev& L, int k, int n, int m, real sigma, const real* __restrict__ ptv, int pnnz,
                                                  const real* __restrict__ av, int annz, const real* __restrict__ rho, const long long pslot_off,
                                                  const long long aslot_off) {
  __shared__ int bad_s;
  const int tid = threadIdx.x;
  real* X = L.Lx + (long long)k * L.panel;
  const int* pd = L.pdiag + (long long)k * n;
  const int* ps = L.pslot + pslot_off;
  const int* as = L.aslot + aslot_off;
  __syncthreads();                                                        // (the caller's last reads of rho / the slab are behind us)
  for (long long i = tid; i < L.panel; i += BS) X[i] = R(0.0);
  __syncthreads();
  // every target slot is written by exactly one item: [x diagonal | upper off-diagonal P | A | rho diagonal] (k_ldl_refill)
  for (int i = tid; i < n; i += BS) { const int q = pd[i]; X[L.dslot[i]] = (q >= 0) ? ptv[q] + sigma : sigma; }
  for (int t = tid; t < pnnz; t += BS) { const int s = ps[t]; if (s >= 0) X[s] = ptv[t]; }
  for (int t = tid; t < annz; t += BS) X[as[t]] = av[t];
  for (int i = tid; i < m; i += BS) X[L.rslot[i]] = -(R(1.0) / rho[i]);
  __syncthreads();
  int pos = 0;
  bool bad = false;
  for (int J = 0; J < L.ns; ++J) ldl_factor_sn<BS>(J, L.sn_first, L.sn_rp, L.sn_rows, L.sn_poff, L.desc_ptr, L.desc, X, pos, bad);
  if (tid == 0) {
    L.nfact[k] += 1; L.npos[k] = pos;
    if (bad) L.fail[k] = 1;
    bad_s = bad ? 1 : 0;
  }
  __syncthreads();
  return bad_s;
}

// solve!(::QdldlKKTSolver) (kktsolver.jl:310-314) on the right-hand side [ls_x; ls_s] = [sigma w_x - q; (b - 2 s) + w_s] (solver.jl:50-51), then
// the rest of admm_x! / admm_w! (solver.jl:55,63-64) as k_mr_tail_full: x_tl = sol[1:n], nu = sol[n+1:end], s_tl = (2 s - w_s) - nu ./ rho, w update.
// w, s, q, b, rho, x_tl, nu, s_tl: problem k's slices.
template <int BS>
__device__ __forceinline__ void bldl_solve(const BLdlDev& L, int k, int n, real sigma, real alpha, real* __restrict__ w, const real* __restrict__ s,
                                           const real* __restrict__ q, const real* __restrict__ b, const real* __restrict__ rho, real* __restrict__ x_tl,
                                           real* __restrict__ nu, real* __restrict__ s_tl) {
  const int tid = threadIdx.x;
  const int N = L.N;
  const real* X = L.Lx + (long long)k * L.panel;
  real* y = L.y + (long long)k * N;
  for (int i = tid; i < N; i += BS) {
    const int p = L.perm[i];
    if (p < n) y[i] = sigma * w[p] - q[p];
    else { const int r = p - n; y[i] = (b[r] - R(2.0) * s[r]) + w[p]; }
  }
  __syncthreads();
  for (int J = 0; J < L.ns; ++J) ldl_fwd_sn<BS>(J, L.sn_first, L.sn_rp, L.sn_rows, L.sn_poff, L.desc_ptr, L.desc, X, y);
  __syncthreads();
  for (int J = L.ns - 1; J >= 0; --J) ldl_bwd_sn<BS>(J, L.sn_first, L.sn_rp, L.sn_rows, L.sn_poff, X, y);
  __syncthreads();
  for (int i = tid; i < N; i += BS) {
    const int p = L.perm[i];
    const real v = y[i];
    if (p < n) { x_tl[p] = v; const real wv = w[p]; w[p] = wv + alpha * (v - wv); }
    else {
      const int r = p - n;
      nu[r] = v;
      const real sv = s[r], wv = w[p];
      const real st = (R(2.0) * sv - wv) - v / rho[r];
      s_tl[r] = st;
      w[p] = wv + alpha * (st - sv);
    }
  }
  __syncthreads();
}

// ---- host side (batch_ldl.hip) ------------------------------------------------------------------------------------------------------------
struct BLdlPlan;
// Union analysis of the members' patterns (PT: per problem the CSR rows of [P | A'] with the split at the P part, A: per problem the CSR of A),
// refill maps, device arrays.  perm: empty = the default ordering.  Returns COSMO_HIP_OK, COSMO_HIP_ERR_INVALID (bad perm) or
// COSMO_HIP_ERR_UNSUPPORTED (over the storage budget; err says why); *out is the plan (also on failure: bldl_free it).
int32_t bldl_build(int nprob, long long n, long long m, const std::vector<HostCsr>& PT, const std::vector<HostCsr>& A, const std::vector<int64_t>& perm,
                   BLdlPlan** out, BLdlDev* dev, std::string& err);
// The first factorisation of every member and the inertia check (nnz(D > 0) == n, kktsolver.jl:304).  PT / A: the batch's device matrices.
int32_t bldl_setup_factor(BLdlPlan* p, const BLdlDev& dev, hipStream_t st, int nprob, int n, int m, real sigma, const int* PT_rowptr, const real* PT_val,
                          const long long* PT_nzoff, const int* A_rowptr, const real* A_val, const long long* A_nzoff, const real* rho, std::string& err);
// The same for `count` listed members only, on the kept analysis with their current rho (new matrix values: cosmo_hip_batch_apply_updates).  d_mem: the
// device list, member j at d_mem[j * stride]; h_mem: its host copy.  A listed member's pivot flag is cleared first, so a valid update restores a member
// that failed before.  INVALID names the first listed member that fails the pivot or the inertia check; the others are factorised all the same.
int32_t bldl_refactor_members(BLdlPlan* p, const BLdlDev& dev, hipStream_t st, int nprob, int count, const int* d_mem, int stride, const int* h_mem, int n, int m,
                              real sigma, const int* PT_rowptr, const real* PT_val, const long long* PT_nzoff, const int* A_rowptr, const real* A_val,
                              const long long* A_nzoff, const real* rho, std::string& err);
// out = {nnz(L), panel reals per problem, supernodes, tree height, widest supernode, analysis ns, factorisations (all members), min positive pivots}
int32_t bldl_info(BLdlPlan* p, const BLdlDev& dev, hipStream_t st, int nprob, int64_t* out, std::string& err);
int32_t bldl_counts(BLdlPlan* p, const BLdlDev& dev, hipStream_t st, int nprob, int64_t* out, std::string& err);
int bldl_first_failed(BLdlPlan* p, const BLdlDev& dev, hipStream_t st, int nprob);      // first member whose loop hit a bad pivot, -1: none
void bldl_free(BLdlPlan* p);
