// ldl.hip -- the direct KKT solver COSMO_HIP_KKT_DIRECT: QdldlKKTSolver (src/linear_solver/kktsolver.jl:285-320) on the device.
//
// Setup (ldl_setup, once per set_params): the symbolic analysis of ldl_symbolic.cpp on the patterns of P and A, the refill maps, one
// numeric factorisation and the inertia check of the reference (:304: nnz(D > 0) must be n, else "Objective function is not convex.").
//
// Numeric factorisation (ldl_enqueue_refactor): k_ldl_zero + k_ldl_refill scatter P + sigma I, A and -1 ./ rho into the supernodal panels
// (ldl.h), then one k_ldl_factor launch per level of the supernodal tree, one workgroup per supernode, left-looking:
//   1. for every descendant K of J in ascending order: panel_J -= L_K[r0:, :] D_K L_K[r0:r1, :]'  (each entry of the update is owned by one
//      thread; a barrier between descendants; no atomics, fixed summation order => the factor is bitwise reproducible);
//   2. dense LDL' of the diagonal block without pivoting (K is quasi-definite: it exists for every symmetric permutation) and the scaling
//      of the panel below it.
// In the loop the three kernels read Ctl::rho_changed (set by the adaptive-rho check, kernels.hip) and return at once when it is clear: a
// refactorisation happens exactly when rho changed, without a host round trip.
//
// Solve (ldl_enqueue_solve, every ADMM iteration): k_ldl_perm (y = rhs[perm]), one k_ldl_fwd launch per level upwards (L y = b, gathering
// the descendants' contributions), one k_ldl_bwd launch per level downwards (D^-1 fused: x_J = D_J^-1 y_J - L_J' x), k_ldl_unperm
// (sol[perm] = x), then the full-KKT tail of the MINRES path (minres.hip: k_mr_tail_full, sol = [x_tl; nu]).
//
// Bytes per solve: the panels are read twice (forward + backward: 2 * nnz_stored reals), y / x a few times per level (sum of the supernodes'
// row counts).  Per factorisation: entry (a, b) of the update of J by descendant K recomputes its own sum over the wk columns of K, so the
// pair (K, J) reads O(na * nb * wk) panel values (na = rows of K from r0 on, nb = r1 - r0) -- not O(na * wk): no reuse through LDS or
// registers yet.  Together with the single workgroup of a wide supernode this is why BASELINE config 5 factorises slowly.
#include "device_utils.h"
#include "ldl.h"
#include "ldl_dev.h"
#include <chrono>
#include <math.h>

#define LDL_BS 256

struct LdlPlan {
  LdlSymbolic S;
  std::vector<int64_t> perm_req;     // the permutation asked for through cosmo_hip_set_kkt_perm (empty: default ordering)
  real* Lx = nullptr;                // panels
  int* sn_first = nullptr;           // ns + 1
  long long* sn_rp = nullptr;        // ns + 1
  int* sn_rows = nullptr;
  long long* sn_poff = nullptr;      // ns + 1
  int* lvl_sn = nullptr;
  int* desc_ptr = nullptr;
  int* desc = nullptr;
  int* perm = nullptr;               // N
  int* pdiag = nullptr;              // n: CSR index of P_jj in h->P, -1 if absent
  long long* dslot = nullptr;        // n
  long long np = 0;
  int* psrc = nullptr;               // np: CSR index of an upper off-diagonal entry of P
  long long* pslot = nullptr;        // np
  long long* aslot = nullptr;        // nnz(A): CSR order of h->A
  long long* rslot = nullptr;        // m
  real* y = nullptr;                 // N: permuted work vector
  real* sol = nullptr;               // N: solution in the original order
  int* dstat = nullptr;              // {pivot error, positive pivots, factorisations}
  double last_factor_s = 0.0;
  bool complete = false;             // every array above is allocated and uploaded
};

static LdlPlan* plan_of(cosmo_hip_handle* h) { return (LdlPlan*)h->ldl; }

template <class T>
static int32_t up(cosmo_hip_handle* h, T** dst, const T* src, size_t count) {
  HIPCHK(h, hipMalloc((void**)dst, sizeof(T) * (count > 0 ? count : 1)));
  if (count) HIPCHK(h, hipMemcpy(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice));
  return COSMO_HIP_OK;
}
template <class T>
static void dfree(T** p) { if (*p) { (void)hipFree(*p); *p = nullptr; } }

void ldl_free(cosmo_hip_handle* h) {
  LdlPlan* L = plan_of(h);
  if (!L) return;
  dfree(&L->Lx); dfree(&L->sn_first); dfree(&L->sn_rp); dfree(&L->sn_rows); dfree(&L->sn_poff); dfree(&L->lvl_sn); dfree(&L->desc_ptr);
  dfree(&L->desc); dfree(&L->perm); dfree(&L->pdiag); dfree(&L->dslot); dfree(&L->psrc); dfree(&L->pslot); dfree(&L->aslot); dfree(&L->rslot);
  dfree(&L->y); dfree(&L->sol); dfree(&L->dstat);
  delete L;
  h->ldl = nullptr;
}

// ---- kernels --------------------------------------------------------------------------------------------------------
// cond = 1 (in the loop): run only when the adaptive-rho check of this iteration changed rho
__device__ __forceinline__ bool ldl_skip(const Ctl* ctl, int cond) { return cond && (ctl->halt || !ctl->rho_changed); }

__global__ __launch_bounds__(LDL_BS) void k_ldl_zero(const Ctl* __restrict__ ctl, int cond, long long size, real* __restrict__ Lx,
                                                     int* __restrict__ dstat) {
  if (ldl_skip(ctl, cond)) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) { dstat[0] = 0; dstat[1] = 0; dstat[2] += 1; }
  for (long long i = (long long)blockIdx.x * LDL_BS + threadIdx.x; i < size; i += (long long)gridDim.x * LDL_BS) Lx[i] = R(0.0);
}

// every target slot is written by exactly one item: [x diagonal | upper off-diagonal P | A | rho diagonal]
__global__ __launch_bounds__(LDL_BS) void k_ldl_refill(const Ctl* __restrict__ ctl, int cond, long long n, long long np, long long na, long long m,
                                                       real sigma, const real* __restrict__ Pval, const int* __restrict__ pdiag,
                                                       const long long* __restrict__ dslot, const int* __restrict__ psrc,
                                                       const long long* __restrict__ pslot, const real* __restrict__ Aval,
                                                       const long long* __restrict__ aslot, const real* __restrict__ rho,
                                                       const long long* __restrict__ rslot, real* __restrict__ Lx) {
  if (ldl_skip(ctl, cond)) return;
  const long long tot = n + np + na + m;
  for (long long i = (long long)blockIdx.x * LDL_BS + threadIdx.x; i < tot; i += (long long)gridDim.x * LDL_BS) {
    if (i < n) {
      const int k = pdiag[i];
      Lx[dslot[i]] = (k >= 0) ? Pval[k] + sigma : sigma;
    } else if (i < n + np) {
      const long long k = i - n;
      Lx[pslot[k]] = Pval[psrc[k]];
    } else if (i < n + np + na) {
      const long long k = i - n - np;
      Lx[aslot[k]] = Aval[k];
    } else {
      const long long k = i - n - np - na;
      Lx[rslot[k]] = -(R(1.0) / rho[k]);
    }
  }
}

__global__ __launch_bounds__(LDL_BS) void k_ldl_factor(Ctl* __restrict__ ctl, int cond, const int* __restrict__ lvl, const int* __restrict__ sn_first,
                                                       const long long* __restrict__ sn_rp, const int* __restrict__ sn_rows,
                                                       const long long* __restrict__ sn_poff, const int* __restrict__ desc_ptr,
                                                       const int* __restrict__ desc, real* __restrict__ Lx, int* __restrict__ dstat) {
  if (ldl_skip(ctl, cond)) return;
  int pos = 0;
  bool bad = false;
  ldl_factor_sn<LDL_BS>(lvl[blockIdx.x], sn_first, sn_rp, sn_rows, sn_poff, desc_ptr, desc, Lx, pos, bad);
  if (threadIdx.x == 0) {
    if (pos) atomicAdd(&dstat[1], pos);               // integer count of positive pivots (inertia check)
    if (bad) {
      dstat[0] = 1;
      if (cond) { ctl->error = COSMO_HIP_ERR_INVALID; ctl->halt = 1; }
    }
  }
}

__global__ __launch_bounds__(LDL_BS) void k_ldl_perm(const Ctl* __restrict__ ctl, int guard, long long N, long long n, const int* __restrict__ perm,
                                                     const real* __restrict__ bx, const real* __restrict__ bs, real* __restrict__ y) {
  if (guard && ctl->halt) return;
  for (long long k = (long long)blockIdx.x * LDL_BS + threadIdx.x; k < N; k += (long long)gridDim.x * LDL_BS) {
    const long long p = perm[k];
    y[k] = (p < n) ? bx[p] : bs[p - n];
  }
}

// forward solve L y = b for the supernodes of one level (L has a unit diagonal)
__global__ __launch_bounds__(LDL_BS) void k_ldl_fwd(const Ctl* __restrict__ ctl, int guard, const int* __restrict__ lvl, const int* __restrict__ sn_first,
                                                    const long long* __restrict__ sn_rp, const int* __restrict__ sn_rows,
                                                    const long long* __restrict__ sn_poff, const int* __restrict__ desc_ptr,
                                                    const int* __restrict__ desc, const real* __restrict__ Lx, real* __restrict__ y) {
  if (guard && ctl->halt) return;
  ldl_fwd_sn<LDL_BS>(lvl[blockIdx.x], sn_first, sn_rp, sn_rows, sn_poff, desc_ptr, desc, Lx, y);
}

// backward solve L' x = D^-1 y for the supernodes of one level (ancestors already solved)
__global__ __launch_bounds__(LDL_BS) void k_ldl_bwd(const Ctl* __restrict__ ctl, int guard, const int* __restrict__ lvl, const int* __restrict__ sn_first,
                                                    const long long* __restrict__ sn_rp, const int* __restrict__ sn_rows,
                                                    const long long* __restrict__ sn_poff, const real* __restrict__ Lx, real* __restrict__ y) {
  if (guard && ctl->halt) return;
  ldl_bwd_sn<LDL_BS>(lvl[blockIdx.x], sn_first, sn_rp, sn_rows, sn_poff, Lx, y);
}

__global__ __launch_bounds__(LDL_BS) void k_ldl_unperm(Ctl* __restrict__ ctl, int guard, long long N, const int* __restrict__ perm,
                                                       const real* __restrict__ y, real* __restrict__ sol) {
  if (guard && ctl->halt) return;
  for (long long k = (long long)blockIdx.x * LDL_BS + threadIdx.x; k < N; k += (long long)gridDim.x * LDL_BS) sol[perm[k]] = y[k];
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->cg_done = 1;      // the tail's "solve finished" flag (a direct solve always finishes)
}

// ---- host side ------------------------------------------------------------------------------------------------------
static int ew(long long N) {
  long long g = (N + LDL_BS - 1) / LDL_BS;
  if (g < 1) g = 1;
  if (g > 4096) g = 4096;
  return (int)g;
}

int32_t ldl_enqueue_refactor(cosmo_hip_handle* h, int cond) {
  LdlPlan* L = plan_of(h);
  if (!L || !L->complete) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "direct KKT solver: no factor (set_params with kkt_kind DIRECT failed or was not called)");
  const LdlSymbolic& S = L->S;
  hipLaunchKernelGGL(k_ldl_zero, dim3(ew(S.panel_size)), dim3(LDL_BS), 0, h->stream, h->ctl, cond, (long long)S.panel_size, L->Lx, L->dstat);
  const long long na = h->A.nnz;
  hipLaunchKernelGGL(k_ldl_refill, dim3(ew(h->n + L->np + na + h->m)), dim3(LDL_BS), 0, h->stream, h->ctl, cond, h->n, L->np, na, h->m,
                     (real)h->prm.sigma, h->P.val, L->pdiag, L->dslot, L->psrc, L->pslot, h->A.val, L->aslot, h->rho, L->rslot, L->Lx);
  for (size_t l = 0; l + 1 < S.lvl_ptr.size(); ++l) {
    const int cnt = S.lvl_ptr[l + 1] - S.lvl_ptr[l];
    hipLaunchKernelGGL(k_ldl_factor, dim3(cnt), dim3(LDL_BS), 0, h->stream, h->ctl, cond, L->lvl_sn + S.lvl_ptr[l], L->sn_first, L->sn_rp,
                       L->sn_rows, L->sn_poff, L->desc_ptr, L->desc, L->Lx, L->dstat);
  }
  HIPCHK(h, hipGetLastError());
  return COSMO_HIP_OK;
}

// a factorisation outside the loop (setup, update_rho): timed, synchronised, pivots checked
int32_t ldl_refactor_now(cosmo_hip_handle* h, bool inertia) {
  LdlPlan* L = plan_of(h);
  if (!L || !L->complete) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "direct KKT solver: no factor (set_params with kkt_kind DIRECT failed or was not called)");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const auto t0 = std::chrono::steady_clock::now();
  CHK(ldl_enqueue_refactor(h, 0));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  L->last_factor_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  int st[3];
  HIPCHK(h, hipMemcpy(st, L->dstat, sizeof st, hipMemcpyDeviceToHost));
  if (st[0]) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "direct KKT solver: zero or non-finite pivot in the LDL' factorisation");
  if (inertia && st[1] != h->n) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "Objective function is not convex.");
  return COSMO_HIP_OK;
}

// analysis, refill maps and device arrays of a new plan (no factorisation); on failure the caller frees the partial plan
static int32_t ldl_build(cosmo_hip_handle* h, const std::vector<int64_t>& perm_req) {
  const long long n = h->n, m = h->m;
  // patterns of P and A from the device (CSR, int32)
  std::vector<int> prp(n + 1), pcol(h->P.nnz), arp(m + 1), acol(h->A.nnz);
  HIPCHK(h, hipMemcpy(prp.data(), h->P.rowptr, sizeof(int) * (n + 1), hipMemcpyDeviceToHost));
  if (h->P.nnz) HIPCHK(h, hipMemcpy(pcol.data(), h->P.col, sizeof(int) * h->P.nnz, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(arp.data(), h->A.rowptr, sizeof(int) * (m + 1), hipMemcpyDeviceToHost));
  if (h->A.nnz) HIPCHK(h, hipMemcpy(acol.data(), h->A.col, sizeof(int) * h->A.nnz, hipMemcpyDeviceToHost));
  std::vector<int64_t> pr, pc, ar(h->A.nnz), ac(h->A.nnz);
  std::vector<int> psrc, pdiag(n, -1);
  for (long long i = 0; i < n; ++i)
    for (int k = prp[i]; k < prp[i + 1]; ++k) {
      const int j = pcol[k];
      if (j == i) pdiag[i] = k;
      else if (i < j) { pr.push_back(i); pc.push_back(j); psrc.push_back(k); }      // upper triangle of P (assemble_kkt_triangle, :U)
    }
  for (long long i = 0; i < m; ++i)
    for (int k = arp[i]; k < arp[i + 1]; ++k) { ar[k] = i; ac[k] = acol[k]; }
  LdlPlan* L = new LdlPlan();
  h->ldl = L;
  L->perm_req = perm_req;
  const char* err = nullptr;
  if (ldl_analyze(n, m, pr, pc, ar, ac, perm_req.empty() ? nullptr : perm_req.data(), L->S, &err) != 0) {
    return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "direct KKT solver: %s", err);
  }
  h->ldl_analyses += 1;
  const LdlSymbolic& S = L->S;
  if (S.sn_rp[S.ns] >= 2147483647LL) { return cosmo_fail(h, COSMO_HIP_ERR_UNSUPPORTED, "direct KKT solver: supernode row lists out of int32 range"); }
  // refill maps
  std::vector<long long> dslot(n), pslot(pr.size()), aslot(ar.size()), rslot(m);
  for (long long j = 0; j < n; ++j) dslot[j] = S.slot(j, j);
  for (size_t k = 0; k < pr.size(); ++k) pslot[k] = S.slot(pr[k], pc[k]);
  for (size_t k = 0; k < ar.size(); ++k) aslot[k] = S.slot(n + ar[k], ac[k]);
  for (long long i = 0; i < m; ++i) rslot[i] = S.slot(n + i, n + i);
  L->np = (long long)pr.size();
  std::vector<int> sn_first(S.sn_first.begin(), S.sn_first.end()), perm(S.perm.begin(), S.perm.end());
  std::vector<long long> sn_rp(S.sn_rp.begin(), S.sn_rp.end()), sn_poff(S.sn_poff.begin(), S.sn_poff.end());
  CHK(up(h, &L->sn_first, sn_first.data(), sn_first.size()));
  CHK(up(h, &L->sn_rp, sn_rp.data(), sn_rp.size()));
  CHK(up(h, &L->sn_rows, S.sn_rows.data(), S.sn_rows.size()));
  CHK(up(h, &L->sn_poff, sn_poff.data(), sn_poff.size()));
  CHK(up(h, &L->lvl_sn, S.lvl_sn.data(), S.lvl_sn.size()));
  CHK(up(h, &L->desc_ptr, S.desc_ptr.data(), S.desc_ptr.size()));
  CHK(up(h, &L->desc, S.desc.data(), S.desc.size()));
  CHK(up(h, &L->perm, perm.data(), perm.size()));
  CHK(up(h, &L->pdiag, pdiag.data(), pdiag.size()));
  CHK(up(h, &L->dslot, dslot.data(), dslot.size()));
  CHK(up(h, &L->psrc, psrc.data(), psrc.size()));
  CHK(up(h, &L->pslot, pslot.data(), pslot.size()));
  CHK(up(h, &L->aslot, aslot.data(), aslot.size()));
  CHK(up(h, &L->rslot, rslot.data(), rslot.size()));
  HIPCHK(h, hipMalloc((void**)&L->Lx, sizeof(real) * (size_t)std::max<int64_t>(S.panel_size, 1)));
  HIPCHK(h, hipMalloc((void**)&L->y, sizeof(real) * (size_t)std::max<int64_t>(S.N, 1)));
  HIPCHK(h, hipMalloc((void**)&L->sol, sizeof(real) * (size_t)std::max<int64_t>(S.N, 1)));
  HIPCHK(h, hipMalloc((void**)&L->dstat, sizeof(int) * 3));
  HIPCHK(h, hipMemset(L->dstat, 0, sizeof(int) * 3));
  L->complete = true;
  return COSMO_HIP_OK;
}

int32_t ldl_setup(cosmo_hip_handle* h, const std::vector<int64_t>& perm_req) {
  LdlPlan* old = plan_of(h);
  if (!(old && old->complete && old->perm_req == perm_req)) {     // a complete plan of this pattern (set_problem drops it) is kept: new values only
    ldl_free(h);
    const int32_t rc = ldl_build(h, perm_req);
    if (rc != COSMO_HIP_OK) { ldl_free(h); return rc; }
  }
  return ldl_refactor_now(h, true);
}

// one solve!: from_loop = the right-hand side [ls_x; ls_s] was produced by k_rhs; else it was uploaded (fine-grained entry point)
int32_t ldl_enqueue_solve(cosmo_hip_handle* h, int guard, bool from_loop) {
  LdlPlan* L = plan_of(h);
  if (!L || !L->complete) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "direct KKT solver: no factor (set_params with kkt_kind DIRECT failed or was not called)");
  const LdlSymbolic& S = L->S;
  if (!from_loop) CHK(enqueue_y2_only(h));             // resets cg_done / cg_k as k_rhs does in the loop
  prof_begin(h, KC_OP_APPLY);
  hipLaunchKernelGGL(k_ldl_perm, dim3(ew(S.N)), dim3(LDL_BS), 0, h->stream, h->ctl, guard, (long long)S.N, (long long)h->n, L->perm, h->ls_x,
                     h->ls_s, L->y);
  const int H = (int)S.lvl_ptr.size() - 1;
  for (int l = 0; l < H; ++l)
    hipLaunchKernelGGL(k_ldl_fwd, dim3(S.lvl_ptr[l + 1] - S.lvl_ptr[l]), dim3(LDL_BS), 0, h->stream, h->ctl, guard, L->lvl_sn + S.lvl_ptr[l],
                       L->sn_first, L->sn_rp, L->sn_rows, L->sn_poff, L->desc_ptr, L->desc, L->Lx, L->y);
  for (int l = H - 1; l >= 0; --l)
    hipLaunchKernelGGL(k_ldl_bwd, dim3(S.lvl_ptr[l + 1] - S.lvl_ptr[l]), dim3(LDL_BS), 0, h->stream, h->ctl, guard, L->lvl_sn + S.lvl_ptr[l],
                       L->sn_first, L->sn_rp, L->sn_rows, L->sn_poff, L->Lx, L->y);
  hipLaunchKernelGGL(k_ldl_unperm, dim3(ew(S.N)), dim3(LDL_BS), 0, h->stream, h->ctl, guard, (long long)S.N, L->perm, L->y, L->sol);
  prof_end(h);
  HIPCHK(h, hipGetLastError());
  CHK(launch_mr_tail_full(h, from_loop ? 1 : 0, L->sol));
  if (!from_loop) CHK(enqueue_count_solve(h));
  return COSMO_HIP_OK;
}

int32_t ldl_info(cosmo_hip_handle* h, int64_t* out) {
  LdlPlan* L = plan_of(h);
  if (!L) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "direct_info: the handle has no direct KKT solver (kkt_kind COSMO_HIP_KKT_DIRECT)");
  int st[3];
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(st, L->dstat, sizeof st, hipMemcpyDeviceToHost));
  const LdlSymbolic& S = L->S;
  out[0] = S.nnz_L; out[1] = S.nnz_stored; out[2] = S.ns; out[3] = S.height; out[4] = S.max_width;
  out[5] = st[2]; out[6] = st[1]; out[7] = (int64_t)(L->last_factor_s * 1e9);
  return COSMO_HIP_OK;
}
