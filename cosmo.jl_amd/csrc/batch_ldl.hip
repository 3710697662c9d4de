// batch_ldl.hip -- host side of the direct KKT solver in batch mode (batch_ldl.h): the union analysis, the per-problem refill maps, the storage
// budget and the set-up factorisation with its inertia check.
//
// Bytes (Float64; half of it in Float32): per problem a slab of panel_size reals and a work vector of n + m reals.  A factorisation reads and
// writes its slab a few times over (zero, refill, the left-looking updates re-read the descendants' panels); a solve reads the slab twice (forward +
// backward) and the work vector a few times per supernode.
#include <algorithm>
#include <chrono>
#include <string.h>
#include "device_utils.h"
#include "ldl.h"
#include "batch_ldl.h"

struct BLdlPlan {
  LdlSymbolic S;
  std::vector<void*> allocs;
  double analysis_s = 0.0, setup_factor_s = 0.0;
};

void bldl_free(BLdlPlan* p) {
  if (!p) return;
  for (void* a : p->allocs) (void)hipFree(a);
  delete p;
}

template <class T>
static int32_t bldl_up(BLdlPlan* p, const T** dst, const std::vector<T>& v, std::string& err) {
  T* d = nullptr;
  if (hipMalloc((void**)&d, sizeof(T) * std::max<size_t>(v.size(), 1)) != hipSuccess) { err = "direct batch: hipMalloc failed"; return COSMO_HIP_ERR_HIP; }
  p->allocs.push_back(d);
  if (!v.empty() && hipMemcpy(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice) != hipSuccess) { err = "direct batch: hipMemcpy failed"; return COSMO_HIP_ERR_HIP; }
  *dst = d;
  return COSMO_HIP_OK;
}
template <class T>
static int32_t bldl_zero(BLdlPlan* p, T** dst, size_t count, std::string& err) {
  T* d = nullptr;
  if (hipMalloc((void**)&d, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) { err = "direct batch: hipMalloc failed"; return COSMO_HIP_ERR_HIP; }
  p->allocs.push_back(d);
  if (hipMemset(d, 0, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) { err = "direct batch: hipMemset failed"; return COSMO_HIP_ERR_HIP; }
  *dst = d;
  return COSMO_HIP_OK;
}

int32_t bldl_build(int nprob, long long n, long long m, const std::vector<HostCsr>& PT, const std::vector<HostCsr>& A, const std::vector<int64_t>& perm,
                   BLdlPlan** out, BLdlDev* dev, std::string& err) {
  BLdlPlan* p = new BLdlPlan();
  *out = p;
  // union of the patterns: strictly upper entries of P (row j < column i of P's row j in [P | A']) and the entries of A
  std::vector<long long> pk, ak;
  for (int k = 0; k < nprob; ++k) {
    const HostCsr& T = PT[(size_t)k];
    for (long long j = 0; j < n; ++j)
      for (int t = T.rowptr[j]; t < T.split[j]; ++t) if (T.col[t] > j) pk.push_back(j * n + T.col[t]);
    const HostCsr& M = A[(size_t)k];
    for (long long i = 0; i < m; ++i)
      for (int t = M.rowptr[i]; t < M.rowptr[i + 1]; ++t) ak.push_back(i * n + M.col[t]);
  }
  std::sort(pk.begin(), pk.end()); pk.erase(std::unique(pk.begin(), pk.end()), pk.end());
  std::sort(ak.begin(), ak.end()); ak.erase(std::unique(ak.begin(), ak.end()), ak.end());
  std::vector<int64_t> pr(pk.size()), pc(pk.size()), ar(ak.size()), ac(ak.size());
  for (size_t q = 0; q < pk.size(); ++q) { pr[q] = pk[q] / n; pc[q] = pk[q] % n; }
  for (size_t q = 0; q < ak.size(); ++q) { ar[q] = ak[q] / n; ac[q] = ak[q] % n; }
  std::vector<long long>().swap(pk); std::vector<long long>().swap(ak);
  const char* aerr = nullptr;
  if (ldl_analyze(n, m, pr, pc, ar, ac, perm.empty() ? nullptr : perm.data(), p->S, &aerr) != 0) {
    err = std::string("direct KKT solver: ") + aerr;
    return COSMO_HIP_ERR_INVALID;
  }
  const LdlSymbolic& S = p->S;
  p->analysis_s = S.seconds;
  if (S.panel_size >= 2147483647LL || S.sn_rp[S.ns] >= 2147483647LL) {
    err = "direct batch: the supernodal panels of one problem are out of int32 range (solve such problems with one handle each)";
    return COSMO_HIP_ERR_UNSUPPORTED;
  }
  // storage budget: the slabs and work vectors of all members plus the refill maps, against half of the free device memory
  size_t ptn = 0, an = 0;
  for (int k = 0; k < nprob; ++k) { ptn += PT[(size_t)k].col.size(); an += A[(size_t)k].col.size(); }
  const double need = (double)nprob * (double)(S.panel_size + S.N) * sizeof(real) + 4.0 * ((double)nprob * n + (double)ptn + (double)an);
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) { err = "direct batch: hipMemGetInfo failed"; return COSMO_HIP_ERR_HIP; }
  if (need > 0.5 * (double)fr) {
    char buf[400];
    snprintf(buf, sizeof buf, "direct batch: the factors need %.1f MiB (panel_size %lld x %d problems x %d bytes, plus work vectors and refill maps), over half of "
             "the %.1f MiB of free device memory: solve these problems with one handle each", need / 1048576.0, (long long)S.panel_size, nprob,
             (int)sizeof(real), (double)fr / 1048576.0);
    err = buf;
    return COSMO_HIP_ERR_UNSUPPORTED;
  }
  // refill maps (per problem, in the storage order of the batch's concatenated matrices)
  std::vector<int> dslot((size_t)n), rslot((size_t)m), pdiag((size_t)nprob * n, -1), pslot, aslot;
  pslot.reserve(ptn); aslot.reserve(an);
  for (long long j = 0; j < n; ++j) dslot[(size_t)j] = (int)S.slot(j, j);
  for (long long i = 0; i < m; ++i) rslot[(size_t)i] = (int)S.slot(n + i, n + i);
  for (int k = 0; k < nprob; ++k) {
    const HostCsr& T = PT[(size_t)k];
    for (long long j = 0; j < n; ++j) {
      for (int t = T.rowptr[j]; t < T.rowptr[j + 1]; ++t) {
        int s = -1;
        if (t < T.split[j]) {
          const long long i = T.col[t];
          if (i == j) pdiag[(size_t)k * n + j] = t;
          else if (i > j) s = (int)S.slot(j, i);
        }
        pslot.push_back(s);
      }
    }
    const HostCsr& M = A[(size_t)k];
    for (long long i = 0; i < m; ++i)
      for (int t = M.rowptr[i]; t < M.rowptr[i + 1]; ++t) aslot.push_back((int)S.slot(n + i, M.col[t]));
  }
  for (int v : aslot) if (v < 0) { err = "direct batch: an entry of A has no slot in the union analysis"; return COSMO_HIP_ERR_INVALID; }
  std::vector<int> sn_first(S.sn_first.begin(), S.sn_first.end()), pm(S.perm.begin(), S.perm.end());
  std::vector<long long> sn_rp(S.sn_rp.begin(), S.sn_rp.end()), sn_poff(S.sn_poff.begin(), S.sn_poff.end());
  BLdlDev& D = *dev;
  memset(&D, 0, sizeof D);
  D.ns = (int)S.ns; D.N = (int)S.N; D.panel = S.panel_size;
  int32_t rc;
  if ((rc = bldl_up(p, &D.sn_first, sn_first, err)) || (rc = bldl_up(p, &D.sn_rp, sn_rp, err)) || (rc = bldl_up(p, &D.sn_rows, S.sn_rows, err)) ||
      (rc = bldl_up(p, &D.sn_poff, sn_poff, err)) || (rc = bldl_up(p, &D.desc_ptr, S.desc_ptr, err)) || (rc = bldl_up(p, &D.desc, S.desc, err)) ||
      (rc = bldl_up(p, &D.perm, pm, err)) || (rc = bldl_up(p, &D.dslot, dslot, err)) || (rc = bldl_up(p, &D.rslot, rslot, err)) ||
      (rc = bldl_up(p, &D.pdiag, pdiag, err)) || (rc = bldl_up(p, &D.pslot, pslot, err)) || (rc = bldl_up(p, &D.aslot, aslot, err)))
    return rc;
  if ((rc = bldl_zero(p, &D.Lx, (size_t)nprob * (size_t)S.panel_size, err)) || (rc = bldl_zero(p, &D.y, (size_t)nprob * (size_t)S.N, err)) ||
      (rc = bldl_zero(p, &D.nfact, (size_t)nprob, err)) || (rc = bldl_zero(p, &D.npos, (size_t)nprob, err)) || (rc = bldl_zero(p, &D.fail, (size_t)nprob, err)))
    return rc;
  return COSMO_HIP_OK;
}

__global__ __launch_bounds__(COSMO_BS) void k_bldl_setup(BLdlDev L, int n, int m, real sigma, const int* __restrict__ PT_rowptr, const real* __restrict__ PT_val,
                                                         const long long* __restrict__ PT_nzoff, const int* __restrict__ A_rowptr, const real* __restrict__ A_val,
                                                         const long long* __restrict__ A_nzoff, const real* __restrict__ rho) {
  const int k = blockIdx.x;
  const int pnnz = PT_rowptr[(long long)k * (n + 1) + n], annz = A_rowptr[(long long)k * (m + 1) + m];
  (void)bldl_refill_factor<COSMO_BS>(L, k, n, m, sigma, PT_val + PT_nzoff[k], pnnz, A_val + A_nzoff[k], annz, rho + (long long)k * m, PT_nzoff[k], A_nzoff[k]);
}

int32_t bldl_setup_factor(BLdlPlan* p, const BLdlDev& dev, hipStream_t st, int nprob, int n, int m, real sigma, const int* PT_rowptr, const real* PT_val,
                          const long long* PT_nzoff, const int* A_rowptr, const real* A_val, const long long* A_nzoff, const real* rho, std::string& err) {
  if (hipStreamSynchronize(st) != hipSuccess) { err = "direct batch: stream synchronisation failed"; return COSMO_HIP_ERR_HIP; }
  const auto t0 = std::chrono::steady_clock::now();
  hipLaunchKernelGGL(k_bldl_setup, dim3(nprob), dim3(COSMO_BS), 0, st, dev, n, m, sigma, PT_rowptr, PT_val, PT_nzoff, A_rowptr, A_val, A_nzoff, rho);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { err = "direct batch: the set-up factorisation failed to run"; return COSMO_HIP_ERR_HIP; }
  p->setup_factor_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::vector<int> pos((size_t)nprob), bad((size_t)nprob);
  if (hipMemcpy(pos.data(), dev.npos, sizeof(int) * nprob, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(bad.data(), dev.fail, sizeof(int) * nprob, hipMemcpyDeviceToHost) != hipSuccess) { err = "direct batch: hipMemcpy failed"; return COSMO_HIP_ERR_HIP; }
  for (int k = 0; k < nprob; ++k) {
    if (bad[(size_t)k]) { err = "direct KKT solver: zero or non-finite pivot in the LDL' factorisation (member " + std::to_string(k) + ")"; return COSMO_HIP_ERR_INVALID; }
    if (pos[(size_t)k] != n) { err = "Objective function is not convex. (member " + std::to_string(k) + ")"; return COSMO_HIP_ERR_INVALID; }
  }
  return COSMO_HIP_OK;
}

// k_bldl_setup for a list of members (cosmo_hip_batch_apply_updates after new matrix values): block j refactors member mem[j * stride] with its current rho
__global__ __launch_bounds__(COSMO_BS) void k_bldl_setup_members(BLdlDev L, int n, int m, real sigma, const int* __restrict__ mem, int stride,
                                                                 const int* __restrict__ PT_rowptr, const real* __restrict__ PT_val,
                                                                 const long long* __restrict__ PT_nzoff, const int* __restrict__ A_rowptr,
                                                                 const real* __restrict__ A_val, const long long* __restrict__ A_nzoff, const real* __restrict__ rho) {
  const int k = mem[(long long)blockIdx.x * stride];
  const int pnnz = PT_rowptr[(long long)k * (n + 1) + n], annz = A_rowptr[(long long)k * (m + 1) + m];
  if (threadIdx.x == 0) L.fail[k] = 0;                                     // (a member that failed before gets a fresh verdict; refill_factor synchronises first)
  (void)bldl_refill_factor<COSMO_BS>(L, k, n, m, sigma, PT_val + PT_nzoff[k], pnnz, A_val + A_nzoff[k], annz, rho + (long long)k * m, PT_nzoff[k], A_nzoff[k]);
}

int32_t bldl_refactor_members(BLdlPlan*, const BLdlDev& dev, hipStream_t st, int nprob, int count, const int* d_mem, int stride, const int* h_mem, int n, int m, real sigma,
                              const int* PT_rowptr, const real* PT_val, const long long* PT_nzoff, const int* A_rowptr, const real* A_val,
                              const long long* A_nzoff, const real* rho, std::string& err) {
  if (count <= 0) return COSMO_HIP_OK;
  hipLaunchKernelGGL(k_bldl_setup_members, dim3(count), dim3(COSMO_BS), 0, st, dev, n, m, sigma, d_mem, stride, PT_rowptr, PT_val, PT_nzoff, A_rowptr, A_val,
                     A_nzoff, rho);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { err = "direct batch: the factorisation of the updated members failed to run"; return COSMO_HIP_ERR_HIP; }
  std::vector<int> npos((size_t)nprob), fail((size_t)nprob);
  if (hipMemcpy(npos.data(), dev.npos, sizeof(int) * nprob, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(fail.data(), dev.fail, sizeof(int) * nprob, hipMemcpyDeviceToHost) != hipSuccess) { err = "direct batch: hipMemcpy failed"; return COSMO_HIP_ERR_HIP; }
  for (int j = 0; j < count; ++j) {
    const int k = h_mem[j], pos = npos[(size_t)k], bad = fail[(size_t)k];
    if (bad) { err = "direct KKT solver: zero or non-finite pivot in the LDL' factorisation (member " + std::to_string(k) + ")"; return COSMO_HIP_ERR_INVALID; }
    if (pos != n) { err = "Objective function is not convex. (member " + std::to_string(k) + ")"; return COSMO_HIP_ERR_INVALID; }
  }
  return COSMO_HIP_OK;
}

int32_t bldl_info(BLdlPlan* p, const BLdlDev& dev, hipStream_t st, int nprob, int64_t* out, std::string& err) {
  std::vector<int> nf((size_t)nprob), pos((size_t)nprob);
  if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(nf.data(), dev.nfact, sizeof(int) * nprob, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(pos.data(), dev.npos, sizeof(int) * nprob, hipMemcpyDeviceToHost) != hipSuccess) { err = "direct batch: hipMemcpy failed"; return COSMO_HIP_ERR_HIP; }
  const LdlSymbolic& S = p->S;
  int64_t tot = 0, mn = INT64_MAX;
  for (int k = 0; k < nprob; ++k) { tot += nf[(size_t)k]; mn = std::min<int64_t>(mn, pos[(size_t)k]); }
  out[0] = S.nnz_L; out[1] = S.panel_size; out[2] = S.ns; out[3] = S.height; out[4] = S.max_width; out[5] = (int64_t)(p->analysis_s * 1e9);
  out[6] = tot; out[7] = mn;
  return COSMO_HIP_OK;
}

int32_t bldl_counts(BLdlPlan*, const BLdlDev& dev, hipStream_t st, int nprob, int64_t* out, std::string& err) {
  std::vector<int> nf((size_t)nprob);
  if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(nf.data(), dev.nfact, sizeof(int) * nprob, hipMemcpyDeviceToHost) != hipSuccess) { err = "direct batch: hipMemcpy failed"; return COSMO_HIP_ERR_HIP; }
  for (int k = 0; k < nprob; ++k) out[k] = nf[(size_t)k];
  return COSMO_HIP_OK;
}

int bldl_first_failed(BLdlPlan*, const BLdlDev& dev, hipStream_t st, int nprob) {
  std::vector<int> bad((size_t)nprob);
  if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(bad.data(), dev.fail, sizeof(int) * nprob, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  for (int k = 0; k < nprob; ++k) if (bad[(size_t)k]) return k;
  return -1;
}
