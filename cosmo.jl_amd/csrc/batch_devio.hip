// batch_devio.hip -- the three kernels behind the device-memory entry points of a batch (batch_devio.h).  All of them are grid-stride passes over
// member-major vectors, one element per thread and trip, no atomics and no shared memory: they move a few bytes per element and are bound by the
// launch, not by the memory system.  Every expression keeps the operand order of the path it replaces (k_batch_update_qb and k_batch_set_w in
// batch.hip, scale_variables! / reverse_scaling! as model.py does them on the host), so the results are the same bits; the library is built with
// -ffp-contract=off, which keeps a * b + c two roundings here as there.
#include "batch_devio.h"
#include <algorithm>

struct BDevioMembers { int32_t k[BDEVIO_CHUNK]; };

static inline int bdevio_grid(long long N) { return (int)std::max<long long>(1, std::min<long long>((N + COSMO_BS - 1) / COSMO_BS, 2048)); }

// Element g of the launch is entry i of [q (n) | b (m)] of listed member j0 + j; its batch member is mem.k[j], or j0 + j itself without a list.  The
// caller's arrays are indexed by the position in the list, the batch's by the member.
__global__ __launch_bounds__(COSMO_BS) void k_batch_update_qb_dev(int n, int m, int j0, int cnt, int listed, BDevioMembers mem,
                                                                  const real* __restrict__ q_raw, const real* __restrict__ b_raw,
                                                                  const real* __restrict__ Dsc, const real* __restrict__ Esc,
                                                                  const real* __restrict__ csc, const unsigned char* __restrict__ nonneg, real big,
                                                                  real* __restrict__ q, real* __restrict__ b, int* __restrict__ cls) {
  const long long N = (long long)cnt * (n + m);
  for (long long g = (long long)blockIdx.x * COSMO_BS + threadIdx.x; g < N; g += (long long)gridDim.x * COSMO_BS) {
    const int j = (int)(g / (n + m)), i = (int)(g % (n + m));
    const long long k = listed ? mem.k[j] : j0 + j, src = j0 + j;
    if (i < n) {
      if (q_raw) q[k * n + i] = (Dsc[k * n + i] * q_raw[src * n + i]) * csc[k];
    } else if (b_raw) {
      const int r = i - n;
      const real bs = Esc[k * m + r] * b_raw[src * m + r];
      b[k * m + r] = bs;
      if (nonneg[r]) cls[k * m + r] = bs > big ? 2 : 0;
    }
  }
}

__global__ __launch_bounds__(COSMO_BS) void k_batch_set_iterates_dev(int nprob, int n, int m, const real* __restrict__ x0, const real* __restrict__ s0,
                                                                     const real* __restrict__ y0, const real* __restrict__ Dinv,
                                                                     const real* __restrict__ Esc, const real* __restrict__ Einv,
                                                                     const real* __restrict__ csc, const real* __restrict__ rho, real* __restrict__ w,
                                                                     real* __restrict__ w_prev, real* __restrict__ s) {
  const long long N = (long long)nprob * (n + m);
  for (long long g = (long long)blockIdx.x * COSMO_BS + threadIdx.x; g < N; g += (long long)gridDim.x * COSMO_BS) {
    const long long k = g / (n + m); const int i = (int)(g % (n + m));
    real wv;
    if (i < n) {
      const long long r = k * n + i;
      wv = x0 ? Dinv[r] * x0[r] : R(0.0);
    } else {
      const long long r = k * m + (i - n);
      const real sv = s0 ? Esc[r] * s0[r] : R(0.0);
      const real mv = y0 ? (Einv[r] * (-y0[r])) * csc[k] : R(0.0);           // mu = -y (src/interface.jl:167)
      wv = (R(1.0) / rho[r]) * mv + sv;
      s[r] = sv;
    }
    w[g] = wv;
    w_prev[g] = wv;
  }
}

__global__ __launch_bounds__(COSMO_BS) void k_batch_export_solution(int nprob, int n, int m, const real* __restrict__ w_prev, const real* __restrict__ s,
                                                                    const real* __restrict__ mu, const real* __restrict__ Dsc,
                                                                    const real* __restrict__ Esc, const real* __restrict__ Einv,
                                                                    const real* __restrict__ cinv, real* __restrict__ x_out, real* __restrict__ s_out,
                                                                    real* __restrict__ y_out) {
  const long long N = (long long)nprob * (n + m);
  for (long long g = (long long)blockIdx.x * COSMO_BS + threadIdx.x; g < N; g += (long long)gridDim.x * COSMO_BS) {
    const long long k = g / (n + m); const int i = (int)(g % (n + m));
    if (i < n) {
      const long long r = k * n + i;
      if (x_out) x_out[r] = Dsc[r] * w_prev[g];                              // x is the head of w_prev (src/types.jl:274)
    } else {
      const long long r = k * m + (i - n);
      if (s_out) s_out[r] = Einv[r] * s[r];
      if (y_out) y_out[r] = -((Esc[r] * mu[r]) * cinv[k]);
    }
  }
}

hipError_t bdevio_update_qb(hipStream_t st, int n, int m, int count, const int64_t* members, const real* q_raw, const real* b_raw, const real* Dsc,
                            const real* Esc, const real* csc, const unsigned char* nonneg, real big, real* q, real* b, int* cls) {
  if (count <= 0 || (!q_raw && !b_raw) || n + m == 0) return hipSuccess;
  BDevioMembers mem;
  for (int e = 0; e < BDEVIO_CHUNK; ++e) mem.k[e] = 0;
  const int step = members ? BDEVIO_CHUNK : count;
  for (int j0 = 0; j0 < count; j0 += step) {
    const int cnt = std::min(step, count - j0);
    if (members) for (int e = 0; e < cnt; ++e) mem.k[e] = (int32_t)members[j0 + e];
    hipLaunchKernelGGL(k_batch_update_qb_dev, dim3(bdevio_grid((long long)cnt * (n + m))), dim3(COSMO_BS), 0, st, n, m, j0, cnt, members ? 1 : 0, mem, q_raw,
                       b_raw, Dsc, Esc, csc, nonneg, big, q, b, cls);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t bdevio_set_iterates(hipStream_t st, int nprob, int n, int m, const real* x0, const real* s0, const real* y0, const real* Dinv, const real* Esc,
                               const real* Einv, const real* csc, const real* rho, real* w, real* w_prev, real* s) {
  if (n + m == 0) return hipSuccess;
  hipLaunchKernelGGL(k_batch_set_iterates_dev, dim3(bdevio_grid((long long)nprob * (n + m))), dim3(COSMO_BS), 0, st, nprob, n, m, x0, s0, y0, Dinv, Esc, Einv,
                     csc, rho, w, w_prev, s);
  return hipGetLastError();
}

hipError_t bdevio_export_solution(hipStream_t st, int nprob, int n, int m, const real* w_prev, const real* s, const real* mu, const real* Dsc,
                                  const real* Esc, const real* Einv, const real* cinv, real* x_out, real* s_out, real* y_out) {
  if (n + m == 0 || (!x_out && !s_out && !y_out)) return hipSuccess;
  hipLaunchKernelGGL(k_batch_export_solution, dim3(bdevio_grid((long long)nprob * (n + m))), dim3(COSMO_BS), 0, st, nprob, n, m, w_prev, s, mu, Dsc, Esc,
                     Einv, cinv, x_out, s_out, y_out);
  return hipGetLastError();
}
