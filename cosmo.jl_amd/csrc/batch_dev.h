// batch_dev.h -- what every translation unit with batch kernels shares (batch.hip, batch_polish.hip): the per-problem control block, the concatenated
// CSR descriptor of a batch's matrices, the row projection of the simple cones, the single-workgroup reductions and the streaming form of the sparse
// passes.  Device code only; every function is inlined into its caller.
#pragma once
#include "device_utils.h"

struct BCtl {                 // per problem, device resident
  int status; int n_rho_updates;
  long long iter, solves, kkt_iters_total;
  real rho, cost, r_prim, r_dual, max_norm_prim, max_norm_dual;
  real rho_updates[COSMO_HIP_MAX_RHO_UPDATES];
};

struct BMat { const int* rowptr; const int* col; const real* val; const int* split; const int* rb;   // concatenated over problems
              const long long* nz_off; const int* rb_off; const int* nb; int nrows; int split_col; };

__device__ __forceinline__ CsrView bview(const BMat& M, int k) {
  CsrView v;
  v.rowptr = M.rowptr + (long long)k * (M.nrows + 1);
  v.col = M.col + M.nz_off[k];
  v.val = M.val + M.nz_off[k];
  v.split = M.split ? M.split + (long long)k * M.nrows : nullptr;
  v.rb = M.rb + M.rb_off[k];
  v.nb = M.nb[k];
  v.nrows = M.nrows;
  v.split_col = M.split_col;
  return v;
}

__device__ __forceinline__ real proj_simple(real x, uint32_t meta, const real* bl, const real* bu) {
  const uint32_t kind = meta & 3u;
  if (kind == 0u) return x;
  if (kind == 1u) return 0.0;
  if (kind == 2u) return (x != x) ? x : ((x > R(0.0)) ? x : R(0.0));
  const uint32_t j = meta >> 2;
  const real l = bl[j], u = bu[j];
  return (x < l) ? l : ((x > u) ? u : x);
}

// Single-workgroup reductions: fixed order, no atomics (red: BS / 64 reals of LDS; the result is broadcast to all threads).
template <int BS>
__device__ __forceinline__ real bsum(real v, real* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  real t = 0.0;
#pragma unroll
  for (int i = 0; i < BS / 64; ++i) t += red[i];
  return t;
}
// Block sum with ONE barrier: consecutive calls alternate between two sets of BS / 64 slots (ph flips).  The set written now was last read two
// calls ago, and every thread has passed the barrier of the call in between since then, so no barrier is needed in front of the writes.  Callers
// put a workgroup barrier between the last classic bsum / bmax on `red` and the first bsum_db (the classic ones start with their own barrier, so
// the other direction needs nothing).  Same additions in the same order as bsum.
template <int BS>
__device__ __forceinline__ real bsum_db(real v, real* red, int& ph) {
  v = wave_sum(v);
  real* r = red + ph * (BS / 64);
  ph ^= 1;
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  real t = 0.0;
#pragma unroll
  for (int i = 0; i < BS / 64; ++i) t += r[i];
  return t;
}
template <int BS>
__device__ __forceinline__ real bmax(real v, real* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  real t = red[0];
#pragma unroll
  for (int i = 1; i < BS / 64; ++i) t = (red[i] > t || red[i] != red[i]) ? red[i] : t;
  return t;
}

// The streaming form of a problem's sparse passes: values / indices stream from global memory tile by tile through a 16 KB LDS product buffer (any
// size); every row goes to one thread that adds the row's products left to right (batch.hip describes it next to the LDS-image form).
struct StreamOps {
  CsrView A, AT, PT;
  real* lds; real* red;
  unsigned char* psd_ws;
  static constexpr bool in_lds = false;
  __device__ __forceinline__ real rowA(int, const real*) const { return R(0.0); }     // (register-CG form: LdsOps only)
  __device__ __forceinline__ real rowAT(int, const real*) const { return R(0.0); }
  __device__ __forceinline__ real rowP(int, const real*) const { return R(0.0); }
  __device__ __forceinline__ real* buf_n(real* g) const { return g; }       // vector the A / P products gather from
  __device__ __forceinline__ real* buf_m(real* g) const { return g; }       // vector the A' products gather from
  __device__ __forceinline__ const real* stage_n(const real* g) const { return g; }
  template <class F> __device__ __forceinline__ void rows_A(const real* x, F fn) {
    for (int t = 0; t < A.nb; ++t) csr_stream_tile(A, x, x, t, lds, red, fn);
  }
  template <class F> __device__ __forceinline__ void rows_AT(const real* y, F fn) {
    for (int t = 0; t < AT.nb; ++t) csr_stream_tile(AT, y, y, t, lds, red, fn);
  }
  template <class F> __device__ __forceinline__ void rows_PT(const real* x1, const real* x2, F fn) {
    for (int t = 0; t < PT.nb; ++t) csr_stream_tile(PT, x1, x2, t, lds, red, fn);
  }
};
