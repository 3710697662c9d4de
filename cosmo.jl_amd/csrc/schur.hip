// schur.hip -- the Schur-complement KKT solver COSMO_HIP_KKT_SCHUR: an exact solve of the reduced system M x = rhs, M = P + sigma I + A' rho A, with the
// semantics of the reference's direct solver (factorise at setup, refactorise when rho changes, no Krylov tolerance).  DESIGN.md "Schur-complement KKT
// solver".  The rows of A are split by length (schur_plan.cpp): M = M_s + A_d' rho_d A_d with M_s block diagonal under a permutation, and by Woodbury
//     M^-1 = M_s^-1 - M_s^-1 A_d' C^-1 A_d M_s^-1,      C = diag(1 ./ rho_d) + A_d M_s^-1 A_d'      (dense SPD, nd x nd).
// Factorisation (setup, update_rho, update_matrices; in the loop behind the adaptive-rho check, every launch a no-op unless Ctl::rho_changed):
//   k_sc_zero + k_sc_refill   the packed blocks of M_s from P.val, A.val, rho and sigma, every entry summed in the plan's fixed order
//   k_sc_small / k_sc_block   Cholesky and explicit inverse of every block: side <= 3 one thread, side <= 64 one wave, larger ones a workgroup
//   k_sc_formC                C, one row per workgroup
//   k_sc_potrf + k_sc_tile    blocked right-looking Cholesky of C (block side SCHUR_NB = 64), the inverse of the factor by block rows and C^-1 = L^-T L^-1;
//                             every product of 64 x 64 tiles runs in the one MFMA tile kernel
// Solve: y = M_s^-1 rhs, t = A_d y, u = C^-1 t, v = A_d' u, x = y - M_s^-1 v, then at most refine_steps steps of iterative refinement against M itself; a
// step is kept only if ||rhs - M x||_2 fell (decided on the device; after a rejected step the remaining ones change nothing).
// No float atomics anywhere: every sum has a fixed order, two runs give the same bits.
#include <stdio.h>
#include <chrono>
#include <algorithm>
#include "internal.h"
#include "device_utils.h"
#include "psd_internal.h"
#include "schur_plan.h"

namespace {
#define SC_BS 256
#define SC_NB SCHUR_NB
#define SC_KC 32                 // k-chunk of the tile kernel staged in LDS
#define SC_FORMC_GRID 64         // workgroups of k_sc_formC, each with an n-vector of scratch

struct ScScal {                  // device scalars of the refinement, indexed by step so that no launch reads a word it writes
  real rhs2;                     // ||rhs||^2
  real best[SCHUR_REFINE_STEPS_MAX + 1];      // ||rhs - M x||^2 of the iterate kept after step s (0: before refinement)
  int stop[SCHUR_REFINE_STEPS_MAX + 1];       // a step up to s was rejected
  int taken;                     // steps kept in the last solve
  real ratio[2];                 // ||rhs - M x|| / ||rhs|| of the last solve: after refinement, before refinement
};

struct SchurDev {
  SchurPlan S;
  int ndp = 0, T = 0;            // nd rounded up to SC_NB (the padding is an identity block), tiles per side
  int refine_steps = SCHUR_REFINE_STEPS_DEFAULT;
  int *perm = nullptr, *pos = nullptr, *blk_of_pos = nullptr, *comp_ptr = nullptr;
  long long *boff = nullptr, *epos = nullptr, *eptr = nullptr;
  int *ta = nullptr, *tb = nullptr, *trow = nullptr;
  int *ad_row = nullptr, *ad_ptr = nullptr, *ad_col = nullptr, *ad_src = nullptr, *adt_ptr = nullptr, *adt_k = nullptr, *adt_src = nullptr;
  real *Bfac = nullptr, *Binv = nullptr;       // packed blocks: Cholesky factors (lower triangles), inverses (full, symmetric)
  real *C = nullptr, *Li = nullptr;            // ndp x ndp, row-major: C -> L -> C^-1; the inverse of L
  real* wbuf = nullptr;                        // SC_FORMC_GRID x n, zero outside k_sc_formC
  real *y = nullptr, *v = nullptr, *x = nullptr, *xc = nullptr, *r = nullptr, *rc = nullptr, *t1 = nullptr, *t2 = nullptr;   // n
  real *tn = nullptr, *un = nullptr;           // ndp (the padding stays zero)
  real* parts = nullptr;                       // (SCHUR_REFINE_STEPS_MAX + 2) x COSMO_MAX_PARTIALS
  ScScal* scal = nullptr;
  int* dstat = nullptr;                        // {pivot error, factorisations, (unused), refinement steps rejected so far}
  double last_factor_s = 0.0;
};

SchurDev* dev_of(cosmo_hip_handle* h) { return (SchurDev*)h->schur; }

template <class T>
void dfree(T** p) { if (*p) { (void)hipFree(*p); *p = nullptr; } }
template <class T>
int32_t dnew(cosmo_hip_handle* h, T** d, size_t count, bool zero) {
  HIPCHK(h, hipMalloc((void**)d, sizeof(T) * std::max<size_t>(count, 1)));
  if (zero) HIPCHK(h, hipMemsetAsync(*d, 0, sizeof(T) * std::max<size_t>(count, 1), h->stream));
  return COSMO_HIP_OK;
}
template <class T, class U>
int32_t up(cosmo_hip_handle* h, T** d, const std::vector<U>& v) {
  std::vector<T> tmp(v.begin(), v.end());
  CHK(dnew(h, d, tmp.size(), false));
  if (!tmp.empty()) HIPCHK(h, hipMemcpy(*d, tmp.data(), sizeof(T) * tmp.size(), hipMemcpyHostToDevice));
  return COSMO_HIP_OK;
}
int ew(long long N) {
  long long g = (N + SC_BS - 1) / SC_BS;
  return (int)std::min<long long>(std::max<long long>(g, 1), COSMO_MAX_PARTIALS);
}

// cond = 1 (the loop): the launch is a no-op unless the adaptive-rho check just changed rho
__device__ __forceinline__ bool sc_skip(const Ctl* ctl, int cond) { return cond && (ctl->halt || !ctl->rho_changed); }
__device__ __forceinline__ void sc_bad_pivot(Ctl* ctl, int cond, int* dstat) {
  dstat[0] = 1;
  if (cond) { ctl->error = COSMO_HIP_ERR_INVALID; ctl->halt = 1; }
}

// ---- refill and block factorisation ------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_BS) void k_sc_zero(const Ctl* __restrict__ ctl, int cond, long long N, real* __restrict__ F, int* __restrict__ dstat) {
  if (sc_skip(ctl, cond)) return;
  for (long long i = (long long)blockIdx.x * SC_BS + threadIdx.x; i < N; i += (long long)gridDim.x * SC_BS) F[i] = R(0.0);
  if (blockIdx.x == 0 && threadIdx.x == 0) { dstat[0] = 0; dstat[1] += 1; }
}

__global__ __launch_bounds__(SC_BS) void k_sc_refill(const Ctl* __restrict__ ctl, int cond, long long ne, const long long* __restrict__ epos,
                                                     const long long* __restrict__ eptr, const int* __restrict__ ta, const int* __restrict__ tb,
                                                     const int* __restrict__ trow, real sigma, const real* __restrict__ Pval,
                                                     const real* __restrict__ Aval, const real* __restrict__ rho, real* __restrict__ F) {
  if (sc_skip(ctl, cond)) return;
  for (long long e = (long long)blockIdx.x * SC_BS + threadIdx.x; e < ne; e += (long long)gridDim.x * SC_BS) {
    real s = R(0.0);
    for (long long t = eptr[e]; t < eptr[e + 1]; ++t) {
      const int b = tb[t];
      s += (b == -2) ? sigma : (b == -1) ? Pval[ta[t]] : (Aval[ta[t]] * Aval[b]) * rho[trow[t]];
    }
    F[epos[e]] = s;
  }
}

// Cholesky of one block in place (lower triangle of L, row-major, side s) by the BS threads of a workgroup; false: a pivot was not positive
template <int BS>
__device__ __forceinline__ bool sc_chol(real* L, int s, int pitch) {
  const int t = threadIdx.x;
  for (int j = 0; j < s; ++j) {
    __syncthreads();
    const real d = L[j * pitch + j];
    if (!(d > R(0.0)) || !(d < REAL_MAX)) return false;        // the same word in every thread: a uniform exit
    const real sd = sqrt(d);
    __syncthreads();
    for (int r = j + t; r < s; r += BS) L[r * pitch + j] = (r == j) ? sd : L[r * pitch + j] / sd;
    __syncthreads();
    const int w = s - j - 1;
    for (int idx = t; idx < w * w; idx += BS) {
      const int r = j + 1 + idx / w, c = j + 1 + idx % w;
      if (c <= r) L[r * pitch + c] -= L[r * pitch + j] * L[c * pitch + j];
    }
  }
  __syncthreads();
  return true;
}

// column c of the inverse of L L': forward, then backward substitution, in place in column c of Z (side s, row-major)
__device__ __forceinline__ void sc_inv_column(const real* L, real* Z, int s, int c) {
  for (int r = c; r < s; ++r) {
    real acc = (r == c) ? R(1.0) : R(0.0);
    for (int k = c; k < r; ++k) acc -= L[r * s + k] * Z[k * s + c];
    Z[r * s + c] = acc / L[r * s + r];
  }
  for (int r = s - 1; r >= 0; --r) {
    real acc = (r >= c) ? Z[r * s + c] : R(0.0);
    for (int k = r + 1; k < s; ++k) acc -= L[k * s + r] * Z[k * s + c];
    Z[r * s + c] = acc / L[r * s + r];
  }
}

// blocks of side <= 3 (93 % of BASELINE config 5's): one thread each
__global__ __launch_bounds__(SC_BS) void k_sc_small(Ctl* __restrict__ ctl, int cond, int nblk, const int* __restrict__ comp_ptr,
                                                    const long long* __restrict__ boff, real* __restrict__ F, real* __restrict__ Z,
                                                    int* __restrict__ dstat) {
  if (sc_skip(ctl, cond)) return;
  for (int k = blockIdx.x * SC_BS + threadIdx.x; k < nblk; k += gridDim.x * SC_BS) {
    const int s = comp_ptr[k + 1] - comp_ptr[k];
    real* L = F + boff[k];
    bool ok = true;
    for (int j = 0; j < s && ok; ++j) {
      const real d = L[j * s + j];
      if (!(d > R(0.0)) || !(d < REAL_MAX)) { ok = false; break; }
      const real sd = sqrt(d);
      L[j * s + j] = sd;
      for (int r = j + 1; r < s; ++r) L[r * s + j] = L[r * s + j] / sd;
      for (int r = j + 1; r < s; ++r)
        for (int c = j + 1; c <= r; ++c) L[r * s + c] -= L[r * s + j] * L[c * s + j];
    }
    if (!ok) { sc_bad_pivot(ctl, cond, dstat); continue; }
    for (int c = 0; c < s; ++c) sc_inv_column(L, Z + boff[k], s, c);
  }
}

// blocks of side <= BS: one workgroup of BS threads each (BS = 64: one wave), the Cholesky by all threads, then one column of the inverse per thread
template <int BS>
__global__ __launch_bounds__(BS) void k_sc_block(Ctl* __restrict__ ctl, int cond, int first, const int* __restrict__ comp_ptr,
                                                 const long long* __restrict__ boff, real* __restrict__ F, real* __restrict__ Z,
                                                 int* __restrict__ dstat) {
  if (sc_skip(ctl, cond)) return;
  const int k = first + blockIdx.x;
  const int s = comp_ptr[k + 1] - comp_ptr[k];
  real* L = F + boff[k];
  if (!sc_chol<BS>(L, s, s)) {
    if (threadIdx.x == 0) sc_bad_pivot(ctl, cond, dstat);
    return;
  }
  for (int c = threadIdx.x; c < s; c += BS) sc_inv_column(L, Z + boff[k], s, c);
}

// ---- the capacitance matrix ---------------------------------------------------------------------------------------------
// Row k of C by one workgroup: w = M_s^-1 A_d[k, :]' in the workgroup's n-vector of scratch (the entries of the row one after the other, so that two
// entries in one block add in a fixed order), then C[k, l] = A_d[l, :] w for every l, then w is cleared again.  Rows k >= nd are the identity padding.
__global__ __launch_bounds__(SC_BS) void k_sc_formC(const Ctl* __restrict__ ctl, int cond, int nd, int ndp, long long n, real* __restrict__ wbuf,
                                                    const int* __restrict__ ad_ptr, const int* __restrict__ ad_col, const int* __restrict__ ad_src,
                                                    const int* __restrict__ ad_row, const real* __restrict__ Aval, const real* __restrict__ rho,
                                                    const int* __restrict__ perm, const int* __restrict__ pos, const int* __restrict__ blk_of_pos,
                                                    const int* __restrict__ comp_ptr, const long long* __restrict__ boff,
                                                    const real* __restrict__ Z, real* __restrict__ C) {
  if (sc_skip(ctl, cond)) return;
  real* w = wbuf + (size_t)blockIdx.x * (size_t)n;
  const int t = threadIdx.x;
  for (int k = blockIdx.x; k < ndp; k += gridDim.x) {
    const int p0 = k < nd ? ad_ptr[k] : 0, p1 = k < nd ? ad_ptr[k + 1] : 0;
    for (int p = p0; p < p1; ++p) {
      const int pi = pos[ad_col[p]];
      const int b = blk_of_pos[pi];
      const int base = comp_ptr[b], s = comp_ptr[b + 1] - base;
      const real a = Aval[ad_src[p]];
      const real* Zb = Z + boff[b];
      for (int r = t; r < s; r += SC_BS) w[perm[base + r]] += Zb[(size_t)r * s + (pi - base)] * a;
      __syncthreads();
    }
    for (int l = t; l < ndp; l += SC_BS) {
      real acc = R(0.0);
      if (l < nd)
        for (int q = ad_ptr[l]; q < ad_ptr[l + 1]; ++q) acc += Aval[ad_src[q]] * w[ad_col[q]];
      if (l == k) acc += (k < nd) ? R(1.0) / rho[ad_row[k]] : R(1.0);
      C[(size_t)k * ndp + l] = acc;
    }
    __syncthreads();
    for (int p = p0; p < p1; ++p) {
      const int pi = pos[ad_col[p]];
      const int b = blk_of_pos[pi];
      const int base = comp_ptr[b], s = comp_ptr[b + 1] - base;
      for (int r = t; r < s; r += SC_BS) w[perm[base + r]] = R(0.0);
    }
    __syncthreads();
  }
}

// ---- dense Cholesky of C and its inverse -----------------------------------------------------------------------------------
// Diagonal block k: Cholesky in LDS, the inverse of the triangle next to it (Z(r, c), r >= c, lives at A[c][r + 1]: the strict upper triangle of the
// 64 x 65 array, which the factor does not use).  L_kk goes back to C (zeros above the diagonal), its inverse to the same tile of Li.
__global__ __launch_bounds__(SC_BS) void k_sc_potrf(Ctl* __restrict__ ctl, int cond, int k, real* __restrict__ C, real* __restrict__ Li, int ld,
                                                    int* __restrict__ dstat) {
  if (sc_skip(ctl, cond)) return;
  __shared__ real A[SC_NB * (SC_NB + 1)];
  const int t = threadIdx.x;
  real* Ck = C + ((size_t)k * SC_NB) * ld + (size_t)k * SC_NB;
  real* Lk = Li + ((size_t)k * SC_NB) * ld + (size_t)k * SC_NB;
  for (int idx = t; idx < SC_NB * SC_NB; idx += SC_BS) { const int r = idx / SC_NB, c = idx % SC_NB; A[r * (SC_NB + 1) + c] = Ck[(size_t)r * ld + c]; }
  if (!sc_chol<SC_BS>(A, SC_NB, SC_NB + 1)) {
    if (t == 0) sc_bad_pivot(ctl, cond, dstat);
    return;
  }
  if (t < SC_NB) {
    const int c = t;
    for (int r = c; r < SC_NB; ++r) {
      real acc = (r == c) ? R(1.0) : R(0.0);
      for (int q = c; q < r; ++q) acc -= A[r * (SC_NB + 1) + q] * A[c * (SC_NB + 1) + q + 1];
      A[c * (SC_NB + 1) + r + 1] = acc / A[r * (SC_NB + 1) + r];
    }
  }
  __syncthreads();
  for (int idx = t; idx < SC_NB * SC_NB; idx += SC_BS) {
    const int r = idx / SC_NB, c = idx % SC_NB;
    Ck[(size_t)r * ld + c] = (c <= r) ? A[r * (SC_NB + 1) + c] : R(0.0);
    Lk[(size_t)r * ld + c] = (c <= r) ? A[c * (SC_NB + 1) + r + 1] : R(0.0);
  }
}

// The one tile kernel: out <- alpha out + beta sum over kk in [k0, k1) of X_kk Y_kk, all tiles SC_NB x SC_NB, X_kk(r, c) = xb[kk xstep + r xrs + c xcs]
// and Y_kk(c, j) = yb[kk ystep + c yrs + j ycs] (a transposed operand is a pair of swapped strides).  Four waves, wave w owns rows 16 w .. 16 w + 15 of
// the tile as four 16 x 16 accumulators of the 16x16x4 matrix instruction; the operands pass through LDS in k-chunks of SC_KC.  An operand may be the
// output tile itself: every read of it is complete before the first store.
enum { SC_PANEL = 0, SC_TRAIL, SC_LINV_SUM, SC_LINV_MUL, SC_PROD };
__global__ __launch_bounds__(SC_BS) void k_sc_tile(const Ctl* __restrict__ ctl, int cond, int mode, int k, int T, real* __restrict__ C,
                                                   real* __restrict__ Li, int ld) {
  if (sc_skip(ctl, cond)) return;
  __shared__ real As[SC_NB * (SC_KC + 1)];
  __shared__ real Bs[SC_KC * (SC_NB + 1)];
  const size_t NB = SC_NB, LD = (size_t)ld;
  real* out; const real* xb; const real* yb;
  size_t xstep = 0, xrs = LD, xcs = 1, ystep = 0, yrs = LD, ycs = 1;
  int k0 = 0, k1 = 1;
  real alpha = R(0.0), beta = R(1.0);
  switch (mode) {
    case SC_PANEL: {           // L_ik = C_ik L_kk^-T
      const size_t ti = (size_t)k + 1 + blockIdx.x;
      out = C + ti * NB * LD + (size_t)k * NB; xb = out;
      yb = Li + (size_t)k * NB * LD + (size_t)k * NB; yrs = 1; ycs = LD;
      break;
    }
    case SC_TRAIL: {           // C_ij -= L_ik L_jk', lower triangle of tiles
      const size_t ti = (size_t)k + 1 + blockIdx.x, tj = (size_t)k + 1 + blockIdx.y;
      if (tj > ti) return;
      out = C + ti * NB * LD + tj * NB; xb = C + ti * NB * LD + (size_t)k * NB;
      yb = C + tj * NB * LD + (size_t)k * NB; yrs = 1; ycs = LD;
      alpha = R(1.0); beta = R(-1.0);
      break;
    }
    case SC_LINV_SUM: {        // S_ij = sum_{kk = j}^{i - 1} L_i,kk Linv_kk,j  (i = k)
      const size_t tj = blockIdx.x;
      out = Li + (size_t)k * NB * LD + tj * NB;
      xb = C + (size_t)k * NB * LD; xstep = NB;
      yb = Li + tj * NB; ystep = NB * LD;
      k0 = (int)tj; k1 = k;
      break;
    }
    case SC_LINV_MUL: {        // Linv_ij = -Linv_ii S_ij
      const size_t tj = blockIdx.x;
      out = Li + (size_t)k * NB * LD + tj * NB;
      xb = Li + (size_t)k * NB * LD + (size_t)k * NB;
      yb = out;
      beta = R(-1.0);
      break;
    }
    default: {                 // C^-1_ij = sum_{kk >= max(i, j)} Linv_kk,i' Linv_kk,j
      const size_t ti = blockIdx.x, tj = blockIdx.y;
      out = C + ti * NB * LD + tj * NB;
      xb = Li + ti * NB; xstep = NB * LD; xrs = 1; xcs = LD;
      yb = Li + tj * NB; ystep = NB * LD;
      k0 = (int)(ti > tj ? ti : tj); k1 = T;
      break;
    }
  }
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l15 = lane & 15, l4 = lane >> 4;
  v4d acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = v4d{R(0.0), R(0.0), R(0.0), R(0.0)};
  for (int kk = k0; kk < k1; ++kk) {
    const real* X = xb + (size_t)kk * xstep;
    const real* Y = yb + (size_t)kk * ystep;
    for (int hc = 0; hc < SC_NB / SC_KC; ++hc) {
      __syncthreads();
      for (int idx = t; idx < SC_NB * SC_KC; idx += SC_BS) {
        // neighbouring threads walk the operand's unit stride
        const int r = (xcs == 1) ? idx / SC_KC : idx % SC_NB, c = (xcs == 1) ? idx % SC_KC : idx / SC_NB;
        As[r * (SC_KC + 1) + c] = X[(size_t)r * xrs + (size_t)(hc * SC_KC + c) * xcs];
        const int cy = (ycs == 1) ? idx / SC_NB : idx % SC_KC, j = (ycs == 1) ? idx % SC_NB : idx / SC_KC;
        Bs[cy * (SC_NB + 1) + j] = Y[(size_t)(hc * SC_KC + cy) * yrs + (size_t)j * ycs];
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < SC_KC; q += 4) {
        const real a = As[(16 * wv + l15) * (SC_KC + 1) + q + l4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = MFMA_REAL(a, Bs[(q + l4) * (SC_NB + 1) + 16 * c + l15], acc[c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      real* o = out + (size_t)(16 * wv + ACC_ROW(lane, q)) * LD + 16 * c + l15;
      const real prev = (alpha != R(0.0)) ? *o : R(0.0);
      *o = alpha * prev + beta * acc[c][q];
    }
}

// ---- the solve ---------------------------------------------------------------------------------------------------------------
// out = a0 + a1 + sgn (M_s^-1 vin) (a0, a1 nullable): one thread per variable, the row of its block's inverse read as a column (the inverse is symmetric)
__global__ __launch_bounds__(SC_BS) void k_sc_bapply(long long n, const int* __restrict__ perm, const int* __restrict__ blk_of_pos,
                                                     const int* __restrict__ comp_ptr, const long long* __restrict__ boff, const real* __restrict__ Z,
                                                     const real* __restrict__ vin, const real* __restrict__ a0, const real* __restrict__ a1, real sgn,
                                                     real* __restrict__ out) {
  for (long long p = (long long)blockIdx.x * SC_BS + threadIdx.x; p < n; p += (long long)gridDim.x * SC_BS) {
    const int b = blk_of_pos[p];
    const int base = comp_ptr[b], s = comp_ptr[b + 1] - base;
    const real* Zb = Z + boff[b];
    const int r = (int)p - base;
    real acc = R(0.0);
    for (int c = 0; c < s; ++c) acc += Zb[(size_t)c * s + r] * vin[perm[base + c]];
    const int i = perm[p];
    real o = sgn * acc;
    if (a1) o = a1[i] + o;
    if (a0) o = a0[i] + o;
    out[i] = o;
  }
}

// t = A_d y: one thread per long row, the row's entries left to right
__global__ __launch_bounds__(SC_BS) void k_sc_ad(int nd, const int* __restrict__ ad_ptr, const int* __restrict__ ad_col, const int* __restrict__ ad_src,
                                                 const real* __restrict__ Aval, const real* __restrict__ y, real* __restrict__ tn) {
  for (int k = blockIdx.x * SC_BS + threadIdx.x; k < nd; k += gridDim.x * SC_BS) {
    real acc = R(0.0);
    for (int p = ad_ptr[k]; p < ad_ptr[k + 1]; ++p) acc += Aval[ad_src[p]] * y[ad_col[p]];
    tn[k] = acc;
  }
}

// v = A_d' u: one thread per variable
__global__ __launch_bounds__(SC_BS) void k_sc_adt(long long n, const int* __restrict__ adt_ptr, const int* __restrict__ adt_k, const int* __restrict__ adt_src,
                                                  const real* __restrict__ Aval, const real* __restrict__ un, real* __restrict__ v) {
  for (long long j = (long long)blockIdx.x * SC_BS + threadIdx.x; j < n; j += (long long)gridDim.x * SC_BS) {
    real acc = R(0.0);
    for (int p = adt_ptr[j]; p < adt_ptr[j + 1]; ++p) acc += Aval[adt_src[p]] * un[adt_k[p]];
    v[j] = acc;
  }
}

// u = C^-1 t, the byte-heavy kernel: one workgroup per row, 16-byte loads of the row and of t (both padded to ndp, a multiple of 64), block_sum
typedef real sc_vec __attribute__((ext_vector_type(16 / sizeof(real))));
__global__ __launch_bounds__(SC_BS) void k_sc_dense(int ndp, const real* __restrict__ Ci, const real* __restrict__ tn, real* __restrict__ un) {
  __shared__ real red[COSMO_BS / 64];
  constexpr int VW = 16 / sizeof(real);
  const sc_vec* row = reinterpret_cast<const sc_vec*>(Ci + (size_t)blockIdx.x * ndp);
  const sc_vec* tv = reinterpret_cast<const sc_vec*>(tn);
  real acc = R(0.0);
  for (int j = threadIdx.x; j < ndp / VW; j += SC_BS) {
    const sc_vec a = row[j], b = tv[j];
#pragma unroll
    for (int e = 0; e < VW; ++e) acc += a[e] * b[e];
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) un[blockIdx.x] = acc;
}

// ---- refinement --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_BS) void k_sc_scale(long long m, const real* __restrict__ rho, real* __restrict__ tm) {
  for (long long i = (long long)blockIdx.x * SC_BS + threadIdx.x; i < m; i += (long long)gridDim.x * SC_BS) tm[i] = rho[i] * tm[i];
}
// r = rhs - (P x + sigma x + A' rho A x) and the partial sums of r' r; with x == nullptr: the partial sums of rhs' rhs
__global__ __launch_bounds__(SC_BS) void k_sc_resid(long long n, const real* __restrict__ rhs, const real* __restrict__ Px, const real* __restrict__ Ax,
                                                    real sigma, const real* __restrict__ x, real* __restrict__ r, real* __restrict__ part) {
  __shared__ real red[COSMO_BS / 64];
  real acc = R(0.0);
  for (long long i = (long long)blockIdx.x * SC_BS + threadIdx.x; i < n; i += (long long)gridDim.x * SC_BS) {
    real ri = rhs[i];
    if (x) { ri = ri - ((Px[i] + sigma * x[i]) + Ax[i]); r[i] = ri; }
    acc += ri * ri;
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
// before the first step: ||rhs||^2 and the residual of the unrefined x
__global__ __launch_bounds__(SC_BS) void k_sc_init(const real* __restrict__ part_rhs, const real* __restrict__ part_r, int np, ScScal* __restrict__ sc) {
  __shared__ real red[COSMO_BS / 64];
  const real a = reduce_partials_sum(part_rhs, np, red);
  const real b = reduce_partials_sum(part_r, np, red);
  if (threadIdx.x == 0) { sc->rhs2 = a; sc->best[0] = b; sc->stop[0] = 0; sc->taken = 0; }
}
// step s: the candidate (xc, rc) replaces (x, r) if no earlier step was rejected and its residual norm fell.  Every workgroup takes the same decision from
// the words of step s - 1; workgroup 0 records those of step s.
__global__ __launch_bounds__(SC_BS) void k_sc_accept(int step, long long n, ScScal* __restrict__ sc, const real* __restrict__ part, int np,
                                                     real* __restrict__ x, const real* __restrict__ xc, real* __restrict__ r, const real* __restrict__ rc,
                                                     int* __restrict__ dstat) {
  __shared__ real red[COSMO_BS / 64];
  const real cand = reduce_partials_sum(part, np, red);
  const real best = sc->best[step - 1];
  const int stopped = sc->stop[step - 1];
  const bool keep = !stopped && cand < best;
  if (keep)
    for (long long i = (long long)blockIdx.x * SC_BS + threadIdx.x; i < n; i += (long long)gridDim.x * SC_BS) { x[i] = xc[i]; r[i] = rc[i]; }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    sc->best[step] = keep ? cand : best;
    sc->stop[step] = keep ? 0 : 1;
    if (keep) sc->taken = step;
    else if (!stopped) dstat[3] += 1;
  }
}
// x_tl = x, the two residual ratios, and the tail's "solve finished" flag (cg_k stays 0: no Krylov iterations)
__global__ __launch_bounds__(SC_BS) void k_sc_finish(Ctl* __restrict__ ctl, int guard, long long n, const real* __restrict__ x, real* __restrict__ x_tl,
                                                     ScScal* __restrict__ sc, int last) {
  if (guard && ctl->halt) return;
  for (long long i = (long long)blockIdx.x * SC_BS + threadIdx.x; i < n; i += (long long)gridDim.x * SC_BS) x_tl[i] = x[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const real nb = sqrt(sc->rhs2);
    sc->ratio[0] = nb > R(0.0) ? sqrt(sc->best[last]) / nb : R(0.0);
    sc->ratio[1] = nb > R(0.0) ? sqrt(sc->best[0]) / nb : R(0.0);
    ctl->cg_done = 1;
    ctl->cg_k = 0;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
void free_dev(SchurDev* D) {
  dfree(&D->perm); dfree(&D->pos); dfree(&D->blk_of_pos); dfree(&D->comp_ptr); dfree(&D->boff); dfree(&D->epos); dfree(&D->eptr);
  dfree(&D->ta); dfree(&D->tb); dfree(&D->trow); dfree(&D->ad_row); dfree(&D->ad_ptr); dfree(&D->ad_col); dfree(&D->ad_src);
  dfree(&D->adt_ptr); dfree(&D->adt_k); dfree(&D->adt_src); dfree(&D->Bfac); dfree(&D->Binv); dfree(&D->C); dfree(&D->Li); dfree(&D->wbuf);
  dfree(&D->y); dfree(&D->v); dfree(&D->x); dfree(&D->xc); dfree(&D->r); dfree(&D->rc); dfree(&D->t1); dfree(&D->t2); dfree(&D->tn); dfree(&D->un);
  dfree(&D->parts); dfree(&D->scal); dfree(&D->dstat);
}

int32_t enqueue_factor(cosmo_hip_handle* h, int cond) {
  SchurDev* D = dev_of(h);
  const SchurPlan& S = D->S;
  hipStream_t st = h->stream;
  const long long ne = (long long)S.epos.size();
  hipLaunchKernelGGL(k_sc_zero, dim3(ew(S.sumsq)), dim3(SC_BS), 0, st, h->ctl, cond, (long long)S.sumsq, D->Bfac, D->dstat);
  hipLaunchKernelGGL(k_sc_refill, dim3(ew(ne)), dim3(SC_BS), 0, st, h->ctl, cond, ne, D->epos, D->eptr, D->ta, D->tb, D->trow, (real)h->prm.sigma,
                     h->P.val, h->A.val, h->rho, D->Bfac);
  if (S.n_small > 0)
    hipLaunchKernelGGL(k_sc_small, dim3(ew(S.n_small)), dim3(SC_BS), 0, st, h->ctl, cond, S.n_small, D->comp_ptr, D->boff, D->Bfac, D->Binv, D->dstat);
  if (S.n_wave > S.n_small)
    hipLaunchKernelGGL(k_sc_block<64>, dim3(S.n_wave - S.n_small), dim3(64), 0, st, h->ctl, cond, S.n_small, D->comp_ptr, D->boff, D->Bfac, D->Binv, D->dstat);
  if ((int)S.ncomp > S.n_wave)
    hipLaunchKernelGGL(k_sc_block<SC_BS>, dim3((int)S.ncomp - S.n_wave), dim3(SC_BS), 0, st, h->ctl, cond, S.n_wave, D->comp_ptr, D->boff, D->Bfac, D->Binv,
                       D->dstat);
  if (S.nd > 0) {
    const int T = D->T, ld = D->ndp;
    hipLaunchKernelGGL(k_sc_formC, dim3(std::min(D->ndp, SC_FORMC_GRID)), dim3(SC_BS), 0, st, h->ctl, cond, (int)S.nd, D->ndp, h->n, D->wbuf, D->ad_ptr,
                       D->ad_col, D->ad_src, D->ad_row, h->A.val, h->rho, D->perm, D->pos, D->blk_of_pos, D->comp_ptr, D->boff, D->Binv, D->C);
    for (int k = 0; k < T; ++k) {
      hipLaunchKernelGGL(k_sc_potrf, dim3(1), dim3(SC_BS), 0, st, h->ctl, cond, k, D->C, D->Li, ld, D->dstat);
      if (k + 1 < T) {
        hipLaunchKernelGGL(k_sc_tile, dim3(T - k - 1), dim3(SC_BS), 0, st, h->ctl, cond, (int)SC_PANEL, k, T, D->C, D->Li, ld);
        hipLaunchKernelGGL(k_sc_tile, dim3(T - k - 1, T - k - 1), dim3(SC_BS), 0, st, h->ctl, cond, (int)SC_TRAIL, k, T, D->C, D->Li, ld);
      }
    }
    for (int i = 1; i < T; ++i) {
      hipLaunchKernelGGL(k_sc_tile, dim3(i), dim3(SC_BS), 0, st, h->ctl, cond, (int)SC_LINV_SUM, i, T, D->C, D->Li, ld);
      hipLaunchKernelGGL(k_sc_tile, dim3(i), dim3(SC_BS), 0, st, h->ctl, cond, (int)SC_LINV_MUL, i, T, D->C, D->Li, ld);
    }
    hipLaunchKernelGGL(k_sc_tile, dim3(T, T), dim3(SC_BS), 0, st, h->ctl, cond, (int)SC_PROD, 0, T, D->C, D->Li, ld);
  }
  HIPCHK(h, hipGetLastError());
  return COSMO_HIP_OK;
}

// out = a0 + M^-1 in (a0 nullable); `in` is not modified
int32_t enqueue_apply(cosmo_hip_handle* h, const real* in, const real* a0, real* out) {
  SchurDev* D = dev_of(h);
  const SchurPlan& S = D->S;
  hipStream_t st = h->stream;
  const int gn = ew(h->n);
  if (S.nd == 0) {
    hipLaunchKernelGGL(k_sc_bapply, dim3(gn), dim3(SC_BS), 0, st, h->n, D->perm, D->blk_of_pos, D->comp_ptr, D->boff, D->Binv, in, a0, (const real*)nullptr,
                       R(1.0), out);
  } else {
    hipLaunchKernelGGL(k_sc_bapply, dim3(gn), dim3(SC_BS), 0, st, h->n, D->perm, D->blk_of_pos, D->comp_ptr, D->boff, D->Binv, in, (const real*)nullptr,
                       (const real*)nullptr, R(1.0), D->y);
    hipLaunchKernelGGL(k_sc_ad, dim3(ew(S.nd)), dim3(SC_BS), 0, st, (int)S.nd, D->ad_ptr, D->ad_col, D->ad_src, h->A.val, D->y, D->tn);
    hipLaunchKernelGGL(k_sc_dense, dim3((int)S.nd), dim3(SC_BS), 0, st, D->ndp, D->C, D->tn, D->un);
    hipLaunchKernelGGL(k_sc_adt, dim3(gn), dim3(SC_BS), 0, st, h->n, D->adt_ptr, D->adt_k, D->adt_src, h->A.val, D->un, D->v);
    hipLaunchKernelGGL(k_sc_bapply, dim3(gn), dim3(SC_BS), 0, st, h->n, D->perm, D->blk_of_pos, D->comp_ptr, D->boff, D->Binv, D->v, a0, D->y, R(-1.0), out);
  }
  HIPCHK(h, hipGetLastError());
  return COSMO_HIP_OK;
}

// r = rhs - M x through the handle's own copies of P, A and A' (M = P + sigma I + A' rho A), the partial sums of r' r into slot `slot`
int32_t enqueue_residual(cosmo_hip_handle* h, const real* x, real* r, int slot) {
  SchurDev* D = dev_of(h);
  hipStream_t st = h->stream;
  CHK(launch_spmv_plain(h, h->P, x, D->t1));
  CHK(launch_spmv_plain(h, h->A, x, h->tmp_m));
  if (h->m > 0) hipLaunchKernelGGL(k_sc_scale, dim3(ew(h->m)), dim3(SC_BS), 0, st, h->m, h->rho, h->tmp_m);
  CHK(launch_spmv_plain(h, h->AT, h->tmp_m, D->t2));
  hipLaunchKernelGGL(k_sc_resid, dim3(ew(h->n)), dim3(SC_BS), 0, st, h->n, h->rhs, D->t1, D->t2, (real)h->prm.sigma, x, r,
                     D->parts + (size_t)slot * COSMO_MAX_PARTIALS);
  HIPCHK(h, hipGetLastError());
  return COSMO_HIP_OK;
}
}  // namespace

void schur_free(cosmo_hip_handle* h) {
  SchurDev* D = dev_of(h);
  if (!D) return;
  free_dev(D);
  delete D;
  h->schur = nullptr;
}

// a factorisation outside the loop (setup, update_rho, update_matrices): synchronised, timed, pivots checked
int32_t schur_refactor_now(cosmo_hip_handle* h) {
  SchurDev* D = dev_of(h);
  if (!D) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "Schur-complement KKT solver: not set up (set_params with kkt_kind SCHUR failed or was not called)");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const auto t0 = std::chrono::steady_clock::now();
  CHK(enqueue_factor(h, 0));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  D->last_factor_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  int st[4];
  HIPCHK(h, hipMemcpy(st, D->dstat, sizeof st, hipMemcpyDeviceToHost));
  if (st[0]) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "Schur-complement KKT solver: non-positive pivot in a block of M_s or in the capacitance matrix "
                               "(Objective function is not convex.)");
  return COSMO_HIP_OK;
}

int32_t schur_enqueue_refactor(cosmo_hip_handle* h, int cond) {
  if (!dev_of(h)) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "Schur-complement KKT solver: not set up");
  return enqueue_factor(h, cond);
}

int32_t schur_setup(cosmo_hip_handle* h) {
  schur_free(h);
  const long long n = h->n, m = h->m;
  std::vector<int> prp(n + 1), pcol(h->P.nnz), arp(m + 1), acol(h->A.nnz);
  HIPCHK(h, hipMemcpy(prp.data(), h->P.rowptr, sizeof(int) * (n + 1), hipMemcpyDeviceToHost));
  if (h->P.nnz) HIPCHK(h, hipMemcpy(pcol.data(), h->P.col, sizeof(int) * h->P.nnz, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(arp.data(), h->A.rowptr, sizeof(int) * (m + 1), hipMemcpyDeviceToHost));
  if (h->A.nnz) HIPCHK(h, hipMemcpy(acol.data(), h->A.col, sizeof(int) * h->A.nnz, hipMemcpyDeviceToHost));
  SchurDev* D = new SchurDev();
  h->schur = D;
  const char* err = nullptr;
  if (schur_analyze(n, m, prp, pcol, arp, acol, h->sc_row_threshold, D->S, &err) != 0) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "%s", err);
  const SchurPlan& S = D->S;
  const long long nd_max = h->sc_nd_max > 0 ? h->sc_nd_max : SCHUR_ND_MAX_DEFAULT, block_max = h->sc_block_max > 0 ? h->sc_block_max : SCHUR_BLOCK_MAX_DEFAULT;
  switch (schur_check_limits(S, nd_max, std::min<long long>(block_max, SCHUR_BLOCK_MAX_DEFAULT), (int)sizeof(real))) {
    case 1: return cosmo_fail(h, COSMO_HIP_ERR_UNSUPPORTED, "kkt_kind SCHUR: %lld rows of A have at least %d entries, more than nd_max = %lld", (long long)S.nd, S.row_threshold, nd_max);
    case 2: return cosmo_fail(h, COSMO_HIP_ERR_UNSUPPORTED, "kkt_kind SCHUR: the largest block of M_s has side %lld, more than block_max = %lld (the kernels' own bound is %d)",
                              (long long)S.largest, block_max, SCHUR_BLOCK_MAX_DEFAULT);
    case 3: return cosmo_fail(h, COSMO_HIP_ERR_UNSUPPORTED, "kkt_kind SCHUR: the capacitance matrix of side %lld and its inverse take %lld bytes, more than the budget of %lld",
                              (long long)S.nd, (long long)schur_dense_bytes(S.nd, (int)sizeof(real)), (long long)SCHUR_MEM_BUDGET);
    default: break;
  }
  D->refine_steps = h->sc_refine_steps;
  D->ndp = (int)((S.nd + SC_NB - 1) / SC_NB * SC_NB);
  D->T = D->ndp / SC_NB;
  CHK(up(h, &D->perm, S.perm)); CHK(up(h, &D->pos, S.pos)); CHK(up(h, &D->blk_of_pos, S.blk_of_pos)); CHK(up(h, &D->comp_ptr, S.comp_ptr));
  CHK(up(h, &D->boff, S.boff)); CHK(up(h, &D->epos, S.epos)); CHK(up(h, &D->eptr, S.eptr));
  CHK(up(h, &D->ta, S.ta)); CHK(up(h, &D->tb, S.tb)); CHK(up(h, &D->trow, S.trow));
  CHK(up(h, &D->ad_row, S.ad_row)); CHK(up(h, &D->ad_ptr, S.ad_ptr)); CHK(up(h, &D->ad_col, S.ad_col)); CHK(up(h, &D->ad_src, S.ad_src));
  CHK(up(h, &D->adt_ptr, S.adt_ptr)); CHK(up(h, &D->adt_k, S.adt_k)); CHK(up(h, &D->adt_src, S.adt_src));
  CHK(dnew(h, &D->Bfac, (size_t)S.sumsq, true)); CHK(dnew(h, &D->Binv, (size_t)S.sumsq, true));
  if (S.nd > 0) {
    CHK(dnew(h, &D->C, (size_t)D->ndp * D->ndp, true)); CHK(dnew(h, &D->Li, (size_t)D->ndp * D->ndp, true));
    CHK(dnew(h, &D->wbuf, (size_t)std::min(D->ndp, SC_FORMC_GRID) * (size_t)n, true));
    CHK(dnew(h, &D->tn, (size_t)D->ndp, true)); CHK(dnew(h, &D->un, (size_t)D->ndp, true));
  }
  CHK(dnew(h, &D->y, (size_t)n, true)); CHK(dnew(h, &D->v, (size_t)n, true)); CHK(dnew(h, &D->x, (size_t)n, true)); CHK(dnew(h, &D->xc, (size_t)n, true));
  CHK(dnew(h, &D->r, (size_t)n, true)); CHK(dnew(h, &D->rc, (size_t)n, true)); CHK(dnew(h, &D->t1, (size_t)n, true)); CHK(dnew(h, &D->t2, (size_t)n, true));
  CHK(dnew(h, &D->parts, (size_t)(SCHUR_REFINE_STEPS_MAX + 2) * COSMO_MAX_PARTIALS, true));
  CHK(dnew(h, &D->scal, 1, true)); CHK(dnew(h, &D->dstat, 4, true));
  return schur_refactor_now(h);
}

// x_tl = M^-1 rhs with refinement; h->rhs holds the right-hand side (enqueue_cg_rhs)
int32_t schur_enqueue_solve(cosmo_hip_handle* h, int guard) {
  SchurDev* D = dev_of(h);
  if (!D) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "Schur-complement KKT solver: not set up");
  hipStream_t st = h->stream;
  const int np = ew(h->n);
  prof_begin(h, KC_OP_APPLY);
  hipLaunchKernelGGL(k_sc_resid, dim3(np), dim3(SC_BS), 0, st, h->n, h->rhs, (const real*)nullptr, (const real*)nullptr, R(0.0), (const real*)nullptr,
                     (real*)nullptr, D->parts);
  CHK(enqueue_apply(h, h->rhs, nullptr, D->x));
  CHK(enqueue_residual(h, D->x, D->r, 1));
  hipLaunchKernelGGL(k_sc_init, dim3(1), dim3(SC_BS), 0, st, D->parts, D->parts + COSMO_MAX_PARTIALS, np, D->scal);
  for (int s = 1; s <= D->refine_steps; ++s) {
    CHK(enqueue_apply(h, D->r, D->x, D->xc));
    CHK(enqueue_residual(h, D->xc, D->rc, 1 + s));
    hipLaunchKernelGGL(k_sc_accept, dim3(np), dim3(SC_BS), 0, st, s, h->n, D->scal, D->parts + (size_t)(1 + s) * COSMO_MAX_PARTIALS, np, D->x, D->xc, D->r,
                       D->rc, D->dstat);
  }
  hipLaunchKernelGGL(k_sc_finish, dim3(np), dim3(SC_BS), 0, st, h->ctl, guard, h->n, D->x, h->x_tl, D->scal, D->refine_steps);
  prof_end(h);
  HIPCHK(h, hipGetLastError());
  return COSMO_HIP_OK;
}

int32_t schur_info(cosmo_hip_handle* h, int64_t* out) {
  SchurDev* D = dev_of(h);
  if (!D) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "schur_info: the handle has no Schur-complement KKT solver (kkt_kind COSMO_HIP_KKT_SCHUR)");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int st[4];
  ScScal sc;
  HIPCHK(h, hipMemcpy(st, D->dstat, sizeof st, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(&sc, D->scal, sizeof sc, hipMemcpyDeviceToHost));
  const SchurPlan& S = D->S;
  out[0] = S.nd; out[1] = S.ncomp; out[2] = S.largest; out[3] = S.sumsq; out[4] = S.nnz_w; out[5] = st[1]; out[6] = sc.taken; out[7] = st[3];
  return COSMO_HIP_OK;
}

int32_t schur_residual(cosmo_hip_handle* h, double* out) {
  SchurDev* D = dev_of(h);
  if (!D) return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "schur_residual: the handle has no Schur-complement KKT solver (kkt_kind COSMO_HIP_KKT_SCHUR)");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ScScal sc;
  HIPCHK(h, hipMemcpy(&sc, D->scal, sizeof sc, hipMemcpyDeviceToHost));
  out[0] = (double)sc.ratio[0]; out[1] = (double)sc.ratio[1];
  return COSMO_HIP_OK;
}

bool schur_describe(const cosmo_hip_handle* h, char* buf, size_t len) {
  const SchurDev* D = (const SchurDev*)h->schur;
  if (!D) return false;
  snprintf(buf, len, "schur: exact reduced solve by Woodbury, %lld blocks of M_s (largest %lld) and a dense %lld x %lld capacitance inverse, %d refinement steps (csrc/schur.hip, opt-in)",
           (long long)D->S.ncomp, (long long)D->S.largest, (long long)D->S.nd, (long long)D->S.nd, D->refine_steps);
  return true;
}
