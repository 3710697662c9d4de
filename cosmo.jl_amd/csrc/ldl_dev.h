// ldl_dev.h -- the per-supernode steps of the supernodal LDL' (panel layout of ldl.h) as device functions of ONE workgroup of BS threads.
// ldl.hip runs them one launch per tree level (one workgroup per supernode of the level); batch_ldl.h walks all supernodes of a problem inside
// the problem's persistent workgroup.  Every step ends with a workgroup barrier behind its last write, so a caller may run the next supernode
// (a parent, or in the backward solve a child) right behind it.  No atomics, a fixed summation order: the factor is bitwise reproducible.
#pragma once
#include "device_utils.h"

// row position of permuted row `row` in rows_J (the columns of J come first, the rest is ascending)
__device__ __forceinline__ int ldl_rowpos(const int* __restrict__ rows, int w, int nr, long long f, int row) {
  if (row < f + w) return (int)(row - f);
  int lo = w, hi = nr - 1;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (rows[mid] < row) lo = mid + 1; else hi = mid; }
  return lo;
}

// Left-looking factorisation of supernode J (its panel holds the refilled values of K):
//   1. for every descendant K of J in ascending order: panel_J -= L_K[r0:, :] D_K L_K[r0:r1, :]'  (each entry of the update is owned by one
//      thread; a barrier between descendants);
//   2. dense LDL' of the diagonal block without pivoting (K is quasi-definite: it exists for every symmetric permutation) and the scaling of the
//      panel below it.
// Thread 0 adds the positive pivots of J to `pos` and sets `bad` on a zero or non-finite pivot (other threads: untouched).
template <int BS>
__device__ __forceinline__ void ldl_factor_sn(int J, const int* __restrict__ sn_first, const long long* __restrict__ sn_rp, const int* __restrict__ sn_rows,
                                              const long long* __restrict__ sn_poff, const int* __restrict__ desc_ptr, const int* __restrict__ desc,
                                              real* __restrict__ Lx, int& pos, bool& bad) {
  const int tid = threadIdx.x;
  const long long f = sn_first[J];
  const int w = sn_first[J + 1] - (int)f;
  const int nr = (int)(sn_rp[J + 1] - sn_rp[J]);
  const int* rows = sn_rows + sn_rp[J];
  real* X = Lx + sn_poff[J];
  for (int d = desc_ptr[J]; d < desc_ptr[J + 1]; ++d) {
    const int K = desc[3 * d], r0 = desc[3 * d + 1], r1 = desc[3 * d + 2];
    const int wk = sn_first[K + 1] - sn_first[K];
    const int nk = (int)(sn_rp[K + 1] - sn_rp[K]);
    const int* rk = sn_rows + sn_rp[K];
    const real* XK = Lx + sn_poff[K];
    const int na = nk - r0, nb = r1 - r0;
    for (long long t = tid; t < (long long)na * nb; t += BS) {
      const int b = (int)(t / na), a = (int)(t % na);
      if (a < b) continue;
      real s = R(0.0);
      for (int c = 0; c < wk; ++c) {
        const real* col = XK + (long long)c * nk;
        s += col[r0 + a] * (col[c] * col[r0 + b]);
      }
      const int ra = (a < nb) ? rk[r0 + a] - (int)f : ldl_rowpos(rows, w, nr, f, rk[r0 + a]);
      const int cb = rk[r0 + b] - (int)f;
      X[ra + (long long)cb * nr] -= s;
    }
    __syncthreads();
  }
  for (int c = 0; c < w; ++c) {
    const real* colc = X + (long long)c * nr;
    const real d = colc[c];
    const int nrr = nr - c - 1, ncc = w - c - 1;
    for (long long t = tid; t < (long long)nrr * ncc; t += BS) {
      const int c2 = c + 1 + (int)(t / nrr), r = c + 1 + (int)(t % nrr);
      if (r < c2) continue;
      X[r + (long long)c2 * nr] -= colc[r] * (colc[c2] / d);
    }
    __syncthreads();
    for (int r = c + 1 + tid; r < nr; r += BS) X[r + (long long)c * nr] = colc[r] / d;
    if (tid == 0) {
      if (!(d != R(0.0) && isfinite(d))) bad = true;
      if (d > R(0.0)) pos += 1;
    }
    __syncthreads();
  }
}

// forward solve L y = b for supernode J (L has a unit diagonal): the descendants' contributions, gathered, then the diagonal block
template <int BS>
__device__ __forceinline__ void ldl_fwd_sn(int J, const int* __restrict__ sn_first, const long long* __restrict__ sn_rp, const int* __restrict__ sn_rows,
                                           const long long* __restrict__ sn_poff, const int* __restrict__ desc_ptr, const int* __restrict__ desc,
                                           const real* __restrict__ Lx, real* __restrict__ y) {
  const int tid = threadIdx.x;
  const int f = sn_first[J];
  const int w = sn_first[J + 1] - f;
  const int nr = (int)(sn_rp[J + 1] - sn_rp[J]);
  const real* X = Lx + sn_poff[J];
  for (int d = desc_ptr[J]; d < desc_ptr[J + 1]; ++d) {
    const int K = desc[3 * d], r0 = desc[3 * d + 1], r1 = desc[3 * d + 2];
    const int fk = sn_first[K], wk = sn_first[K + 1] - fk;
    const int nk = (int)(sn_rp[K + 1] - sn_rp[K]);
    const int* rk = sn_rows + sn_rp[K];
    const real* XK = Lx + sn_poff[K];
    for (int b = r0 + tid; b < r1; b += BS) {
      real s = R(0.0);
      for (int c = 0; c < wk; ++c) s += XK[b + (long long)c * nk] * y[fk + c];
      y[rk[b]] -= s;
    }
    __syncthreads();
  }
  for (int c = 0; c + 1 < w; ++c) {
    const real yc = y[f + c];
    for (int r = c + 1 + tid; r < w; r += BS) y[f + r] -= X[r + (long long)c * nr] * yc;
    __syncthreads();
  }
}

// backward solve L' x = D^-1 y for supernode J (its ancestors already solved): one wave per column for the rows below the diagonal block (fixed
// reduction tree), then the diagonal block
template <int BS>
__device__ __forceinline__ void ldl_bwd_sn(int J, const int* __restrict__ sn_first, const long long* __restrict__ sn_rp, const int* __restrict__ sn_rows,
                                           const long long* __restrict__ sn_poff, const real* __restrict__ Lx, real* __restrict__ y) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = sn_first[J];
  const int w = sn_first[J + 1] - f;
  const int nr = (int)(sn_rp[J + 1] - sn_rp[J]);
  const int* rows = sn_rows + sn_rp[J];
  const real* X = Lx + sn_poff[J];
  for (int c = wave; c < w; c += BS / 64) {
    const real* col = X + (long long)c * nr;
    real s = R(0.0);
    for (int r = w + lane; r < nr; r += 64) s += col[r] * y[rows[r]];
    s = wave_sum(s);
    if (lane == 0) y[f + c] = y[f + c] / col[c] - s;
  }
  __syncthreads();
  for (int r = w - 1; r > 0; --r) {
    const real xr = y[f + r];
    for (int c = tid; c < r; c += BS) y[f + c] -= X[r + (long long)c * nr] * xr;
    __syncthreads();
  }
}
