// batch_ruiz.hip -- scale_ruiz! (src/scaling.jl:21-116) for every member of a batch in one launch.
//
// One workgroup of BRUIZ_BS threads per member, grid = members.  The workgroup runs the whole sequence for its member without a host round trip: the
// `iterations` rounds (kkt_col_norms!, limit_scaling!, inv_sqrt!, scale_data!, the cost scaling), rectify_set_scalings!, scale_sets! (Box bounds) and
// the reciprocals.  It works on the three CSR copies batch.hip stages per member -- A, A', and the merged rows [P | A'] -- and on q, b and the bounds:
//   column norms of A   = row maxima of the A' copy,
//   column norms of P   = row maxima of the P part of the merged rows (P is symmetric: cosmo_hip_batch_scale_ruiz refuses anything else),
//   row norms of A      = row maxima of the A copy;
// no atomics.  A row of fewer than BRUIZ_LONG entries is walked by one thread, a longer one by a whole wave (lane l takes entries l, l + 64, ...);
// a maximum does not depend on the order.  Every stored entry is updated as val * (L[i] * R[j]) -- the factors multiplied first, as k_scale_csr
// (scaling.hip) and the host's _scale_csc do -- so the three copies of a value stay bit-identical; the cost scaling P *= ctmp, q *= ctmp is its own
// multiplication after the norms of the scaled P, as in the reference.  ||q||_inf keeps a NaN (scaling.hip).
//
// Sums.  Two quantities depend on an order of additions: mean(column norms of P) per round and mean(E) per scalar-scaled cone.  Both are taken by
// ordered_sum below: thread t (of BRUIZ_BS = 256) adds the terms t, t + 256, t + 512, ... in ascending order into p_t, then the p_t are added by the
// halving tree p_t += p_{t + s}, s = 128, 64, ..., 1.  A cone of at most 64 rows is summed by one wave with the same tree from s = 32 down (its p_t
// are zero for t >= 64 and x + 0 = x for the non-negative terms here, so the bits are those of the workgroup-wide form).  The order depends on the
// number of terms only -- not on the number of members, the slot of a member, or the work-vector route.
//
// Work vectors.  D, E, Dwork, Ework (2 (n + m) reals) live in the launch's dynamic LDS behind the BRUIZ_BS reals of the reduction tree when
// (BRUIZ_BS + 2 (n + m)) * sizeof(real) <= BRUIZ_LDS_MAX (64 KiB, what a launch gets without raising the kernel's limit; six workgroups per CU at
// config 3's n + m = 1500); otherwise they live in a per-member slab of global memory and the LDS holds the tree alone.  bruiz_run decides and
// reports it (cosmo_hip_batch_ruiz_info).
#include "batch_ruiz.h"
#include "device_utils.h"
#include <math.h>
#include <string.h>
#include <algorithm>

#define BRUIZ_BS 256
#define BRUIZ_LONG 64
#define BRUIZ_LDS_MAX 65536

namespace {

struct BRuizDev {
  int n, m, nbox, ncones, rounds;
  real lo, hi;
  // concatenated over members; row pointers and the split are member-local positions, nz = {A, A', [P | A']} value offsets per member
  const int *A_rp, *A_col, *AT_rp, *AT_col, *PT_rp, *PT_col, *PT_split;
  const long long* nz;          // 3 per member
  const int* flags;             // per member: bit 0 / 1 / 2 = a row of >= BRUIZ_LONG entries in A / A' / [P | A'], bit 3 = skip
  const int* cone;              // 4 per cone: {scalar-scaled, offset, dimension, first Box bound or -1}
  int any_scalar;               // some cone is scalar-scaled (rectify_set_scalings! changes E)
  real *A_val, *AT_val, *PT_val, *q, *b, *box_l, *box_u;
  real *D, *E, *Dinv, *Einv, *c, *cinv;     // results, member-major
  real* slab;                   // global work vectors (2 (n + m) per member) or null: LDS
};

__device__ __forceinline__ real absmax2(real a, real t) { return a > t ? a : t; }

// out[r] = max(merge ? out[r] : 0, max |val| over entries [lo(r), hi(r)))
template <class Lo, class Hi>
__device__ __forceinline__ void rows_absmax(int nrows, bool any_long, Lo lo, Hi hi, const real* __restrict__ val, real* out, bool merge) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int r = tid; r < nrows; r += BRUIZ_BS) {
    const int a = lo(r), e = hi(r);
    if (e - a >= BRUIZ_LONG) continue;
    real mx = merge ? out[r] : R(0.0);
    for (int k = a; k < e; ++k) mx = absmax2(mx, fabs(val[k]));
    out[r] = mx;
  }
  if (!any_long) return;
  for (int r = wave; r < nrows; r += BRUIZ_BS / 64) {          // (wave-uniform: all 64 lanes take the shuffles)
    const int a = lo(r), e = hi(r);
    if (e - a < BRUIZ_LONG) continue;
    real mx = R(0.0);
    for (int k = a + lane; k < e; k += 64) mx = absmax2(mx, fabs(val[k]));
    for (int s = 32; s > 0; s >>= 1) mx = absmax2(mx, __shfl_xor(mx, s));
    if (lane == 0) out[r] = merge ? absmax2(out[r], mx) : mx;
  }
}

// f(r, k) for every entry k of every row r, rows split between threads and waves as above
template <class Lo, class Hi, class F>
__device__ __forceinline__ void rows_each(int nrows, bool any_long, Lo lo, Hi hi, F f) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int r = tid; r < nrows; r += BRUIZ_BS) {
    const int a = lo(r), e = hi(r);
    if (e - a >= BRUIZ_LONG) continue;
    for (int k = a; k < e; ++k) f(r, k);
  }
  if (!any_long) return;
  for (int r = wave; r < nrows; r += BRUIZ_BS / 64) {
    const int a = lo(r), e = hi(r);
    if (e - a < BRUIZ_LONG) continue;
    for (int k = a + lane; k < e; k += 64) f(r, k);
  }
}

// the fixed order of the file header: strided partials, then the halving tree (red: BRUIZ_BS reals of LDS); the result in every thread
__device__ __forceinline__ real ordered_sum(const real* v, int count, real* red) {
  const int tid = threadIdx.x;
  real p = R(0.0);
  for (int i = tid; i < count; i += BRUIZ_BS) p += v[i];
  __syncthreads();
  red[tid] = p;
  __syncthreads();
  for (int s = BRUIZ_BS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}
// ||v||_inf, a NaN kept (the rule of block_max, device_utils.h)
__device__ __forceinline__ real ordered_absmax_nan(const real* v, int count, real* red) {
  const int tid = threadIdx.x;
  real p = R(0.0);
  for (int i = tid; i < count; i += BRUIZ_BS) { const real a = fabs(v[i]); if (a > p || a != a) p = a; }
  __syncthreads();
  red[tid] = p;
  __syncthreads();
  for (int s = BRUIZ_BS / 2; s > 0; s >>= 1) {
    if (tid < s) { const real a = red[tid], t = red[tid + s]; red[tid] = (t > a || t != t) ? t : a; }
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ real limit_scaling(real s, real lo, real hi) { return s < lo ? R(1.0) : (s > hi ? hi : s); }     // src/algebra.jl:5-7

__global__ __launch_bounds__(BRUIZ_BS) void k_batch_ruiz(BRuizDev S) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bruiz_lds[];
  const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fl = S.flags[k];
  if (fl & 8) return;                                              // the caller's own scaling stays (block-uniform)
  const int n = S.n, m = S.m;
  real* red = reinterpret_cast<real*>(bruiz_lds);
  real* wv = S.slab ? S.slab + (long long)k * 2 * (n + m) : red + BRUIZ_BS;
  real *D = wv, *E = D + n, *Dw = E + m, *Ew = Dw + n;
  const int* Arp = S.A_rp + (long long)k * (m + 1);
  const int* Trp = S.AT_rp + (long long)k * (n + 1);
  const int* Prp = S.PT_rp + (long long)k * (n + 1);
  const int* Psp = S.PT_split + (long long)k * n;
  const long long oA = S.nz[3 * k], oT = S.nz[3 * k + 1], oP = S.nz[3 * k + 2];
  const int *Acol = S.A_col + oA, *Tcol = S.AT_col + oT, *Pcol = S.PT_col + oP;
  real *Av = S.A_val + oA, *Tv = S.AT_val + oT, *Pv = S.PT_val + oP;
  real *q = S.q + (long long)k * n, *b = S.b + (long long)k * m;
  const bool longA = fl & 1, longT = fl & 2, longP = fl & 4;
  auto A_lo = [&](int r) { return Arp[r]; };  auto A_hi = [&](int r) { return Arp[r + 1]; };
  auto T_lo = [&](int r) { return Trp[r]; };  auto T_hi = [&](int r) { return Trp[r + 1]; };
  auto P_lo = [&](int r) { return Prp[r]; };  auto P_hi = [&](int r) { return Prp[r + 1]; };  auto P_sp = [&](int r) { return Psp[r]; };
  const real lo = S.lo, hi = S.hi;

  for (int i = tid; i < n; i += BRUIZ_BS) D[i] = R(1.0);
  for (int i = tid; i < m; i += BRUIZ_BS) E[i] = R(1.0);
  real c = R(1.0);
  __syncthreads();
  for (int it = 0; it < S.rounds; ++it) {
    // kkt_col_norms! (scaling.jl:3-8): Dw = max(col norms P, col norms A), Ew = row norms A
    rows_absmax(n, longP, P_lo, P_sp, Pv, Dw, false);
    rows_absmax(m, longA, A_lo, A_hi, Av, Ew, false);
    __syncthreads();
    rows_absmax(n, longT, T_lo, T_hi, Tv, Dw, true);
    __syncthreads();
    for (int i = tid; i < n; i += BRUIZ_BS) Dw[i] = R(1.0) / sqrt(limit_scaling(Dw[i], lo, hi));      // limit_scaling!, inv_sqrt!
    for (int i = tid; i < m; i += BRUIZ_BS) Ew[i] = R(1.0) / sqrt(limit_scaling(Ew[i], lo, hi));
    __syncthreads();
    // scale_data!(P, A, q, b, Dw, Ew, 1): the entry (i, j) of the original matrix *= L[i] * R[j] in each of its copies
    rows_each(m, longA, A_lo, A_hi, [&](int r, int e) { Av[e] = Av[e] * (Ew[r] * Dw[Acol[e]]); });
    rows_each(n, longT, T_lo, T_hi, [&](int r, int e) { Tv[e] = Tv[e] * (Ew[Tcol[e]] * Dw[r]); });
    rows_each(n, longP, P_lo, P_hi, [&](int r, int e) {
      const int cc = Pcol[e];
      Pv[e] = cc < n ? Pv[e] * (Dw[cc] * Dw[r]) : Pv[e] * (Ew[cc - n] * Dw[r]);
    });
    for (int i = tid; i < n; i += BRUIZ_BS) { q[i] = q[i] * Dw[i]; D[i] = D[i] * Dw[i]; }
    for (int i = tid; i < m; i += BRUIZ_BS) { b[i] = b[i] * Ew[i]; E[i] = E[i] * Ew[i]; }
    __syncthreads();
    // cost scaling (scaling.jl:65-83): mean column norm of the scaled P and ||q||_inf
    rows_absmax(n, longP, P_lo, P_sp, Pv, Dw, false);
    __syncthreads();
    const real sum_col = ordered_sum(Dw, n, red);
    const real mean_col = n ? sum_col / (real)n : R(0.0);
    real nq = ordered_absmax_nan(q, n, red);
    if (mean_col != R(0.0) && nq != R(0.0)) {                      // (block-uniform)
      nq = limit_scaling(nq, lo, hi);
      const real sc = limit_scaling(nq < mean_col ? mean_col : nq, lo, hi);
      const real ctmp = R(1.0) / sc;
      rows_each(n, longP, P_lo, P_sp, [&](int, int e) { Pv[e] = Pv[e] * ctmp; });     // scalarmul!(P, ctmp)
      for (int i = tid; i < n; i += BRUIZ_BS) q[i] = q[i] * ctmp;
      c = c * ctmp;
    }
    __syncthreads();
  }
  // rectify_set_scalings! (scaling.jl:129-142): one scalar per second-order / PSD / exponential / power cone (convexset.jl:953-982)
  if (S.any_scalar) {
    for (int i = tid; i < m; i += BRUIZ_BS) Ew[i] = R(1.0);
    __syncthreads();
    for (int cn = wave; cn < S.ncones; cn += BRUIZ_BS / 64) {      // cones of at most 64 rows: one wave each
      const int sc = S.cone[4 * cn], o = S.cone[4 * cn + 1], d = S.cone[4 * cn + 2];
      if (!sc || d <= 0 || d > 64) continue;                      // (wave-uniform)
      const real e = lane < d ? E[o + lane] : R(0.0);
      real v = e;
      for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s);
      const real tmp = __shfl(v, 0) / (real)d;                    // rectify_scalar_scaling!: mean(E) ./ E
      if (lane < d) Ew[o + lane] = tmp / e;
    }
    for (int cn = 0; cn < S.ncones; ++cn) {                         // larger cones: the workgroup
      const int sc = S.cone[4 * cn], o = S.cone[4 * cn + 1], d = S.cone[4 * cn + 2];
      if (!sc || d <= 64) continue;                               // (block-uniform)
      const real tmp = ordered_sum(E + o, d, red) / (real)d;
      for (int i = tid; i < d; i += BRUIZ_BS) Ew[o + i] = tmp / E[o + i];
      __syncthreads();
    }
    __syncthreads();
    // scale_data!(P, A, q, b, I, Ework, 1)
    rows_each(m, longA, A_lo, A_hi, [&](int r, int e) { Av[e] = Av[e] * Ew[r]; });
    rows_each(n, longT, T_lo, T_hi, [&](int, int e) { Tv[e] = Tv[e] * Ew[Tcol[e]]; });
    rows_each(n, longP, P_sp, P_hi, [&](int, int e) { Pv[e] = Pv[e] * Ew[Pcol[e] - n]; });
    for (int i = tid; i < m; i += BRUIZ_BS) { b[i] = b[i] * Ew[i]; E[i] = E[i] * Ew[i]; }
    __syncthreads();
  }
  // scale_sets! (scaling.jl:145-154): Box bounds
  if (S.nbox > 0) {
    real* bl = S.box_l + (long long)k * S.nbox;
    real* bu = S.box_u + (long long)k * S.nbox;
    for (int cn = 0; cn < S.ncones; ++cn) {
      const int o = S.cone[4 * cn + 1], d = S.cone[4 * cn + 2], bo = S.cone[4 * cn + 3];
      if (bo < 0) continue;
      for (int i = tid; i < d; i += BRUIZ_BS) { bl[bo + i] = bl[bo + i] * E[o + i]; bu[bo + i] = bu[bo + i] * E[o + i]; }
    }
  }
  // D, E, their reciprocals, c and cinv (scaling.jl:103-110)
  real *Do = S.D + (long long)k * n, *Eo = S.E + (long long)k * m, *Di = S.Dinv + (long long)k * n, *Ei = S.Einv + (long long)k * m;
  for (int i = tid; i < n; i += BRUIZ_BS) { const real d = D[i]; Do[i] = d; Di[i] = R(1.0) / d; }
  for (int i = tid; i < m; i += BRUIZ_BS) { const real e = E[i]; Eo[i] = e; Ei[i] = R(1.0) / e; }
  if (tid == 0) { S.c[k] = c; S.cinv[k] = R(1.0) / c; }
}

template <class T>
void append(std::vector<T>& dst, const std::vector<T>& src) { dst.insert(dst.end(), src.begin(), src.end()); }

bool has_long_row(const std::vector<int>& rp) {
  for (size_t r = 0; r + 1 < rp.size(); ++r) if (rp[r + 1] - rp[r] >= BRUIZ_LONG) return true;
  return false;
}

struct DevBuf {                 // freed when bruiz_run returns, whatever the path
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

}  // namespace

#define RHIP(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) { err = std::string(#call) + " failed: " + hipGetErrorString(e__); return COSMO_HIP_ERR_HIP; } } while (0)

int32_t bruiz_run(BRuizStage& S, hipStream_t st, long long iterations, real min_scaling, real max_scaling, int64_t info[4], std::string& err) {
  const int nprob = S.nprob;
  const long long n = S.n, m = S.m;
  const size_t Nn = (size_t)nprob * n, Nm = (size_t)nprob * m, Nb = (size_t)nprob * S.nbox;
  // ---- integers: row pointers, columns, the split, value offsets, flags, the cone table -- one upload
  std::vector<int> ints;
  std::vector<long long> nz((size_t)3 * nprob);
  std::vector<int> flags((size_t)nprob, 0);
  size_t totA = 0, totT = 0, totP = 0;
  for (int k = 0; k < nprob; ++k) {
    nz[(size_t)3 * k] = (long long)totA; nz[(size_t)3 * k + 1] = (long long)totT; nz[(size_t)3 * k + 2] = (long long)totP;
    totA += (*S.A)[k].val.size(); totT += (*S.AT)[k].val.size(); totP += (*S.PT)[k].val.size();
    flags[k] = (has_long_row((*S.A)[k].rowptr) ? 1 : 0) | (has_long_row((*S.AT)[k].rowptr) ? 2 : 0) | (has_long_row((*S.PT)[k].rowptr) ? 4 : 0) |
               ((*S.skip)[k] ? 8 : 0);
  }
  ints.reserve((size_t)nprob * (m + 1 + 3 * n + 2) + totA + totT + totP + 4 * S.cones->type.size());
  const size_t oArp = ints.size(); for (int k = 0; k < nprob; ++k) append(ints, (*S.A)[k].rowptr);
  const size_t oTrp = ints.size(); for (int k = 0; k < nprob; ++k) append(ints, (*S.AT)[k].rowptr);
  const size_t oPrp = ints.size(); for (int k = 0; k < nprob; ++k) append(ints, (*S.PT)[k].rowptr);
  const size_t oPsp = ints.size(); for (int k = 0; k < nprob; ++k) append(ints, (*S.PT)[k].split);
  const size_t oAc = ints.size(); for (int k = 0; k < nprob; ++k) append(ints, (*S.A)[k].col);
  const size_t oTc = ints.size(); for (int k = 0; k < nprob; ++k) append(ints, (*S.AT)[k].col);
  const size_t oPc = ints.size(); for (int k = 0; k < nprob; ++k) append(ints, (*S.PT)[k].col);
  const size_t oFl = ints.size(); append(ints, flags);
  const size_t oCn = ints.size();
  const ConeTable& C = *S.cones;
  int any_scalar = 0;
  { long long boxp = 0;
    for (size_t cn = 0; cn < C.type.size(); ++cn) {
      const int scalar = (C.type[cn] >= COSMO_HIP_SOC && C.dim[cn] > 0) ? 1 : 0;      // (as cosmo_hip_scale_ruiz)
      any_scalar |= scalar;
      ints.push_back(scalar); ints.push_back((int)C.off[cn]); ints.push_back((int)C.dim[cn]);
      ints.push_back(C.type[cn] == COSMO_HIP_BOX ? (int)boxp : -1);
      if (C.type[cn] == COSMO_HIP_BOX) boxp += C.dim[cn];
    } }
  // ---- reals: [values of A | A' | [P | A'] | q | b | Box bounds] up, the same plus [D | E | Dinv | Einv | c | cinv] down -- one copy each way
  const size_t rA = 0, rT = rA + totA, rP = rT + totT, rq = rP + totP, rb = rq + Nn, rbl = rb + Nm, rbu = rbl + Nb, r_in = rbu + Nb;
  const size_t rD = r_in, rE = rD + Nn, rDi = rE + Nm, rEi = rDi + Nn, rc = rEi + Nm, rci = rc + (size_t)nprob, r_all = rci + (size_t)nprob;
  std::vector<real> reals(r_all, R(1.0));
  for (int k = 0; k < nprob; ++k) {
    std::copy((*S.A)[k].val.begin(), (*S.A)[k].val.end(), reals.begin() + rA + (size_t)nz[(size_t)3 * k]);
    std::copy((*S.AT)[k].val.begin(), (*S.AT)[k].val.end(), reals.begin() + rT + (size_t)nz[(size_t)3 * k + 1]);
    std::copy((*S.PT)[k].val.begin(), (*S.PT)[k].val.end(), reals.begin() + rP + (size_t)nz[(size_t)3 * k + 2]);
  }
  std::copy(S.q->begin(), S.q->begin() + Nn, reals.begin() + rq);
  std::copy(S.b->begin(), S.b->begin() + Nm, reals.begin() + rb);
  if (Nb) { std::copy(S.box_l->begin(), S.box_l->begin() + Nb, reals.begin() + rbl); std::copy(S.box_u->begin(), S.box_u->begin() + Nb, reals.begin() + rbu); }
  // ---- work vectors: LDS where they fit the launch's dynamic request, else a global slab per member
  const size_t lds_tree = (size_t)BRUIZ_BS * sizeof(real), lds_full = lds_tree + (size_t)2 * (n + m) * sizeof(real);
  const bool in_lds = lds_full <= BRUIZ_LDS_MAX;
  const size_t lds = in_lds ? lds_full : lds_tree;
  DevBuf dI, dZ, dR, dS;
  RHIP(hipMalloc(&dI.p, std::max<size_t>(1, ints.size()) * sizeof(int)));
  RHIP(hipMalloc(&dZ.p, nz.size() * sizeof(long long)));
  RHIP(hipMalloc(&dR.p, r_all * sizeof(real)));
  if (!in_lds) RHIP(hipMalloc(&dS.p, (size_t)nprob * 2 * (n + m) * sizeof(real)));
  RHIP(hipMemcpyAsync(dI.p, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice, st));
  RHIP(hipMemcpyAsync(dZ.p, nz.data(), nz.size() * sizeof(long long), hipMemcpyHostToDevice, st));
  RHIP(hipMemcpyAsync(dR.p, reals.data(), r_in * sizeof(real), hipMemcpyHostToDevice, st));
  BRuizDev V;
  memset(&V, 0, sizeof V);
  V.n = (int)n; V.m = (int)m; V.nbox = S.nbox; V.ncones = (int)C.type.size(); V.rounds = (int)iterations;
  V.lo = min_scaling; V.hi = max_scaling;
  const int* di = static_cast<const int*>(dI.p);
  V.A_rp = di + oArp; V.AT_rp = di + oTrp; V.PT_rp = di + oPrp; V.PT_split = di + oPsp; V.A_col = di + oAc; V.AT_col = di + oTc; V.PT_col = di + oPc;
  V.flags = di + oFl; V.cone = di + oCn; V.any_scalar = any_scalar;
  V.nz = static_cast<const long long*>(dZ.p);
  real* dr = static_cast<real*>(dR.p);
  V.A_val = dr + rA; V.AT_val = dr + rT; V.PT_val = dr + rP; V.q = dr + rq; V.b = dr + rb; V.box_l = dr + rbl; V.box_u = dr + rbu;
  V.D = dr + rD; V.E = dr + rE; V.Dinv = dr + rDi; V.Einv = dr + rEi; V.c = dr + rc; V.cinv = dr + rci;
  V.slab = static_cast<real*>(dS.p);
  hipLaunchKernelGGL(k_batch_ruiz, dim3(nprob), dim3(BRUIZ_BS), lds, st, V);
  RHIP(hipGetLastError());
  // (skipped members keep what the upload put there: their values, and ones in the result sections, which are not copied out for them)
  RHIP(hipMemcpyAsync(reals.data(), dR.p, r_all * sizeof(real), hipMemcpyDeviceToHost, st));
  RHIP(hipStreamSynchronize(st));
  int scaled = 0;
  for (int k = 0; k < nprob; ++k) {
    if ((*S.skip)[k]) continue;
    ++scaled;
    HostCsr &A = (*S.A)[k], &AT = (*S.AT)[k], &PT = (*S.PT)[k];
    std::copy(reals.begin() + rA + (size_t)nz[(size_t)3 * k], reals.begin() + rA + (size_t)nz[(size_t)3 * k] + A.val.size(), A.val.begin());
    std::copy(reals.begin() + rT + (size_t)nz[(size_t)3 * k + 1], reals.begin() + rT + (size_t)nz[(size_t)3 * k + 1] + AT.val.size(), AT.val.begin());
    std::copy(reals.begin() + rP + (size_t)nz[(size_t)3 * k + 2], reals.begin() + rP + (size_t)nz[(size_t)3 * k + 2] + PT.val.size(), PT.val.begin());
    const size_t kn = (size_t)k * n, km = (size_t)k * m, kb = (size_t)k * S.nbox;
    std::copy(reals.begin() + rq + kn, reals.begin() + rq + kn + n, S.q->begin() + kn);
    std::copy(reals.begin() + rb + km, reals.begin() + rb + km + m, S.b->begin() + km);
    if (S.nbox) {
      std::copy(reals.begin() + rbl + kb, reals.begin() + rbl + kb + S.nbox, S.box_l->begin() + kb);
      std::copy(reals.begin() + rbu + kb, reals.begin() + rbu + kb + S.nbox, S.box_u->begin() + kb);
    }
    std::copy(reals.begin() + rD + kn, reals.begin() + rD + kn + n, S.D->begin() + kn);
    std::copy(reals.begin() + rDi + kn, reals.begin() + rDi + kn + n, S.Dinv->begin() + kn);
    std::copy(reals.begin() + rE + km, reals.begin() + rE + km + m, S.E->begin() + km);
    std::copy(reals.begin() + rEi + km, reals.begin() + rEi + km + m, S.Einv->begin() + km);
    (*S.c)[k] = reals[rc + k]; (*S.cinv)[k] = reals[rci + k];
  }
  info[0] = in_lds ? 0 : 1; info[1] = (int64_t)lds; info[2] = scaled; info[3] = iterations;
  return COSMO_HIP_OK;
}
