// batch_polish.hip -- k_batch_polish: the active-set polish of batch_polish.h, one workgroup of COSMO_BS threads per member, grid-strided over the members
// (a persistent grid of at most one workgroup per CU; a member never leaves its workgroup, so every synchronisation is a workgroup barrier).  Streaming
// form: the member's CSR arrays, slab and vectors stay in global memory (L2), any size the direct batch takes.
//
// Work per member: one refill + factorisation of its polish slab (ldl_factor_sn over the supernodes), 1 + refine_iter forward / backward sweeps,
// 2 * refine_iter sparse passes for r - K t, and 5 sparse passes around them (2 for the residuals of the iterates, 1 for the candidate's slack, 2 for its
// residuals; the passes of StreamOps, one row per thread, products added left to right).  No float atomics; every sum is a fixed-order single-workgroup
// sum (bsum) and every norm a maximum (bmax): two polishes of the same state give the same bits, whichever workgroup takes a member.
#include "batch_polish.h"

// t = K~^-1 rhs, or t += K~^-1 rhs (accumulate): rhs and t in the original order [x (n); rows (m)], X the member's factor slab, y its permuted work vector.
// The right-hand side is an argument: the same factor serves any other solve with K~ (an adjoint, for one).
template <int BS>
__device__ __forceinline__ void bpolish_solve(const BLdlDev& L, const real* __restrict__ X, real* __restrict__ y, const real* __restrict__ rhs,
                                              real* __restrict__ t, const bool accumulate) {
  const int tid = threadIdx.x, N = L.N;
  for (int i = tid; i < N; i += BS) y[i] = rhs[L.perm[i]];
  __syncthreads();
  for (int J = 0; J < L.ns; ++J) ldl_fwd_sn<BS>(J, L.sn_first, L.sn_rp, L.sn_rows, L.sn_poff, L.desc_ptr, L.desc, X, y);
  __syncthreads();
  for (int J = L.ns - 1; J >= 0; --J) ldl_bwd_sn<BS>(J, L.sn_first, L.sn_rp, L.sn_rows, L.sn_poff, X, y);
  __syncthreads();
  for (int i = tid; i < N; i += BS) { const int p = L.perm[i]; t[p] = accumulate ? t[p] + y[i] : y[i]; }
  __syncthreads();
}

__global__ __launch_bounds__(COSMO_BS) void k_batch_polish(BPolishDev P) {
  constexpr int BS = COSMO_BS;
  __shared__ real lds[COSMO_NNZ_PER_BLOCK];
  __shared__ real red[BS / 64];
  __shared__ int bad_s;
  const int tid = threadIdx.x;
  const int n = P.n, m = P.m;
  const BLdlDev& L = P.L;
  const bool unscale = P.unscale != 0;
  for (int k = blockIdx.x; k < P.nprob; k += gridDim.x) {
    BCtl* ctl = P.ctl + k;
    real* info = P.info + (long long)k * BPOLISH_INFO;
    if (!P.elig[k]) {                                                       // not Solved: left untouched (block-uniform)
      if (tid == 0) { P.status[k] = 0; info[0] = ctl->r_prim; info[1] = ctl->r_dual; info[2] = R(0.0); info[3] = R(0.0); info[4] = R(0.0); info[5] = R(0.0); }
      continue;
    }
    const long long on = (long long)k * n, om = (long long)k * m, onm = (long long)k * (n + m);
    const real *q = P.q + on, *b = P.b + om, *Dinv = P.Dinv + on, *Einv = P.Einv + om, *rho = P.rho + om;
    const real cinv = P.cinv[k];
    const real *bl = P.box_l + (long long)k * P.nbox, *bu = P.box_u + (long long)k * P.nbox;
    real *w = P.w + onm, *w_prev = P.w_prev + onm, *s = P.s + om, *mu = P.mu + om;
    unsigned char* mask = P.mask + om;
    real *shat = P.shat + om, *muc = P.muc + om, *sc = P.sc + om, *t = P.t + onm, *res = P.res + onm;
    real* X = L.Lx + (long long)k * L.panel;
    real* yw = L.y + (long long)k * L.N;
    StreamOps ops;
    ops.A = bview(P.A, k); ops.AT = ops.A; ops.PT = bview(P.PT, k); ops.lds = lds; ops.red = red; ops.psd_ws = nullptr;

    // r_prim, r_dual and the cost of (x, sv, -muv) as the batch kernels evaluate them for termination (batch.hip: residuals)
    auto residuals = [&](const real* xp, const real* sv_, const real* muv_, real& rp, real& rd, real& cost) {
      real a_rp = 0.0;
      ops.rows_A(xp, [&](int row, real s1, real s2) {
        const real ax = s1 + s2;
        real rv = ax + sv_[row]; rv = rv - b[row];
        if (unscale) rv = rv * Einv[row];
        a_rp = amax(a_rp, rv); });
      rp = bmax<BS>(a_rp, red);
      __syncthreads();
      real a_rd = 0.0, xpx = 0.0, qx = 0.0;
      ops.rows_PT(xp, muv_, [&](int row, real px, real atm) {
        const real xv = xp[row], qv = q[row];
        real rv = px + qv; rv = rv - atm;
        if (unscale) rv = (rv * Dinv[row]) * cinv;
        a_rd = amax(a_rd, rv);
        xpx += px * xv; qx += qv * xv; });
      rd = bmax<BS>(a_rd, red);
      xpx = bsum<BS>(xpx, red); qx = bsum<BS>(qx, red);
      cost = (unscale ? cinv : R(1.0)) * (R(0.5) * xpx + qx);
      __syncthreads();
    };

    // ---- the residuals of the iterates the member holds: what the candidate has to match.  mu as recover_mu! forms it (solver.jl:167): behind the loop
    // these are the bits of the stored mu, and behind cosmo_hip_batch_set_iterates (which writes w and s only) they are the mu that was set ----
    for (int i = tid; i < m; i += BS) muc[i] = rho[i] * (w_prev[n + i] - s[i]);
    __syncthreads();
    real rp0, rd0, cost0;
    residuals(w_prev, s, muc, rp0, rd0, cost0);

    // ---- 1. the active rows (mask) and their fixed slack ----
    real cnt = 0.0;
    for (int i = tid; i < m; i += BS) {
      const uint32_t me = P.meta[i], kind = me & 3u;
      const real sv = s[i], yv = -muc[i];
      unsigned char a = 0; real sh = 0.0;
      if (kind == 1u) a = 3;
      else if (kind == 2u) { if (sv < yv) a = 1; }
      else if (kind == 3u) {
        const real l = bl[me >> 2], u = bu[me >> 2];
        const real dl = sv - l, du = u - sv;
        bool low = fabs(l) < P.big && dl < yv, upp = fabs(u) < P.big && du < -yv;
        if (low && upp) { if (dl <= du) upp = false; else low = false; }
        if (low) { a = 1; sh = l; } else if (upp) { a = 2; sh = u; }
      }
      mask[i] = a; shat[i] = sh;
      if (a) cnt += R(1.0);
    }
    const real nact = bsum<BS>(cnt, red);                                   // (small integers: exact; its barriers also publish mask and shat)

    // ---- 2. the polish slab: K~ = K + diag(delta, -delta on the active rows), rows of A outside the active set as explicit zeros ----
    {
      const long long po = P.PT.nz_off[k], ao = P.A.nz_off[k];
      const real* ptv = P.PT.val + po; const real* av = P.A.val + ao;
      const int pnnz = P.PT.rowptr[(long long)k * (n + 1) + n];
      const int* arp = P.A.rowptr + (long long)k * (m + 1);
      const int* pd = L.pdiag + (long long)k * n;
      const int* ps = L.pslot + po;
      const int* as = L.aslot + ao;
      for (long long i = tid; i < L.panel; i += BS) X[i] = R(0.0);
      __syncthreads();
      // every target slot is written by exactly one item: [x diagonal | upper off-diagonal P | active rows of A | row diagonal] (bldl_refill_factor)
      for (int i = tid; i < n; i += BS) { const int d = pd[i]; X[L.dslot[i]] = (d >= 0) ? ptv[d] + P.delta : P.delta; }
      for (int e = tid; e < pnnz; e += BS) { const int sl = ps[e]; if (sl >= 0) X[sl] = ptv[e]; }
      for (int i = tid; i < m; i += BS) {
        const bool act = mask[i] != 0;
        if (act) for (int e = arp[i]; e < arp[i + 1]; ++e) X[as[e]] = av[e];
        X[L.rslot[i]] = act ? -P.delta : R(-1.0);
      }
      __syncthreads();
    }

    // ---- 3. factorise ----
    {
      int pos = 0; bool bad = false;
      for (int J = 0; J < L.ns; ++J) ldl_factor_sn<BS>(J, L.sn_first, L.sn_rp, L.sn_rows, L.sn_poff, L.desc_ptr, L.desc, X, pos, bad);
      if (tid == 0) bad_s = bad ? 1 : 0;
      __syncthreads();
    }
    if (bad_s) {                                                            // a zero or non-finite pivot: rejected, nothing else (block-uniform)
      if (tid == 0) { P.status[k] = -1; info[0] = rp0; info[1] = rd0; info[2] = INFINITY; info[3] = INFINITY; info[4] = INFINITY; info[5] = nact; }
      __syncthreads();
      continue;
    }

    // ---- 4. + 5. r = [-q; M (b - s^)], t = K~^-1 r ----
    for (int i = tid; i < n + m; i += BS) {
      if (i < n) res[i] = -q[i];
      else { const int r = i - n; res[i] = mask[r] ? b[r] - shat[r] : R(0.0); }
    }
    __syncthreads();
    bpolish_solve<BS>(L, X, yw, res, t, false);

    // ---- 6. iterative refinement: t += K~^-1 (r - K t), K t from the member's CSR arrays and the mask ----
    for (int it = 0; it < P.refine_iter; ++it) {
      for (int i = tid; i < m; i += BS) muc[i] = mask[i] ? t[n + i] : R(0.0);      // M t_y: what the columns of (M A)' multiply
      __syncthreads();
      ops.rows_A(t, [&](int row, real s1, real s2) {
        res[n + row] = mask[row] ? (b[row] - shat[row]) - (s1 + s2) : t[n + row]; });    // (an inactive row of K is -1 on the diagonal and its r is 0)
      ops.rows_PT(t, muc, [&](int row, real px, real atm) { res[row] = (-q[row] - px) - atm; });
      __syncthreads();
      bpolish_solve<BS>(L, X, yw, res, t, true);
    }

    // ---- 7. the candidate: y clipped to the sign its bound permits, s = s^ on the active rows and Pi(b - A x) elsewhere ----
    real nf = 0.0;
    for (int i = tid; i < n + m; i += BS) if (!isfinite(t[i])) nf += R(1.0);
    ops.rows_A(t, [&](int row, real s1, real s2) {
      const unsigned char a = mask[row];
      real yv = a ? t[n + row] : R(0.0);
      if (a == 1) yv = (yv > R(0.0)) ? yv : R(0.0);
      else if (a == 2) yv = (yv < R(0.0)) ? yv : R(0.0);
      muc[row] = -yv;
      sc[row] = a ? shat[row] : proj_simple(b[row] - (s1 + s2), P.meta[row], bl, bu); });
    nf = bsum<BS>(nf, red);
    __syncthreads();

    // ---- 8. its residuals and cost ----
    real rp1, rd1, cost1;
    residuals(t, sc, muc, rp1, rd1, cost1);

    // ---- 9. keep it only if nothing got worse ----
    const bool ok = nf == R(0.0) && isfinite(rp1) && isfinite(rd1) && isfinite(cost1) && rp1 <= rp0 && rd1 <= rd0;
    if (ok) {
      for (int i = tid; i < n + m; i += BS) {
        if (i < n) { const real v = t[i]; w[i] = v; w_prev[i] = v; }
        else {
          const int r = i - n;
          const real sv = sc[r], mv = muc[r];
          const real wv = (R(1.0) / rho[r]) * mv + sv;                     // w_s = mu ./ rho + s (solver.jl:128-129): recover_mu! gives mu back
          s[r] = sv; mu[r] = mv; w[i] = wv; w_prev[i] = wv;
        }
      }
      if (tid == 0) { ctl->cost = cost1; ctl->r_prim = rp1; ctl->r_dual = rd1; }
    }
    if (tid == 0) { P.status[k] = ok ? 1 : -1; info[0] = rp0; info[1] = rd0; info[2] = rp1; info[3] = rd1; info[4] = cost1; info[5] = nact; }
    __syncthreads();                                                        // the next member reuses lds, red and bad_s
  }
}

hipError_t bpolish_launch(hipStream_t st, const BPolishDev& P, int grid) {
  if (P.nprob <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_batch_polish, dim3(grid < 1 ? 1 : (grid > P.nprob ? P.nprob : grid)), dim3(COSMO_BS), 0, st, P);
  return hipGetLastError();
}
