// batch_polish.h -- polishing of the solved QP members of a batch on their active set (cosmo_hip_batch_polish; kernel: batch_polish.hip, entry points and
// storage: batch.hip).  What OSQP calls `polish`: guess the active rows from the ADMM solution, solve the equality-constrained KKT system once with a
// regularised LDL' factor and a few steps of iterative refinement, keep the result only if both residuals are no worse.
//
// Per member, on the SCALED problem the batch holds (x = head of w_prev, s, mu = rho .* (w_prev_s - s) = -y as recover_mu! forms it; scaled q, b, box bounds):
//   active set   Zero rows always (s^ = 0); a Nonnegatives row iff s_i < y_i (s^ = 0); a Box row at l_i iff s_i - l_i < y_i, at u_i iff u_i - s_i < -y_i,
//                the nearer side if both; a bound with |bound| >= COSMO_INFTY * MIN_SCALING is never active.
//   system       K t = r,  K = [P, (M A)'; M A, -(I - M)],  r = [-q; M (b - s^)],  M = diag(1 on the active rows): the union pattern of the ADMM KKT matrix
//                with explicit zeros, so the analysis and the refill maps of batch_ldl.h serve as they are.
//   factor       K~ = K + diag(delta 1_n, -delta on the active rows): quasi-definite for every guess, any ordering.  t = K~^-1 r, then refine_iter times
//                t += K~^-1 (r - K t) with K t from the member's own CSR arrays and the mask.
//   candidate    x = t[:n]; y on active rows = t[n + i] clipped to the sign its bound permits, 0 elsewhere; s = s^ on active rows, Pi(b - A x) elsewhere.
//   acceptance   the residuals of residuals.jl:30-96 as the batch kernels evaluate them for termination (unscaled with Einv, Dinv, cinv when the batch
//                unscales), of the current iterates and of the candidate: accepted iff everything is finite and neither residual grew.  Accepted: x into
//                the heads of w and w_prev, s, mu, w_s = mu ./ rho + s, and BCtl::{cost, r_prim, r_dual}.  Rejected: nothing is written.
// Never touched: rho, the ADMM factor slabs of a direct batch, the accelerator, iteration counters, statuses.
#pragma once
#include "batch_dev.h"
#include "batch_ldl.h"

#define BPOLISH_INFO 6                   // reals per member in BPolishDev::info: r_prim, r_dual before; r_prim, r_dual, cost of the candidate; active rows

struct BPolishDev {                      // (plain data, passed to the kernel by value)
  int nprob, n, m;
  BMat A, PT;
  const real *q, *b, *Dinv, *Einv, *cinv;
  const uint32_t* meta; const real *box_l, *box_u; int nbox;
  const real* rho;
  real *w, *w_prev, *s, *mu;
  BCtl* ctl;
  BLdlDev L;                             // the batch's analysis and refill maps; Lx and y are the polish's OWN slabs and work vectors
  const int* elig;                       // nprob: 1 = the last cosmo_hip_batch_optimize reported this member Solved
  unsigned char* mask;                   // nprob * m: 0 inactive, 1 active at the lower bound (or at 0), 2 active at the upper bound, 3 Zero row
  real *shat, *muc, *sc;                 // nprob * m: fixed slack of the active rows; -y and s of the candidate
  real *t, *res;                         // nprob * (n + m): the solution and the right-hand side / residual of the system, original order
  int* status;                           // nprob: 1 accepted, -1 rejected, 0 not attempted
  real* info;                            // nprob * BPOLISH_INFO
  real delta, big;
  int refine_iter, unscale;
};

// One persistent workgroup per `grid` slot, grid-strided over the members.  Returns the launch error.
hipError_t bpolish_launch(hipStream_t st, const BPolishDev& P, int grid);
