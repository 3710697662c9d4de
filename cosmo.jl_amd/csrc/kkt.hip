// kkt.hip -- the route of a handle's KKT solves: which solver, which Krylov recurrence and which form of the reduced operator.  kkt_configure
// decides it once per set_params (and once more for set_row_shard), builds what it needs and frees what the previous route left behind; every
// other function here is one switch over the route.  The routes and how to select them: DESIGN.md section 5.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include "internal.h"

// Default rule of the partial assembly (profiles/cg_fold_prescatter.txt): sum over the rows that would stay factored of len^2 - 2 len
#define FOLD_FACTOR_FILL_DEFAULT 300000LL

static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
static bool env_zero(const char* name) {   // "=0": a default switched off
  const char* e = getenv(name);
  return e && e[0] == '0';
}

// the literal recurrence the persistent kernel's start-up leaves the loop to (its fallback; its operator is never assembled)
static KktRoute literal_route(const cosmo_hip_handle* h) { return h->cg_ru ? KKT_CG_FUSED : KKT_CG_PLAIN; }

void kkt_free(cosmo_hip_handle* h) {
  free_op_split(h);
  ldl_free(h);
  schur_free(h);
  pcg_free(h);
  sr_free(h);
  h->route = KKT_NONE;
}

// The switches that select a route are read here only:
//   COSMO_HIP_OP_SPLIT=0       the reduced operator stays P + sigma I + A' rho A with the whole A (no split form, hence no assembly)
//   COSMO_HIP_OP_FOLD=0        no assembled operator
//   COSMO_HIP_CG_FUSE_DIR=0    the four-launch literal recurrence (k_cg_dirA needs the {r, u} records, which the assembled operator gathers too)
//   COSMO_HIP_CG_PERSIST=1     the persistent single-launch CG where the operator fits it (the split operator stays unassembled)
//   COSMO_HIP_FOLD_FACTOR=0|1  partial assembly off / forced: rows of A with >= COSMO_HIP_FOLD_FACTOR_MIN (4) nonzeros stay factored (literal recurrence
//                              only).  Unset: factored where that avoids at least COSMO_HIP_FOLD_FACTOR_FILL (FOLD_FACTOR_FILL_DEFAULT) assembled entries
//   COSMO_HIP_FOLD_PRESCATTER=0  factored rows: the CSR-stream update kernel k_cg_updF0 instead of the pre-scattered image (read in cg_fold.hip: fold_build)
//   COSMO_HIP_CG_SR_DEFAULT=1  lab switch: kkt_kind CG on a fully assembled operator runs the one-launch single-reduction recurrence
// force_split (set_row_shard): h->A becomes a row slice, so the reduced operator must be the split form of the WHOLE A, for any A; the persistent
// kernel, whose operands are sized for the unsharded handle, gives way to the multi-kernel loop.  Everything else of the route stays.
int32_t kkt_configure(cosmo_hip_handle* h, bool force_split) {
  const int kind = h->prm.kkt_kind;
  const bool cg = kind == COSMO_HIP_KKT_CG || kind == COSMO_HIP_KKT_CG_SR || kind == COSMO_HIP_KKT_CG_JACOBI;
  const bool split = !env_zero("COSMO_HIP_OP_SPLIT") || force_split;
  const bool fold = !env_zero("COSMO_HIP_OP_FOLD");
  const bool fuse = env_int("COSMO_HIP_CG_FUSE_DIR", 1) != 0;
  const bool persist = env_int("COSMO_HIP_CG_PERSIST", 0) != 0;
  // partial assembly: forced either way by COSMO_HIP_FOLD_FACTOR; unset, the rows stay factored where the fill that avoids reaches FOLD_FACTOR_FILL_DEFAULT
  // (decided once per plan from the row lengths of A; cg_fold.hip: fold_build)
  int factor_min = 0;
  long long factor_fill_min = 0;
  if (kind == COSMO_HIP_KKT_CG && !env_zero("COSMO_HIP_FOLD_FACTOR")) {
    factor_min = env_int("COSMO_HIP_FOLD_FACTOR_MIN", 4); if (factor_min < 2) factor_min = 4;
    if (env_int("COSMO_HIP_FOLD_FACTOR", 0) == 0) { factor_fill_min = FOLD_FACTOR_FILL_DEFAULT; if (const char* e = getenv("COSMO_HIP_FOLD_FACTOR_FILL")) factor_fill_min = atoll(e); }
  }
  const bool sr_default = env_int("COSMO_HIP_CG_SR_DEFAULT", 0) != 0;
  if (sr_default && factor_fill_min > 0) factor_min = 0;      // the lab switch asks for the fully assembled operator; only a forced factoring overrides it
  if (force_split) {
    if (h->route == KKT_CG_PERSIST) { pcg_free(h); h->route = literal_route(h); }
    if (h->op_split) return COSMO_HIP_OK;
  } else {
    // what the previous route of this handle left behind (a complete factor of the same pattern is kept: ldl_setup reuses its analysis)
    free_op_split(h);
    pcg_free(h);
    sr_free(h);
    if (kind != COSMO_HIP_KKT_DIRECT) ldl_free(h);
    schur_free(h);
    h->route = KKT_NONE;
    if (h->mr) { (void)hipFree(h->mr); h->mr = nullptr; }
    if (h->cg_ru) { (void)hipFree(h->cg_ru); h->cg_ru = nullptr; }
    if (kind == COSMO_HIP_KKT_MINRES || kind == COSMO_HIP_KKT_MINRES_REDUCED) CHK(minres_alloc(h));
    if (kind == COSMO_HIP_KKT_CG_SR) CHK(sr_alloc(h));
    if ((kind == COSMO_HIP_KKT_CG || kind == COSMO_HIP_KKT_CG_JACOBI) && fuse && h->n > 0) {
      // fused direction + A product (k_cg_dirA): one launch less per Krylov iteration, bit-identical
      HIPCHK(h, hipMalloc((void**)&h->cg_ru, sizeof(real) * 2 * (size_t)h->n));
      HIPCHK(h, hipMemsetAsync(h->cg_ru, 0, sizeof(real) * 2 * (size_t)h->n, h->stream));
    }
  }
  // the reduced operator: the split form for the CG recurrences (and for the reduced MINRES of a row-sharded handle), assembled where sparse
  // enough for the recurrences that gather records -- {r, u} of the fused literal pair, {r, w, s, p} of the single-reduction one
  bool sr = kind == COSMO_HIP_KKT_CG_SR;
  if (split && (cg || (force_split && kind == COSMO_HIP_KKT_MINRES_REDUCED)))
    CHK(build_op_split(h, force_split, cg && fold && !persist && (sr || h->cg_ru), factor_min, factor_fill_min));
  // LAB SWITCH (COSMO_HIP_CG_SR_DEFAULT=1; round 6): kkt_kind CG on an ASSEMBLED reduced operator runs the one-launch
  // single-reduction recurrence (cg_sr.hip: k_sr_M) instead of the literal pair.  Measured as a candidate default and REJECTED (BASELINE config 5:
  // 12.42 vs 11.50 us per Krylov iteration -- the 24-byte gathers of {r, w, s} from 32-byte records cost more than the launch they save, every
  // XCD re-fetches the whole table through the fabric at each kernel boundary --, 236.6 vs 244.9 it/s; and at a 1e-10 stopping threshold the
  // recurrence needs +1.2 % Krylov iterations, outside the +-1 per solve the parity tests allow; profiles/r06_cg_one_launch_default.txt).
  // A partially assembled operator belongs to the literal pair.
  if (kind == COSMO_HIP_KKT_CG && h->op_fold && ((FoldPlan*)h->fold)->nd == 0 && sr_default) {
    sr = true;
    if (h->cg_ru) { (void)hipFree(h->cg_ru); h->cg_ru = nullptr; }      // the {r, u} records of the literal pair
    CHK(sr_alloc(h));
  }
  switch (kind) {
    case COSMO_HIP_KKT_DIRECT:
      // QdldlKKTSolver (kktsolver.jl:285-307): analysis (kept while the pattern and the requested ordering stay), factorisation, inertia check.
      // A refused factor stays readable through cosmo_hip_direct_info (positive pivots).
      h->route = KKT_DIRECT;
      return ldl_setup(h, h->kkt_perm);
    case COSMO_HIP_KKT_SCHUR:
      // exact solve of the reduced system (schur.hip): analysis, limits (UNSUPPORTED beyond them, no fallback), factorisation, pivot check
      h->route = KKT_SCHUR;
      return schur_setup(h);
    case COSMO_HIP_KKT_MINRES: h->route = KKT_MINRES_FULL; break;
    case COSMO_HIP_KKT_MINRES_REDUCED: h->route = KKT_MINRES_REDUCED; break;
    case COSMO_HIP_KKT_CG_JACOBI:
      // the opt-in Jacobi-preconditioned CG lives on the ASSEMBLED reduced operator (its diagonal is the preconditioner): no silent fallback to the
      // unpreconditioned recurrence when the operator cannot be assembled (dense A' rho A: BASELINE config 2, where Jacobi makes the count worse anyway)
      if (!h->op_fold) return cosmo_fail(h, COSMO_HIP_ERR_UNSUPPORTED, "kkt_kind CG_JACOBI needs the assembled reduced operator (csrc/cg_fold.hip: A' rho A too dense here, or COSMO_HIP_OP_FOLD=0 / COSMO_HIP_CG_FUSE_DIR=0)");
      h->route = KKT_CG_JACOBI;
      break;
    default:
      if (h->op_fold) h->route = sr ? KKT_CG_SR_M : ((FoldPlan*)h->fold)->nd > 0 ? KKT_CG_FOLD_PARTIAL : KKT_CG_FOLD;
      else if (sr) h->route = KKT_CG_SR;
      else if (persist && !force_split && h->n > 0) {
        bool accepted = false;
        CHK(pcg_setup(h, &accepted));
        h->route = accepted ? KKT_CG_PERSIST : literal_route(h);
      } else h->route = literal_route(h);
  }
  return refresh_op_split(h);      // the rho-dependent values of the split / assembled operator (the Jacobi preconditioner with them)
}

int32_t kkt_update_rho(cosmo_hip_handle* h) {
  if (h->route != KKT_DIRECT && h->route != KKT_SCHUR) return refresh_op_split(h);
  const int32_t rc = h->route == KKT_SCHUR ? schur_refactor_now(h) : ldl_refactor_now(h, false);     // update_rho!(::QdldlKKTSolver): new values, refactor (:316-320)
  if (rc != COSMO_HIP_OK) { h->have_params = false; h->have_iterates = false; }    // a zero pivot leaves no usable factor
  return rc;
}

// P.val / A.val and the other resident copies hold new values of the same pattern (cosmo_hip_update_matrices): what the route derived from them follows.
// No route caches values anywhere else (DESIGN.md "Matrix value updates"): the persistent kernel and both MINRES kinds read the copies themselves, the
// direct solver refills its panels from P.val / A.val, so no route needs kkt_configure again (upd_host_rebuilds stays 0).
int32_t kkt_update_values(cosmo_hip_handle* h) {
  switch (h->route) {
    case KKT_NONE: return cosmo_fail(h, COSMO_HIP_ERR_INVALID, "update_matrices: the handle has no KKT route (set_params failed)");
    case KKT_MINRES_FULL: case KKT_MINRES_REDUCED: return COSMO_HIP_OK;
    case KKT_DIRECT: {
      const int32_t rc = ldl_refactor_now(h, true);      // same analysis, same plan; the inertia check because the new P may not be convex
      if (rc != COSMO_HIP_OK) { h->have_params = false; h->have_iterates = false; }
      return rc;
    }
    case KKT_SCHUR: {
      const int32_t rc = schur_refactor_now(h);           // the maps read P.val / A.val themselves: refill, refactorise, pivot check
      if (rc != COSMO_HIP_OK) { h->have_params = false; h->have_iterates = false; }
      return rc;
    }
    default:
      CHK(upd_refresh_operator(h));
      return refresh_op_split(h);      // k_op_refresh, k_fold_refresh, k_fold_dinv and the padded copy: the rho-dependent values
  }
}

// rho may have changed on the device: the diagonal part of A' rho A follows (cheap, unconditional); the direct solver refills and
// refactorises, each launch a no-op unless rho changed
int32_t kkt_enqueue_refresh(cosmo_hip_handle* h) {
  if (h->route == KKT_SCHUR) return schur_enqueue_refactor(h, 1);
  return h->route == KKT_DIRECT ? ldl_enqueue_refactor(h, 1) : refresh_op_split(h);
}

// ---- the CG routes ------------------------------------------------------------------------------------------------------------------------
static real tol_for_solve(const cosmo_hip_handle* h, long long k) {
  return h->prm.tol_constant / pow((real)k, h->prm.tol_exponent);  // get_tolerance, kktsolver_indirect.jl:168-170
}

// rhs = A' y2 + ls_x, r0 = rhs - L x0 and the tolerance of the solve; the single-reduction recurrences add w0 = L r0 and their records
int32_t kkt_enqueue_start(cosmo_hip_handle* h, int guard, real tol_k) {
  CHK(enqueue_cg_rhs(h, guard));
  switch (h->route) {
    case KKT_CG_SR_M: CHK(fold_enqueue_start(h, guard, tol_k)); return sr_enqueue_start(h, guard);
    case KKT_CG_SR: CHK(enqueue_cg_start(h, guard, tol_k)); return sr_enqueue_start(h, guard);
    case KKT_CG_JACOBI: case KKT_CG_FOLD_PARTIAL: case KKT_CG_FOLD: return fold_enqueue_start(h, guard, tol_k);
    default: return enqueue_cg_start(h, guard, tol_k);
  }
}

// Krylov iterations k_begin .. k_begin + count - 1 and the stopping rule behind the last one
int32_t kkt_enqueue_iterations(cosmo_hip_handle* h, int guard, int k_begin, int count) {
  switch (h->route) {
    case KKT_CG_SR_M: case KKT_CG_SR: return sr_enqueue_iterations(h, guard, k_begin, count);
    case KKT_CG_JACOBI: case KKT_CG_FOLD_PARTIAL: case KKT_CG_FOLD: return fold_enqueue_iterations(h, guard, k_begin, count);
    default: return enqueue_cg_iterations(h, guard, k_begin, count);
  }
}

// a failed start-up rendezvous of the persistent kernel stalls the solve before it modified anything: the loop continues with the multi-kernel recurrence
static void pcg_fallback(cosmo_hip_handle* h) {
  h->route = literal_route(h);
  h->pcg_fallbacks += 1;
}

// one solve of the loop, enqueued without synchronisation behind k_rhs
int32_t kkt_enqueue_loop_solve(cosmo_hip_handle* h) {
  switch (h->route) {
    case KKT_DIRECT: return ldl_enqueue_solve(h, 1, true);
    case KKT_SCHUR:          // the right-hand side of the CG routes, the exact solve, the tail; no Krylov budget
      CHK(enqueue_cg_rhs(h, 1));
      CHK(schur_enqueue_solve(h, 1));
      return enqueue_tail(h, 1);
    case KKT_MINRES_FULL: case KKT_MINRES_REDUCED: return minres_enqueue_solve(h, 1, true);
    default: break;
  }
  CHK(kkt_enqueue_start(h, 1, tol_for_solve(h, h->host_solves + 1)));
  if (h->route == KKT_CG_PERSIST) {
    CHK(pcg_enqueue_solve(h, 1));        // the whole Krylov loop in one launch (cg_persist.hip)
  } else if (h->exact_launches) {
    // measurement mode: one Krylov iteration per host round trip, so that every launch does full work
    CHK(kkt_enqueue_iterations(h, 1, 0, 0));
    for (int k = 0;; ++k) {
      CHK(sync_ctl(h));
      if (h->ctl_host->cg_done || h->ctl_host->halt) break;
      CHK(kkt_enqueue_iterations(h, 1, k, 1));
    }
  } else {
    int bud = 0;
    CHK(solve_budget(h, &bud));
    CHK(kkt_enqueue_iterations(h, 1, 0, bud));
    h->cg_k_likely = 0x7fffffff;
  }
  CHK(enqueue_tail(h, 1));
  return feedback_record(h);
}

// one solve of cosmo_hip_kkt_solve (ls_x / ls_s uploaded), paced by the host in doubling chunks of Krylov iterations
int32_t kkt_solve_now(cosmo_hip_handle* h) {
  switch (h->route) {
    case KKT_DIRECT: return ldl_enqueue_solve(h, 0, false);          // the full (n+m) system, as solve!(::QdldlKKTSolver) (kktsolver.jl:310-313)
    case KKT_MINRES_FULL: case KKT_MINRES_REDUCED: return minres_enqueue_solve(h, 0, false);
    case KKT_SCHUR:
      CHK(enqueue_y2_only(h));
      CHK(enqueue_cg_rhs(h, 0));
      CHK(schur_enqueue_solve(h, 0));
      CHK(enqueue_tail(h, 0));
      return enqueue_count_solve(h);
    default: break;
  }
  CHK(enqueue_y2_only(h));
  CHK(kkt_enqueue_start(h, 0, tol_for_solve(h, h->host_solves + 1)));
  bool solved = false;
  if (h->route == KKT_CG_PERSIST) {
    CHK(pcg_enqueue_solve(h, 0));
    CHK(sync_ctl(h));
    solved = !h->ctl_host->stalled;
    if (!solved) { pcg_fallback(h); CHK(enqueue_clear_stall(h)); }
  }
  for (int k = 0, chunk = std::max(h->budget, 4); !solved; k += chunk, chunk = std::min(chunk * 2, 1024)) {
    CHK(kkt_enqueue_iterations(h, 0, k, chunk));
    CHK(sync_ctl(h));
    solved = h->ctl_host->cg_done;
  }
  CHK(enqueue_tail(h, 0));
  return enqueue_count_solve(h);
}

// the Krylov budget of a loop solve ran out before convergence: clear the stall and enqueue `extra` more iterations of it
int32_t kkt_resume(cosmo_hip_handle* h, int extra) {
  CHK(enqueue_clear_stall(h));
  switch (h->route) {
    case KKT_DIRECT: case KKT_SCHUR: return COSMO_HIP_OK;        // no Krylov budget: a direct solve does not stall
    case KKT_MINRES_FULL: case KKT_MINRES_REDUCED: return minres_resume(h, extra);
    case KKT_CG_PERSIST: pcg_fallback(h); break;
    default: break;
  }
  CHK(kkt_enqueue_iterations(h, 1, h->ctl_host->cg_k, extra));
  return enqueue_tail(h, 1);
}

// cosmo_hip_time_krylov: the recurrences of the loop it times (not the persistent kernel, not the two-launch single-reduction form), their
// algorithmic bytes and launches per Krylov iteration
bool kkt_krylov_model(const cosmo_hip_handle* h, double* bytes, int* launches) {
  const double n = (double)h->n, m = (double)h->m;
  switch (h->route) {
    case KKT_CG_JACOBI: case KKT_CG_SR_M: case KKT_CG_FOLD_PARTIAL: case KKT_CG_FOLD: {
      const FoldPlan* f = (const FoldPlan*)h->fold;
      // B_spmv(M) of the FULLY assembled operator (the unit since round 2; a partially assembled operator streams fewer entries for the same
      // product) + B_cgvec (n-side); Jacobi adds dinv: + 8 n.  The one-launch recurrence: the SAME algorithmic bytes (SURVEY 8d prices a Krylov
      // iteration of the reference: operator + 10 n-vectors; the records {r, w, s, p} read and written once by their owners + x read and written
      // are 10 n words too)
      *bytes = 12.0 * (double)f->nnz_full + 4.0 * (n + 1) + 16.0 * n + 8.0 * 10.0 * n + (h->route == KKT_CG_JACOBI ? 8.0 * n : 0.0);
      *launches = h->route == KKT_CG_SR_M ? 1 : 2;
      return true;
    }
    case KKT_CG_FUSED: case KKT_CG_PLAIN: {
      const CsrDev& Ao = h->op_split ? h->Am : h->A;
      const CsrDev& PTo = h->op_split ? h->PTm : h->PT;
      *bytes = (12.0 * Ao.nnz + 4.0 * (Ao.nrows + 1) + 8.0 * n + 8.0 * Ao.nrows) + (12.0 * PTo.nnz + 8.0 * (n + 1) + 8.0 * (n + Ao.nrows) + 8.0 * n) + 8.0 * (10.0 * n + m);
      *launches = h->route == KKT_CG_FUSED ? 3 : 4;
      return true;
    }
    default: return false;
  }
}

extern "C" const char* cosmo_hip_kkt_recurrence(cosmo_hip_handle* h) {
  if (!h || !h->have_params) return "not set up";
  static const char* sr_names[] = {"", "k_sr_M<1>", "k_sr_M<2>", "k_sr_M<3>", "k_sr_M<4>", "", "", "", "k_sr_M<8>"};
  static const char* pair_names[] = {"", "k_cg_dirM<1, false> + k_cg_upd<false>", "k_cg_dirM<2, false> + k_cg_upd<false>", "k_cg_dirM<3, false> + k_cg_upd<false>",
                                     "k_cg_dirM<4, false> + k_cg_upd<false>", "", "", "", "k_cg_dirM<8, false> + k_cg_upd<false>"};
  static const char* updf_names[] = {"", "k_cg_dirM<1, false> + k_cg_updF", "k_cg_dirM<2, false> + k_cg_updF", "k_cg_dirM<3, false> + k_cg_updF", "k_cg_dirM<4, false> + k_cg_updF", "", "", "",
                                     "k_cg_dirM<8, false> + k_cg_updF"};
  static const char* pc_names[] = {"", "k_cg_dirM<1, true> + k_cg_upd<true>", "k_cg_dirM<2, true> + k_cg_upd<true>", "k_cg_dirM<3, true> + k_cg_upd<true>",
                                   "k_cg_dirM<4, true> + k_cg_upd<true>", "", "", "", "k_cg_dirM<8, true> + k_cg_upd<true>"};
  static thread_local char buf[256];
  const FoldPlan* f = (const FoldPlan*)h->fold;
  const int sl = (h->op_fold && f) ? ((f->slots >= 1 && f->slots <= 4) ? f->slots : 8) : 0;
  switch (h->route) {
    case KKT_NONE: break;
    case KKT_DIRECT: return "direct: supernodal LDL' of the full KKT system, one launch per tree level (csrc/ldl.hip)";
    case KKT_SCHUR: return schur_describe(h, buf, sizeof buf) ? buf : "not set up";
    case KKT_MINRES_FULL: return "minres on the full KKT system (csrc/minres.hip)";
    case KKT_MINRES_REDUCED: return "minres on the reduced system (csrc/minres.hip)";
    case KKT_CG_PERSIST: return "cg: literal recurrence in one persistent launch (csrc/cg_persist.hip, opt-in)";
    case KKT_CG_JACOBI: snprintf(buf, sizeof buf, "cg: Jacobi-preconditioned recurrence on the assembled operator (opt-in), %s", pc_names[sl]); return buf;
    case KKT_CG_SR_M:
      snprintf(buf, sizeof buf, "cg: one-launch single-reduction recurrence on the assembled operator%s, %s",
               h->prm.kkt_kind == COSMO_HIP_KKT_CG ? " (lab switch COSMO_HIP_CG_SR_DEFAULT=1)" : " (opt-in kkt_kind CG_SR)", sr_names[sl]);
      return buf;
    case KKT_CG_SR: return "cg: single-reduction recurrence, two launches per iteration (kkt_kind CG_SR), k_sr_update_A + k_sr_op";
    case KKT_CG_FOLD_PARTIAL:
      snprintf(buf, sizeof buf, "cg: literal recurrence on the partially assembled operator (%d rows of A kept factored), two launches per iteration, %s%s", f->nd, updf_names[sl],
               f->ps_mode == 2 ? "" : f->ps_mode == 1 ? " (dense-row image without pre-scattered operands, COSMO_HIP_FOLD_PRESCATTER=2)"
                                                      : " (CSR-stream dense rows k_cg_updF0, COSMO_HIP_FOLD_PRESCATTER=0)");      // default: k_cg_dirMs<SL, 2> + k_cg_updF<2>
      return buf;
    case KKT_CG_FOLD: snprintf(buf, sizeof buf, "cg: literal recurrence on the assembled operator, two launches per iteration, %s", pair_names[sl]); return buf;
    case KKT_CG_FUSED: return "cg: literal recurrence, three launches per iteration, k_cg_dirA + k_op_apply + k_cg_upd<false>";
    case KKT_CG_PLAIN: return "cg: literal recurrence, four launches per iteration, k_cg_dir + k_spmv_A_rho + k_op_apply + k_cg_upd<false>";
  }
  return "not set up";
}
