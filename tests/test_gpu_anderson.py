"""GPU tests of the accelerated loop: Anderson acceleration (type II, QR, restarted memory, mem 15) with
safeguarding on the device against the oracle's restatement of the same algorithm.  COSMOAccelerators.jl is not part of
the reference tree, so PARITY IS UNPINNED for this path: what is checked is (a) device == oracle restatement (same status,
iteration counts within one check interval, same solution), (b) the assertions the reference's own tests make on
accelerated runs (test/UnitTests/AccelerationTests, and every status / objective golden, which the reference asserts under
its default = accelerated settings).

What these whole-solve tests cover: the ORDER of the accelerated loop (acceleration_pre! before admm_z!, the safeguarding step and its
extra ADMM iteration after the solve), the rho updates and infeasibility checks DEFERRED to the next non-accelerated iteration, the restart
after a rho adaption, the activation rules inside a run, and the counters of a solve (accelerated / accepted / declined / restarts,
safeguarding_iter in Result.iter) -- an accelerated run is chaotic in its last bits, so they compare at the end of a solve and within wide
tolerances, which a subtly wrong accelerator survives (the safeguard declines a bad candidate and ADMM converges anyway).  The ARITHMETIC
of the accelerator -- the Gram-Schmidt / Gram-matrix update, the least-squares solve, the candidate, the singular / eta_max / min_mem /
memory-restart branches, the safeguard's norm and reset, for every kind, at one to three workgroups and l up to 32 -- is checked one update
and one candidate at a time against a long-double reference in tests/test_gpu_anderson_steps.py (this file's kernels, through
Handle.accel_pre / accel_post / accel_restart) and tests/test_gpu_batch_anderson_steps.py (the batch kernels' copy)."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from oracle import cosmo_oracle as O
from tests import util

pytestmark = pytest.mark.gpu
F = cj._ffi

P_SIMPLE = np.array([[4.0, 1], [1, 2]]); Q_SIMPLE = np.array([1.0, 1])


def _simple_cons(mod):
    A = np.array([[1.0, 1], [1, 0], [0, 1]])
    l = np.array([1.0, 0, 0]); u = np.array([1.0, 0.7, 0.7])
    if mod is cj:
        return [cj.Constraint(np.vstack([-A, A]), np.concatenate([u, -l]), cj.Nonnegatives)]
    return [O.Constraint(np.vstack([-A, A]), np.concatenate([u, -l]), O.Nonnegatives(6))]


def _both(P, q, cons_model, cons_oracle, tol_iter=25, **st):
    # Anderson acceleration of an inexactly evaluated fixed-point map is chaotic in the last bits of the KKT solves (with the default
    # CG tolerance 1/k^1.5 a 1e-16 change of the operator's rounding moves the iteration count by tens), so trajectories are
    # compared with a tight constant CG tolerance on both sides
    model = cj.Model()
    tight = cj.with_options(cj.CGIndirectKKTSolver, tol_constant=1e-10, tol_exponent=0.0)
    cj.assemble(model, P, q, cons_model, settings=cj.Settings(accelerator=cj.AndersonAccelerator, kkt_solver=tight, **st))
    res = cj.optimize(model)
    stats = model.handle.accel_stats()
    A, b, cones = O.assemble(cons_oracle)
    ws = O.Workspace(P, q, A, b, cones, O.Settings(kkt_solver="cg", tol_constant=1e-10, tol_exponent=0.0, accelerator="anderson", **st))
    ref = ws.optimize()
    assert res.status == ref.status, (res.status, ref.status)
    assert abs(res.iter - ref.iter) <= tol_iter, (res.iter, ref.iter)
    return res, ref, stats, ws


@pytest.mark.parametrize("fold", [False, True])
def test_simple_qp_accelerated_matches_oracle_and_goldens(fold, monkeypatch):
    # fold = False: the assembled operator of csrc/cg_fold.hip is off (COSMO_HIP_OP_FOLD=0), the association the tolerance of +-1 accelerated
    # step was written for; fold = True (the default build): same operator, different association, one more acceptance decision may move.
    # (The eta-norm acceptance test sits at a tie on this 2-variable problem: measured with the unsplit operator, COSMO_HIP_OP_SPLIT=0, the
    # count moves by 3 -- the sensitivity is the problem's, not a property of one association.)
    if not fold:
        monkeypatch.setenv("COSMO_HIP_OP_FOLD", "0")
    res, ref, stats, ws = _both(P_SIMPLE, Q_SIMPLE, _simple_cons(cj), _simple_cons(O), tol_iter=2)
    assert res.status == "Solved"                                              # AccelerationTests/anderson_accelerator.jl:37-43
    assert abs(res.obj_val - 1.88) < 1e-3 and np.linalg.norm(res.x - [0.3, 0.7]) < 1e-3     # simple.jl:45-47
    # the eta-norm acceptance test sits at a tie on this 2-variable problem: a different association of the reduced operator (operator
    # split / assembled operator, csrc/cg_fold.hip) moves one or two acceptance decisions while iterates and iteration count agree
    assert stats["accelerated"] > 0 and abs(stats["accelerated"] - ws.accelerator.num_accelerated_steps) <= (1 if not fold else 2)
    assert abs(stats["safeguarding_iter"] - ws.safeguarding_iter) <= 1
    assert np.linalg.norm(res.x - ref.x) < 1e-7
    # fewer iterations than the plain loop
    model = cj.Model(); cj.assemble(model, P_SIMPLE, Q_SIMPLE, _simple_cons(cj), settings=cj.Settings())
    plain = cj.optimize(model)
    assert res.iter <= plain.iter


def test_rho_adaption_goldens_with_accelerator():
    # AccelerationTests/max_rho_adaption.jl:19-32
    res, ref, _, _ = _both(P_SIMPLE, Q_SIMPLE, _simple_cons(cj), _simple_cons(O), adaptive_rho_interval=25, adaptive_rho_max_adaptions=2,
                           rho=1e-6, eps_abs=1e-6, eps_rel=1e-4)
    assert len(res.info.rho_updates) - 1 == 2 == len(ref.rho_updates) - 1
    assert np.allclose(res.info.rho_updates, ref.rho_updates, rtol=1e-6)
    res, ref, _, _ = _both(P_SIMPLE, Q_SIMPLE, _simple_cons(cj), _simple_cons(O), tol_iter=10 ** 6, adaptive_rho_interval=25,
                           adaptive_rho_max_adaptions=1, rho=1e-6, eps_abs=1e-4, eps_rel=1e-4, max_iter=300)
    assert len(res.info.rho_updates) - 1 == 1


def test_max_iter_counts_safeguarding_steps():
    model = cj.Model()
    tight = cj.with_options(cj.CGIndirectKKTSolver, tol_constant=1e-10, tol_exponent=0.0)
    cj.assemble(model, P_SIMPLE, Q_SIMPLE, _simple_cons(cj), settings=cj.Settings(accelerator=cj.AndersonAccelerator, kkt_solver=tight, max_iter=20, eps_abs=1e-12, eps_rel=1e-12))
    res = cj.optimize(model)
    st = model.handle.accel_stats()
    A, b, cones = O.assemble(_simple_cons(O))
    ws = O.Workspace(P_SIMPLE, Q_SIMPLE, A, b, cones, O.Settings(kkt_solver="cg", tol_constant=1e-10, tol_exponent=0.0, accelerator="anderson", max_iter=20, eps_abs=1e-12, eps_rel=1e-12))
    ref = ws.optimize()
    assert (res.iter, st["safeguarding_iter"], res.status) == (ref.iter, ws.safeguarding_iter, ref.status)      # solver.jl:140,173 quirk included


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_qp_accelerated_matches_oracle(seed):
    rng = np.random.default_rng(seed)
    prob = util.random_qp(rng, 40, 4, 30, 25, soc_dims=(5, 3), p_shift=2.0)
    st = dict(eps_abs=1e-7, eps_rel=1e-7)
    # Anderson acceleration of an INEXACT fixed-point map is noise sensitive (with the default CG tolerance 1/k^1.5 the
    # oracle needs 125 .. >5000 iterations on these instances, against 75 .. 125 with an exact KKT solve), so the comparison
    # of trajectories uses a tight constant CG tolerance on both sides
    tight = cj.with_options(cj.CGIndirectKKTSolver, tol_constant=1e-10, tol_exponent=0.0)
    model = cj.Model(); model.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], cj.Settings(accelerator=cj.AndersonAccelerator, kkt_solver=tight, **st))
    res = cj.optimize(model)
    ws = O.Workspace(prob["P"], prob["q"], prob["A"], prob["b"], util.oracle_cones(prob["sets"]),
                     O.Settings(kkt_solver="cg", tol_constant=1e-10, tol_exponent=0.0, accelerator="anderson", **st))
    ref = ws.optimize()
    assert ref.iter <= 150
    assert res.status == ref.status == "Solved"
    assert abs((res.iter - res.safeguarding_iter) - (ref.iter - ref.safeguarding_iter)) <= 25       # loop indices (Result.iter adds the safeguarding steps)
    assert abs(res.obj_val - ref.obj_val) <= 1e-5 * (1 + abs(ref.obj_val))
    assert np.linalg.norm(res.x - ref.x) <= 1e-4 * max(1.0, np.linalg.norm(ref.x))
    plain = cj.Model(); plain.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], cj.Settings(kkt_solver=tight, **st))
    rp = cj.optimize(plain)
    assert rp.status == "Solved" and abs(rp.obj_val - res.obj_val) <= 1e-5 * (1 + abs(rp.obj_val))
    assert res.iter < rp.iter


def test_accelerated_infeasibility_and_cones():
    E3 = sp.identity(3, format="csc"); P0 = sp.csc_matrix((3, 3))
    # Box goldens (qp-box.jl:50,87) under the accelerated loop: deferred infeasibility checks (update_suggested)
    for (Am, b, P, q, l, u, want) in [([[1.0, 0], [1, 0]], [2.0, 0], np.eye(2), [1.0, -1], [0.0, 0], [1.0, 1], "Primal_infeasible"),
                                      (np.eye(2), [1.0, 1], np.zeros((2, 2)), [1.0, 1], [0.0, -np.inf], [1.0, 3], "Dual_infeasible")]:
        res, ref, _, _ = _both(sp.csc_matrix(np.array(P, dtype=float)), np.array(q, dtype=float),
                               [cj.Constraint(sp.csc_matrix(np.array(Am, dtype=float)), b, cj.Box(l, u))],
                               [O.Constraint(sp.csc_matrix(np.array(Am, dtype=float)), b, O.Box(l, u))], tol_iter=40)
        assert res.status == want
    # exponential cone golden (exp_cone.jl:19-42)
    A2 = sp.csc_matrix(np.array([[0, 1.0, 0], [0, 0, 1]])); b2 = np.array([-1.0, -math.exp(5)])
    res, ref, st, _ = _both(P0, np.array([-1.0, 0, 0]),
                            [cj.Constraint(E3, np.zeros(3), cj.ExponentialCone), cj.Constraint(A2, b2, cj.ZeroSet)],
                            [O.Constraint(E3, np.zeros(3), O.ExponentialCone()), O.Constraint(A2, b2, O.ZeroSet(2))], eps_abs=1e-4, eps_rel=1e-4)
    assert res.status == "Solved" and abs(res.obj_val + 5.0) < 1e-2
    # small closest-correlation SDP (closestcorr.jl structure): PSD projection inside the accelerated loop
    pr = cj.problems.closest_correlation(d=10, seed=4)
    model = cj.Model(); model.set(pr["P"], pr["q"], pr["A"], pr["b"], pr["sets"], cj.Settings(accelerator=cj.AndersonAccelerator, eps_abs=1e-6, eps_rel=1e-6))
    res = cj.optimize(model)
    ws = O.Workspace(pr["P"], pr["q"], pr["A"], pr["b"], util.oracle_cones(pr["sets"]), O.Settings(kkt_solver="cg", accelerator="anderson", eps_abs=1e-6, eps_rel=1e-6))
    ref = ws.optimize()
    # (the loop index stops on a multiple of check_termination; Result.iter adds the safeguarding steps, src/solver.jl:196)
    assert res.status == ref.status == "Solved" and abs((res.iter - res.safeguarding_iter) - (ref.iter - ref.safeguarding_iter)) <= 25
    # both stop at eps = 1e-6 on slightly different iterations of an accelerated run: SURVEY 8c default-schedule tolerance is 1e-4 (1 + |obj|)
    assert abs(res.obj_val - ref.obj_val) < 1e-5 * (1 + abs(ref.obj_val))


def test_accelerated_run_is_bitwise_reproducible_and_restartable():
    rng = np.random.default_rng(5)
    prob = util.random_qp(rng, 50, 3, 30, 30, p_shift=2.0)
    outs = []
    for _ in range(2):
        model = cj.Model(); model.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"],
                                      cj.Settings(accelerator=cj.with_options(cj.AndersonAccelerator, mem=8), max_iter=120, eps_abs=0, eps_rel=0))
        r = cj.optimize(model)
        outs.append(np.concatenate([r.x, r.s, r.y]))
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64))
    r2 = cj.optimize(model)                                       # warm-started second optimize!: accelerator restarted (setup.jl:47-49)
    assert r2.status in ("Max_iter_reached", "Undetermined")


def test_accuracy_activation_matches_oracle():
    """AccuracyActivation(eps) (src/accelerator_interface.jl:14-21,38-46): the accelerator stays off until a termination check
    sees residuals below eps; device and oracle switch it on at the same check and then follow the same trajectory."""
    rng = np.random.default_rng(5)
    p = util.random_qp(rng, 40, 4, 30, 0, p_shift=1.0)
    tight = cj.with_options(cj.CGIndirectKKTSolver, tol_constant=1e-10, tol_exponent=0.0)
    out = {}
    for name, act, okw in (("accuracy", cj.AccuracyActivation(1e-2), dict(acc_start_accuracy=1e-2)), ("immediate", 2, {})):
        model = cj.Model()
        model.set(p["P"], p["q"], p["A"], p["b"], p["sets"],
                  cj.Settings(accelerator=cj.AndersonAccelerator, accelerator_activation=act, kkt_solver=tight, eps_abs=1e-7, eps_rel=1e-7))
        res = cj.optimize(model)
        stats = model.handle.accel_stats()
        ws = O.Workspace(p["P"], p["q"], p["A"], p["b"], util.oracle_cones(p["sets"]),
                         O.Settings(kkt_solver="cg", tol_constant=1e-10, tol_exponent=0.0, accelerator="anderson", eps_abs=1e-7, eps_rel=1e-7, **okw))
        ref = ws.optimize()
        assert res.status == ref.status == "Solved"
        assert abs((res.iter - res.safeguarding_iter) - (ref.iter - ref.safeguarding_iter)) <= 25, (name, res.iter, ref.iter)
        assert abs(stats["accelerated"] - ws.accelerator.num_accelerated_steps) <= max(2, 0.1 * ws.accelerator.num_accelerated_steps)
        assert np.linalg.norm(res.x - ref.x) <= 1e-5 * max(1.0, np.linalg.norm(ref.x))
        out[name] = (res, stats)
    # activation by accuracy starts later, so it accelerates fewer steps than immediate activation
    assert 0 < out["accuracy"][1]["accelerated"] < out["immediate"][1]["accelerated"]


# ---- the non-default variants of docs/src/acceleration.md:23-26 (round 6): Type1 / Type2{NormalEquations} x RestartedMemory / RollingMemory ------
VARIANTS = [("anderson_type1_rolling", (cj.Type1, cj.RollingMemory)), ("anderson_type1_restarted", (cj.Type1, cj.RestartedMemory)),
            ("anderson_type2ne_rolling", (cj.Type2[cj.NormalEquations], cj.RollingMemory)),
            ("anderson_type2ne_restarted", (cj.Type2[cj.NormalEquations], cj.RestartedMemory))]


@pytest.mark.parametrize("oname,params", VARIANTS)
def test_accelerator_variants_match_the_oracle(oname, params):
    """Device (csrc/anderson.hip: k_aa_prep_ne / k_aa_gram / k_aa_solve_ne) against oracle.AndersonAcceleratorNE -- PARITY UNPINNED like the default
    variant: the simple QP of the reference's tests to its golden (simple.jl:45-47) and a random conic QP with a tight constant CG tolerance on both
    sides: same status, loop index within one check interval, same solution, fewer iterations than the plain loop; the accelerator's own counters
    (accelerated steps, safeguarding steps) within a few decisions of the oracle's."""
    acc = cj.AndersonAccelerator[params]
    assert acc.accel_kind in (F.ACCEL_ANDERSON_TYPE1_RESTARTED, F.ACCEL_ANDERSON_TYPE1_ROLLING, F.ACCEL_ANDERSON_TYPE2NE_RESTARTED, F.ACCEL_ANDERSON_TYPE2NE_ROLLING)
    tight = cj.with_options(cj.CGIndirectKKTSolver, tol_constant=1e-10, tol_exponent=0.0)
    okw = dict(kkt_solver="cg", tol_constant=1e-10, tol_exponent=0.0, accelerator=oname)
    # simple QP
    model = cj.Model()
    cj.assemble(model, P_SIMPLE, Q_SIMPLE, _simple_cons(cj), settings=cj.Settings(accelerator=acc, kkt_solver=tight))
    res = cj.optimize(model)
    st = model.handle.accel_stats()
    A, b, cones = O.assemble(_simple_cons(O))
    ws = O.Workspace(P_SIMPLE, Q_SIMPLE, A, b, cones, O.Settings(**okw))
    ref = ws.optimize()
    # (the mem x mem normal equations of a 2-variable problem are rank deficient to rounding: which candidates pass the eta-norm test and the
    #  safeguard differs between two correct implementations -- measured 17 against 12 safeguarding steps with the SAME loop index -- so the
    #  loop index, the solution and the golden are compared, the counters only for plausibility)
    assert res.status == ref.status == "Solved", (res.status, ref.status)
    assert abs((res.iter - res.safeguarding_iter) - (ref.iter - ref.safeguarding_iter)) <= 25, (res.iter, res.safeguarding_iter, ref.iter, ref.safeguarding_iter)
    assert abs(res.obj_val - 1.88) < 1e-3 and np.linalg.norm(res.x - [0.3, 0.7]) < 1e-3 and np.linalg.norm(res.x - ref.x) < 1e-6
    assert st["accelerated"] > 0 and ws.accelerator.num_accelerated_steps > 0 and st["safeguarding_iter"] == res.safeguarding_iter
    if params[1] is cj.RollingMemory:
        assert st["restarts"] == 0
    # random conic QP
    rng = np.random.default_rng(21)
    prob = util.random_qp(rng, 40, 4, 30, 25, soc_dims=(5, 3), p_shift=2.0)
    tol = dict(eps_abs=1e-7, eps_rel=1e-7)
    model = cj.Model(); model.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], cj.Settings(accelerator=acc, kkt_solver=tight, **tol))
    res = cj.optimize(model)
    ws = O.Workspace(prob["P"], prob["q"], prob["A"], prob["b"], util.oracle_cones(prob["sets"]), O.Settings(**okw, **tol))
    ref = ws.optimize()
    assert res.status == ref.status == "Solved"
    assert abs((res.iter - res.safeguarding_iter) - (ref.iter - ref.safeguarding_iter)) <= 25, (res.iter, ref.iter)
    assert abs(res.obj_val - ref.obj_val) <= 1e-5 * (1 + abs(ref.obj_val)) and np.linalg.norm(res.x - ref.x) <= 1e-4 * max(1.0, np.linalg.norm(ref.x))
    plain = cj.Model(); plain.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], cj.Settings(kkt_solver=tight, **tol))
    assert res.iter < cj.optimize(plain).iter


def test_accelerator_variants_reproducible_float32_and_in_a_batch_group():
    """A variant run is bitwise reproducible; the Float32 library runs it; optimize_batch on models with a variant: the persistent batch kernels carry
    the default variant only, so the group solves every member on its own handle (cosmo_hip_batch_set_accelerator: UNSUPPORTED -> fallback) with the
    same result as a single solve."""
    rng = np.random.default_rng(6)
    prob = util.random_qp(rng, 50, 3, 30, 30, p_shift=2.0)
    acc = cj.with_options(cj.AndersonAccelerator[cj.Type1, cj.RollingMemory], mem=6)
    outs = []
    for _ in range(2):
        model = cj.Model(); model.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], cj.Settings(accelerator=acc, max_iter=120, eps_abs=0, eps_rel=0))
        r = cj.optimize(model)
        outs.append(np.concatenate([r.x, r.s, r.y]))
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64))
    m32 = cj.Model(dtype=np.float32); m32.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], cj.Settings(accelerator=acc, eps_abs=1e-4, eps_rel=1e-4))
    m64 = cj.Model(); m64.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], cj.Settings(accelerator=acc, eps_abs=1e-4, eps_rel=1e-4))
    r32, r64 = cj.optimize(m32), cj.optimize(m64)
    assert r32.status == r64.status == "Solved" and abs(r32.obj_val - r64.obj_val) <= 1e-3 * (1 + abs(r64.obj_val))
    probs = [util.random_qp(np.random.default_rng(60 + k), 30, 2, 20, 10, p_shift=2.0) for k in range(3)]
    st = cj.Settings(accelerator=cj.AndersonAccelerator[cj.Type2[cj.NormalEquations], cj.RestartedMemory])
    mods = []
    for p in probs:
        md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st); mods.append(md)
    rb = cj.optimize_batch(mods)
    assert cj.model.LAST_BATCH_INFO["own_handle_members"] == 3, cj.model.LAST_BATCH_INFO
    for p, r in zip(probs, rb):
        md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st)
        rs = cj.optimize(md)
        assert r.status == rs.status == "Solved" and r.iter == rs.iter and np.array_equal(r.x, rs.x)
