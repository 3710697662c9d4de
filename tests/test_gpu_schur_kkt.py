"""The Schur-complement KKT solver on the device (kkt_kind KKT_SCHUR, csrc/schur.hip): an exact solve of the reduced system by block inverses, a
dense capacitance inverse (Woodbury) and safeguarded iterative refinement.  Problems with a prescribed split: tests/schur_cases.py.

  * one fine-grained solve against np.linalg.solve on the full KKT matrix, over the block sides at which the factorisation changes kernel (1, 2, 3 | 4
    .. 64 | 65 .. 256) and over numbers of long rows around the block side 64 of the dense factorisation (ragged last blocks, 1 .. 3 blocks);
  * refinement and its safeguard on P = 0 problems (cond M_s ~ 1e10 and ~ 1e4), Float64 and Float32;
  * whole solves against the NumPy oracle's direct path, as tests/test_gpu_direct_kkt.py holds the LDL' route;
  * update_rho / update_matrices / adaptive rho: the new system is solved, the factorisation count follows;
  * the refusals (limits, row sharding, non-convex P, batch members on their own handles) and bitwise repeatability.

Bars.  Float64: the reference's own for direct solvers, 1e-10 relative (test/UnitTests/kktsolver.jl:40).  Float32: those of the LDL' route
(tests/test_gpu_direct_kkt.py), 1e-5 without equality rows and 1e-4 with them."""
import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from oracle import cosmo_oracle as O
from tests import schur_cases as S
from tests import util

pytestmark = pytest.mark.gpu
SCHUR = cj._ffi.KKT_SCHUR


def _ws(prob, kkt="qdldl", **kw):
    return O.Workspace(prob["P"], prob["q"], prob["A"], prob["b"], util.oracle_cones(prob["sets"]), O.Settings(kkt_solver=kkt, **kw))


def _handle(ws, dtype=np.float64, opts=None):
    """util.make_handle_from_workspace with set_schur_options in front of set_params"""
    h = cj.Handle(0, dtype=dtype)
    h.set_problem(ws.P, ws.q, ws.A, ws.b)
    bl = np.concatenate([c.l for c in ws.cones if c.kind == O.BOX] or [np.zeros(0)])
    bu = np.concatenate([c.u for c in ws.cones if c.kind == O.BOX] or [np.zeros(0)])
    h.set_cones([c.kind for c in ws.cones], [c.dim for c in ws.cones], bl, bu, cone_param=[c.alpha for c in ws.cones])
    st = ws.st
    p = h.default_params()
    p.kkt_kind = SCHUR
    p.sigma, p.alpha, p.rho = st.sigma, st.alpha, st.rho
    p.eps_abs, p.eps_rel = st.eps_abs, st.eps_rel
    p.rho_min, p.rho_max, p.rho_tol = st.RHO_MIN, st.RHO_MAX, st.RHO_TOL
    p.rho_eq_over_rho_ineq = st.RHO_EQ_OVER_RHO_INEQ
    p.adaptive_rho_tolerance = st.adaptive_rho_tolerance
    p.cosmo_infty_min_scaling = st.COSMO_INFTY * st.MIN_SCALING
    p.max_iter = st.max_iter
    p.adaptive_rho_max_adaptions = min(st.adaptive_rho_max_adaptions, 2 ** 62)
    p.check_termination = st.check_termination
    p.check_infeasibility = st.check_infeasibility
    p.adaptive_rho = 1 if st.adaptive_rho else 0
    p.adaptive_rho_interval = st.adaptive_rho_interval
    p.unscale_residuals = 1 if st.scaling != 0 else 0
    if opts:
        h.set_schur_options(**opts)
    h.set_params(p)
    h.set_scaling_full(ws.sm.D, ws.sm.Dinv, ws.sm.E, ws.sm.Einv, ws.sm.c, ws.sm.cinv)
    return h


def _kkt_dense(P, A, sigma, rho_vec):
    n = A.shape[1]
    return np.block([[P.toarray() + sigma * np.eye(n), A.toarray().T], [A.toarray(), -np.diag(1.0 / rho_vec)]])


def _rel_err(h, K, rhs, dtype):
    ref = np.linalg.solve(K, rhs)
    lhs, _ = h.kkt_solve(rhs.astype(dtype))
    return np.linalg.norm(lhs.astype(np.float64) - ref) / np.linalg.norm(ref), lhs, ref


# ---- the fine-grained solve against a dense solve -----------------------------------------------------------------------------------------
# axis 1: the block sides of M_s (with 17 long rows); axis 2: the number of long rows around the block side b = 64 of the dense factorisation
_B = S.NB
SIZE_CASES = {"side_1": (1,) * 9, "side_1_2_3": (1, 1, 2, 2, 3, 3), "side_4": (4, 4, 3, 1), "side_63": (63, 2, 1), "side_64": (64, 3, 1),
              "side_65": (65, 1, 1), "side_63_64_65": (63, 64, 65, 5), "side_block_max": (S.BLOCK_MAX, 3, 1)}
ND_CASES = [0, 1, 15, 16, 17, _B - 1, _B, _B + 1, 2 * _B + 5, 3 * _B]
SOLVE_CASES = [(name, sizes, 17) for name, sizes in SIZE_CASES.items()] + [("nd_%d" % nd, (1, 2, 3, 5, 40, 66), nd) for nd in ND_CASES]


@pytest.mark.parametrize("dtype,tol,zero_rows", [(np.float64, 1e-10, True), (np.float32, 1e-4, True), (np.float32, 1e-5, False)],
                         ids=["f64", "f32_equality_rows", "f32"])
@pytest.mark.parametrize("name,sizes,nd", SOLVE_CASES, ids=[c[0] for c in SOLVE_CASES])
def test_kkt_solve_matches_a_dense_solve(name, sizes, nd, dtype, tol, zero_rows):
    prob = S.build(sizes, nd, seed=7, zero_rows=zero_rows)
    assert prob["n"] <= 400
    ws = _ws(prob, scaling=0)
    h = _handle(ws, dtype)
    assert h.kkt_recurrence().startswith("schur")
    info = h.schur_info()
    want = S.components(ws.P, ws.A)
    assert (info["nd"], info["components"], info["largest"], info["sum_size2"]) == want[:4] == (nd, len(sizes), max(sizes), sum(s * s for s in sizes))
    rhs = np.random.default_rng(5).standard_normal(ws.n + ws.m)
    err, lhs, _ = _rel_err(h, _kkt_dense(ws.P, ws.A, ws.st.sigma, ws.rho_vec), rhs, dtype)
    print("schur kkt_solve %s %s: rel err %.3e, residual ratios %s, info %s" % (name, np.dtype(dtype).name, err, h.schur_residual(), info))
    assert err <= tol, err
    again, _ = h.kkt_solve(rhs.astype(dtype))
    assert np.array_equal(lhs, again)                              # reproducibility: same right-hand side, same factor, identical bits
    h2 = _handle(ws, dtype)
    other, _ = h2.kkt_solve(rhs.astype(dtype))
    assert np.array_equal(lhs, other)                              # ... and a second factorisation of the same problem gives the same bits


# ---- refinement and its safeguard --------------------------------------------------------------------------------------------------------------
def _p_zero_problem():
    # P = 0 and singleton rows on half of the variables only: the other directions see sigma = 1e-6 next to rho * 1e3 on the equality rows
    return S.build((1, 2, 3, 30, 70), 40, seed=11, p_zero=True, single_frac=0.5)


def test_refinement_lowers_the_residual_on_a_p_zero_problem():
    ws = _ws(_p_zero_problem(), scaling=0)
    K = _kkt_dense(ws.P, ws.A, ws.st.sigma, ws.rho_vec)
    rhs = np.random.default_rng(3).standard_normal(ws.n + ws.m)
    # M_s alone has condition 4e8 here (cond M = 3e4), and a NumPy model of the scheme (block inverses, explicit C^-1) gives residual ratios
    # 8e-4 -> 1.5e-5 -> 1.6e-8 -> 5e-11 -> 7e-14 with errors 6e-3 -> 1e-4 -> 1e-7 -> 4e-10 -> 5e-13 against the dense solve of the full system: the
    # bar of 1e-10 needs four steps on this problem, the default two must at least lower the residual
    h2 = _handle(ws)
    h2.kkt_solve(rhs)
    after2, before2 = h2.schur_residual()
    assert after2 < before2 and h2.schur_info()["refine_steps_taken"] >= 1
    h = _handle(ws, opts=dict(refine_steps=4))
    err, _, _ = _rel_err(h, K, rhs, np.float64)
    after, before = h.schur_residual()
    info = h.schur_info()
    print("schur refinement f64: err %.3e, residual ratio %.3e -> %.3e (two steps: %.3e), steps kept %d, rejected %d"
          % (err, before, after, after2, info["refine_steps_taken"], info["refine_steps_rejected"]))
    assert before == before2 and after < after2 and info["refine_steps_taken"] >= 3
    assert err <= 1e-10
    h0 = _handle(ws, opts=dict(refine_steps=0))
    h0.kkt_solve(rhs)
    a0, b0 = h0.schur_residual()
    assert a0 == b0 == before and h0.schur_info()["refine_steps_taken"] == 0


def test_the_safeguard_keeps_the_best_iterate_in_float32():
    """P = 0 in Float32 is outside what the solver can do ("Schur-complement KKT solver"): a documented limit, not a parity case.
    Where a block of M_s is covered by no singleton row it is sigma = 1e-6 away from singular next to entries of 1e2 .. 1e5, below Float32's resolution:
    the block's Cholesky meets a non-positive pivot and set-up refuses (INVALID).  Where every block is covered, refinement stalls at Float32's floor
    (a NumPy model in Float32: 4.5e-4 -> 1.6e-6 -> 1.8e-7 -> 1.5e-7 -> 1.3e-7 ...): the call returns, the safeguard never lets the residual grow, and x
    is the iterate whose residual is reported."""
    with pytest.raises(cj._ffi.CosmoHipError, match="non-positive pivot") as e:
        _handle(_ws(_p_zero_problem(), scaling=0), np.float32)
    assert e.value.code == 1
    ws = _ws(S.build((1, 2, 3, 30, 70), 40, seed=11, p_zero=True, single_frac=0.9), scaling=0)
    n, m = ws.n, ws.m
    rhs = np.random.default_rng(3).standard_normal(n + m)
    h = _handle(ws, np.float32, opts=dict(refine_steps=8))
    lhs, _ = h.kkt_solve(rhs.astype(np.float32))
    after, before = h.schur_residual()
    info = h.schur_info()
    assert np.all(np.isfinite(lhs))
    assert info["refine_steps_rejected"] >= 1 or after <= before
    assert after <= before
    # the residual of the returned x, recomputed on the host from the Float32 data the device holds
    A32 = ws.A.astype(np.float32).astype(np.float64); rho = ws.rho_vec.astype(np.float32).astype(np.float64)
    r32 = rhs.astype(np.float32).astype(np.float64)
    red = r32[:n] + A32.T @ (rho * r32[n:])
    x = lhs[:n].astype(np.float64)
    Mx = np.float64(np.float32(ws.st.sigma)) * x + A32.T @ (rho * (A32 @ x))
    host = np.linalg.norm(red - Mx) / np.linalg.norm(red)
    print("schur safeguard f32: residual ratio %.3e -> %.3e (host %.3e), steps kept %d, rejected %d" % (before, after, host, info["refine_steps_taken"], info["refine_steps_rejected"]))
    # the device's ratio is a Float32 evaluation of a residual near Float32's resolution of ||M|| ||x||: the two agree to that resolution
    floor = 2.0 ** -23 * np.sqrt(n) * np.linalg.norm(np.abs(A32.T) @ (rho * (np.abs(A32) @ np.abs(x)))) / np.linalg.norm(red)
    assert abs(host - after) <= 8 * floor + 1e-3 * after, (host, after, floor)


# ---- the loop against the oracle's direct path ----------------------------------------------------------------------------------------------------
def _loop_cases():
    return [("mixed", S.build((1, 2, 3, 20, 34), 12, seed=21), dict(max_iter=4000)),
            ("rho_updates", S.build((1, 1, 2, 3, 30, 43), 70, seed=22), dict(max_iter=4000, rho=1e-4, adaptive_rho_interval=10)),
            ("block_diagonal", S.build((2, 3, 25, 30), 0, seed=23), dict(max_iter=4000))]


@pytest.mark.parametrize("name,prob,kw", _loop_cases(), ids=[c[0] for c in _loop_cases()])
def test_loop_equals_the_oracles_direct_path(name, prob, kw):
    ws = _ws(prob, **kw)
    h = _handle(ws)
    h.set_iterates(None, None, None)
    ref = ws.optimize()
    r = h.optimize()
    assert cj._ffi.STATUS_NAMES[r.status] == ref.status and r.iter == ref.iter
    got = [r.rho_updates[i] for i in range(r.n_rho_updates)]
    assert np.allclose(got, ref.rho_updates, rtol=1e-9, atol=0)
    w, w_prev, s, mu = h.get_iterates()
    scale = max(np.max(np.abs(ref.w)), 1e-300)
    devs = [np.max(np.abs(w - ref.w)) / scale] + [np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1.0) for a, b in ((s, ref.s_scaled), (mu, ref.mu_scaled))]
    print("schur loop %s: status %s, %d iterations, %d rho updates, deviations %s" % (name, ref.status, r.iter, r.n_rho_updates, devs))
    assert max(devs) <= 1e-8
    assert r.kkt_iters_total == 0                                   # no Krylov iterations
    assert h.schur_info()["factorizations"] == 1 + (r.n_rho_updates - 1)      # the set-up one, then one per entry rho_updates gained
    if name == "rho_updates":
        assert r.n_rho_updates >= 3, "this case must refactorise inside the loop more than once"


def _simple_constraints():
    A = np.array([[1.0, 1], [1, 0], [0, 1]])
    l = np.array([1.0, 0, 0]); u = np.array([1.0, 0.7, 0.7])
    return [cj.Constraint(-A, u, cj.Nonnegatives), cj.Constraint(A, -l, cj.Nonnegatives)]


def test_simple_qp_golden_of_the_reference():
    md = cj.Model()
    cj.assemble(md, np.array([[4.0, 1], [1, 2]]), np.array([1.0, 1]), _simple_constraints(), settings=cj.Settings(kkt_solver=cj.SchurComplementKKTSolver))
    res = cj.optimize(md)
    assert res.status == "Solved"                                             # test/UnitTests/simple.jl:45-47
    assert np.linalg.norm(res.x - np.array([0.3, 0.7])) < 1e-3
    assert abs(res.obj_val - 1.8800000298331538) < 1e-3
    A, b, cones = O.assemble([O.Constraint(c.A, c.b, O.Nonnegatives(3)) for c in _simple_constraints()])
    ref = O.solve(np.array([[4.0, 1], [1, 2]]), np.array([1.0, 1]), A, b, cones, O.Settings(kkt_solver="qdldl"))
    assert res.status == ref.status and res.iter == ref.iter
    assert np.allclose(res.info.rho_updates, ref.rho_updates, rtol=1e-9, atol=0)
    for a, r in ((res.x, ref.x), (res.y, ref.y), (res.s, ref.s)):
        assert np.max(np.abs(a - r)) <= 1e-8 * max(np.max(np.abs(r)), 1.0)
    assert res.info.schur["components"] == 1 and res.info.schur["factorizations"] == len(res.info.rho_updates)


def test_chordal_sdp_with_decomposition_against_the_oracle():
    from tests.test_chordal_host import _equivalence_problem          # the reference's chordal_decomposition_triangle.jl problem (P = 0)
    A, b, q, kinds, dims = _equivalence_problem(144545)
    sets = [{cj._ffi.PSD_TRIANGLE: cj.PsdConeTriangle, cj._ffi.ZERO: cj.ZeroSet, cj._ffi.NONNEG: cj.Nonnegatives}[k](d) for k, d in zip(kinds, dims)]
    md = cj.Model()
    md.set(sp.csc_matrix((1, 1)), q, A, b, sets, cj.Settings(kkt_solver=cj.with_options(cj.SchurComplementKKTSolver, refine_steps=3), decompose=True,
                                                             merge_strategy=cj.NoMerge, max_iter=5000))
    cj.model._chordal_decomposition(md)
    Pd, qd, Ad, bd, cones = md.P.copy(), md.q.copy(), md.A.copy(), md.b.copy(), util.oracle_cones(md.sets)
    res = cj.optimize(md)
    ref = O.solve(Pd, qd, Ad, bd, cones, O.Settings(kkt_solver="qdldl", max_iter=5000))
    print("schur chordal: %s after %d (oracle %d), plan %s" % (res.status, res.iter, ref.iter, res.info.schur))
    assert res.status == ref.status == "Solved" and res.iter == ref.iter
    assert np.allclose(res.info.rho_updates, ref.rho_updates, rtol=1e-8, atol=0)       # (the LDL' route's bar on this P = 0 problem, test_gpu_direct_kkt.py)
    assert np.max(np.abs(res.x - ref.x[:res.x.size])) <= 1e-8 * max(np.max(np.abs(ref.x)), 1.0)
    assert abs(res.obj_val - ref.obj_val) <= 1e-8 * (1 + abs(ref.obj_val))


# ---- rho changes and value updates ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 1e-4)], ids=["f64", "f32"])
def test_update_rho_and_update_matrices_solve_the_new_system(dtype, tol):
    prob = S.build((1, 2, 3, 10, 70), 70, seed=31)
    ws = _ws(prob, scaling=0)
    h = _handle(ws, dtype)
    n, m = ws.n, ws.m
    rng = np.random.default_rng(9)
    rhs = rng.standard_normal(n + m)
    assert h.schur_info()["factorizations"] == 1
    rho = rng.uniform(0.05, 20.0, m)
    h.update_rho(rho.astype(dtype))
    assert h.schur_info()["factorizations"] == 2
    err, _, _ = _rel_err(h, _kkt_dense(ws.P, ws.A, ws.st.sigma, rho), rhs, dtype)
    print("schur update_rho %s: %.3e" % (np.dtype(dtype).name, err))
    assert err <= tol
    P2 = ws.P.copy(); P2.data = P2.data * 1.5                      # same pattern, still convex (a positive multiple)
    A2 = ws.A.copy(); A2.data = A2.data * rng.uniform(0.5, 1.5, A2.nnz)
    h.update_matrices(P2.data, A2.data)
    assert h.schur_info()["factorizations"] == 3
    err, _, _ = _rel_err(h, _kkt_dense(P2, A2, ws.st.sigma, rho), rhs, dtype)
    print("schur update_matrices %s: %.3e" % (np.dtype(dtype).name, err))
    assert err <= tol


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_with_the_sizes_in_the_message():
    ws = _ws(S.build((1, 2, 3, 20), 9, seed=41), scaling=0)
    with pytest.raises(cj._ffi.CosmoHipError, match=r"9 rows .* nd_max = 8") as e:
        _handle(ws, opts=dict(nd_max=8))
    assert e.value.code == 6                                # COSMO_HIP_ERR_UNSUPPORTED
    with pytest.raises(cj._ffi.CosmoHipError, match=r"side 20, more than block_max = 19") as e:
        _handle(ws, opts=dict(block_max=19))
    assert e.value.code == 6
    _handle(ws, opts=dict(nd_max=9, block_max=20))          # exactly at the limits: accepted
    big = _ws(S.build((S.BLOCK_MAX + 1, 2), 3, seed=42), scaling=0)
    with pytest.raises(cj._ffi.CosmoHipError, match=r"side 257") as e:
        _handle(big)
    assert e.value.code == 6


def test_row_sharding_is_refused():
    ws = _ws(S.build((1, 2, 3, 20), 9, seed=43), scaling=0)
    h = _handle(ws)
    with pytest.raises(cj._ffi.CosmoHipError) as e:
        h.set_row_shard([0, len(ws.cones)])
    assert e.value.code == 6


def test_nonconvex_objective_is_refused_at_setup():
    prob = S.build((1, 2, 3, 20), 9, seed=44)
    P = prob["P"].tolil(); P[0, 0] = -1e4; prob["P"] = P.tocsc()           # below -(sigma + A_s' rho A_s): a negative pivot in a block of M_s
    ws = O.Workspace(prob["P"], prob["q"], prob["A"], prob["b"], util.oracle_cones(prob["sets"]), O.Settings(kkt_solver="cg", scaling=0))
    with pytest.raises(cj._ffi.CosmoHipError, match="not convex") as e:
        _handle(ws)
    assert e.value.code == 1                                # COSMO_HIP_ERR_INVALID


def test_optimize_batch_runs_such_members_on_their_own_handles():
    probs = [S.build((1, 2, 3, 20, 30), 12, seed=51), S.build((2, 3, 40), 20, seed=52)]
    kkt = cj.with_options(cj.SchurComplementKKTSolver, refine_steps=1)

    def models():
        out = []
        for pr in probs:
            md = cj.Model()
            md.set(pr["P"], pr["q"], pr["A"], pr["b"], pr["sets"], cj.Settings(kkt_solver=kkt, max_iter=4000))
            out.append(md)
        return out
    batch = cj.optimize_batch(models())
    assert cj.model.LAST_BATCH_INFO["own_handle_members"] == 2
    for md, rb in zip(models(), batch):
        r1 = cj.optimize(md)
        assert rb.status == r1.status == "Solved" and rb.iter == r1.iter
        assert np.array_equal(rb.x, r1.x) and np.array_equal(rb.y, r1.y)
