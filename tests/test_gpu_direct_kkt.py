"""The direct KKT solver on the device (kkt_kind KKT_DIRECT, csrc/ldl.hip): QdldlKKTSolver (src/linear_solver/kktsolver.jl:285-320).

  * one solve! against a dense solve of the same quasi-definite system (the reference's bars, test/UnitTests/kktsolver.jl:40), after update_rho!
    with a non-uniform rho, and bitwise repeatability;
  * whole solves against the NumPy oracle's direct path (kkt_solver="qdldl": exact LDL' solves, refactorised at every rho update);
  * the inertia check ("Objective function is not convex."), the refusal of row sharding, the Float32 library.

Structural coverage (supernodes wider / taller than the workgroup, thousands of descendants or levels, N > 4096 * 256, missing diagonals, P = 0,
m = 0, empty lines) against a derived backward-error bound: tests/test_gpu_ldl_structures.py."""
import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from oracle import cosmo_oracle as O
from tests import util

pytestmark = pytest.mark.gpu


def _prob(seed, n=60, **kw):
    rng = np.random.default_rng(seed)
    args = dict(soc_dims=(5, 7), psd_tri_dims=(3,), p_shift=1.0)
    args.update(kw)
    return util.random_qp(rng, n, 5, 40, 30, **args)


def _ws(prob, kkt="qdldl", **kw):
    return O.Workspace(prob["P"], prob["q"], prob["A"], prob["b"], util.oracle_cones(prob["sets"]), O.Settings(kkt_solver=kkt, **kw))


def _kkt_dense(ws, rho_vec):
    n, m = ws.n, ws.m
    P = ws.P.toarray(); A = ws.A.toarray()
    Pu = np.triu(P); Ps = Pu + np.triu(Pu, 1).T                 # assemble_kkt_triangle(:U): the upper triangle of P
    return np.block([[Ps + ws.st.sigma * np.eye(n), A.T], [A, -np.diag(1.0 / rho_vec)]])


# The reference's bars (test/UnitTests/kktsolver.jl:40) are 1e-10 (Float64) and 1e-5 (Float32).  Equality rows carry rho 1e3 times larger, and
# -1/rho_eq next to sigma = 1e-6 costs Float32 about a digit (Float32 note): the Float32 case WITH equality rows is held to a
# looser, documented 1e-4 (measured 1.3e-5 on this problem), the one without them to the reference's bar.
@pytest.mark.parametrize("dtype,tol,m_zero", [(np.float64, 1e-10, 0), (np.float64, 1e-10, 5), (np.float32, 1e-5, 0), (np.float32, 1e-4, 5)],
                         ids=["f64", "f64_equality_rows", "f32", "f32_equality_rows"])
def test_kkt_solve_matches_a_dense_solve(dtype, tol, m_zero):
    if m_zero:
        prob = _prob(11)
    else:
        prob = util.random_qp(np.random.default_rng(11), 60, 0, 40, 30, soc_dims=(5, 7), psd_tri_dims=(3,), p_shift=5.0)
    ws = _ws(prob, scaling=0)
    h = util.make_handle_from_workspace(ws, kkt_kind=cj._ffi.KKT_DIRECT, dtype=dtype)
    assert h.kkt_recurrence().startswith("direct")
    n, m = ws.n, ws.m
    rng = np.random.default_rng(5)
    rhs = rng.standard_normal(n + m)
    rho = ws.rho_vec.copy()
    for rnd in range(2):
        K = _kkt_dense(ws, rho)
        ref = np.linalg.solve(K, rhs)
        lhs, _ = h.kkt_solve(rhs.astype(dtype))
        err = np.linalg.norm(lhs.astype(np.float64) - ref) / np.linalg.norm(ref)
        assert err <= tol, (rnd, err)
        again, _ = h.kkt_solve(rhs.astype(dtype))
        assert np.array_equal(lhs, again)                      # same right-hand side, same factor: bitwise identical
        rho = rng.uniform(0.05, 20.0, m)                       # non-uniform rho: update_rho! refactorises
        h.update_rho(rho.astype(dtype))
    info = h.direct_info()
    assert info["factorizations"] == 3 and info["positive_pivots"] == n and info["nnz_L"] > 0     # setup + two update_rho


def test_user_permutation_gives_the_same_solution():
    prob = _prob(12)
    ws = _ws(prob, scaling=0)
    h1 = util.make_handle_from_workspace(ws, kkt_kind=cj._ffi.KKT_DIRECT)
    rhs = np.random.default_rng(1).standard_normal(ws.n + ws.m)
    a, _ = h1.kkt_solve(rhs)
    h2 = cj.Handle(0)
    h2.set_problem(ws.P, ws.q, ws.A, ws.b)
    h2.set_kkt_perm(np.arange(ws.n + ws.m)[::-1].copy())
    with pytest.raises(cj._ffi.CosmoHipError):
        h2.set_kkt_perm(np.zeros(ws.n + ws.m, np.int64))
    h2.set_kkt_perm(np.arange(ws.n + ws.m)[::-1].copy())
    bl = np.concatenate([c.l for c in ws.cones if c.kind == O.BOX] or [np.zeros(0)])
    bu = np.concatenate([c.u for c in ws.cones if c.kind == O.BOX] or [np.zeros(0)])
    h2.set_cones([c.kind for c in ws.cones], [c.dim for c in ws.cones], bl, bu, cone_param=[c.alpha for c in ws.cones])
    p = h2.default_params(); p.kkt_kind = cj._ffi.KKT_DIRECT; p.sigma, p.rho = ws.st.sigma, ws.st.rho
    h2.set_params(p)
    b, _ = h2.kkt_solve(rhs)
    assert np.linalg.norm(a - b) <= 1e-10 * np.linalg.norm(a)


def _loop_cases():
    return [("qp_mixed", _prob(21), dict(max_iter=4000)),
            ("qp_rho_updates", _prob(22, n=80, p_shift=0.05), dict(max_iter=4000, rho=1e-4, adaptive_rho_interval=10)),
            ("qp_psd", _prob(23, psd_tri_dims=(6, 10)), dict(max_iter=4000))]


@pytest.mark.parametrize("name,prob,kw", _loop_cases(), ids=[c[0] for c in _loop_cases()])
def test_loop_equals_the_oracles_direct_path(name, prob, kw):
    ws = _ws(prob, **kw)
    h = util.make_handle_from_workspace(ws, kkt_kind=cj._ffi.KKT_DIRECT)
    h.set_iterates(None, None, None)
    ref = ws.optimize()
    r = h.optimize()
    assert cj._ffi.STATUS_NAMES[r.status] == ref.status and r.iter == ref.iter
    got = [r.rho_updates[i] for i in range(r.n_rho_updates)]
    assert np.allclose(got, ref.rho_updates, rtol=1e-9, atol=0)
    w, w_prev, s, mu = h.get_iterates()
    scale = max(np.max(np.abs(ref.w)), 1e-300)
    assert np.max(np.abs(w - ref.w)) <= 1e-8 * scale
    for a, b in ((s, ref.s_scaled), (mu, ref.mu_scaled)):          # s and the dual iterate (y = mu after unscaling)
        assert np.max(np.abs(a - b)) <= 1e-8 * max(np.max(np.abs(b)), 1.0)
    if name == "qp_rho_updates":
        assert r.n_rho_updates >= 3, "this case must refactorise inside the loop more than once"
        assert h.direct_info()["factorizations"] == 1 + (r.n_rho_updates - 1)


def _simple_constraints():
    A = np.array([[1.0, 1], [1, 0], [0, 1]])
    l = np.array([1.0, 0, 0]); u = np.array([1.0, 0.7, 0.7])
    return [cj.Constraint(-A, u, cj.Nonnegatives), cj.Constraint(A, -l, cj.Nonnegatives)]


def _simple_model(dtype=np.float64, **kw):
    md = cj.Model(dtype=dtype) if dtype is not np.float64 else cj.Model()
    cj.assemble(md, np.array([[4.0, 1], [1, 2]]), np.array([1.0, 1]), _simple_constraints(), settings=cj.Settings(kkt_solver=cj.QdldlKKTSolver, **kw))
    return md


def test_simple_qp_golden_with_the_default_solver_of_the_reference():
    res = cj.optimize(_simple_model())
    assert res.status == "Solved"                                             # test/UnitTests/simple.jl:45-47
    assert np.linalg.norm(res.x - np.array([0.3, 0.7])) < 1e-3
    assert abs(res.obj_val - 1.8800000298331538) < 1e-3
    A, b, cones = O.assemble([O.Constraint(c.A, c.b, O.Nonnegatives(3)) for c in _simple_constraints()])
    ref = O.solve(np.array([[4.0, 1], [1, 2]]), np.array([1.0, 1]), A, b, cones, O.Settings(kkt_solver="qdldl"))
    assert res.status == ref.status and res.iter == ref.iter
    assert np.allclose(res.info.rho_updates, ref.rho_updates, rtol=1e-9, atol=0)
    for a, r in ((res.x, ref.x), (res.y, ref.y), (res.s, ref.s)):
        assert np.max(np.abs(a - r)) <= 1e-8 * max(np.max(np.abs(r)), 1.0)


def test_model_level_random_qp_against_the_oracle():
    prob = _prob(31, n=70)
    ref = O.solve(prob["P"], prob["q"], prob["A"], prob["b"], util.oracle_cones(prob["sets"]), O.Settings(kkt_solver="qdldl", max_iter=4000))
    md = cj.Model()
    md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], cj.Settings(kkt_solver=cj.QdldlKKTSolver, max_iter=4000))
    res = cj.optimize(md)
    assert res.status == ref.status == "Solved" and res.iter == ref.iter
    assert np.allclose(res.info.rho_updates, ref.rho_updates, rtol=1e-9, atol=0)
    for a, r in ((res.x, ref.x), (res.y, ref.y), (res.s, ref.s)):
        assert np.max(np.abs(a - r)) <= 1e-8 * max(np.max(np.abs(r)), 1.0)


def test_chordal_sdp_with_decomposition_against_the_oracle():
    """decompose=True: the decomposed problem (what chordal_decomposition! hands to the loop) is solved by the oracle's direct path too."""
    from tests.test_chordal_host import _equivalence_problem          # the reference's chordal_decomposition_triangle.jl problem (P = 0)
    A, b, q, kinds, dims = _equivalence_problem(144545)
    sets = [{cj._ffi.PSD_TRIANGLE: cj.PsdConeTriangle, cj._ffi.ZERO: cj.ZeroSet, cj._ffi.NONNEG: cj.Nonnegatives}[k](d) for k, d in zip(kinds, dims)]
    md = cj.Model()
    md.set(sp.csc_matrix((1, 1)), q, A, b, sets, cj.Settings(kkt_solver=cj.QdldlKKTSolver, decompose=True, merge_strategy=cj.NoMerge, max_iter=5000))
    n0 = md.n
    cj.model._chordal_decomposition(md)                     # the first step of optimize() on a fresh model (src/solver.jl:88-94)
    assert md.chordal is not None and md.n > n0
    Pd, qd, Ad, bd, cones = md.P.copy(), md.q.copy(), md.A.copy(), md.b.copy(), util.oracle_cones(md.sets)
    res = cj.optimize(md)
    ref = O.solve(Pd, qd, Ad, bd, cones, O.Settings(kkt_solver="qdldl", max_iter=5000))
    assert res.status == ref.status == "Solved" and res.iter == ref.iter
    # (P = 0 and PSD projections on both sides: the new rho, a square root of residual ratios, agrees to 1.4e-9 here -- held to the 1e-8 bar of x)
    assert np.allclose(res.info.rho_updates, ref.rho_updates, rtol=1e-8, atol=0)
    assert np.max(np.abs(res.x - ref.x[:res.x.size])) <= 1e-8 * max(np.max(np.abs(ref.x)), 1.0)
    assert abs(res.obj_val - ref.obj_val) <= 1e-8 * (1 + abs(ref.obj_val))


def test_optimize_batch_of_mixed_models_equals_optimize():
    probs = [_prob(41, n=50), _prob(42, n=65, psd_tri_dims=(4,))]
    def models():
        out = []
        for pr in probs:
            md = cj.Model()
            md.set(pr["P"], pr["q"], pr["A"], pr["b"], pr["sets"], cj.Settings(kkt_solver=cj.QdldlKKTSolver, max_iter=4000))
            out.append(md)
        return out
    batch = cj.optimize_batch(models())
    for md, rb in zip(models(), batch):
        r1 = cj.optimize(md)
        assert rb.status == r1.status == "Solved" and rb.iter == r1.iter
        assert np.array_equal(rb.x, r1.x) and np.array_equal(rb.y, r1.y)


def test_nonconvex_objective_is_refused_at_setup():
    prob = _prob(51, n=30)
    P = prob["P"].toarray()
    P[0, 0] = -5.0                                          # a negative eigenvalue
    P = sp.csc_matrix(P)
    ws = O.Workspace(P, prob["q"], prob["A"], prob["b"], util.oracle_cones(prob["sets"]), O.Settings(kkt_solver="cg", scaling=0))
    h = cj.Handle(0)
    h.set_problem(ws.P, ws.q, ws.A, ws.b)
    bl = np.concatenate([c.l for c in ws.cones if c.kind == O.BOX] or [np.zeros(0)])
    bu = np.concatenate([c.u for c in ws.cones if c.kind == O.BOX] or [np.zeros(0)])
    h.set_cones([c.kind for c in ws.cones], [c.dim for c in ws.cones], bl, bu, cone_param=[c.alpha for c in ws.cones])
    p = h.default_params(); p.kkt_kind = cj._ffi.KKT_DIRECT
    with pytest.raises(cj._ffi.CosmoHipError, match="Objective function is not convex."):
        h.set_params(p)
    assert h.direct_info()["positive_pivots"] < ws.n
    with pytest.raises(cj._ffi.CosmoHipError):              # the refused factor is not usable: no solve, no loop until set_params succeeds
        h.kkt_solve(np.ones(ws.n + ws.m))
    with pytest.raises(cj._ffi.CosmoHipError):
        h.set_iterates(None, None, None)
    md = cj.Model()
    with pytest.raises(cj._ffi.CosmoHipError, match="Objective function is not convex."):
        md.set(P, prob["q"], prob["A"], prob["b"], prob["sets"], cj.Settings(kkt_solver=cj.QdldlKKTSolver))
        cj.optimize(md)


def test_row_sharding_is_refused():
    prob = _prob(61, n=30)
    ws = _ws(prob, scaling=0)
    h = util.make_handle_from_workspace(ws, kkt_kind=cj._ffi.KKT_DIRECT)
    with pytest.raises(cj._ffi.CosmoHipError) as e:
        h.set_row_shard([0, len(ws.cones)])
    assert e.value.code == 6                                # COSMO_HIP_ERR_UNSUPPORTED

    class _Dist:                                           # a two-rank run: refused before any sharding is set up
        def get_world_size(self):
            return 2

        def get_rank(self):
            return 0
    md = cj.Model()
    md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], cj.Settings(kkt_solver=cj.QdldlKKTSolver))
    with pytest.raises(NotImplementedError):
        cj.optimize(md, dist=_Dist())


def test_float32_library_solves_the_simple_qp():
    md = _simple_model(dtype=np.float32, eps_abs=1e-4, eps_rel=1e-4)
    res = cj.optimize(md)
    assert md.handle.dtype == np.float32 and res.status == "Solved"
    assert np.linalg.norm(res.x - np.array([0.3, 0.7])) < 1e-3
