"""The direct KKT solver in batch mode (Settings.direct_batch, csrc/batch_ldl.hip): QdldlKKTSolver (src/linear_solver/kktsolver.jl:285-320) inside the
persistent batch kernels -- one analysis of the union of the members' patterns, one LDL' factor per member, refactorised by the member's own workgroup
when its rho changes.

  * members of one pattern and of different patterns against the NumPy oracle's direct path (the bars of test_gpu_direct_kkt.py's loop test) and
    against the single-problem DIRECT handle;
  * the factorisation count of every member against its rho updates, certificates, the inertia check, the accelerator, Float32, groups and the
    reference's portfolio example as a batch over the risk aversion."""
import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from oracle import cosmo_oracle as O
from tests import infeasible_instances as INF
from tests import util

pytestmark = pytest.mark.gpu


def _family(seed, count, n=40, p_shift=1.0, q_spread=0.0):
    """`count` members of ONE sparsity pattern: a random_qp with Zero, Nonnegatives, Box, SOC and PSD-triangle(3) cones whose rows are scaled per cone
    block (per row for Zero / Nonnegatives / Box, with the Box bounds; per cone for SOC / PSD) and whose q is redrawn -- varied q, b and values of A,
    every member feasible."""
    base = util.random_qp(np.random.default_rng(seed), n, 4, 20, 10, soc_dims=(5,), psd_tri_dims=(3,), p_shift=p_shift)
    rng = np.random.default_rng(seed + 1000)
    out = []
    for j in range(count):
        d, sets, off = [], [], 0
        for K in base["sets"]:
            if K.kind in (cj._ffi.ZERO, cj._ffi.NONNEG, cj._ffi.BOX):
                f = rng.uniform(0.5, 2.0, K.dim)
            else:
                f = np.full(K.dim, rng.uniform(0.5, 2.0))
            d.append(f)
            sets.append(cj.Box(K.l * f, K.u * f) if K.kind == cj._ffi.BOX else type(K)(K.dim))
            off += K.dim
        Dm = sp.diags(np.concatenate(d))
        q = rng.standard_normal(n) * (10.0 ** (q_spread * (j / max(count - 1, 1)) - q_spread / 2))
        out.append(dict(P=base["P"], q=q, A=(Dm @ base["A"]).tocsc(), b=Dm @ base["b"], sets=sets))
    return out


def _models(probs, st, dtype=np.float64):
    out = []
    for p in probs:
        md = cj.Model(dtype=dtype) if dtype is not np.float64 else cj.Model()
        md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st)
        out.append(md)
    return out


def _oracle(p, **kw):
    return O.solve(p["P"], p["q"], p["A"], p["b"], util.oracle_cones(p["sets"]), O.Settings(kkt_solver="qdldl", **kw))


def _close(a, b, tol):
    return np.max(np.abs(a - b)) <= tol * max(np.max(np.abs(b)), 1.0)


def _against_oracle(probs, res, rho_rtol=1e-9, **kw):
    for k, (p, r) in enumerate(zip(probs, res)):
        ref = _oracle(p, **kw)
        assert r.status == ref.status and r.iter == ref.iter, (k, r.status, ref.status, r.iter, ref.iter)
        assert np.allclose(r.info.rho_updates, ref.rho_updates, rtol=rho_rtol, atol=0), (k, r.info.rho_updates, ref.rho_updates)
        for a, b in ((r.x, ref.x), (r.s, ref.s), (r.y, ref.y)):
            assert _close(a, b, 1e-8), k
        assert abs(r.obj_val - ref.obj_val) <= 1e-8 * max(abs(ref.obj_val), 1.0), k


DIRECT = dict(kkt_solver=cj.QdldlKKTSolver, direct_batch=True, max_iter=4000)


def test_same_pattern_batch_against_the_oracles_direct_path_and_the_single_handle():
    probs = _family(101, 32)
    st = cj.Settings(**DIRECT)
    res = cj.optimize_batch(_models(probs, st))
    info = cj.model.LAST_BATCH_INFO
    assert not info["mixed"] and "direct_info" in info                     # the DIRECT form of the batch kernels ran, not own handles
    di = info["direct_info"]
    assert di["factorizations"] >= len(probs) and di["min_positive_pivots"] == probs[0]["P"].shape[0] and di["supernodes"] > 0
    assert sum(r.status == "Solved" for r in res) >= len(probs) - 2
    _against_oracle(probs, res, max_iter=4000)
    for p, r in zip(probs[:12], res):                                        # the single-problem DIRECT handle (csrc/ldl.hip)
        md = _models([p], cj.Settings(kkt_solver=cj.QdldlKKTSolver, max_iter=4000))[0]
        r1 = cj.optimize(md)
        assert r.status == r1.status and r.iter == r1.iter
        assert _close(r.x, r1.x, 1e-9) and _close(r.y, r1.y, 1e-9)


def test_every_member_refactorises_on_its_own_rho_updates():
    probs = _family(202, 12, n=50, p_shift=0.05, q_spread=4.0)
    st = cj.Settings(rho=1e-4, adaptive_rho_interval=10, **DIRECT)
    B, _ = cj.model.prepare_batch(_models(probs, st), 0)
    rs = B.optimize()
    counts = B.direct_counts()
    B.close()
    lens = [r.n_rho_updates for r in rs]
    assert list(counts) == lens                                             # the set-up factorisation + one per rho update of THAT member
    assert max(lens) >= 4 and len(set(lens)) > 1, lens                      # at least three in-loop refactorisations; members differ
    res = cj.optimize_batch(_models(probs, st))
    _against_oracle(probs, res, max_iter=4000, rho=1e-4, adaptive_rho_interval=10)


def test_union_analysis_of_members_with_different_patterns():
    n = 40
    probs = [util.random_qp(np.random.default_rng(300 + j), n, 4, 20, 10, soc_dims=(5,), psd_tri_dims=(3,), p_shift=1.0) for j in range(6)]
    assert len({tuple(p["A"].indices) for p in probs}) == len(probs)
    st = cj.Settings(**DIRECT)
    res = cj.optimize_batch(_models(probs, st))
    di = cj.model.LAST_BATCH_INFO["direct_info"]
    # the batch's fill is that of one analysis of the union of the patterns (upper triangle of P, A)
    Pu = sum(sp.triu(abs(p["P"])) for p in probs).tocsc(); Au = sum(abs(p["A"]) for p in probs).tocsc()
    Pu.sort_indices(); Au.sort_indices()
    ref = cj._ffi.ldl_analyze(n, Au.shape[0], Pu, Au)
    assert di["nnz_L"] == ref["nnz_L"] and di["supernodes"] == ref["supernodes"]
    # (the union's ordering is not the one the oracle picks for a member's own pattern: the solves round differently, and the new rho, a square root of
    #  a ratio of residuals of ~1e-7, carries that difference at ~5e-8 -- measured 4.6e-8 on member 4; iterates and objective keep the 1e-8 bar)
    _against_oracle(probs, res, rho_rtol=1e-7, max_iter=4000)


def _inf_model(P, q, cons, st):
    sets = {INF.ZERO: cj.ZeroSet, INF.NONNEG: cj.Nonnegatives, INF.SOC: cj.SecondOrderCone, INF.PSD_SQUARE: cj.PsdCone}
    md = cj.Model()
    cj.assemble(md, P, q, [cj.Constraint(A, b, sets[k]) for (A, b, k, d) in cons], settings=st)
    return md


def test_certificates_in_a_mixed_batch():
    st = cj.Settings(**DIRECT)
    cases = [INF.primal_infeasible_1(3), INF.dual_infeasible_1(4), INF.primal_infeasible_1(5), INF.dual_infeasible_1(6)]
    feas = _family(401, 2)
    mods = [_inf_model(P, q, c, st) for P, q, c in cases] + _models(feas, st)
    res = cj.optimize_batch(mods)
    assert cj.model.LAST_BATCH_INFO["own_handle_members"] == 0
    singles = [cj.optimize(_inf_model(P, q, c, cj.Settings(kkt_solver=cj.QdldlKKTSolver, max_iter=4000))) for P, q, c in cases]
    singles += [cj.optimize(md) for md in _models(feas, cj.Settings(kkt_solver=cj.QdldlKKTSolver, max_iter=4000))]
    assert [r.status for r in res] == [r.status for r in singles]
    assert [r.status for r in res[:4]] == ["Primal_infeasible", "Dual_infeasible", "Primal_infeasible", "Dual_infeasible"]


def test_nonconvex_member_is_refused_at_setup():
    probs = _family(501, 4)
    P = probs[2]["P"].toarray(); P[0, 0] = -5.0
    probs[2] = dict(probs[2], P=sp.csc_matrix(P))
    mods = _models(probs, cj.Settings(**DIRECT))
    with pytest.raises(cj._ffi.CosmoHipError, match=r"Objective function is not convex\. \(member 2\)"):
        cj.optimize_batch(mods)
    assert not any(md.is_optimized for md in mods)


def test_anderson_accelerator_matches_the_single_direct_handle():
    probs = _family(601, 8)
    st = cj.Settings(accelerator=cj.AndersonAccelerator, **DIRECT)
    res = cj.optimize_batch(_models(probs, st))
    assert "direct_info" in cj.model.LAST_BATCH_INFO
    for p, r in zip(probs, res):
        r1 = cj.optimize(_models([p], cj.Settings(accelerator=cj.AndersonAccelerator, kkt_solver=cj.QdldlKKTSolver, max_iter=4000))[0])
        assert r.status == r1.status == "Solved" and abs(r.iter - r1.iter) <= 25, (r.iter, r1.iter)
        assert _close(r.x, r1.x, 1e-6) and _close(r.y, r1.y, 1e-6)


def test_float32_library():
    A = np.array([[1.0, 1], [1, 0], [0, 1]])
    l = np.array([1.0, 0, 0]); u = np.array([1.0, 0.7, 0.7])
    st = cj.Settings(eps_abs=1e-4, eps_rel=1e-4, **DIRECT)
    mods = []
    for _ in range(4):
        md = cj.Model(dtype=np.float32)
        cj.assemble(md, np.array([[4.0, 1], [1, 2]]), np.array([1.0, 1]), [cj.Constraint(-A, u, cj.Nonnegatives), cj.Constraint(A, -l, cj.Nonnegatives)], settings=st)
        mods.append(md)
    for r in cj.optimize_batch(mods):                                          # test/UnitTests/simple.jl:45-47
        assert r.status == "Solved" and np.linalg.norm(r.x - np.array([0.3, 0.7])) < 1e-3
    # random QPs without equality rows (Float32 note) against the oracle: the ADMM tolerance (1e-4) bounds the agreement, not the solves
    probs = [util.random_qp(np.random.default_rng(700 + j), 30, 0, 30, 0, soc_dims=(4,), p_shift=2.0) for j in range(8)]
    res = cj.optimize_batch(_models(probs, st, np.float32))
    for p, r in zip(probs, res):
        ref = _oracle(p)
        assert r.status == ref.status == "Solved"
        assert abs(r.obj_val - ref.obj_val) <= 1e-3 * max(abs(ref.obj_val), 1.0)


def test_groups_run_every_class_on_the_direct_batch_form():
    probs = _family(801, 3) + _family(802, 3, n=55)
    st = cj.Settings(**DIRECT)
    res = cj.optimize_batch(_models(probs, st))
    info = cj.model.LAST_BATCH_INFO
    assert info["mixed"] and info["own_handle_members"] == 0
    G, _ = cj.model.prepare_batch_group(_models(probs, st), 0)
    _, _, modes = G.class_info(with_modes=True)
    G.close()
    assert list(modes) == [0] * len(probs)
    for p, r in zip(probs, res):
        r1 = cj.optimize(_models([p], cj.Settings(kkt_solver=cj.QdldlKKTSolver, max_iter=4000))[0])
        assert r.status == r1.status and r.iter == r1.iter
        assert _close(r.x, r1.x, 1e-9) and _close(r.y, r1.y, 1e-9)
    G, _ = cj.model.prepare_batch_group(_models(probs, cj.Settings(kkt_solver=cj.QdldlKKTSolver, max_iter=4000)), 0)
    _, _, modes = G.class_info(with_modes=True)
    G.close()
    assert list(modes) == [1] * len(probs)                                 # without the switch: one own handle per member, as before


def portfolio_batch(count=256):
    """examples/portfolio_optimisation.jl of the reference (n = 200 assets, k = 10 factors, :25-46) over `count` values of the risk aversion gamma,
    built as test_gpu_batch.py's portfolio test builds it: dense budget row, k + 1 equality rows."""
    n_assets, k = 200, 10
    rng = np.random.default_rng(1)
    Dd = rng.uniform(size=n_assets) * np.sqrt(k)
    F = sp.random(n_assets, k, density=0.5, random_state=rng, data_rvs=rng.standard_normal).tocsc()
    mu = (3.0 + 9.0 * rng.uniform(size=n_assets)) / 100.0
    P = sp.block_diag([2.0 * sp.diags(Dd), 2.0 * sp.identity(k)]).tocsc()
    A = sp.vstack([sp.hstack([F.T, -sp.identity(k)]), sp.hstack([sp.csr_matrix(np.ones((1, n_assets))), sp.csr_matrix((1, k))]),
                   sp.hstack([-sp.identity(n_assets), sp.csr_matrix((n_assets, k))])]).tocsc()
    b = np.concatenate([np.zeros(k), [1.0], np.zeros(n_assets)])
    sets = [cj.ZeroSet(k + 1), cj.Nonnegatives(n_assets)]
    return [dict(P=P, q=np.concatenate([-mu / g, np.zeros(k)]), A=A, b=b, sets=sets) for g in np.logspace(-2, 1, count)]


def test_portfolio_example_as_a_batch_over_gamma():
    probs = portfolio_batch(256)
    res = cj.optimize_batch(_models(probs, cj.Settings(kkt_solver=cj.QdldlKKTSolver, direct_batch=True)))
    assert "direct_info" in cj.model.LAST_BATCH_INFO
    for p, r in zip(probs, res):
        ref = _oracle(p)
        assert r.status == ref.status
        assert abs(r.obj_val - ref.obj_val) <= 1e-6 * max(abs(ref.obj_val), 1.0)
