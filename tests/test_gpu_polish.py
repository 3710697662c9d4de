"""Polishing of the solved QP members of a batch on their active set (Settings.polish, cosmo_hip_batch_polish, csrc/batch_polish.hip) on the MI355X.

The inputs are the strictly complementary QPs of tests/polish_cases.py, whose solution (x*, y*, s*) is known by construction; tests/test_polish_cases_host.py
shows on the CPU that the active-set rule finds their active sets from ADMM solutions at eps = 1e-5 and 1e-3, that the dense numpy polish reproduces the
solution to <= 3.8e-15 and that cond(K) <= 1.1e2.  The bound here is 1e-10 * max(1, ||.*||_inf): that measured 4e-15 with four orders of margin, because the
sparse factor eliminates in another order; 1e3 * cond * eps ~ 2e-11 is the expected scale."""
import numpy as np
import pytest
import torch

import cosmo_jl_amd as cj
from cosmo_jl_amd import _ffi
from tests import polish_cases as PC

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _settings(**kw):
    return cj.Settings(**kw)


def _solve(members, **kw):
    return cj.optimize_batch(PC.models(members, _settings(**kw), cj))


def _check_exact(members, res, tol=TOL, label=""):
    for k, (c, r) in enumerate(zip(members, res)):
        e = PC.errors(c, r.x, r.y, r.s)
        print("%s member %d: status %s iter %d polish %d  err x %.2e y %.2e s %.2e  res %.2e %.2e (before %.2e %.2e)" % (
            label, k, r.status, r.iter, r.info.polish_status, e[0][0], e[1][0], e[2][0], r.info.r_prim, r.info.r_dual, r.info.polish_res_prim_before,
            r.info.polish_res_dual_before))
    for k, (c, r) in enumerate(zip(members, res)):
        assert r.status == "Solved" and r.info.polish_status == 1, (k, r.status, r.info.polish_status)
        for err, scale in PC.errors(c, r.x, r.y, r.s):
            assert err <= tol * scale, (k, err, scale)
        assert r.info.r_prim <= r.info.polish_res_prim_before and r.info.r_dual <= r.info.polish_res_dual_before, k


def _check_reported_residuals(members, res):
    for k, (c, r) in enumerate(zip(members, res)):
        rp, rd = PC.residuals(c, r.x, r.y, r.s)
        print("member %d: reported %.3e %.3e  numpy %.3e %.3e" % (k, r.info.r_prim, r.info.r_dual, rp, rd))
        assert abs(r.info.r_prim - rp) <= 1e-12 * rp + 1e-14 and abs(r.info.r_dual - rd) <= 1e-12 * rd + 1e-14, (k, r.info.r_prim, rp, r.info.r_dual, rd)
        obj = 0.5 * r.x @ (c["P"] @ r.x) + c["q"] @ r.x
        assert abs(r.obj_val - obj) <= 1e-12 * max(1.0, abs(obj)), (k, r.obj_val, obj)


# ---- 1. accuracy ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-5, 1e-3])
def test_accuracy_of_the_polished_fixture(eps):
    """The test that fails without the feature: the same call without polish misses 1e-7 on at least one member."""
    B = PC.batch()
    res = _solve(B, polish=True, eps_abs=eps, eps_rel=eps)
    _check_exact(B, res, label="eps %g" % eps)
    info = cj.model.LAST_BATCH_INFO
    assert not info["mixed"]
    _check_reported_residuals(B, res)
    plain = _solve(B, eps_abs=eps, eps_rel=eps)
    worst = max(PC.errors(c, r.x, r.y, r.s)[0][0] for c, r in zip(B, plain))
    print("without polish: worst |x - x*| = %.2e" % worst)
    assert worst > 1e-7
    assert all(r.info.polish_status == 0 and np.isnan(r.info.polish_res_prim_before) for r in plain)


def test_active_row_counts_and_info_through_the_library():
    B = PC.batch()
    st = _settings()
    Bt, _ = cj.model.prepare_batch(PC.models(B, st, cj), 0)
    try:
        Bt.optimize()
        Bt.polish(1e-6, 3)
        info = Bt.polish_info()
        assert list(info["status"]) == [1] * 8
        assert list(info["active_rows"]) == [int(c["act"].sum()) for c in B]
        assert np.all(info["r_prim"] <= info["r_prim_before"]) and np.all(info["r_dual"] <= info["r_dual_before"])
    finally:
        Bt.close()


# ---- 2. both solver kinds ---------------------------------------------------------------------------------------------------------------------------
def test_cg_batch_builds_its_own_plan():
    B = PC.batch()
    res = _solve(B, polish=True, kkt_solver=cj.CGIndirectKKTSolver)
    assert cj.model.LAST_BATCH_INFO["kernel_form"] != "streaming"            # the register / LDS kernels ran the loop; the polish streams
    _check_exact(B, res, label="cg")


def test_direct_batch_shares_its_plan_and_keeps_its_factorisation_counts():
    B = PC.batch()
    st = _settings(kkt_solver=cj.QdldlKKTSolver, direct_batch=True)
    Bt, _ = cj.model.prepare_batch(PC.models(B, st, cj), 0)
    try:
        Bt.optimize()
        before = Bt.direct_counts().copy()
        Bt.polish(1e-6, 3)
        assert np.array_equal(Bt.direct_counts(), before)
        assert list(Bt.polish_info()["status"]) == [1] * 8
    finally:
        Bt.close()
    res = _solve(B, polish=True, kkt_solver=cj.QdldlKKTSolver, direct_batch=True)
    assert "direct_info" in cj.model.LAST_BATCH_INFO
    _check_exact(B, res, label="direct")


# ---- 3. untouched members ---------------------------------------------------------------------------------------------------------------------------
def _same_member(a, b):
    return (np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y) and np.array_equal(a.s, b.s) and a.status == b.status and a.iter == b.iter and
            np.array_equal(a.info.r_prim, b.info.r_prim) and np.array_equal(a.info.r_dual, b.info.r_dual) and np.array_equal(a.obj_val, b.obj_val))


def test_members_that_are_not_solved_keep_every_bit():
    """max_iter = 10 is a setting of the whole batch, so the member that IS solved within it starts next to its solution (1e-4 off, eps = 1e-3: converged at
    the first check, still 1e-4 from x*); the second starts cold and is stopped by max_iter, the third is primal infeasible (and stopped as well)."""
    members = PC.on_union_pattern([PC.member(0), PC.member(1), PC.infeasible()])

    def run(polish):
        mds = PC.models(members, _settings(polish=polish, max_iter=10, eps_abs=1e-3, eps_rel=1e-3), cj)
        c = members[0]
        rng = np.random.default_rng(5)
        cj.warm_start_primal(mds[0], c["x"] + 1e-4 * rng.standard_normal(c["n"]))
        cj.warm_start_slack(mds[0], c["s"]); cj.warm_start_dual(mds[0], c["y"])
        return cj.optimize_batch(mds)
    pol, plain = run(True), run(False)
    print([(r.status, r.iter, r.info.polish_status) for r in pol])
    assert [r.status for r in plain] == ["Solved", "Max_iter_reached", "Max_iter_reached"]
    assert [r.info.polish_status for r in pol] == [1, 0, 0]
    assert _same_member(pol[1], plain[1]) and _same_member(pol[2], plain[2])
    assert PC.errors(members[0], plain[0].x, plain[0].y, plain[0].s)[0][0] > 1e-6
    _check_exact(members[:1], pol[:1], label="warm")


def test_an_infeasible_member_is_left_alone():
    members = PC.on_union_pattern([PC.member(0), PC.infeasible()])
    pol = cj.optimize_batch(PC.models(members, _settings(polish=True), cj))
    plain = cj.optimize_batch(PC.models(members, _settings(), cj))
    assert [r.status for r in pol] == ["Solved", "Primal_infeasible"] and [r.info.polish_status for r in pol] == [1, 0]
    assert _same_member(pol[1], plain[1])
    _check_exact(members[:1], pol[:1], label="next to an infeasible member")


# ---- 4. rejected candidates -------------------------------------------------------------------------------------------------------------------------
def _scaled_residuals(c, x, s, mu):
    """of the device's iterates when scaling = 0 (the device problem is the raw one; y = -mu)"""
    return PC.residuals(c, x, -mu, s)


def test_a_wrong_guess_never_makes_a_member_worse():
    """mu negated through cosmo_hip_batch_set_iterates: the rule picks a wrong set.  The library decides between -1 and 1; either way no residual grows,
    and on -1 not a bit of the iterates changes.  Second member: an active Nonnegatives row twice (the active rows of A are rank deficient)."""
    members = PC.on_union_pattern([PC.member(0), PC.duplicated_active_row()])
    n, m = members[0]["n"], members[0]["m"]
    Bt, _ = cj.model.prepare_batch(PC.models(members, _settings(scaling=0), cj), 0)
    try:
        rs = Bt.optimize()
        assert [_ffi.STATUS_NAMES[r.status] for r in rs] == ["Solved", "Solved"]
        it = [Bt.get_iterates(k) for k in range(2)]
        x0 = np.concatenate([w_prev[:n] for _, w_prev, _, _ in it]); s0 = np.concatenate([s for _, _, s, _ in it])
        mu0 = np.concatenate([-it[0][3], it[1][3]])                            # member 0: the negated mu; member 1 as it is
        Bt.set_iterates(x0, s0, mu0)
        held = [Bt.get_iterates(k) for k in range(2)]
        before = [_scaled_residuals(members[k], x0[k * n:(k + 1) * n], s0[k * m:(k + 1) * m], mu0[k * m:(k + 1) * m]) for k in range(2)]
        Bt.polish(1e-6, 3)                                                      # returns OK (raises otherwise)
        info = Bt.polish_info()
        print("status", info["status"], "before", before, "candidate", info["r_prim"], info["r_dual"], "active", info["active_rows"])
        for k in range(2):
            assert info["status"][k] in (-1, 1)
            assert np.isfinite(info["r_prim_before"][k]) and np.isfinite(info["r_dual_before"][k])
            assert abs(info["r_prim_before"][k] - before[k][0]) <= 1e-12 * before[k][0] + 1e-14
            assert abs(info["r_dual_before"][k] - before[k][1]) <= 1e-12 * before[k][1] + 1e-14
            w, w_prev, s, mu = Bt.get_iterates(k)
            assert all(np.all(np.isfinite(v)) for v in (w, w_prev, s, mu))
            if info["status"][k] == 1:
                rp, rd = _scaled_residuals(members[k], w_prev[:n], s, mu)
                assert rp <= before[k][0] and rd <= before[k][1], (k, rp, rd, before[k])
            else:
                assert all(np.array_equal(a, b) for a, b in zip((w, w_prev, s, mu), held[k])), k
        # the duplicated row: x* and s* are still the solution (y* is not unique), and the regularised factor finds them
        assert info["status"][1] == 1
        w, w_prev, s, mu = Bt.get_iterates(1)
        assert np.max(np.abs(w_prev[:n] - members[1]["x"])) <= 1e-6 and np.max(np.abs(s - members[1]["s"])) <= 1e-6
    finally:
        Bt.close()


# ---- 5. edge shapes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["no_inequality_active", "every_row_active", "upper_bounds_infinite", "single_row"])
def test_edge_members(name):
    members = getattr(PC, name)()
    res = _solve(members, polish=True)                                          # (also: a batch of 1 member)
    _check_exact(members, res, label=name)


def test_without_refinement_the_regularised_solve_is_accepted():
    """refine_iter = 0 leaves the regularisation in the answer: residuals of delta * |(x, y)| ~ 3e-6 and an error of delta * ||K^-1|| * |(x, y)| <= 1e-4 (cond <=
    1.1e2).  That is accepted against ADMM solutions coarser than 3e-6, hence eps = 1e-3 here (at the default eps the loop's residuals reach 1e-8 on some
    members and the acceptance rule rightly keeps those)."""
    B = PC.batch()
    res = _solve(B, polish=True, polish_refine_iter=0, eps_abs=1e-3, eps_rel=1e-3)
    for k, (c, r) in enumerate(zip(B, res)):
        print("member %d: polish %d err %.2e res %.2e %.2e (before %.2e %.2e)" % (k, r.info.polish_status, PC.errors(c, r.x, r.y, r.s)[0][0], r.info.r_prim, r.info.r_dual,
                                                                                  r.info.polish_res_prim_before, r.info.polish_res_dual_before))
    for c, r in zip(B, res):
        assert r.info.polish_status == 1
        assert PC.errors(c, r.x, r.y, r.s)[0][0] <= 1e-4


def test_more_members_than_resident_workgroups():
    """300 members of the smallest fixture: the grid has at most one workgroup per CU (256), so some workgroups take a second member."""
    members = PC.batch(seeds=tuple(range(300)), **PC.SMALL)
    res = _solve(members, polish=True)
    bad = [k for k, (c, r) in enumerate(zip(members, res)) if r.status != "Solved" or r.info.polish_status != 1 or
           any(err > TOL * scale for err, scale in PC.errors(c, r.x, r.y, r.s))]
    assert not bad, bad


# ---- 6. resident use --------------------------------------------------------------------------------------------------------------------------------
def test_resident_batches_polish_on_the_device_and_reproducibly():
    B = PC.batch()

    def sequence():
        out = []
        with cj.BatchSolver(PC.models(B, _settings(polish=True), cj)) as S:
            d = S.optimize(results="device")
            assert d.polish_status.dtype == torch.int32 and d.polish_status.is_cuda and d.polish_status.cpu().tolist() == [1] * 8
            out += [d.x.cpu().numpy(), d.y.cpu().numpy(), d.s.cpu().numpy()]
            q2 = torch.tensor(np.stack([1.01 * c["q"] for c in B]), device=d.x.device)
            S.update_device(q=q2)
            d2 = S.optimize(warm_start="device", results="device")
            assert d2.status == ["Solved"] * 8 and d2.polish_status.cpu().tolist() == [1] * 8
            out += [d2.x.cpu().numpy(), d2.y.cpu().numpy(), d2.s.cpu().numpy(), d2.r_prim, d2.r_dual, d2.obj_val]
        return out
    a, b = sequence(), sequence()
    assert all(np.array_equal(u, v) for u, v in zip(a, b))                      # two identical sequences: identical bits
    with cj.BatchSolver(PC.models(B, _settings(polish=True), cj)) as S:
        res = S.optimize(results="models")
    assert np.array_equal(np.stack([r.x for r in res]), a[0])                   # the device x is the models' x to the bit
    _check_exact(B, res, label="resident")
    # the re-solve with q scaled by 1.01 is polished too: P x + 1.01 q + A' y = 0 to rounding
    for k, c in enumerate(B):
        assert np.max(np.abs(c["P"] @ a[3][k] + 1.01 * c["q"] + c["A"].T @ a[4][k])) <= 1e-12


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------
def _soc_model(st):
    rng = np.random.default_rng(1)
    n = 6
    md = cj.Model()
    md.set(np.eye(n), rng.standard_normal(n), -np.eye(n)[:4], np.zeros(4), [cj.SecondOrderCone(4)], st)
    return md


def test_what_cannot_be_polished_is_refused_aloud_and_untouched_without_polish():
    c = PC.batch()[0]
    small = PC.batch(seeds=(0,), **PC.SMALL)[0]
    for polish in (True, False):
        st = _settings(polish=polish)
        cases = [lambda: cj.optimize_batch([_soc_model(st), _soc_model(st)]),                                   # another cone
                 lambda: cj.optimize_batch(PC.models([c], st, cj) + PC.models([small], st, cj)),                 # a mixed list
                 lambda: cj.optimize(PC.models([c], st, cj)[0])]                                                # a single optimize() on its own handle
        for fn in cases:
            if polish:
                with pytest.raises(NotImplementedError, match="polish"):
                    fn()
            else:
                out = fn()
                assert all(r.status == "Solved" for r in (out if isinstance(out, list) else [out]))
    st = _settings(polish=True, persistent_kernel=True)                         # ... while the persistent-kernel route polishes one model
    r = cj.optimize(PC.models([c], st, cj)[0])
    _check_exact([c], [r], label="persistent_kernel")


def test_the_library_refuses_before_a_solve_bad_arguments_and_other_cones():
    Bt, _ = cj.model.prepare_batch(PC.models(PC.batch()[:2], _settings(), cj), 0)
    try:
        for call in (lambda: Bt.polish(1e-6, 3), lambda: Bt.polish_info()):
            with pytest.raises(_ffi.CosmoHipError) as e:
                call()
            assert _ffi.ERR_NAMES.get(e.value.code) == "INVALID"
        Bt.optimize()
        for delta, it in ((0.0, 3), (-1.0, 3), (1e-6, -1)):
            with pytest.raises(_ffi.CosmoHipError) as e:
                Bt.polish(delta, it)
            assert _ffi.ERR_NAMES.get(e.value.code) == "INVALID"
        Bt.polish(1e-6, 3)
    finally:
        Bt.close()
    st = _settings()
    Bs, _ = cj.model.prepare_batch([_soc_model(st)], 0)
    try:
        Bs.optimize()
        with pytest.raises(_ffi.CosmoHipError, match="SecondOrderCone") as e:
            Bs.polish(1e-6, 3)
        assert _ffi.ERR_NAMES.get(e.value.code) == "UNSUPPORTED"
    finally:
        Bs.close()


# ---- 8. Float32 -------------------------------------------------------------------------------------------------------------------------------------
def test_float32_against_the_float32_restatement():
    """The float32 library with delta = POLISH_DELTA_F32 = 1e-3.  Yardstick: the dense float32 numpy polish of the same members from the same kind of
    start (the constructed solution perturbed by 1e-3, which the rule resolves), worst |x - x*| over the fixture.  Measured: restatement 5.5e-7 on the CPU;
    the device figure is printed by this test (bound: 10 x the restatement)."""
    B = PC.batch()
    rng = np.random.default_rng(7)
    ref = 0.0
    for c in B:
        p = PC.polish_dense(c["P"], c["q"], c["A"], c["b"], c["s"] + 1e-3 * rng.standard_normal(c["m"]), c["y"] + 1e-3 * rng.standard_normal(c["m"]),
                            c["lo"], c["hi"], c["mz"], delta=cj.model.POLISH_DELTA_F32, refine_iter=3, dtype=np.float32)
        assert np.array_equal(p["act"], c["act"])
        ref = max(ref, PC.errors(c, p["x"], p["y"], p["s"])[0][0])
    res = cj.optimize_batch(PC.models(B, _settings(polish=True, eps_abs=1e-4, eps_rel=1e-4), cj, dtype=np.float32))
    worst = 0.0
    for k, (c, r) in enumerate(zip(B, res)):
        assert r.status == "Solved" and r.info.polish_status in (1, -1), (k, r.status)
        if r.info.polish_status == 1:
            assert r.info.r_prim <= r.info.polish_res_prim_before and r.info.r_dual <= r.info.polish_res_dual_before, k
            worst = max(worst, PC.errors(c, r.x, r.y, r.s)[0][0])
    print("float32: accepted %d of 8, worst |x - x*| = %.2e, restatement %.2e" % (sum(r.info.polish_status == 1 for r in res), worst, ref))
    assert any(r.info.polish_status == 1 for r in res)
    assert worst <= 10 * ref
