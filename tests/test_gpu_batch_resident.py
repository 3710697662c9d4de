"""Resident batches (cj.BatchSolver; csrc/batch.hip: k_batch_update_qb, k_batch_warm_restart): update!(model; q, b) on the device and optimize! again
with the reference's re-solve semantics (src/interface.jl:187-211, src/setup.jl:18-62) -- checked member by member against a single-problem handle that
goes through the same update and optimize."""
import numpy as np
import pytest

import cosmo_jl_amd as cj
from tests import util
from tests.test_gpu_batch_direct import portfolio_batch

pytestmark = pytest.mark.gpu

TIGHT_CG = cj.with_options(cj.CGIndirectKKTSolver, tol_constant=1e-10, tol_exponent=0.0)


def _settings(**kw):
    kw.setdefault("kkt_solver", TIGHT_CG)
    return cj.Settings(device_scaling=False, **kw)     # host Ruiz scaling, as the batch set-up does it


def _models(probs, dtype=np.float64, **kw):
    st = _settings(**kw)
    out = []
    for p in probs:
        md = cj.Model(dtype=dtype)
        md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st)
        out.append(md)
    return out


def _single(p, q=None, b=None, dtype=np.float64, **kw):
    """The single handle's optimize, update, optimize."""
    md = _models([p], dtype=dtype, **kw)[0]
    r0 = cj.optimize(md)
    cj.update(md, q=q, b=b)
    r1 = cj.optimize(md)
    return md, r0, r1


def _agree(r, one, tol=1e-4, iters=25):
    """batch vs single handle (test_gpu_batch.py's bars): status, iterations within one termination check, objective; x and y at the solution's accuracy"""
    assert r.status == one.status, (r.status, one.status)
    assert abs(r.iter - one.iter) <= iters, (r.iter, one.iter)
    assert abs(r.obj_val - one.obj_val) <= tol * (1 + abs(one.obj_val)), (r.obj_val, one.obj_val)
    for a, c in ((r.x, one.x), (r.y, one.y)):
        assert np.max(np.abs(a - c)) <= 100 * tol * max(np.max(np.abs(c)), 1.0)


def test_portfolio_resolve_over_gamma_matches_the_single_handle():
    probs = portfolio_batch(64)
    models = _models(probs, eps_abs=1e-7, eps_rel=1e-7)
    with cj.BatchSolver(models) as rb:
        r0 = rb.optimize()
        kinfo = rb.batch.kernel_info()
        for md, p in zip(models, probs):
            cj.update(md, q=0.5 * p["q"])                  # gamma doubled
        r1 = rb.optimize()
        assert rb.batch.kernel_info() == kinfo            # the same batch and kernel: nothing was set up again
    assert all(r.status == "Solved" for r in r0 + r1)
    assert sum(r.iter for r in r1) < sum(r.iter for r in r0)  # warm-started from the previous solution
    for k in range(0, 64, 9):
        _, one0, one1 = _single(probs[k], q=0.5 * probs[k]["q"], eps_abs=1e-7, eps_rel=1e-7)
        _agree(r0[k], one0)
        _agree(r1[k], one1)
    # what update! hands to the solver: the host mirror holds the scaled q, as the reference's model.p.q
    assert np.allclose(models[3].q, (models[3].sm.D * (0.5 * probs[3]["q"])) * models[3].sm.c, rtol=0, atol=0)


def _family(count, seed=7):
    """members of one structure (Zero, Nonnegatives, Box rows) with different data"""
    return [util.random_qp(np.random.default_rng(seed + j), 30, 4, 20, 12, p_shift=1.0) for j in range(count)]


def test_mixed_update_reclassifies_and_leaves_unchanged_members_converged():
    probs = _family(12)
    models = _models(probs)
    rng = np.random.default_rng(99)
    with cj.BatchSolver(models) as rb:
        r0 = rb.optimize()
        upd = {}
        for k in range(0, 4):                              # q only
            upd[k] = dict(q=probs[k]["q"] + 0.3 * rng.standard_normal(30))
        for k in range(4, 8):                              # b only: every row, one Nonnegatives row of member 5 made infinite (class 2)
            b = probs[k]["b"] * rng.uniform(0.8, 1.2, probs[k]["b"].size)
            if k == 5:
                b[4 + 3] = 1e22
            upd[k] = dict(b=b)
        upd[8] = dict(q=probs[8]["q"] * 1.1, b=probs[8]["b"] * 1.05)
        for k, u in upd.items():
            cj.update(models[k], **u)
        r1 = rb.optimize()
        cls5 = rb.batch.get_rho_classes(5)
    assert cls5[4 + 3] == 2
    for k in range(12):
        if k in upd:
            md, one0, one1 = _single(probs[k], **upd[k])
            _agree(r0[k], one0)
            _agree(r1[k], one1)
            if k == 5:
                assert np.array_equal(cls5, md.handle.get_rho_classes())
        else:
            assert r1[k].status == "Solved" and r1[k].iter <= 25, (k, r1[k].iter)   # stops at the first termination check
            assert np.allclose(r1[k].x, r0[k].x, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_scaling_of_updates_is_bitwise_the_host_formula(dtype):
    probs = _family(6, seed=21)
    models = _models(probs, dtype=dtype, kkt_solver=cj.CGIndirectKKTSolver, eps_abs=1e-4, eps_rel=1e-4)
    rng = np.random.default_rng(5)
    with cj.BatchSolver(models) as rb:
        rb.optimize()
        B = rb.batch
        before = [B.get_qb(k) for k in range(6)]
        newq = {k: rng.standard_normal(30) for k in (0, 2, 3)}
        newb = {k: probs[k]["b"] * rng.uniform(0.9, 1.1, models[k].m) for k in (1, 3, 5)}
        for k in range(6):
            if k in newq or k in newb:
                B.stage_qb(k, newq.get(k), newb.get(k))
        B.apply_updates()
        t = np.dtype(dtype).type
        for k in range(6):
            q, b = B.get_qb(k)
            sm = models[k].sm
            if k in newq:
                assert np.array_equal(q, (sm.D.astype(dtype) * newq[k].astype(dtype)) * t(sm.c)), k
            else:
                assert np.array_equal(q, before[k][0]), k
            if k in newb:
                assert np.array_equal(b, sm.E.astype(dtype) * newb[k].astype(dtype)), k
            else:
                assert np.array_equal(b, before[k][1]), k
        r = rb.optimize()                                  # nothing staged any more: an empty flush, then the re-solve
        assert all(x.status == "Solved" for x in r), [x.status for x in r]


def test_direct_batch_keeps_its_factor_across_update_and_resolve():
    probs = portfolio_batch(32)
    kw = dict(kkt_solver=cj.QdldlKKTSolver, direct_batch=True, adaptive_rho=False, eps_abs=1e-7, eps_rel=1e-7)
    models = _models(probs, **kw)
    with cj.BatchSolver(models) as rb:
        r0 = rb.optimize()
        info0, counts0 = rb.batch.direct_info(), rb.batch.direct_counts()
        for md, p in zip(models, probs):
            cj.update(md, q=2.0 * p["q"])
        r1 = rb.optimize()
        info1, counts1 = rb.batch.direct_info(), rb.batch.direct_counts()
    assert np.array_equal(counts0, counts1)
    assert info0 == info1                                  # no analysis, no factorisation
    for k in (0, 13, 31):
        _, one0, one1 = _single(probs[k], q=2.0 * probs[k]["q"], **kw)
        _agree(r0[k], one0)
        _agree(r1[k], one1)


def test_group_with_an_own_handle_member_resolves():
    rng = np.random.default_rng(12)
    small = [util.random_qp(rng, 30, 4, 20, 40) for _ in range(3)]
    big = util.random_qp(np.random.default_rng(3), 20, 0, 0, 0, psd_tri_dims=(70,), p_shift=1.0)
    other = util.random_qp(rng, 24, 3, 10, 5)
    probs = [small[0], big, small[1], other, small[2]]
    kw = dict(decompose=False, kkt_solver=cj.CGIndirectKKTSolver)
    models = _models(probs, **kw)
    upd = {0: dict(q=probs[0]["q"] * 0.7), 1: dict(q=probs[1]["q"] + 0.1), 3: dict(b=probs[3]["b"] * 1.1), 4: dict(q=probs[4]["q"] * 1.3, b=probs[4]["b"] * 0.9)}
    with cj.BatchSolver(models) as rb:
        r0 = rb.optimize()
        assert rb.mixed
        _, _, modes = rb.batch.class_info(with_modes=True)
        assert modes.tolist() == [0, 1, 0, 0, 0]
        for k, u in upd.items():
            cj.update(models[k], **u)
        r1 = rb.optimize()
        q0, _ = rb.batch.get_qb(0)
        assert np.array_equal(q0, (models[0].sm.D * (probs[0]["q"] * 0.7)) * models[0].sm.c)
    for k, p in enumerate(probs):
        _, one0, one1 = _single(p, **upd.get(k, {}), **kw)
        for r, one in ((r0[k], one0), (r1[k], one1)):
            assert r.status == one.status == "Solved", (k, r.status, one.status)
            assert abs(r.obj_val - one.obj_val) <= 1e-4 * (1 + abs(one.obj_val)), (k, r.obj_val, one.obj_val)
    assert r1[2].iter <= 25                                # not updated: converged at the first check


def test_accelerated_resolve_matches_the_single_handle():
    probs = portfolio_batch(16)
    kw = dict(accelerator=cj.AndersonAccelerator, eps_abs=1e-7, eps_rel=1e-7)
    models = _models(probs, **kw)
    with cj.BatchSolver(models) as rb:
        r0 = rb.optimize()
        for md, p in zip(models, probs):
            cj.update(md, q=0.25 * p["q"])
        r1 = rb.optimize()
        stats = rb.batch.accel_stats()
    assert stats["accelerated"].sum() > 0                  # counted from the restart: this solve's accelerated steps
    for k in (0, 7, 15):
        _, one0, one1 = _single(probs[k], q=0.25 * probs[k]["q"], **kw)
        for r, one in ((r0[k], one0), (r1[k], one1)):
            assert r.status == one.status == "Solved"
            assert abs(r.obj_val - one.obj_val) <= 1e-4 * (1 + abs(one.obj_val)), (k, r.obj_val, one.obj_val)


def test_update_errors_on_a_bound_model_and_warm_start_from_models():
    probs = _family(3, seed=40)
    models = _models(probs)
    with cj.BatchSolver(models) as rb:
        r0 = rb.optimize()
        with pytest.raises(ValueError, match="dimension of q"):
            cj.update(models[0], q=np.zeros(31))
        with pytest.raises(ValueError, match="dimension of b"):
            cj.update(models[1], b=np.zeros(3))
        r1 = rb.optimize(warm_start="models")               # the models' x, s, mu (written back by the first solve) through set_iterates
    for a, c in zip(r0, r1):
        assert c.status == "Solved" and c.iter <= 25 and abs(a.obj_val - c.obj_val) <= 1e-4 * (1 + abs(a.obj_val))
