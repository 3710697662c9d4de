"""Residuals, termination and the rho rule of a single handle (csrc/kernels.hip: k_chk_prim, k_chk_dual, k_chk_final, k_rho_apply), one check at a time.

cosmo_hip_optimize runs init, then per iteration admm_z (w_prev = w, s = Pi(w_s)), the optional rho rule, the KKT solve, the check; the KKT solve writes
neither w_prev nor s.  get_iterates after the call therefore returns exactly the w_prev and s the last check was computed from, and the exact reference
of tests/residual_cases.py is evaluated on those FETCHED iterates: the accuracy of the inner solve never enters.  Every comparison is held to the
rounding bound of that file; every decision is provoked by a threshold MARGIN = 10 bounds on either side of the exact value.
tests/test_residual_cases_host.py proves the problems, the reference, the bounds' power to see the wrong formulas, and the threshold plans on the CPU.

Every test prints the largest observed error / bound per quantity (WORST).  The run that introduced this file (MI355X), over all shapes, both precisions on each:

                             type   r_prim  r_dual  max_norm_prim  max_norm_dual  cost     new rho
  cosmo_hip_residuals        f64    0.24    0.16    0.28           0.11           0.15
  cosmo_hip_residuals        f32    0.31    0.11    0.22           0.11           0.050
  the loop's check           f64    0.26    0.15    0.23           0.13           0.045
  the loop's check           f32    0.25    0.12    0.13           0.31           0.071
  the check after the rule   f64    0.26    0.20    0.23           0.21           0.045    0.077
  the check after the rule   f32    0.25    0.17    0.13           0.10           0.071    0.079

Not observable through the ABI and therefore not compared: w[n:] right after an adaptation (the KKT solve overwrites it before the call returns)."""
import contextlib
import faulthandler
import os
import types
from fractions import Fraction

import numpy as np
import pytest

import cosmo_jl_amd as cj
from tests import residual_cases as R
from tests.residual_gpu import CASE_LIMIT_S, MAX_ITER, SOLVED, UNSOLVED, F, cone_args, params, recovered_mu, same_bits

pytestmark = pytest.mark.gpu

DIDS = ("f64", "f32")
WORST = {}


@pytest.fixture(autouse=True)
def _case_time_limit():
    """a case that hangs takes the whole process down instead of holding the GPU: nothing runs after a hang"""
    faulthandler.dump_traceback_later(CASE_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def make_handle(pb, **kw):
    dtype = R.DTYPES[pb.dtype_id]
    with _env(R.HANDLE_ENV.get(pb.name.split("/")[0], {})):
        h = cj.Handle(0, dtype=dtype)
        h.set_problem(pb.P, pb.q, pb.A, pb.b)
        kinds, dims, bl, bu = cone_args(pb)
        h.set_cones(kinds, dims, bl, bu)
        h.set_params(params(dtype, **kw))
        h.set_scaling_full(1.0 / pb.Dinv, pb.Dinv, 1.0 / pb.Einv, pb.Einv, 1.0 / pb.cinv, pb.cinv)
    return h


def solve(pb, **kw):
    """a fresh handle, set_iterates(x0, s0, mu0), optimize: what it reports and what it leaves behind"""
    h = make_handle(pb, **kw)
    try:
        h.set_iterates(pb.x0, pb.s0, pb.mu0)
        res = h.optimize()
        w, w_prev, s, mu = h.get_iterates()
        rho = h.get_rho_vec() if pb.m else np.zeros(0, dtype=h.dtype)
        assert np.array_equal(h.get_rho_classes(), pb.cls) if pb.m else True
    finally:
        h.close()
    n = pb.n
    return types.SimpleNamespace(status=res.status, iter=res.iter, five=[res.r_prim, res.r_dual, res.max_norm_prim, res.max_norm_dual, res.cost], rho=res.rho,
                                 n_rho_updates=res.n_rho_updates, rho_updates=[res.rho_updates[i] for i in range(res.n_rho_updates)],
                                 w=w, w_prev=w_prev, s=s, mu=mu, rho_vec=rho, x=w_prev[:n].astype(np.float64), s64=s.astype(np.float64),
                                 wps=w_prev[n:].astype(np.float64))


_first = {}


def first_run(pb):
    """max_iter = 1, check_termination = 1, eps = 0, no adaptation: once per problem for all tests of this file"""
    if pb.name + pb.dtype_id not in _first:
        _first[pb.name + pb.dtype_id] = solve(pb, max_iter=1)
    return _first[pb.name + pb.dtype_id]


def note(kind, did, name, ratio):
    key = (kind, did, name)
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def report():
    print("worst error / bound so far: " + ", ".join("%s %s %s %.3g" % (k + (v,)) for k, v in sorted(WORST.items())))


def within(got5, c, kind, where, which=range(5)):
    """the five reported numbers against the exact ones, each within its bound"""
    for k in which:
        val, bound = c.five()[k]
        err = abs(Fraction(float(got5[k])) - val)
        assert err <= Fraction(bound), where + (R.FIVE[k], got5[k], float(val), float(err), bound)
        if bound > 0:
            note(kind, where[1], R.FIVE[k], float(err) / bound)


SHAPE_PARAMS = [(name, did) for name in R.HANDLE_SHAPES for did in DIDS]
SHAPE_IDS = ["%s-%s" % p for p in SHAPE_PARAMS]
LOOP_SHAPES = SHAPE_PARAMS
ROWS_SHAPES = [p for p in LOOP_SHAPES if p[0] != "no_rows"]


def test_the_defaults_are_the_constants_of_the_case_file():
    for did in DIDS:
        p = F.default_params(R.DTYPES[did])
        assert (p.rho, p.rho_min, p.rho_max, p.rho_eq_over_rho_ineq, p.adaptive_rho_tolerance) == (R.RHO, R.RHO_MIN, R.RHO_MAX, R.RHO_EQ, R.ADAPT_TOL)
        assert p.cosmo_infty_min_scaling == 1e16 and p.rho_tol == 1e-4


@pytest.mark.parametrize("name,did", SHAPE_PARAMS, ids=SHAPE_IDS)
def test_residuals_entry_point_at_chosen_iterates(name, did):
    """cosmo_hip_residuals right after set_iterates: the iterates are the chosen ones, so every placement of the case file applies literally -- each of
    Ax, s, b, Px, q, A'mu is the strict arg-max of its max-norm at the first row, the last, the end of a tile, an index >= 512, the long row"""
    t = R.DTYPES[did]
    for pb in R.handle_problems(name, did):
        h = make_handle(pb)
        try:
            h.set_iterates(pb.x0, pb.s0, pb.mu0)
            out = h.residuals()
            w, w_prev, s, mu = h.get_iterates()
            rho = h.get_rho_vec() if pb.m else np.zeros(0, dtype=t)
            again = h.residuals()
        finally:
            h.close()
        rv = R.rho_vec(R.RHO, pb.cls, did)
        assert same_bits(rho.astype(np.float64), rv)
        assert same_bits(w_prev[:pb.n], pb.x0.astype(t)) and same_bits(s, pb.s0.astype(t)) and same_bits(w, w_prev)
        assert same_bits(w_prev[pb.n:], (t(1.0) / rv.astype(t)) * pb.mu0.astype(t) + pb.s0.astype(t))            # solver.jl:129 in the type
        assert same_bits(mu, rv.astype(t) * (w_prev[pb.n:] - s))
        c = R.termination(pb, w_prev[:pb.n].astype(np.float64), s.astype(np.float64), w_prev[pb.n:].astype(np.float64), rv)
        within(out, c, "residuals()", (pb.name, did, pb.place))
        assert same_bits(out, again)
        if pb.place is not None:                                              # the placement survived the trip: the reported max-norm IS the placed term
            term = pb.place[0]
            k = 2 if term in R.TERMS_PRIM else 3
            others = max(c.norms[o][0] for o in (R.TERMS_PRIM if k == 2 else R.TERMS_DUAL) if o != term)
            assert Fraction(float(out[k])) > 8 * others and c.norms[term][1] == pb.place[2], (pb.name, did, pb.place)
    report()


@pytest.mark.parametrize("name,did", LOOP_SHAPES, ids=["%s-%s" % p for p in LOOP_SHAPES])
def test_the_loop_reports_the_values_of_its_last_check(name, did):
    """max_iter = 1: the check of iteration 1, then calculate_result_info! at max_iter, both on the fetched w_prev and s"""
    for pb in R.handle_problems(name, did):
        run = first_run(pb)
        assert (run.status, run.iter, run.n_rho_updates) == (MAX_ITER, 1, 1), (pb.name, did, run.status, run.iter)
        rv = R.rho_vec(R.RHO, pb.cls, did)
        assert same_bits(run.rho_vec.astype(np.float64), rv) and same_bits(run.mu, recovered_mu(run, rv, did))
        within(run.five, R.termination(pb, run.x, run.s64, run.wps, rv), "loop", (pb.name, did))
    report()


@pytest.mark.parametrize("name,did", LOOP_SHAPES, ids=["%s-%s" % p for p in LOOP_SHAPES])
def test_thresholds_on_either_side_of_the_exact_value_decide(name, did):
    """A second run with max_iter = 2 and one threshold MARGIN bounds below / above the exact value: Max_iter_reached after 2 iterations on one side,
    Solved after 1 on the other -- with the iterates of the first run bit for bit -- wherever the reference decides with MARGIN bounds to spare
    (the two residual gates share eps_abs and eps_rel: a verdict whose other gate sits closer than that is not one to hold the device to)."""
    sole, flips = set(), set()
    for pb in R.handle_problems(name, did):
        one = first_run(pb)
        two = solve(pb, max_iter=2)
        assert (two.status, two.iter) == (MAX_ITER, 2)
        c = R.termination(pb, one.x, one.s64, one.wps, R.rho_vec(R.RHO, pb.cls, did))
        for label, gate, below, above in R.plan_decisions(c, did):
            for side, prm in (("below", below), ("above", above)):
                g = R.gates(c, did, **prm)
                solved, margin, failing = R.decided(g)
                assert g[gate][0] == (side == "above") and float(g[gate][1]) >= R.MARGIN
                if margin < R.MARGIN:                                          # a neighbouring gate too close to the shared threshold: nothing to hold the device to
                    continue
                run = solve(pb, max_iter=2, **prm)
                where = (pb.name, did, label, gate, side, prm, failing, margin)
                if solved:
                    assert (run.status, run.iter) == (SOLVED, 1), where + (run.status, run.iter, run.five)
                    assert same_bits(run.w_prev, one.w_prev) and same_bits(run.s, one.s), where
                    within(run.five, c, "loop", (pb.name, did))
                    flips.add(label)
                else:
                    assert (run.status, run.iter) == (MAX_ITER, 2), where + (run.status, run.iter, run.five)
                    assert same_bits(run.w_prev, two.w_prev) and same_bits(run.s, two.s) and same_bits(run.w, two.w), where
                    if failing == [gate] and all(mg is None or mg >= R.MARGIN for _, mg in g.values()):
                        sole.add(gate)
    print("%s %s: sole failing gates %s, thresholds that turned Solved into Max_iter_reached %s" % (name, did, sorted(sole), sorted(flips)))
    # every gate stopped a run alone and every kind of threshold turned Solved into Max_iter_reached, within this shape (without rows r_prim = 0 has
    # no bound to straddle and max_norm_prim = 0 leaves eps_rel nothing to scale)
    want = ({"dual", "obj"}, {"eps_abs", "obj_true"}) if name == "no_rows" else ({"prim", "dual", "obj"}, {"eps_abs", "eps_rel", "obj_true"})
    assert (sole, flips) == want, (name, did, sole, flips)
    report()


@pytest.mark.parametrize("did", DIDS)
def test_a_cost_beyond_1e20_is_unsolved(did):
    pb = R.special("huge_cost", did)
    run = solve(pb, max_iter=2, eps_abs=1e30)
    c = R.termination(pb, run.x, run.s64, run.wps, R.rho_vec(R.RHO, pb.cls, did))
    assert abs(c.cost) - Fraction(1e20) > R.MARGIN * Fraction(c.b_cost), (float(c.cost), c.b_cost)
    assert (run.status, run.iter) == (UNSOLVED, 1), (run.status, run.iter, run.five)
    within(run.five, c, "loop", (pb.name, did), which=[4])


def check_adapted(pb, did, run, one, rl, where):
    """an adaptation at iteration 1: rho_updates[1], rho, the rho vector by class, and the check that follows with mu = rho_new .* (w_prev_s - s)"""
    t = R.DTYPES[did]
    assert run.n_rho_updates == 2 and run.rho_updates[0] == float(t(R.RHO)) and run.rho_updates[1] == run.rho, where + (run.rho_updates, run.rho)
    assert rl.lo <= Fraction(run.rho) <= rl.hi, where + (run.rho, float(rl.lo), rl.new_rho, float(rl.hi))
    if rl.rel > 0:
        note("rho rule", did, "new_rho", abs(Fraction(run.rho) - rl.exact) / (rl.rel * rl.exact))
    assert same_bits(run.w_prev, one.w_prev) and same_bits(run.s, one.s), where   # the rule ran on the iterates of the first run
    new_rv = R.rho_vec(run.rho, pb.cls, did)
    assert same_bits(run.rho_vec.astype(np.float64), new_rv), where
    assert same_bits(run.mu, recovered_mu(run, new_rv, did)), where
    after = R.termination(pb, run.x, run.s64, run.wps, new_rv)
    within(run.five, after, "after adaptation", (pb.name, did))
    stale = R.termination(pb, run.x, run.s64, run.wps, R.rho_vec(R.RHO, pb.cls, did))
    return abs(stale.r_dual - after.r_dual) > R.MARGIN * Fraction(after.b_dual)  # would mu from the old rho have shown?


def check_not_adapted(run, one, where):
    assert run.n_rho_updates == 1 and run.rho == one.rho, where + (run.rho_updates,)
    assert same_bits(run.w, one.w) and same_bits(run.rho_vec, one.rho_vec) and same_bits(run.mu, one.mu) and same_bits(run.five, one.five), where


@pytest.mark.parametrize("name,did", ROWS_SHAPES, ids=["%s-%s" % p for p in ROWS_SHAPES])
def test_the_rho_rule_at_iteration_one(name, did):
    """adaptive_rho_interval = 1: the rule runs at iteration 1 on the working variables of the first run.  With the default tolerance and with a
    tolerance MARGIN bounds on either side of new_rho / rho: adapted or not as the reference says; not adapted leaves w, rho and the count exactly as
    a run without the rule; adaptive_rho_max_adaptions = 1 over two intervals adapts once."""
    planned = shown = 0
    for pb in R.handle_problems(name, did):
        one = first_run(pb)
        rl = R.rule(pb, one.x, one.s64, one.wps, R.RHO)
        tols = [R.ADAPT_TOL] + list(R.plan_tolerances(rl, did) or ())
        planned += len(tols) == 3
        for j, tol in enumerate(tols):
            adapted, margin = R.adapts(rl, did, tol)
            assert j == 0 or (adapted == (j == 1) and margin >= R.MARGIN)
            if margin < R.MARGIN:
                continue
            run = solve(pb, max_iter=1, adaptive_rho=1, adaptive_rho_tolerance=tol)
            where = (pb.name, did, "tolerance", tol, "ratio", rl.ratio, "margin", margin)
            assert (run.status, run.iter) == (MAX_ITER, 1), where
            if adapted:
                shown += check_adapted(pb, did, run, one, rl, where)
                if j == 1:
                    capped = solve(pb, max_iter=2, adaptive_rho=1, adaptive_rho_tolerance=tol, adaptive_rho_max_adaptions=1)
                    assert capped.n_rho_updates == 2 and capped.rho_updates[1] == run.rho and capped.rho == run.rho, where + (capped.rho_updates,)
                    assert same_bits(capped.rho_vec, run.rho_vec), where
            else:
                check_not_adapted(run, one, where)
    print("%s %s: %d problems with a tolerance on either side, %d adaptations after which mu from the old rho would have shown" % (name, did, planned, shown))
    assert planned >= 1 and shown >= 1
    report()


@pytest.mark.parametrize("did", DIDS)
def test_the_rule_clamps_to_rho_min_and_rho_max(did):
    """r_prim exactly 0 (A = 0, b = 0, ZeroSet rows): rho_min; a tiny r_dual (P = 0, q = 0, A of order 1e-20: the rule asks for about 4000 rho) with
    rho_max = 100: rho_max.  Both are exact: the reference's interval collapses onto the clamp."""
    t = R.DTYPES[did]
    for name, kw, expect in (("zero_prim", {}, R.RHO_MIN), ("tiny_dual", dict(rho_max=100.0), 100.0)):
        pb = R.special(name, did)
        one = first_run(pb)
        rl = R.rule(pb, one.x, one.s64, one.wps, R.RHO, rho_max=kw.get("rho_max", R.RHO_MAX))
        assert rl.lo == rl.hi == rl.exact == Fraction(float(t(expect))), (name, float(rl.lo), float(rl.hi))
        if name == "zero_prim":
            assert rl.chk.r_prim == 0 and rl.chk.b_prim == 0
        run = solve(pb, max_iter=1, adaptive_rho=1, **kw)
        assert run.n_rho_updates == 2 and run.rho == float(t(expect)) and run.rho_updates[1] == run.rho, (name, did, run.rho_updates)
        assert same_bits(run.rho_vec.astype(np.float64), R.rho_vec(run.rho, pb.cls, did))
        within(run.five, R.termination(pb, run.x, run.s64, run.wps, R.rho_vec(run.rho, pb.cls, did)), "after adaptation", (pb.name, did))


@pytest.mark.parametrize("did", DIDS)
def test_a_residual_of_zero_is_not_below_zero(did):
    """everything zero but P and A: r_prim = r_dual = cost = 0 exactly, at every iteration.  Under eps_abs = eps_rel = 0 the comparison is 0 < 0
    (residuals.jl:100): not converged, whatever the objective gate says; with eps_abs = 1 and |obj_true - cost| = obj_true_tol = 0 it is 0 < 1 and
    0 <= 0 (residuals.jl:136): Solved at the first check.  `<=` for `<`, or `<` for `<=`, fails here."""
    pb = R.clamp_batch(did)[0]
    for kw in ({}, dict(obj_true=0.0, obj_true_tol=0.0)):
        run = solve(pb, max_iter=2, **kw)
        c = R.termination(pb, run.x, run.s64, run.wps, R.rho_vec(R.RHO, pb.cls, did))
        assert c.r_prim == c.r_dual == c.cost == 0 and c.b_prim == c.b_dual == c.b_cost == 0
        assert (run.status, run.iter, run.five) == (MAX_ITER, 2, [0.0] * 5), (did, kw, run.status, run.iter, run.five)
    run = solve(pb, max_iter=2, eps_abs=1.0, obj_true=0.0, obj_true_tol=0.0)
    assert (run.status, run.iter, run.five) == (SOLVED, 1, [0.0] * 5), (did, run.status, run.iter, run.five)
