"""Residuals, termination and the rho rule of the persistent batch kernels (csrc/batch.hip: the `residuals` lambdas of batch_admm_body -- streaming and
LDS-image kernels, with and without the accelerator, register-CG form -- and of the register kernels -- sliced, long-row and plain instantiations,
<512, 1, 2> and <512, 2, 4>, P in registers or not), one check at a time.

The method is that of tests/test_gpu_residual_checks.py (shared device-side helpers: tests/residual_gpu.py): cosmo_hip_batch_optimize runs init,
then per iteration admm_z, the optional rho rule, the KKT solve and the check; Batch.get_iterates returns the w_prev and s the last check was computed from, and the exact reference of tests/residual_cases.py
is evaluated on those fetched iterates.  Every batch holds three DIFFERENT problems (data a factor 8 apart) under ONE set of parameters: a threshold
placed MARGIN = 10 rounding bounds beside the exact value of one problem decides the other two as well, and each is held to what the reference decides
for it wherever that rests on MARGIN bounds or more.  Every form is asserted through kernel_info().

A batch has no getter for its rho vector: it shows through mu = rho .* (w_prev_s - s), which get_iterates returns after recover_mu! and which must be,
bit for bit, classes x the reported rho applied to the fetched w_prev and s.  Not observable and not compared: w[n:] right after an adaptation.

Every test prints the largest observed error / bound per form, precision and quantity.  The run that introduced this file (MI355X), largest error /
bound of r_prim, r_dual, max_norm_prim, max_norm_dual, cost over the values and the checks after an adaptation, and of the new rho:

  form                 type   r_prim  r_dual  max_p   max_d   cost     new rho
  streaming            f64    0.27    0.11    0.11    0.074   0.0062   0.043
  streaming            f32    0.15    0.068   0.064   0.043   0.014    0.037
  streaming_aa         f64    0.10    0.11    0.11    0.074   0.0062   0.043
  streaming_aa         f32    0.09    0.068   0.064   0.043   0.014    0.018
  lds_bs256            f64    0.27    0.11    0.11    0.074   0.0062   0.043
  lds_bs256            f32    0.15    0.068   0.064   0.043   0.014    0.037
  lds_bs512            f64    0.12    0.087   0.10    0.10    0.032    0.052
  lds_bs512            f32    0.16    0.072   0.13    0.11    0.027    0.066
  lds_bs1024           f64    0.28    0.11    0.11    0.074   0.0062   0.043
  lds_bs1024           f32    0.16    0.078   0.13    0.11    0.014    0.018
  lds_aa               f64    0.098   0.048   0.10    0.046   0.0094   0.013
  lds_aa               f32    0.032   0.064   0.064   0.063   0.012    0.039
  lds_regcg_sorted     f64    0.10    0.048   0.10    0.046   0.0094   0.026
  lds_regcg_sorted     f32    0.15    0.064   0.064   0.12    0.012    0.039
  lds_regcg_unsorted   f64    0.10    0.11    0.11    0.074   0.0062   0.043
  lds_regcg_unsorted   f32    0.15    0.068   0.073   0.043   0.014    0.018
  reg12_sliced         f64    0.24    0.054   0.10    0.092   0.015    0.026
  reg12_plain          f64    0.24    0.054   0.10    0.092   0.015    0.026
  reg12_plain          f32    0.17    0.11    0.094   0.12    0.027    0.060
  reg12_long           f64    0.047   0.17    0.12    0.16    0.0066   0.0039
  reg12_long           f32    0.099   0.088   0.033   0.066   0.0048   0.0086
  reg12_aa             f64    0.10    0.048   0.10    0.046   0.0094   0.026
  reg12_aa             f32    0.15    0.064   0.064   0.12    0.012    0.039
  reg24                f64    0.21    0.076   0.096   0.19    0.0042   0.028
  reg24                f32    0.16    0.048   0.13    0.12    0.0022   0.035
  reg24_aa             f64    0.21    0.076   0.086   0.09    0.0013   0.028
  reg24_aa             f32    0.16    0.03    0.13    0.057   0.0018   0.018

The inf-norms use a fifth to a third of their bounds (rows of 2 to 70 entries: the bound is the worst case of about as many roundings as the error has),
the cost a hundredth (600 to 1000 terms whose errors cancel); nothing is near 1 and nothing below 1e-3, so the bounds are kept as derived."""
import contextlib
import faulthandler
import os
import types
from fractions import Fraction

import numpy as np
import pytest

from tests import residual_cases as R
from tests import residual_gpu as H
from tests.residual_gpu import CASE_LIMIT_S, MAX_ITER, SOLVED, UNSOLVED, F

pytestmark = pytest.mark.gpu

SWITCHES = ("COSMO_HIP_BATCH_LDS", "COSMO_HIP_BATCH_REG", "COSMO_HIP_BATCH_BS", "COSMO_HIP_BATCH_LDSCG", "COSMO_HIP_BATCH_EXT", "COSMO_HIP_BATCH_LDSCG_SORTED",
            "COSMO_HIP_BATCH_SLICED", "COSMO_HIP_BATCH_LONG", "COSMO_HIP_BATCH_STORE_SORTED", "COSMO_HIP_BATCH_SORTED", "COSMO_HIP_BATCH_COLOR")
NO_REG = {"COSMO_HIP_BATCH_REG": "0"}
# name -> (environment, accelerator set (never active), shapes, precisions, what kernel_info must report)
FORMS = {
    "streaming": ({"COSMO_HIP_BATCH_LDS": "0"}, False, ("small", "slots"), ("f64", "f32"), dict(form="streaming")),
    "streaming_aa": ({"COSMO_HIP_BATCH_LDS": "0"}, True, ("small",), ("f64", "f32"), dict(form="streaming")),
    "lds_bs256": (dict(NO_REG, COSMO_HIP_BATCH_BS="256"), False, ("small", "slots"), ("f64", "f32"), dict(form="lds_image")),
    "lds_bs512": (dict(NO_REG, COSMO_HIP_BATCH_BS="512"), False, ("small_pdiag", "reg24_m"), ("f64", "f32"), dict(form="lds_image")),
    "lds_bs1024": (dict(NO_REG, COSMO_HIP_BATCH_BS="1024"), False, ("small", "reg24_n"), ("f64", "f32"), dict(form="lds_image")),
    "lds_aa": (NO_REG, True, ("small",), ("f64", "f32"), dict(form="lds_image")),
    "lds_regcg_sorted": (dict(NO_REG, COSMO_HIP_BATCH_EXT="1"), False, ("small", "slots"), ("f64", "f32"), dict(form="lds_image", sorted_assignment=True)),
    "lds_regcg_unsorted": (dict(NO_REG, COSMO_HIP_BATCH_EXT="1", COSMO_HIP_BATCH_LDSCG_SORTED="0"), False, ("small", "slots"), ("f64", "f32"),
                           dict(form="lds_image", sorted_assignment=False)),
    "reg12_sliced": ({}, False, ("small", "small_pdiag", "slots"), ("f64",), dict(form="register_1_2", sliced=True, long_rows=False)),
    "reg12_plain": ({"COSMO_HIP_BATCH_SLICED": "0"}, False, ("small", "small_pdiag", "slots"), ("f64", "f32"), dict(form="register_1_2", sliced=False, long_rows=False)),
    "reg12_long": ({}, False, ("long64",), ("f64", "f32"), dict(form="register_1_2", sliced=False, long_rows=True)),
    "reg12_aa": ({}, True, ("small", "slots"), ("f64", "f32"), dict(form="register_1_2")),
    "reg24": ({}, False, ("reg24_n", "reg24_m"), ("f64", "f32"), dict(form="register_2_4", sliced=False)),
    "reg24_aa": ({}, True, ("reg24_n",), ("f64", "f32"), dict(form="register_2_4")),
}
COMBOS = [(form, shape, did) for form, (_, _, shapes, dids, _) in FORMS.items() for shape in shapes for did in dids]
COMBO_IDS = ["%s-%s-%s" % c for c in COMBOS]
P_DIAGONAL = ("small_pdiag", "reg24_m")
WORST = {}                                      # (form, precision, kind, quantity) -> worst observed error / bound


@pytest.fixture(autouse=True)
def _case_time_limit():
    """a case that hangs takes the whole process down instead of holding the GPU: nothing runs after a hang"""
    faulthandler.dump_traceback_later(CASE_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@contextlib.contextmanager
def _switches(env):
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def solve(form, pbs, expect=None, **kw):
    """a fresh batch of the problems in the given form, set_iterates, optimize: per problem what it reports and what it leaves behind"""
    env, accelerated, _, _, info_expected = FORMS[form]
    did = pbs[0].dtype_id
    dtype = R.DTYPES[did]
    n, m, nprob = pbs[0].n, pbs[0].m, len(pbs)
    with _switches(env):
        B = F.Batch(nprob, n, m, 0, dtype=dtype)
        try:
            if accelerated:
                B.set_accelerator(start_iter=10 ** 9)                         # before set_params: the AA instantiations, never active
            for k, pb in enumerate(pbs):
                B.set_problem(k, pb.P, pb.q, pb.A, pb.b)
                B.set_scaling_full(k, 1.0 / pb.Dinv, pb.Dinv, 1.0 / pb.Einv, pb.Einv, 1.0 / pb.cinv, pb.cinv)
            kinds, dims, bl, bu = H.cone_args(pbs[0])
            B.set_cones(kinds, dims, np.tile(bl, nprob) if bl.size else None, np.tile(bu, nprob) if bu.size else None)
            B.set_params(H.params(dtype, **kw))
            info = B.kernel_info()
            want = dict(info_expected if expect is None else expect)
            assert {k: info[k] for k in want} == want, (form, pbs[0].name, info)
            B.set_iterates(np.concatenate([pb.x0 for pb in pbs]), np.concatenate([pb.s0 for pb in pbs]), np.concatenate([pb.mu0 for pb in pbs]))
            rs = B.optimize()
            out = []
            for k, (pb, res) in enumerate(zip(pbs, rs)):
                assert np.array_equal(B.get_rho_classes(k), pb.cls)
                w, w_prev, s, mu = B.get_iterates(k)
                out.append(types.SimpleNamespace(
                    status=res.status, iter=res.iter, five=[res.r_prim, res.r_dual, res.max_norm_prim, res.max_norm_dual, res.cost], rho=res.rho,
                    n_rho_updates=res.n_rho_updates, rho_updates=[res.rho_updates[i] for i in range(res.n_rho_updates)], w=w, w_prev=w_prev, s=s, mu=mu,
                    x=w_prev[:n].astype(np.float64), s64=s.astype(np.float64), wps=w_prev[n:].astype(np.float64)))
        finally:
            B.close()
    return out, info


def note(form, did, kind, name, ratio):
    key = (form, did, kind, name)
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def report(form, did):
    print("worst error / bound: " + ", ".join("%s %s %s %s %.3g" % (k + (v,)) for k, v in sorted(WORST.items()) if k[0] == form and k[1] == did))


def within(form, got5, c, kind, where, which=range(5)):
    for k in which:
        val, bound = c.five()[k]
        err = abs(Fraction(float(got5[k])) - val)
        assert err <= Fraction(bound), where + (R.FIVE[k], got5[k], float(val), float(err), bound)
        if bound > 0:
            note(form, where[1], kind, R.FIVE[k], float(err) / bound)


def first_checks(form, pbs):
    """the run with max_iter = 1 and eps = 0, the values it reports against the reference, and the exact check of every problem"""
    did = pbs[0].dtype_id
    runs, info = solve(form, pbs, max_iter=1)
    checks = []
    for pb, run in zip(pbs, runs):
        assert (run.status, run.iter, run.n_rho_updates) == (MAX_ITER, 1, 1), (form, pb.name, run.status, run.iter)
        rv = R.rho_vec(R.RHO, pb.cls, did)
        assert H.same_bits(run.mu, H.recovered_mu(run, rv, did)), (form, pb.name)
        c = R.termination(pb, run.x, run.s64, run.wps, rv)
        within(form, run.five, c, "values", (pb.name, did))
        checks.append(c)
    return runs, checks, info


@pytest.mark.parametrize("form,shape,did", COMBOS, ids=COMBO_IDS)
def test_values_and_termination_decisions(form, shape, did):
    """max_iter = 1: the five reported numbers of every problem within their bounds.  Then, with max_iter = 2, one threshold on either side of the exact
    r_prim, r_dual, r / max_norm and cost of each problem in turn: Solved after 1 iteration with the iterates of the first run bit for bit, or
    Max_iter_reached after 2 with those of a run without thresholds; one problem with a cost beyond 1e20 is Unsolved next to its neighbours."""
    pbs = R.batch_problems(shape, did)
    ones, checks, info = first_checks(form, pbs)
    if form.startswith("reg"):                                                # (a diagonal P moves into registers in the sliced form only: kernel_info)
        assert info["p_in_registers"] == (info["sliced"] and shape in P_DIAGONAL), info
    twos, _ = solve(form, pbs, max_iter=2)
    assert all((r.status, r.iter) == (MAX_ITER, 2) for r in twos)
    sole, flips, held = set(), set(), 0
    for k in range(len(pbs)):
        for label, gate, below, above in R.plan_decisions(checks[k], did):
            for side, prm in (("below", below), ("above", above)):
                verdicts = [R.decided(R.gates(c, did, **prm)) for c in checks]
                assert R.gates(checks[k], did, **prm)[gate][0] == (side == "above")
                runs, _ = solve(form, pbs, max_iter=2, **prm)
                for j, (pb, run, one, two, (solved, margin, failing)) in enumerate(zip(pbs, runs, ones, twos, verdicts)):
                    if margin < R.MARGIN:
                        continue
                    held += 1
                    where = (form, pb.name, did, "straddling", k, label, gate, side, prm, failing, margin)
                    if solved:
                        assert (run.status, run.iter) == (SOLVED, 1), where + (run.status, run.iter, run.five)
                        assert H.same_bits(run.w_prev, one.w_prev) and H.same_bits(run.s, one.s), where
                        within(form, run.five, checks[j], "values", (pb.name, did))
                        if j == k:
                            flips.add(label)
                    else:
                        assert (run.status, run.iter) == (MAX_ITER, 2), where + (run.status, run.iter, run.five)
                        assert H.same_bits(run.w_prev, two.w_prev) and H.same_bits(run.s, two.s) and H.same_bits(run.w, two.w), where
                        if j == k and failing == [gate]:
                            sole.add(gate)
    print("%s %s %s: %d verdicts held, sole failing gates %s, thresholds that turned Solved into Max_iter_reached %s" % (form, shape, did, held, sorted(sole), sorted(flips)))
    assert sole == {"prim", "dual", "obj"} and flips == {"eps_abs", "eps_rel", "obj_true"}, (sole, flips)
    # |cost| > 1e20 in the middle problem only
    mixed = [pbs[0], R.with_huge_q(pbs[1]), pbs[2]]
    runs, _ = solve(form, mixed, max_iter=2, eps_abs=0.0)
    c = R.termination(mixed[1], runs[1].x, runs[1].s64, runs[1].wps, R.rho_vec(R.RHO, mixed[1].cls, did))
    assert abs(c.cost) - Fraction(1e20) > R.MARGIN * Fraction(c.b_cost)
    assert [(r.status, r.iter) for r in runs] == [(MAX_ITER, 2), (UNSOLVED, 1), (MAX_ITER, 2)], [(r.status, r.iter, r.five[4]) for r in runs]
    within(form, runs[1].five, c, "values", (mixed[1].name, did), which=[4])
    for j in (0, 2):
        assert H.same_bits(runs[j].w, twos[j].w) and H.same_bits(runs[j].five, twos[j].five)
    report(form, did)


def check_adapted(form, pb, did, run, one, rl, where):
    t = R.DTYPES[did]
    assert run.n_rho_updates == 2 and run.rho_updates[0] == float(t(R.RHO)) and run.rho_updates[1] == run.rho, where + (run.rho_updates, run.rho)
    assert rl.lo <= Fraction(run.rho) <= rl.hi, where + (run.rho, float(rl.lo), rl.new_rho, float(rl.hi))
    if rl.rel > 0:
        note(form, did, "rho rule", "new_rho", abs(Fraction(run.rho) - rl.exact) / (rl.rel * rl.exact))
    assert H.same_bits(run.w_prev, one.w_prev) and H.same_bits(run.s, one.s), where
    new_rv = R.rho_vec(run.rho, pb.cls, did)
    assert H.same_bits(run.mu, H.recovered_mu(run, new_rv, did)), where         # the rho vector: classes x the reported rho
    after = R.termination(pb, run.x, run.s64, run.wps, new_rv)
    within(form, run.five, after, "after adaptation", (pb.name, did))
    stale = R.termination(pb, run.x, run.s64, run.wps, R.rho_vec(R.RHO, pb.cls, did))
    return abs(stale.r_dual - after.r_dual) > R.MARGIN * Fraction(after.b_dual)


def check_not_adapted(run, one, where):
    assert run.n_rho_updates == 1 and run.rho == one.rho, where + (run.rho_updates,)
    assert H.same_bits(run.w, one.w) and H.same_bits(run.mu, one.mu) and H.same_bits(run.five, one.five), where


@pytest.mark.parametrize("form,shape,did", COMBOS, ids=COMBO_IDS)
def test_the_rho_rule_at_iteration_one(form, shape, did):
    """adaptive_rho_interval = 1: with the default tolerance and with a tolerance on either side of new_rho / rho of each problem in turn, every problem
    adapts or not as the reference says for it; an adaptation reports the new rho within the propagated bound, recovers mu with it at the check that
    follows and leaves w_prev and s alone; no adaptation leaves w, mu, the five numbers and the count as a run without the rule;
    adaptive_rho_max_adaptions = 1 over two intervals adapts once."""
    pbs = R.batch_problems(shape, did)
    ones, _, _ = first_checks(form, pbs)
    rules = [R.rule(pb, one.x, one.s64, one.wps, R.RHO) for pb, one in zip(pbs, ones)]
    tols = [(None, R.ADAPT_TOL)]
    for k, rl in enumerate(rules):
        tols += [(k, t) for t in (R.plan_tolerances(rl, did) or ())]
    planned = shown = adaptations = 0
    capped_with = None
    for k, tol in tols:
        verdicts = [R.adapts(rl, did, tol) for rl in rules]
        runs, _ = solve(form, pbs, max_iter=1, adaptive_rho=1, adaptive_rho_tolerance=tol)
        for j, (pb, run, one, rl, (adapted, margin)) in enumerate(zip(pbs, runs, ones, rules, verdicts)):
            where = (form, pb.name, did, "tolerance", tol, "of problem", k, "ratio", rl.ratio, "margin", margin)
            assert (run.status, run.iter) == (MAX_ITER, 1), where
            if margin < R.MARGIN:
                assert j != k
                continue
            planned += j == k
            if adapted:
                adaptations += 1
                shown += check_adapted(form, pb, did, run, one, rl, where)
                if j == k and capped_with is None:
                    capped_with = (tol, [r.rho for r in runs], [r.n_rho_updates for r in runs])
            else:
                check_not_adapted(run, one, where)
    assert planned >= 2 and adaptations >= 1 and shown >= 1 and capped_with is not None, (planned, adaptations, shown)
    tol, rhos, counts = capped_with
    runs, _ = solve(form, pbs, max_iter=2, adaptive_rho=1, adaptive_rho_tolerance=tol, adaptive_rho_max_adaptions=1)
    for run, rho, count in zip(runs, rhos, counts):
        if count == 2:                                                        # adapted at iteration 1: the cap keeps iteration 2 from adapting again
            assert run.n_rho_updates == 2 and run.rho == rho and run.rho_updates[1] == rho, (form, shape, did, run.rho_updates, rho)
        else:
            assert run.n_rho_updates <= 2
    print("%s %s %s: %d tolerances placed, %d adaptations checked, %d after which mu from the old rho would have shown" % (form, shape, did, planned, adaptations, shown))
    report(form, did)


# every form that can take a batch of n = 12, m = 20: the long-row form needs a row of LONG_ROW = 64 entries, <512, 2, 4> needs n > 512 or m > 1024
CLAMP_FORMS = [(form, did) for form in FORMS if form not in ("reg12_long", "reg24", "reg24_aa") for did in FORMS[form][3]]


@pytest.mark.parametrize("form,did", CLAMP_FORMS, ids=["%s-%s" % c for c in CLAMP_FORMS])
def test_the_rule_clamps_and_a_residual_of_zero_is_not_below_zero(form, did):
    """one batch: a problem whose residuals are exactly 0 (the rule asks for 0: rho_min), one with a tiny r_dual (thousands of rho: rho_max = 100), an
    ordinary one; the two clamps are exact, the reference's interval collapses onto them.  The first problem under eps_abs = eps_rel = 0 is the one
    place where `<` and `<=` part (residuals.jl:100): 0 < 0 does not hold, it runs to max_iter."""
    t = R.DTYPES[did]
    pbs = R.clamp_batch(did)
    expect = {k: v for k, v in FORMS[form][4].items() if k in ("form", "sorted_assignment")}
    ones, _ = solve(form, pbs, expect=expect, max_iter=1, rho_max=100.0)
    runs, _ = solve(form, pbs, expect=expect, max_iter=1, rho_max=100.0, adaptive_rho=1)
    for j, (pb, one, run, want) in enumerate(zip(pbs, ones, runs, (R.RHO_MIN, 100.0, None))):
        rl = R.rule(pb, one.x, one.s64, one.wps, R.RHO, rho_max=100.0)
        where = (form, did, pb.name, run.rho_updates, float(rl.lo), float(rl.hi))
        if want is not None:
            assert rl.lo == rl.hi == Fraction(float(t(want))), where
            assert run.n_rho_updates == 2 and run.rho == float(t(want)) == run.rho_updates[1], where
        adapted, margin = R.adapts(rl, did, R.ADAPT_TOL)
        if margin >= R.MARGIN and adapted:
            check_adapted(form, pb, did, run, one, rl, where)
        elif margin >= R.MARGIN:
            check_not_adapted(run, one, where)
    assert ones[0].five == [0.0] * 5 and not ones[0].w.any()
    twos, _ = solve(form, pbs, expect=expect, max_iter=2)
    c = R.termination(pbs[0], twos[0].x, twos[0].s64, twos[0].wps, R.rho_vec(R.RHO, pbs[0].cls, did))
    assert c.r_prim == c.r_dual == 0 and c.b_prim == c.b_dual == 0
    assert (twos[0].status, twos[0].iter, twos[0].five) == (MAX_ITER, 2, [0.0] * 5), (form, did, twos[0].status, twos[0].iter, twos[0].five)
    # ... and with the objective gate on its threshold, |obj_true - cost| = obj_true_tol = 0, where `<=` does hold (residuals.jl:136): still the residuals' 0 < 0
    tied, _ = solve(form, pbs, expect=expect, max_iter=2, obj_true=0.0, obj_true_tol=0.0)
    assert (tied[0].status, tied[0].iter) == (MAX_ITER, 2)
    open_, _ = solve(form, pbs, expect=expect, max_iter=2, eps_abs=1.0, obj_true=0.0, obj_true_tol=0.0)    # 0 < 1 twice and 0 <= 0: Solved
    assert (open_[0].status, open_[0].iter, open_[0].five) == (SOLVED, 1, [0.0] * 5), (form, did, open_[0].status, open_[0].iter)
