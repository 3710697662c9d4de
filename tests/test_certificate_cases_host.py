"""The cases and the reference of tests/certificate_cases.py on the CPU (no GPU): what test_gpu_certificates.py relies on.

  * for every member, the definition-level reference (long double) and the oracle's is_primal_infeasible / is_dual_infeasible, applied in the
    reference's order, give the expected status -- on the Float64 numbers and on the Float32 numbers of the case;
  * every member is a tie or decisive: every comparison the evaluation goes through is exact in the type under test or at least MARGIN rounding bounds
    away from its threshold; a tie's deciding comparison is exact and within one ulp of its threshold;
  * every gate and every cone kind has members that pass it and members that fail it, in both certificates where it occurs in both;
  * each mutation of the scaling case (E for Einv, D for Dinv, c = 1, 1 / c, the two tolerances exchanged) flips the members that name it;
  * at most 10 % of the 3-d cone draws are dropped and both verdicts stay;
  * the sizes are the ones the kernels' constants ask for (read from csrc/internal.h)."""
import math
import os
import re

import numpy as np
import pytest

from oracle import cosmo_oracle as O
from tests import certificate_cases as C
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [(n, d) for n in C.CASES for d in (("f64", "f32") if C.float32_runs(n) else ("f64",))]
IDS = ["%s-%s" % p for p in PARAMS]


def _oracle_status(cs, mb):
    """solver.jl:336-347: the primal certificate first"""
    dtype = C.DTYPES[cs.dtype_id]
    rd = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)
    cones = util.oracle_cones(util.projection_sets(cs.cones))
    for oc, c in zip(cones, cs.cones):
        if c.kind == C.BOX:
            oc.l, oc.u = rd(c.l), rd(c.u)
        if c.kind in (C.POW, C.DUAL_POW):
            oc.alpha = float(rd(c.alpha))
    D, E = rd(cs.D), rd(cs.E)
    sm = O.ScaleMatrices(D, 1.0 / D, E, 1.0 / E, float(cs.c), 1.0 / float(cs.c))
    st = O.Settings(eps_prim_inf=C.EPS_PRIM_INF, eps_dual_inf=C.EPS_DUAL_INF)
    ops = O.Operators(cs.P.astype(dtype).astype(np.float64).tocsc(), cs.A.astype(dtype).astype(np.float64).tocsc())
    with np.errstate(all="ignore"):
        if O.is_primal_infeasible(rd(mb.dy), ops, rd(cs.b), cones, sm, st):
            return C.PRIMAL
        if O.is_dual_infeasible(rd(mb.dx), ops, rd(cs.q), cones, sm, st):
            return C.DUAL
    return C.UNDETERMINED


def test_the_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "cosmo.jl_amd", "csrc", "internal.h")).read()
    got = {k: int(re.search(r"#define\s+%s\s+(\d+)" % k, src).group(1)) for k in ("COSMO_BS", "COSMO_MAX_PARTIALS", "COSMO_NNZ_PER_BLOCK")}
    assert got == dict(COSMO_BS=C.COSMO_BS, COSMO_MAX_PARTIALS=C.COSMO_MAX_PARTIALS, COSMO_NNZ_PER_BLOCK=C.COSMO_NNZ_PER_BLOCK)
    big = C.case("reductions_big")
    assert big.n + big.m == C.COSMO_BS * C.COSMO_MAX_PARTIALS + 1000 and big.m > C.COSMO_BS * C.COSMO_MAX_PARTIALS and not big.batch
    assert C.case("reductions_300").n + C.case("reductions_300").m == 300
    rb = C.case("reductions_batch")
    assert (rb.n, rb.m) == (600, 4000) and rb.batch and not rb.handle
    for cs in (big, rb):
        counts = np.diff(cs.A.tocsc().indptr)
        assert counts.max() == 3000 > C.COSMO_NNZ_PER_BLOCK and (np.diff(cs.A.tocsr().indptr) == 1).all()      # one long [P | A'] row, one nonzero per row of A
    assert (C.case("gates").n, C.case("gates").m, C.case("gates").c) == (4, 6, 8.0)
    sc = C.case("scaling")
    ex_d, ex_e = np.log2(sc.D), np.log2(sc.E)
    assert (sc.n, sc.m, sc.c) == (40, 60, 8.0) and (ex_d == np.round(ex_d)).all() and (ex_e == np.round(ex_e)).all()
    assert max(np.abs(ex_d).max(), np.abs(ex_e).max()) <= 6 and len(set(ex_d)) > 5 and len(set(ex_e)) > 5
    assert C.EPS_PRIM_INF == 2.0 ** -10 and C.EPS_DUAL_INF == 2.0 ** -8


def test_the_cases_are_the_ones_the_gpu_test_needs():
    for mode in ("primal", "dual"):
        assert [c.dim for c in C.case("soc_" + mode).cones if c.kind == C.SOC] == [1, 2, 3, 64, 65, 66, 129, 1000]
        assert sum(c.kind == C.SOC for c in C.case("soc70_" + mode).cones) == 70
        many = C.case("soc16400_" + mode)
        assert sum(c.kind == C.SOC for c in many.cones) == 16400 > 4 * 4096 and {c.dim for c in many.cones if c.kind == C.SOC} == {1, 2} and not many.batch
        sides = lambda name: [(c.side, c.kind) for c in C.case(name + "_" + mode).cones if c.kind in C.PSD]
        assert sorted(s for s, _ in sides("psd_small9")) == [2, 2, 2, 3, 3, 3, 16, 16, 16] and {k for _, k in sides("psd_small9")} == set(C.PSD)
        assert [s for s, _ in sides("psd_mid3")] == [17, 33, 64] and {k for _, k in sides("psd_mid3")} == set(C.PSD)
        assert [s for s, _ in sides("psd_large")] == [65, 130] and [s for s, _ in sides("psd_257")] == [257]
        assert not C.case("psd_large_" + mode).batch and not C.case("psd_257_" + mode).batch
        assert [s for s, _ in sides("psd_side1")].count(1) == 3
        for kind in C.CONE3:
            assert sum(c.kind == kind for c in C.case("cone3_%s_%s" % (kind, mode)).cones) == 300
        kinds = [c.kind for c in C.case("simple_" + mode).cones]
        assert kinds.count(C.BOX) >= 2 and kinds.count(C.ZERO) >= 2 and kinds.count(C.NONNEG) >= 3
    box = [c for c in C.case("simple_finite_primal").cones if c.kind == C.BOX][0]
    assert np.isinf(box.l).any() and np.isinf(box.u).any() and (box.l == box.u).any() and (np.isfinite(box.l) & np.isfinite(box.u) & (box.l < box.u)).any()
    po = C.case("poison")
    flags = [mb.poisoned for mb in po.members]
    assert any(flags[i] and not flags[i - 1] and not flags[i + 1] for i in range(1, len(flags) - 1)) and po.clean == [i for i, f in enumerate(flags) if not f]
    assert any(np.isnan(mb.dy).any() and mb.expected == C.DUAL for mb in po.members)              # NaN in dy: the dual certificate is still evaluated
    assert all(mb.expected != C.DUAL for mb in po.members if np.isnan(mb.dx).any()) and any(np.isnan(mb.dx).any() for mb in po.members)
    assert any(np.isinf(mb.dy).any() for mb in po.members) and any(np.isinf(mb.dx).any() for mb in po.members)


@pytest.mark.parametrize("name,dtype_id", PARAMS, ids=IDS)
def test_reference_and_oracle_give_the_expected_status(name, dtype_id):
    cs = C.case(name, dtype_id)
    dtype = C.DTYPES[dtype_id]
    assert len({mb.name for mb in cs.members}) == len(cs.members)
    for k, mb in enumerate(cs.members):
        for v in (mb.dx, mb.dy, cs.q, cs.b, cs.D, cs.E, cs.A.data, cs.P.data):                     # every number of the case is a number of the type
            v = np.asarray(v, dtype=np.float64)
            assert np.array_equal(v.astype(dtype).astype(np.float64), v, equal_nan=True), (name, k)
        status, _ = C.verdict(name, dtype_id, k)
        assert status == mb.expected, (name, dtype_id, k, mb.name, "reference", status)
        orc = _oracle_status(cs, mb)
        assert orc == mb.expected, (name, dtype_id, k, mb.name, "oracle", orc)


@pytest.mark.parametrize("name,dtype_id", PARAMS, ids=IDS)
def test_every_member_is_a_tie_or_decisive(name, dtype_id):
    cs = C.case(name, dtype_id)
    dtype = C.DTYPES[dtype_id]
    for k, mb in enumerate(cs.members):
        _, checks = C.verdict(name, dtype_id, k)
        assert mb.kind in ("tie", "decisive")
        close = [ck for ck in checks if ck.ratio < C.MARGIN]
        assert not close, (name, dtype_id, k, mb.name, close)                                    # exact, or MARGIN bounds away: both kinds
        deciding = [ck for ck in checks if mb.deciding in ck.name]
        assert deciding, (name, dtype_id, k, mb.name, mb.deciding, [ck.name for ck in checks])
        if mb.kind == "tie":                                                                     # exact and on its threshold or one ulp to either side
            # one ulp of the largest number that forms the quantity or its threshold (Check.scale): the threshold itself for a scaled norm against eps,
            # tol or x[1] for a second-order cone, the largest term of a sum whose perturbed term is larger than its total
            near = [ck for ck in deciding if ck.bound == 0.0 and abs(ck.value - ck.threshold) <= float(np.spacing(dtype(ck.scale)))]
            assert near, (name, dtype_id, k, mb.name, deciding)


def _all_checks():
    for name, dtype_id in PARAMS:
        cs = C.case(name, dtype_id)
        for k in range(len(cs.members)):
            for ck in C.verdict(name, dtype_id, k)[1]:
                yield name, ck


def test_every_gate_and_every_cone_kind_has_members_of_each_outcome():
    seen = {}
    for name, ck in _all_checks():
        label = ck.name if ck.name in C.GATES else re.sub(r"^cone \d+ ", "", ck.name)
        mode = name.rsplit("_", 1)[-1] if (name.endswith(("_primal", "_dual")) and ck.name not in C.GATES) else ""
        seen.setdefault((label, mode), set()).add(ck.passed)
    for g in C.GATES:
        assert seen[(g, "")] == {True, False}, g
    for mode in ("primal", "dual"):
        for label in ("soc |x[2:]| <= tol + x[1]", "psd lambda_min > -tol", "psd 1x1 x > -tol", "exp -x exp(y/x) - e z <= tol", "exp y exp(x/y) <= z + tol",
                      "pow s^a t^(1-a) >= |w| k - tol", "exp exact comparisons"):
            assert seen.get((label, mode)) == {True, False}, (label, mode, seen.get((label, mode)))
        assert seen.get(("pow exact comparisons", mode)) == {False}                              # s < -tol, t < -tol or a negative base: no closure branch to pass
    for label in ("nonneg min x >= -tol", "box |y| > tol picks u"):
        assert seen.get((label, "primal")) == {True, False}, label
    for label in ("zero max|x| <= tol", "nonneg max x <= tol", "box recc max x <= tol where u = Inf", "box recc min x >= -tol where l = -Inf"):
        assert seen.get((label, "dual")) == {True, False}, label
    # each status from each kind of case
    for name in C.CASES:
        got = {mb.expected for mb in C.case(name).members}
        assert len(got) >= 2, (name, got)


def test_each_scaling_mutation_flips_its_members():
    for dtype_id in ("f64", "f32"):
        cs = C.case("scaling", dtype_id)
        named = set()
        for k, mb in enumerate(cs.members):
            status = C.verdict("scaling", dtype_id, k)[0]
            for mu in C.MUTATIONS:
                mutated, checks = C.evaluate(cs, mb.dx, mb.dy, mutate=(mu,))
                if mu in mb.flips:
                    named.add(mu)
                    assert mutated != status, (dtype_id, k, mb.name, mu)
                    assert all(ck.ratio >= C.MARGIN for ck in checks), (dtype_id, k, mb.name, mu)      # the wrong formula's verdict is as clear as the right one's
        assert named == set(C.MUTATIONS)
        # every place a scaling or a tolerance enters has its member
        want = {"E": 3, "D": 3, "c1": 2, "cinv": 2, "eps": 6}
        for mu, cnt in want.items():
            assert sum(mu in mb.flips for mb in cs.members) >= cnt, mu


def test_the_cone3_draws_keep_both_verdicts_within_the_cap():
    for mode in ("primal", "dual"):
        for kind in C.CONE3:
            cs = C.case("cone3_%s_%s" % (kind, mode))
            drawn, dropped, inside, outside = cs.dropped
            assert drawn == 300 and dropped <= C.CONE3_DROP_CAP * drawn and inside >= 20 and outside >= 20, (kind, mode, cs.dropped)
            at = [int(mb.name.split()[-1]) for mb in cs.members if mb.name.startswith("outside point at cone")]
            assert len(at) >= 20 and max(at) >= 256                                              # a violator in the second trip of a 256-thread loop


def test_the_unsymmetric_blocks_tell_the_upper_triangle_from_the_symmetrised_matrix():
    for mode in ("primal", "dual"):
        cs = C.case("psd_unsym_" + mode)
        v = cs.members[0].dy[:4] if mode == "primal" else -cs.members[0].dx[:4]
        X = v.reshape(2, 2, order="F")
        assert np.linalg.eigvalsh(np.triu(X) + np.triu(X, 1).T).min() > 0 > np.linalg.eigvalsh((X + X.T) / 2).min() + C.EPS_DUAL_INF
        assert cs.members[0].expected != C.UNDETERMINED and cs.members[1].expected == C.UNDETERMINED


def test_float32_is_left_out_only_where_it_cannot_be_decisive():
    """side 257 alone.  A matrix that fails has lambda_min < -tol, so ||X||_F >= |lambda_min| and its distance |lambda_min| - tol from the threshold is
    below 1 / (64 d eps32) bounds: 510 at d = 257.  At d = 130 that figure is 1008: the Float32 members there fail with lambda_min = -0.9 and nothing else
    in the matrix (1003 bounds against the dual tolerance, 1007 against the primal one)."""
    out = [n for n in C.CASES if not C.float32_runs(n)]
    assert sorted(out) == ["psd_257_dual", "psd_257_primal"]
    assert max(c.side for n in C.CASES if C.float32_runs(n) for c in C.case(n).cones if c.kind in C.PSD) == 130
    assert 1 / (64 * 257 * C.EPS32) < C.MARGIN < (0.9 - C.EPS_DUAL_INF) / 0.9 / (64 * 130 * C.EPS32)
