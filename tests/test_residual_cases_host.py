"""The problems and the exact reference of tests/residual_cases.py on the CPU (no GPU): what test_gpu_residual_checks.py and
test_gpu_batch_residual_checks.py rely on.

  * the reference agrees with the oracle's calculate_residuals / max_res_component_norm / calculate_cost within its own rounding bound, scaled and
    unscaled, at the iterates set_iterates loads and at the iterates of the oracle's loop after the initial step and one iteration;
  * the placements hold: the placed term is the strict arg-max of its max-norm at the chosen row, the six terms and the five positions all occur, and
    every shape reaches the code path it is named after (tile counts from build_row_blocks, row lengths against the constants of the kernels);
  * sensitivity: each wrong formula of residual_cases.MUTATIONS moves some reported quantity by more than MARGIN = 10 rounding bounds on at least one
    problem -- a bound loose enough to hide one of them fails here.  The test prints which problem catches which mutation."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from oracle import cosmo_oracle as O
from tests import residual_cases as R
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIDS = ("f64", "f32")


def start(pb, rho=R.RHO):
    """(x, s, w_prev[n:], rho vector) right after set_iterates: w = [x0 ; (1 / rho) mu0 + s0] evaluated in the type (solver.jl:128-129)"""
    t = R.DTYPES[pb.dtype_id]
    rv = R.rho_vec(rho, pb.cls, pb.dtype_id)
    wps = ((t(1.0) / rv.astype(t)) * pb.mu0.astype(t) + pb.s0.astype(t)).astype(np.float64)
    return pb.x0, pb.s0, wps, rv


def oracle_step(pb):
    """(x, s, w_prev[n:], rho vector) of the first check of the oracle's loop: initial step, then one iteration (solver.jl:137-155), rounded to the type"""
    cones = util.oracle_cones(util.projection_sets(pb.cones))
    st = O.Settings(scaling=0, kkt_solver="cg", max_iter=1, check_termination=1, adaptive_rho=False, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9)
    ws = O.Workspace(pb.P, pb.q, pb.A, pb.b, cones, st, x0=pb.x0, s0=pb.s0, mu0=pb.mu0)
    assert np.array_equal(ws.rho_class, pb.cls)
    seen = {}
    ws.optimize(record=lambda it, w, w_prev, s, sol: seen.update(w_prev=w_prev.copy(), s=s.copy()))
    r = lambda a: R.rnd(a, pb.dtype_id)
    return r(seen["w_prev"][:pb.n]), r(seen["s"]), r(seen["w_prev"][pb.n:]), R.rho_vec(R.RHO, pb.cls, pb.dtype_id)


def oracle_five(pb, x, s, wps, rv, unscale):
    ops = O.Operators(pb.P, pb.A)
    sm = O.ScaleMatrices(1.0 / pb.Dinv, pb.Dinv, 1.0 / pb.Einv, pb.Einv, 1.0 / pb.cinv, pb.cinv)
    mu = rv * (wps - s)
    rp, rd = O.calculate_residuals(ops, x, s, mu, pb.q, pb.b, sm, unscale)
    mp, md = O.max_res_component_norm(ops, x, s, mu, pb.q, pb.b, sm, unscale)
    return [rp, rd, mp, md, O.calculate_cost(ops, x, pb.q, pb.cinv if unscale else 1.0)]


def all_problems(did):
    out = []
    for name in R.HANDLE_SHAPES:
        out += R.handle_problems(name, did)
    for name in R.BATCH_SHAPES:
        out += R.batch_problems(name, did)
    return out + [R.special(nm, did) for nm in ("small_norms", "huge_cost", "zero_prim", "tiny_dual")]


def test_the_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "cosmo.jl_amd", "csrc", "internal.h")).read()
    assert int(re.search(r"#define\s+COSMO_NNZ_PER_BLOCK\s+(\d+)", src).group(1)) == R.CHUNKED_ABOVE
    assert int(re.search(r"#define\s+COSMO_BS\s+(\d+)", src).group(1)) == R.TILE_ROWS
    batch = open(os.path.join(ROOT, "cosmo.jl_amd", "csrc", "batch_image.h")).read()     # (shared by the kernels of batch.hip and the image planner)
    assert int(re.search(r"#define\s+LONG_ROW\s+(\d+)", batch).group(1)) == R.LONG_ROW
    api = open(os.path.join(ROOT, "cosmo.jl_amd", "csrc", "api.hip")).read()
    assert "if (nnz_total <= 256LL * 768) tile = 256;" in api and R.SMALL_OPERATOR == 256 * 768 and R.TILE == 256


@pytest.mark.parametrize("did", DIDS)
def test_the_reference_agrees_with_the_oracle_within_its_bound(did):
    worst = [0.0] * 5
    for pb in all_problems(did):
        points = [start(pb), oracle_step(pb)]
        for x, s, wps, rv in points:
            for unscale in (True, False):
                c = R.check(pb, x, s, wps, rv, unscale, unscale, unscale)
                for k, (got, (val, bound)) in enumerate(zip(oracle_five(pb, x, s, wps, rv, unscale), c.five())):
                    err = abs(float(Fraction(got) - val))
                    assert err <= bound, (pb.name, did, unscale, R.FIVE[k], got, float(val), err, bound)
                    if bound > 0:
                        worst[k] = max(worst[k], err / bound)
    print("oracle (Float64 arithmetic) against the exact reference, %s bounds, worst error / bound: %s"
          % (did, ", ".join("%s %.3g" % kv for kv in zip(R.FIVE, worst))))


@pytest.mark.parametrize("did", DIDS)
def test_the_placements_hold_and_the_shapes_reach_their_paths(did):
    terms, positions = set(), set()
    for shapes, get in ((R.HANDLE_SHAPES, R.handle_problems), (R.BATCH_SHAPES, R.batch_problems)):
        for name in shapes:
            for pb in get(name, did):
                if pb.place is None:
                    continue
                term, position, i = pb.place
                c = R.termination(pb, *start(pb))
                group = R.TERMS_PRIM if term in R.TERMS_PRIM else R.TERMS_DUAL
                assert c.norms[term][1] == i and all(c.norms[term][0] > 8 * c.norms[o][0] for o in group if o != term), (pb.name, pb.place, c.norms)
                assert (c.max_norm_prim if term in R.TERMS_PRIM else c.max_norm_dual) == c.norms[term][0]
                ta, tp = R.tiles(pb)
                blocks = ta if term in R.TERMS_PRIM else tp
                size = pb.m if term in R.TERMS_PRIM else pb.n
                if position == "tile_end":
                    assert len(blocks) > 2 and i == blocks[1] - 1 and 0 < i < size - 1
                if position == "idx512":
                    assert i >= 512
                if position == "long":
                    assert i == pb.long[0 if term in R.TERMS_PRIM else 1]
                assert (position, i) != ("first", size - 1) and {"first": i == 0, "last": i == size - 1}.get(position, True)
                if shapes is R.HANDLE_SHAPES:
                    terms.add(term); positions.add(position)
    assert terms == set(R.TERMS_PRIM + R.TERMS_DUAL) and positions == set(R.POSITIONS)
    # the shapes
    ntiles = {name: [tuple(len(t) - 1 for t in R.tiles(pb)) for pb in R.handle_problems(name, did)] for name in R.HANDLE_SHAPES}
    assert all(t == (1, 1) for t in ntiles["tiny"] + ntiles["one_tile"]), ntiles
    assert all(min(t) >= 3 for t in ntiles["multi_tile"]), ntiles
    cap = int(R.HANDLE_ENV["wrapped"]["COSMO_HIP_GRID_CAP"])
    assert all(min(t) > cap for t in ntiles["wrapped"]), ntiles
    for pb in R.handle_problems("long_row", did):
        A, P, AT = pb.csr
        lr, lc = pb.long
        assert np.diff(A.indptr)[lr] > R.CHUNKED_ABOVE and np.diff(AT.indptr)[lc] + np.diff(P.indptr)[lc] > R.CHUNKED_ABOVE
        assert np.sort(np.diff(A.indptr))[-2] <= R.TILE                      # the long row alone takes the chunked path
    for pb in R.handle_problems("empty_rows", did):
        A, P, AT = pb.csr
        assert all(np.diff(A.indptr)[r] == 0 for r in (0, pb.m // 2, pb.m - 1)) and all(np.diff(AT.indptr)[c] == 0 for c in (0, pb.n - 1))
    assert all(pb.m == 0 for pb in R.handle_problems("no_rows", did))
    for name in R.HANDLE_SHAPES:
        for pb in R.handle_problems(name, did):
            if pb.m:
                assert set(pb.cls.tolist()) == {0, 1, 2}, name                 # the three rho classes
    for name in R.BATCH_SHAPES:
        pbs = R.batch_problems(name, did)
        assert len(pbs) == 3 and len({pb.A.nnz for pb in pbs}) + len({float(pb.q[0]) for pb in pbs}) > 3
        for pb in pbs:
            A, P, AT = pb.csr
            longest = max(np.diff(A.indptr).max(), np.diff(AT.indptr).max())
            assert (longest >= R.LONG_ROW) == (name == "long64"), (name, longest)
            assert set(pb.cls.tolist()) == {0, 1, 2}
            diag = all(P.indices[P.indptr[j]:P.indptr[j + 1]].tolist() in ([], [j]) for j in range(pb.n))
            assert diag == name.endswith("pdiag") or name == "reg24_m", name


def _moved(true, mut):
    """the largest |mutated - true| / bound over the five numbers of a check"""
    out = 0.0
    for (a, ba), (b, _) in zip(true.five(), mut.five()):
        d = abs(float(a - b))
        out = max(out, d / ba if ba > 0 else (np.inf if d > 0 else 0.0))
    return out


@pytest.mark.parametrize("did", DIDS)
def test_every_mutation_shows_beyond_ten_bounds_on_some_problem(did):
    pbs = []
    for name in ("tiny", "one_tile", "multi_tile"):
        pbs += R.handle_problems(name, did)
    pbs += [R.special("small_norms", did), R.special("tiny_dual", did)]      # (Float32: only a tiny r_dual / max_norm_dual lets the third 1e-10 show)
    caught = {}
    for pb in pbs:
        for label, (x, s, wps, rv) in (("set_iterates", start(pb)), ("oracle step", oracle_step(pb))):
            true = R.termination(pb, x, s, wps, rv)
            rl = R.rule(pb, x, s, wps, R.RHO)
            new_rv = R.rho_vec(rl.new_rho, pb.cls, did)
            after = R.termination(pb, x, s, wps, new_rv)
            for mu_ in R.MUTATIONS:
                if mu_ in caught:
                    continue
                if mu_.startswith(("drop:", "skip:")):
                    moved = _moved(true, R.termination(pb, x, s, wps, rv, mutate=(mu_,)))
                elif mu_.startswith(("apply:", "no_eps:")):
                    moved = abs(R.rule(pb, x, s, wps, R.RHO, mutate=(mu_,)).new_rho - rl.new_rho) / max(float(rl.rel) * rl.new_rho, 1e-300)
                elif mu_ == "old_rho_mu":                                     # the check after an adaptation with the rho vector from before it
                    moved = _moved(after, true) if (rl.ratio > 2 or rl.ratio < 0.5) else 0.0
                else:                                                         # no_eq / no_min: the rho vector by class, seen through mu at the next check
                    moved = _moved(after, R.termination(pb, x, s, wps, R.rho_vec(rl.new_rho, pb.cls, did, mutate=(mu_,))))
                if moved > R.MARGIN:
                    caught[mu_] = "%s at %s (%.3g bounds)" % (pb.name, label, moved)
    for mu_ in R.MUTATIONS:
        print("%-14s %s: %s" % (mu_, did, caught.get(mu_, "NOT CAUGHT")))
    assert set(caught) == set(R.MUTATIONS), sorted(set(R.MUTATIONS) - set(caught))


@pytest.mark.parametrize("did", DIDS)
def test_the_planned_thresholds_decide_with_ten_bounds_to_spare(did):
    """what the GPU tests rely on when they place thresholds (plan_decisions, plan_tolerances), here on the oracle's iterates: the straddled gate passes
    on one side and fails on the other, MARGIN bounds from its threshold; each of the three gates is the only failing one in some run and every kind of
    threshold turns Solved into not Solved somewhere; a planned adaptive_rho_tolerance adapts on one side only"""
    sole, flips, planned = set(), set(), 0
    for name in ("tiny", "one_tile", "multi_tile", "empty_rows", "no_rows"):
        for pb in R.handle_problems(name, did):
            x, s, wps, rv = oracle_step(pb)
            c = R.termination(pb, x, s, wps, rv)
            for label, gate, below, above in R.plan_decisions(c, did):
                g_lo, g_hi = R.gates(c, did, **below), R.gates(c, did, **above)
                assert not g_lo[gate][0] and g_hi[gate][0], (pb.name, label, gate)
                assert min(float(g[gate][1]) for g in (g_lo, g_hi)) >= R.MARGIN, (pb.name, label, gate)
                solved_lo, margin_lo, failing = R.decided(g_lo)
                assert not solved_lo and margin_lo >= R.MARGIN
                if failing == [gate] and all(mg is None or mg >= R.MARGIN for _, mg in g_lo.values()):
                    sole.add(gate)
                solved_hi, margin_hi, _ = R.decided(g_hi)
                if solved_hi and margin_hi >= R.MARGIN:
                    flips.add(label)
            if pb.m:
                rl = R.rule(pb, x, s, wps, R.RHO)
                plan = R.plan_tolerances(rl, did)
                if plan is not None:
                    planned += 1
                    (a_yes, m_yes), (a_no, m_no) = R.adapts(rl, did, plan[0]), R.adapts(rl, did, plan[1])
                    assert a_yes and not a_no and min(m_yes, m_no) >= R.MARGIN, (pb.name, plan, m_yes, m_no)
    assert sole == {"prim", "dual", "obj"} and flips == {"eps_abs", "eps_rel", "obj_true"} and planned >= 5, (sole, flips, planned)


@pytest.mark.parametrize("did", DIDS)
@pytest.mark.parametrize("shape", list(R.BATCH_SHAPES))
def test_every_batch_shape_can_show_every_gate_and_the_rule(shape, did):
    """the three problems of a batch shape, on the oracle's iterates: among them each gate is the only failing one under some planned threshold, every
    kind of threshold turns Solved into not Solved, and at least two of them leave room for an adaptive_rho_tolerance on either side"""
    pbs = R.batch_problems(shape, did)
    points = [oracle_step(pb) for pb in pbs]
    checks = [R.termination(pb, *pt) for pb, pt in zip(pbs, points)]
    sole, flips = set(), set()
    for c in checks:
        for label, gate, below, above in R.plan_decisions(c, did):
            for prm in (below, above):
                solved, margin, failing = R.decided(R.gates(c, did, **prm))
                if margin >= R.MARGIN and solved:
                    flips.add(label)
                elif margin >= R.MARGIN and failing == [gate]:
                    sole.add(gate)
    planned = sum(R.plan_tolerances(R.rule(pb, pt[0], pt[1], pt[2], R.RHO), did) is not None for pb, pt in zip(pbs, points))
    assert sole == {"prim", "dual", "obj"} and flips == {"eps_abs", "eps_rel", "obj_true"} and planned >= 2, (sole, flips, planned)
