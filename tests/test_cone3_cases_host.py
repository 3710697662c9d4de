"""The fixture tests/golden/cone3_reference.npz and the cases of tests/cone3_cases.py on the CPU (no GPU): what test_gpu_cone3_reference.py relies on.

  * every stored reference satisfies the optimality conditions of the projection in float64 (projection_cases.cone3_violation at 1e-12);
  * every family reaches the cases of project! it is named for, all four cases occur in every kind, the pairs of branch_edge* sit on both sides;
  * with mpmath: five points of every family regenerated give the stored reference to one ulp and the stored cpu_err to a factor 1.01;
  * today's oracle reproduces the stored Float64 cpu run, today's cone3_cases.project_cpu the stored Float32 one: the fixture has not drifted from
    the algorithm it measures;
  * project_cpu in float64 is the oracle's algorithm: held to the bound the device is held to;
  * the dual kinds hold the negated points of the primal kinds, their reference is -v + Proj_K(v);
  * the cases deal every family to every member and fit every batch kernel form."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import cosmo_oracle as O
from tests import cone3_cases as C3
from tests import projection_cases as S

KP = [(k, p) for k in C3.KINDS for p in C3.PRECISIONS]
KP_IDS = ["%s-%s" % kp for kp in KP]
OKIND = {S.EXP: O.EXP, S.DUAL_EXP: O.DUAL_EXP, S.POW: O.POW, S.DUAL_POW: O.DUAL_POW}
# the cases of project! a family is there for, counted from the stored (exact) case
FAMILY_CASES = {
    S.EXP: {"uniform": {1, 2, 3, 4}, "branch_interior": {1, 2, 3, 4}, "branch_edge": {1, 2, 3, 4}, "branch_edge_polar": {2, 4}, "y_small": {1, 3, 4},
            "ratio_large": {1, 4}, "scale_1e-6": {4}, "scale_1e-3": {4}, "scale_1e3": {4}, "scale_1e6": {4}},
    S.POW: {"uniform": {1, 2, 4}, "branch_interior": {1, 2, 3, 4}, "branch_edge": {1, 3, 4}, "branch_edge_polar": {2, 4}, "z_tiny": {3, 4},
            "xy_zero": {4}, "z_sign": {4}, "alpha_0.01": {4}, "alpha_0.5": {4}, "alpha_0.99": {4}, "scale_1e-6": {4}, "scale_1e-3": {4},
            "scale_1e3": {4}, "scale_1e6": {4}},
}


def _generator():
    spec = importlib.util.spec_from_file_location("make_fixtures_cone3", os.path.join(os.path.dirname(C3.FIXTURE), "make_fixtures_cone3.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _oracle(kind, v, alpha):
    is_exp = C3.PRIMAL[kind] == S.EXP
    out = np.array(v, dtype=np.float64)
    O.project_cone(out, O.Cone(OKIND[kind], 3, alpha=float(alpha), max_iter=C3.MAX_ITER_EXP if is_exp else C3.MAX_ITER_POW, tol=C3.TOL))
    return out


def _near_member(kind, q, a, tol):
    """q lies within tol (per entry) of the power cone `kind`: its first two entries raised by tol.  x^a y^(1 - a) is not Lipschitz at x = 0 and y = 0, so
    a float64 residual p - v whose small entry was cancelled away (|p_x - v_x| = 1e-40 |v_x|) can miss the membership test by far more than its
    distance from the cone."""
    q = np.array(q, dtype=np.float64) + np.array([tol, tol, 0.0])
    return (S._in_pow if kind == S.POW else S._in_pow_dual)(q, a, tol)


@pytest.mark.parametrize("kind,prec", KP, ids=KP_IDS)
def test_every_stored_reference_satisfies_the_optimality_conditions(kind, prec):
    """p in K, p - v in K*, <p, p - v> = 0 to 1e-12 in float64.  Where the float64 subtraction p - v has lost the entry that decides the membership of
    K_pow* (or of K_pow, for a dual kind) -- at most 6 % of the power-cone points -- p - v is held to lie within 1e-12 of that cone instead."""
    P = C3.points(kind, prec)
    assert np.isfinite(P.ref).all() and np.isfinite(P.v).all()
    near = 0
    for i in range(P.n):
        cone = S.Cone(kind, 3, alpha=float(P.alpha[i]))
        miss = S.cone3_violation(cone, P.v[i], P.ref[i], tol=1e-12)
        if miss:
            assert miss == ["residual_in_dual"] and C3.PRIMAL[kind] == S.POW, (kind, prec, i, P.names[P.family[i]], miss, P.v[i], P.ref[i])
            sc = max(1.0, float(np.max(np.abs(P.v[i]))))
            other = S.DUAL_POW if kind == S.POW else S.POW
            assert _near_member(other, (P.ref[i] - P.v[i]) / sc, float(P.alpha[i]), 1e-12), (kind, prec, i, P.v[i], P.ref[i])
            near += 1
    assert near <= 0.06 * P.n, (kind, prec, near)


@pytest.mark.parametrize("kind,prec", KP, ids=KP_IDS)
def test_every_family_reaches_the_cases_it_is_named_for(kind, prec):
    P = C3.points(kind, prec)
    want = FAMILY_CASES[C3.PRIMAL[kind]]
    assert set(P.names) == set(want)
    for nm in P.names:
        idx = P.rows_of(nm)
        assert len(idx) == 30, (nm, len(idx))
        seen = set(int(b) for b in P.branch[idx])
        assert want[nm] <= seen <= {1, 2, 3, 4}, (kind, prec, nm, seen)
    assert set(int(b) for b in P.branch) == {1, 2, 3, 4}
    # branch_interior: the four cases about equally often; branch_edge*: pairs, one point on each side of the boundary the pair names
    counts = np.bincount(P.branch[P.rows_of("branch_interior")], minlength=5)[1:]
    assert counts.min() >= 7, counts
    for nm in ("branch_edge", "branch_edge_polar"):
        idx = P.rows_of(nm)
        assert (P.pair[idx] > 0).all() and np.array_equal(P.pair[idx[0::2]], P.pair[idx[1::2]])
        if prec == "f64":                                                     # (rounding to Float32 moves a point at relative distance 1e-8 across)
            for a, b in zip(idx[0::2], idx[1::2]):
                assert {int(P.branch[a]), int(P.branch[b])} == set(int(t) for t in P.pair[a]), (kind, nm, a)
        else:
            assert all(int(P.branch[i]) in set(int(t) for t in P.pair[i]) for i in idx)
    others = np.setdiff1d(np.arange(P.n), np.concatenate([P.rows_of("branch_edge"), P.rows_of("branch_edge_polar")]))
    assert not P.pair[others].any()


@pytest.mark.parametrize("kind", C3.KINDS)
def test_the_float32_set_is_the_float64_set_rounded_and_the_duals_are_negated_primals(kind):
    P64, P32 = C3.points(kind, "f64"), C3.points(kind, "f32")
    assert np.array_equal(P32.v, P64.v.astype(np.float32).astype(np.float64)) and np.array_equal(P32.alpha, P64.alpha.astype(np.float32).astype(np.float64))
    assert np.array_equal(P32.family, P64.family) and P32.names == P64.names
    assert (P64.v != P32.v).any()
    for prec in C3.PRECISIONS:
        D, Pp = C3.points(kind, prec), C3.points(C3.PRIMAL[kind], prec)
        if kind != C3.PRIMAL[kind]:
            assert np.array_equal(D.v, -Pp.v) and np.array_equal(D.alpha, Pp.alpha) and np.array_equal(D.branch, Pp.branch)
            # Moreau: Proj_K*(-v) = -v + Proj_K(v); both references were rounded once from 100 digits
            assert np.max(C3.error(D.ref, Pp.ref + D.v, D.v)) <= 2 * S.EPS
        is_pow = C3.PRIMAL[kind] == S.POW
        assert bool(((D.alpha > 0) & (D.alpha < 1)).all()) == is_pow and (is_pow or not D.alpha.any())


@pytest.mark.parametrize("kind,prec", KP, ids=KP_IDS)
def test_the_stored_cpu_run_is_todays_algorithm(kind, prec):
    """Float64: the oracle.  Float32: project_cpu with np.float32 scalars.  Per point, the error against the reference to a factor 1.01 (4 eps aside);
    the stored worsts and the weak marks follow from the stored errors."""
    P = C3.points(kind, prec)
    for i in range(P.n):
        now = _oracle(kind, P.v[i], P.alpha[i]) if prec == "f64" else C3.project_cpu(P.v[i], kind, P.alpha[i], np.float32)[0].astype(np.float64)
        e = float(C3.error(now, P.ref[i], P.v[i])[0])
        assert abs(e - P.cpu_err[i]) <= 0.01 * P.cpu_err[i] + 4 * C3.EPS[prec], (kind, prec, i, P.names[P.family[i]], e, P.cpu_err[i])
    assert np.array_equal(P.cpu_err, C3.error(P.cpu, P.ref, P.v))
    for k, nm in enumerate(P.names):
        assert P.worst[k] == P.cpu_err[P.rows_of(nm)].max()
        assert C3.bound(kind, nm, prec) == max(4 * P.worst[k], 16 * C3.EPS[prec])
    assert C3.weak_families(kind) == [nm for k, nm in enumerate(P.names) if C3.points(kind, "f64").worst[k] > 1e-5]


def test_the_weak_families_are_the_ones_the_case_file_lists():
    assert C3.weak_families(S.EXP) == [] and C3.weak_families(S.DUAL_EXP) == []
    assert C3.weak_families(S.POW) == C3.weak_families(S.DUAL_POW) == ["branch_edge_polar", "xy_zero"]
    for kind in (S.POW, S.DUAL_POW):
        P = C3.points(kind, "f64")
        for nm, lo, hi in (("branch_edge_polar", 5e-5, 1e-4), ("xy_zero", 1e-2, 2e-2)):      # the values in the docstring of cone3_cases
            assert lo < P.worst[P.names.index(nm)] < hi
            assert nm in C3.__doc__
    # every other Float64 worst is far below the mark: no family sits on the edge of being weak
    for kind in C3.KINDS:
        P = C3.points(kind, "f64")
        assert all(w < 1e-6 for w, weak in zip(P.worst, P.weak) if not weak), (kind, P.worst)


@pytest.mark.parametrize("kind", C3.KINDS)
def test_project_cpu_in_float64_is_the_oracles_algorithm(kind):
    """the restatement that gives the Float32 numbers, run in float64: within the device's bound of the reference on every family that is not weak, the
    stored case on branch_interior, the mirror image on z_sign"""
    P = C3.points(kind, "f64")
    out = np.empty_like(P.v)
    br = np.empty(P.n, dtype=np.int64)
    for i in range(P.n):
        out[i], br[i] = C3.project_cpu(P.v[i], kind, P.alpha[i], np.float64)
    err = C3.error(out, P.ref, P.v)
    for nm, weak in zip(P.names, P.weak):
        idx = P.rows_of(nm)
        if weak:
            assert C3.error(out[idx], P.cpu[idx], P.v[idx]).max() <= 1e-5, (kind, nm)
        else:
            assert err[idx].max() <= C3.bound(kind, nm, "f64"), (kind, nm, err[idx].max(), C3.bound(kind, nm, "f64"))
    idx = P.rows_of("branch_interior")
    assert np.array_equal(br[idx], P.branch[idx])
    if C3.PRIMAL[kind] == S.POW:
        idx = P.rows_of("z_sign")
        assert np.array_equal(P.v[idx[0::2]] * [1, 1, -1], P.v[idx[1::2]]) and np.array_equal(out[idx[0::2]] * [1, 1, -1], out[idx[1::2]])


def test_a_sample_regenerated_with_mpmath_reproduces_the_fixture():
    pytest.importorskip("mpmath")
    G = _generator()
    for primal in (S.EXP, S.POW):
        names, family, v64, alpha64, pair, _ = G.build_inputs(primal)
        assert names == C3.points(primal, "f64").names and np.array_equal(family, C3.points(primal, "f64").family)
        assert np.array_equal(pair, C3.points(primal, "f64").pair)
        idx = np.concatenate([np.flatnonzero(family == k)[G.SAMPLE] for k in range(len(names))])
        for kind in (k for k in C3.KINDS if C3.PRIMAL[k] == primal):
            for prec in C3.PRECISIONS:
                P = C3.points(kind, prec)
                cols = G.rows_of(kind, prec, v64, alpha64, idx)
                assert np.array_equal(cols["v"], P.v[idx]) and np.array_equal(cols["alpha"], P.alpha[idx]) and np.array_equal(cols["branch"], P.branch[idx])
                assert np.max(np.abs(cols["ref"] - P.ref[idx]) - np.spacing(np.abs(P.ref[idx]))) <= 0, (kind, prec)             # one ulp
                for k, nm in enumerate(names):                                # the worst over the sample, new against stored
                    sel = family[idx] == k
                    new, old = cols["cpu_err"][sel].max(), P.cpu_err[idx][sel].max()
                    assert abs(new - old) <= 0.01 * old + 4 * C3.EPS[prec], (kind, prec, nm, new, old)


def test_the_cases_are_the_ones_the_gpu_test_needs():
    for kind, prec in KP:
        P, case = C3.points(kind, prec), C3.case(kind, prec)
        assert 600 >= P.n >= 270 and P.n <= 680 and case.m == P.n <= 2040 and len(case.members) == 3       # every batch kernel form takes it
        assert all(c.kind == kind and c.dim == 3 for c in case.cones)
        for k, mb in enumerate(case.members):
            assert np.array_equal(mb.rows.reshape(-1, 3), P.v[k::3]) and mb.branch == [int(b) for b in P.branch[k::3]]
            assert sorted(set(mb.note)) == sorted(P.names)                    # every member sees every family
            assert all(mb.note.count(nm) == 10 for nm in P.names)
            assert np.array_equal([c.alpha for c in case.cones], P.alpha[k::3])
        assert np.array_equal(C3.gather(P, [mb.rows for mb in case.members]), P.v)
        if prec == "f32":
            assert np.array_equal(P.v.astype(np.float32).astype(np.float64), P.v)
    for prec in C3.PRECISIONS:
        case = C3.poison_case(prec)
        kinds = [c.kind for c in case.cones]
        assert [kinds.count(k) for k in C3.KINDS] == [12] * 4 and len(case.members) == 4 and case.m <= 1024
        a, b = case.members[1].rows, case.members[3].rows
        e, p = case.poisoned
        assert kinds[e] == S.EXP and kinds[p] == S.POW and kinds.index(S.EXP) == e and kinds.index(S.POW) == p
        assert np.isnan(b[3 * e:3 * e + 3]).sum() == 1 and np.isposinf(b[3 * p]) and np.isfinite(a).all()
        diff = np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))
        assert sorted(diff) == [3 * e + 1, 3 * p]
        assert all(np.isfinite(mb.rows).all() for mb in case.members[:3])
