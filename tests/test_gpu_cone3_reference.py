"""The projections onto ExponentialCone, PowerCone and their duals (csrc/cone3.h) against a certified reference, on every route that calls them:
Handle.project (k_cone3_project, csrc/cone3.hip) and the streaming, LDS-image (both COSMO_HIP_BATCH_LDSCG settings) and register batch kernels
(batch_project_cone3, csrc/batch.hip) through the one-step machinery of tests/test_gpu_batch_projections.py, in Float64 and in Float32.

Everything expected comes from tests/golden/cone3_reference.npz (tests/cone3_cases.py; tests/test_cone3_cases_host.py proves it on the CPU):

  accuracy    per family, worst max |device - ref| / max(1, ||v||_inf) <= max(4 * cpu_err worst of the family, 16 eps)  (cone3_cases.bound)
  weak        the families on which the reference algorithm itself is far from the projection: parity with the stored CPU run of the same algorithm
              in the same precision, to the 1e-5 of test_projection_matches_oracle
  branches    Handle.project's case per cone: the stored one on branch_interior, the stored one or the one across the boundary on branch_edge*
  Moreau      the dual kind on -v returns -v + (the device's own primal result on v), bit for bit: project_kind computes t + v0 in that order
  finite      every result, Float32 included
  isolation   a NaN in one exponential cone and +inf in one power cone of one member change no other cone of the batch

The observed error / bound is printed per (kind, family, precision, route)."""
import faulthandler

import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from tests import cone3_cases as C3
from tests import projection_cases as S
from tests import test_gpu_batch_projections as BP
from tests import util

pytestmark = pytest.mark.gpu

FORMS = ["streaming", "lds_ldscg1", "lds_ldscg0", "register"]
ROUTES = ["handle"] + FORMS
PARITY = 1e-5
KP = [(k, p) for k in C3.KINDS for p in C3.PRECISIONS]
KP_IDS = ["%s-%s" % kp for kp in KP]


@pytest.fixture(autouse=True)
def _case_time_limit():
    """a case that hangs takes the whole process down instead of holding the GPU (as in test_gpu_batch_projections.py)"""
    faulthandler.dump_traceback_later(BP.CASE_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _plus_zero(rows):
    """k_batch_set_w turns -0.0 into +0.0 on the way in; Handle.project gets the same bits"""
    rows = rows.copy()
    rows[rows == 0] = 0.0
    return rows


def _handle_project(case, dtype, members):
    """Handle.project of the given members: (inputs, results, cases per cone)"""
    sets = util.projection_sets(case.cones)
    h = cj.Handle(0, dtype=dtype)
    try:
        h.set_problem(sp.identity(2, format="csc"), np.zeros(2), sp.csc_matrix((case.m, 2)), np.zeros(case.m))
        h.set_cones([K.kind for K in sets], [K.dim for K in sets], np.zeros(0), np.zeros(0), cone_param=[getattr(K, "alpha", 0.0) for K in sets])
        ins = [_plus_zero(case.members[k].rows.astype(dtype)) for k in members]
        res = [h.project(x) for x in ins]
    finally:
        h.close()
    return ins, [r[0] for r in res], [np.asarray(r[2]) for r in res]


def _batch_project(case, dtype, members, form):
    assert form in BP.variants_of(case), (case.name, form)
    res, _ = BP.project_step(case, members, dtype, form)                      # asserts kernel_info()["form"]
    for sent, got_in, _ in res:
        assert BP.same_bits(got_in, _plus_zero(sent)), (case.name, form)
    return [r[1] for r in res], [r[2] for r in res]


_runs = {}


def device(kind, prec, route):
    """(inputs (N, 3), results (N, 3), cases (N) or None) of all points of one kind in point order, once per route for all tests of this file"""
    key = (kind, prec, route)
    if key not in _runs:
        case, P, dtype = C3.case(kind, prec), C3.points(kind, prec), C3.DTYPES[prec]
        members = tuple(range(C3.MEMBERS))
        if route == "handle":
            ins, outs, brs = _handle_project(case, dtype, members)
            br = np.empty(P.n, dtype=np.int64)
            for k, b in enumerate(brs):
                br[k::C3.MEMBERS] = b
        else:
            ins, outs = _batch_project(case, dtype, members, route)
            br = None
        got_in, out = C3.gather(P, ins), C3.gather(P, outs)
        assert got_in.dtype == out.dtype == np.dtype(dtype)
        assert BP.same_bits(got_in, _plus_zero(P.v.astype(dtype))), key       # the device saw the stored points
        _runs[key] = (got_in, out, br)
    return _runs[key]


def test_the_cases_reach_every_batch_form():
    for kind, prec in KP:
        case = C3.case(kind, prec)
        assert BP.variants_of(case) == FORMS, (kind, prec, case.m)
        assert len(case.members) == C3.MEMBERS and case.m == C3.points(kind, prec).n
    assert BP.variants_of(C3.poison_case("f64")) == FORMS


@pytest.mark.parametrize("kind,prec", KP, ids=KP_IDS)
def test_every_route_meets_the_certified_reference(kind, prec):
    """every family that is not weak, every route: worst error against the certified reference <= max(4 * cpu_err worst, 16 eps); all results finite"""
    P = C3.points(kind, prec)
    bad = []
    for route in ROUTES:
        _, out, _ = device(kind, prec, route)
        assert np.isfinite(out).all(), (kind, prec, route, [P.names[f] for f in np.unique(P.family[~np.isfinite(out).all(axis=1)])])
        err = C3.error(out, P.ref, P.v)
        for nm in (n for n, weak in zip(P.names, P.weak) if not weak):
            idx = P.rows_of(nm)
            ratio = float(err[idx].max()) / C3.bound(kind, nm, prec)
            print("%-8s %-17s %s %-10s error/bound %.3g" % (kind, nm, prec, route, ratio))
            if not ratio <= 1.0:
                i = idx[int(np.argmax(err[idx]))]
                bad.append("%s %s %.3g: v %r alpha %r device %r ref %r cpu %r" % (nm, route, ratio, P.v[i].tolist(), float(P.alpha[i]), out[i].tolist(),
                                                                                  P.ref[i].tolist(), P.cpu[i].tolist()))
    assert not bad, "\n".join(bad)


WEAK_KP = [(k, p) for k, p in KP if C3.weak_families(k)]


@pytest.mark.parametrize("kind,prec", WEAK_KP, ids=["%s-%s" % kp for kp in WEAK_KP])
def test_weak_families_keep_parity_with_the_cpu_run(kind, prec):
    """the families on which the reference algorithm is far from the projection (cone3_cases: WEAK): every route against the stored CPU run of the same
    algorithm in the same precision, to 1e-5 relative.

    This test found the one departure of the port from the CPU run: with powf of the device math library the Float32 result at
    v = (-0.20159173, -1.0564574, 1.0000589), alpha = 0.44860491 (branch_edge_polar, 5.9e-5 outside the polar cone, projection (1.31e-4, 3.07e-5,
    5.89e-5)) was (1.14e-3, 2.69e-4, 2.68e-4), 1.08e-3 = 108 x the bound from the CPU run: Newton's r halves per step towards the root, and below 3e-4
    the last bit of pow() decides where the unconverged iteration ends (NumPy's own float32 power against the correctly rounded one: 1e-4 apart).
    pow_r of cone3.h now evaluates the Float32 power in double and rounds once, as the reference's Float32 `^` does, and so does project_cpu: every
    operation of pow_project is then correctly rounded on both sides (the library is built without contraction or fast-math)."""
    P = C3.points(kind, prec)
    bad = []
    for route in ROUTES:
        _, out, _ = device(kind, prec, route)
        par = C3.error(out, P.cpu, P.v)
        for nm in C3.weak_families(kind):
            idx = P.rows_of(nm)
            ratio = float(par[idx].max()) / PARITY
            print("%-8s %-17s %s %-10s parity/1e-5 %.3g" % (kind, nm, prec, route, ratio))
            if not ratio <= 1.0:
                i = idx[int(np.argmax(par[idx]))]
                bad.append("%s %s %.3g: v %r alpha %r device %r cpu %r ref %r" % (nm, route, ratio, P.v[i].tolist(), float(P.alpha[i]), out[i].tolist(),
                                                                                  P.cpu[i].tolist(), P.ref[i].tolist()))
    print("\n".join(bad))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind,prec", KP, ids=KP_IDS)
def test_every_batch_form_returns_the_bits_of_the_single_problem_projection(kind, prec):
    _, single, _ = device(kind, prec, "handle")
    for form in FORMS:
        _, out, _ = device(kind, prec, form)
        diff = np.flatnonzero(~((BP.bits(out) == BP.bits(single)) | (np.isnan(out) & np.isnan(single))).all(axis=1))
        assert diff.size == 0, (kind, prec, form, diff[:10], out[diff[:3]], single[diff[:3]])


@pytest.mark.parametrize("kind,prec", KP, ids=KP_IDS)
def test_branch_codes(kind, prec):
    P = C3.points(kind, prec)
    _, _, br = device(kind, prec, "handle")
    assert set(np.unique(br)) <= {1, 2, 3, 4}
    idx = P.rows_of("branch_interior")
    assert np.array_equal(br[idx], P.branch[idx]), (kind, prec, idx[br[idx] != P.branch[idx]], br[idx], P.branch[idx])
    for nm in (n for n in P.names if n.startswith("branch_edge")):
        for i in P.rows_of(nm):
            assert P.pair[i, 0] > 0 and br[i] in {int(P.branch[i]), int(P.pair[i, 0]), int(P.pair[i, 1])}, (kind, prec, nm, i, br[i], P.branch[i], P.pair[i],
                                                                                                           P.v[i])


@pytest.mark.parametrize("prec", C3.PRECISIONS)
@pytest.mark.parametrize("primal,dual", [(S.EXP, S.DUAL_EXP), (S.POW, S.DUAL_POW)])
def test_duals_are_the_primal_through_moreau(primal, dual, prec):
    """Proj_K*(w) = w + Proj_K(-w) with w = -v: from the device's own primal result on v, bit for bit"""
    for route in ROUTES:
        v, pv, _ = device(primal, prec, route)
        w, pw, _ = device(dual, prec, route)
        assert np.array_equal(w, -v)
        want = pv + w                                                         # one rounding per entry, as t + v0 in project_kind
        diff = np.flatnonzero(~((BP.bits(pw) == BP.bits(want)) | (np.isnan(pw) & np.isnan(want))).all(axis=1))
        assert diff.size == 0, (primal, prec, route, diff[:10], v[diff[:3]], pw[diff[:3]], want[diff[:3]])


@pytest.mark.parametrize("prec", C3.PRECISIONS)
def test_the_power_cones_mirror_the_sign_of_z(prec):
    """z_sign: (x, y, -z) projects to the mirror image of the projection of (x, y, z), to the last bit (fabs(v.z), z0 * r / az)"""
    for kind in (S.POW, S.DUAL_POW):
        P = C3.points(kind, prec)
        idx = P.rows_of("z_sign")
        for route in ROUTES:
            v, out, _ = device(kind, prec, route)
            a, b = idx[0::2], idx[1::2]
            assert np.array_equal(v[a] * np.array([1, 1, -1], dtype=v.dtype), v[b])
            assert np.array_equal(out[a] * np.array([1, 1, -1], dtype=out.dtype), out[b]), (kind, prec, route)     # equal values: the same bits, +-0 aside


@pytest.mark.parametrize("prec", C3.PRECISIONS)
def test_a_poisoned_cone_stays_alone(prec):
    """member 3 is member 1 with a NaN in its first exponential cone and +inf in its first power cone: every other cone of the batch (0, 3, 2) has the bits
    it has in the batch (0, 1, 2).  All loops of cone3.h are bounded (150, 2000, max_iter): the poisoned cones return, whatever they return."""
    case = C3.poison_case(prec)
    dtype = C3.DTYPES[prec]
    keep = np.ones(case.m, dtype=bool)
    for j in case.poisoned:
        keep[3 * j:3 * j + 3] = False
    assert keep.sum() == case.m - 6
    bad = case.members[3].rows
    assert np.isnan(bad).sum() == 1 and np.isinf(bad).sum() == 1 and np.array_equal(bad[keep], case.members[1].rows[keep])
    _, single, _ = _handle_project(case, dtype, (0, 1, 2, 3))
    assert BP.same_bits(single[3][keep], single[1][keep])
    for form in BP.variants_of(case):
        _, clean = _batch_project(case, dtype, (0, 1, 2), form)
        _, full = _batch_project(case, dtype, (0, 3, 2), form)
        for k in range(3):
            assert BP.same_bits(full[k][keep], clean[k][keep]), (prec, form, k)
            assert np.isfinite(full[k][keep]).all(), (prec, form, k)
            assert BP.same_bits(clean[k], single[k]), (prec, form, k)
        assert BP.same_bits(full[0], clean[0]) and BP.same_bits(full[2], clean[2]), (prec, form)
