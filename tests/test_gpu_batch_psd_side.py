"""PSD cones of side 65 .. 256 in the persistent batch kernels (Settings.batch_psd_side_max; csrc/psdwg.h: psdwg_jacobi_rounds), one step at a time.

Projections by the one-step method of test_gpu_batch_projections.py (set_iterates, iterate(1), s against projection_cases.ref_psd of the fetched
w_prev[n:] within 64 d eps ||X||_F), the definiteness tests of the certificates through cosmo_hip_batch_check_certificates with the members, verdicts
and margins of certificate_cases.py, and the refusals and the routing of the opt-in.  Everything runs in Float64 and Float32."""
import faulthandler

import numpy as np
import pytest

import cosmo_jl_amd as cj
from tests import batch_psd_side_cases as BP
from tests import certificate_cases as C
from tests import projection_cases as S
from tests import util

pytestmark = pytest.mark.gpu

CASE_LIMIT_S = 120
F = cj._ffi
NAMES = {C.UNDETERMINED: "Undetermined", C.PRIMAL: "Primal_infeasible", C.DUAL: "Dual_infeasible"}
LAYOUTS = [(side, S.PSD_TRI) for side in BP.SIDES] + [(side, S.PSD_SQ) for side in BP.SQUARE_SIDES]
FORMS = [(side, kind, "streaming") for side, kind in LAYOUTS] + [(side, S.PSD_TRI, "lds_image") for side in BP.LDS_SIDES]


@pytest.fixture(autouse=True)
def _case_time_limit():
    """a case that hangs takes the whole process down instead of holding the GPU: nothing runs after a hang"""
    faulthandler.dump_traceback_later(CASE_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.mark.parametrize("dtype_id", ["f64", "f32"])
@pytest.mark.parametrize("side,kind,variant", FORMS, ids=["%d-%s-%s" % f for f in FORMS])
def test_one_projection_of_a_large_cone_meets_the_psd_bound(side, kind, variant, dtype_id):
    """five spectra, two members per batch; a member returns the same bits whatever its place in the batch and whatever the order of the fetches"""
    cs = BP.case(side, kind)
    seen = {}
    worst = 0.0
    for j, members in enumerate(BP.BATCHES):
        out, info = BP.project_step(cs, members, BP.DTYPES[dtype_id], variant, 256, fetch_reversed=bool(j & 1))
        for k, (sent, got_in, got) in zip(members, out):
            if k in seen:
                assert BP.same_bits(seen[k], got), (cs.name, variant, dtype_id, "member", k, "depends on its place in the batch", members)
                continue
            seen[k] = got
            worst = max(worst, BP.check_member(cs, k, dtype_id, variant, sent, got_in, got))
    assert sorted(seen) == list(range(len(BP.SPECTRA)))
    # all negative -> the zero matrix, all positive -> the identity map (to the bound above; the zero matrix exactly: no eigenvalue of G exceeds the shift)
    neg, pos = BP.SPECTRA.index("negdef"), BP.SPECTRA.index("psd")
    assert not seen[neg].any()
    assert seen[pos].any()
    print("side %d %s %s %s: worst error / bound %.3g" % (side, kind, variant, dtype_id, worst))


@pytest.mark.parametrize("dtype_id", ["f64", "f32"])
def test_three_code_paths_in_one_problem(dtype_id):
    """a cone of side 9 (one wave), one of side 40 (one block pair per wave) and one of side 96 (rounds) with simple rows between them"""
    cs = BP.three_paths_case()
    assert sorted(c.side for c in cs.cones if c.kind in S.PSD) == [9, 40, 96]
    out, _ = BP.project_step(cs, (0, 1), BP.DTYPES[dtype_id], "streaming", 256)
    back, _ = BP.project_step(cs, (1, 0), BP.DTYPES[dtype_id], "streaming", 128, fetch_reversed=True)
    for k in (0, 1):
        BP.check_member(cs, k, dtype_id, "streaming", *out[k])
        assert BP.same_bits(out[k][2], back[1 - k][2]), k


@pytest.mark.parametrize("dtype_id", ["f64", "f32"])
@pytest.mark.parametrize("variant", ["streaming", "lds_image"])
def test_side_64_keeps_its_bits_when_the_limit_is_raised(variant, dtype_id):
    """the side-64 triangle case of the existing suite: the same bits with the limit at 256 as at the default"""
    cs = S.case("psd_mid_64_tri")
    members = tuple(range(len(cs.members)))
    base, i0 = BP.project_step(cs, members, BP.DTYPES[dtype_id], variant, 64)
    high, i1 = BP.project_step(cs, members, BP.DTYPES[dtype_id], variant, 256)
    assert i0 == i1
    for k, ((_, in0, s0), (_, in1, s1)) in enumerate(zip(base, high)):
        assert BP.same_bits(in0, in1) and BP.same_bits(s0, s1), (variant, dtype_id, k)
        assert s0.any()


@pytest.mark.parametrize("dtype_id", ["f64", "f32"])
@pytest.mark.parametrize("mode", ["primal", "dual"])
def test_certificates_of_large_cones_return_the_expected_verdicts(mode, dtype_id):
    """in_dual! / in_pol_recc! at sides 65 (triangle) and 129 (square): all members in ONE batch with mixed verdicts, then in reversed order"""
    cs = BP.certificate_case(mode, dtype_id)
    nm = len(cs.members)
    assert nm == 7 and {mb.expected for mb in cs.members} == {C.UNDETERMINED, C.PRIMAL if mode == "primal" else C.DUAL}
    B = BP.certificate_batch(cs, nm, 256)
    try:
        orders = [list(range(nm)), list(range(nm))[::-1]]
        got = [B.check_certificates(np.concatenate([cs.members[k].dx for k in o]), np.concatenate([cs.members[k].dy for k in o])) for o in orders]
    finally:
        B.close()
    for order, g in zip(orders, got):
        wrong = [(k, cs.members[k].name, "expected " + NAMES[cs.members[k].expected], "got " + NAMES.get(v, str(v))) for k, v in zip(order, g)
                 if v != cs.members[k].expected]
        assert not wrong, wrong
    relied = min(ck.ratio for k in range(nm) for ck in C.evaluate(cs, cs.members[k].dx, cs.members[k].dy)[1])
    print("%s %s: %d members, smallest |quantity - threshold| / bound relied on: %.3g" % (cs.name, dtype_id, nm, relied))
    assert relied >= C.MARGIN


def _sdp65(nprob, seed):
    rng = np.random.default_rng(seed)
    return [util.random_qp(rng, 40, 3, 10, 12, soc_dims=(5, 8), psd_tri_dims=(65,), p_shift=1.0) for _ in range(nprob)]


def test_refusals_name_the_limit():
    probs = _sdp65(2, 5)
    with pytest.raises(Exception, match="side <= 64"):                           # the default: unchanged
        cj.model.prepare_batch(BP.models(probs, cj.Settings()), 0)
    B, _ = cj.model.prepare_batch(BP.models(probs, cj.Settings(batch_psd_side_max=128)), 0)
    B.close()
    rng = np.random.default_rng(6)
    p129 = [util.random_qp(rng, 40, 3, 10, 0, psd_tri_dims=(129,), p_shift=1.0, density=0.02) for _ in range(2)]
    with pytest.raises(Exception, match="side <= 128 .side 129"):
        cj.model.prepare_batch(BP.models(p129, cj.Settings(batch_psd_side_max=128)), 0)
    for dtype in (np.float64, np.float32):
        B = F.Batch(2, 4, 65 * 66 // 2, 0, dtype=dtype)
        G = F.BatchGroup(2, 0, dtype=dtype)
        try:
            for side in (63, 257, -1):
                assert F.ERR_NAMES.get(B.lib.cosmo_hip_batch_set_psd_side_max(B._b, side)) == "INVALID"
                assert F.ERR_NAMES.get(G.lib.cosmo_hip_batch_group_set_psd_side_max(G._g, side)) == "INVALID"
            assert F.ERR_NAMES.get(B.lib.cosmo_hip_batch_set_psd_side_max(None, 64)) == "INVALID"
            with pytest.raises(F.CosmoHipError, match="side <= 64 .side 65"):
                B.set_cones([F.PSD_TRIANGLE], [65 * 66 // 2])
            B.set_psd_side_max(64); B.set_psd_side_max(256); B.set_psd_side_max(65)
            G.set_psd_side_max(256)
            B.set_cones([F.PSD_TRIANGLE], [65 * 66 // 2])
            assert F.ERR_NAMES.get(B.lib.cosmo_hip_batch_set_psd_side_max(B._b, 128)) == "INVALID"       # after set_cones
            assert "before batch_set_cones" in B.lib.cosmo_hip_batch_last_error(B._b).decode()
        finally:
            B.close(); G.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_opt_in_keeps_side_65_members_in_the_batch_kernels(dtype):
    """optimize_batch of two side-65 members: own handles at the default, none with the opt-in; both routes solve, objectives within 1e-4 (1 + |obj|)"""
    probs = _sdp65(2, 5)
    kw = dict(decompose=False) if dtype == np.float64 else dict(decompose=False, eps_abs=1e-4, eps_rel=1e-4)
    own = cj.optimize_batch(BP.models(probs, cj.Settings(**kw), dtype))
    info_own = dict(cj.model.LAST_BATCH_INFO)
    kept = cj.optimize_batch(BP.models(probs, cj.Settings(batch_psd_side_max=65, **kw), dtype))
    info_kept = dict(cj.model.LAST_BATCH_INFO)
    assert info_own["mixed"] and info_own["own_handle_members"] == 2, info_own
    assert not info_kept["mixed"] and info_kept["own_handle_members"] == 0 and info_kept["kernel_form"] in ("streaming", "lds_image"), info_kept
    for k, (a, b) in enumerate(zip(own, kept)):
        print("member %d: %s / %s, objective %.9g / %.9g, iterations %d / %d" % (k, a.status, b.status, a.obj_val, b.obj_val, a.iter, b.iter))
        assert a.status == b.status == "Solved", (k, a.status, b.status)
        assert abs(a.obj_val - b.obj_val) <= 1e-4 * (1 + abs(a.obj_val)), (k, a.obj_val, b.obj_val)


def test_a_group_with_the_opt_in_keeps_both_structures_in_batches():
    """two structures (side 65 and side 96) in one list: a batch group; with the limit at 96 both classes run in the batch kernels, with the limit at 65
    the side-96 class keeps its own handles"""
    rng = np.random.default_rng(9)
    probs = _sdp65(2, 7) + [util.random_qp(rng, 40, 3, 10, 0, psd_tri_dims=(96,), p_shift=1.0, density=0.02) for _ in range(2)]
    st = dict(decompose=False, max_iter=200)
    r96 = cj.optimize_batch(BP.models(probs, cj.Settings(batch_psd_side_max=96, **st)))
    info96 = dict(cj.model.LAST_BATCH_INFO)
    r65 = cj.optimize_batch(BP.models(probs, cj.Settings(batch_psd_side_max=65, **st)))
    info65 = dict(cj.model.LAST_BATCH_INFO)
    assert info96["mixed"] and info96["own_handle_members"] == 0, info96
    assert info65["mixed"] and info65["own_handle_members"] == 2, info65
    for a, b in zip(r96[:2], r65[:2]):                                           # the side-65 class runs the same batch kernel in both groups
        assert a.status == b.status and a.iter == b.iter and np.array_equal(a.x, b.x)
    for a, b in zip(r96[2:], r65[2:]):
        assert a.status == b.status, (a.status, b.status)
        assert abs(a.obj_val - b.obj_val) <= 1e-4 * (1 + abs(a.obj_val)), (a.obj_val, b.obj_val)
