"""Device Ruiz equilibration of batches (Settings.batch_device_scaling; csrc/batch_ruiz.hip: k_batch_ruiz, one workgroup per member, one launch).

  * every case of tests/batch_scaling_cases.py through `_ffi.Batch` against the host `scale_ruiz` on copies: D, E, c, the scaled P and A values, q, b, the
    Box bounds and the rho classes -- bit for bit where nothing in the case depends on the order of a sum (the bitwise class), else within the bound of
    that module; `get_scaled_problem` succeeding shows that the three staged copies of every value agree in every bit;
  * slot independence, the two work-vector routes, bad calls;
  * optimize_batch / BatchSolver with the field on against the field off and against single-handle solves, the models' state, re-entry, and the host path
    for an asymmetric P."""
import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from tests import batch_scaling_cases as BC
from tests.test_gpu_batch_resident import _agree, _single

pytestmark = pytest.mark.gpu

TIGHT_CG = cj.with_options(cj.CGIndirectKKTSolver, tol_constant=1e-10, tol_exponent=0.0)


def _device_scale(probs, scaling, dtype, finalize=True):
    """the staged members scaled by the device pass: (per member dict like BC.host_scale's plus rho classes, ruiz_info)"""
    st = BC.settings(scaling)
    n, m = probs[0]["A"].shape[1], probs[0]["A"].shape[0]
    B = cj._ffi.Batch(len(probs), n, m, dtype=dtype)
    try:
        bl, bu = [], []
        for k, p in enumerate(probs):
            B.set_problem(k, p["P"], p["q"], p["A"], p["b"])
            bl += [K.l for K in p["sets"] if K.kind == cj._ffi.BOX]; bu += [K.u for K in p["sets"] if K.kind == cj._ffi.BOX]
        sets = probs[0]["sets"]
        nbox = sum(K.dim for K in sets if K.kind == cj._ffi.BOX)
        with np.errstate(over="ignore"):
            B.set_cones([K.kind for K in sets], [K.dim for K in sets], np.concatenate(bl) if bl else None, np.concatenate(bu) if bu else None,
                        cone_param=[getattr(K, "alpha", 0.0) for K in sets])
        B.scale_ruiz(scaling, st.MIN_SCALING, st.MAX_SCALING)
        info = B.ruiz_info()
        out = []
        for k, p in enumerate(probs):
            D, E, c = B.get_scaling(k)
            Pv, Av, q, b, l, u = B.get_scaled_problem(k, sp.csc_matrix(p["P"]).nnz, sp.csc_matrix(p["A"]).nnz, nbox)     # raises if the three copies differ
            out.append(dict(D=D, E=E, c=np.dtype(dtype).type(c), P=Pv, A=Av, q=q, b=b, box_l=l, box_u=u))
        if finalize:
            B.set_params(cj.model._params_from_settings(None, cj.Settings(scaling=scaling)))
            for k in range(len(probs)):
                out[k]["cls"] = B.get_rho_classes(k)
        return out, info
    finally:
        B.close()


@pytest.mark.parametrize("name,scaling,dtype", BC.runs(), ids=lambda v: getattr(v, "__name__", str(v)))
def test_device_pass_against_the_host(name, scaling, dtype):
    probs = BC.batch(name)
    ref, _, _, bitwise = BC.reference(name, scaling, dtype)
    dev, info = _device_scale(probs, scaling, dtype)
    assert info["members"] == len(probs) and info["rounds"] == scaling
    u = np.finfo(dtype).eps / 2
    print("%s scaling=%d %s: %s class, device vs host %.1f u" % (name, scaling, np.dtype(dtype).name, "bitwise" if bitwise else "bounded",
                                                                 max(BC.spread(d, r) for d, r in zip(dev, ref)) / u))
    st = BC.settings(scaling)
    for k, (p, d, r) in enumerate(zip(probs, dev, ref)):
        rtol = BC.bound(p, scaling, dtype)
        for f in BC.FIELDS:
            assert np.asarray(d[f]).dtype == np.asarray(r[f]).dtype, (name, k, f)
            if bitwise:
                assert np.asarray(d[f]).tobytes() == np.asarray(r[f]).tobytes(), (name, k, f)
            else:
                assert BC.close(d[f], r[f], rtol), (name, k, f)
        assert np.array_equal(d["cls"], BC.rho_classes(p, r, st)), (name, k)


def test_a_member_does_not_depend_on_its_slot_or_on_the_batch_size():
    probs = BC.batch("many")
    for dtype in (np.float64, np.float32):
        whole, _ = _device_scale(probs, 10, dtype, finalize=False)
        alone, _ = _device_scale(probs[69:], 10, dtype, finalize=False)
        assert BC.same_bits(whole[69], alone[0])


def test_work_vector_routes():
    _, info = _device_scale(BC.batch("dense_qp_65"), 10, np.float64, finalize=False)
    n, m = 65, 80
    assert info["work_vectors"] == "lds" and info["lds_bytes"] == 8 * (256 + 2 * (n + m))
    _, info = _device_scale(BC.batch("wide"), 1, np.float64, finalize=False)
    assert info["work_vectors"] == "global" and info["lds_bytes"] == 8 * 256


def test_bad_calls():
    p = BC.batch("dense_qp_65")[0]
    sets = p["sets"]

    def staged(P=None, cones=True):
        B = cj._ffi.Batch(1, 65, 80)
        B.set_problem(0, p["P"] if P is None else P, p["q"], p["A"], p["b"])
        if cones:
            B.set_cones([K.kind for K in sets], [K.dim for K in sets])
        return B

    def code_of(fn):
        with pytest.raises(cj.CosmoHipError) as e:
            fn()
        return cj._ffi.ERR_NAMES[e.value.code]
    B = staged()
    B.scale_ruiz(10)
    assert code_of(lambda: B.scale_ruiz(10)) == "INVALID"                     # twice
    B.set_params(cj.model._params_from_settings(None, cj.Settings()))
    assert code_of(lambda: B.scale_ruiz(10)) == "INVALID"                     # after set_params
    assert code_of(lambda: B.get_scaled_problem(0, p["P"].nnz, p["A"].nnz)) == "INVALID"
    B.close()
    B = staged()
    B.set_params(cj.model._params_from_settings(None, cj.Settings()))
    assert code_of(lambda: B.scale_ruiz(10)) == "INVALID"                     # after set_params, never scaled
    assert code_of(B.ruiz_info) == "INVALID"
    B.close()
    B = staged(cones=False)
    assert code_of(lambda: B.scale_ruiz(10)) == "INVALID"                     # before the cones
    B.close()
    B = cj._ffi.Batch(2, 65, 80)
    B.set_problem(0, p["P"], p["q"], p["A"], p["b"])
    B.set_cones([K.kind for K in sets], [K.dim for K in sets])
    assert code_of(lambda: B.scale_ruiz(10)) == "INVALID"                     # a member is missing
    B.close()
    B = staged()
    assert code_of(lambda: B.scale_ruiz(-1)) == "INVALID"
    assert code_of(lambda: B.scale_ruiz(10, 0.0, 1e4)) == "INVALID"
    assert code_of(lambda: B.scale_ruiz(10, 1e-4, 1e-5)) == "INVALID"
    B.scale_ruiz(0)                                                           # no rounds: D = E = 1, c = 1, the data untouched
    D, E, c = B.get_scaling(0)
    assert np.all(D == 1.0) and np.all(E == 1.0) and c == 1.0
    B.close()
    Pa = sp.lil_matrix(p["P"]); Pa[0, 1] += 0.25
    B = staged(P=Pa.tocsc())
    assert code_of(lambda: B.scale_ruiz(10)) == "UNSUPPORTED"                 # an asymmetric P
    B.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
def _models(probs, dtype=np.float64, **kw):
    kw.setdefault("kkt_solver", TIGHT_CG)
    st = cj.Settings(**kw)
    out = []
    for p in probs:
        md = cj.Model(dtype=dtype)
        md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st)
        out.append(md)
    return out


def _on_against_off(probs, **kw):
    off = cj.optimize_batch(_models(probs, **kw))
    models = _models(probs, batch_device_scaling=True, **kw)
    on = cj.optimize_batch(models)
    for md in models:
        assert md.is_scaled and md.device_scaled
    for a, b in zip(on, off):
        _agree(a, b)
    return on, off, models


def test_cg_batch_kernel_form():
    on, _, _ = _on_against_off(BC.socp_small(8), eps_abs=1e-7, eps_rel=1e-7)
    assert all(r.status == "Solved" for r in on)
    assert not cj.model.LAST_BATCH_INFO["mixed"] and cj.model.LAST_BATCH_INFO["kernel_form"].startswith("register")


def test_psd_exponential_and_power_cones_on_the_image_and_the_streaming_form(monkeypatch):
    _on_against_off(BC.psd_exp_pow(8), eps_abs=1e-6, eps_rel=1e-6, max_iter=3000)
    assert cj.model.LAST_BATCH_INFO["kernel_form"] == "lds_image"          # a PSD cone of side 24: no register kernel
    monkeypatch.setenv("COSMO_HIP_BATCH_LDS", "0")                           # read by set_params: no image, the streaming kernel
    _on_against_off(BC.psd_exp_pow(8), eps_abs=1e-6, eps_rel=1e-6, max_iter=3000)
    assert cj.model.LAST_BATCH_INFO["kernel_form"] == "streaming"


def test_direct_batch():
    on, _, _ = _on_against_off(BC.dense_qp_65(8), kkt_solver=cj.QdldlKKTSolver, direct_batch=True, eps_abs=1e-7, eps_rel=1e-7)
    assert all(r.status == "Solved" for r in on)
    assert "direct_info" in cj.model.LAST_BATCH_INFO and cj.model.LAST_BATCH_INFO["kernel_form"] == "streaming"      # the LDL' form is a streaming kernel


def test_accelerated_batch():
    on, _, _ = _on_against_off(BC.dense_qp_65(8), accelerator=cj.AndersonAccelerator, eps_abs=1e-7, eps_rel=1e-7)
    assert all(r.status == "Solved" for r in on)


def test_mixed_list_with_a_member_on_its_own_handle():
    probs = BC.socp_small(4) + BC.psd_side_65(2) + BC.dense_qp_65(4)
    on, _, models = _on_against_off(probs, eps_abs=1e-6, eps_rel=1e-6, max_iter=3000, decompose=False)
    assert cj.model.LAST_BATCH_INFO["mixed"] and cj.model.LAST_BATCH_INFO["own_handle_members"] == 2      # cosmo_hip_scale_ruiz through the group
    for md, p in zip(models, probs):
        assert np.array_equal(md.P.data, sp.csc_matrix(p["P"]).data) and np.array_equal(md.q, (md.sm.D * p["q"]) * md.sm.c)


def test_a_member_of_a_device_scaled_batch_solved_again_on_its_own_handle():
    """optimize_batch leaves device_scaled models without a handle; a later optimize() keeps the scaling and uploads c D P D and E A D"""
    probs = BC.socp_small(4)
    kw = dict(eps_abs=1e-7, eps_rel=1e-7)
    models = _models(probs, batch_device_scaling=True, **kw)
    cj.optimize_batch(models)
    md = models[2]
    assert md.device_scaled and md.handle is None
    sm = md.sm
    md.x[:] = 0.0; md.s[:] = 0.0; md.mu[:] = 0.0          # a cold start, as the fresh solve below
    r = cj.optimize(md)
    assert md.sm is sm and md.handle is not None
    assert np.array_equal(md.P.data, sp.csc_matrix(probs[2]["P"]).data) and np.array_equal(md.A.data, sp.csc_matrix(probs[2]["A"]).data)
    fresh = cj.optimize(_models([probs[2]], device_scaling=False, **kw)[0])
    assert r.status == "Solved"
    _agree(r, fresh)


def test_calls_after_the_pass_that_would_mix_scaled_and_unscaled_staging_are_refused():
    p = BC.batch("clip")[0]
    sets = p["sets"]
    bl = np.concatenate([K.l for K in sets if K.kind == cj._ffi.BOX]); bu = np.concatenate([K.u for K in sets if K.kind == cj._ffi.BOX])
    B = cj._ffi.Batch(1, 33, 40)
    B.set_problem(0, p["P"], p["q"], p["A"], p["b"])
    B.set_cones([K.kind for K in sets], [K.dim for K in sets], bl, bu)
    B.scale_ruiz(10)
    for call in (lambda: B.set_problem(0, p["P"], p["q"], p["A"], p["b"]), lambda: B.set_cones([K.kind for K in sets], [K.dim for K in sets], bl, bu),
                 lambda: B.set_scaling(0, np.ones(33), np.ones(40), 1.0), lambda: B.set_scaling_full(0, np.ones(33), np.ones(33), np.ones(40), np.ones(40), 1.0, 1.0)):
        with pytest.raises(cj.CosmoHipError) as e:
            call()
        assert cj._ffi.ERR_NAMES[e.value.code] == "INVALID"
    B.set_params(cj.model._params_from_settings(None, cj.Settings()))
    B.close()


def test_persistent_kernel_route():
    p = BC.socp_small(1)[0]
    one = cj.optimize(_models([p], eps_abs=1e-7, eps_rel=1e-7, persistent_kernel=True)[0])
    md = _models([p], eps_abs=1e-7, eps_rel=1e-7, persistent_kernel=True, batch_device_scaling=True)[0]
    r = cj.optimize(md)
    assert md.handle is None and md.device_scaled
    _agree(r, one)


def _solve_update_solve_again(probs, new_q, new_b, check_state=False, **kw):
    """BatchSolver: solve, update half of the members, solve again, close; then the same models through optimize_batch once more"""
    models = _models(probs, **kw)
    with cj.BatchSolver(models) as rb:
        r0 = rb.optimize()
        if check_state:                                      # the single handle's device_scaled state
            for md, p in zip(models, probs):
                assert md.is_scaled and md.device_scaled
                assert np.array_equal(md.P.data, sp.csc_matrix(p["P"]).data) and np.array_equal(md.A.data, sp.csc_matrix(p["A"]).data)
                assert np.array_equal(md.q, (md.sm.D * p["q"]) * md.sm.c) and np.array_equal(md.b, md.sm.E * p["b"])
        for k in new_q:
            cj.update(models[k], q=new_q[k], b=new_b[k])
        r1 = rb.optimize()
    sms = [md.sm for md in models]
    r2 = cj.optimize_batch(models)                           # re-entry: warm-started from the models' solution, the scaling kept
    assert all(md.sm is sm for md, sm in zip(models, sms))
    return r0, r1, r2


def test_resident_batch_model_state_and_reentry():
    probs = BC.socp_small(8)
    kw = dict(eps_abs=1e-7, eps_rel=1e-7)
    rng = np.random.default_rng(7)
    new_q = {k: probs[k]["q"] * (1.0 + 0.1 * rng.standard_normal(probs[k]["q"].size)) for k in range(0, 8, 2)}
    new_b = {k: probs[k]["b"] + 0.05 * np.abs(probs[k]["b"]) * (np.arange(probs[k]["b"].size) % 19 == 0) for k in range(0, 8, 2)}     # the cones' first rows: still strictly feasible
    r0, r1, r2 = _solve_update_solve_again(probs, new_q, new_b, check_state=True, batch_device_scaling=True, **kw)
    for k, p in enumerate(probs):
        _, s0, s1 = _single(p, q=new_q.get(k), b=new_b.get(k), **kw)
        _agree(r0[k], s0)
        _agree(r1[k], s1)
    # re-entry: a device-scaled model keeps D, E, c and is uploaded with c D P D and E A D formed on the host -- the same solve as the host-scaled
    # models' second optimize_batch, and the solution of the resident batch's last solve
    _, _, h2 = _solve_update_solve_again(probs, new_q, new_b, **kw)
    for k in range(len(probs)):
        _agree(r2[k], h2[k])
        assert r2[k].status == r1[k].status == "Solved"
        assert abs(r2[k].obj_val - r1[k].obj_val) <= 1e-4 * (1 + abs(r1[k].obj_val))
        for a, c in ((r2[k].x, r1[k].x), (r2[k].y, r1[k].y)):
            assert np.max(np.abs(a - c)) <= 1e-2 * max(np.max(np.abs(c)), 1.0)


def test_an_asymmetric_member_sends_the_whole_list_to_the_host_path():
    probs = [dict(p) for p in BC.dense_qp_65(4)]
    Pa = sp.lil_matrix(probs[2]["P"]); Pa[0, 1] += 0.25
    probs[2]["P"] = Pa.tocsc()
    kw = dict(eps_abs=1e-6, eps_rel=1e-6)
    off = cj.optimize_batch(_models(probs, **kw))
    models = _models(probs, batch_device_scaling=True, **kw)
    on = cj.optimize_batch(models)
    for md, a, b in zip(models, on, off):
        assert md.is_scaled and not getattr(md, "device_scaled", False)
        assert a.status == b.status and a.iter == b.iter and a.obj_val == b.obj_val
        assert a.x.tobytes() == b.x.tobytes() and a.y.tobytes() == b.y.tobytes() and a.s.tobytes() == b.s.tobytes()
