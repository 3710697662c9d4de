"""CPU tests of the batch device equilibration's yardstick (tests/batch_scaling_cases.py): which cases depend on the order of a sum at all, how far the
host's own restatements of the two means move the result, and that the bound the GPU test holds the device to covers that spread.  Also the Settings field
and the bindings of the new entry points."""
import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from tests import batch_scaling_cases as BC


@pytest.mark.parametrize("name,scaling,dtype", BC.runs(), ids=lambda v: getattr(v, "__name__", str(v)))
def test_host_restatements_stay_inside_the_bound(name, scaling, dtype):
    probs = BC.batch(name)
    ref, fwd, bwd, bitwise = BC.reference(name, scaling, dtype)
    u = np.finfo(dtype).eps / 2
    worst = max(max(BC.spread(b, a), BC.spread(c, a)) for a, b, c in zip(ref, fwd, bwd))
    print("%s scaling=%d %s: %s class, spread %.1f u, bound %.0f u" % (name, scaling, np.dtype(dtype).name, "bitwise" if bitwise else "bounded", worst / u,
                                                                       BC.bound(probs[0], scaling, dtype) / u))
    if name in BC.MUST_BE_BITWISE:
        assert bitwise, name
    for p, a, b, c in zip(probs, ref, fwd, bwd):
        rtol = BC.bound(p, scaling, dtype)
        for f in BC.FIELDS:
            assert BC.close(b[f], a[f], rtol) and BC.close(c[f], a[f], rtol), (name, f)
            if bitwise:
                assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes() == np.asarray(c[f]).tobytes()


def test_the_bitwise_class_does_not_empty_out():
    for scaling in BC.SCALINGS:
        outside = [name for name in BC.CASES if not BC.reference(name, scaling, np.float64)[3]]
        assert 2 * len(outside) <= len(BC.CASES), outside
        assert not set(outside) & set(BC.MUST_BE_BITWISE), outside


def test_float64_host_scaling_is_what_it_was():
    """the dtype / mean parameters of scale_ruiz leave the default arithmetic alone: the straight-line Float64 restatement of the function's body"""
    p = BC.batch("socp_small")[0]
    st = cj.Settings()
    P = sp.csc_matrix(p["P"], copy=True); A = sp.csc_matrix(p["A"], copy=True); q = p["q"].copy(); b = p["b"].copy()
    sm = cj.model.scale_ruiz(P, q, A, b, [cj.model._copy_set(K) for K in p["sets"]], st)
    assert sm.D.dtype == sm.E.dtype == np.float64 and isinstance(sm.c, float) and isinstance(sm.cinv, float)
    assert sm.cinv == 1.0 / sm.c and np.array_equal(sm.Dinv, 1.0 / sm.D) and np.array_equal(sm.Einv, 1.0 / sm.E)
    r = BC.host_scale(p, st.scaling, np.float64)
    assert np.array_equal(r["D"], sm.D) and np.array_equal(r["E"], sm.E) and float(r["c"]) == sm.c and np.array_equal(r["A"], A.data)
    # the scaled matrix is E A0 D to a few roundings
    A0 = sp.csc_matrix(p["A"])
    assert abs(sp.diags(sm.E) @ A0 @ sp.diags(sm.D) - A).max() <= 64 * np.finfo(np.float64).eps * abs(A).max()


def test_settings_field_and_bindings():
    assert cj.Settings().batch_device_scaling is False
    assert cj.Settings(batch_device_scaling=True).batch_device_scaling is True
    for name in ("cosmo_hip_batch_scale_ruiz", "cosmo_hip_batch_get_scaling", "cosmo_hip_batch_get_scaled_problem", "cosmo_hip_batch_ruiz_info",
                 "cosmo_hip_batch_group_set_device_scaling", "cosmo_hip_batch_group_get_scaling"):
        assert name in cj._ffi.SIGNATURES, name
    for cls, meths in ((cj._ffi.Batch, ("scale_ruiz", "get_scaling", "get_scaled_problem", "ruiz_info")), (cj._ffi.BatchGroup, ("set_device_scaling", "get_scaling"))):
        for mname in meths:
            assert callable(getattr(cls, mname))
    assert cj._ffi.ABI_VERSION == 1005


def test_the_device_pass_applies_only_where_the_single_handle_rule_allows():
    sym = BC.batch("dense_qp_65")[0]
    asym = dict(sym); Pa = sp.lil_matrix(sym["P"]); Pa[0, 1] += 0.25; asym["P"] = Pa.tocsc()

    def models(probs, **kw):
        out = []
        for p in probs:
            md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], cj.Settings(**kw)); out.append(md)
        return out
    applies = cj.model._batch_device_scaling_applies
    assert applies(models([sym, sym], batch_device_scaling=True), cj.Settings(batch_device_scaling=True))
    assert not applies(models([sym, sym]), cj.Settings())
    assert not applies(models([sym, sym], batch_device_scaling=True, scaling=0), cj.Settings(batch_device_scaling=True, scaling=0))
    assert not applies(models([sym, asym], batch_device_scaling=True), cj.Settings(batch_device_scaling=True))
    assert cj.model._is_symmetric(sym["P"]) and not cj.model._is_symmetric(asym["P"])
    # the library's rule is structural as well: a stored zero at (i, j) with nothing at (j, i) takes the host path
    Pz = sp.csc_matrix((np.array([1.0, 0.0, 1.0]), np.array([0, 0, 1]), np.array([0, 1, 3])), shape=(2, 2))
    assert (abs(Pz - Pz.T)).nnz == 0 and not cj.model._is_symmetric(Pz)


def test_a_device_scaled_model_is_uploaded_with_its_scaled_matrices():
    """the re-entry rule: D, E, c are kept and c D P D, E A D are formed once on the host"""
    p = BC.batch("socp_small")[0]
    md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], cj.Settings())
    P0, A0 = md.P.copy(), md.A.copy()
    assert cj.model._upload_matrices(md)[0] is md.P
    r = BC.host_scale(p, 10, np.float64)
    cj.model._adopt_device_scaling(md, r["D"], r["E"], float(r["c"]))
    assert md.is_scaled and md.device_scaled and np.array_equal(md.q, (r["D"] * p["q"]) * float(r["c"])) and np.array_equal(md.b, r["E"] * p["b"])
    Pu, Au = cj.model._upload_matrices(md)
    assert np.array_equal(md.P.data, P0.data) and np.array_equal(md.A.data, A0.data)           # the model's own stay unscaled
    eps = np.finfo(np.float64).eps
    assert np.allclose(Au.data, r["A"], rtol=64 * eps, atol=0) and np.allclose(Pu.data, r["P"], rtol=64 * eps, atol=0)
