"""Host-side tests of the batch matrix update (cosmo_hip_batch_stage_matrices and its kin): the entry points through header, libraries, ctypes and Julia
glue, and cj.update(model, P=, A=) on a member of a BatchSolver before the batch is on the device.  No GPU."""
import os
import re

import numpy as np
import pytest

import cosmo_jl_amd as cj
from cosmo_jl_amd import _ffi
from tests import batch_update_cases as BC
from tests.test_julia_glue_signatures import glue_ccalls, header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = _ffi.C

NEW = {
    "cosmo_hip_batch_stage_matrices": "batch_stage_matrices!",
    "cosmo_hip_batch_update_matrices": "batch_update_matrices!",
    "cosmo_hip_batch_update_matrices_info": "batch_update_matrices_info",
    "cosmo_hip_batch_get_matrix_values": "batch_get_matrix_values",
    "cosmo_hip_batch_get_image": "batch_get_image",
    "cosmo_hip_batch_group_stage_matrices": "batch_group_stage_matrices!",
}
CTYPE = {"handle": C.c_void_p, "p_void": C.c_void_p, "i64": C.c_int64, "i32": C.c_int32, "p_real": _ffi._PR, "p_i64": _ffi._PI64}


def test_entry_points_in_header_libraries_bindings_and_glue():
    src = open(os.path.join(ROOT, "include", "cosmo_hip.h")).read()
    protos = header_prototypes()
    glue = open(os.path.join(ROOT, "cosmo.jl_amd", "julia", "CosmoHIP.jl")).read()
    bound = {c[0] for c in glue_ccalls()}
    libs = [cj.load_library(), cj.load_library("float32")]
    for name, jl in NEW.items():
        assert re.search(r"^COSMO_HIP_API int32_t %s\(" % name, src, flags=re.M), name
        ret, params = protos[name]
        assert ret == "i32"
        assert name in _ffi.SIGNATURES, name
        assert _ffi.SIGNATURES[name] == (C.c_int32, [CTYPE[p] for p in params]), (name, params)
        for lib in libs:
            assert getattr(lib, name) is not None, name          # exported by both libraries
        assert name in bound and re.search(r"^function %s\(" % re.escape(jl), glue, flags=re.M), name
    for meth in ("stage_matrices", "update_matrices", "update_matrices_info", "get_matrix_values", "get_image"):
        assert callable(getattr(_ffi.Batch, meth))
    assert callable(_ffi.BatchGroup.stage_matrices)
    assert "have no counterpart" not in src


def test_abi_version_is_unchanged():
    src = open(os.path.join(ROOT, "include", "cosmo_hip.h")).read()
    assert _ffi.ABI_VERSION == 1005
    assert re.search(r"#define COSMO_HIP_ABI_VERSION 1005\b", src)


def _bound_models(count=3):
    probs = BC.resident_family(count)
    models = []
    for p in probs:
        md = cj.Model()
        md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], cj.Settings())
        models.append(md)
    return probs, models, cj.BatchSolver(models)


def test_update_before_the_first_optimize_changes_host_data_only():
    probs, models, rb = _bound_models()
    try:
        assert rb.batch is None
        cj.update(models[1], P=probs[1]["P2"], A=probs[1]["A2"])
        cj.update(models[2], A=probs[2]["A2"])
        assert rb.batch is None and all(md.handle is None for md in models)
        assert np.array_equal(models[1].P.data, probs[1]["P2"].data) and np.array_equal(models[1].A.data, probs[1]["A2"].data)
        assert np.array_equal(models[2].A.data, probs[2]["A2"].data) and np.array_equal(models[2].P.data, probs[2]["P"].data)
        assert np.array_equal(models[0].A.data, probs[0]["A"].data)
        assert np.array_equal(models[1].A.indices, probs[1]["A"].indices) and np.array_equal(models[1].P.indptr, probs[1]["P"].indptr)
    finally:
        rb.close()
    assert all(md.resident is None for md in models)


def test_update_on_a_member_refuses_another_pattern():
    probs, models, rb = _bound_models()
    try:
        A3 = probs[0]["A"].tolil(); A3[0, :] = 0.0; A3[0, 1] = 1.0; A3[0, 2] = 1.0; A3[0, 3] = 3.0
        with pytest.raises(ValueError, match="A"):
            cj.update(models[0], A=A3.tocsc())
        with pytest.raises(ValueError, match="P"):
            cj.update(models[0], P=np.eye(models[0].n + 1))
        Az = probs[0]["A2"].copy(); Az.data[0] = 0.0             # explicit zeros are stored entries ...
        cj.update(models[0], A=Az)
        Ae = Az.copy(); Ae.eliminate_zeros()                     # ... dropping one changes the pattern
        with pytest.raises(ValueError, match="A"):
            cj.update(models[0], A=Ae)
        assert np.array_equal(models[0].A.data, Az.data)
    finally:
        rb.close()


def test_an_owner_that_is_no_batch_solver_still_refuses():
    probs, models, rb = _bound_models(1)
    rb.close()
    md = models[0]
    md.resident = (object(), 0)
    for kw in (dict(A=probs[0]["A2"]), dict(P=probs[0]["P2"])):
        with pytest.raises(NotImplementedError, match="resident"):
            cj.update(md, **kw)
    assert np.array_equal(md.A.data, probs[0]["A"].data) and np.array_equal(md.P.data, probs[0]["P"].data)
