"""CPU tests of the resident batch (cosmo_jl_amd.BatchSolver, csrc/batch.hip: cosmo_hip_batch_stage_qb / apply_updates / warm_restart): the new entry
points are declared, exported by both libraries and bound with the header's signatures; update!'s argument checks (src/interface.jl:187-211) and the
BatchSolver's own checks raise before anything reaches a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from cosmo_jl_amd import _ffi as F
from tests.test_chordal_host import _equivalence_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cosmo_hip_batch_set_scaling_full", "cosmo_hip_batch_stage_qb", "cosmo_hip_batch_apply_updates", "cosmo_hip_batch_update_qb",
       "cosmo_hip_batch_warm_restart", "cosmo_hip_batch_get_qb", "cosmo_hip_batch_group_stage_qb", "cosmo_hip_batch_group_apply_updates",
       "cosmo_hip_batch_group_warm_restart", "cosmo_hip_batch_group_get_qb"]


def _model(n=6, m=5, seed=0):
    rng = np.random.default_rng(seed)
    md = cj.Model()
    md.set(sp.identity(n, format="csc"), rng.standard_normal(n), sp.random(m, n, density=0.5, random_state=seed, format="csc") + sp.eye(m, n),
           np.abs(rng.standard_normal(m)), [cj.ZeroSet(2), cj.Nonnegatives(m - 2)])
    return md


@pytest.mark.parametrize("path", [F.LIB_PATH, F.LIB_PATH_F32])
def test_resident_entry_points_are_declared_exported_and_bound(path):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cosmo_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(path)
    for nm in NEW:
        assert re.search(r"COSMO_HIP_API\s+int32_t\s+%s\s*\(" % nm, src), nm
        assert hasattr(lib, nm), nm
        assert nm in F.SIGNATURES, nm


def test_update_checks_follow_the_reference():
    md = cj.Model()
    with pytest.raises(RuntimeError, match="assembled"):
        cj.update(md, q=np.zeros(3))
    md = _model()
    with pytest.raises(ValueError, match="dimension of q"):
        cj.update(md, q=np.zeros(md.n + 1))
    with pytest.raises(ValueError, match="dimension of b"):
        cj.update(md, b=np.zeros(md.m - 1))
    A, b, q, kinds, dims = _equivalence_problem(144545)
    dec = cj.Model()
    dec.set(sp.csc_matrix((1, 1)), q, A, b, [cj.PsdConeTriangle(10), cj.ZeroSet(2), cj.PsdConeTriangle(10), cj.PsdConeTriangle(6)])
    cj.model._chordal_decomposition(dec)
    assert dec.chordal is not None
    with pytest.raises(RuntimeError, match="Problem vector q can not be updated if the model has been chordally decomposed before."):
        cj.update(dec, q=np.zeros(dec.n))
    with pytest.raises(RuntimeError, match="Problem vector b can not be updated"):
        cj.update(dec, b=np.zeros(dec.m))
    with pytest.raises(ValueError, match="chordally decomposed"):
        cj.BatchSolver([dec])


def test_batch_solver_binding_and_its_own_checks():
    class TwoRanks:
        def get_world_size(self):
            return 2
    a, b = _model(seed=1), _model(seed=2)
    with pytest.raises(NotImplementedError, match="not sharded"):
        cj.BatchSolver([a, b], dist=TwoRanks())
    with pytest.raises(RuntimeError, match="assembled"):
        cj.BatchSolver([a, cj.Model()])
    with pytest.raises(ValueError, match="twice"):
        cj.BatchSolver([a, a])
    with pytest.raises(ValueError, match="empty"):
        cj.BatchSolver([])
    rb = cj.BatchSolver([a, b])
    assert a.resident == (rb, 0) and b.resident == (rb, 1) and rb.batch is None
    with pytest.raises(ValueError, match="at most one resident batch"):
        cj.BatchSolver([b])
    with pytest.raises(ValueError, match="warm_start"):
        rb.optimize(warm_start="nowhere")
    q = np.arange(a.n, dtype=float)
    cj.update(a, q=q)                                     # before the first optimize: only the host data changes (set-up uploads it)
    assert np.array_equal(a.q, q)
    with pytest.raises(ValueError, match="dimension of b"):
        cj.update(b, b=np.zeros(b.m + 2))
    rb.close()
    assert a.resident is None and b.resident is None
    cj.BatchSolver([a]).close()                           # free to join another batch now
