"""Resident batches (cj.BatchSolver): update(model, P=, A=) on members of a batch that stays on the device -- new values on the same pattern, applied by
the next optimize() in one copy and one launch (csrc/batch.hip: k_batch_update_matrices) -- checked member by member against a single-problem handle
that goes through the same update and optimize, on the bars of tests/test_gpu_batch_resident.py."""
import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from cosmo_jl_amd.model import _scale_csc
from tests import batch_update_cases as BC
from tests import update_matrix_cases as UC
from tests import util
from tests.test_gpu_batch_resident import TIGHT_CG, _agree

pytestmark = pytest.mark.gpu


def _models(probs, **kw):
    kw.setdefault("kkt_solver", TIGHT_CG)
    st = cj.Settings(**kw)
    out = []
    for p in probs:
        md = cj.Model()
        md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st)
        out.append(md)
    return out


def _single(p, upd, **kw):
    """The single handle's optimize, update, optimize."""
    md = _models([p], **kw)[0]
    r0 = cj.optimize(md)
    cj.update(md, **upd)
    r1 = cj.optimize(md)
    return md, r0, r1


def _updates(probs):
    """a third of the 12 members: A only, P only, both, both and q"""
    return {0: dict(A=probs[0]["A2"]), 1: dict(P=probs[1]["P2"]), 2: dict(P=probs[2]["P2"], A=probs[2]["A2"]),
            3: dict(P=probs[3]["P2"], A=probs[3]["A2"], q=1.2 * probs[3]["q"])}


def _resolve(probs, single_kw, **kw):
    models = _models(probs, **kw)
    upd = _updates(probs)
    with cj.BatchSolver(models) as rb:
        r0 = rb.optimize()
        assert not rb.mixed
        kinfo = rb.batch.kernel_info()
        for k, u in upd.items():
            cj.update(models[k], **u)
        r1 = rb.optimize()
        assert rb.batch.kernel_info() == kinfo               # the same batch and kernel: nothing was set up again
        info = rb.batch.update_matrices_info()
        dev = {k: (rb.batch.get_matrix_values(k, "AT"), rb.batch.get_matrix_values(k, "PT")) for k in upd}
        assert "apply_s" in rb.last_times
    assert info["updates"] == 1 and info["host_rebuilds"] == 0
    for k in range(len(probs)):
        if k in upd:
            _, one0, one1 = _single(probs[k], upd[k], **single_kw)
            _agree(r0[k], one0)
            _agree(r1[k], one1)
            assert abs(r1[k].obj_val - r0[k].obj_val) > 2e-4 * (1 + abs(r0[k].obj_val)), k       # the new values took effect: twice _agree's bar, so agreeing with one1 excludes the stale solve
        else:
            assert r1[k].status == "Solved" and r1[k].iter <= 25, (k, r1[k].iter)   # stops at the first termination check
            assert np.allclose(r1[k].x, r0[k].x, rtol=1e-5, atol=1e-6)
    return models, upd, dev, info


def _scaled_data(M, L, R, c=None):
    M = sp.csc_matrix(M, dtype=np.float64, copy=True); M.sort_indices()
    _scale_csc(M, L, R)
    if c is not None:
        M.data *= c
    return M.data


def test_members_with_new_matrices_match_the_single_handle():
    probs = BC.resident_family()
    kw = dict(device_scaling=False)                          # host Ruiz scaling, as the batch set-up does it
    models, upd, dev, _ = _resolve(probs, kw, **kw)
    for k, u in upd.items():                                 # the host mirror: scaled with the kept ScaleMatrices, the formula of _scale_csc bit for bit
        sm = models[k].sm
        if "A" in u:
            want = _scaled_data(u["A"], sm.E, sm.D)
            assert np.array_equal(models[k].A.data, want) and np.array_equal(dev[k][0], want)
        if "P" in u:
            assert np.array_equal(models[k].P.data, _scaled_data(u["P"], sm.D, sm.D, sm.c))


def test_members_with_new_matrices_and_device_scaling():
    probs = BC.resident_family()
    models, upd, dev, _ = _resolve(probs, {}, batch_device_scaling=True)
    for k, u in upd.items():                                 # raw values on the host, scaled on the device with the batch's D, E, c
        md = models[k]
        assert md.device_scaled
        if "A" in u:
            assert np.array_equal(md.A.data, u["A"].data)
            assert np.array_equal(dev[k][0], _scaled_data(u["A"], md.sm.E, md.sm.D))
        if "P" in u:
            assert np.array_equal(md.P.data, u["P"].data)


def test_direct_batch_refactors_the_updated_members():
    probs = BC.resident_family()
    kw = dict(kkt_solver=cj.QdldlKKTSolver, device_scaling=False)
    _, upd, _, info = _resolve(probs, kw, direct_batch=True, **kw)
    assert info["factorizations"] == len(upd)


def test_group_updates_a_class_member_and_an_own_handle_member():
    rng = np.random.default_rng(12)
    small = [util.random_qp(rng, 30, 4, 20, 40) for _ in range(3)]
    big = util.random_qp(np.random.default_rng(3), 20, 0, 0, 0, psd_tri_dims=(70,), p_shift=1.0)      # the batch kernels refuse a PSD cone of side 70
    probs = [small[0], big, small[1]]
    for p in probs:
        L = sp.tril(p["P"], k=-1)
        p["P"] = (L + L.T + sp.diags(p["P"].diagonal())).tocsc(); p["P"].sort_indices(); p["A"].sort_indices()
    upd = {0: dict(P=UC.perturbed_psd(probs[0]["P"], rng), A=UC.perturbed(probs[0]["A"], rng, lo=0.95, hi=1.05)),
           1: dict(P=UC.perturbed_psd(probs[1]["P"], rng, lo=0.5, hi=0.8))}
    kw = dict(decompose=False, kkt_solver=cj.CGIndirectKKTSolver, device_scaling=False)
    models = _models(probs, **kw)
    with cj.BatchSolver(models) as rb:
        r0 = rb.optimize()
        assert rb.mixed
        _, _, modes = rb.batch.class_info(with_modes=True)
        assert modes.tolist() == [0, 1, 0]
        for k, u in upd.items():
            cj.update(models[k], **u)
        r1 = rb.optimize()
    for k, p in enumerate(probs):
        _, one0, one1 = _single(p, upd.get(k, {}), **kw)
        for r, one in ((r0[k], one0), (r1[k], one1)):
            assert r.status == one.status == "Solved", (k, r.status, one.status)
            assert abs(r.obj_val - one.obj_val) <= 1e-4 * (1 + abs(one.obj_val)), (k, r.obj_val, one.obj_val)
        if k in upd:
            assert abs(r1[k].obj_val - r0[k].obj_val) > 2e-4 * (1 + abs(r0[k].obj_val)), k        # both kinds of member took the new values (twice the bar above)
    assert r1[2].iter <= 25                                  # not updated: converged at the first check
