"""Whole solves with PSD cones of side 65 .. 256 in the batch kernels (Settings.batch_psd_side_max), modelled on
test_gpu_batch.py::test_batch_of_sdps_with_cones_of_side_17_to_64 with that test's bars.

The workloads were run through the compiled oracle on the CPU first: the eight default-settings instances (seed 6572) end Solved after 100 .. 150
iterations, so the window 0.5 it - 25 <= iter <= 2 it + 25 is [25, 225] .. [50, 325] and not vacuous; the four tight-CG instances (seed 72130) run
their 60 iterations.

Float32: the default-settings leg runs in both precisions (eps 1e-4 in Float32, objective to the 1e-2 the project holds its Float32 batches to against
the Float64 oracle, tests/test_gpu_batch.py); the trajectory bars (1e-3 / 1e-7 / 1e-8 after 60 tight iterations, bit equality of the resident
re-solve) are Float64 statements, the re-solve in Float32 is held to the 4 unit roundoffs of test_gpu_batch_device_io.py."""
import faulthandler
import os
import subprocess

import numpy as np
import pytest
import torch

import cosmo_jl_amd as cj
from oracle import cosmo_oracle as O
from tests import batch_psd_side_cases as BP
from tests import util

pytestmark = pytest.mark.gpu

CASE_LIMIT_S = 300
U32 = 2.0 ** -24


@pytest.fixture(autouse=True)
def _case_time_limit():
    """a case that hangs takes the whole process down instead of holding the GPU: nothing runs after a hang"""
    faulthandler.dump_traceback_later(CASE_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _oracle_c():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "oracle")], check=True, capture_output=True)
    from oracle import cosmo_oracle_c as OC
    return OC


_ref = {}


def _reference(name, probs, st):
    """the compiled oracle on every problem, once"""
    if name not in _ref:
        OC = _oracle_c()
        _ref[name] = [OC.run(O.Workspace(p["P"], p["q"], p["A"], p["b"], util.oracle_cones(p["sets"]), st)) for p in probs]
    return _ref[name]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_default_settings_against_the_compiled_oracle(dtype):
    probs = BP.sdps_default()
    f32 = dtype == np.float32
    kw = dict(eps_abs=1e-4, eps_rel=1e-4) if f32 else {}
    res = cj.optimize_batch(BP.models(probs, cj.Settings(batch_psd_side_max=256, **kw), dtype))
    info = dict(cj.model.LAST_BATCH_INFO)
    assert not info["mixed"] and info["own_handle_members"] == 0, info
    refs = _reference("default32" if f32 else "default", probs, O.Settings(kkt_solver="cg", **kw))
    for k, (r, c) in enumerate(zip(res, refs)):
        print("problem %d: %s / %s, %d / %d iterations, objective %.9g / %.9g" % (k, r.status, c["status"], r.iter, c["iter"], r.obj_val, c["obj_val"]))
        assert r.status == c["status"] == "Solved", (k, r.status, c["status"])
        assert abs(r.obj_val - c["obj_val"]) <= (1e-2 if f32 else 1e-4) * (1 + abs(c["obj_val"])), (k, r.obj_val, c["obj_val"])
        assert 0.5 * c["iter"] - 25 <= r.iter <= 2.0 * c["iter"] + 25, (k, r.iter, c["iter"])


def test_tight_trajectories_against_the_oracle_the_other_form_and_a_single_handle():
    probs = BP.sdps_tight()
    tight = cj.with_options(cj.CGIndirectKKTSolver, tol_constant=1e-10, tol_exponent=0.0)
    st = cj.Settings(kkt_solver=tight, max_iter=60, eps_abs=0.0, eps_rel=0.0, batch_psd_side_max=256)
    st_o = O.Settings(kkt_solver="cg", tol_constant=1e-10, tol_exponent=0.0, max_iter=60, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9)

    def run():
        B, _ = cj.model.prepare_batch(BP.models(probs, st), 0)
        form = B.kernel_info()["form"]
        B.close()
        res = cj.optimize_batch(BP.models(probs, st))
        assert cj.model.LAST_BATCH_INFO["own_handle_members"] == 0 and cj.model.LAST_BATCH_INFO["kernel_form"] == form
        return form, res
    form_s, stream = BP.with_env({"COSMO_HIP_BATCH_LDS": "0"}, run)
    form_d, default = BP.with_env({}, run)
    assert form_s == "streaming"
    refs = _reference("tight", probs, st_o)
    for k, (r, c) in enumerate(zip(stream, refs)):
        devs = [float(np.max(np.abs(v - c[key])) / max(np.max(np.abs(c[key])), 1.0)) for key, v in (("x", r.x), ("s", r.s), ("y", r.y))]
        print("problem %d: x, s, y against the oracle %s" % (k, devs))
        assert r.iter == c["iter"] == 60 and max(devs) <= 1e-3, (k, devs)
    if form_d == "lds_image":                                                     # both forms take the batch: they agree to 1e-8 (the image does not fit: no such leg)
        for k, (r, r2) in enumerate(zip(default, stream)):
            for u, v in ((r.x, r2.x), (r.s, r2.s), (r.y, r2.y)):
                assert np.max(np.abs(u - v)) <= 1e-8 * max(1.0, float(np.max(np.abs(u)))), k
    else:
        assert form_d == "streaming"
        print("the LDS image does not fit (m = %d): no second form to compare" % probs[0]["b"].size)
    single = cj.optimize(BP.models(probs[:1], st)[0])
    dev = float(np.max(np.abs(single.x - stream[0].x)) / max(np.max(np.abs(stream[0].x)), 1.0))
    print("one member on a single-problem handle against the batch: %.3g" % dev)
    assert dev <= 1e-7, dev


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_resident_batch_of_large_cones_resolves_on_the_device_as_on_the_host(dtype):
    """BatchSolver over four such members is a resident single-structure batch: update_device(q=...) and optimize(results="device") return what the host
    path (cj.update, optimize) returns -- bit for bit in Float64"""
    probs = BP.sdps_tight()
    nprob, n = len(probs), probs[0]["q"].size
    st = dict(kkt_solver=cj.CGIndirectKKTSolver, eps_abs=1e-4, eps_rel=1e-4, max_iter=150, device_scaling=False, batch_psd_side_max=130)
    mh, md = BP.models(probs, cj.Settings(**st), dtype), BP.models(probs, cj.Settings(**st), dtype)
    rng = np.random.default_rng(31)
    with cj.BatchSolver(mh) as host, cj.BatchSolver(md) as dev:
        host.optimize(); dev.optimize()
        assert host.mixed is False and dev.mixed is False and isinstance(dev.batch, cj._ffi.Batch)
        q = np.stack([p["q"] + 0.2 * rng.standard_normal(n) for p in probs])
        for k, m_ in enumerate(mh):
            cj.update(m_, q=q[k])
        rh = host.optimize()
        dev.update_device(q=torch.from_numpy(np.ascontiguousarray(q, dtype=dtype)).to("cuda:0"))
        rd = dev.optimize(results="device")
        x, y, s = rd.x.cpu().numpy(), rd.y.cpu().numpy(), rd.s.cpu().numpy()
        for k, r in enumerate(rh):
            assert rd.status[k] == r.status and rd.iter[k] == r.iter and rd.obj_val[k] == r.obj_val, (k, rd.status[k], r.status, rd.iter[k], r.iter)
            if dtype == np.float64:
                assert np.array_equal(x[k], r.x) and np.array_equal(y[k], r.y) and np.array_equal(s[k], r.s), k
            else:                                                                  # _write_back multiplies in float64 (test_gpu_batch_device_io.py)
                for a, c in ((x[k], r.x), (y[k], r.y), (s[k], r.s)):
                    assert np.all(np.abs(a - c) <= 4 * U32 * np.abs(c)), k
