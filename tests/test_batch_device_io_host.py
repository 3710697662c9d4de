"""CPU tests of the device-memory entry points of a resident batch (cosmo_hip_batch_update_qb_device / set_iterates_device / get_solution_device,
csrc/batch_devio.hip; cosmo_jl_amd.BatchSolver.update_device, optimize(x0=, results="device")): they are declared, exported by both libraries and bound
with the header's signatures, and the Python layer refuses anything but a device tensor of the right kind before a pointer reaches the library."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cosmo_jl_amd as cj
from cosmo_jl_amd import _ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cosmo_hip_batch_update_qb_device", "cosmo_hip_batch_set_iterates_device", "cosmo_hip_batch_get_solution_device"]


def _model(n=6, m=5, seed=0, dtype=np.float64):
    rng = np.random.default_rng(seed)
    md = cj.Model(dtype=dtype)
    md.set(sp.identity(n, format="csc"), rng.standard_normal(n), sp.random(m, n, density=0.5, random_state=seed, format="csc") + sp.eye(m, n),
           np.abs(rng.standard_normal(m)), [cj.ZeroSet(2), cj.Nonnegatives(m - 2)])
    return md


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cosmo_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("path", [F.LIB_PATH, F.LIB_PATH_F32])
def test_device_entry_points_are_declared_exported_and_bound(path):
    src = _header()
    lib = ctypes.CDLL(path)
    for nm in NEW:
        assert re.search(r"COSMO_HIP_API\s+int32_t\s+%s\s*\(" % nm, src), nm
        assert hasattr(lib, nm), nm
        assert nm in F.SIGNATURES, nm
    # csrc/exports.map lets them through: they are in the dynamic symbol table as functions
    pattern = re.search(r"global:\s*([^;]+);", open(os.path.join(ROOT, "cosmo.jl_amd", "csrc", "exports.map")).read()).group(1).strip()
    assert all(re.fullmatch(pattern.replace("*", ".*"), nm) for nm in NEW)
    nm_tool = shutil.which("nm")
    if nm_tool is not None:
        out = subprocess.run([nm_tool, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        table = {ln.split()[-1]: ln.split()[-2] for ln in out.splitlines() if ln.strip()}
        assert all(table.get(nm) == "T" for nm in NEW), [table.get(nm) for nm in NEW]
    assert cj.load_library().cosmo_hip_version() == F.ABI_VERSION == 1005           # entry points were added, nothing changed


def test_real_pointers_and_the_stream_sit_where_the_header_puts_them():
    src = _header()
    for nm in NEW:
        params = [a.strip() for a in re.search(r"\b%s\s*\((.*?)\)\s*;" % nm, src, re.S).group(1).split(",")]
        res, args = F.SIGNATURES[nm]
        assert res is ctypes.c_int32 and len(params) == len(args), (nm, params)
        for prm, a in zip(params, args):
            assert (a is F._PR) == bool(re.search(r"cosmo_hip_real\s*\*", prm)), (nm, prm)
            assert (a is F._PI64) == bool(re.search(r"int64_t\s*\*", prm)), (nm, prm)
            assert (a is ctypes.c_void_p) == bool(re.search(r"cosmo_hip_batch\s*\*|void\s*\*", prm)), (nm, prm)
        assert re.search(r"void\s*\*\s*stream$", params[-1]), (nm, params[-1])       # the caller's stream comes last
    f32 = cj.load_library(np.float32)
    assert f32.cosmo_hip_batch_get_solution_device.argtypes[1] is F._PF and cj.load_library().cosmo_hip_batch_get_solution_device.argtypes[1] is F._PD


def test_the_header_states_the_stream_contract():
    raw = open(os.path.join(ROOT, "include", "cosmo_hip.h")).read()
    proto = raw.index("COSMO_HIP_API int32_t cosmo_hip_batch_update_qb_device")
    comment = raw[raw.rindex("/*", 0, proto):proto]
    for phrase in ("Stream contract", "HIP stream handle", "null stream", "records an event", "hipPointerGetAttributes", "apply_updates first"):
        assert phrase in comment, phrase


def test_update_device_needs_a_batch_on_the_device():
    a, b = _model(seed=1), _model(seed=2)
    with cj.BatchSolver([a, b]) as rb:
        assert rb.batch is None
        with pytest.raises(RuntimeError, match="before the first optimize"):
            rb.update_device(q=torch.zeros((2, a.n), dtype=torch.float64))
        with pytest.raises(RuntimeError, match="before the first optimize"):
            rb.update_device()
    with pytest.raises(RuntimeError, match="closed"):
        rb.update_device(q=torch.zeros((2, a.n), dtype=torch.float64))


CPU = torch.device("cpu")
GPU0 = torch.device("cuda", 0)


@pytest.mark.parametrize("dtype, tdt, other", [(np.float64, torch.float64, torch.float32), (np.float32, torch.float32, torch.float64)])
def test_check_device_tensor_names_what_is_wrong(dtype, tdt, other):
    good = torch.zeros((3, 7), dtype=tdt)
    assert F.check_device_tensor(good, (3, 7), dtype, CPU, "q") is good            # (the only device a CPU test has: the rule itself is the same)
    assert F.check_device_tensor(None, (3, 7), dtype, GPU0, "q") is None
    with pytest.raises(ValueError, match="q lives on cpu, the batch on cuda:0"):
        F.check_device_tensor(good, (3, 7), dtype, GPU0, "q")
    with pytest.raises(ValueError, match="dtype"):
        F.check_device_tensor(torch.zeros((3, 7), dtype=other), (3, 7), dtype, CPU, "q")
    for bad in (torch.zeros((7, 3), dtype=tdt), torch.zeros(21, dtype=tdt), torch.zeros((3, 8), dtype=tdt), torch.zeros((4, 7), dtype=tdt)):
        with pytest.raises(ValueError, match="shape"):
            F.check_device_tensor(bad, (3, 7), dtype, CPU, "q")
    for bad in (torch.zeros((7, 3), dtype=tdt).t(), torch.zeros((3, 14), dtype=tdt)[:, ::2]):
        assert tuple(bad.shape) == (3, 7)
        with pytest.raises(ValueError, match="not contiguous"):
            F.check_device_tensor(bad, (3, 7), dtype, CPU, "q")
    with pytest.raises(ValueError, match="torch tensor"):
        F.check_device_tensor(np.zeros((3, 7), dtype=dtype), (3, 7), dtype, CPU, "q")


@pytest.mark.parametrize("dtype, tdt, other", [(np.float64, torch.float64, torch.float32), (np.float32, torch.float32, torch.float64)])
def test_optimize_refuses_bad_tensors_before_anything_is_set_up(dtype, tdt, other):
    models = [_model(seed=3, dtype=dtype), _model(seed=4, dtype=dtype)]
    n, m = models[0].n, models[0].m
    with cj.BatchSolver(models) as rb:
        bad = [dict(x0=torch.zeros((2, n), dtype=tdt)),                               # a CPU tensor
               dict(y0=torch.zeros((2, m), dtype=other)),                             # wrong dtype
               dict(s0=torch.zeros((2, n), dtype=tdt)),                               # wrong shape: s0 is (nprob, m)
               dict(x0=torch.zeros((3, n), dtype=tdt)),                               # wrong member count
               dict(x0=torch.zeros((n, 2), dtype=tdt).t()),                           # not contiguous
               dict(x0=np.zeros((2, n), dtype=dtype)),                                # not a tensor
               dict(results="device", out=(torch.zeros((2, n), dtype=tdt), torch.zeros((2, m), dtype=tdt), torch.zeros((2, m), dtype=tdt))),
               dict(results="device", out=(torch.zeros((2, n), dtype=tdt),)),
               dict(out=(None, None, None)),                                          # out belongs to results="device"
               dict(results="somewhere")]
        for kw in bad:
            with pytest.raises(ValueError):
                rb.optimize(**kw)
            assert rb.batch is None, kw                                               # refused before the set-up touched a device
