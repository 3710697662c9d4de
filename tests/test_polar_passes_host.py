"""Cone-local workgroup ids of the batch's populate-type kernels (csrc/polar_tiles.h: polar_wg_grid / polar_wg_id / polar_wg_decode; k_bpolar_norm and
k_bpolar_populate2 of csrc/psd_polar.hip decode blockIdx.x with them), checked on the host through tests/polar_passes_probe.cpp (g++, its own shared object,
nothing preloaded).  The kernels take for granted that every (cone, bx) of the batch is the work of exactly one workgroup of the 1-D grid and that the ids of a
short last group of cones decode to "none"; the speed rests on all workgroups of a cone sharing id % 8, one XCD under round-robin dispatch."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BPX = 16        # workgroups per cone in the kernels (BPX of psd_polar.hip)
_lib = None


def _probe():
    global _lib
    if _lib is None:
        csrc = os.path.join(_ROOT, "cosmo.jl_amd", "csrc")
        tmp = tempfile.mkdtemp(prefix="polar_passes_probe_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "polar_passes_probe.so")
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + csrc, "-o", so,
                        os.path.join(_ROOT, "tests", "polar_passes_probe.cpp")], check=True)
        lib = ctypes.CDLL(so)
        lib.polar_passes_grid.argtypes = [ctypes.c_int] * 2
        lib.polar_passes_id.argtypes = [ctypes.c_int] * 3
        lib.polar_passes_decode.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)]
        _lib = lib
    return _lib


def _decode(id_, n, bpx=BPX):
    out = (ctypes.c_int * 2)()
    _probe().polar_passes_decode(id_, n, bpx, out)
    return out[0], out[1]


@pytest.mark.parametrize("n", range(1, 41))
def test_every_cone_and_part_is_one_workgroup(n):
    lib = _probe()
    grid = lib.polar_passes_grid(n, BPX)
    assert grid == 8 * BPX * ((n + 7) // 8)
    seen = {}
    for id_ in range(grid):
        cone, bx = _decode(id_, n)
        if cone < 0:
            continue
        assert 0 <= cone < n and 0 <= bx < BPX
        assert (cone, bx) not in seen, (id_, seen[(cone, bx)])
        seen[(cone, bx)] = id_
        assert lib.polar_passes_id(cone, bx, BPX) == id_                 # the inverse
    assert len(seen) == n * BPX                                          # ... and every one of them is produced
    for cone in range(n):
        assert {seen[(cone, bx)] % 8 for bx in range(BPX)} == {cone % 8}  # one XCD per cone


@pytest.mark.parametrize("n", range(1, 41))
def test_ids_past_the_last_cone_are_none(n):
    lib = _probe()
    grid = lib.polar_passes_grid(n, BPX)
    none = [id_ for id_ in range(grid) if _decode(id_, n)[0] < 0]
    assert len(none) == grid - n * BPX
    for id_ in none:                                                      # exactly the ids whose cone would be n or more
        assert 8 * ((id_ // 8) // BPX) + id_ % 8 >= n
    for id_ in (-1, grid, grid + 7, grid + 8 * BPX):                       # outside the grid
        assert _decode(id_, n)[0] == -1


def test_other_part_counts():
    """the mapping does not depend on BPX being 16"""
    lib = _probe()
    for bpx in (1, 3, 8):
        for n in (1, 8, 9, 23):
            got = sorted(_decode(id_, n, bpx) for id_ in range(lib.polar_passes_grid(n, bpx)) if _decode(id_, n, bpx)[0] >= 0)
            assert got == [(c, b) for c in range(n) for b in range(bpx)]
