"""The library builds the LDS images that the host-only planner plans, and runs what it ran before the planner left csrc/batch.hip: for every case of
tests/batch_image_cases.py get_image(k) equals the bytes of the probe (tests/batch_image_probe.cpp on csrc/batch_image.cpp) for the same inputs, and
kernel_info() equals the recorded one; for the eleven kernel forms the iterates after 30 iterations hash to the recorded value.  The recorded answers
are those of the commit before the planner (tests/golden/make_fixtures_batch_image.py)."""
import os

import numpy as np
import pytest

from cosmo_jl_amd import _ffi
from tests import batch_image_cases as IC

pytestmark = pytest.mark.gpu
_seen = {}


def run(case):
    """the case's batch under its switches (read at set_params): kernel_info, every member's image, the recorded kind of answers"""
    if case not in _seen:
        saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("COSMO_HIP_BATCH_")}
        os.environ.update(IC.env_of(case))
        try:
            B = IC.finalized_batch(case)
        finally:
            for k in IC.env_of(case):
                del os.environ[k]
            os.environ.update(saved)
        images = [B.get_image(k) for k in range(B.nprob)]
        _seen[case] = dict(images=images, answers=IC.answers(case, B))
        B.close()
    return _seen[case]


def test_the_cone_codes_are_the_librarys():
    assert (IC.ZERO, IC.NONNEG, IC.BOX, IC.SOC, IC.PSD_SQUARE, IC.PSD_TRIANGLE, IC.EXP, IC.DUAL_EXP, IC.POW, IC.DUAL_POW) == \
        (_ffi.ZERO, _ffi.NONNEG, _ffi.BOX, _ffi.SOC, _ffi.PSD_SQUARE, _ffi.PSD_TRIANGLE, _ffi.EXP, _ffi.DUAL_EXP, _ffi.POW, _ffi.DUAL_POW)


@pytest.mark.parametrize("case", list(IC.CASES))
def test_the_library_uploads_the_bytes_the_planner_planned(case):
    got, f = run(case), IC.family(IC.CASES[case]["family"])
    info = got["answers"]["kernel_info"]
    pl = IC.plan(case)
    for k in range(f.nprob):
        want = IC.image_bytes(pl, k, info["sliced"], f.n) if info["form"] != "streaming" else np.zeros(0, dtype=np.uint8)
        assert np.array_equal(got["images"][k], want), k
    assert got["answers"]["image"] == IC.HASHES[case]["image"]


@pytest.mark.parametrize("case", list(IC.CASES))
def test_the_batch_runs_the_kernel_it_ran_before(case):
    assert run(case)["answers"]["kernel_info"] == IC.HASHES[case]["kernel_info"]


@pytest.mark.parametrize("case", IC.FORMS)
def test_thirty_iterations_give_the_bits_they_gave_before(case):
    assert run(case)["answers"]["iterates"] == IC.HASHES[case]["iterates"]
