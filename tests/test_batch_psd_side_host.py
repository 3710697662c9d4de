"""Settings.batch_psd_side_max on the host: the default, what the routing predicates answer, the two C entry points in the header and the export map,
and the round schedule of psdwg_jacobi_rounds (csrc/psdwg.h) as a Python model -- the condition that makes a wave's sequential visits safe."""
import fnmatch
import itertools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from tests import batch_psd_side_cases as BP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cosmo_hip_batch_set_psd_side_max", "cosmo_hip_batch_group_set_psd_side_max")


def _model(cone, **kw):
    m = cone.dim
    md = cj.Model()
    md.set(sp.identity(2, format="csc"), np.zeros(2), sp.csc_matrix((np.ones(m), (np.arange(m), np.arange(m) % 2)), shape=(m, 2)), np.zeros(m), [cone],
           cj.Settings(**kw))
    return md


def test_the_default_limit_is_64_and_not_a_reference_setting():
    assert cj.Settings().batch_psd_side_max == 64
    assert cj.model._batch_psd_side_max_of(cj.Settings()) == 64
    for bad in (63, 257, 0):
        with pytest.raises(ValueError, match="64 .. 256"):
            cj.model._batch_psd_side_max_of(cj.Settings(batch_psd_side_max=bad))


@pytest.mark.parametrize("cone", [cj.PsdConeTriangle, cj.PsdCone])
def test_the_batch_kernels_take_a_model_within_the_limit(cone):
    dim = (lambda d: d * (d + 1) // 2) if cone is cj.PsdConeTriangle else (lambda d: d * d)
    take = cj.model._batch_kernels_take
    assert take(_model(cone(dim(64))))
    assert not take(_model(cone(dim(65))))
    assert take(_model(cone(dim(65)), batch_psd_side_max=65))
    assert not take(_model(cone(dim(66)), batch_psd_side_max=65))
    assert take(_model(cone(dim(256)), batch_psd_side_max=256))
    assert not take(_model(cone(dim(257)), batch_psd_side_max=256))


def test_the_eigen_projection_check_follows_the_limit():
    check = cj.model._check_batch_psd_projection
    d65, d129 = 65 * 66 // 2, 129 * 130 // 2
    check([_model(cj.PsdConeTriangle(d65))])                                   # the default projection: nothing to refuse
    with pytest.raises(NotImplementedError, match="side 65 > 64"):
        check([_model(cj.PsdConeTriangle(d65), psd_projection="eigen")])
    check([_model(cj.PsdConeTriangle(d65), psd_projection="eigen", batch_psd_side_max=65)])
    check([_model(cj.PsdConeTriangle(d65), psd_projection="eigen", batch_psd_side_max=128)])
    with pytest.raises(NotImplementedError, match="side 129 > 128"):
        check([_model(cj.PsdConeTriangle(d129), psd_projection="eigen", batch_psd_side_max=128)])


def test_the_header_declares_the_entry_points_and_the_export_map_lists_them():
    header = open(os.path.join(ROOT, "include", "cosmo_hip.h")).read()
    assert re.search(r"COSMO_HIP_API\s+int32_t\s+cosmo_hip_batch_set_psd_side_max\(cosmo_hip_batch\*\s*b,\s*int32_t\s+side\);", header)
    assert re.search(r"COSMO_HIP_API\s+int32_t\s+cosmo_hip_batch_group_set_psd_side_max\(cosmo_hip_batch_group\*\s*g,\s*int32_t\s+side\);", header)
    assert re.search(r"#define\s+COSMO_HIP_ABI_VERSION\s+1005\b", header)            # new entry points only
    exports = open(os.path.join(ROOT, "cosmo.jl_amd", "csrc", "exports.map")).read()
    exported = re.search(r"global:\s*([^;]*);", exports).group(1).split()
    for name in ENTRY_POINTS:
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), (name, exported)
        assert name in cj._ffi.SIGNATURES


@pytest.mark.parametrize("nw", [4, 8])
@pytest.mark.parametrize("nb", [10, 16, 18, 32])
def test_the_round_schedule_visits_disjoint_pairs_and_every_pair_once(nb, nw):
    npairs = nb // 2
    met = {}
    for st in range(-1, nb - 1):                                               # -1: the diagonal pass
        pairs = BP.step_pairs(nb, st)
        assert len(pairs) == npairs
        # within a step every block index occurs in exactly one pair: the visits of a step touch disjoint columns, in any order and on any wave
        assert sorted(b for p in pairs for b in p) == list(range(nb)), (st, pairs)
        # the waves share the step's pairs: wave wv takes wv, wv + NW, ...; together every pair exactly once
        visits = [BP.wave_visits(nb, nw, wv) for wv in range(nw)]
        for wv, v in enumerate(visits):
            assert v == list(range(wv, npairs, nw)) and all(b - a == nw for a, b in zip(v, v[1:]))
        assert sorted(w for v in visits for w in v) == list(range(npairs))
        assert max(len(v) for v in visits) == -(-npairs // nw)                 # the rounds of the step
        if st >= 0:
            for p in pairs:
                assert p[0] < p[1]
                met[p] = met.get(p, 0) + 1
    # over the nb - 1 tournament steps every pair of blocks meets exactly once (the diagonal pass rotates inside the blocks (2w, 2w + 1) in front)
    assert met == {p: 1 for p in itertools.combinations(range(nb), 2)}
    assert BP.step_pairs(nb, -1) == [(2 * w, 2 * w + 1) for w in range(npairs)]


def test_the_model_restates_the_kernels_schedule():
    """the text of csrc/psdwg.h: the tournament formula and the round loop the model stands for; the geometry of the sides the GPU tests run"""
    src = open(os.path.join(ROOT, "cosmo.jl_amd", "csrc", "psdwg.h")).read()
    assert "if (w == 0) { I = st % m; J = m; }" in src and "else { I = (st + w) % m; J = (st - w + m) % m; }" in src
    body = src[src.index("int psdwg_jacobi_rounds("):src.index("int psdwg_jacobi_batch(")]
    assert body.count("for (int st = -1; st < nb - 1; ++st)") == 1             # the diagonal pass (st = -1), then the tournament steps ...
    assert body.count("for (int w = wv; w < npairs; w += NW)") == 1            # ... and in each of them this wave's pairs, one after the other
    assert "int I = 2 * w, Jb = 2 * w + 1;" in body and "if (st >= 0) rr_pair(nb, st, w, I, Jb);" in body and "while" not in body
    batch = src[src.index("int psdwg_jacobi_batch("):]
    assert "if (nb / 2 <= 4) return psdwg_jacobi<4>(" in batch and "return psdwg_jacobi_rounds<4>(" in batch
    for side, (nb, npairs) in BP.SIDES.items():
        ld, nb_, ncp = BP.geometry(side)
        assert (nb_, nb_ // 2) == (nb, npairs) and ld % 16 == 0 and ld >= side and ncp >= ld and ncp % 8 == 0
    assert BP.geometry(64)[1] // 2 == 4 and BP.geometry(65)[1] // 2 == 5 and BP.geometry(129)[0] == 144
    # int offsets of the kernels: the largest cone's rows and its slab of G, and the slab of a member (long long in the library)
    assert 256 * 256 < 2 ** 31 and BP.geometry(256) == (256, 32, 256) and 256 * 256 * 8 == 512 * 1024
