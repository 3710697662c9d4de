"""CPU tests of the matrix value update: the value maps of csrc/value_maps.cpp, the host logic of cosmo_jl_amd.update(model, P=, A=) and the binding."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from cosmo_jl_amd import _ffi
from cosmo_jl_amd.model import _scale_csc
from tests import update_matrix_cases as UC
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the four-copy maps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,P,A", UC.map_patterns(), ids=[p[0] for p in UC.map_patterns()])
def test_gathering_new_values_through_the_maps_gives_the_csr_copies(name, P, A):
    rng = np.random.default_rng(1)
    n, m = P.shape[0], A.shape[0]
    mp = UC.maps_of(n, m, P.indptr, P.indices, A.indptr, A.indices)
    newP, newA = rng.standard_normal(P.nnz), rng.standard_normal(A.nnz)
    P2, A2 = UC.same_pattern(P, newP), UC.same_pattern(A, newA)
    for M2, new, key in ((A2, newA, "A"), (P2, newP, "P")):
        R = M2.tocsr(); R.sort_indices()
        assert np.array_equal(mp[key + "_rowptr"], R.indptr)
        assert np.array_equal(new[mp[key + "_map"]], R.data)
        assert sorted(mp[key + "_map"].tolist()) == list(range(M2.nnz))                      # a permutation: every source is used exactly once
    # the transposes share the caller's arrays: the CSR of A' IS (A.indptr, A.indices, new) -- the identity needs no map
    At = A2.T.tocsr(); At.sort_indices()
    assert np.array_equal(At.data, newA) and np.array_equal(At.indices, A.indices)
    # merged [P | A']: row j = row j of P, then column j of A with its columns shifted by n
    Pr = P2.tocsr(); Pr.sort_indices()
    rowptr = Pr.indptr + At.indptr
    assert np.array_equal(mp["PT_rowptr"], rowptr)
    assert np.array_equal(mp["PT_split"], rowptr[:-1] + np.diff(Pr.indptr))
    want = np.concatenate([np.concatenate([Pr.data[Pr.indptr[j]:Pr.indptr[j + 1]], At.data[At.indptr[j]:At.indptr[j + 1]]]) for j in range(n)] or [np.zeros(0)])
    in_P = np.concatenate([np.concatenate([np.ones(Pr.indptr[j + 1] - Pr.indptr[j], bool), np.zeros(At.indptr[j + 1] - At.indptr[j], bool)]) for j in range(n)]
                          or [np.zeros(0, bool)])
    idx = mp["PT_map"]
    got = np.where(in_P, newP[np.where(in_P, idx, 0)] if P.nnz else 0.0, newA[np.where(in_P, 0, idx)] if A.nnz else 0.0)
    assert np.array_equal(got, want)


def test_maps_keep_duplicates_and_unsorted_rows_apart():
    n, m, (pp, pi), (ap, ai) = UC.raw_duplicate_pattern()
    mp = UC.maps_of(n, m, pp, pi, ap, ai)
    rng = np.random.default_rng(2)
    for key, nr, nc, ptr, ind in (("A", m, n, ap, ai), ("P", n, n, pp, pi)):
        new = rng.standard_normal(ind.size)
        cols = np.repeat(np.arange(nc), np.diff(ptr))
        rowptr, mapping = mp[key + "_rowptr"], mp[key + "_map"]
        assert sorted(mapping.tolist()) == list(range(ind.size))
        dense = np.zeros((nr, nc))
        np.add.at(dense, (ind, cols), new)
        got = np.zeros((nr, nc))
        for r in range(nr):
            src = mapping[rowptr[r]:rowptr[r + 1]]
            assert np.all(ind[src] == r)                                                     # every entry of CSR row r comes from a source in row r ...
            assert np.all(np.diff(cols[src]) >= 0)                                           # ... columns ascending, a column's entries in their stored order
            assert np.all(np.diff(src)[np.diff(cols[src]) == 0] > 0)
            np.add.at(got[r], cols[src], new[src])
        assert np.array_equal(got, dense)
    # merged layout: per row j the P sources of row j, then the stored entries of column j of A in their order
    for j in range(n):
        seg = mp["PT_map"][mp["PT_rowptr"][j]:mp["PT_rowptr"][j + 1]]
        k = mp["PT_split"][j] - mp["PT_rowptr"][j]
        assert np.array_equal(seg[:k], mp["P_map"][mp["P_rowptr"][j]:mp["P_rowptr"][j + 1]])
        assert np.array_equal(seg[k:], np.arange(ap[j], ap[j + 1]))


# ---- update(model, P=, A=) on the host ----------------------------------------------------------------------------------------------------------
def _model(case, **st):
    md = cj.Model()
    md.set(case["P"], case["q"], case["A"], case["b"], case["sets"], cj.Settings(**st))
    return md


def test_update_without_a_handle_replaces_the_host_copies():
    case = UC.mixed_case()
    md = _model(case)
    cj.update(md, P=case["P2"].toarray(), A=case["A2"])                                     # anything Model.set accepts: dense, sparse
    assert md.handle is None
    assert np.array_equal(md.P.data, case["P2"].data) and np.array_equal(md.A.data, case["A2"].data)
    assert np.array_equal(md.P.indices, case["P"].indices) and np.array_equal(md.A.indptr, case["A"].indptr)
    x0 = np.arange(md.n, dtype=np.float64)
    cj.warm_start_primal(md, x0)
    assert np.array_equal(md.s, case["b"] - case["A2"] @ x0)


def test_update_refuses_another_pattern():
    case = UC.mixed_case()
    md = _model(case)
    A3 = case["A"].tolil(); A3[0, :] = 0.0; A3[0, 1] = 1.0; A3[0, 2] = 1.0; A3[0, 3] = 3.0
    with pytest.raises(ValueError, match="A"):
        cj.update(md, A=A3.tocsc())
    P3 = (case["P"] + sp.csc_matrix(([1e-3, 1e-3], ([0, md.n - 1], [md.n - 1, 0])), shape=case["P"].shape)).tocsc()
    assert P3.nnz != case["P"].nnz
    with pytest.raises(ValueError, match="P"):
        cj.update(md, P=P3)
    with pytest.raises(ValueError, match="P"):
        cj.update(md, P=sp.identity(md.n + 1, format="csc"))
    # explicit zeros are stored entries: dropping one changes the pattern
    Az = case["A2"].copy(); Az.data[0] = 0.0
    cj.update(md, A=Az)
    Ae = Az.copy(); Ae.eliminate_zeros()
    with pytest.raises(ValueError, match="A"):
        cj.update(md, A=Ae)


def test_update_refuses_decomposed_and_resident_models():
    case = UC.mixed_case()
    md = _model(case)
    md.chordal = object()
    with pytest.raises(RuntimeError, match="chordally decomposed"):
        cj.update(md, P=case["P2"])
    with pytest.raises(RuntimeError, match="chordally decomposed"):
        cj.update(md, A=case["A2"])
    md.chordal = None
    md.resident = (object(), 0)
    with pytest.raises(NotImplementedError, match="resident"):
        cj.update(md, A=case["A2"])


def test_update_of_a_host_scaled_model_scales_with_the_kept_matrices():
    case = UC.mixed_case()
    md = _model(case, scaling=10)
    st = md.settings
    md.sm = cj.model.scale_ruiz(md.P, md.q, md.A, md.b, md.sets, st)                         # what setup() does for host scaling, without a device
    md.is_scaled = True
    sm = md.sm
    D0, E0, c0 = sm.D.copy(), sm.E.copy(), sm.c
    cj.update(md, P=case["P2"], A=case["A2"])
    assert np.array_equal(sm.D, D0) and np.array_equal(sm.E, E0) and sm.c == c0              # the scaling is frozen
    P2 = case["P2"].copy(); A2 = case["A2"].copy()
    _scale_csc(P2, D0, D0); P2.data *= c0
    _scale_csc(A2, E0, D0)
    assert np.array_equal(md.P.data, P2.data) and np.array_equal(md.A.data, A2.data)
    want = (sp.diags(D0) @ case["P2"] @ sp.diags(D0) * c0).toarray()
    assert np.allclose(md.P.toarray(), want, rtol=1e-14, atol=0.0)
    assert np.allclose(md.A.toarray(), (sp.diags(E0) @ case["A2"] @ sp.diags(D0)).toarray(), rtol=1e-14, atol=0.0)


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------
def test_header_and_bindings_declare_the_update():
    src = open(os.path.join(ROOT, "include", "cosmo_hip.h")).read()
    for name in ("cosmo_hip_update_matrices", "cosmo_hip_update_matrices_info"):
        assert re.search(r"^COSMO_HIP_API int32_t %s\(" % name, src, flags=re.M), name
        assert name in _ffi.SIGNATURES
    assert _ffi.SIGNATURES["cosmo_hip_update_matrices"][1] == [_ffi.C.c_void_p, _ffi._PR, _ffi._PR, _ffi.C.c_int32]
    assert _ffi.SIGNATURES["cosmo_hip_update_matrices_info"][1] == [_ffi.C.c_void_p, _ffi._PI64]
    assert _ffi.ABI_VERSION == 1005
    assert re.search(r"#define COSMO_HIP_ABI_VERSION 1005\b", src)
    glue = open(os.path.join(ROOT, "cosmo.jl_amd", "julia", "CosmoHIP.jl")).read()
    assert "function update_matrices!" in glue and ":cosmo_hip_update_matrices" in glue
