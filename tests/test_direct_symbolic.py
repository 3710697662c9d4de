"""Symbolic analysis of the direct KKT solver (csrc/ldl_symbolic.cpp, cosmo_hip_ldl_analyze): host only, no GPU.

Pinned against the compiled checker's elimination-tree count (oracle/cosmo_oracle_c.c: cosmo_oracle_c_ldl_nnz) on the same permutation, and the
default ordering (singleton rows of A first, then approximate minimum degree) against the oracle's minimum-degree ordering."""
import os
import subprocess
import time

import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from oracle import cosmo_oracle as O
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def OC():
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, capture_output=True)
    from oracle import cosmo_oracle_c
    return cosmo_oracle_c


def _ws(prob):
    return O.Workspace(prob["P"], prob["q"], prob["A"], prob["b"], util.oracle_cones(prob["sets"]), O.Settings(kkt_solver="cg", max_iter=1))


def _dense_row_qp(seed):
    rng = np.random.default_rng(seed)
    prob = util.random_qp(rng, 60, 4, 40, 30, soc_dims=(5,), p_shift=1.0)
    A = prob["A"].tolil()
    A[prob["A"].shape[0] - 1, :] = rng.standard_normal(prob["A"].shape[1])       # one dense row (the last Box row)
    prob["A"] = A.tocsc()
    return prob


def _cases():
    out = []
    for seed in range(4):
        rng = np.random.default_rng(100 + seed)
        out.append(("mixed%d" % seed, util.random_qp(rng, 50 + 10 * seed, 5, 40, 30, soc_dims=(4, 6), psd_tri_dims=(3, 6), p_shift=1.0)))
    rng = np.random.default_rng(7)
    out.append(("zero_only", util.random_qp(rng, 40, 30, 0, 0, p_shift=1.0)))
    rng = np.random.default_rng(8)
    out.append(("psd_square", util.random_qp(rng, 45, 3, 10, 0, psd_sq_dims=(16,), p_shift=1.0)))
    out.append(("dense_row", _dense_row_qp(9)))
    out.append(("chordal_small", cj.problems.chordal_sdp(ncliques=12, dmin=4, dmax=9, sep_min=1, sep_max=3, n_total=400, n_zero=10, n_nonneg=20)))
    return out


CASES = _cases()


def _analyze(ws, perm=None):
    return cj._ffi.ldl_analyze(ws.n, ws.m, ws.P, ws.A, perm)


@pytest.mark.parametrize("name,prob", CASES, ids=[c[0] for c in CASES])
def test_fill_equals_the_checkers_count_on_the_oracle_ordering(OC, name, prob):
    ws = _ws(prob)
    perm = OC.kkt_ordering(ws, cache=False)
    r = _analyze(ws, perm)
    assert r["nnz_L"] == OC.ldl_nnz(ws, perm)
    assert r["amalgamation_zeros"] == 0 and r["nnz_stored"] == r["nnz_L"]
    assert 1 <= r["supernodes"] <= ws.n + ws.m and 1 <= r["height"] <= r["supernodes"] and r["max_width"] >= 1


@pytest.mark.parametrize("name,prob", CASES, ids=[c[0] for c in CASES])
def test_default_ordering_fill_within_twice_the_oracle_ordering(OC, name, prob):
    ws = _ws(prob)
    ref = OC.ldl_nnz(ws, OC.kkt_ordering(ws, cache=False))
    r = _analyze(ws)
    assert r["nnz_L"] <= 2 * max(ref, 1), (r["nnz_L"], ref)


def test_identity_and_reversed_orderings_match_the_checker(OC):
    ws = _ws(CASES[0][1])
    N = ws.n + ws.m
    for perm in (np.arange(N), np.arange(N)[::-1].copy()):
        assert _analyze(ws, perm)["nnz_L"] == OC.ldl_nnz(ws, perm)


def test_bad_permutations_are_refused():
    ws = _ws(CASES[0][1])
    N = ws.n + ws.m
    bad = np.arange(N); bad[3] = bad[4]
    with pytest.raises(cj._ffi.CosmoHipError):
        _analyze(ws, bad)
    with pytest.raises(ValueError):
        _analyze(ws, np.arange(N - 1))


def test_analysis_is_deterministic():
    ws = _ws(CASES[1][1])
    assert _analyze(ws) == _analyze(ws)


def test_cfg5_committed_ordering_and_default_ordering(OC):
    """BASELINE config 5: the committed ordering of oracle/kkt_perm/ gives the committed fill exactly; the default ordering stays within 2x."""
    prob = cj.problems.chordal_sdp()
    ws = _ws(prob)
    perm = OC.kkt_ordering(ws)            # read from the committed cache file (no write: the file exists)
    assert _analyze(ws, perm)["nnz_L"] == 15226798
    t0 = time.perf_counter()
    r = _analyze(ws)
    dt = time.perf_counter() - t0
    print("cfg5 default ordering: nnz(L) = %d (%.3fx the oracle ordering), %d supernodes, height %d, widest %d, analysis %.2f s"
          % (r["nnz_L"], r["nnz_L"] / 15226798, r["supernodes"], r["height"], r["max_width"], dt))
    assert r["nnz_L"] <= 2 * 15226798
