"""Host analysis of the Schur-complement KKT solver (csrc/schur_plan.cpp, cosmo_hip_schur_analyze): host only, no GPU.

  * the builder of tests/schur_cases.py produces exactly the requested split (checked with scipy.sparse.csgraph, independent of the code under test);
  * cosmo_hip_schur_analyze reports SciPy's figures on those problems and on the edge cases (no long row, one component equal to all of n, a row
    exactly at the threshold, stored duplicates, an empty P), deterministically, and its accepted flag flips exactly at the default limits;
  * BASELINE config 5 (problems.chordal_sdp()) is accepted at the default threshold with the figures DESIGN.md records;
  * tests/schur_plan_probe.cpp, a stand-alone program built with -fsanitize=address,undefined, walks every map of the plan: all indices in range,
    and every block entry written by exactly the sources SciPy's pattern of M_s predicts;
  * the ABI: version unchanged, the new entry points declared and exported."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from cosmo_jl_amd import _ffi
from tests import schur_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"small_sides": ((1,) * 9, 17), "no_long_row": ((1, 1, 2, 2, 3, 3), 0), "one_component": ((40,), 6), "wave_switch": ((63, 64, 65, 4), 133),
         "block_max": ((S.BLOCK_MAX, 3, 1), 5), "p_zero": ((1, 2, 3, 30, 70), 40)}


def _case(name):
    sizes, nd = CASES[name]
    return S.build(sizes, nd, seed=3, p_zero=(name == "p_zero"), single_frac=0.5 if name == "p_zero" else 1.0)


@pytest.mark.parametrize("name", list(CASES))
def test_the_builder_gives_the_requested_split(name):
    p = _case(name)
    nd, nc, largest, sumsq, lab = S.components(p["P"], p["A"])
    assert nd == p["nd"] and sorted(np.bincount(lab).tolist()) == p["sizes"]
    assert nc == len(p["sizes"]) and largest == max(p["sizes"]) and sumsq == sum(s * s for s in p["sizes"])
    for k in range(nc):                                    # SciPy's components are the builder's, member for member
        assert len(set(p["label"][lab == k])) == 1
    kinds = [type(K).__name__ for K in p["sets"]]
    assert kinds.count("PsdConeTriangle") == 2 and "Nonnegatives" in kinds and "ZeroSet" in kinds
    if p["nd"] >= 2:                                       # rho * 1e3 rows on both sides of the split
        nz = p["sets"][0].dim
        lens = S.row_lengths(p["A"])[:nz]
        assert (lens >= 3).any() and (lens < 3).any()


@pytest.mark.parametrize("name", list(CASES))
def test_analyze_reports_scipys_figures(name):
    p = _case(name)
    got = _ffi.schur_analyze(p["n"], p["m"], p["P"], p["A"])
    nd, nc, largest, sumsq, _ = S.components(p["P"], p["A"])
    assert (got["nd"], got["components"], got["largest"], got["sum_size2"]) == (nd, nc, largest, sumsq)
    assert got["nnz_W"] == S.nnz_w(p["P"], p["A"]) and got["accepted"] == 1
    assert got["small_components"] == sum(1 for s in p["sizes"] if s <= S.SMALL_MAX)
    ndp = -(-nd // S.NB) * S.NB
    assert got["dense_bytes"] == 2 * ndp * ndp * 8
    assert _ffi.schur_analyze(p["n"], p["m"], p["P"], p["A"], dtype=np.float32)["dense_bytes"] == 2 * ndp * ndp * 4
    assert _ffi.schur_analyze(p["n"], p["m"], p["P"], p["A"]) == got                       # determinism
    for thr in (2, 4, 7):                                                                   # other thresholds: SciPy's split again
        g = _ffi.schur_analyze(p["n"], p["m"], p["P"], p["A"], thr)
        nd, nc, largest, sumsq, _ = S.components(p["P"], p["A"], thr)
        assert (g["nd"], g["components"], g["largest"], g["sum_size2"], g["nnz_W"]) == (nd, nc, largest, sumsq, S.nnz_w(p["P"], p["A"], thr))


def test_a_row_exactly_at_the_threshold_is_long_and_stored_duplicates_count():
    n = 6
    P = sp.csc_matrix((n, n))
    # row 0: columns 0, 1 (short: joins 0 and 1); row 1: columns 2, 3, 4 (exactly three entries: long at threshold 3, short at 4);
    # row 2: column 5 stored twice (two stored entries: short, one component); row 3: column 0 stored three times (three stored entries: long)
    indptr = np.array([0, 2, 5, 7, 10])
    indices = np.array([0, 1, 2, 3, 4, 5, 5, 0, 0, 0])
    A = sp.csr_matrix((np.ones(10), indices, indptr), shape=(4, n))
    Ac = sp.csc_matrix((np.ones(10), np.array([0, 3, 3, 3, 0, 1, 1, 1, 2, 2]), np.array([0, 4, 5, 6, 7, 8, 10])), shape=(4, n))   # the same entries, CSC with duplicates kept
    assert (Ac.toarray() == A.toarray()).all() and Ac.nnz == 10
    g3 = _ffi.schur_analyze(n, 4, P, Ac, 3)
    assert (g3["nd"], g3["components"], g3["largest"], g3["sum_size2"]) == (2, 5, 2, 8)          # {0, 1}, 2, 3, 4, 5
    assert g3["nnz_W"] == 3 + 2                                                                 # row 1 fills three singletons, row 3 the block {0, 1}
    g4 = _ffi.schur_analyze(n, 4, P, Ac, 4)
    assert (g4["nd"], g4["components"], g4["largest"], g4["sum_size2"]) == (0, 3, 3, 4 + 9 + 1)  # {0, 1}, {2, 3, 4}, 5
    g0 = _ffi.schur_analyze(n, 4, P, Ac, 0)
    assert g0 == g3                                                                              # 0: the default threshold


def test_the_accepted_flag_flips_exactly_at_the_default_limits():
    def chain(side, nd):
        n = side + 2
        rows = [[i, i + 1] for i in range(side - 1)] + [[0, side, side + 1]] * nd
        ri = np.concatenate([np.full(len(r), k) for k, r in enumerate(rows)]); ci = np.concatenate(rows)
        A = sp.csr_matrix((np.ones(ri.size), ci, np.concatenate([[0], np.cumsum([len(r) for r in rows])])), shape=(len(rows), n))
        return n, len(rows), sp.csc_matrix((n, n)), A.tocsc()
    for side, want in ((S.BLOCK_MAX, 1), (S.BLOCK_MAX + 1, 0)):
        g = _ffi.schur_analyze(*chain(side, 3))
        assert (g["largest"], g["nd"], g["accepted"]) == (side, 3, want)
    for nd, want in ((S.ND_MAX, 1), (S.ND_MAX + 1, 0)):
        g = _ffi.schur_analyze(*chain(4, nd))
        assert (g["largest"], g["nd"], g["accepted"]) == (4, nd, want)


def test_config_5_is_accepted_with_the_recorded_figures():
    p = cj.problems.chordal_sdp()
    m, n = p["A"].shape
    assert (n, m) == (50000, 2861207)
    lens = S.row_lengths(p["A"])
    assert (int((lens == 1).sum()), int((lens == 2).sum())) == (2828464, 26070)
    g = _ffi.schur_analyze(n, m, p["P"], p["A"])
    assert (g["nd"], g["components"], g["largest"], g["sum_size2"], g["nnz_W"], g["accepted"]) == (6672, 23933, 145, 385764, 478133, 1)
    g4 = _ffi.schur_analyze(n, m, p["P"], p["A"], 4)
    assert (g4["nd"], g4["components"], g4["largest"], g4["sum_size2"], g4["nnz_W"], g4["accepted"]) == (5993, 22575, 369, 811318, 972556, 0)
    nd, nc, largest, sumsq, _ = S.components(p["P"], p["A"])
    assert (g["nd"], g["components"], g["largest"], g["sum_size2"]) == (nd, nc, largest, sumsq)


# ---- the stand-alone sanitiser probe ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.fail("no host C++ compiler for tests/schur_plan_probe.cpp")
    tmp = tempfile.mkdtemp(prefix="schur_probe_")
    exe = os.path.join(tmp, "schur_plan_probe")
    csrc = os.path.join(ROOT, "cosmo.jl_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "schur_plan_probe.cpp"), os.path.join(csrc, "schur_plan.cpp")], check=True)
    yield exe
    shutil.rmtree(tmp, ignore_errors=True)


@pytest.mark.parametrize("name", ["wave_switch", "p_zero"])
def test_the_probe_walks_the_maps_under_the_sanitisers(probe, name):
    p = _case(name)
    n, m = p["n"], p["m"]
    P = sp.csr_matrix(p["P"]); A = sp.csr_matrix(p["A"])
    text = "%d %d 3\n" % (n, m) + "\n".join(" ".join(map(str, a.tolist())) for a in (P.indptr, P.indices, A.indptr, A.indices)) + "\n"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([probe], input=text, capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    fig, perm, blocks, entries, ad, adt = None, None, [], {}, [], {}
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "figures":
            fig = list(map(int, w[1:]))
        elif w[0] == "perm":
            perm = list(map(int, w[1:]))
        elif w[0] == "block":
            blocks.append(tuple(map(int, w[1:])))
        elif w[0] == "entry":
            key = (int(w[1]), int(w[2]))
            assert key not in entries
            entries[key] = w[3:]
        elif w[0] == "ad":
            ad.append((int(w[1]), list(map(int, w[2:]))))
        elif w[0] == "adt":
            adt[int(w[1])] = [tuple(map(int, t.split(":"))) for t in w[2:]]
    nd, nc, largest, sumsq, lab = S.components(P, A)
    assert fig[:5] == [nd, nc, largest, sumsq, S.nnz_w(P, A)]
    assert sorted(perm) == list(range(n))
    for k, first, side, off in blocks:                     # every block is one of SciPy's components
        assert len(set(lab[perm[first:first + side]])) == 1 and int((lab == lab[perm[first]]).sum()) == side
    # the sources SciPy's pattern of M_s predicts, entry by entry
    want = {}
    for i in range(n):
        want.setdefault((i, i), []).append("S")
        for k in range(P.indptr[i], P.indptr[i + 1]):
            want.setdefault((i, int(P.indices[k])), []).append("P%d" % k)
    lens = np.diff(A.indptr)
    for r in np.flatnonzero(lens < 3):
        for ka in range(A.indptr[r], A.indptr[r + 1]):
            for kb in range(A.indptr[r], A.indptr[r + 1]):
                want.setdefault((int(A.indices[ka]), int(A.indices[kb])), []).append("A%d:%d:%d" % (ka, kb, r))
    assert set(entries) == set(want)
    Ms = S.ms_pattern(P, A)
    assert set(entries) <= set(zip(*map(lambda a: a.tolist(), Ms.nonzero())))
    for key, terms in entries.items():
        assert sorted(terms) == sorted(want[key]), key
        assert terms[0] == "S" or key[0] != key[1]          # fixed order: sigma first, then P, then the rows of A ascending
        rows = [int(t.split(":")[2]) for t in terms if t[0] == "A"]
        assert rows == sorted(rows)
    long_rows = np.flatnonzero(lens >= 3)
    assert [r for r, _ in ad] == long_rows.tolist()
    for r, src in ad:
        assert src == list(range(A.indptr[r], A.indptr[r + 1]))
    for j, lst in adt.items():
        assert sorted(s for _, s in lst) == sorted(k for r in long_rows for k in range(A.indptr[r], A.indptr[r + 1]) if A.indices[k] == j)
        for kd, s in lst:
            assert A.indptr[long_rows[kd]] <= s < A.indptr[long_rows[kd] + 1]
    assert sum(len(v) for v in adt.values()) == int(lens[long_rows].sum())


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_version_is_unchanged_and_the_new_entry_points_are_declared():
    assert _ffi.ABI_VERSION == 1005
    names = ["cosmo_hip_set_schur_options", "cosmo_hip_schur_analyze", "cosmo_hip_schur_info", "cosmo_hip_schur_residual", "cosmo_hip_batch_group_set_schur_options"]
    header = open(os.path.join(ROOT, "include", "cosmo_hip.h")).read()
    for dtype in (np.float64, np.float32):
        lib = _ffi.load_library(dtype)
        for nm in names:
            assert nm in _ffi.SIGNATURES and hasattr(lib, nm)
            assert "COSMO_HIP_API int32_t %s(" % nm in header
    assert _ffi.KKT_SCHUR == 6 and "COSMO_HIP_KKT_SCHUR = 6" in header
    assert cj.model._KKT_KIND[cj.SchurComplementKKTSolver] == 6
