"""The structures of tests/ldl_structures.py on the CPU (no GPU): what test_gpu_ldl_structures.py relies on.

  * the symbolic analysis (cosmo_hip_ldl_analyze, csrc/ldl_symbolic.cpp) reports the structure every generator promises, and every loop of
    csrc/ldl_dev.h / csrc/ldl.hip that today's small problems never drive past its first trip is reached by a named structure (one test per row of
    the table in ldl_structures.py);
  * the derived backward-error bound holds for a plain NumPy no-pivot LDL' + substitution in Float64 AND Float32, in two summation orders -- the
    bound is not too tight;
  * three emulated kernel faults violate it -- the bound is sharp enough to catch a subtly wrong kernel.

The only tolerance in this file is the bound of ldl_structures.Reference.bound (and cond_est times it for the forward check)."""
import numpy as np
import pytest

import cosmo_jl_amd as cj
from tests import ldl_structures as S

NAMES = list(S.CASES)
DTYPES = [np.float64, np.float32]
# the figures of the default ordering on the three random patterns (cosmo_hip_ldl_analyze; deterministic): pinned as reported
PINNED = {
    "p_zero_300_500": dict(nnz_L=28549, supernodes=591, height=13, max_width=210),
    "empty_lines_300_400": dict(nnz_L=18527, supernodes=533, height=11, max_width=166),
    "default_ordering_medium": dict(nnz_L=147191, supernodes=1083, height=16, max_width=505),
    "default_ordering_large": dict(nnz_L=871036, supernodes=2716, height=16, max_width=1278),
}


def _analyze(st, perm="own"):
    return cj._ffi.ldl_analyze(st.n, st.m, st.P, st.A, st.perm if isinstance(perm, str) else perm)


def _figures(name):
    return S.library_order(S.structure(name))[1]


# ---- the promised structure -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_analysis_reports_the_promised_structure(name):
    st = S.structure(name)
    r = _analyze(st)
    want = dict(st.facts)
    want.update(PINNED.get(name, {}))
    assert want, name
    assert {k: r[k] for k in want} == want
    assert r["amalgamation_zeros"] == 0 and r["nnz_stored"] == r["nnz_L"]
    order, fig = S.library_order(st)
    assert fig["supernodes"] == r["supernodes"]                             # the probe sees the analysis the library reports
    assert sorted(order.tolist()) == list(range(st.N))
    if st.perm is not None:                                                   # a requested ordering is kept up to a postorder of its tree: same last node
        assert order[-1] == st.perm[-1]
        assert _analyze(st, order)["nnz_L"] == r["nnz_L"]
    # P positive semidefinite by construction, checked: K is quasi-definite and the factorisation exists for every ordering
    if (st.P - S.sp.diags(st.P.diagonal())).nnz == 0:
        assert (st.P.diagonal() >= 0).all()
    else:
        assert np.linalg.eigvalsh(st.P.toarray()).min() > 0


# ---- one test per row of the table in ldl_structures.py ----------------------------------------------------------------------------------------
def test_row_factor_panel_scaling_takes_a_second_trip():
    """ldl_factor_sn: for (r = c + 1 + tid; r < nr; r += BS) -- a supernode with more than BS rows"""
    for name in ("dense_block_257", "dense_block_350", "dense_block_700", "tall_panel_4_640", "default_ordering_large"):
        assert _figures(name)["widest_rows"] > S.BS, name
    assert S.structure("dense_block_257").N == S.BS + 1                       # one past the workgroup size
    assert S.structure("dense_block_700").N > 2 * S.BS                        # a third trip
    fig = _figures("tall_panel_4_640")                                        # the 4-wide hub: 640 rows below its block, three trips of 256
    assert fig["rows_below_block"] == 640 > 2 * S.BS


def test_row_forward_gather_and_diagonal_block_take_a_second_trip():
    """ldl_fwd_sn: gather for (b = r0 + tid; b < r1; b += BS) -- a descendant that updates more than BS columns; diagonal block r += BS -- width > BS"""
    for name in ("dense_border_3000_300", "tall_panel_4_640", "default_ordering_medium", "default_ordering_large"):
        assert _figures(name)["gather_columns"] > S.BS, name
    assert _figures("dense_border_3000_300")["gather_columns"] == 300          # every leaf updates all 300 rows of the root
    for name in ("dense_block_257", "dense_block_350", "dense_block_700", "dense_border_3000_300", "default_ordering_large"):
        assert _analyze(S.structure(name))["max_width"] > S.BS, name


def test_row_backward_diagonal_block_takes_a_second_trip():
    """ldl_bwd_sn: for (c = tid; c < r; c += BS) -- a supernode wider than BS"""
    assert _analyze(S.structure("dense_block_257"))["max_width"] == 257
    assert _analyze(S.structure("dense_border_3000_300"))["max_width"] == 301
    assert _analyze(S.structure("tall_panel_4_640"))["max_width"] == 641
    assert _analyze(S.structure("default_ordering_large"))["max_width"] > S.BS      # the issue's condition on the default ordering
    assert _analyze(S.structure("default_ordering_medium"))["max_width"] > S.BS


def test_row_backward_wave_loop_goes_past_its_first_trip():
    """ldl_bwd_sn: for (r = w + lane; r < nr; r += 64) -- more than 64 rows below the diagonal block"""
    assert _figures("tall_panel_4_640")["rows_below_block"] == 640            # ten trips under a block of width 4
    assert _figures("dense_border_3000_300")["rows_below_block"] == 300       # every one of the 2999 leaves
    assert _figures("default_ordering_large")["rows_below_block"] > 64        # the issue's condition on the default ordering
    assert _figures("default_ordering_medium")["rows_below_block"] > 64
    assert _figures("dense_border_3000_5")["rows_below_block"] == 5           # (the short first trip stays covered too)


def test_row_rowpos_searches_a_long_row_list():
    """ldl_rowpos: binary search of a descendant's tail rows in a long rows_J"""
    st = S.structure("tall_panel_4_640")
    assert _figures("tall_panel_4_640")["searched_list"] == 640
    # by construction: the leaf v (column 0) has hub_0 and three rows of A below its diagonal; those rows sit at positions 5, 320 and 639 of the hub's 640
    col = st.A[:, 0].tocoo()
    assert sorted(col.row.tolist()) == st.deep_rows == [5, 320, 639] and st.P[1, 0] != 0
    assert _figures("default_ordering_large")["searched_list"] > 1000
    assert _figures("chain_3000_3")["searched_list"] == 3                     # (and the shortest lists)


def test_row_descendant_loop_runs_thousands_of_descendants():
    """ldl_factor_sn / ldl_fwd_sn: for (d = desc_ptr[J]; ...) with a barrier per descendant -- a supernode with thousands of descendants"""
    assert _figures("dense_border_3000_300")["descendants"] == 2999
    assert _figures("dense_border_3000_5")["descendants"] == 2999
    assert _figures("chain_3000_3")["descendants"] == 2999                    # the fill of the singleton rows reaches the last supernode from every column
    assert _figures("default_ordering_large")["descendants"] > 2000


def test_row_one_launch_per_level_thousands_of_levels():
    """ldl.hip: one k_ldl_factor / k_ldl_fwd / k_ldl_bwd launch per level -- a tree height in the thousands"""
    for name, rows in (("chain_3000_0", 0), ("chain_3000_3", 3)):
        st = S.structure(name)
        r = _analyze(st)
        assert st.m == rows and r["height"] == r["supernodes"]                # one supernode per level: a path
        assert r["height"] >= st.N - 2 - rows
    assert _analyze(S.structure("chain_3000_0"))["height"] == 2999


def test_row_one_level_with_a_very_large_grid():
    """k_ldl_factor: a grid of >= 1e5 workgroups in one level, each adding its positive pivots with atomicAdd(&dstat[1], pos)"""
    for name in ("flat_600000", "flat_600000_absent_diag"):
        r = _analyze(S.structure(name))
        assert r["height"] == 1 and r["supernodes"] == 600000 >= 10 ** 5


def test_row_capped_elementwise_grids_take_a_second_trip():
    """ew() caps the grids of k_ldl_zero / refill / perm / unperm at 4096 workgroups: N and the panel size beyond 4096 * 256 elements"""
    for name in ("flat_600000", "flat_600000_absent_diag"):
        st = S.structure(name)
        r = _analyze(st)
        assert st.N == 1200000 > S.EW_CAP == 1048576                          # k_ldl_perm, k_ldl_unperm
        assert r["panel_size"] == 2400000 > 2 * S.EW_CAP                      # k_ldl_zero: a third trip
        assert st.n + 0 + st.A.nnz + st.m == 1800000 > S.EW_CAP               # k_ldl_refill: [x diagonal | upper P (none) | A | rho diagonal]


def test_row_degenerate_patterns():
    """pdiag[i] < 0 (no stored P_jj), P = 0, m = 0, empty rows / columns of A"""
    st = S.structure("flat_600000_absent_diag")
    stored = np.zeros(st.n, bool)
    stored[st.P.tocoo().row] = True
    assert not stored[1::2].any() and stored[0::2].all()                     # every second P_jj absent from the pattern
    assert np.abs(st.A.data[1::2]).min() >= 16.0                              # (its A entry: the 2 x 2 block stays well conditioned)
    st = S.structure("p_zero_300_500")
    assert st.P.nnz == 0 and st.P.shape == (300, 300)
    assert np.linalg.matrix_rank(st.A.toarray()) == st.n                      # full column rank
    st = S.structure("chain_3000_0")
    assert st.m == 0 and st.A.shape == (0, 3000)
    st = S.structure("empty_lines_300_400")
    assert (np.diff(st.A.tocsr().indptr)[st.empty_rows] == 0).all() and st.empty_rows.size == 58
    assert (np.diff(st.A.tocsc().indptr)[st.empty_cols] == 0).all() and st.empty_cols.size == 60


def test_rho_is_non_uniform_with_equality_rows():
    for name in NAMES:
        st = S.structure(name)
        if st.m == 0:
            continue
        rho = S.rho_vector(st, 1)
        ineq = np.setdiff1d(np.arange(st.m), st.eq_rows)
        assert 0.05 <= rho[ineq].min() and rho[ineq].max() <= 20.0
        if st.m >= 2:
            assert st.eq_rows.size >= 1 and rho[st.eq_rows].min() >= 50.0 and rho[st.eq_rows].max() <= 2e4


# ---- the bound holds for the reference alone --------------------------------------------------------------------------------------------------
_refs = {}


def _reference(name, dtype, order_key="own"):
    key = (name, np.dtype(dtype).name, order_key)
    if key not in _refs:
        st = S.structure(name)
        order, _ = S.library_order(st, st.perm if order_key == "own" else order_key)
        _refs[key] = S.Reference(st, S.rho_vector(st, 1), dtype, order)
    return _refs[key]


def _numpy_solve(ref, rhs, dtype, order, fault=None):
    """the whole solve in NumPy arrays of `dtype`: no-pivot LDL' of the permuted K, then row-oriented substitution"""
    st = ref.st
    if st.closed_form:
        return S.flat_closed_form(st, S.rho_vector(st, 1), dtype, rhs)[2]
    L, d = S.ldl_nopivot(S.permuted_dense(ref.K, ref.perm), dtype, fault=fault)
    x = np.empty(st.N, dtype=dtype)
    x[ref.perm] = S.ldl_solve(L, d, np.asarray(rhs, dtype=dtype)[ref.perm], order)
    return x


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_bound_holds_for_the_reference(name, dtype):
    ref = _reference(name, dtype)
    st = ref.st
    for rname, rhs in S.rhs_pair(st, ref.perm, dtype):
        for order in (("closed_form",) if st.closed_form else ("dot", "reversed")):
            x = _numpy_solve(ref, rhs, dtype, order)
            assert x.dtype == np.dtype(dtype) and np.isfinite(x).all()
            bad, worst = ref.violations(x, rhs)
            print("%s %s %s %s: W = %d, worst |r_i| / bound_i = %.3g" % (name, np.dtype(dtype).name, rname, order, ref.W, worst))
            assert not bad, (rname, order, bad)
            if name in S.WELL_CONDITIONED:
                err, lim = ref.forward_check(x, rhs)
                print("    forward: ||x - x_ref||_inf = %.3g <= %.3g" % (err, lim))
                assert err <= lim, (rname, order, err, lim)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_bound_holds_under_the_other_ordering(dtype):
    """default_ordering_medium under the identity ordering (nearly dense), dense_border_3000_5 under the default ordering: the same K, another factor"""
    for name in ("default_ordering_medium", "dense_border_3000_5"):
        st = S.structure(name)
        other = np.arange(st.N) if st.perm is None else None
        order, _ = S.library_order(st, other)
        ref = S.Reference(st, S.rho_vector(st, 1), dtype, order)
        rname, rhs = S.rhs_pair(st, order, dtype)[0]
        x = _numpy_solve(ref, rhs, dtype, "dot")
        bad, worst = ref.violations(x, rhs)
        print("%s %s other ordering: W = %d, worst ratio %.3g" % (name, np.dtype(dtype).name, ref.W, worst))
        assert not bad, bad


# ---- the bound catches a subtly wrong kernel ----------------------------------------------------------------------------------------------------
def _fault_entry(ref, kind, x, rhs_p):
    """Where to plant the fault: the entry whose error term is the largest share of its row's bound (the issue: among the largest of |L|, with a dense
    nonzero x -- an entry that multiplies a zero, or that drowns among a thousand larger terms of its row, is a fault nobody could see).
    With z = D L' x (so that L z = b), an error e in L[r, c] changes residual component r by e * z_c."""
    fig = S.library_order(ref.st, ref.perm)[1]
    f, nr = fig["widest_first"], fig["widest_rows"]
    L, d = S.ldl_nopivot(S.permuted_dense(ref.K, ref.perm))
    xp = np.asarray(x, dtype=np.float64)[ref.perm]
    z = d * (L.T @ xp)
    bound_p = ref.bound(x)[ref.perm].astype(np.float64)
    N = L.shape[0]
    if kind == "unscaled":          # (a) a row at panel position >= BS of a column of the widest supernode: the second trip of the scaling loop skipped
        assert nr > S.BS and f + nr == N                                      # the widest supernode is the root: panel position = row - f
        cols = np.arange(f, min(f + 32, N - S.BS))
        rows = np.arange(f + S.BS, N)
        share = np.abs(L[np.ix_(rows, cols)] * ((d[cols] - 1.0) * z[cols])[None, :]) / bound_p[rows][:, None]
        i, j = np.unravel_index(np.argmax(share), share.shape)
        return ("unscaled", int(rows[i]), int(cols[j]))
    if kind == "dropped":           # (b) the update of entry (r, c2) by column c is lost: K - L D L' is off by l_rc d_c l_c2c at (r, c2) and (c2, r)
        c = f
        below = np.arange(c + 1, N)
        lc = L[below, c]
        share = np.abs(np.outer(lc, d[c] * lc) * xp[below][None, :]) / bound_p[below][:, None]
        share = np.tril(share, -1)                                            # r > c2
        i, j = np.unravel_index(np.argmax(share), share.shape)
        return ("dropped", int(below[i]), int(below[j]), int(c))
    rel = 1e-6 if ref.dtype == np.float64 else 1e-2   # (c) one entry of L off by a relative 1e-6 / 1e-2
    Ls = S.sp.coo_matrix(np.tril(L, -1))
    share = np.abs(Ls.data * z[Ls.col]) / bound_p[Ls.row]
    k = int(np.argmax(share))
    return ("perturbed", int(Ls.row[k]), int(Ls.col[k]), rel)


@pytest.mark.parametrize("kind", ["unscaled", "dropped", "perturbed"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["dense_block_350", "default_ordering_large"])
def test_bound_catches_an_emulated_kernel_fault(name, dtype, kind):
    ref = _reference(name, dtype)
    st = ref.st
    rname, rhs = S.rhs_pair(st, ref.perm, dtype)[0]                           # dense and nonzero: standard normal
    good = _numpy_solve(ref, rhs, dtype, "dot")
    assert not ref.violations(good, rhs)[0]
    fault = _fault_entry(ref, kind, good, None)
    x = _numpy_solve(ref, rhs, dtype, "dot", fault=fault)
    assert not np.array_equal(x, good), fault                                 # the fault did change the solution
    bad, worst = ref.violations(x, rhs)
    print("%s %s %s: |r_i| / bound_i = %.3g at the worst component (fault-free: %.3g)" % (name, np.dtype(dtype).name, (fault,), worst,
                                                                                        ref.violations(good, rhs)[1]))
    assert bad, (fault, worst)
