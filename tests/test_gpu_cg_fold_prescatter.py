"""The PRE-SCATTERED image of the factored rows of A (csrc/cg_fold.hip: k_cg_dirMs + k_cg_updF<2>; COSMO_HIP_FOLD_PRESCATTER): a tile-major padded copy of
the dense rows Ad with r_j and c_j kept in slot order by the kernels that write r and c, so that a dense-tile workgroup of the update kernel needs one
memory round trip instead of descriptor -> columns -> gathers.  Only where operands come from changes: every test compares the form against the CSR-stream
form (COSMO_HIP_FOLD_PRESCATTER=0, k_cg_updF0) under COSMO_HIP_FOLD_FACTOR=1 BIT FOR BIT -- x, s, y, Krylov totals, rho updates -- on shapes that take every
path of the image: columns shared by several dense rows, columns in none, a column whose slots lie in two tiles, one dense row, more than 256 dense rows,
n < 256, a single row longer than a tile (declined by the image), rho adaptation, the captured chain, zero-iteration and maxiter solves, Float32."""
import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj

pytestmark = pytest.mark.gpu

ADSL_TILE = 4 * 256          # nonzeros of a dense-row tile (cg_fold.hip: ADSL * COSMO_BS)
FILL_DEFAULT = 300000        # kkt.hip: FOLD_FACTOR_FILL_DEFAULT


def bounds_qp(n=1500, nrows=40, seed=3):
    """tests/test_gpu_cg_fold.py: QP with a general sparse P, simple bounds on every variable and a few dense-ish coupling rows."""
    rng = np.random.default_rng(seed)
    S = sp.random(n, n, density=3.0 / n, random_state=rng, format="csc", data_rvs=lambda k: 0.2 * rng.standard_normal(k))
    Ps = (S + S.T).tocsc()
    P = (Ps + sp.diags(np.asarray(abs(Ps).sum(axis=1)).ravel() + rng.uniform(0.1, 1.0, n))).tocsc()
    P.sort_indices()
    G = sp.random(nrows, n, density=12.0 / n, random_state=rng, format="csc", data_rvs=rng.standard_normal)
    x0 = rng.standard_normal(n)
    A = sp.vstack([-sp.eye(n), -G], format="csc"); A.sort_indices()
    lo = np.concatenate([x0 - np.abs(rng.standard_normal(n)), G @ x0 - 0.1])
    hi = np.concatenate([x0 + np.abs(rng.standard_normal(n)), G @ x0 + 0.1])
    hi[n:n + nrows // 4] = lo[n:n + nrows // 4]                      # some equality rows: rho class x 1e3
    return dict(P=P, q=rng.standard_normal(n), A=A, b=np.zeros(n + nrows), sets=[cj.Box(lo, hi)])


PROBLEMS = {
    "chordal_sdp": lambda: cj.problems.chordal_sdp(ncliques=12, dmin=4, dmax=70, sep_min=1, sep_max=3, n_total=2500, n_zero=40, n_nonneg=80),
    "bounds_qp": bounds_qp,
}


def dense_rows_qp(n, row_lens, col_hi=None, p_per_row=3.0, seed=5):
    """Bounds on every variable (single-nonzero rows of A) + coupling rows with exactly row_lens[k] nonzeros in the columns [0, col_hi): the rows that stay
    factored.  col_hi < n leaves columns that occur in no dense row; few columns and many rows make every column occur in several rows.  (The operator is
    split, and then assembled, only where the single-nonzero rows hold at least half of nnz(A): n >= sum(row_lens).)"""
    rng = np.random.default_rng(seed)
    col_hi = n if col_hi is None else col_hi
    S = sp.random(n, n, density=p_per_row / n, random_state=rng, format="csc", data_rvs=lambda k: 0.2 * rng.standard_normal(k))
    Ps = (S + S.T).tocsc()
    P = (Ps + sp.diags(np.asarray(abs(Ps).sum(axis=1)).ravel() + rng.uniform(0.1, 1.0, n))).tocsc()
    P.sort_indices()
    rows, cols, vals = [], [], []
    for k, ln in enumerate(row_lens):
        cc = rng.choice(col_hi, size=ln, replace=False)
        rows += [k] * ln; cols += list(cc); vals += list(rng.standard_normal(ln))
    nrows = len(row_lens)
    G = sp.csc_matrix((vals, (rows, cols)), shape=(nrows, n))
    x0 = rng.standard_normal(n)
    A = sp.vstack([-sp.eye(n), -G], format="csc"); A.sort_indices()
    lo = np.concatenate([x0 - np.abs(rng.standard_normal(n)), G @ x0 - 0.1])
    hi = np.concatenate([x0 + np.abs(rng.standard_normal(n)), G @ x0 + 0.1])
    hi[n:n + (nrows + 3) // 4] = lo[n:n + (nrows + 3) // 4]
    return dict(P=P, q=rng.standard_normal(n), A=A, b=np.zeros(n + nrows), sets=[cj.Box(lo, hi)])


TIGHT = dict(kkt_solver=cj.with_options(cj.CGIndirectKKTSolver, tol_constant=1e-10, tol_exponent=0.0))
FIXED = dict(eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9)


def _solve(monkeypatch, prob, iters, factor="1", prescatter=None, dtype=None, env=(), **st_kw):
    for k in ("COSMO_HIP_FOLD_FACTOR", "COSMO_HIP_FOLD_PRESCATTER", "COSMO_HIP_CG_GRAPH", "COSMO_HIP_CG_GRAPH_LEN"):
        monkeypatch.delenv(k, raising=False)
    if factor is not None:
        monkeypatch.setenv("COSMO_HIP_FOLD_FACTOR", factor)
    if prescatter is not None:
        monkeypatch.setenv("COSMO_HIP_FOLD_PRESCATTER", prescatter)
    for k, v in env:
        monkeypatch.setenv(k, v)
    md = cj.Model() if dtype is None else cj.Model(dtype=dtype)
    md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], cj.Settings(max_iter=iters, **st_kw))
    r = cj.optimize(md)
    return md, r


def _same_bits(a, b):
    assert np.array_equal(a.x, b.x) and np.array_equal(a.s, b.s) and np.array_equal(a.y, b.y)
    assert a.kkt_iters_total == b.kkt_iters_total > 0
    assert list(a.info.rho_updates) == list(b.info.rho_updates)


def _both_forms(monkeypatch, prob, iters, rows=None, **kw):
    """(pre-scattered, CSR-stream) runs of the factored operator; the forms really ran."""
    md1, r1 = _solve(monkeypatch, prob, iters, prescatter="1", **kw)
    fs = md1.handle.fold_stats()
    assert fs["enabled"] == 1 and fs["factored_rows"] > 0, fs
    if rows is not None:
        assert fs["factored_rows"] == rows, fs
    assert "PRESCATTER" not in md1.handle.kkt_recurrence()
    md0, r0 = _solve(monkeypatch, prob, iters, prescatter="0", **kw)
    assert md0.handle.fold_stats() == fs and "COSMO_HIP_FOLD_PRESCATTER=0" in md0.handle.kkt_recurrence()
    _same_bits(r1, r0)
    return r1, r0


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_prescattered_rows_match_the_csr_stream_form_bit_for_bit(name, monkeypatch):
    """The two instances of tests/test_gpu_cg_fold.py in tight mode; the chordal SDP also against the fully assembled operator at the fold tests' tolerances
    (1e-7 trajectories, Krylov totals +-1 per solve)."""
    prob = PROBLEMS[name]()
    iters = 60
    r1, _ = _both_forms(monkeypatch, prob, iters, **FIXED, **TIGHT)
    if name == "chordal_sdp":
        md2, r2 = _solve(monkeypatch, prob, iters, factor="0", **FIXED, **TIGHT)
        assert md2.handle.fold_stats()["enabled"] == 1 and md2.handle.fold_stats()["factored_rows"] == 0
        assert abs(r1.kkt_iters_total - r2.kkt_iters_total) <= iters + 1, (r1.kkt_iters_total, r2.kkt_iters_total)
        for a, b in ((r1.x, r2.x), (r1.s, r2.s), (r1.y, r2.y)):
            assert np.max(np.abs(a - b)) <= 1e-7 * max(1.0, float(np.max(np.abs(b))))


SHAPES = {
    # 120 rows x 20 nonzeros in 200 of 2500 columns: three tiles; every used column occurs ~12 times (two slots in its record, the rest in the overflow list) and
    # in more than one tile; the other columns occur in no dense row
    "shared_columns_three_tiles": (lambda: dense_rows_qp(2500, [20] * 120, col_hi=200), 120),
    "one_dense_row": (lambda: dense_rows_qp(400, [12], seed=6), 1),
    # 300 rows x 4 nonzeros: the first tile is full by rows AND by nonzeros (256 rows, 1024 nonzeros), the second holds 44 rows
    "more_rows_than_a_tile": (lambda: dense_rows_qp(1300, [4] * 300, seed=7), 300),
    "n_below_256": (lambda: dense_rows_qp(100, [9, 5, 17, 30, 4, 8, 11], col_hi=80, seed=8), 7),
    # a row of 1030 nonzeros is a tile of its own beyond the 1024 slots of the image (generic path, no slots) between ordinary tiles; P is dense enough that the
    # assembly's cost gate (terms <= 6 x streamed entries) still accepts the 1030^2 terms
    "row_longer_than_a_tile": (lambda: dense_rows_qp(2500, [20] * 30 + [ADSL_TILE + 6] + [25] * 30, p_per_row=48.0, seed=9), 61),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shapes_of_the_image(shape, monkeypatch):
    build, rows = SHAPES[shape]
    _both_forms(monkeypatch, build(), 25, rows=rows, **FIXED, **TIGHT)


def test_rho_adaptation_reaches_the_image(monkeypatch):
    """Default schedule (loose Krylov tolerance, rho adapted on the device): the refreshed values of [Ms | Ad' rho] and the image's operands stay consistent."""
    r1, _ = _both_forms(monkeypatch, PROBLEMS["chordal_sdp"](), 130, eps_abs=0.0, eps_rel=0.0, kkt_solver=cj.CGIndirectKKTSolver)
    assert len(r1.info.rho_updates) >= 2


def test_captured_chain_against_direct_launches(monkeypatch):
    """An odd requested chain length (rounded up: the slot-ordered r alternates by parity like the records), COSMO_HIP_CG_GRAPH=0 against 1, and both against
    the CSR-stream form."""
    prob = PROBLEMS["chordal_sdp"]()
    res = {}
    for ps in ("1", "0"):
        for graph in ("0", "1"):
            md, res[ps, graph] = _solve(monkeypatch, prob, 90, prescatter=ps, env=(("COSMO_HIP_CG_GRAPH", graph), ("COSMO_HIP_CG_GRAPH_LEN", "3")), **FIXED)
            assert md.handle.fold_stats()["factored_rows"] > 0
    for key in (("1", "1"), ("0", "0"), ("0", "1")):
        _same_bits(res["1", "0"], res[key])


def test_zero_iteration_and_maxiter_solves(monkeypatch):
    """AbstractKKTSolver.solve! directly: a start residual that already meets the tolerance (cg! compares ||r|| with tol / ||rhs||: a tiny right-hand side) ends
    with zero Krylov iterations, a tolerance of zero ends at maxiter = n; then an ordinary solve on the same handle (the next solve start refills the slots)."""
    prob = dense_rows_qp(100, [9, 5, 17, 30, 4, 8, 11], col_hi=80, seed=8)
    out = {}
    for ps in ("1", "0"):
        res = []
        for tolc in (1.0, 0.0):
            md, _ = _solve(monkeypatch, prob, 3, prescatter=ps, scaling=0, adaptive_rho=False, **FIXED,
                           kkt_solver=cj.with_options(cj.CGIndirectKKTSolver, tol_constant=tolc, tol_exponent=0.0))
            h = md.handle
            assert h.fold_stats()["factored_rows"] == 7
            n, m = md.n, md.m
            g = np.random.default_rng(23).standard_normal(n + m)
            for rhs in ((1e-9 / np.linalg.norm(g)) * g, 50.0 * g):
                sol, its = h.kkt_solve(rhs)
                res.append((sol, its))
        out[ps] = res
    its = [t for _, t in out["1"]]
    assert its[0] == 0 and 0 < its[1] <= 100 and its[2] == 100 and its[3] == 100, its
    for (a, ia), (b, ib) in zip(out["1"], out["0"]):
        assert ia == ib and np.array_equal(a, b)


def test_float32_library(monkeypatch):
    prob = PROBLEMS["chordal_sdp"]()
    md1, r1 = _solve(monkeypatch, prob, 60, prescatter="1", dtype=np.float32, **FIXED)
    assert md1.handle.dtype == np.float32 and md1.handle.fold_stats()["factored_rows"] > 0
    md0, r0 = _solve(monkeypatch, prob, 60, prescatter="0", dtype=np.float32, **FIXED)
    assert r1.x.dtype == np.float32
    _same_bits(r1, r0)


def test_default_rule(monkeypatch):
    """No switch set: rows stay factored only where that avoids at least FOLD_FACTOR_FILL_DEFAULT assembled entries (sum of len^2 - 2 len over the rows);
    COSMO_HIP_FOLD_FACTOR=0 forces the assembled form there."""
    for name in sorted(PROBLEMS):
        md, _ = _solve(monkeypatch, PROBLEMS[name](), 2, factor=None, **FIXED)
        fs = md.handle.fold_stats()
        assert fs["enabled"] == 1 and fs["factored_rows"] == 0 and "partially" not in md.handle.kkt_recurrence(), (name, fs)
    rows, ln = 360, 30
    assert rows * (ln * ln - 2 * ln) >= FILL_DEFAULT > (rows - 20) * (ln * ln - 2 * ln)
    for nrows, factored in ((rows, rows), (rows - 20, 0)):
        prob = dense_rows_qp(11000, [ln] * nrows, seed=10)
        md, _ = _solve(monkeypatch, prob, 2, factor=None, **FIXED)
        fs = md.handle.fold_stats()
        assert fs["enabled"] == 1 and fs["factored_rows"] == factored, fs
        assert ("partially assembled" in md.handle.kkt_recurrence()) == (factored > 0)
    md, _ = _solve(monkeypatch, dense_rows_qp(11000, [ln] * rows, seed=10), 2, factor="0", **FIXED)
    assert md.handle.fold_stats()["factored_rows"] == 0
