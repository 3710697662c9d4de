"""tests/krylov_cases.py on the CPU: the reference is as good as it claims, every case reaches the path it is named for under the library's own
rules (restated in the case module), the tolerance sits 256 floors up, the oracle stays inside every bound the GPU test applies, the drift
constant is the measured one, and the bounds catch emulated kernel faults."""
import numpy as np
import pytest

from tests import krylov_cases as K

F32_CASES = sorted({c for c, _, _ in K.F32_RUNS})
PLANS = [(c, "f64") for c in K.CASES] + [(c, "f32") for c in F32_CASES]


@pytest.mark.parametrize("name,dtype_name", PLANS, ids=["%s-%s" % p for p in PLANS])
def test_reference_residual_and_tolerance(name, dtype_name):
    pl = K.plan(name, dtype_name)
    for s in pl.solves:
        print("%s %s: own relative residual %.2e, floor %.3e, abstol = %.1f floors" % (name, dtype_name, s.own_residual, s.floor, s.abstol / s.floor))
        assert s.own_residual <= K.REFERENCE_RESIDUAL_LIMIT
        assert s.abstol >= K.FLOOR_MARGIN * s.floor * (1 - 1e-12)                  # T / ||b|| >= 256 floors for every right-hand side of the case
    assert min(s.abstol / s.floor for s in pl.solves) <= K.FLOOR_MARGIN * (1 + 1e-12)  # ... and T is the smallest such value
    # M itself: symmetric, and the same matrix as the dense definition P + sigma I + A' rho A at Float64 accuracy
    for ref in (pl.ref1, pl.ref2):
        cs = pl.case
        A = cs.A.astype(pl.dtype).astype(np.float64).toarray()
        dense = cs.P.astype(pl.dtype).astype(np.float64).toarray() + float(ref.sigma) * np.eye(cs.n) + A.T @ (ref.rho.astype(np.float64)[:, None] * A)
        assert np.array_equal(ref.M, ref.M.T)
        assert np.max(np.abs(ref.M64 - dense)) <= 64 * np.finfo(np.float64).eps * np.max(np.abs(dense))


def test_row_blocks_cover_the_rows_and_respect_the_tile():
    rng = np.random.default_rng(5)
    for tile in (64, 256, 768, 2048):
        lens = rng.integers(0, 40, 900)
        lens[17] = 3000                                                              # a single long row: its own tile
        ptr = np.concatenate([[0], np.cumsum(lens)])
        rb = K.row_blocks(ptr, tile)
        assert rb[0] == 0 and rb[-1] == 900 and all(a < b for a, b in zip(rb, rb[1:]))
        for a, b in zip(rb, rb[1:]):
            assert ptr[b] - ptr[a] <= tile or b - a == 1
            assert b - a <= (K.BS if tile < K.NNZ_PER_BLOCK else 4 * K.BS)


@pytest.mark.parametrize("name", K.CASES)
def test_case_takes_the_path_it_is_named_for(name):
    cs = K.case(name)
    lens = cs.row_len
    assert K.split_ok(cs), "the operator split is refused: no assembled operator"
    assert (np.bincount(cs.A.tocsr()[lens == 1].indices, minlength=cs.n) >= 1).all()       # a bound row on every column
    full = {sl: K.fold_plan(cs, K.TILES[sl]) for sl in K.ALL_SL}
    part = {sl: K.fold_plan(cs, K.TILES[sl], 4) for sl in K.ALL_SL}
    for sl in K.ALL_SL:
        assert full[sl]["enabled"] == 1 and full[sl]["slots"] == sl and full[sl]["gate"][0] <= full[sl]["gate"][1]
    coupling = lens[lens != 1]
    if name in ("one_tile", "one_tile_f"):
        assert cs.n == 40 and all(full[sl]["tiles"] == 1 and full[sl]["stored_entries"] <= K.BS for sl in K.ALL_SL)
        if name == "one_tile":
            assert (coupling == 3).all() and len(coupling) == 12 and full[1]["stored_entries"] == 186
            assert all(part[sl]["factored_rows"] == 0 for sl in K.ALL_SL)              # rows of 3 cannot stay factored: one_tile_f is the case for that
        else:
            assert (coupling == 4).all() and all(part[sl]["factored_rows"] == 10 and part[sl]["tiles"] == 1 for sl in K.ALL_SL)
    if name.startswith("edge_257"):
        assert cs.n == K.BS + 1 and (coupling == 0).sum() == 2 and set(coupling[coupling > 0]) == {2, 3, 4, 5, 6}
        P = cs.P.toarray()
        offdiag_tail = P[:, 157:] - np.diag(np.diag(P))[:, 157:]
        assert not offdiag_tail.any() and (np.diag(P)[157:] != 0).all() == (name == "edge_257_pd") and (name == "edge_257_pd" or not P[:, 157:].any())
        assert cs.A.tocsc()[:, 256].nnz >= 3                                           # the element past the workgroup is coupled, not only bounded
        assert full[1]["tiles"] > 1 and part[1]["factored_rows"] > 0
    if name == "mixed_700":
        assert cs.n == 700 and len(coupling) == 120 and coupling.min() == 3 and coupling.max() == 12 and int(cs.eq.sum()) == 30
        assert full[1]["tiles"] > K.GRID_CAP and part[1]["tiles"] > K.GRID_CAP            # COSMO_HIP_GRID_CAP=64 at tile 256: a workgroup folds several tiles
        assert all(1 < full[sl]["tiles"] for sl in K.ALL_SL) and part[3]["factored_rows"] == int((coupling >= 4).sum())
        assert part[3]["max_slots_per_column"] > 2
    if name == "hub_2304":
        assert cs.n == 2304 and cs.P.nnz == 0
        assert all(full[sl]["longest_row"] == 2304 > K.TILES[sl] for sl in (1, 3, 8))     # the full row exceeds every tile: the generic chunked path
        assert full[8]["tile_fill"] == 2304
    if name == "factored_long":
        assert cs.n < 1500
        for sl in (3, 8):
            p = part[sl]
            assert p["factored_rows"] == 151 and p["ad_longest_tile"] == K.LONG_ROW > K.ADSL * K.BS and p["ad_tiles"] >= 2
            assert p["max_slots_per_column"] > 2                                       # columns in more than two image slots: the overflow list
            assert p["tiles"] <= K.MAX_PARTIALS


def test_run_lists_cover_every_tile_form_of_every_recurrence():
    for rec in K.ASSEMBLED:
        assert {sl for _, r, sl in K.ASSEMBLED_RUNS if r == rec} == set(K.ALL_SL), rec
    for name, rec, sl in K.ASSEMBLED_RUNS:
        p = K.fold_plan(K.case(name), K.TILES[sl], K.factor_min_of(rec))
        assert p["enabled"] == 1 and p["slots"] == sl and (p["factored_rows"] > 0) == K.ASSEMBLED[rec][4], (name, rec, sl)
        assert K.ASSEMBLED[rec][1] in K.oracle_kinds(name), (name, rec)
    assert {(c, sl) for c, _, sl in K.F32_RUNS} == {(c, sl) for c in ("one_tile", "mixed_700") for sl in (1, 3, 8)}
    for rec in K.FULL + K.PARTIAL:                                                       # the full cross product on the one-tile cases and mixed_700
        assert {sl for c, r, sl in K.ASSEMBLED_RUNS if r == rec and c == "mixed_700"} == set(K.ALL_SL)
        assert {sl for c, r, sl in K.ASSEMBLED_RUNS if r == rec and c in ("one_tile", "one_tile_f")} == set(K.ALL_SL)


ORACLE_RUNS = [(c, kind, "f64") for c in K.CASES for kind in K.oracle_kinds(c)] + [(c, "CG", "f32") for c in F32_CASES]


@pytest.mark.parametrize("name,kind,dtype_name", ORACLE_RUNS, ids=["%s-%s-%s" % r for r in ORACLE_RUNS])
def test_oracle_stays_inside_every_bound(name, kind, dtype_name):
    seq = K.oracle_sequence(name, kind, dtype_name)
    n = K.case(name).n
    assert K.verify(name, dtype_name, kind, seq, "oracle " + kind) == []
    ks = [k for _, k in seq]
    if (name, kind) in K.RUNS_TO_MAXITER:
        assert max(ks[:2]) < n and ks[2] == n, "the listed pair no longer runs to maxiter: take it off the list"
    else:
        assert max(ks) < n and min(ks[:3]) > 0 and ks[3] <= 1


@pytest.mark.parametrize("name,kind,dtype_name", ORACLE_RUNS, ids=["%s-%s-%s" % r for r in ORACLE_RUNS])
def test_krylov_counts_do_not_depend_on_the_rounding(name, kind, dtype_name):
    """A kernel that sums in another order is another rounding of the same recurrence.  On a case whose residual swings around the threshold the count
    then moves by more than the allowance with no fault anywhere (an earlier factored_long: 104 .. 112 for an oracle count of 104): the count check of
    such a case decides nothing.  Here: over eight other roundings of the oracle's own sequence the count moves by at most the allowance minus one."""
    base, dev, worst = K.count_spread(name, kind, dtype_name)
    print("%s %s %s: oracle counts %s, largest change under another rounding %s" % (name, kind, dtype_name, base, dev))
    listed = (name, kind) in K.RUNS_TO_MAXITER
    for step in range(3):
        if listed and step == 2:
            assert dev[step] == 0                                  # every rounding runs to n
        else:
            assert dev[step] + 1 <= K.krylov_allowance(base[step]), (step, base, dev)
    assert listed or worst[3] <= 1


@pytest.mark.parametrize("name", K.CASES)
def test_the_drift_constant_is_the_measured_one(name):
    d = K.measure_drift(name)
    print("%s: worst (true residual - threshold) / floor at stagnation = %.3f (recorded %.2f)" % (name, d, K.ORACLE_WORST_DRIFT_BY_CASE[name]))
    assert d <= K.ORACLE_WORST_DRIFT_BY_CASE[name]
    assert K.C_DRIFT == max(16.0, 16.0 * max(K.ORACLE_WORST_DRIFT_BY_CASE.values()))


@pytest.mark.parametrize("name", ["one_tile", "mixed_700"])
def test_the_bounds_catch_emulated_faults(name):
    cs = K.case(name)
    n = cs.n
    good = K.oracle_sequence(name, "CG")

    def broken(step, change):
        seq = [(sol.copy(), k) for sol, k in good]
        change(seq[step][0])
        return {s for s, _ in K.verify(name, "f64", "CG", seq, "emulated fault")}

    def one_entry_of_x(sol):                  # one row of M applied with one term missing moves x by far more than this
        sol[n // 2] *= 1 + 1e-6
    def one_row_of_nu(sol):
        sol[n + cs.m - 1] *= 1 + 1e-9
    def stale_rho(sol):                       # nu formed with rho where rho' holds
        sol[n:] *= cs.rho / cs.rho2

    assert broken(1, one_entry_of_x) == {1}
    assert broken(0, one_row_of_nu) == {0}
    assert broken(2, stale_rho) == {2}
    # the solution of the previous rho returned after update_rho (k_fold_refresh skipped): residual far above the bound
    seq = [(sol.copy(), k) for sol, k in good]
    seq[2] = (seq[0][0].copy(), seq[2][1])
    assert 2 in {s for s, _ in K.verify(name, "f64", "CG", seq, "stale operator")}
    # a Krylov count off by more than the allowance
    seq = [(sol.copy(), k) for sol, k in good]
    seq[0] = (seq[0][0], int(seq[0][1] * 1.1) + 3)
    assert {s for s, _ in K.verify(name, "f64", "CG", seq, "count")} == {0}
