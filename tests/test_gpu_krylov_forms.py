"""The CG routes of a bare handle, ONE KKT solve at a time, in every tile form the assembled-operator kernels compile: k_cg_dirM<SL, PC>,
k_cg_dirMs<SL, PSM>, k_sr_M<SL> (csrc/cg_fold.hip, csrc/cg_sr.hip) at SL = 1, 2, 3, 4, 8, with the padded copy, without the XCD-affine tile order
and with fewer workgroups than tiles, plus the unassembled recurrences -- each against a dense high-precision solve of the same system.

tests/krylov_cases.py holds the structures, the reference, the bounds (all derived there: residual <= abstol + C floor, nu row by row, Krylov
counts against the oracle) and the list of forms; tests/test_krylov_cases_host.py proves on the CPU which path every structure takes and that
the oracle itself stays inside the bounds.

Per (case, form), on a fresh handle with the switches set before it is created:  set_problem -> set_cones -> set_params(rho) ->
  1. rhs1 from the cold start      2. rhs2 from the warm start x1 (the start residual with x != 0, k_ad_dot on factored rows)
  3. update_rho(rho'), rhs1 against the reference of rho' (k_fold_refresh, the padded values, the Jacobi diagonal)
  4. rhs1 again: k <= 1            5. a zero right-hand side on a fresh handle: exact zeros, k = 0
fold_stats() and kkt_recurrence() are compared with the plan restated on the host, so a case that falls onto another route fails."""
import faulthandler

import numpy as np
import pytest

import cosmo_jl_amd as cj
from tests import krylov_cases as K

pytestmark = pytest.mark.gpu
F = cj._ffi
KINDS = {"CG": F.KKT_CG, "CG_JACOBI": F.KKT_CG_JACOBI, "CG_SR": F.KKT_CG_SR}
CASE_LIMIT_S = 120


@pytest.fixture(autouse=True)
def _case_time_limit():
    """a case that hangs takes the whole process down instead of holding the GPU: nothing runs after a hang"""
    faulthandler.dump_traceback_later(CASE_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _handle(monkeypatch, name, dtype_name, kind, env):
    for k in K.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pl = K.plan(name, dtype_name)
    cs = pl.case
    h = F.Handle(0, dtype=pl.dtype)
    h.set_problem(cs.P, np.zeros(cs.n), cs.A, np.zeros(cs.m))
    h.set_cones([F.NONNEG], [cs.m])
    p = h.default_params()
    p.kkt_kind = KINDS[kind]
    p.sigma = K.SIGMA
    p.tol_constant, p.tol_exponent = pl.T, 0.0
    p.adaptive_rho = 0
    h.set_params(p, rho_vec=cs.rho.astype(pl.dtype))
    return h


def _sequence(h, name, dtype_name):
    cs, dt = K.case(name), K.DTYPES[dtype_name]
    out = [h.kkt_solve(cs.rhs1.astype(dt)), h.kkt_solve(cs.rhs2.astype(dt))]
    h.update_rho(cs.rho2.astype(dt))
    assert np.array_equal(h.get_rho_vec(), cs.rho2.astype(dt))
    out += [h.kkt_solve(cs.rhs1.astype(dt)), h.kkt_solve(cs.rhs1.astype(dt))]
    assert all(sol.dtype == np.dtype(dt) for sol, _ in out)
    return out


def _zero_rhs(monkeypatch, name, dtype_name, kind, env):
    h = _handle(monkeypatch, name, dtype_name, kind, env)
    try:
        cs = K.case(name)
        sol, k = h.kkt_solve(np.zeros(cs.n + cs.m))
        assert k == 0 and not np.isnan(sol).any() and not sol.any(), (k, sol[np.flatnonzero(sol)[:5]])
    finally:
        h.close()


def _check_plan(h, name, recurrence, sl, tile):
    """the handle runs the form that was asked for: the assembled operator, its factored rows, its tiles, and the <SL, ...> instantiation"""
    kind, _, _, route, factored = K.ASSEMBLED[recurrence]
    want = K.fold_plan(K.case(name), tile, K.factor_min_of(recurrence))
    fs = h.fold_stats()
    rec = h.kkt_recurrence()
    print("%s %s SL = %d: %s; %s" % (name, recurrence, sl, rec, fs))
    assert fs["enabled"] == 1 and fs["factored_rows"] == want["factored_rows"] and (fs["factored_rows"] > 0) == factored, (fs, want)
    assert fs["tiles"] == want["tiles"] and fs["stored_entries"] == want["stored_entries"], (fs, want)
    if factored:
        assert rec.startswith("cg: literal recurrence on the partially assembled operator (%d rows of A kept factored)" % want["factored_rows"]) and rec.endswith(route % sl), rec
    else:
        assert rec == route % sl
    return fs


def _run_form(monkeypatch, name, dtype_name, recurrence, sl, extra=None, tile=None):
    kind, oracle_kind, env, _, _ = K.ASSEMBLED[recurrence]
    tile = K.TILES[sl] if tile is None else tile
    env = dict(env, COSMO_HIP_FOLD_TILE=str(tile), **(extra or {}))
    h = _handle(monkeypatch, name, dtype_name, kind, env)
    try:
        fs = _check_plan(h, name, recurrence, sl, tile)
        route = h.kkt_recurrence()
        out = _sequence(h, name, dtype_name)
        assert h.kkt_recurrence() == route and h.fold_stats() == fs
    finally:
        h.close()
    return out, fs, oracle_kind, env


def _same_bits(a, b):
    return all(ka == kb and np.array_equal(sa, sb) for (sa, ka), (sb, kb) in zip(a, b))


@pytest.mark.parametrize("name,recurrence,sl", K.ASSEMBLED_RUNS, ids=["%s-%s-SL%d" % r for r in K.ASSEMBLED_RUNS])
def test_assembled_form_against_the_dense_solve(name, recurrence, sl, monkeypatch):
    out, _, oracle_kind, env = _run_form(monkeypatch, name, "f64", recurrence, sl)
    assert K.verify(name, "f64", oracle_kind, out, "%s SL = %d" % (recurrence, sl)) == []
    _zero_rhs(monkeypatch, name, "f64", K.ASSEMBLED[recurrence][0], env)


@pytest.mark.parametrize("name,recurrence,sl", K.F32_RUNS, ids=["%s-%s-SL%d" % r for r in K.F32_RUNS])
def test_float32_library_against_the_dense_solve(name, recurrence, sl, monkeypatch):
    out, _, oracle_kind, env = _run_form(monkeypatch, name, "f32", recurrence, sl)
    assert K.verify(name, "f32", oracle_kind, out, "%s SL = %d" % (recurrence, sl)) == []
    _zero_rhs(monkeypatch, name, "f32", K.ASSEMBLED[recurrence][0], env)


@pytest.mark.parametrize("sl", [1, 2, 4])
@pytest.mark.parametrize("recurrence", ["literal", "jacobi"])
def test_padded_copy_is_bit_identical_at_every_tile_it_exists_for(recurrence, sl, monkeypatch):
    """COSMO_HIP_FOLD_PAD=1 (tile-major padded (col, val), refreshed by k_fold_refresh after update_rho) against the CSR arrays: the same bits"""
    pad, _, oracle_kind, _ = _run_form(monkeypatch, "mixed_700", "f64", recurrence, sl, {"COSMO_HIP_FOLD_PAD": "1"})
    csr, _, _, _ = _run_form(monkeypatch, "mixed_700", "f64", recurrence, sl, {"COSMO_HIP_FOLD_PAD": "0"})
    assert K.verify("mixed_700", "f64", oracle_kind, pad, "%s SL = %d padded" % (recurrence, sl)) == []
    assert _same_bits(pad, csr)


@pytest.mark.parametrize("recurrence", ["literal", "jacobi", "sr", "partial_ps2"])
def test_tile_order_does_not_change_the_bits(recurrence, monkeypatch):
    """COSMO_HIP_XCD_AFFINE=0: partials are indexed by tile and grid == nb, so the identity order gives the same bits"""
    ident, _, oracle_kind, _ = _run_form(monkeypatch, "mixed_700", "f64", recurrence, 3, {"COSMO_HIP_XCD_AFFINE": "0"})
    affine, _, _, _ = _run_form(monkeypatch, "mixed_700", "f64", recurrence, 3)
    assert K.verify("mixed_700", "f64", oracle_kind, ident, "%s identity tile order" % recurrence) == []
    assert _same_bits(ident, affine)


@pytest.mark.parametrize("recurrence", ["literal", "jacobi", "sr", "partial_ps2", "partial_ps1", "partial_csr"])
def test_fewer_workgroups_than_tiles(recurrence, monkeypatch):
    """COSMO_HIP_GRID_CAP=64 at tile 256: every workgroup folds several tiles (the grid-stride path, the partials summed in another order)"""
    out, fs, oracle_kind, _ = _run_form(monkeypatch, "mixed_700", "f64", recurrence, 1, {"COSMO_HIP_GRID_CAP": str(K.GRID_CAP)})
    assert fs["tiles"] > K.GRID_CAP
    assert K.verify("mixed_700", "f64", oracle_kind, out, "%s grid cap" % recurrence) == []


UNASSEMBLED_RUNS = [(c, r) for r in K.UNASSEMBLED for c in K.UNASSEMBLED_CASES]


@pytest.mark.parametrize("name,route", UNASSEMBLED_RUNS, ids=["%s-%s" % r for r in UNASSEMBLED_RUNS])
def test_unassembled_route_against_the_dense_solve(name, route, monkeypatch):
    kind, oracle_kind, env, want = K.UNASSEMBLED[route]
    h = _handle(monkeypatch, name, "f64", kind, env)
    try:
        if route == "persist" and h.cg_persist_stats()["enabled"] == 0:
            pytest.skip("the persistent single-launch CG does not accept this operator on this device")
        assert h.kkt_recurrence() == want and h.fold_stats()["enabled"] == 0
        out = _sequence(h, name, "f64")
        assert h.kkt_recurrence() == want                      # (a persistent kernel that fell back would say so)
    finally:
        h.close()
    assert K.verify(name, "f64", oracle_kind, out, route) == []
    _zero_rhs(monkeypatch, name, "f64", kind, env)
