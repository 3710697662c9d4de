"""GPU tests of cosmo_hip_update_matrices / cosmo_jl_amd.update(model, P=, A=): new values of P and A on a set-up handle.

PURITY: a handle U that was set up with the old values and then updated must hold the bits of a handle F that was set up with the new values.
The bar is bitwise equality, and it is derived, not measured: the refresh passes (csrc/update.hip) perform the floating-point operations of the
host build in the same order, and every later kernel is the same code on the same bits.  Anything weaker would hide a wrong map entry whose
effect is small."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from cosmo_jl_amd import _ffi
from cosmo_jl_amd.model import _scale_csc
from oracle import cosmo_oracle as O
from tests import update_matrix_cases as UC
from tests import util

pytestmark = pytest.mark.gpu

CG, SR, JACOBI, MR, MRR, DIRECT = _ffi.KKT_CG, _ffi.KKT_CG_SR, _ffi.KKT_CG_JACOBI, _ffi.KKT_MINRES, _ffi.KKT_MINRES_REDUCED, _ffi.KKT_DIRECT
SWITCHES = ("COSMO_HIP_OP_SPLIT", "COSMO_HIP_OP_FOLD", "COSMO_HIP_CG_FUSE_DIR", "COSMO_HIP_CG_PERSIST", "COSMO_HIP_FOLD_FACTOR", "COSMO_HIP_FOLD_FACTOR_MIN",
            "COSMO_HIP_CG_SR_DEFAULT", "COSMO_HIP_FOLD_PAD", "COSMO_HIP_FOLD_TILE")

_cases = {}


def case(name):
    if name not in _cases:
        split = UC.split_case()
        _cases.update(split=split, mixed=UC.mixed_case(), p0=UC.split_case(with_P=False))
        _cases["split_v"] = UC.zeros_and_flips(split)
        _cases["mixed_v"] = UC.zeros_and_flips(_cases["mixed"])
    return _cases[name]


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _bounds(sets):
    bl = np.concatenate([K.l for K in sets if K.kind == _ffi.BOX] or [np.zeros(0)])
    bu = np.concatenate([K.u for K in sets if K.kind == _ffi.BOX] or [np.zeros(0)])
    return bl, bu


def _scaling_of(c):
    rng = np.random.default_rng(17)
    m, n = c["A"].shape
    return rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, m), 0.75


def _params(h, kind):
    p = h.default_params()
    p.kkt_kind = kind
    p.tol_constant, p.tol_exponent = (1e-4, 0.0) if h.dtype == np.float32 else (1e-9, 0.0)      # a fixed tight Krylov threshold: many iterations per solve
    p.adaptive_rho_interval = 10                                                                # rho adapts inside the 30 iterations below
    return p


def handle(c, P, A, kind, dtype=np.float64, scaling=True, q=None, b=None, bounds=None):
    """set_problem, set_cones, set_params, set_scaling_full: no solve"""
    h = cj.Handle(0, dtype=dtype)
    h.set_problem(P, c["q"] if q is None else q, A, c["b"] if b is None else b)
    bl, bu = _bounds(c["sets"]) if bounds is None else bounds
    h.set_cones([K.kind for K in c["sets"]], [K.dim for K in c["sets"]], bl, bu)
    h.set_params(_params(h, kind))
    if scaling:
        D, E, cc = _scaling_of(c) if scaling is True else scaling
        h.set_scaling_full(D, 1.0 / D, E, 1.0 / E, cc, 1.0 / cc)
    return h


def same_bits(U, F, admm=True, seed=23):
    rng = np.random.default_rng(seed)
    n, m = U.n, U.m
    assert np.array_equal(U.get_rho_vec(), F.get_rho_vec())
    for which, k in ((_ffi.MAT_A, n), (_ffi.MAT_AT, m), (_ffi.MAT_P, n)):
        x = rng.standard_normal(k)
        assert np.array_equal(U.spmv(which, x), F.spmv(which, x)), which
    for _ in range(2):
        rhs = rng.standard_normal(n + m)
        xu, ku = U.kkt_solve(rhs); xf, kf = F.kkt_solve(rhs)
        assert ku == kf and np.array_equal(xu, xf), (ku, kf, float(np.max(np.abs(xu - xf))))
    if not admm:
        return
    x0, s0, mu0 = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    outs = []
    for h in (U, F):
        h.set_iterates(x0, s0, mu0); h.admm_init(); h.admm_iterate(30)
        outs.append(h.get_iterates())
    for a, b in zip(*outs):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b), float(np.max(np.abs(a - b)))


ROUTES = {
    # name: (kkt_kind, switches, what kkt_recurrence() must say, value arrays one update refreshes on the device)
    "cg_assembled": (CG, {}, "literal recurrence on the assembled operator", 5),
    "cg_split_only": (CG, {"COSMO_HIP_OP_FOLD": "0"}, "three launches", 3),
    "cg_unsplit": (CG, {"COSMO_HIP_OP_SPLIT": "0"}, "three launches", 0),
    "cg_default": (CG, {}, "cg: literal recurrence", 0),             # on a structure whose split is inactive
    "cg_unfused": (CG, {"COSMO_HIP_CG_FUSE_DIR": "0"}, "four launches", 3),
    "cg_jacobi": (JACOBI, {}, "Jacobi-preconditioned", 5),
    "cg_sr": (SR, {}, "one-launch single-reduction recurrence on the assembled operator", 5),
    "minres": (MR, {}, "minres on the full KKT system", 0),
    "minres_reduced": (MRR, {}, "minres on the reduced system", 0),
    "direct": (DIRECT, {}, "direct: supernodal", 0),
    "cg_partial": (CG, {"COSMO_HIP_FOLD_FACTOR": "1", "COSMO_HIP_FOLD_FACTOR_MIN": "3"}, "partially assembled", 6),
    "cg_persist": (CG, {"COSMO_HIP_CG_PERSIST": "1"}, "one persistent launch", 3),
}


def purity(monkeypatch, c, route, dtype=np.float64, update_P=True, update_A=True, unsplit=False):
    kind, env, says, refreshed = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)                                   # read at set_params
    P2 = c["P2"] if update_P else c["P"]
    A2 = c["A2"] if update_A else c["A"]
    U = handle(c, c["P"], c["A"], kind, dtype)
    F = handle(c, P2, A2, kind, dtype)
    assert says in U.kkt_recurrence() and says in F.kkt_recurrence(), U.kkt_recurrence()
    before = U.update_matrices_info()
    U.update_matrices(c["P2"].data if update_P and c["P"].nnz else None, c["A2"].data if update_A else None)
    info = U.update_matrices_info()
    assert info["updates"] == before["updates"] + 1 and info["host_rebuilds"] == 0 and info["analyses"] == before["analyses"]
    assert info["refreshed_arrays"] == (0 if unsplit else refreshed), info
    assert says in U.kkt_recurrence()
    same_bits(U, F)
    return U, F


# ---- structure (i): the split operator, every route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [r for r in ROUTES if r != "cg_default"])
def test_updated_handle_equals_fresh_handle_on_the_split_structure(monkeypatch, route):
    purity(monkeypatch, case("split"), route)


# ---- structure (ii): Zero / Nonnegatives / Box / SOC rows at density 0.1, the split is inactive -------------------------------------------------------
@pytest.mark.parametrize("route", ["cg_default", "minres", "minres_reduced", "direct"])
def test_updated_handle_equals_fresh_handle_without_the_split(monkeypatch, route):
    purity(monkeypatch, case("mixed"), route, unsplit=True)


def test_updated_handle_equals_fresh_handle_without_the_split_single_reduction(monkeypatch):
    c = case("mixed")
    U = handle(c, c["P"], c["A"], SR); F = handle(c, c["P2"], c["A2"], SR)
    assert "single-reduction recurrence, two launches" in U.kkt_recurrence()
    U.update_matrices(c["P2"].data, c["A2"].data)
    assert U.update_matrices_info()["host_rebuilds"] == 0
    same_bits(U, F)


# ---- (iii) P = 0, (iv) one matrix only, (v) exact zeros and sign flips ------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["cg_assembled", "direct"])
def test_update_with_an_empty_P(monkeypatch, route):
    purity(monkeypatch, case("p0"), route)


@pytest.mark.parametrize("route", ["cg_assembled", "direct"])
@pytest.mark.parametrize("which", ["P", "A"])
def test_update_of_one_matrix_only(monkeypatch, route, which):
    purity(monkeypatch, case("split"), route, update_P=which == "P", update_A=which == "A")


@pytest.mark.parametrize("name,route,unsplit", [("split_v", "cg_assembled", False), ("split_v", "direct", False), ("mixed_v", "cg_default", True)])
def test_update_with_exact_zeros_and_sign_flips(monkeypatch, name, route, unsplit):
    purity(monkeypatch, case(name), route, unsplit=unsplit)


@pytest.mark.parametrize("route", ["cg_assembled", "direct"])
def test_float32_library(monkeypatch, route):
    U, F = purity(monkeypatch, case("split"), route, dtype=np.float32)
    assert U.dtype == np.float32 and U.spmv(_ffi.MAT_P, np.ones(U.n)).dtype == np.float32


def test_update_before_set_params_changes_the_copies_only():
    c = case("split")
    hs = []
    for P, A in ((c["P"], c["A"]), (c["P2"], c["A2"])):
        h = cj.Handle(0)
        h.set_problem(P, c["q"], A, c["b"])
        hs.append(h)
    U, F = hs
    U.update_matrices(c["P2"].data, c["A2"].data)                 # before set_cones
    for h in hs:
        h.set_cones([K.kind for K in c["sets"]], [K.dim for K in c["sets"]])
        h.set_params(_params(h, CG))
    assert U.update_matrices_info()["refreshed_arrays"] == 0
    same_bits(U, F)


# ---- apply_scaling = 1: the handle's D, E, c applied on the device ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,route", [("split", "cg_assembled"), ("split", "direct"), ("mixed", "cg_default")])
def test_apply_scaling_matches_values_scaled_on_the_host(monkeypatch, name, route):
    c = case(name)
    kind, env, says, _ = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bl, bu = _bounds(c["sets"])
    U = cj.Handle(0)
    U.set_problem(c["P"], c["q"], c["A"], c["b"])
    U.set_cones([K.kind for K in c["sets"]], [K.dim for K in c["sets"]], bl, bu)
    D, E, cc = U.scale_ruiz(10)
    assert np.ptp(D) > 0 and np.ptp(E) > 0
    qs, bs = (D * c["q"]) * cc, E * c["b"]
    U.update_qb(qs, bs)                                            # the same bits of q and b on both handles (the Ruiz rounds scale them step by step)
    U.set_params(_params(U, kind))
    U.update_matrices(c["P2"].data, c["A2"].data, apply_scaling=True)
    Ps, As = c["P2"].copy(), c["A2"].copy()
    _scale_csc(Ps, D, D); Ps.data *= cc                            # (p * (D_i * D_j)) * c
    _scale_csc(As, E, D)                                           # a * (E_i * D_j)
    off, sl, su = 0, [], []
    for K in c["sets"]:
        if K.kind == _ffi.BOX:
            sl.append(K.l * E[off:off + K.dim]); su.append(K.u * E[off:off + K.dim])
        off += K.dim
    F = handle(c, Ps, As, kind, scaling=(D, E, cc), q=qs, b=bs, bounds=(np.concatenate(sl or [np.zeros(0)]), np.concatenate(su or [np.zeros(0)])))
    assert says in U.kkt_recurrence() and U.update_matrices_info()["host_rebuilds"] == 0
    same_bits(U, F)


def test_apply_scaling_without_a_scaling_takes_the_values_as_they_are():
    c = case("split")
    U = handle(c, c["P"], c["A"], CG, scaling=False); F = handle(c, c["P2"], c["A2"], CG, scaling=False)
    U.update_matrices(c["P2"].data, c["A2"].data, apply_scaling=True)
    same_bits(U, F, admm=False)


# ---- the capped grid: more than 4096 x 256 entries --------------------------------------------------------------------------------------------------
def test_second_grid_stride_trip():
    n = 300_000
    rng = np.random.default_rng(4)
    I = sp.identity(n, format="csc")
    A = sp.vstack([I, I, I, I]).tocsc(); A.sort_indices()
    assert A.nnz == 4 * n > 4096 * 256 and A.shape[0] == A.nnz     # all singleton rows: a second trip in the copy refresh and in the a * a refresh
    c = dict(P=sp.identity(n, format="csc"), q=np.zeros(n), b=np.zeros(4 * n), sets=[cj.Nonnegatives(4 * n)])
    c["A"] = UC.same_pattern(A, rng.uniform(0.5, 1.5, A.nnz)); c["A2"] = UC.same_pattern(A, rng.uniform(0.5, 1.5, A.nnz) * rng.choice([-1.0, 1.0], A.nnz))
    c["P2"] = UC.same_pattern(c["P"], rng.uniform(0.5, 1.5, n))
    U = handle(c, c["P"], c["A"], CG, scaling=False); F = handle(c, c["P2"], c["A2"], CG, scaling=False)
    U.update_matrices(c["P2"].data, c["A2"].data)
    assert U.update_matrices_info()["host_rebuilds"] == 0
    for which, k in ((_ffi.MAT_A, n), (_ffi.MAT_AT, 4 * n), (_ffi.MAT_P, n)):
        x = rng.standard_normal(k)
        assert np.array_equal(U.spmv(which, x), F.spmv(which, x))
    rhs = rng.standard_normal(5 * n)
    xu, ku = U.kkt_solve(rhs); xf, kf = F.kkt_solve(rhs)
    assert ku == kf and np.array_equal(xu, xf)


# ---- DIRECT specifics ---------------------------------------------------------------------------------------------------------------------------------
def test_direct_update_refactors_on_the_kept_analysis_and_checks_the_inertia():
    c = case("split")
    U = handle(c, c["P"], c["A"], DIRECT); F = handle(c, c["P2"], c["A2"], DIRECT)
    d0, i0 = U.direct_info(), U.update_matrices_info()
    U.update_matrices(c["P2"].data, c["A2"].data)
    d1, i1 = U.direct_info(), U.update_matrices_info()
    assert d1["factorizations"] == d0["factorizations"] + 1 and d1["nnz_L"] == d0["nnz_L"] and d1["supernodes"] == d0["supernodes"]
    assert i1["analyses"] == i0["analyses"] == 1
    with pytest.raises(_ffi.CosmoHipError, match="Objective function is not convex.") as e:
        U.update_matrices(-c["P2"].data, None)                     # an indefinite P
    assert e.value.code == 1                                       # COSMO_HIP_ERR_INVALID, as a failed update_rho
    with pytest.raises(_ffi.CosmoHipError):
        U.kkt_solve(np.ones(U.n + U.m))
    U.update_matrices(c["P2"].data, None)                          # a valid update restores the handle
    assert U.update_matrices_info()["analyses"] == 1
    same_bits(U, F, admm=False)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = case("split")
    h = cj.Handle(0)
    h.nnz_P, h.nnz_A = c["P"].nnz, c["A"].nnz
    with pytest.raises(_ffi.CosmoHipError) as e:
        h.update_matrices(c["P"].data, c["A"].data)                # before set_problem
    assert e.value.code == 1
    h = handle(c, c["P"], c["A"], CG)
    before = h.update_matrices_info()
    h.update_matrices(None, None)                                  # both NULL: nothing happens
    assert h.update_matrices_info() == before and before["updates"] == 0
    with pytest.raises(ValueError):
        h.update_matrices(c["P"].data[:-1], None)
    h.comm_init_hostshm(0, 1, "/cosmo_updmat_%d" % os.getpid())
    h.set_row_shard([0, len(c["sets"])])
    with pytest.raises(_ffi.CosmoHipError, match="row-sharded") as e:
        h.update_matrices(c["P2"].data, c["A2"].data)
    assert e.value.code == 6                                       # COSMO_HIP_ERR_UNSUPPORTED


# ---- re-solve through the model API -----------------------------------------------------------------------------------------------------------------
def _resolve_problem():
    rng = np.random.default_rng(31)
    pr = util.random_qp(rng, 50, 6, 60, 0, soc_dims=(5, 9), density=0.15, p_shift=1.0)
    L = sp.tril(pr["P"], k=-1)
    P = (L + L.T + sp.diags(pr["P"].diagonal())).tocsc(); P.sort_indices()
    A = pr["A"]; A.sort_indices()
    x0 = rng.standard_normal(50)
    s0 = [np.zeros(6), rng.uniform(0.1, 1.0, 60)]
    for d in (5, 9):
        v = rng.standard_normal(d - 1)
        s0.append(np.concatenate([[np.linalg.norm(v) + 0.5], v]))
    s0 = np.concatenate(s0)
    # values perturbed by 10-30 %, P2 = G P G still PSD
    A2 = UC.same_pattern(A, A.data * (1.0 + rng.choice([-1.0, 1.0], A.nnz) * rng.uniform(0.1, 0.3, A.nnz)))
    P2 = UC.perturbed_psd(P, rng, 0.75, 1.25)
    return dict(P=P, q=pr["q"], A=A, b=A @ x0 + s0, sets=pr["sets"], P2=P2, A2=A2, b2=A2 @ x0 + s0)     # b2: the same point stays feasible


@pytest.mark.parametrize("mode", ["unscaled", "host_scaling", "device_scaling"])
def test_resolve_through_the_model_api(mode):
    pr = _resolve_problem()
    st = dict(eps_abs=1e-7, eps_rel=1e-7, max_iter=20000, scaling=0 if mode == "unscaled" else 10, device_scaling=mode == "device_scaling")
    md = cj.Model()
    md.set(pr["P"], pr["q"], pr["A"], pr["b"], pr["sets"], cj.Settings(kkt_solver=cj.CGIndirectKKTSolver, **st))
    r1 = cj.optimize(md)
    assert r1.status == "Solved"
    assert bool(getattr(md, "device_scaled", False)) == (mode == "device_scaling")
    h = md.handle
    cj.update(md, P=pr["P2"], A=pr["A2"], b=pr["b2"])
    r2 = cj.optimize(md)
    assert md.handle is h and h.update_matrices_info()["host_rebuilds"] == 0 and h.update_matrices_info()["updates"] == 1
    ref = O.solve(pr["P2"], pr["q"], pr["A2"], pr["b2"], util.oracle_cones(pr["sets"]), O.Settings(kkt_solver="cg", eps_abs=1e-7, eps_rel=1e-7, max_iter=20000,
                                                                                                    scaling=st["scaling"]))
    tol = 1e-4                                                     # the bars of test_gpu_batch_resident._agree without its iteration-count bar (the warm start changes it)
    print("status %s / %s, objective %.9g / %.9g, iterations %d / %d" % (r2.status, ref.status, r2.obj_val, ref.obj_val, r2.iter, ref.iter))
    assert r2.status == ref.status == "Solved"
    assert abs(r2.obj_val - ref.obj_val) <= tol * (1 + abs(ref.obj_val)), (r2.obj_val, ref.obj_val)
    for a, b in ((r2.x, ref.x), (r2.y, ref.y)):
        assert np.max(np.abs(a - b)) <= 100 * tol * max(np.max(np.abs(b)), 1.0)
    x0 = np.ones(md.n)
    cj.warm_start_primal(md, x0)                                   # reads model.A: the new values (scaled as the model keeps them)
    assert np.all(np.isfinite(md.s))


def test_scaling_A_of_a_two_variable_lp():
    md = cj.Model()
    cj.assemble(md, np.zeros((2, 2)), np.array([1.0, 1]), cj.Constraint(np.eye(2), [-2.0, -3.0], cj.Nonnegatives), settings=cj.Settings(check_termination=20))
    r = cj.optimize(md)
    assert np.linalg.norm(r.x - [2.0, 3.0]) < 1e-3                 # x >= (2, 3)
    h = md.handle
    A = md.A.toarray()                                             # the internal A (A x + s = b); a host-scaled model keeps E A D
    if md.is_scaled and not getattr(md, "device_scaled", False):
        A = md.sm.Einv[:, None] * A * md.sm.Dinv[None, :]
    cj.update(md, A=2.0 * A)
    r2 = cj.optimize(md)
    assert md.handle is h and h.update_matrices_info()["updates"] == 1
    assert np.linalg.norm(r2.x - [1.0, 1.5]) < 1e-3                # 2 x >= (2, 3)
