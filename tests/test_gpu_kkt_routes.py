"""The KKT solve routes of a single-problem handle (csrc/kkt.hip): every route is reached through kkt_kind and the route
switches and named by cosmo_hip_kkt_recurrence, and a set_params that changes the route of a handle leaves it exactly where a fresh handle
configured with the new route starts -- nothing of the previous route survives."""
import numpy as np
import pytest

import cosmo_jl_amd as cj

pytestmark = pytest.mark.gpu
F = cj._ffi

SWITCHES = ("COSMO_HIP_OP_SPLIT", "COSMO_HIP_OP_FOLD", "COSMO_HIP_CG_FUSE_DIR", "COSMO_HIP_CG_PERSIST", "COSMO_HIP_FOLD_FACTOR", "COSMO_HIP_CG_SR_DEFAULT")

# route -> (kkt_kind, route switches, recurrence string on the problem below)
ROUTES = {
    "direct": (F.KKT_DIRECT, {}, "direct: supernodal LDL' of the full KKT system, one launch per tree level (csrc/ldl.hip)"),
    "minres": (F.KKT_MINRES, {}, "minres on the full KKT system (csrc/minres.hip)"),
    "minres_reduced": (F.KKT_MINRES_REDUCED, {}, "minres on the reduced system (csrc/minres.hip)"),
    "persist": (F.KKT_CG, {"COSMO_HIP_CG_PERSIST": "1"}, "cg: literal recurrence in one persistent launch (csrc/cg_persist.hip, opt-in)"),
    "jacobi": (F.KKT_CG_JACOBI, {}, "cg: Jacobi-preconditioned recurrence on the assembled operator (opt-in), k_cg_dirM<3, true> + k_cg_upd<true>"),
    "sr_assembled": (F.KKT_CG_SR, {}, "cg: one-launch single-reduction recurrence on the assembled operator (opt-in kkt_kind CG_SR), k_sr_M<3>"),
    "sr_lab_switch": (F.KKT_CG, {"COSMO_HIP_CG_SR_DEFAULT": "1"},
                      "cg: one-launch single-reduction recurrence on the assembled operator (lab switch COSMO_HIP_CG_SR_DEFAULT=1), k_sr_M<3>"),
    "sr": (F.KKT_CG_SR, {"COSMO_HIP_OP_FOLD": "0"}, "cg: single-reduction recurrence, two launches per iteration (kkt_kind CG_SR), k_sr_update_A + k_sr_op"),
    "partially_assembled": (F.KKT_CG, {"COSMO_HIP_FOLD_FACTOR": "1"},
                            "cg: literal recurrence on the partially assembled operator (118 rows of A kept factored), two launches per iteration, "
                            "k_cg_dirM<3, false> + k_cg_updF"),
    "assembled": (F.KKT_CG, {}, "cg: literal recurrence on the assembled operator, two launches per iteration, k_cg_dirM<3, false> + k_cg_upd<false>"),
    "fused": (F.KKT_CG, {"COSMO_HIP_OP_FOLD": "0"}, "cg: literal recurrence, three launches per iteration, k_cg_dirA + k_op_apply + k_cg_upd<false>"),
    "plain": (F.KKT_CG, {"COSMO_HIP_CG_FUSE_DIR": "0"},
              "cg: literal recurrence, four launches per iteration, k_cg_dir + k_spmv_A_rho + k_op_apply + k_cg_upd<false>"),
}

# (A, B): every route as A and as B, among them DIRECT -> CG, persistent -> Jacobi, CG_SR -> CG and MINRES -> DIRECT
TRANSITIONS = [("minres", "direct"), ("direct", "assembled"), ("assembled", "persist"), ("persist", "jacobi"), ("jacobi", "sr_assembled"),
               ("sr_assembled", "partially_assembled"), ("partially_assembled", "sr"), ("sr", "fused"), ("fused", "plain"),
               ("plain", "minres_reduced"), ("minres_reduced", "sr_lab_switch"), ("sr_lab_switch", "minres")]


@pytest.fixture(scope="module")
def prob():
    # a chordal SDP whose reduced operator has a split form that can be assembled: every route exists on it
    return cj.problems.chordal_sdp(ncliques=12, dmin=4, dmax=70, sep_min=1, sep_max=3, n_total=2500, n_zero=40, n_nonneg=80)


def _handle(prob):
    h = F.Handle(0)
    h.set_problem(prob["P"], prob["q"], prob["A"], prob["b"])
    sets = prob["sets"]
    bl = np.concatenate([K.l for K in sets if K.kind == F.BOX] or [np.zeros(0)])
    bu = np.concatenate([K.u for K in sets if K.kind == F.BOX] or [np.zeros(0)])
    h.set_cones([K.kind for K in sets], [K.dim for K in sets], bl, bu, cone_param=[getattr(K, "alpha", 0.0) for K in sets])
    return h


def _configure(h, route, monkeypatch):
    kind, env, _ = ROUTES[route]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = h.default_params()
    p.kkt_kind = kind
    p.eps_abs = p.eps_rel = 0.0                       # fixed work: no termination check ends the run early
    p.check_infeasibility = 10 ** 9
    h.set_params(p)


def _run(h):
    h.set_iterates()
    h.admm_init()
    h.admm_iterate(30)
    return h.get_iterates()


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route_is_reached_and_named(route, prob, monkeypatch):
    h = _handle(prob)
    try:
        _configure(h, route, monkeypatch)
        assert h.kkt_recurrence() == ROUTES[route][2]
        assert h.cg_persist_stats()["enabled"] == (1 if route == "persist" else 0)
        _run(h)
        assert h.kkt_recurrence() == ROUTES[route][2]
    finally:
        h.close()


@pytest.mark.parametrize("a,b", TRANSITIONS, ids=["%s->%s" % t for t in TRANSITIONS])
def test_route_change_matches_a_fresh_handle(a, b, prob, monkeypatch):
    h = _handle(prob)
    fresh = _handle(prob)
    try:
        _configure(h, a, monkeypatch)
        _run(h)
        _configure(h, b, monkeypatch)
        _configure(fresh, b, monkeypatch)
        assert h.kkt_recurrence() == fresh.kkt_recurrence() == ROUTES[b][2]
        assert h.cg_persist_stats()["enabled"] == fresh.cg_persist_stats()["enabled"]
        assert h.fold_stats()["enabled"] == fresh.fold_stats()["enabled"]
        w1, _, s1, mu1 = _run(h)
        w2, _, s2, mu2 = _run(fresh)
        assert np.array_equal(w1, w2) and np.array_equal(s1, s2) and np.array_equal(mu1, mu2)
    finally:
        h.close()
        fresh.close()
