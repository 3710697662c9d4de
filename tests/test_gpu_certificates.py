"""The infeasibility certificates (csrc/infeas.hip, batch_inf_check_body of csrc/batch.hip), one check at a time.

Handle.check_certificates / Batch.check_certificates load w_prev = 0, s = 0, w = [dx; 0] and the captured dy, and run the code the loop runs after an
iteration with those differences.  Every member of every case of tests/certificate_cases.py goes through both; the expected status is the one the
definition-level reference of that file and the oracle agree on (tests/test_certificate_cases_host.py).  The inputs of a tie are exact in any summation
order, so the device has to return the expected status on the threshold and one ulp to either side; every other member is at least 1000 rounding bounds
away from every threshold it meets.  Each test prints the smallest |quantity - threshold| / bound it relied on."""
import contextlib
import ctypes
import faulthandler
import math
import os

import numpy as np
import pytest

import cosmo_jl_amd as cj
from tests import certificate_cases as C
from tests import util

pytestmark = pytest.mark.gpu

CASE_LIMIT_S = 120
SWITCHES = ("COSMO_HIP_BATCH_LDS", "COSMO_HIP_BATCH_REG", "COSMO_HIP_BATCH_BS", "COSMO_HIP_BATCH_LDSCG")
FORMS = ("streaming", "lds_image", "register_1_2", "register_2_4")
STREAMING_CASES = ("gates", "scaling", "reductions_batch", "psd_small9_primal", "psd_mid3_dual", "cone3_exp_primal", "soc70_dual")
NAMES = {C.UNDETERMINED: "Undetermined", C.PRIMAL: "Primal_infeasible", C.DUAL: "Dual_infeasible"}
F = cj._ffi


@pytest.fixture(autouse=True)
def _case_time_limit():
    """a case that hangs takes the whole process down instead of holding the GPU: nothing runs after a hang"""
    faulthandler.dump_traceback_later(CASE_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@contextlib.contextmanager
def _switches(env):
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _cone_args(cs):
    sets = util.projection_sets(cs.cones)
    bl = np.concatenate([K.l for K in sets if K.kind == F.BOX] or [np.zeros(0)])
    bu = np.concatenate([K.u for K in sets if K.kind == F.BOX] or [np.zeros(0)])
    return [K.kind for K in sets], [K.dim for K in sets], bl, bu, [getattr(K, "alpha", 0.0) for K in sets]


def _params(dtype, **kw):
    p = F.default_params(dtype)
    p.kkt_kind = F.KKT_CG
    p.eps_prim_inf, p.eps_dual_inf = C.EPS_PRIM_INF, C.EPS_DUAL_INF
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def make_handle(cs):
    dtype = C.DTYPES[cs.dtype_id]
    h = cj.Handle(0, dtype=dtype)
    h.set_problem(cs.P, cs.q, cs.A, cs.b)
    kinds, dims, bl, bu, alpha = _cone_args(cs)
    h.set_cones(kinds, dims, bl, bu, cone_param=alpha)
    h.set_params(_params(dtype))
    h.set_scaling_full(cs.D, 1.0 / cs.D, cs.E, 1.0 / cs.E, cs.c, 1.0 / cs.c)
    return h


def make_batch(cs, nprob, env=None, accelerated=False, **params):
    dtype = C.DTYPES[cs.dtype_id]
    with _switches(env or {}):
        B = F.Batch(nprob, cs.n, cs.m, 0, dtype=dtype)
        if accelerated:
            B.set_accelerator()                                                             # before set_params: the accelerated kernels
        for k in range(nprob):
            B.set_problem(k, cs.P, cs.q, cs.A, cs.b)
            B.set_scaling_full(k, cs.D, 1.0 / cs.D, cs.E, 1.0 / cs.E, cs.c, 1.0 / cs.c)
        kinds, dims, bl, bu, alpha = _cone_args(cs)
        B.set_cones(kinds, dims, np.tile(bl, nprob) if bl.size else None, np.tile(bu, nprob) if bu.size else None, cone_param=alpha)
        B.set_params(_params(dtype, **params))
    return B


def _stack(cs, order):
    return np.concatenate([cs.members[k].dx for k in order]), np.concatenate([cs.members[k].dy for k in order])


def _relied_on(name, dtype_id, members):
    """the smallest |quantity - threshold| / bound over the inexact comparisons the reference went through (inf: everything was exact)"""
    worst = math.inf
    for k in members:
        worst = min([worst] + [ck.ratio for ck in C.verdict(name, dtype_id, k)[1]])
    return worst


def _wrong(cs, order, got):
    return [(k, cs.members[k].name, cs.members[k].kind, "decided by: " + cs.members[k].deciding, "expected " + NAMES[cs.members[k].expected], "got " + NAMES.get(g, str(g)))
            for k, g in zip(order, got) if g != cs.members[k].expected]


def _params_of(which):
    out = []
    for name in C.CASES:
        for dtype_id in ("f64", "f32") if C.float32_runs(name) else ("f64",):
            cs_flag = {"handle": name not in ("reductions_batch",), "batch": not name.startswith(("reductions_big", "soc16400", "psd_large", "psd_257"))}[which]
            if cs_flag:
                out.append((name, dtype_id))
    return out


HANDLE_PARAMS, BATCH_PARAMS = _params_of("handle"), _params_of("batch")


def test_the_parameters_are_the_flags_of_the_case_file():
    for name in C.CASES:
        cs = C.case(name)
        assert ((name, "f64") in HANDLE_PARAMS) == cs.handle and ((name, "f64") in BATCH_PARAMS) == cs.batch, name
        assert ((name, "f32") in HANDLE_PARAMS + BATCH_PARAMS) == C.float32_runs(name), name


@pytest.mark.parametrize("name,dtype_id", HANDLE_PARAMS, ids=["%s-%s" % p for p in HANDLE_PARAMS])
def test_handle_returns_the_expected_status_of_every_member(name, dtype_id):
    """one handle, one call per member, verdicts mixed: a call must not inherit the flags, the partial sums or the halt of the call before; then a second
    pass in reversed order (over the first and last four members where a call moves megabytes: reductions_big)"""
    cs = C.case(name, dtype_id)
    h = make_handle(cs)
    try:
        order = list(range(len(cs.members)))
        got = [h.check_certificates(cs.members[k].dx, cs.members[k].dy) for k in order]
        again = order if cs.m <= 40000 else order[:4] + order[-4:]
        back = [h.check_certificates(cs.members[k].dx, cs.members[k].dy) for k in again[::-1]][::-1]
    finally:
        h.close()
    print("%s %s: %d members, smallest |quantity - threshold| / bound relied on: %.3g" % (name, dtype_id, len(order), _relied_on(name, dtype_id, order)))
    assert not _wrong(cs, order, got), _wrong(cs, order, got)
    assert len(again) >= min(8, len(order)) and not _wrong(cs, again, back), "a second pass in reversed order changes verdicts: %r" % (_wrong(cs, again, back),)


@pytest.mark.parametrize("name,dtype_id", BATCH_PARAMS, ids=["%s-%s" % p for p in BATCH_PARAMS])
def test_batch_returns_the_expected_status_of_every_member(name, dtype_id):
    """the members form ONE batch with mixed verdicts; the same batch again in reversed order and in a random order (per-problem indexing, no state kept
    between calls); the streaming form once more for the cases of STREAMING_CASES"""
    cs = C.case(name, dtype_id)
    nm = len(cs.members)
    variants = [({}, None)] + ([({"COSMO_HIP_BATCH_LDS": "0"}, "streaming")] if name in STREAMING_CASES else [])
    forms = []
    for env, form in variants:
        B = make_batch(cs, nm, env)
        try:
            info = B.kernel_info()
            assert info["form"] in FORMS and (form is None or info["form"] == form), (name, info)
            forms.append(info["form"])
            orders = [list(range(nm)), list(range(nm))[::-1], np.random.default_rng(5).permutation(nm).tolist()]
            got = [B.check_certificates(*_stack(cs, order)) for order in orders]
        finally:
            B.close()
        for order, g in zip(orders, got):
            assert not _wrong(cs, order, g), (info["form"], _wrong(cs, order, g))
    print("%s %s: %d members in one batch (%s), smallest |quantity - threshold| / bound relied on: %.3g"
          % (name, dtype_id, nm, ", ".join(forms), _relied_on(name, dtype_id, range(nm))))


@pytest.mark.parametrize("dtype_id", ["f64", "f32"])
def test_an_accelerated_batch_checks_every_problem(dtype_id):
    """a batch with the Anderson accelerator runs the check kernel on flagged problems only inside optimize (BAa::need_inf); check_certificates launches
    it for all of them: every member of the gates and scaling cases gets its verdict, none is skipped as unflagged, and the batch still solves after"""
    for name in ("gates", "scaling"):
        cs = C.case(name, dtype_id)
        nm = len(cs.members)
        B = make_batch(cs, nm, accelerated=True, max_iter=60, check_termination=20, check_infeasibility=20)
        try:
            assert B.accel_stats()["accelerated"].shape == (nm,)
            orders = [list(range(nm)), list(range(nm))[::-1]]
            got = [B.check_certificates(*_stack(cs, order)) for order in orders]
            B.set_iterates(None, None, None)
            rs = B.optimize()
            after = B.check_certificates(*_stack(cs, orders[0]))
        finally:
            B.close()
        for order, g in zip(orders + [orders[0]], got + [after]):
            assert not _wrong(cs, order, g), (name, _wrong(cs, order, g))
        assert len(rs) == nm


@pytest.mark.parametrize("dtype_id", ["f64", "f32"])
def test_a_poisoned_member_stays_alone(dtype_id):
    """NaN and +-Inf in dx or dy of some members: the clean members between them return what they return in the batch without them"""
    cs = C.case("poison", dtype_id)
    assert cs.clean and any(mb.poisoned for mb in cs.members) and not cs.members[0].poisoned and not cs.members[-1].poisoned
    for env in ({}, {"COSMO_HIP_BATCH_LDS": "0"}):
        full = make_batch(cs, len(cs.members), env)
        part = make_batch(cs, len(cs.clean), env)
        try:
            g_full = full.check_certificates(*_stack(cs, range(len(cs.members))))
            g_part = part.check_certificates(*_stack(cs, cs.clean))
        finally:
            full.close(); part.close()
        assert [g_full[k] for k in cs.clean] == g_part == [cs.members[k].expected for k in cs.clean], (env, g_full, g_part)
        assert not _wrong(cs, range(len(cs.members)), g_full), _wrong(cs, range(len(cs.members)), g_full)


@pytest.mark.parametrize("name", ["gates", "soc70_primal"])
def test_a_batch_solves_after_a_check_as_a_fresh_batch_does(name):
    """check_certificates leaves every problem undecided and without iterates; set_iterates and a short optimize then return what a batch that never
    ran the check returns, bit for bit"""
    cs = C.case(name)
    nm = len(cs.members)
    prm = dict(max_iter=60, check_termination=20, check_infeasibility=20)
    used, fresh = make_batch(cs, nm, **prm), make_batch(cs, nm, **prm)
    try:
        got = used.check_certificates(*_stack(cs, range(nm)))
        assert not _wrong(cs, range(nm), got)
        with pytest.raises(F.CosmoHipError) as e:
            used.optimize()
        assert F.ERR_NAMES.get(e.value.code) == "INVALID"
        rng = np.random.default_rng(3)
        x0, s0, mu0 = rng.standard_normal(nm * cs.n), rng.standard_normal(nm * cs.m), rng.standard_normal(nm * cs.m)
        out = []
        for B in (used, fresh):
            B.set_iterates(x0, s0, mu0)
            rs = B.optimize()
            out.append([(r.status, r.iter, np.float64(r.cost).tobytes(), np.float64(r.r_prim).tobytes(), np.float64(r.r_dual).tobytes()) for r in rs]
                       + [B.get_iterates(k)[0].tobytes() for k in range(nm)])
        assert out[0] == out[1]
        assert used.check_certificates(*_stack(cs, range(nm))) == got                       # and the check again after a solve that decided statuses
    finally:
        used.close(); fresh.close()


def test_a_handle_solves_after_a_check_as_a_fresh_handle_does():
    cs = C.case("gates")
    used, fresh = make_handle(cs), make_handle(cs)
    try:
        got = [used.check_certificates(mb.dx, mb.dy) for mb in cs.members]
        assert not _wrong(cs, range(len(cs.members)), got)
        with pytest.raises(F.CosmoHipError) as e:
            used.optimize()
        assert F.ERR_NAMES.get(e.value.code) == "INVALID"
        out = []
        for h in (used, fresh):
            h.set_iterates(None, None, None)
            r = h.optimize()
            out.append((r.status, r.iter, np.float64(r.cost).tobytes(), h.get_iterates()[0].tobytes()))
        assert out[0] == out[1]
        assert [used.check_certificates(mb.dx, mb.dy) for mb in cs.members] == got         # the solve halted the stream: the check starts it again
    finally:
        used.close(); fresh.close()


def test_error_paths():
    cs = C.case("gates")
    mb = cs.members[0]
    st = ctypes.c_int32(0)
    dxp, dyp = F._dp(np.ascontiguousarray(mb.dx)), F._dp(np.ascontiguousarray(mb.dy))
    # handle: before set_cones / set_params
    h = cj.Handle(0)
    try:
        h.set_problem(cs.P, cs.q, cs.A, cs.b)
        for stage in ("problem", "cones"):
            with pytest.raises(F.CosmoHipError) as e:
                h.check_certificates(mb.dx, mb.dy)
            assert F.ERR_NAMES.get(e.value.code) == "INVALID", stage
            if stage == "problem":
                kinds, dims, bl, bu, alpha = _cone_args(cs)
                h.set_cones(kinds, dims, bl, bu, cone_param=alpha)
        h.set_params(_params(np.float64))
        assert h.check_certificates(mb.dx, mb.dy) in NAMES
        for args in ((None, dyp, ctypes.byref(st)), (dxp, None, ctypes.byref(st)), (dxp, dyp, None)):
            assert F.ERR_NAMES.get(h.lib.cosmo_hip_check_certificates(h._h, *args)) == "INVALID"
        with pytest.raises(ValueError):
            h.check_certificates(mb.dx[:-1], mb.dy)
        with pytest.raises(ValueError):
            h.check_certificates(None, mb.dy)
        h.comm_init(0, 1, cj.Handle.comm_unique_id())                                       # with a communicator: refused
        with pytest.raises(F.CosmoHipError) as e:
            h.check_certificates(mb.dx, mb.dy)
        assert F.ERR_NAMES.get(e.value.code) == "UNSUPPORTED"
    finally:
        h.close()
    # batch: before set_params
    B = F.Batch(2, cs.n, cs.m, 0)
    try:
        for k in range(2):
            B.set_problem(k, cs.P, cs.q, cs.A, cs.b)
            B.set_scaling_full(k, cs.D, 1.0 / cs.D, cs.E, 1.0 / cs.E, cs.c, 1.0 / cs.c)
        kinds, dims, bl, bu, alpha = _cone_args(cs)
        B.set_cones(kinds, dims, None, None, cone_param=alpha)
        with pytest.raises(F.CosmoHipError) as e:
            B.check_certificates(*_stack(cs, [0, 1]))
        assert F.ERR_NAMES.get(e.value.code) == "INVALID"
        B.set_params(_params(np.float64))
        assert B.check_certificates(*_stack(cs, [0, 1])) == [cs.members[0].expected, cs.members[1].expected]
        st2 = (ctypes.c_int32 * 2)()
        dx2, dy2 = _stack(cs, [0, 1])
        for args in ((None, F._dp(dy2), st2), (F._dp(dx2), None, st2), (F._dp(dx2), F._dp(dy2), None)):
            assert F.ERR_NAMES.get(B.lib.cosmo_hip_batch_check_certificates(B._b, *args)) == "INVALID"
        with pytest.raises(ValueError):
            B.check_certificates(dx2[:-1], dy2)
    finally:
        B.close()
    assert F.ERR_NAMES.get(cj.load_library().cosmo_hip_batch_check_certificates(None, None, None, None)) == "INVALID"
