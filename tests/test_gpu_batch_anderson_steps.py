"""The accelerator inside the persistent batch kernels (aa_pre / aa_declined / aa_reset of csrc/batch.hip, inlined into four kernel forms and two copies
of the accelerated loop), one candidate at a time and with no entry point of its own.

Batch.iterate(1) runs aa_pre -> admm_z (w_prev = w) -> KKT solve and update of w -> safeguard (batch_admm_body), so after every call get_iterates(k) returns
in w_prev the candidate the accelerator produced (or g again, after a declined candidate or a step without acceleration) and in (w, w_prev) the pair the
next aa_pre is given.  The fetched pairs go to tests/anderson_cases.ReferenceAccelerator (explicit history, np.longdouble least squares); the accuracy of
the KKT solve does not enter.  Three DIFFERENT problems per batch, so a history slab or a state record taken from the neighbour shows; 45 iterations, two
memory restarts; every step of every problem is compared, none is left out (tests/test_anderson_cases_host.py: cond stays below 1e5 on these inputs in
the oracle's loop; the bound scales with the cond of the step at hand in any case).

The bound on a candidate is C eps cond (||g|| + ||dG|| ||eta||) with the constant of tests/anderson_cases.py in both dtypes.  At cond 1e3 - 1e4 that is a
COARSE check in Float32 (C eps32 cond = 2e-3 .. 2e-2: it catches a wrong column, slot or problem, not a wrong last digit) and a sharp one in Float64
(4e-12 .. 4e-11)."""
import contextlib
import faulthandler
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from tests import anderson_cases as A
from tests import util

pytestmark = pytest.mark.gpu
F = cj._ffi
CASE_LIMIT_S = 120
ITERS = 45
SWITCHES = ("COSMO_HIP_BATCH_LDS", "COSMO_HIP_BATCH_REG", "COSMO_HIP_BATCH_BS", "COSMO_HIP_BATCH_LDSCG")
VARIANTS = {                                     # name -> (environment, the form kernel_info must report)
    "streaming": ({"COSMO_HIP_BATCH_LDS": "0"}, "streaming"),
    "lds_image": ({"COSMO_HIP_BATCH_REG": "0"}, "lds_image"),
    "register_1_2": ({}, "register_1_2"),
    "register_2_4": ({}, "register_2_4"),
}
# (problems, mem, variant)
RUNS = [("small", 15, "streaming"), ("small", 15, "lds_image"), ("small", 15, "register_1_2"),
        ("small", 16, "streaming"), ("small", 16, "lds_image"), ("small", 16, "register_1_2"),
        ("large", 15, "streaming"), ("wide", 15, "register_2_4"), ("wide", 15, "streaming"),
        ("simple", 15, "register_1_2"), ("simple", 15, "streaming")]


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


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    v = np.int64 if a.dtype == np.float64 else np.int32
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all(a.view(v) == b.view(v)))


def models_of(name, mem, dtype):
    st = cj.Settings(accelerator=cj.with_options(cj.AndersonAccelerator, mem=mem), kkt_solver=cj.CGIndirectKKTSolver, eps_abs=0.0, eps_rel=0.0, adaptive_rho=False,
                     check_infeasibility=10 ** 9, max_iter=10 ** 6)
    out = []
    for seed in (0, 1, 2):
        md = cj.Model(dtype=dtype)
        if name == "simple":                                     # the reference's 2-variable QP (simple.jl), N = 8: mem is clipped; three different q
            Ps = sp.csc_matrix(np.array([[4.0, 1], [1, 2]])); q = np.array([1.0, 1]) + 0.25 * seed
            Am = np.array([[1.0, 1], [1, 0], [0, 1]]); l = np.array([1.0, 0, 0]); u = np.array([1.0, 0.7, 0.7])
            cj.assemble(md, Ps, q, [cj.Constraint(-Am, u, cj.Nonnegatives), cj.Constraint(Am, -l, cj.Nonnegatives)], settings=st)
        else:
            rng = np.random.default_rng(seed)
            # large: at the default density its image (62 000 entries of A) does not fit the LDS, so it runs the streaming kernel whatever the switches say;
            # wide: n > 512 with few enough entries for an image, the <2, 4> register kernel
            p = {"small": lambda: util.random_qp(rng, 30, 3, 20, 15, soc_dims=(5, 3), p_shift=2.0),
                 "large": lambda: util.random_qp(rng, 600, 50, 500, 400, soc_dims=(50, 30), p_shift=2.0),
                 "wide": lambda: util.random_qp(rng, 520, 10, 100, 50, soc_dims=(5, 3), density=0.01, p_shift=2.0)}[name]()
            md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st)
        out.append(md)
    return out


@pytest.mark.parametrize("name,mem,variant", RUNS)
@pytest.mark.parametrize("dtype_id", ["f64", "f32"])
def test_every_batch_step_against_the_reference(dtype_id, name, mem, variant):
    dtype = A.DTYPES[dtype_id]
    eps = A.eps_of(dtype)
    models = models_of(name, mem, dtype)
    env, form = VARIANTS[variant]
    with _switches(env):
        B, _ = cj.model.prepare_batch(models, 0)
    try:
        info = B.kernel_info()
        assert info["form"] == form, (name, variant, info)
        N = B.n + B.m
        nprob = len(models)
        refs = [A.ReferenceAccelerator("qr", N, mem, A.MIN_MEM, dtype=dtype) for _ in range(nprob)]
        assert refs[0].mem == min(mem, N)
        B.iterate(1, with_init=True)                                                  # loop index 1: before start_iter = 2, no accelerator
        keys = ("accelerated", "accepted", "declined", "restarts", "safeguarding_iter")
        stats = B.accel_stats()
        assert not any(stats[k].any() for k in keys)
        pairs = [tuple(v.copy() for v in B.get_iterates(k)[:2]) for k in range(nprob)]
        worst, compared, candidates, declined_total, plain = 0.0, [0] * nprob, [0] * nprob, 0, 0
        for it in range(2, ITERS + 1):
            B.iterate(1)
            new = B.accel_stats()
            for k in range(nprob):
                at = (name, mem, variant, dtype_id, "problem", k, "iteration", it)
                g, x = pairs[k]
                S = refs[k].step(g, x, it=it)
                w, w_prev = (v.copy() for v in B.get_iterates(k)[:2])
                d = {key: int(new[key][k] - stats[key][k]) for key in keys}
                assert new["restarts"][k] == S.restarts, (at, new["restarts"][k], S.restarts)
                assert new["active"][k] == 1
                candidates[k] += d["accelerated"]
                assert d["accelerated"] in (0, 1) and d["declined"] + d["accepted"] == d["accelerated"] and d["safeguarding_iter"] == d["declined"], (at, d)
                if d["accelerated"] and not d["declined"]:
                    assert S.success or not S.decided, (at, S.l, S.singular, S.eta_norm, S.cond)
                    if S.success:
                        e = refs[k].error(w_prev, S) / (A.C_BOUND * eps)
                        worst = max(worst, e); compared[k] += 1
                        assert e <= 1.0, (at, e, S.cond, S.l, S.j)
                elif d["declined"]:
                    assert same_bits(w_prev, g), at                                   # reset to the last pair's g, one plain step from there
                    assert S.success or not S.decided, (at, S.l, S.singular, S.eta_norm, S.cond)
                    declined_total += 1
                else:
                    assert same_bits(w_prev, g), at                                   # no candidate: admm_z copied g
                    # (an undecided step -- C_ETA eps cond >= 1/2, the iteration has converged to rounding noise -- says nothing about the device's flag)
                    agrees = S.l < A.MIN_MEM or it < 2 or S.singular or not (S.eta_norm < A.ETA_MAX / 2) or not S.decided
                    assert agrees, (at, S.l, S.eta_norm, S.cond)
                    plain += 1
                pairs[k] = (w, w_prev)
            stats = new
        print("BATCH_ANDERSON_STEP problems=%s mem=%d variant=%s form=%s dtype=%s worst_e_over_Ceps=%.3g compared=%s candidates=%s declined=%d not_accelerated=%d restarts=%s"
              % (name, mem, variant, info["form"], dtype_id, worst, compared, candidates, declined_total, plain, stats["restarts"].tolist()))
        # candidates: as many as the oracle's loop produces on these inputs (tests/test_anderson_cases_host.py); a declined one is seen only through its reset.
        # The simple QP has converged to rounding noise after some twenty iterations
        assert min(candidates) >= (25 if name != "simple" else 8) and min(compared) >= (10 if name != "simple" else 5), (candidates, compared)
        if name != "simple":
            assert int(stats["restarts"].min()) == 2
    finally:
        B.close()
