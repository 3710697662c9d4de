"""CPU: the sequences and the reference of tests/anderson_cases.py, proven before any GPU run.  The oracle's AndersonAccelerator /
AndersonAcceleratorNE (Float64 numpy) is run against ReferenceAccelerator (explicit history, np.longdouble solves) on every kind, sequence and shape
tests/test_gpu_anderson_steps.py sends to the device: same bookkeeping, same flags, candidates within the bound whose constant is measured here; and the
inputs satisfy the conditions the GPU tests lean on (well-conditioned `random`, restarts and wrap-arounds, enough successful candidates, the flags of
the degenerate sequences).  The batch trajectories of tests/test_gpu_batch_anderson_steps.py are replayed on the oracle's Workspace."""
import functools

import numpy as np
import pytest

import cosmo_jl_amd as cj
from oracle import cosmo_oracle as O
from tests import anderson_cases as A
from tests import util

EPS64 = np.finfo(np.float64).eps
CASES = [(n, m, mem, mm) for (n, m, mem) in A.SHAPES for mm in ((A.MIN_MEM, 1) if n + m == 40 else (A.MIN_MEM,))]


@functools.lru_cache(maxsize=None)
def run(kind, seq, n, m, mem, min_mem):
    return A.run_oracle(O, kind, seq, n, m, mem, min_mem)


def flags(recs):
    return "".join("s" if S.singular else "e" if S.eta_too_large else "+" if S.success else "." for _, S in recs)


def oracle_flags(recs):
    return "".join("s" if r["singular"] else "e" if r["eta_too_large"] else "+" if r["success"] else "." for r, _ in recs)


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize("n,m,mem,min_mem", CASES)
@pytest.mark.parametrize("kind", list(A.KINDS))
def test_oracle_against_reference_normal_sequences(kind, n, m, mem, min_mem):
    for seq in ("random", "contractive", "scaled_up", "scaled_down"):
        recs = run(kind, seq, n, m, mem, min_mem)
        worst = 0.0
        for k, (r, S) in enumerate(recs):
            assert (r["l"], r["j"], r["restarts"]) == (S.l, S.j, S.restarts), (seq, k)
            if S.decided:
                assert (r["success"], r["singular"], r["eta_too_large"]) == (S.success, S.singular, S.eta_too_large), (seq, k, S.cond, S.eta_norm)
            if not r["success"]:
                assert np.array_equal(r["cand"], r["g"]), (seq, k)
            elif S.success:
                e = A.ReferenceAccelerator.error(None, r["cand"], S)
                worst = max(worst, e / EPS64)
                assert e <= A.C_BOUND * EPS64, (seq, k, e / EPS64, S.cond)
        print("%s %s N=%d mem=%d min_mem=%d: worst e/eps %.3g  %s" % (kind, seq, n + m, mem, min_mem, worst, flags(recs)))


@pytest.mark.parametrize("n,m,mem,min_mem", CASES)
@pytest.mark.parametrize("kind", list(A.KINDS))
def test_oracle_against_reference_degenerate_sequences(kind, n, m, mem, min_mem):
    rolling = A.KINDS[kind][2]
    mem_eff = min(mem, n + m)
    for seq in A.DEGENERATE:
        recs = run(kind, seq, n, m, mem, min_mem)
        for k, (r, S) in enumerate(recs):
            assert (r["l"], r["j"], r["restarts"]) == (S.l, S.j, S.restarts), (seq, k)
            if S.decided:
                assert (r["success"], r["singular"], r["eta_too_large"]) == (S.success, S.singular, S.eta_too_large), (seq, k, S.cond, S.eta_norm)
            if r["success"] and S.success:
                assert A.ReferenceAccelerator.error(None, r["cand"], S) <= A.C_BOUND * EPS64, (seq, k)
        fl = flags(recs)
        # the bad column is number DEGENERATE_AT - 1; a restarted memory drops it with the update that finds the memory full (pair mem + 1), a rolling one
        # overwrites it mem updates later
        gone = mem_eff + 1 if not rolling else A.DEGENERATE_AT + mem_eff
        if rolling and seq == "near_dependent":
            gone -= 1                   # the dependence ends as soon as the column it copies (number DEGENERATE_AT - 2) is overwritten
        bad = fl[A.DEGENERATE_AT:gone]
        if seq == "repeat":
            assert set(bad) == {"s"}, (kind, fl)
        else:                           # the first candidate with the dependent column may still pass (f itself lies almost in the span), every later one fails
            assert set(bad[1:]) == {"e"} and bad[0] in "e+", (kind, fl)
        assert set(fl[:A.DEGENERATE_AT]) <= {".", "+"} and "+" in fl[:A.DEGENERATE_AT]
        after = fl[gone:]
        assert set(after) <= {".", "+"} and after.count("+") >= min(mem_eff, len(after)) - min_mem, (kind, fl)
        if not rolling:                 # recovery: nothing until min_mem columns are back, success from l = min_mem on
            ls = [S.l for _, S in recs[gone:]]
            assert all((c == "+") == (l >= min_mem) for c, l in zip(after, ls)), (kind, fl, ls)


@pytest.mark.parametrize("n,m,mem,min_mem", CASES)
@pytest.mark.parametrize("kind", list(A.KINDS))
def test_oracle_against_reference_eta_threshold(kind, n, m, mem, min_mem):
    """`large_eta`: ||eta|| > eta_max by the size of f, at a cond(M) at which the decision is the reference's to take in every kind and in both dtypes.  The
    oracle takes the same decision at every decided step; at least mem - MIN_MEM of them fail on eta; at N >= 1025 both outcomes occur in one run."""
    mem_eff = min(mem, n + m)
    recs = run(kind, "large_eta", n, m, mem, min_mem)
    failed = 0
    for k, (r, S) in enumerate(recs):
        assert (r["l"], r["j"], r["restarts"]) == (S.l, S.j, S.restarts), k
        assert not S.singular and not r["singular"]
        if S.decided:
            assert (r["success"], r["eta_too_large"]) == (S.success, S.eta_too_large), (k, S.cond, S.eta_norm)
            failed += S.eta_too_large
        if not r["success"]:
            assert np.array_equal(r["cand"], r["g"]), k
        elif S.success:
            assert A.ReferenceAccelerator.error(None, r["cand"], S) <= A.C_BOUND * EPS64, k
    assert failed >= mem_eff - A.MIN_MEM, (flags(recs), oracle_flags(recs))
    for dtype_id, dtype in A.DTYPES.items():               # the reference alone, in the dtype the device is given: as many decided failures
        seq = A.Sequence("large_eta", n + m, 0, dtype)
        ref = A.ReferenceAccelerator(kind, n + m, mem, min_mem, eta_max=A.eta_max_of("large_eta"), dtype=dtype)
        steps = [ref.step(*seq.next()) for _ in range(A.steps_of(mem, n + m))]
        assert sum(S.decided and S.eta_too_large for S in steps) >= mem_eff - A.MIN_MEM, (dtype_id, "".join("e" if S.eta_too_large else "+" if S.success else "." for S in steps))
        assert all(S.cond_M < 1e6 for S in steps if S.attempted)
        if n + m >= 1025 and kind != "type1_rolling":
            assert any(S.decided and S.success for S in steps), dtype_id


@pytest.mark.parametrize("dtype_id", list(A.DTYPES))
@pytest.mark.parametrize("kind", list(A.KINDS))
def test_first_contractive_candidate_is_comparable(kind, dtype_id):
    """the first candidate of `contractive` is taken on pairs that no earlier candidate has entered, so an implementation and the reference are given the same
    numbers: it is decided and inside C eps cond < 1/2 in every kind, shape and dtype.  (Later pairs continue from the implementation's own candidate.)"""
    dtype = A.DTYPES[dtype_id]
    for (n, m, mem, min_mem) in CASES:
        seq = A.Sequence("contractive", n + m, 0, dtype)
        ref = A.ReferenceAccelerator(kind, n + m, mem, min_mem, dtype=dtype)
        cand = None
        for _ in range(A.steps_of(mem, n + m)):
            g, x = seq.next(cand)
            S = ref.step(g, x)
            cand = np.asarray(S.cand, dtype=dtype)
            if S.attempted:
                assert S.success and S.decided and A.C_BOUND * A.eps_of(dtype) * S.cond < 0.5, (n + m, min_mem, S.cond)
                break


def test_repeat_with_mem_6_fails_singular_until_the_memory_restarts():
    """mem = 6, fail_singular at every step from the repeated pair until the memory restarts, success again from l = 3"""
    N, mem = 40, 6
    seq = A.Sequence("repeat", N, 0, np.float64)
    ref = A.ReferenceAccelerator("qr", N, mem)
    aa = O.AndersonAccelerator(N, mem, A.MIN_MEM)
    got, want, ls = "", "", []
    for k in range(2 * mem + 5):
        g, x = seq.next()
        S = ref.step(g, x)
        with np.errstate(all="ignore"):
            fs = aa.fail_singular
            aa.update(g, x); c = g.copy(); aa.accelerate(c)
        got += "s" if aa.fail_singular > fs else "+" if aa.was_successful() else "."
        want += "s" if S.singular else "+" if S.success else "."
        ls.append(S.l)
    assert got == want == "...++ss..++++..++", (got, want)
    assert ls[7:10] == [1, 2, 3]


@pytest.mark.parametrize("kind", list(A.KINDS))
def test_conditions_on_the_inputs(kind):
    ne, rolling = A.KINDS[kind][3], A.KINDS[kind][2]
    for (n, m, mem, min_mem) in CASES:
        mem_eff = min(mem, n + m)
        for seq in A.SEQUENCES:
            recs = run(kind, seq, n, m, mem, min_mem)
            steps = [S for _, S in recs]
            if seq == "random":
                for S in steps:
                    if S.attempted:
                        assert S.cond_dF < 1e3 and S.cond_M < 1e7, (n + m, S.cond_dF, S.cond_M)
            if rolling:
                assert steps[-1].restarts == 0 and len(steps) - 1 > 2 * mem_eff          # wrapped at least once (twice, in fact)
                assert [S.j for S in steps[1:]] == [d % mem_eff for d in range(len(steps) - 1)]
            else:
                assert steps[-1].restarts >= 2
            if seq not in A.DEGENERATE and seq != "large_eta":
                assert sum(S.success for S in steps) >= mem_eff, (seq, n + m, flags(recs))


@pytest.mark.parametrize("kind", list(A.KINDS))
def test_scaled_candidates_are_the_unscaled_ones_times_the_factor(kind):
    for (n, m, mem, min_mem) in CASES:
        base = run(kind, "random", n, m, mem, min_mem)
        for seq in ("scaled_up", "scaled_down"):
            fac = np.longdouble(A.SCALE[(seq, "f64")])
            for (r0, S0), (r1, S1) in zip(base, run(kind, seq, n, m, mem, min_mem)):
                assert (S0.success, S0.l, S0.j) == (S1.success, S1.l, S1.j)
                if S0.success:
                    for cand in (S1.cand, r1["cand"]):           # the reference's and the oracle's scaled candidate against the reference's unscaled one
                        d = np.asarray(cand, dtype=np.longdouble) / fac - S0.cand
                        g_norm = float(np.sqrt(S0.g @ S0.g))
                        assert float(np.sqrt(d @ d)) <= A.C_BOUND * EPS64 * S0.cond * (g_norm + S0.norm_dG * S0.eta_norm)


def test_the_constant_of_the_bound_is_the_measured_one():
    """measures the oracle's worst e / eps, and its worst eta error over the bound of eta with C = 1, again: the constants written in tests/anderson_cases.py are this machine's measurement (BLAS may sum in another
    order elsewhere: the measurement has to stay inside the bound, 16 times the recorded figure)"""
    for kind in A.KINDS:
        worst = worst_eta = 0.0
        unit = A.ReferenceAccelerator(kind, 8, 1, C=1.0)                  # for eta_bound with C = 1
        for (n, m, mem, min_mem) in CASES:
            for seq in A.SEQUENCES:
                for r, S in run(kind, seq, n, m, mem, min_mem):
                    if r["success"] and S.success:
                        worst = max(worst, A.ReferenceAccelerator.error(None, r["cand"], S) / EPS64)
                        d = np.asarray(r["eta"][:S.l], dtype=np.longdouble) - S.eta
                        d, bound = float(np.sqrt(d @ d)), unit.eta_bound(S)                # eta in slot order on both sides
                        assert d <= 2.0 * A.ORACLE_WORST_ETA_BY_KIND[kind] * bound, (kind, seq, n + m, d / bound if bound else d)
                        if bound > 0:
                            worst_eta = max(worst_eta, d / bound)
        print("%s: worst oracle e/eps %.3g (recorded %.3g), eta %.3g x its bound with C = 1 (recorded %.3g)"
              % (kind, worst, A.ORACLE_WORST_BY_KIND[kind], worst_eta, A.ORACLE_WORST_ETA_BY_KIND[kind]))
        assert worst <= 2.0 * A.ORACLE_WORST_BY_KIND[kind]
    assert A.C_BOUND == max(4.0, 16.0 * max(A.ORACLE_WORST_BY_KIND.values())) <= A.C_LIMIT
    assert A.C_ETA == max(A.C_BOUND, 16.0 * max(A.ORACLE_WORST_ETA_BY_KIND.values())) <= A.C_LIMIT


# ---- the batch trajectories of tests/test_gpu_batch_anderson_steps.py on the oracle's loop ------------------------------------------------------------------
class _Done(Exception):
    pass


def batch_problem(size, seed):
    rng = np.random.default_rng(seed)
    if size == "small":
        return util.random_qp(rng, 30, 3, 20, 15, soc_dims=(5, 3), p_shift=2.0)
    if size == "wide":                        # n > 512 and sparse enough for an LDS image: the <2, 4> register kernel (tests/test_gpu_batch_anderson_steps.py)
        return util.random_qp(rng, 520, 10, 100, 50, soc_dims=(5, 3), density=0.01, p_shift=2.0)
    return util.random_qp(rng, 600, 50, 500, 400, soc_dims=(50, 30), p_shift=2.0)


BATCH_ITERS = 45


def replay_on_oracle(p, mem):
    """45 iterations of the oracle's accelerated loop with eps = 0; the (g, x) pairs its accelerator is given go to the reference.  Returns per iteration
    (reference Step, oracle success) and the workspace."""
    st = O.Settings(kkt_solver="cg", accelerator="anderson", acc_mem=mem, eps_abs=0.0, eps_rel=0.0, adaptive_rho=False, check_infeasibility=10 ** 9, max_iter=10 ** 6)
    ws = O.Workspace(p["P"], p["q"], p["A"], p["b"], util.oracle_cones(p["sets"]), st)
    acc = ws.accelerator
    ref = A.ReferenceAccelerator("qr", ws.n + ws.m, mem, st.acc_min_mem)
    out = []
    update, accelerate = acc.update, acc.accelerate

    def upd(g, x):
        out.append([ref.step(g, x), None])
        update(g, x)

    def accel(g):
        accelerate(g)
        out[-1][1] = acc.was_successful()
        S = out[-1][0]
        if S.success and acc.was_successful():
            assert ref.error(g, S) <= A.C_BOUND * EPS64

    acc.update, acc.accelerate = upd, accel

    def record(it, *_):
        if it == BATCH_ITERS:
            raise _Done()

    with pytest.raises(_Done):
        ws.optimize(record=record)
    return out, ws


@pytest.mark.parametrize("size,mem", [("small", 15), ("small", 16), ("large", 15), ("wide", 15)])
def test_batch_trajectories_on_the_oracle(size, mem):
    for seed in (0, 1, 2):
        out, ws = replay_on_oracle(batch_problem(size, seed), mem)
        conds = [S.cond for S, _ in out if S.attempted]
        succ = sum(bool(ok) for _, ok in out)
        print("%s seed %d mem %d: cond <= %.3g, %d successes, %d restarts, %d safeguarding steps" % (size, seed, mem, max(conds), succ, out[-1][0].restarts, ws.safeguarding_iter))
        assert max(conds) < 1e5
        assert succ >= 25
        for S, ok in out:
            if S.l >= ws.st.acc_min_mem:
                assert S.success and ok and not S.singular and not S.eta_too_large
