"""The single-problem accelerator (csrc/anderson.hip) one update and one candidate at a time, through the step hooks Handle.accel_pre / accel_post /
accel_restart, which run the functions the accelerated loop of cosmo_hip_optimize runs (aa_enqueue_pre, aa_fetch_flags, aa_enqueue_guard,
aa_enqueue_reset, aa_restart) on vectors given by the test.  Every step is compared with tests/anderson_cases.ReferenceAccelerator fed the same pairs:
bookkeeping and flags exactly, inner products within the dot-product bound, R and the candidate within C eps cond, eta within its own measured constant
C_ETA (ReferenceAccelerator.eta_bound) -- the constants and the metric: module docstring and constants of tests/anderson_cases.py;
tests/test_anderson_cases_host.py proves the cases and the reference on the CPU.  Measured on an MI355X: worst e / (C eps) of a candidate 0.032 over all
kinds, shapes, sequences and both dtypes.

Shapes (n, m, mem) -- the smallest that reach each path:
    2, 6, 15         N = 8: mem clipped to N, square history, l = 8 is the top of the <8> instantiations
    10, 30, 32       N = 40: l crosses 8 -> 9 and 16 -> 17, the <AA_MAX_MEM> instantiations of k_aa_qtf / k_aa_apply / k_aa_gram up to l = 32 (min_mem 3 and 1)
    300, 725, 17     N = 1025: two workgroups, the second owns one element; reduce_partials_sum with nparts = 2; l 16 -> 17
    1000, 2000, 9    N = 3000: three workgroups, ragged last one; l 8 -> 9
A threshold decision (||eta|| <= eta_max) the reference takes closer to the threshold than the error bound of eta, or at C eps cond >= 1/2, decides nothing
about the device's flag: such a step is `undecided`; its bookkeeping, inner products and the bit-for-bit rules are still checked.  On `near_dependent`
(cond(M) about 1e14) that leaves the eta_max test compared for the QR kind in Float64 only; the sequence `large_eta` (eta_max = 3, ||eta|| large by the size of
f at cond(M) < 1e6) drives it decided in every kind, shape and dtype, and the test counts its failures."""
import faulthandler

import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from tests import anderson_cases as A

pytestmark = pytest.mark.gpu
F = cj._ffi
LD = np.longdouble
CASE_LIMIT_S = 120
CASES = [(n, m, mem, mm) for (n, m, mem) in A.SHAPES for mm in ((A.MIN_MEM, 1) if n + m == 40 else (A.MIN_MEM,))]
TAU = 2.0


@pytest.fixture(autouse=True)
def _case_time_limit():
    """a case that hangs takes the whole process down instead of holding the GPU: nothing runs after a hang"""
    faulthandler.dump_traceback_later(CASE_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def handle():
    """handle(n, m, dtype_id): P = I, one nonzero per row of A, Nonnegatives, CG, no scaling; iterates set.  One handle per shape and dtype for the module,
    closed after its last test; every test installs the accelerator it needs first."""
    made = {}

    def get(n, m, dtype_id):
        key = (n, m, dtype_id)
        if key not in made:
            dtype = A.DTYPES[dtype_id]
            h = cj.Handle(0, dtype=dtype)
            h.set_problem(sp.identity(n, format="csc"), np.zeros(n), sp.csc_matrix((np.ones(m), (np.arange(m), np.arange(m) % n)), shape=(m, n)), np.zeros(m))
            h.set_cones([F.NONNEG], [m])
            p = F.default_params(dtype)
            p.kkt_kind = F.KKT_CG
            h.set_params(p)
            h.set_iterates()
            made[key] = h
        return made[key]

    yield get
    for h in made.values():
        h.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def nrm(v):
    v = np.asarray(v, dtype=LD)
    return float(np.sqrt(v @ v))


def install(h, kind, mem, min_mem, eta_max=A.ETA_MAX, **kw):
    h.set_accelerator(A.KINDS[kind][0], mem=mem, min_mem=min_mem, safeguard=True, safeguard_tol=TAU, eta_max=eta_max, **kw)


def drive(h, kind, seq_name, n, m, mem, min_mem, dtype_id, steps=None):
    """the sequence through the device and the reference: list of (g, x, w, info, Step)"""
    dtype = A.DTYPES[dtype_id]
    N = n + m
    seq = A.Sequence(seq_name, N, 0, dtype)
    ref = A.ReferenceAccelerator(kind, N, mem, min_mem, eta_max=A.eta_max_of(seq_name), dtype=dtype)
    out, cand = [], None
    for k in range(steps or A.steps_of(mem, N)):
        g, x = seq.next(cand)
        S = ref.step(g, x, it=k + 2)
        w, info = h.accel_pre(k + 2, g, x)
        out.append((g, x, w, info, S))
        cand = w
    return out


def check_steps(recs, kind, dtype_id, N):
    """every rule of the module docstring on one run; returns (worst e / (C eps) of the candidates, compared candidates, undecided steps, decided steps
    that failed on eta on the device and in the reference)"""
    dtype = A.DTYPES[dtype_id]
    eps = A.eps_of(dtype)
    ne = A.KINDS[kind][3]
    gam = A.gamma(N + 2, dtype)
    worst, compared, undecided, eta_failures = 0.0, 0, 0, 0
    prev_fail = (0, 0)
    ref = A.ReferenceAccelerator(kind, N, 1, dtype=dtype)                # for its bounds only
    for k, (g, x, w, info, S) in enumerate(recs):
        at = (kind, dtype_id, N, k)
        l = S.l
        assert (info["attempted"], info["l"], info["j"], info["restarts"], info["active"]) == (int(S.attempted), S.l, S.j, S.restarts, 1), (at, info, S.l, S.j, S.restarts)
        assert info["mem"] >= l
        if S.j == -1 or (k > 0 and S.restarts != recs[k - 1][4].restarts):       # the history was emptied (first pair, memory restart): the failure counters start over
            prev_fail = (0, 0)
        d_sing, d_eta = info["fail_singular"] - prev_fail[0], info["fail_eta"] - prev_fail[1]
        prev_fail = (info["fail_singular"], info["fail_eta"])
        assert (d_sing, d_eta) in ((0, 0), (1, 0), (0, 1)) and info["success"] == int(bool(info["attempted"]) and d_sing == 0 and d_eta == 0), (at, info)
        if not info["success"]:
            assert same_bits(w, g), at                                   # no candidate: g comes back bit for bit
        if not S.attempted:
            continue
        # ---- inner products: the dot-product bound, no constant ----
        assert abs(float(info["nrm_f"]) - S.nrm_f) <= (gam + 2 * eps) * S.nrm_f, (at, info["nrm_f"], S.nrm_f)
        if ne:
            Md = np.asarray(info["R"][:l, :l], dtype=LD)
            assert np.all(np.abs(Md - S.M) <= gam * S.M_abs + eps * np.abs(S.M)), (at, np.argwhere(~(np.abs(Md - S.M) <= gam * S.M_abs + eps * np.abs(S.M)))[:4].tolist())
        en = nrm(info["eta"][:l])
        if d_sing == 0 and np.isfinite(en):
            assert abs(float(info["eta_norm"]) - en) <= 4 * eps * en, (at, info["eta_norm"], en)
        rel = A.C_BOUND * eps * S.cond
        # ---- flags ----
        if S.decided:
            assert (info["success"], d_sing, d_eta) == (int(S.success), int(S.singular), int(S.eta_too_large)), (at, info, S.cond, S.eta_norm)
            eta_failures += d_eta
        else:
            undecided += 1
        if S.singular or d_sing or not rel < 0.5:
            continue
        if not ne:
            Rd = np.asarray(info["R"][:l, :l], dtype=LD)
            assert not np.tril(Rd, -1).any(), at
            assert nrm((Rd - S.R).ravel()) <= rel * S.norm_dF, (at, nrm((Rd - S.R).ravel()) / (rel * S.norm_dF))
        if S.success and info["success"]:
            assert nrm(np.asarray(info["eta"][:l], dtype=LD) - S.eta) <= ref.eta_bound(S), (at, nrm(np.asarray(info["eta"][:l], dtype=LD) - S.eta) / max(ref.eta_bound(S), 1e-300))
            e = A.ReferenceAccelerator.error(None, w, S) / (A.C_BOUND * eps)
            worst = max(worst, e); compared += 1
            assert e <= 1.0, (at, e, S.cond)
    return worst, compared, undecided, eta_failures


@pytest.mark.parametrize("seq", A.SEQUENCES)
@pytest.mark.parametrize("n,m,mem,min_mem", CASES)
@pytest.mark.parametrize("dtype_id", ["f64", "f32"])
@pytest.mark.parametrize("kind", list(A.KINDS))
def test_every_step_against_the_reference(handle, kind, dtype_id, n, m, mem, min_mem, seq):
    h = handle(n, m, dtype_id)
    install(h, kind, mem, min_mem, eta_max=A.eta_max_of(seq))
    recs = drive(h, kind, seq, n, m, mem, min_mem, dtype_id)
    mem_eff = min(mem, n + m)
    assert recs[0][3]["mem"] == mem_eff
    worst, compared, undecided, eta_failures = check_steps(recs, kind, dtype_id, n + m)
    dev = "".join("." if not i["attempted"] else "+" if i["success"] else "x" for _, _, _, i, _ in recs)
    print("ANDERSON_STEP kind=%s dtype=%s N=%d mem=%d min_mem=%d seq=%s worst_e_over_Ceps=%.3g compared=%d undecided=%d eta_failures=%d %s"
          % (kind, dtype_id, n + m, mem, min_mem, seq, worst, compared, undecided, eta_failures, dev))
    # floors, so that what is compared cannot shrink unnoticed; each is a property of the inputs that tests/test_anderson_cases_host.py proves on the reference
    if seq in ("random", "scaled_up", "scaled_down"):
        assert compared >= mem_eff
        if dtype_id == "f64":
            assert undecided == 0
    if seq == "contractive":            # the first candidate is taken on the reference's own numbers; in Float64 at N >= 1025 cond stays small throughout
        assert compared >= (mem_eff if dtype_id == "f64" and n + m >= 1025 else 1)
    if seq == "large_eta":              # ||eta|| > eta_max, decided in every kind and dtype: the device's fail_eta counted the reference's failures
        assert eta_failures >= mem_eff - A.MIN_MEM
    if seq == "repeat":                                                 # an exactly zero column: decided in either dtype
        assert sum(i["fail_singular"] > 0 and not i["success"] and i["attempted"] for _, _, _, i, _ in recs) >= 2


@pytest.mark.parametrize("n,m,mem,min_mem", CASES)
@pytest.mark.parametrize("dtype_id", ["f64", "f32"])
@pytest.mark.parametrize("kind", list(A.KINDS))
def test_post_hook_declines_far_above_the_threshold_and_resets(handle, kind, dtype_id, n, m, mem, min_mem):
    dtype = A.DTYPES[dtype_id]
    N = n + m
    eps = A.eps_of(dtype)
    h = handle(n, m, dtype_id)
    install(h, kind, mem, min_mem)
    recs = drive(h, kind, "random", n, m, mem, min_mem, dtype_id, steps=A.MIN_MEM + 2)
    g, x, cand, info, S = recs[-1]
    assert info["success"] == 1 and S.success
    u = np.random.default_rng(7).standard_normal(N)
    u /= np.linalg.norm(u)
    for factor, want in ((0.5, 0), (1.5, 1)):
        w_in = (cand.astype(np.float64) - factor * TAU * S.nrm_f * u).astype(dtype)
        w, wp, declined, na = h.accel_post(w_in, cand)
        d = (cand - w_in).astype(dtype)                                   # one rounding per element, as on the device
        assert declined == want, (kind, dtype_id, N, factor, na, S.nrm_f)
        assert abs(float(na) - nrm(d)) <= (A.gamma(N + 2, dtype) + 2 * eps) * nrm(d)
        if declined:
            assert same_bits(w, g) and same_bits(wp, g)
        else:
            assert same_bits(w, w_in) and same_bits(wp, cand)
    # the guard left the history alone: the next update continues the run
    rng = np.random.default_rng(11)
    _, nxt = h.accel_pre(99, rng.standard_normal(N).astype(dtype), rng.standard_normal(N).astype(dtype))
    assert (nxt["l"], nxt["j"], nxt["success"]) == (info["l"] + 1, info["j"] + 1, 1)


@pytest.mark.parametrize("dtype_id", ["f64", "f32"])
@pytest.mark.parametrize("kind", list(A.KINDS))
def test_restart_and_a_fresh_accelerator_give_identical_bits(handle, kind, dtype_id):
    n, m, mem = 300, 725, 9                                               # two workgroups; 2 * 9 + 5 = 23 steps, three runs
    h = handle(n, m, dtype_id)
    install(h, kind, mem, A.MIN_MEM)
    runs = [drive(h, kind, "random", n, m, mem, A.MIN_MEM, dtype_id)]
    h.accel_restart()
    runs.append(drive(h, kind, "random", n, m, mem, A.MIN_MEM, dtype_id))
    install(h, kind, mem, A.MIN_MEM)
    runs.append(drive(h, kind, "random", n, m, mem, A.MIN_MEM, dtype_id))
    for run in runs:
        assert (run[0][3]["j"], run[0][3]["l"], run[0][3]["attempted"]) == (-1, 0, 0)
    for other in runs[1:]:
        for (_, _, w0, i0, _), (_, _, w1, i1, _) in zip(runs[0], other):
            assert same_bits(w0, w1)
            assert {k: i0[k] for k in F.Handle.ACCEL_PRE_INFO} == {k: i1[k] for k in F.Handle.ACCEL_PRE_INFO}
            assert same_bits(i0["R"], i1["R"]) and same_bits(i0["eta"], i1["eta"])
            assert same_bits(np.array([i0["nrm_f"], i0["eta_norm"]]), np.array([i1["nrm_f"], i1["eta_norm"]]))
    assert runs[0][-1][3]["restarts"] == 2 * (not A.KINDS[kind][2])


@pytest.mark.parametrize("dtype_id", ["f64", "f32"])
def test_activation_and_refusals(handle, dtype_id):
    n, m = 10, 30
    dtype = A.DTYPES[dtype_id]
    h = handle(n, m, dtype_id)
    rng = np.random.default_rng(3)
    g, x = rng.standard_normal(n + m).astype(dtype), rng.standard_normal(n + m).astype(dtype)
    install(h, "qr", 5, 1, start_iter=5)
    for it in (1, 4):
        w, info = h.accel_pre(it, g, x)
        assert (info["attempted"], info["success"], info["active"], info["j"], info["l"]) == (0, 0, 0, -1, 0) and same_bits(w, g)
    w, info = h.accel_pre(5, g, x)
    assert (info["attempted"], info["active"], info["j"], info["l"]) == (0, 1, -1, 0) and same_bits(w, g)      # active: the first pair initialises
    w, info = h.accel_pre(2, 2 * g, x)                                                                        # once active it stays active
    assert (info["attempted"], info["active"], info["j"], info["l"]) == (1, 1, 0, 1)
    install(h, "qr", 5, 1, start_accuracy=1e-3)                    # AccuracyActivation: only a termination check of the loop activates it
    for it in (2, 100, 10 ** 6):
        w, info = h.accel_pre(it, g, x)
        assert (info["attempted"], info["active"], info["j"]) == (0, 0, -1) and same_bits(w, g)
    h.set_accelerator(F.ACCEL_EMPTY)
    for call in (lambda: h.accel_pre(2, g, x), lambda: h.accel_post(g, x), h.accel_restart):
        with pytest.raises(F.CosmoHipError) as e:
            call()
        assert e.value.code == 1                                    # COSMO_HIP_ERR_INVALID: no accelerator
    stats = h.accel_stats()
    assert stats["accelerated"] == 0 and stats["safeguarding_iter"] == 0
