"""COSMO_HIP_STEP_PASSES: the passes and the host sequencing around the two big kernels of an ADMM step (csrc/psd_polar.hip, csrc/kernels.hip, csrc/api.hip).
  1 (default)  k_bpolar_norm + k_bpolar_populate2 on cone-local workgroup ids instead of populate + scale; the persistent launch's counters cleared by populate2
               instead of a memset kernel; the verification decision of round 0 read from a mapped host word behind an event, with finish / rank enqueued gated
               before the host waits; k_tail stores the Krylov count into the mapped feedback ring and keeps s_tl in registers.
  0            the kernels and the sequence of before, in the same binary.
Every thread keeps its arithmetic, so the two forms must give the same BITS: the projections (reference semantics: src/convexset.jl:219-263), the ranks, the
verification record, the iterates of the loop and its Krylov counts.  Handles with the adaptive depth, with speculative fallback rounds and profiling handles
keep the old verification sequence under either value.
Sides: 17 ... 200, so that the padding up to ld and the stride of 16 columns per cone both leave remainders; batches of 1, 7, 8, 9 and 17 cones, so that the
last group of eight cones of the workgroup grid is short."""
import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj

pytestmark = pytest.mark.gpu

SIDES = (17, 33, 64, 65, 100, 129, 200)
ENV = ("COSMO_HIP_STEP_PASSES", "COSMO_HIP_POLAR_DATAFLOW", "COSMO_HIP_POLAR_DATAFLOW_GRID", "COSMO_HIP_POLAR_KLIFT", "COSMO_HIP_POLAR_ADAPT",
       "COSMO_HIP_POLAR_SPECULATE")
REC = ("verified", "unverified", "fallback_rounds", "err_max_e18")


def _env(monkeypatch, passes, **extra):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("COSMO_HIP_STEP_PASSES", passes)
    for k, v in extra.items():
        monkeypatch.setenv(k, v)


def _problem(tri_sides, sq_sides=(), seed=7, n=40):
    """min 1/2 |x|^2 + q'x  s.t.  A x + s = b, s in a product of PSD cones; one entry of A per row, b = indefinite symmetric matrices"""
    rng = np.random.default_rng(seed)
    sets, blocks = [], []
    for d in tri_sides:
        G = rng.standard_normal((d, d))
        blocks.append(cj.problems.svec((G + G.T) * (0.5 * rng.uniform(0.1, 10.0))))
        sets.append(cj.PsdConeTriangle(d * (d + 1) // 2))
    for d in sq_sides:
        G = rng.standard_normal((d, d))
        blocks.append(((G + G.T) * 0.5).reshape(-1, order="F"))
        sets.append(cj.PsdCone(d * d))
    b = np.concatenate(blocks)
    m = b.size
    A = sp.csc_matrix((rng.standard_normal(m), (np.arange(m), rng.integers(0, n, m))), shape=(m, n))
    return dict(P=sp.identity(n, format="csc"), q=rng.standard_normal(n), A=A, b=b, sets=sets)


def _inputs(tri_sides, sq_sides, seed, dtype):
    """four vectors s: random symmetric matrices; the same with an all-zero first cone (inv = 0); positive definite; negative definite"""
    rng = np.random.default_rng(seed)

    def vec(make):
        out = []
        for d in tri_sides:
            out.append(cj.problems.svec(make(d)))
        for d in sq_sides:
            out.append(make(d).reshape(-1, order="F"))
        return np.concatenate(out).astype(dtype)

    def sym(d):
        G = rng.standard_normal((d, d))
        return (G + G.T) * 0.5

    def spd(d):
        G = rng.standard_normal((d, d))
        return G @ G.T / d + 0.5 * np.eye(d)

    rnd = vec(sym)
    zero = rnd.copy()
    d0 = (list(tri_sides) + list(sq_sides))[0]
    zero[:(d0 * (d0 + 1) // 2 if tri_sides else d0 * d0)] = 0.0
    return dict(random=rnd, zero_cone=zero, posdef=vec(spd), negdef=-vec(spd))


def _project_all(prob, inputs, monkeypatch, passes, dtype=np.float64, **extra):
    _env(monkeypatch, passes, **extra)
    md = cj.Model(dtype=dtype); md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], cj.Settings(max_iter=5))
    cj.model.setup(md)
    h = md.handle
    out = {}
    for name, s in inputs.items():
        p, ranks, _ = h.project(s)
        ps = h.polar_stats()
        assert ps["batch_cones"] == len(prob["sets"])
        out[name] = (p, ranks.copy(), tuple(ps[k] for k in REC))
    h.close()
    return out


def _same_projections(a, b, what):
    for name in a:
        (pa, ra, ca), (pb, rb, cb) = a[name], b[name]
        assert np.all(np.isfinite(pa)), (what, name)
        assert np.array_equal(pa, pb), (what, name, int(np.sum(pa != pb)))
        assert np.array_equal(ra, rb), (what, name, ra, rb)
        assert ca == cb, (what, name, ca, cb)


def _sides(n, shift=0):
    return tuple(SIDES[(k + shift) % len(SIDES)] for k in range(n))


@pytest.mark.parametrize("n, form", [(1, "per_product"), (7, "per_product"), (8, "per_product"), (9, "per_product"), (17, "per_product"), (17, "dataflow")])
def test_projection_alone_is_bit_identical(n, form, monkeypatch):
    """cosmo_hip_project on a batch of n PsdConeTriangle cones: the launch-per-product schedule (the default of a small batch) and, for the largest batch,
    the persistent launch, whose counters populate2 clears"""
    extra = dict(COSMO_HIP_POLAR_DATAFLOW="0") if form == "per_product" else dict(COSMO_HIP_POLAR_DATAFLOW="1", COSMO_HIP_POLAR_DATAFLOW_GRID="16")
    tri = _sides(n, shift=n)
    prob, inputs = _problem(tri, seed=n), _inputs(tri, (), 100 + n, np.float64)
    old = _project_all(prob, inputs, monkeypatch, "0", **extra)
    new = _project_all(prob, inputs, monkeypatch, "1", **extra)
    _same_projections(new, old, (n, form))
    d0 = tri[0]
    assert np.all(new["zero_cone"][0][:d0 * (d0 + 1) // 2] == 0.0) and new["zero_cone"][1][0] == 0          # the zero matrix: inv = 0, rank 0
    assert list(new["posdef"][1]) == list(tri) and list(new["negdef"][1]) == [0] * n                          # full rank / rank 0


def test_projection_with_a_square_layout_cone(monkeypatch):
    tri, sq = _sides(17, shift=2), (100, 33)
    prob, inputs = _problem(tri, sq_sides=sq, seed=3), _inputs(tri, sq, 31, np.float64)
    for extra in (dict(COSMO_HIP_POLAR_DATAFLOW="0"), dict(COSMO_HIP_POLAR_DATAFLOW="1", COSMO_HIP_POLAR_DATAFLOW_GRID="16")):
        _same_projections(_project_all(prob, inputs, monkeypatch, "1", **extra), _project_all(prob, inputs, monkeypatch, "0", **extra), extra)


def test_projection_float32_library(monkeypatch):
    tri, sq = _sides(17, shift=4), (65,)
    prob, inputs = _problem(tri, sq_sides=sq, seed=11), _inputs(tri, sq, 41, np.float32)
    for extra in (dict(COSMO_HIP_POLAR_DATAFLOW="0"), dict(COSMO_HIP_POLAR_DATAFLOW="1", COSMO_HIP_POLAR_DATAFLOW_GRID="16")):
        new = _project_all(prob, inputs, monkeypatch, "1", dtype=np.float32, **extra)
        _same_projections(new, _project_all(prob, inputs, monkeypatch, "0", dtype=np.float32, **extra), extra)
        assert new["random"][0].dtype == np.float32


def _optimize(prob, monkeypatch, passes, iters, **extra):
    _env(monkeypatch, passes, **extra)
    st = cj.Settings(max_iter=iters, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9)
    md = cj.Model(); md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
    r = cj.optimize(md)
    ps = md.handle.polar_stats()
    md.handle.close()
    return r, ps


def _same_runs(a, b):
    (ra, pa), (rb, pb) = a, b
    assert np.array_equal(ra.x, rb.x) and np.array_equal(ra.s, rb.s) and np.array_equal(ra.y, rb.y)
    assert tuple(pa[k] for k in REC) == tuple(pb[k] for k in REC), (pa, pb)
    assert ra.kkt_iters_total == rb.kkt_iters_total and ra.iter == rb.iter


def test_failing_verification_small_batch(monkeypatch):
    """A main schedule of two lifting steps (COSMO_HIP_POLAR_KLIFT=2) cannot lift the small eigenvalues of these matrices: round 0 fails in every projection,
    the gated finish / rank are skipped on the device, the repair rounds run and finish / rank are enqueued again behind them."""
    prob = _problem(_sides(17, shift=1), sq_sides=(65,), seed=5)
    for extra in (dict(COSMO_HIP_POLAR_DATAFLOW="0"), dict(COSMO_HIP_POLAR_DATAFLOW="1", COSMO_HIP_POLAR_DATAFLOW_GRID="16")):
        old = _optimize(prob, monkeypatch, "0", 4, COSMO_HIP_POLAR_KLIFT="2", **extra)
        new = _optimize(prob, monkeypatch, "1", 4, COSMO_HIP_POLAR_KLIFT="2", **extra)
        assert old[1]["fallback_rounds"] > 0 and new[1]["fallback_rounds"] > 0
        _same_runs(new, old)


def test_failing_verification_behind_the_persistent_launch(monkeypatch):
    """The means of tests/test_gpu_polar_paired_tiles.py::test_repair_rounds_behind_the_paired_launch: BASELINE config 5 for 50 iterations, in which some
    projections fail their verification at the default depth."""
    prob = cj.problems.chordal_sdp()
    old = _optimize(prob, monkeypatch, "0", 50)
    new = _optimize(prob, monkeypatch, "1", 50)
    assert old[1]["fallback_rounds"] > 0 and new[1]["fallback_rounds"] > 0
    assert new[1]["unverified"] == 0
    _same_runs(new, old)


def _loop(prob, monkeypatch, passes, pieces=(1, 2, 4, 5), profiling=False, **extra):
    _env(monkeypatch, passes, **extra)
    st = cj.Settings(max_iter=10 ** 6, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9, check_termination=10 ** 9)
    md = cj.Model(); md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
    cj.model.setup(md)
    h = md.handle
    if profiling:
        h.set_profiling(1)
    h.set_iterates(md.x, md.s, md.mu); h.admm_init()
    for k in pieces:
        h.admm_iterate_checked(k)
    its, stats, ps = h.get_iterates(), h.get_stats(), h.polar_stats()
    h.close()
    assert stats["admm_iters"] == sum(pieces)
    return its, (stats["kkt_iters_total"], stats["kkt_budget_stalls"]), tuple(ps[k] for k in REC)


def _same_loops(a, b, what):
    for va, vb, name in zip(a[0], b[0], ("w", "w_prev", "s", "mu")):
        assert np.all(np.isfinite(va)), (what, name)
        assert np.array_equal(va, vb), (what, name, int(np.sum(va != vb)))
    assert a[1] == b[1] and a[1][0] > 0, (what, a[1], b[1])
    assert a[2] == b[2], (what, a[2], b[2])


@pytest.fixture(scope="module")
def small_sdp():
    return cj.problems.chordal_sdp(ncliques=6, dmin=20, dmax=70, n_total=1500, n_zero=30, n_nonneg=100, seed=5)


def test_loop_in_uneven_pieces_is_bit_identical(small_sdp, monkeypatch):
    """12 iterations as calls of 1, 2, 4 and 5: the feedback ring filled by k_tail, the s_tl store dropped, the verification decision without a copy"""
    _same_loops(_loop(small_sdp, monkeypatch, "1"), _loop(small_sdp, monkeypatch, "0"), "loop")


def test_loop_with_the_persistent_launch_is_bit_identical(monkeypatch):
    """the same on 24 cliques with the persistent launch forced on: its counters are cleared by populate2 in every iteration"""
    prob = cj.problems.chordal_sdp(ncliques=24, dmin=20, dmax=70, n_total=4000, n_zero=50, n_nonneg=200, seed=6)
    extra = dict(COSMO_HIP_POLAR_DATAFLOW="1", COSMO_HIP_POLAR_DATAFLOW_GRID="16")
    _same_loops(_loop(prob, monkeypatch, "1", **extra), _loop(prob, monkeypatch, "0", **extra), "loop, persistent launch")


@pytest.mark.parametrize("shape", ["adapt", "speculate", "profiling"])
def test_handles_that_keep_the_old_verification_sequence(shape, small_sdp, monkeypatch):
    """adaptive depth, speculative rounds, profiling: the same bits under either switch value"""
    extra = {"adapt": dict(COSMO_HIP_POLAR_ADAPT="1"), "speculate": dict(COSMO_HIP_POLAR_SPECULATE="1"), "profiling": {}}[shape]
    new = _loop(small_sdp, monkeypatch, "1", profiling=shape == "profiling", **extra)
    old = _loop(small_sdp, monkeypatch, "0", profiling=shape == "profiling", **extra)
    _same_loops(new, old, shape)
