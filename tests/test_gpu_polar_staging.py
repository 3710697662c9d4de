"""How a tile's operand panels reach LDS in the ragged product kernels (csrc/psd_polar.hip: symm_mainloop_r).  A diagonal tile of a square product
(Y = U^2, Y^2: both operands the same matrix, i0 == j0) loads and stores ONE panel per k-step and reads both fragments from its image; every other tile
stages two panels as before.  The values reaching each matrix instruction and their order are unchanged, so every form must give the same BITS:
  * persistent  -- k_polar_dataflow (COSMO_HIP_POLAR_DATAFLOW=1): single-panel diagonal tiles, operands read past the L1,
  * per product -- k_symm_gemm_batch_r (COSMO_HIP_POLAR_DATAFLOW=0): single-panel diagonal tiles, plain loads,
  * quadrant    -- k_symm_gemm_batch (COSMO_HIP_POLAR_BATCH_RAGGED=0): the 64 x 64 quadrant kernel, which always stages both panels: the reference.
Reference semantics: the PSD projections of src/convexset.jl:219-263; LAPACK (numpy.linalg.eigh) is the independent check of the values.
The sides cover k-loops of 2...13 panels (the loop is peeled at its last panel and alternates two LDS buffers: even / odd counts end in different
buffers), one to four parts per side, part widths of 1-4 blocks of 16, diagonal and off-diagonal tiles."""
import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj

pytestmark = pytest.mark.gpu
F = cj._ffi
EPS = np.finfo(np.float64).eps
SIDES = [17, 31, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 113, 129, 160, 193, 200]
FORMS = {"persistent": dict(COSMO_HIP_POLAR_DATAFLOW="1"), "per_product": dict(COSMO_HIP_POLAR_DATAFLOW="0"),
         "quadrant": dict(COSMO_HIP_POLAR_DATAFLOW="0", COSMO_HIP_POLAR_BATCH_RAGGED="0")}


def _sets(kind):
    return [cj.PsdConeTriangle(d * (d + 1) // 2) if kind == "tri" else cj.PsdCone(d * d) for d in SIDES]


def _inputs(kind, seed):
    """random symmetric indefinite matrices (Gaussian entries: about half of each spectrum on either side of 0), one scale per cone"""
    rng = np.random.default_rng(seed)
    mats = []
    for d in SIDES:
        G = rng.standard_normal((d, d))
        mats.append((G + G.T) * (0.5 * rng.uniform(0.1, 10.0)))
    s = np.concatenate([cj.problems.svec(X) if kind == "tri" else X.reshape(-1, order="F") for X in mats])
    return mats, s


def _handle(sets, form, monkeypatch):
    for k in ("COSMO_HIP_POLAR_DATAFLOW", "COSMO_HIP_POLAR_BATCH_RAGGED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    m = sum(K.dim for K in sets)
    h = cj.Handle(0)
    h.set_problem(sp.identity(2, format="csc"), np.zeros(2), sp.csc_matrix((m, 2)), np.zeros(m))
    h.set_cones([K.kind for K in sets], [K.dim for K in sets], None, None)
    return h


def _project_all(kind, form, inputs, monkeypatch):
    """the projections of `inputs`, one after the other on ONE handle: [(s, ranks, err_max_e18)], and whether the persistent launch ran"""
    sets = _sets(kind)
    h = _handle(sets, form, monkeypatch)
    res = []
    for s in inputs:
        out, ranks, _ = h.project(s)
        ps = h.polar_stats()
        assert ps["batch_cones"] == len(sets) and ps["unverified"] == 0
        res.append((out.copy(), np.asarray(ranks).copy(), ps["err_max_e18"]))
    df = h.polar_dataflow_stats()
    h.close()
    assert df["enabled"] == (1 if form == "persistent" else 0) and (df["launches"] >= len(inputs)) == (form == "persistent")
    return res


@pytest.fixture(scope="module")
def five_inputs():
    return {kind: [_inputs(kind, 4100 + i) for i in range(5)] for kind in ("tri", "square")}


@pytest.mark.parametrize("kind", ["tri", "square"])
def test_every_loop_shape_is_bit_identical_in_all_three_forms(kind, five_inputs, monkeypatch):
    """One projection per form of the 17 sides: s, ranks and the verification's error bound are the same bits in the persistent form, the
    launch-per-product form (both single-panel on diagonal tiles of square products) and the quadrant kernel (two panels everywhere)."""
    s = five_inputs[kind][0][1]
    ref = _project_all(kind, "quadrant", [s], monkeypatch)[0]
    for form in ("persistent", "per_product"):
        got = _project_all(kind, form, [s], monkeypatch)[0]
        assert np.array_equal(got[0], ref[0]), form
        assert np.array_equal(got[1], ref[1]), form
        assert got[2] == ref[2], (form, got[2], ref[2])


@pytest.mark.parametrize("kind", ["tri", "square"])
def test_five_projections_on_reused_work_buffers_stay_bit_identical(kind, five_inputs, monkeypatch):
    """Five different inputs through the same handle: from the second on, every work matrix a tile reads was written by an earlier projection and
    rewritten by this one -- a panel served from a stale cache line, or a fragment read from the wrong LDS image, can only show here."""
    inputs = [s for _, s in five_inputs[kind]]
    ref = _project_all(kind, "quadrant", inputs, monkeypatch)
    for form in ("persistent", "per_product"):
        got = _project_all(kind, form, inputs, monkeypatch)
        for i, (g, r) in enumerate(zip(got, ref)):
            assert np.array_equal(g[0], r[0]) and np.array_equal(g[1], r[1]) and g[2] == r[2], (form, i)


@pytest.mark.parametrize("kind", ["tri", "square"])
def test_against_lapack(kind, five_inputs, monkeypatch):
    """The persistent form against numpy.linalg.eigh: ||dX+||_F <= 64 d eps ||X||_F per cone (the bound of tests/test_gpu_baseline_configs.py)."""
    mats, s = five_inputs[kind][0]
    out = _project_all(kind, "persistent", [s], monkeypatch)[0][0]
    off = 0
    for d, X, K in zip(SIDES, mats, _sets(kind)):
        lam, Q = np.linalg.eigh(X)
        P = (Q * np.maximum(lam, 0.0)) @ Q.T
        P = (P + P.T) / 2
        ref = cj.problems.svec(P) if kind == "tri" else P.reshape(-1, order="F")
        err = np.linalg.norm(out[off:off + K.dim] - ref)                  # svec is an isometry: the Frobenius norm in both layouts
        assert err <= 64 * d * EPS * np.linalg.norm(X), (d, err / (d * EPS * np.linalg.norm(X)))
        off += K.dim


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_twelve_admm_iterations_persistent_form_against_the_quadrant_kernel(dtype, monkeypatch):
    """A 40-clique chordal SDP, persistent form forced on, against the same loop on the quadrant kernel: the iterates and the Krylov counts of twelve
    ADMM iterations are identical, in both libraries (the single-panel load is in the Float64 and the Float32 instantiation)."""
    prob = cj.problems.chordal_sdp(ncliques=40, n_total=6000, n_zero=100, n_nonneg=500)
    res = {}
    for form in ("quadrant", "persistent"):
        for k in ("COSMO_HIP_POLAR_DATAFLOW", "COSMO_HIP_POLAR_BATCH_RAGGED"):
            monkeypatch.delenv(k, raising=False)
        for k, v in FORMS[form].items():
            monkeypatch.setenv(k, v)
        st = cj.Settings(max_iter=12, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9)
        md = cj.Model(dtype=dtype); md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
        r = cj.optimize(md)
        df = md.handle.polar_dataflow_stats()
        md.handle.close()
        assert r.iter == 12 and df["enabled"] == (1 if form == "persistent" else 0)
        res[form] = r
    a, b = res["quadrant"], res["persistent"]
    assert np.array_equal(a.x, b.x) and np.array_equal(a.s, b.s) and np.array_equal(a.y, b.y)
    assert a.kkt_iters_total == b.kkt_iters_total
