"""Paired product tiles in the persistent launch of the batched sign iteration (csrc/psd_polar.hip: k_polar_dataflow_pair, paired_item).  A queue item is
two ragged tiles (I, J), (I, J + 1) of one cone executed by one workgroup of 512 threads: waves 0-3 compute the first tile, waves 4-7 the second, the A panel
of block row I is staged in LDS once per k-panel for both, and on a diagonal + neighbour item of a square product its image is also the diagonal tile's B.
Every half runs ragged_tile's block-to-wave deal, matrix instruction sequence and k order, so the iterates must be the same BITS as in the launch-per-product
form (COSMO_HIP_POLAR_DATAFLOW=0, k_symm_gemm_batch_r), with the same verification record.  Reference semantics: the PSD projections of
src/convexset.jl:219-263, independent of each other across cones.
A side d is cut into P = ceil(ceil(d / 16) / 4) parts; block row I of the upper triangle holds P - I tiles, taken two at a time from the diagonal:
  P = 1  one single diagonal tile                                  (17, 64)
  P = 2  diagonal + neighbour, one lone diagonal                   (65, 100, 128)
  P = 3  ... and a single off-diagonal tile left over in row 0     (129, 192)
  P = 4  ... and a pair of off-diagonal tiles in row 0             (193, 200)
A small COSMO_HIP_POLAR_DATAFLOW_GRID (two workgroups per XCD) makes every workgroup walk through many items of several cones and products."""
import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj

pytestmark = pytest.mark.gpu

CASES = {"P1": (17, 64), "P2": (65, 100, 128), "P3": (129, 192), "P4": (193, 200)}
MIXED = (17, 64, 65, 100, 129, 193, 200)
# COSMO_HIP_POLAR_PAIRED: 1 = paired items (the form under test), 3 = the tiles that leaves single paired along the last block column as well (they share
# the column's B panel), 2 = the 512-thread kernel with every tile a single item, 0 = the 256-thread kernel
FORMS = {"per_product": dict(COSMO_HIP_POLAR_DATAFLOW="0"),
         "paired": dict(COSMO_HIP_POLAR_DATAFLOW="1", COSMO_HIP_POLAR_DATAFLOW_GRID="16", COSMO_HIP_POLAR_PAIRED="1"),
         "paired_columns": dict(COSMO_HIP_POLAR_DATAFLOW="1", COSMO_HIP_POLAR_DATAFLOW_GRID="16", COSMO_HIP_POLAR_PAIRED="3"),
         "singles": dict(COSMO_HIP_POLAR_DATAFLOW="1", COSMO_HIP_POLAR_DATAFLOW_GRID="16", COSMO_HIP_POLAR_PAIRED="2"),
         "tiles256": dict(COSMO_HIP_POLAR_DATAFLOW="1", COSMO_HIP_POLAR_DATAFLOW_GRID="16", COSMO_HIP_POLAR_PAIRED="0")}
ENV = ("COSMO_HIP_POLAR_DATAFLOW", "COSMO_HIP_POLAR_DATAFLOW_GRID", "COSMO_HIP_POLAR_PAIRED")


def _problem(tri_sides, sq_sides=(), seed=7, n=40):
    """min 1/2 |x|^2 + q'x  s.t.  A x + s = b, s in a product of PSD cones; one entry of A per row, b = indefinite symmetric matrices (about half of every
    spectrum is cut off by the projections, from the first iteration on)"""
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


def _run(prob, form, monkeypatch, iters=3, dtype=np.float64):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    st = cj.Settings(max_iter=iters, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9)
    md = cj.Model(dtype=dtype); md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
    r = cj.optimize(md)
    h = md.handle
    w, _, s, mu = h.get_iterates()
    ps, df = h.polar_stats(), h.polar_dataflow_stats()
    h.close()
    assert r.iter == iters and ps["batch_cones"] == len(prob["sets"]) and ps["unverified"] == 0
    if form == "per_product":
        assert df["enabled"] == 0 and df["launches"] == 0
    else:
        assert df["enabled"] == 1 and df["launches"] >= iters and df["workgroups"] == 16
    return dict(w=w, s=s, mu=mu, rec=(ps["verified"], ps["fallback_rounds"], ps["err_max_e18"]), tiles=df["tiles_per_product"])


def _same(a, b, what):
    for k in ("w", "s", "mu"):
        assert np.all(np.isfinite(a[k])), (what, k)
        assert np.array_equal(a[k], b[k]), (what, k, int(np.sum(a[k] != b[k])))
    assert a["rec"] == b["rec"], (what, a["rec"], b["rec"])


@pytest.mark.parametrize("case", sorted(CASES))
def test_each_pairing_case_is_bit_identical_to_the_launch_per_product_form(case, monkeypatch):
    """24-36 triangle cones of one P (three or more per XCD), three ADMM iterations: w, s, mu and the verification record."""
    prob = _problem(CASES[case] * 12)
    ref = _run(prob, "per_product", monkeypatch)
    got = _run(prob, "paired", monkeypatch)
    _same(got, ref, case)
    _same(_run(prob, "paired_columns", monkeypatch), ref, case + " columns")
    P = {"P1": 1, "P2": 2, "P3": 3, "P4": 4}[case]
    assert got["tiles"] == len(prob["sets"]) * P * (P + 1) // 2      # the sides do produce this case


def test_mixed_batch_with_a_square_cone_all_queue_forms(monkeypatch):
    """All pairing cases in one batch, three cones of every side plus two PsdCone (square layout) cones: the paired items, the same kernel with single
    items only and the 256-thread kernel all give the bits of the launch-per-product form."""
    prob = _problem(MIXED * 3, sq_sides=(100, 193))
    ref = _run(prob, "per_product", monkeypatch)
    for form in ("paired", "paired_columns", "singles", "tiles256"):
        _same(_run(prob, form, monkeypatch), ref, form)


def test_float32_library_mixed_batch(monkeypatch):
    """libcosmo_hip_f32.so: the same code for float (8-byte operand pairs, v_mfma_f32_16x16x4_f32)."""
    prob = _problem(MIXED * 3, sq_sides=(100,), seed=11)
    ref = _run(prob, "per_product", monkeypatch, dtype=np.float32)
    _same(_run(prob, "paired", monkeypatch, dtype=np.float32), ref, "float32")


def test_repair_rounds_behind_the_paired_launch(monkeypatch):
    """BASELINE config 5 for 50 iterations (tests/test_gpu_polar_dataflow.py): some projections fail their verification and are repaired by
    launch-per-product rounds behind the persistent launch, which here runs its default items (pairs along rows and the last column) at its default grid."""
    prob = cj.problems.chordal_sdp()
    out = {}
    for form, env in (("paired", dict(COSMO_HIP_POLAR_DATAFLOW="1")), ("per_product", dict(COSMO_HIP_POLAR_DATAFLOW="0"))):
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        st = cj.Settings(max_iter=50, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9)
        md = cj.Model(); md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
        r = cj.optimize(md)
        out[form] = (r, md.handle.polar_stats(), md.handle.polar_dataflow_stats())
        md.handle.close()
    (r1, p1, d1), (r0, p0, d0) = out["paired"], out["per_product"]
    assert d1["enabled"] == 1 and d1["launches"] >= 50 and d0["enabled"] == 0
    assert p1["fallback_rounds"] > 0                                  # a repair round did run behind the launch
    assert np.array_equal(r0.x, r1.x) and np.array_equal(r0.s, r1.s) and np.array_equal(r0.y, r1.y)
    assert (p0["verified"], p0["fallback_rounds"], p0["err_max_e18"]) == (p1["verified"], p1["fallback_rounds"], p1["err_max_e18"]) and p1["unverified"] == 0
    assert r0.kkt_iters_total == r1.kkt_iters_total
