"""The numeric kernels of the direct KKT solver (csrc/ldl.hip, csrc/ldl_dev.h; in the batch kernels csrc/batch_ldl.h) on structures that drive their
loops past the first trip: supernodes wider and taller than the workgroup, thousands of descendants, thousands of levels, one level of 600 000
workgroups, vectors longer than the capped element-wise grids, missing diagonals, P = 0, m = 0, empty lines -- in Float64 and Float32.

tests/ldl_structures.py holds the structures, the NumPy reference factorisation and the derived componentwise backward-error bound (the only
tolerance of the unit tests here, with cond_est times it for the forward check); tests/test_ldl_structures_host.py proves on the CPU that every
structure reaches the loop it is named for, that the bound holds for the reference alone and that it catches three emulated kernel faults.
The loop / batch tests at the end reuse, unchanged, the bars of test_gpu_direct_kkt.py::test_model_level_random_qp_against_the_oracle (the
model-level form of test_loop_equals_the_oracles_direct_path) and of
test_gpu_batch_direct.py::test_same_pattern_batch_against_the_oracles_direct_path_and_the_single_handle.

Every case is one call sequence on one handle, under a watchdog that ends the process if the case takes longer than CASE_LIMIT_S."""
import faulthandler
import time

import numpy as np
import pytest

import cosmo_jl_amd as cj
from oracle import cosmo_oracle as O
from tests import ldl_structures as S

pytestmark = pytest.mark.gpu

CASE_LIMIT_S = 300
DTYPES = [np.float64, np.float32]


@pytest.fixture(autouse=True)
def _case_time_limit():
    """a case that hangs (on the device or anywhere else) takes the whole process down after CASE_LIMIT_S instead of holding the GPU: nothing runs
    after a hang"""
    faulthandler.dump_traceback_later(CASE_LIMIT_S, exit=True)
    t0 = time.perf_counter()
    yield
    faulthandler.cancel_dump_traceback_later()
    print("[case wall time %.1f s]" % (time.perf_counter() - t0))


def _handle(st, dtype, perm, rho):
    """as test_gpu_direct_kkt.py builds its handles: scaling off, KKT_DIRECT; the rows are one Nonnegatives cone and rho is handed over explicitly
    (its equality rows carry the 1e3 times larger value), so that kkt_solve is the unit under test"""
    h = cj.Handle(0, dtype=dtype)
    h.set_problem(st.P, np.zeros(st.n), st.A, np.zeros(st.m))
    if perm is not None:
        h.set_kkt_perm(perm)
    if st.m:
        h.set_cones([cj._ffi.NONNEG], [st.m])
    else:
        h.set_cones([], [])
    p = h.default_params()
    p.kkt_kind = cj._ffi.KKT_DIRECT
    p.sigma = S.SIGMA
    h.set_params(p, rho_vec=np.asarray(rho, dtype=dtype))
    assert h.kkt_recurrence().startswith("direct")
    return h


def _check_solves(h, st, ref, dtype, label, forward):
    for rname, rhs in S.rhs_pair(st, ref.perm, dtype):
        x, _ = h.kkt_solve(rhs)
        assert x.dtype == np.dtype(dtype)
        again, _ = h.kkt_solve(rhs)
        assert np.array_equal(x, again), (label, rname)                       # 3. same right-hand side, same factor: bitwise identical
        assert np.isfinite(x).all(), (label, rname)
        bad, worst = ref.violations(x, rhs)                                   # 2. (index, |r_i|, bound_i) of the worst violations
        print("%s %s %s %s: W = %d, worst |r_i| / bound_i = %.3g" % (st.name, np.dtype(dtype).name, label, rname, ref.W, worst))
        assert not bad, (label, rname, bad)
        if forward:
            err, lim = ref.forward_check(x, rhs)
            print("    forward: ||x - x_ref||_inf = %.3g <= %.3g" % (err, lim))
            assert err <= lim, (label, rname, err, lim)


def _check_info(h, st, perm, factorizations):
    want = cj._ffi.ldl_analyze(st.n, st.m, st.P, st.A, perm)                  # 1. the analysis on the host, same pattern and permutation
    info = h.direct_info()
    assert {k: info[k] for k in ("nnz_L", "supernodes", "height", "max_width")} == {k: want[k] for k in ("nnz_L", "supernodes", "height", "max_width")}
    assert info["positive_pivots"] == st.n                                    # the inertia, summed over the workgroups of every level by atomicAdd
    assert info["factorizations"] == factorizations
    return info


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(S.CASES))
def test_factor_and_solve_satisfy_the_backward_error_bound(name, dtype):
    """Which loop of the kernels each structure drives past its first trip: the table in tests/ldl_structures.py (asserted structure by structure in
    tests/test_ldl_structures_host.py::test_row_*)."""
    st = S.structure(name)
    perm = S.analysis_perm(st)
    order, _ = S.library_order(st, perm)
    forward = name in S.WELL_CONDITIONED
    rho = S.rho_vector(st, 1)
    h = _handle(st, dtype, perm, rho)
    if st.m:
        assert np.array_equal(h.get_rho_vec(), rho.astype(dtype))
    info = _check_info(h, st, perm, 1)
    print("%s %s: set-up factorisation %.1f ms on the device" % (name, np.dtype(dtype).name, info["last_factor_ns"] / 1e6))
    _check_solves(h, st, S.Reference(st, rho, dtype, order), dtype, "setup", forward)
    if st.m:                                                                  # 4. a fresh non-uniform rho: update_rho refactorises
        rho2 = S.rho_vector(st, 2)
        h.update_rho(rho2.astype(dtype))
        _check_info(h, st, perm, 2)
        _check_solves(h, st, S.Reference(st, rho2, dtype, order), dtype, "update_rho", forward)
    h.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(S.BOTH_ORDERINGS))
def test_the_other_ordering_satisfies_the_bound_on_the_same_matrix(name, dtype):
    """5. identity and default ordering differ: the structure's own ordering runs in the test above, the other one here, against the same K.
    (default_ordering_large under the identity ordering is nearly dense at N = 3994 -- its NumPy reference alone takes over a minute; the same
    generator at N = 1592, default_ordering_medium, stands in for it.)"""
    st = S.structure(name)
    other = np.arange(st.N) if st.perm is None else None
    order, _ = S.library_order(st, other)
    rho = S.rho_vector(st, 1)
    h = _handle(st, dtype, other, rho)
    _check_info(h, st, other, 1)
    _check_solves(h, st, S.Reference(st, rho, dtype, order), dtype, "identity" if other is not None else "default", False)
    h.close()


# ---- in the loop and in the batch kernels ------------------------------------------------------------------------------------------------------
# (name, q scale, member): chosen on the CPU with the oracle so that the solve changes rho at least twice inside its 200 iterations AND so that the
# oracle itself moves by no more than 1e-11 (rho updates, iterates) when its pivoted sparse LU is replaced by ldl_structures.ldl_nopivot in the
# structure's ordering -- the bars below compare roundings of two solvers, and an instance must be conditioned well enough to carry them
# (tall_panel at q scale 1e6 is not: the NumPy no-pivot factor alone moves its second rho by 1.4e-9).
LOOP = [("dense_block_350", 100.0, 0), ("tall_panel_4_640", 1e3, 2)]


def _settings(p, **kw):
    return cj.Settings(kkt_solver=cj.with_options(cj.QdldlKKTSolver, perm=p["perm"]), max_iter=200, **kw)


def _model(p, **kw):
    md = cj.Model()
    md.set(p["P"], p["q"], p["A"], p["b"], [cj.Nonnegatives(p["A"].shape[0])], _settings(p, **kw))
    return md


def _oracle(p):
    return O.solve(p["P"], p["q"], p["A"], p["b"], [O.Nonnegatives(p["A"].shape[0])], O.Settings(kkt_solver="qdldl", max_iter=200))


@pytest.mark.parametrize("name,q_scale,member", LOOP, ids=[c[0] for c in LOOP])
def test_loop_on_a_wide_supernode_equals_the_oracles_direct_path(name, q_scale, member):
    """6. the cond = 1 refactorisation (ldl_skip, Ctl::rho_changed) on a supernode wider / taller than the workgroup"""
    p = S.loop_problem(name, member, q_scale)
    ref = _oracle(p)
    assert len(ref.rho_updates) >= 3, "this instance must refactorise inside the loop at least twice"
    md = _model(p)
    res = cj.optimize(md)
    assert res.status == ref.status and res.iter == ref.iter
    assert np.allclose(res.info.rho_updates, ref.rho_updates, rtol=1e-9, atol=0)
    for a, r in ((res.x, ref.x), (res.y, ref.y), (res.s, ref.s)):
        assert np.max(np.abs(a - r)) <= 1e-8 * max(np.max(np.abs(r)), 1.0)
    info = md.handle.direct_info()
    want = cj._ffi.ldl_analyze(md.n, md.m, p["P"], p["A"], p["perm"])
    assert info["max_width"] == want["max_width"] > S.BS and info["supernodes"] == want["supernodes"]
    assert info["factorizations"] == 1 + (len(ref.rho_updates) - 1) and info["positive_pivots"] == md.n


@pytest.mark.parametrize("name,q_scale,member", LOOP, ids=[c[0] for c in LOOP])
def test_batch_on_a_wide_supernode_equals_the_single_handle(name, q_scale, member):
    """7. eight members of one pattern with different values in the batch kernels (their own block size, their own refill, the same device functions)"""
    probs = [S.loop_problem(name, k, q_scale) for k in range(8)]
    res = cj.optimize_batch([_model(p, direct_batch=True) for p in probs])
    info = cj.model.LAST_BATCH_INFO
    assert not info["mixed"] and "direct_info" in info                      # the DIRECT form of the batch kernels ran, not own handles
    di = info["direct_info"]
    want = cj._ffi.ldl_analyze(probs[0]["P"].shape[0], probs[0]["A"].shape[0], probs[0]["P"], probs[0]["A"], probs[0]["perm"])
    assert di["max_width"] == want["max_width"] > S.BS and di["supernodes"] == want["supernodes"] and di["nnz_L"] == want["nnz_L"]
    assert di["min_positive_pivots"] == probs[0]["P"].shape[0]
    assert list(info["direct_counts"]) == [len(r.info.rho_updates) for r in res]      # the set-up factorisation + one per rho update of THAT member
    assert max(len(r.info.rho_updates) for r in res) >= 3
    for k, (p, r) in enumerate(zip(probs, res)):
        r1 = cj.optimize(_model(p))
        assert r.status == r1.status and r.iter == r1.iter, k
        for a, b in ((r.x, r1.x), (r.y, r1.y)):
            assert np.max(np.abs(a - b)) <= 1e-9 * max(np.max(np.abs(b)), 1.0), k
