"""The heads of the latency-bound Krylov kernels (csrc/device_utils.h: partials_request / partials_fold, pin_args, CtlHead; profiles/krylov_heads.txt):
branch-free loads of the reduction partials from a clamped index, one batch of kernel arguments, one batch of control-block words.  No expression
changed, so the results are held to the BITS of the parent build (tests/golden/krylov_heads_parent.json, written on the GPU from the parent commit by
tests/golden/make_fixtures_krylov_heads.py) and, independently, to the oracle at the tolerances of tests/test_gpu_cg_fold.py.

The sizes put the number of partials a Krylov kernel folds (ceil(n / 256), at most 2048) at 1, 2, 255, 256, 257, 2048 and the capped grid: every count at
which a thread's eight clamped loads change between "own slot", "slot 0, masked" and "all eight slots".  Three routes per size: the assembled operator
(k_cg_dirM + k_cg_upd), the dense rows kept factored (k_cg_dirMs + k_cg_updF on the pre-scattered image) and the unassembled operator (k_cg_dirA /
k_cg_dir + k_op_apply + k_cg_upd)."""
import hashlib
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from oracle import cosmo_oracle as O
from tests import util

pytestmark = pytest.mark.gpu

NS = (200, 257, 65280, 65536, 65537, 524288, 524289)
ROUTES = {
    "assembled": {"COSMO_HIP_OP_FOLD": "1", "COSMO_HIP_FOLD_FACTOR": "0"},
    "factored": {"COSMO_HIP_OP_FOLD": "1", "COSMO_HIP_FOLD_FACTOR": "1"},
    "unassembled": {"COSMO_HIP_OP_FOLD": "0"},
}
ITERS = 3
NDENSE = 8                                                               # coupling rows of 6 nonzeros each (>= 4: the rows the factored route keeps)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "krylov_heads_parent.json")


def heads_qp(n):
    """Box-constrained QP: tridiagonal diagonally dominant P (a few dozen Krylov iterations at 1e-10), bounds on every variable (the single-nonzero rows
    of A) and NDENSE coupling rows of 6 nonzeros."""
    rng = np.random.default_rng(1000 + n)
    off = -0.5 * rng.uniform(0.5, 1.0, n - 1)
    P = sp.diags([off, 2.0 + rng.uniform(0.0, 1.0, n), off], [-1, 0, 1], format="csc")
    P.sort_indices()
    rows = np.repeat(np.arange(NDENSE), 6)
    cols = np.concatenate([rng.choice(n, 6, replace=False) for _ in range(NDENSE)])
    G = sp.csc_matrix((rng.standard_normal(6 * NDENSE), (rows, cols)), shape=(NDENSE, n))
    x0 = rng.standard_normal(n)
    A = sp.vstack([-sp.eye(n), -G], format="csc"); A.sort_indices()
    lo = np.concatenate([x0 - np.abs(rng.standard_normal(n)), G @ x0 - 0.1])
    hi = np.concatenate([x0 + np.abs(rng.standard_normal(n)), G @ x0 + 0.1])
    return dict(P=P, q=rng.standard_normal(n), A=A, b=np.zeros(n + NDENSE), sets=[cj.Box(lo, hi)])


def settings():
    return cj.Settings(max_iter=ITERS, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9,
                       kkt_solver=cj.with_options(cj.CGIndirectKKTSolver, tol_constant=1e-10, tol_exponent=0.0))


def run_case(route, n, prob, setenv):
    """-> (x, Krylov iterations of the run, fold_stats); setenv(name, value) sets the route's switches for the set-up."""
    for k in ("COSMO_HIP_OP_FOLD", "COSMO_HIP_FOLD_FACTOR"):
        setenv(k, ROUTES[route].get(k, "0"))
    md = cj.Model(); md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], settings())
    r = cj.optimize(md)
    fs = md.handle.fold_stats()
    assert r.iter == ITERS
    return np.ascontiguousarray(r.x, dtype=np.float64), int(r.kkt_iters_total), fs


def x_hash(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype=np.float64).tobytes()).hexdigest()


_CACHE = {}


def _problem_and_reference(n):
    """The problem and the oracle's run, computed once per size and shared by the three routes (never modified)."""
    if n not in _CACHE:
        prob = heads_qp(n)
        ref = O.solve(prob["P"], prob["q"], prob["A"], prob["b"], util.oracle_cones(prob["sets"]),
                      O.Settings(max_iter=ITERS, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9, kkt_solver="cg", tol_constant=1e-10, tol_exponent=0.0))
        _CACHE[n] = (prob, np.asarray(ref.x, dtype=np.float64), int(np.sum(ref.cg_iters)), int(ref.iter))
    return _CACHE[n]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_krylov_heads_against_the_oracle_and_the_parents_bits(route, n, monkeypatch):
    prob, x_ref, k_ref, it_ref = _problem_and_reference(n)
    x, kkt, fs = run_case(route, n, prob, monkeypatch.setenv)
    # the route really ran
    if route == "unassembled":
        assert fs["enabled"] == 0, fs
    else:
        assert fs["enabled"] == 1 and fs["factored_rows"] == (NDENSE if route == "factored" else 0), fs
    print("%s n=%d: Krylov %d (oracle %d), max |x - x_ref| = %.3e, max |x_ref| = %.3e" % (route, n, kkt, k_ref, float(np.max(np.abs(x - x_ref))), float(np.max(np.abs(x_ref)))))
    # the oracle, at the tolerances of tests/test_gpu_cg_fold.py: 1e-7 trajectories, +-1 Krylov iteration per solve
    assert it_ref == ITERS
    assert np.max(np.abs(x - x_ref)) <= 1e-7 * max(1.0, float(np.max(np.abs(x_ref))))
    assert abs(kkt - k_ref) <= ITERS + 1, (kkt, k_ref)
    # the parent build, bit for bit
    with open(GOLDEN) as f:
        gold = json.load(f)["cases"]["%s-%d" % (route, n)]
    assert kkt == gold["kkt_iters"], (kkt, gold["kkt_iters"])
    assert x_hash(x) == gold["x_sha256"]
