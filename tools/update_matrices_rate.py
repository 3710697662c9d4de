"""Time of cosmo_hip_update_matrices against what a user had to do before it existed: destroy the handle and set it up again.

    python tools/update_matrices_rate.py [--out profiles/update_matrices_rate.jsonl] [--runs 20] [--warmup 3]

Per problem and route, after `warmup` untimed repetitions, the median of `runs` repetitions of
  update : update_matrices(P values, A values)            -- upload + copy refresh + operator refresh (+ refactorisation where DIRECT)
  fresh  : close(); Handle(); set_problem; set_cones; set_params; set_scaling_full on the same data
each bracketed by a device synchronisation (torch.cuda.synchronize() = hipDeviceSynchronize), plus the bytes the value maps hold on the device
(update_matrices_info) next to the expectation 4 * (2 nnz(A) + 2 nnz(P) + nnz(Am) + nnz(PTm) + 2 terms).  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cosmo_jl_amd as cj  # noqa: E402
from cosmo_jl_amd import _ffi  # noqa: E402


def portfolio():
    """the portfolio problem of tests/test_gpu_batch_resident.py (200 assets, 10 factors), one value of gamma"""
    n_assets, k = 200, 10
    rng = np.random.default_rng(1)
    Dd = rng.uniform(size=n_assets) * np.sqrt(k)
    F = sp.random(n_assets, k, density=0.5, random_state=rng, data_rvs=rng.standard_normal).tocsc()
    mu = (3.0 + 9.0 * rng.uniform(size=n_assets)) / 100.0
    P = sp.block_diag([2.0 * sp.diags(Dd), 2.0 * sp.identity(k)]).tocsc()
    A = sp.vstack([sp.hstack([F.T, -sp.identity(k)]), sp.hstack([sp.csr_matrix(np.ones((1, n_assets))), sp.csr_matrix((1, k))]),
                   sp.hstack([-sp.identity(n_assets), sp.csr_matrix((n_assets, k))])]).tocsc()
    b = np.concatenate([np.zeros(k), [1.0], np.zeros(n_assets)])
    return dict(P=P, q=np.concatenate([-mu, np.zeros(k)]), A=A, b=b, sets=[cj.ZeroSet(k + 1), cj.Nonnegatives(n_assets)])


def setup(pr, kind):
    h = cj.Handle(0)
    h.set_problem(pr["P"], pr["q"], pr["A"], pr["b"])
    bl = np.concatenate([K.l for K in pr["sets"] if K.kind == _ffi.BOX] or [np.zeros(0)])
    bu = np.concatenate([K.u for K in pr["sets"] if K.kind == _ffi.BOX] or [np.zeros(0)])
    h.set_cones([K.kind for K in pr["sets"]], [K.dim for K in pr["sets"]], bl, bu, cone_param=[getattr(K, "alpha", 0.0) for K in pr["sets"]])
    p = h.default_params()
    p.kkt_kind = kind
    h.set_params(p)
    n, m = h.n, h.m
    h.set_scaling_full(np.ones(n), np.ones(n), np.ones(m), np.ones(m), 1.0, 1.0)
    return h


def measure(name, pr, kind, kind_name, runs, warmup):
    import torch
    sync = torch.cuda.synchronize
    P = sp.csc_matrix(pr["P"]); P.sort_indices()
    A = sp.csc_matrix(pr["A"]); A.sort_indices()
    pr = dict(pr, P=P, A=A)
    rng = np.random.default_rng(0)
    h = setup(pr, kind)
    t_upd, t_fresh = [], []
    for k in range(warmup + runs):
        g = rng.uniform(0.95, 1.05, P.shape[0])                    # G P G: the same pattern, still PSD
        cols = np.repeat(np.arange(P.shape[1]), np.diff(P.indptr))
        pv = P.data * (g[P.indices] * g[cols]); av = A.data * rng.uniform(0.95, 1.05, A.nnz)
        sync(); t0 = time.perf_counter()
        h.update_matrices(pv if P.nnz else None, av)
        sync(); t1 = time.perf_counter()
        if k >= warmup:
            t_upd.append(t1 - t0)
    info = h.update_matrices_info()
    route = h.kkt_recurrence()
    # the expectation for the maps: 4 bytes x (2 nnz(A) + 2 nnz(P) + nnz(Am) + nnz([P | Am']) + 2 terms); the split / assembled parts only where the route has them
    lens = np.diff(A.tocsr().indptr)
    split = info["refreshed_arrays"] > 0
    nnz_am = int(np.sum(lens[lens >= 2])) if split else 0
    nnz_ptm = int(P.nnz) + nnz_am if split else 0
    terms = h.fold_stats()["terms"] if split else 0
    expect = 4 * (2 * A.nnz + 2 * P.nnz + nnz_am + nnz_ptm + 2 * terms)
    for k in range(warmup + runs):
        sync(); t0 = time.perf_counter()
        h.close()
        h = setup(pr, kind)
        sync(); t1 = time.perf_counter()
        if k >= warmup:
            t_fresh.append(t1 - t0)
    h.close()
    u, f = statistics.median(t_upd), statistics.median(t_fresh)
    return dict(problem=name, kkt=kind_name, route=route, n=int(P.shape[0]), m=int(A.shape[0]), nnz_P=int(P.nnz), nnz_A=int(A.nnz), runs=runs, warmup=warmup,
                update_ms=1e3 * u, update_min_ms=1e3 * min(t_upd), update_max_ms=1e3 * max(t_upd), fresh_setup_ms=1e3 * f, fresh_min_ms=1e3 * min(t_fresh),
                fresh_max_ms=1e3 * max(t_fresh), ratio_fresh_over_update=f / u, map_bytes=info["map_bytes"], map_bytes_expected_at_most=int(expect), bytes_uploaded_last=info["bytes_uploaded"],
                refreshed_arrays_per_update=info["refreshed_arrays"] // max(info["updates"], 1), host_rebuilds=info["host_rebuilds"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_matrices_rate.jsonl"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-config5", action="store_true")
    a = ap.parse_args()
    jobs = [("config 1 (dense QP)", cj.problems.dense_qp, _ffi.KKT_DIRECT, "DIRECT"), ("config 1 (dense QP)", cj.problems.dense_qp, _ffi.KKT_CG, "CG"),
            ("portfolio (200 assets, 10 factors)", portfolio, _ffi.KKT_CG, "CG"), ("portfolio (200 assets, 10 factors)", portfolio, _ffi.KKT_DIRECT, "DIRECT")]
    if not a.skip_config5:
        jobs.append(("config 5 (chordal SDP)", cj.problems.chordal_sdp, _ffi.KKT_CG, "CG"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for name, make, kind, kind_name in jobs:
            rec = measure(name, make(), kind, kind_name, a.runs, a.warmup)
            f.write(json.dumps(rec) + "\n"); f.flush()
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
