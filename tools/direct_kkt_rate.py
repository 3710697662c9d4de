"""Direct KKT solver (kkt_kind KKT_DIRECT, csrc/ldl.hip) on BASELINE config 5 (problems.chordal_sdp()) and config 1 (problems.dense_qp()).

Per problem: host analysis seconds (cosmo_hip_ldl_analyze on the pattern), nnz(L), supernodes, tree height, widest supernode, the setup
factorisation and one refactorisation (update_rho with a new rho vector) in ms, us per fine-grained kkt_solve call (host copies of the
(n+m)-vectors included), and ADMM it/s of optimize() with Settings(kkt_solver=QdldlKKTSolver) over a fixed iteration count.
Usage: python tools/direct_kkt_rate.py [--iters 50] [--only cfg1|cfg5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cosmo_jl_amd as cj  # noqa: E402


def measure(name, p, iters):
    t0 = time.perf_counter()
    a = cj._ffi.ldl_analyze(p["A"].shape[1], p["A"].shape[0], p["P"], p["A"])
    t_an = time.perf_counter() - t0
    md = cj.Model()
    md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], cj.Settings(kkt_solver=cj.QdldlKKTSolver, max_iter=iters, eps_abs=0.0, eps_rel=0.0,
                                                               check_infeasibility=10 ** 9))
    t0 = time.perf_counter()
    res = cj.optimize(md)
    t_opt = time.perf_counter() - t0
    h = md.handle
    info0 = h.direct_info()
    factor_ms = info0["last_factor_ns"] * 1e-6
    n, m = h.n, h.m
    rng = np.random.default_rng(0)
    rhs = rng.standard_normal(n + m)
    h.kkt_solve(rhs)
    reps = 10
    t0 = time.perf_counter()
    for _ in range(reps):
        h.kkt_solve(rhs)
    us_solve = (time.perf_counter() - t0) / reps * 1e6
    h.update_rho(rng.uniform(0.05, 2.0, m))
    refactor_ms = h.direct_info()["last_factor_ns"] * 1e-6
    out = dict(problem=name, n=int(n), m=int(m), analysis_s=round(t_an, 3), nnz_L=info0["nnz_L"], supernodes=info0["supernodes"],
               height=info0["height"], max_width=info0["max_width"], factor_ms=round(factor_ms, 3), refactor_ms=round(refactor_ms, 3),
               us_per_kkt_solve_call=round(us_solve, 1), admm_iters=int(res.iter), iter_time_s=round(res.times.iter_time, 4),
               it_per_s=round(res.iter / res.times.iter_time, 2) if res.times.iter_time > 0 else None, setup_s=round(res.times.setup_time, 3),
               optimize_wall_s=round(t_opt, 3), factorizations=h.direct_info()["factorizations"], status=res.status,
               analysis_pairs=a["update_pairs"])
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    for name, gen in (("cfg1", cj.problems.dense_qp), ("cfg5", cj.problems.chordal_sdp)):
        if args.only and args.only != name:
            continue
        measure(name, gen(), args.iters)


if __name__ == "__main__":
    main()
