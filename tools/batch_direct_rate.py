"""QdldlKKTSolver in batch mode: three routes on two batches, one JSON line per (batch, route) into profiles/batch_direct_rate.jsonl.

Batches: the reference's portfolio example (examples/portfolio_optimisation.jl, n = 210, m = 211) over 256 values of the risk aversion gamma (as
tests/test_gpu_batch_direct.py builds it), and cfg1-size QPs of one pattern (problems.dense_qp(): n = 200, m = 300, dense P) with redrawn q.
Routes:
  direct_batch  Settings(kkt_solver=QdldlKKTSolver, direct_batch=True): one union analysis, one LDL' per member inside its persistent workgroup;
  own_handles   Settings(kkt_solver=QdldlKKTSolver): the batch group gives every member its own single-problem DIRECT handle (analysis + factor each);
  cg_batch      Settings(): the CG batch kernels.
Each route runs a fixed number of ADMM iterations (eps = 0, no certificates).  Recorded: set-up seconds (scaling, upload, analysis, set-up
factorisation), the analysis seconds where the route reports them, the factorisations, and the per-iteration time of the whole batch.  The
own-handle route on cfg1 runs --own-cfg1 members only (its host analysis is ~1.6 s per member); its per-member set-up is reported too.
Usage: python tools/batch_direct_rate.py [--iters 200] [--count 256] [--own-cfg1 32] [--out profiles/batch_direct_rate.jsonl] [--only portfolio|cfg1]
       [--route direct_batch] (one route, for a kernel trace)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cosmo_jl_amd as cj  # noqa: E402
from tests.test_gpu_batch_direct import portfolio_batch  # noqa: E402


def cfg1_batch(count):
    p = cj.problems.dense_qp()
    rng = np.random.default_rng(3)
    return [dict(p, q=p["q"] + 0.1 * rng.standard_normal(p["q"].size)) for _ in range(count)]


def run(name, probs, route, iters):
    kw = dict(max_iter=iters, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9)
    st = {"direct_batch": cj.Settings(kkt_solver=cj.QdldlKKTSolver, direct_batch=True, **kw),
          "own_handles": cj.Settings(kkt_solver=cj.QdldlKKTSolver, **kw), "cg_batch": cj.Settings(**kw)}[route]
    mods = []
    for p in probs:
        md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st); mods.append(md)
    t0 = time.perf_counter()
    B, _ = cj.model.prepare_batch_group(mods, 0) if route == "own_handles" else cj.model.prepare_batch(mods, 0)
    t_setup = time.perf_counter() - t0
    t0 = time.perf_counter()
    rs = B.optimize()
    t_opt = time.perf_counter() - t0
    out = dict(batch=name, route=route, problems=len(probs), n=int(probs[0]["P"].shape[0]), m=int(probs[0]["A"].shape[0]), setup_s=round(t_setup, 4),
               setup_per_member_ms=round(1e3 * t_setup / len(probs), 3), iters=int(max(r.iter for r in rs)), optimize_s=round(t_opt, 4),
               us_per_batch_iter=round(1e6 * t_opt / max(max(r.iter for r in rs), 1), 1))
    if route == "direct_batch":
        di = B.direct_info()
        out.update(analysis_s=round(di["analysis_ns"] * 1e-9, 4), factorizations=di["factorizations"], nnz_L=di["nnz_L"], panel_size=di["panel_size"],
                   supernodes=di["supernodes"], height=di["height"], max_width=di["max_width"])
    elif route == "own_handles":
        nc, _, modes = B.class_info(with_modes=True)
        out.update(own_handle_members=int(np.sum(modes == 1)))
    B.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--own-cfg1", type=int, default=32)
    ap.add_argument("--only", default=None)
    ap.add_argument("--route", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for name in ("portfolio", "cfg1"):
        if args.only and args.only != name:
            continue
        for route in ("direct_batch", "own_handles", "cg_batch"):
            if args.route and args.route != route:
                continue
            count = args.own_cfg1 if (name == "cfg1" and route == "own_handles") else args.count
            probs = portfolio_batch(count) if name == "portfolio" else cfg1_batch(count)
            rows.append(run(name, probs, route, args.iters))
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
