"""Resident batches (cj.BatchSolver): what a repeated solve costs besides its iterations, one JSON line per (batch, route) into
profiles/batch_resolve_rate.jsonl.

Batches of 256 members: the reference's portfolio example (n = 210, m = 211) over the risk aversion gamma (tests/test_gpu_batch_direct.py's builder), on
the CG batch kernels and on the direct batch (Settings.direct_batch), and cfg1-size QPs (problems.dense_qp(): n = 200, m = 300) on the CG batch kernels.
Every solve runs a fixed number of ADMM iterations (eps = 0, no certificates).  Recorded:
  first_setup_s      the first BatchSolver.optimize's set-up (host Ruiz scaling, CSR conversion, images, uploads; analysis + factorisations if direct);
  stage_s            cj.update(model, q=...) of every member (host: checks, the model's scaled mirror, staging);
  apply_s            cosmo_hip_batch_apply_updates: one copy of upload_bytes and one launch of k_batch_update_qb;
  restart_s          cosmo_hip_batch_warm_restart: one launch of k_batch_warm_restart plus the control-state reset;
  resolve_overhead_s stage + apply + restart, i.e. the re-solve's cost outside its iterations;
  optimize_s         the re-solve's optimize (the iterations themselves, for scale);
  optimize_batch_setup_s  cj.optimize_batch on the same models, which rebuilds the device batch on every call (its set-up, LAST_BATCH_INFO).
Usage: python tools/batch_resolve_rate.py [--iters 200] [--count 256] [--resolves 5] [--out profiles/batch_resolve_rate.jsonl]"""
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
from tools.batch_direct_rate import cfg1_batch  # noqa: E402


def run(name, probs, route, iters, resolves):
    kw = dict(max_iter=iters, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9)
    st = cj.Settings(kkt_solver=cj.QdldlKKTSolver, direct_batch=True, **kw) if route == "direct_batch" else cj.Settings(**kw)
    mods = []
    for p in probs:
        md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st); mods.append(md)
    rb = cj.BatchSolver(mods)
    rb.optimize()
    first = rb.last_times["setup_s"]
    rng = np.random.default_rng(0)
    stage, apply, restart, opt = [], [], [], []
    for _ in range(resolves):
        f = rng.uniform(0.5, 2.0)
        t0 = time.perf_counter()
        for md, p in zip(mods, probs):
            cj.update(md, q=f * p["q"])
        stage.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        rs = rb.optimize()
        opt.append(time.perf_counter() - t0 - rb.last_times["apply_s"] - rb.last_times["restart_s"])
        apply.append(rb.last_times["apply_s"]); restart.append(rb.last_times["restart_s"])
        assert max(r.iter for r in rs) == iters
    n, m = int(probs[0]["P"].shape[0]), int(probs[0]["A"].shape[0])
    isz = 8
    upload = (2 * 4 * len(probs) + 15) // 16 * 16 + len(probs) * (n + m) * isz
    rb.close()
    cj.optimize_batch(mods)
    ob_setup = cj.model.LAST_BATCH_INFO["setup_seconds"]
    med = lambda v: float(np.median(v))  # noqa: E731
    out = dict(batch=name, route=route, problems=len(probs), n=n, m=m, iters=iters, resolves=resolves, first_setup_s=round(first, 4),
               stage_s=round(med(stage), 5), apply_s=round(med(apply), 6), restart_s=round(med(restart), 6),
               resolve_overhead_s=round(med(stage) + med(apply) + med(restart), 5), device_overhead_s=round(med(apply) + med(restart), 6),
               upload_bytes=upload, optimize_s=round(med(opt), 4), optimize_batch_setup_s=round(ob_setup, 4),
               overhead_vs_first_setup=round((med(stage) + med(apply) + med(restart)) / first, 5))
    print(json.dumps(out), flush=True)
    return out


def _warm_models():
    out = []
    for p in portfolio_batch(2):
        md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], cj.Settings(max_iter=10)); out.append(md)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--resolves", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cj.optimize_batch(_warm_models())    # the process's HIP initialisation stays out of the first row
    rows = [run("portfolio", portfolio_batch(args.count), "cg_batch", args.iters, args.resolves),
            run("portfolio", portfolio_batch(args.count), "direct_batch", args.iters, args.resolves),
            run("cfg1", cfg1_batch(args.count), "cg_batch", args.iters, args.resolves)]
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
