"""Resident batches: what a re-solve costs OUTSIDE cosmo_hip_batch_optimize when the new q arrives from the host and the results return to it, against
the same re-solve fed from and read into device tensors.  One JSON line per batch into profiles/batch_device_io.jsonl.

Batches: the three 256-member batches of tools/batch_resolve_rate.py (portfolio on the CG batch kernels and on the direct batch, cfg1-size QPs) and
1024 members of the BASELINE config-3 structure (problems.socp(): n = 500, m = 1000).  ONE BatchSolver per batch; its re-solves alternate between the two
paths, so both see the same batch, the same process and the same minute of the machine.  Every solve runs a fixed number of ADMM iterations (eps = 0, no
certificates); the solve itself is outside both windows.  Each window is a host clock around calls that end in torch.cuda.synchronize():
  host path    in:  cj.update(model, q=) of every member, cosmo_hip_batch_apply_updates, cosmo_hip_batch_warm_restart
               out: model._write_back (4 device-to-host copies per member, unscaling in numpy, one Result per member) -- reported on its own as well
  device path  in:  BatchSolver.update_device(q=tensor) (k_batch_update_qb_dev), cosmo_hip_batch_warm_restart
               out: cosmo_hip_batch_get_solution_device into three preallocated tensors (k_batch_export_solution)
The new q of a device re-solve is made on the device before its window opens (the caller's pipeline is not the library's overhead).  Reported per path:
the median over the re-solves, the quartiles (spread = q75 - q25) and the extremes, in seconds.  `device_saves_s` is the difference of the medians and
`beyond_noise` says whether it exceeds three times the larger spread.
Usage: python tools/batch_device_io_rate.py [--iters 20] [--resolves 20] [--warmup 3] [--count 256] [--count3 1024] [--out profiles/batch_device_io.jsonl]"""
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


def _stats(v):
    v = np.asarray(v, dtype=np.float64)
    q25, med, q75 = np.percentile(v, [25, 50, 75])
    return dict(median_s=round(float(med), 7), q25_s=round(float(q25), 7), q75_s=round(float(q75), 7), spread_s=round(float(q75 - q25), 7),
                min_s=round(float(v.min()), 7), max_s=round(float(v.max()), 7))


def run(name, probs, route, iters, resolves, warmup):
    import torch
    kw = dict(max_iter=iters, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9)
    st = cj.Settings(kkt_solver=cj.QdldlKKTSolver, direct_batch=True, **kw) if route == "direct_batch" else cj.Settings(**kw)
    mods = []
    for p in probs:
        md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st); mods.append(md)
    nprob, n, m = len(mods), mods[0].n, mods[0].m
    sync = torch.cuda.synchronize
    with cj.BatchSolver(mods) as rb:
        rb.optimize()
        assert not rb.mixed
        B = rb.batch
        q0 = np.stack([p["q"] for p in probs])
        q0_dev = torch.from_numpy(q0).to("cuda:0")
        x = torch.empty((nprob, n), dtype=torch.float64, device="cuda:0"); y = torch.empty((nprob, m), dtype=torch.float64, device="cuda:0")
        s = torch.empty_like(y)
        rng = np.random.default_rng(0)
        t = dict(host_in=[], host_out=[], dev_in=[], dev_out=[], optimize=[])
        for it in range(2 * (warmup + resolves)):
            f = float(rng.uniform(0.5, 2.0))
            keep = it >= 2 * warmup
            if it % 2 == 0:                                              # host path
                sync(); t0 = time.perf_counter()
                for md, p in zip(mods, probs):
                    cj.update(md, q=f * p["q"])
                B.apply_updates(); B.warm_restart()
                sync(); t1 = time.perf_counter()
                rs = B.optimize()
                sync(); t2 = time.perf_counter()
                out = cj.model._write_back(mods, B, rs, rb._st, False, t2, 0.0)
                sync(); t3 = time.perf_counter()
                assert len(out) == nprob
                if keep:
                    t["host_in"].append(t1 - t0); t["host_out"].append(t3 - t2); t["optimize"].append(t2 - t1)
            else:                                                        # device path
                q_dev = q0_dev * f
                sync(); t0 = time.perf_counter()
                rb.update_device(q=q_dev)
                B.warm_restart()
                sync(); t1 = time.perf_counter()
                rs = B.optimize()
                sync(); t2 = time.perf_counter()
                B.get_solution_device(x=x, s=s, y=y)
                sync(); t3 = time.perf_counter()
                if keep:
                    t["dev_in"].append(t1 - t0); t["dev_out"].append(t3 - t2); t["optimize"].append(t2 - t1)
            assert max(r.iter for r in rs) == iters
        # both paths end in the same solution of the last device re-solve: the export against the write-back of that very state
        out = cj.model._write_back(mods, B, rs, rb._st, False, 0.0, 0.0)
        assert np.array_equal(x.cpu().numpy(), np.stack([r.x for r in out])) and np.array_equal(y.cpu().numpy(), np.stack([r.y for r in out]))
    host = _stats(np.add(t["host_in"], t["host_out"])); dev = _stats(np.add(t["dev_in"], t["dev_out"]))
    saves = host["median_s"] - dev["median_s"]
    noise = 3.0 * max(host["spread_s"], dev["spread_s"])
    row = dict(batch=name, route=route, problems=nprob, n=n, m=m, iters=iters, resolves_per_path=resolves, warmup_per_path=warmup,
               host_overhead=host, host_in=_stats(t["host_in"]), host_write_back=_stats(t["host_out"]),
               device_overhead=dev, device_in=_stats(t["dev_in"]), device_out=_stats(t["dev_out"]),
               optimize_median_s=round(float(np.median(t["optimize"])), 6), device_saves_s=round(saves, 7), three_spreads_s=round(noise, 7),
               beyond_noise=bool(saves > noise))
    print(json.dumps(row), flush=True)
    return row


def _warm_models():
    out = []
    for p in portfolio_batch(2):
        md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], cj.Settings(max_iter=10)); out.append(md)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--resolves", type=int, default=20, help="timed re-solves per path (at least 20 for a committed figure)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed re-solves per path")
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--count3", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cj.optimize_batch(_warm_models())    # the process's HIP initialisation stays out of the first row
    a = (args.iters, args.resolves, args.warmup)
    rows = []
    for name, build, route in (("portfolio", lambda: portfolio_batch(args.count), "cg_batch"), ("portfolio", lambda: portfolio_batch(args.count), "direct_batch"),
                               ("cfg1", lambda: cfg1_batch(args.count), "cg_batch"),
                               ("cfg3", lambda: [cj.problems.socp(seed=1000 + k) for k in range(args.count3)], "cg_batch")):
        rows.append(run(name, build(), route, *a))
        if args.out:                                                     # (row by row: a later batch that fails keeps the earlier figures)
            with open(args.out, "w") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
