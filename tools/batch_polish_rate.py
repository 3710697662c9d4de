"""Polishing in batch mode (Settings.polish, csrc/batch_polish.hip): what it costs and what it buys.  One JSON line per measurement.

Batches: 256 members of the polish fixture (tests/polish_cases.py: n = 30, m = 32, known solutions) and the reference's portfolio example over 256 values
of the risk aversion (tests/test_gpu_batch_direct.py: n = 210, m = 211), each with the CG batch kernels and with the direct batch.
  cost      cosmo_hip_batch_polish alone behind a default solve (eps = 1e-5): the first call (plan for a CG batch, slabs, vectors) and the median of
            --reps further calls (every call does the same work whether its candidate is accepted or not), against one ADMM iteration of the same
            batch (a second batch run for --iters iterations at eps = 0).  Host clock around calls that end in a stream synchronise.
  accuracy  solve (eps = 1e-5) + polish against solves alone at eps = 1e-7, 1e-9, 1e-11: seconds of optimize (+ polish) on a batch that is already set
            up, and the worst error in x against the reference (over all members, and over the members whose polish was accepted) -- the fixture's constructed x*,
            for the portfolio a direct-batch solve at eps = 1e-12.
  kernel    registers / scratch / LDS of k_batch_polish are compile-time figures (hipcc -Rpass-analysis=kernel-resource-usage).
Usage: python tools/batch_polish_rate.py [--count 256] [--reps 20] [--iters 200] [--only fixture|portfolio] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cosmo_jl_amd as cj  # noqa: E402
from tests import polish_cases as PC  # noqa: E402
from tests.test_gpu_batch_direct import portfolio_batch  # noqa: E402

ROUTES = {"cg": dict(), "direct": dict(kkt_solver=cj.QdldlKKTSolver, direct_batch=True)}


def fixture_batch(count):
    members = PC.batch(seeds=tuple(range(count)))
    return [dict(P=c["P_csc"], q=c["q"], A=c["A_csc"], b=c["b"], sets=PC.cone_sets(c, cj), x=c["x"]) for c in members]


def models(probs, st):
    out = []
    for p in probs:
        md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st); out.append(md)
    return out


def solutions(B, mods):
    return np.stack([md.sm.D * B.get_iterates(k)[1][:md.n] for k, md in enumerate(mods)])


def cost(name, probs, route, reps, iters):
    mods = models(probs, cj.Settings(**ROUTES[route]))
    B, _ = cj.model.prepare_batch(mods, 0)
    t0 = time.perf_counter(); rs = B.optimize(); t_opt = time.perf_counter() - t0
    t0 = time.perf_counter(); B.polish(1e-6, 3); first = time.perf_counter() - t0
    status = B.polish_info()["status"]
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); B.polish(1e-6, 3); ts.append(time.perf_counter() - t0)
    B.close()
    kw = dict(max_iter=iters, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9)
    B2, _ = cj.model.prepare_batch(models(probs, cj.Settings(**ROUTES[route], **kw)), 0)
    t0 = time.perf_counter(); r2 = B2.optimize(); t_it = (time.perf_counter() - t0) / max(max(r.iter for r in r2), 1)
    form = B2.kernel_info()["form"]
    B2.close()
    med = float(np.median(ts))
    return dict(measure="cost", batch=name, route=route, problems=len(probs), n=int(mods[0].n), m=int(mods[0].m), admm_kernel=form,
                solve_iters_max=int(max(r.iter for r in rs)), solve_s=round(t_opt, 5), polish_first_call_ms=round(1e3 * first, 3),
                polish_ms=round(1e3 * med, 4), polish_ms_min=round(1e3 * min(ts), 4), polish_ms_max=round(1e3 * max(ts), 4),
                admm_iter_us=round(1e6 * t_it, 2), polish_in_admm_iters=round(med / t_it, 1), accepted=int(np.sum(status == 1)), rejected=int(np.sum(status == -1)))


def accuracy(name, probs, route, ref):
    rows = []
    for label, eps, polish in (("1e-5+polish", 1e-5, True), ("1e-5", 1e-5, False), ("1e-7", 1e-7, False), ("1e-9", 1e-9, False), ("1e-11", 1e-11, False)):
        mods = models(probs, cj.Settings(eps_abs=eps, eps_rel=eps, max_iter=100000, **ROUTES[route]))
        B, _ = cj.model.prepare_batch(mods, 0)
        if polish:                                           # (the first polish call allocates: take it out of the timed window with a throw-away batch state)
            B.optimize(); B.polish(1e-6, 3)
            B.set_iterates(None, None, None)
        t0 = time.perf_counter()
        rs = B.optimize()
        if polish:
            B.polish(1e-6, 3)
        dt = time.perf_counter() - t0
        x = solutions(B, mods)
        ok = B.polish_info()["status"] == 1 if polish else np.zeros(len(mods), bool)
        acc = int(np.sum(ok))
        B.close()
        rows.append(dict(measure="accuracy", batch=name, route=route, leg=label, seconds=round(dt, 5), iters_max=int(max(r.iter for r in rs)),
                         solved=int(sum(cj._ffi.STATUS_NAMES[r.status] == "Solved" for r in rs)), accepted=acc,
                         worst_x_error=float(np.max(np.abs(x - ref))),
                         worst_x_error_accepted=float(np.max(np.abs(x - ref)[ok])) if acc else None))
    return rows


def reference(probs, name):
    if name == "fixture":
        return np.stack([p["x"] for p in probs])
    mods = models(probs, cj.Settings(eps_abs=1e-12, eps_rel=1e-12, max_iter=200000, **ROUTES["direct"]))
    B, _ = cj.model.prepare_batch(mods, 0)
    B.optimize()
    x = solutions(B, mods)
    B.close()
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "tools/batch_polish_rate.py measures on the MI355X"
    rows = []
    for name in ("fixture", "portfolio"):
        if args.only and args.only != name:
            continue
        probs = fixture_batch(args.count) if name == "fixture" else portfolio_batch(args.count)
        ref = reference(probs, name)
        for route in ROUTES:
            cost(name, probs, route, 2, 20)                                   # warm-up: code objects, allocator
            rows.append(cost(name, probs, route, args.reps, args.iters)); print(json.dumps(rows[-1]), flush=True)
            for r in accuracy(name, probs, route, ref):
                rows.append(r); print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
