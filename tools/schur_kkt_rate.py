"""Schur-complement KKT solver (kkt_kind KKT_SCHUR, csrc/schur.hip) on BASELINE config 5 (problems.chordal_sdp()) next to the default CG route.

Records: the plan figures (cosmo_hip_schur_analyze and its host seconds), the set-up wall time of optimize() (analysis, uploads and the first
factorisation), seconds per factorisation (a synchronous update_rho with a new vector, wall clock), us per fine-grained kkt_solve call (host copies of
the (n+m)-vectors included) with 0 and with the default 2 refinement steps, the residual ratios of cosmo_hip_schur_residual, and ADMM it/s in
iterations 11 .. 50 (two optimize() runs of 10 and 50 iterations, the difference of their loop times) -- alternating with the parent's default CG
route in the same session, `--rounds` times each (the project's convention: eight rounds; a difference counts above three standard deviations of the
CG rounds).  The split of a factorisation and of a solve into kernels is read from a kernel trace of this script (rocprofv3 --kernel-trace --stats).
Usage: python tools/schur_kkt_rate.py [--rounds 8] [--refine-steps 2] [--out profiles/schur_kkt_rate.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cosmo_jl_amd as cj  # noqa: E402


def loop_rate(p, kkt):
    """it/s over ADMM iterations 11 .. 50, and the handle of the 50-iteration run"""
    t, md = {}, None
    for iters in (10, 50):
        md = cj.Model()
        md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], cj.Settings(kkt_solver=kkt, max_iter=iters, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9))
        res = cj.optimize(md)
        t[iters] = (res.times.iter_time, res.times.setup_time, res.kkt_iters_total, res.iter, len(res.info.rho_updates))
    return 40.0 / (t[50][0] - t[10][0]), t, md


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--refine-steps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(obj):
        s = json.dumps(obj)
        print(s, flush=True)
        lines.append(s)
    p = cj.problems.chordal_sdp()
    m, n = p["A"].shape
    t0 = time.perf_counter()
    plan = cj._ffi.schur_analyze(n, m, p["P"], p["A"])
    say(dict(problem="cfg5", n=n, m=m, analysis_s=round(time.perf_counter() - t0, 3), plan=plan))
    schur = cj.with_options(cj.SchurComplementKKTSolver, refine_steps=args.refine_steps)
    rates = {"schur": [], "cg": []}
    md_schur = None
    for rnd in range(args.rounds):
        for name, kkt in (("cg", cj.CGIndirectKKTSolver), ("schur", schur)):
            r, t, md = loop_rate(p, kkt)
            rates[name].append(r)
            say(dict(round=rnd, route=name, it_per_s_11_50=round(r, 2), iter_time_50_s=round(t[50][0], 4), setup_s=round(t[50][1], 3), kkt_iters_total=t[50][2],
                     rho_updates=t[50][4], recurrence=md.handle.kkt_recurrence()))
            if name == "schur":
                md_schur = md
    for name in ("cg", "schur"):
        a = np.array(rates[name])
        say(dict(route=name, it_per_s_mean=round(float(a.mean()), 2), it_per_s_std=round(float(a.std(ddof=1)) if a.size > 1 else 0.0, 3), rounds=int(a.size)))
    h = md_schur.handle
    rng = np.random.default_rng(0)
    rhs = rng.standard_normal(n + m)
    out = dict(info=h.schur_info())
    fac = []
    for _ in range(3):
        t0 = time.perf_counter()
        h.update_rho(rng.uniform(0.05, 2.0, m))
        fac.append(time.perf_counter() - t0)
    out["factorisation_s"] = [round(x, 4) for x in fac]
    for steps in (0, args.refine_steps):
        h.set_schur_options(refine_steps=steps)
        h.set_params(cj.model._params_from_settings(None, md_schur.settings))
        h.kkt_solve(rhs)
        reps = 20
        t0 = time.perf_counter()
        for _ in range(reps):
            h.kkt_solve(rhs)
        out["us_per_kkt_solve_call_refine_%d" % steps] = round((time.perf_counter() - t0) / reps * 1e6, 1)
        out["residual_ratio_refine_%d" % steps] = h.schur_residual()
    say(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/schur_kkt_rate.py --rounds %d --refine-steps %d\n" % (args.rounds, args.refine_steps))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
