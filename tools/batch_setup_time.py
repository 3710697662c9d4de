"""Set-up time of a batch with the host Ruiz scaling (Settings.batch_device_scaling = False, the default) and with the device pass (True;
csrc/batch_ruiz.hip), one JSON line per batch into profiles/batch_device_ruiz.jsonl.

Batches: 1024 x problems.socp() (config 3's batch) and 256 x problems.dense_qp() (config 1's size) on the CG batch kernels and on the direct batch.
Per batch, field off and on ALTERNATE in one process: one warm-up of each, then `--repeats` measured pairs.  Recorded per side:
  setup_s     wall time of prepare_batch -- host clock; it ends after cosmo_hip_batch_set_params, which synchronises -- median and the spread
              (max - min) over the repeats;
  optimize_s  wall time of the following optimize (a fixed number of ADMM iterations: eps = 0, no certificates), median.
and: ratio = setup_s off / on; accepted = the on-side median is below the off-side median by more than three times the larger spread;
ruiz_info of the pass; model_bytes = what the pass moves by the byte model rounds x three copies x (read + write) x sizeof(value) -- the kernel's own time
comes from a separate `rocprofv3 --kernel-trace --stats` run of `--profile-workload` (k_batch_ruiz), never from this script's clocks.
Usage: python tools/batch_setup_time.py [--repeats 3] [--iters 50] [--socp 1024] [--qp 256] [--out profiles/batch_device_ruiz.jsonl]
       python tools/batch_setup_time.py --profile-workload socp|qp    (one device-scaled set-up of that batch, nothing timed)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cosmo_jl_amd as cj  # noqa: E402


def socp_batch(count):
    return [cj.problems.socp(seed=1000 + k) for k in range(count)]


def qp_batch(count):
    return [cj.problems.dense_qp(seed=1 + k) for k in range(count)]


def models_of(probs, st):
    out = []
    for p in probs:
        md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st); out.append(md)
    return out


def one_side(probs, st):
    """(prepare_batch seconds, optimize seconds, ruiz_info or None) on fresh models"""
    mods = models_of(probs, st)
    t0 = time.perf_counter()
    B, _ = cj.model.prepare_batch(mods, 0)               # ends after set_params (synchronises) and set_iterates
    t1 = time.perf_counter()
    rs = B.optimize()
    t2 = time.perf_counter()
    assert max(r.iter for r in rs) == st.max_iter
    info = B.ruiz_info() if st.batch_device_scaling else None
    B.close()
    return t1 - t0, t2 - t1, info


def model_bytes(probs, rounds, isz=8):
    """rounds x the three staged copies (A, A', [P | A']) x read + write of their values"""
    nnz = sum(3 * int(p["A"].nnz) + int(p["P"].nnz) for p in probs)
    return int(rounds * nnz * 2 * isz)


def measure(name, probs, route, iters, repeats):
    kw = dict(max_iter=iters, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9)
    if route == "direct_batch":
        kw.update(kkt_solver=cj.QdldlKKTSolver, direct_batch=True)
    sides = {False: cj.Settings(**kw), True: cj.Settings(batch_device_scaling=True, **kw)}
    for on in (False, True):                              # warm-up of each shape and side
        one_side(probs, sides[on])
    setup = {False: [], True: []}; opt = {False: [], True: []}; info = None
    for _ in range(repeats):
        for on in (False, True):                          # alternate in the same process
            s, o, i = one_side(probs, sides[on])
            setup[on].append(s); opt[on].append(o); info = i or info
    med = lambda v: float(np.median(v))  # noqa: E731
    spr = lambda v: float(max(v) - min(v))  # noqa: E731
    n, m = int(probs[0]["P"].shape[0]), int(probs[0]["A"].shape[0])
    spread = max(spr(setup[False]), spr(setup[True]))
    return dict(batch=name, route=route, problems=len(probs), n=n, m=m, iters=iters, repeats=repeats,
                setup_off_s=round(med(setup[False]), 4), setup_off_spread_s=round(spr(setup[False]), 4),
                setup_on_s=round(med(setup[True]), 4), setup_on_spread_s=round(spr(setup[True]), 4),
                ratio=round(med(setup[False]) / med(setup[True]), 2),
                accepted=bool(med(setup[False]) - med(setup[True]) > 3.0 * spread),
                optimize_off_s=round(med(opt[False]), 4), optimize_on_s=round(med(opt[True]), 4),
                ruiz_info=info, model_bytes=model_bytes(probs, sides[True].scaling))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--socp", type=int, default=1024)
    ap.add_argument("--qp", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_device_ruiz.jsonl"))
    ap.add_argument("--profile-workload", choices=("socp", "qp"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("batch_setup_time.py measures on the MI355X; there is no CPU path")
    if a.profile_workload:
        probs = socp_batch(a.socp) if a.profile_workload == "socp" else qp_batch(a.qp)
        _, _, info = one_side(probs, cj.Settings(batch_device_scaling=True, max_iter=1, eps_abs=0.0, eps_rel=0.0, check_infeasibility=10 ** 9))
        print(json.dumps(dict(workload=a.profile_workload, problems=len(probs), ruiz_info=info, model_bytes=model_bytes(probs, 10))))
        return
    lines = []
    socp = socp_batch(a.socp)
    lines.append(measure("cfg3_socp", socp, "cg", a.iters, a.repeats))
    print(json.dumps(lines[-1]), flush=True)
    qp = qp_batch(a.qp)
    for route in ("cg", "direct_batch"):
        lines.append(measure("cfg1_dense_qp", qp, route, a.iters, a.repeats))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
