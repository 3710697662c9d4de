"""Batches of SDPs with one PSD cone of side 96 or 128: the persistent batch kernels (Settings.batch_psd_side_max) against the build of the parent
commit, where optimize_batch gives every such member its own single-problem handle.  One JSON line per workload into profiles/batch_psd_side.jsonl.

Workloads: 16, 64 and 256 members of problems.closest_correlation(d) with different seeds, d = 96 and d = 128, default settings.
Sides:     "new"    this tree, Settings(batch_psd_side_max=256): one persistent workgroup per member;
           "parent" a BUILT checkout of the parent commit (--parent ROOT), Settings(): a group of own handles.  It is not emulated with this build.
The two sides run in alternating rounds, each round a fresh process (`--worker`), --rounds per side; a workload's figures are the mean and the
standard deviation over the rounds of a side.  Per round and workload: wall time of optimize() (the set-up apart), iterations per member, statuses.
A gain is claimed only where parent mean - new mean exceeds three standard deviations of the parent's rounds.  Round 0 of the new side also solves
one d = 128 member through the single-problem handle (psd_projection "sign", the default, and "eigen"): the per-problem yardstick.

Usage: python tools/batch_psd_side_rate.py --parent /path/to/built/parent [--rounds 8] [--counts 16,64,256] [--sides 96,128]
                                            [--out profiles/batch_psd_side.jsonl] [--raw FILE] [--limit 600]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(args):
    """one round of one side in this process; one JSON line per workload on stdout"""
    sys.path.insert(0, args.root)
    import cosmo_jl_amd as cj
    assert os.path.dirname(os.path.dirname(os.path.abspath(cj.__file__))) == os.path.abspath(args.root), (cj.__file__, args.root)
    kw = dict(batch_psd_side_max=256) if args.worker == "new" else {}

    def models(d, count, **more):
        out = []
        for k in range(count):
            p = cj.problems.closest_correlation(d, seed=1000 + k)
            md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], cj.Settings(**kw, **more)); out.append(md)
        return out

    def solve(d, count):
        t0 = time.perf_counter()
        rs = cj.optimize_batch(models(d, count))
        info = dict(cj.model.LAST_BATCH_INFO)
        return dict(side=args.worker, round=args.round, d=d, members=count, wall_s=time.perf_counter() - t0, setup_s=info["setup_seconds"],
                    optimize_s=info["optimize_seconds"], own_handle_members=int(info.get("own_handle_members", 0)), mixed=bool(info["mixed"]),
                    kernel_form=info.get("kernel_form"), iters=[int(r.iter) for r in rs], solved=int(sum(r.status == "Solved" for r in rs)),
                    obj0=float(rs[0].obj_val))
    for d in args.sides:
        solve(d, 2)                                                               # warm-up: code objects, allocator, the shapes of this side
        for count in args.counts:
            print(json.dumps(solve(d, count)), flush=True)
    if args.worker == "new" and args.round == 0 and 128 in args.sides:
        for proj in ("sign", "eigen"):
            for rep in range(2):                                                  # the second solve is the warm one
                md = models(128, 1, psd_projection=proj)[0]
                t0 = time.perf_counter()
                r = cj.optimize(md)
                out = dict(side="single_handle", psd_projection=proj, d=128, members=1, wall_s=time.perf_counter() - t0, iters=[int(r.iter)],
                           solved=int(r.status == "Solved"), obj0=float(r.obj_val), warm=bool(rep))
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="root of a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--counts", default="16,64,256")
    ap.add_argument("--sides", default="96,128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_psd_side.jsonl"))
    ap.add_argument("--raw", default=None, help="every round's lines as they come")
    ap.add_argument("--limit", type=int, default=600, help="seconds a round may take")
    ap.add_argument("--worker", default=None, choices=["new", "parent"])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--round", type=int, default=0)
    args = ap.parse_args()
    args.counts = [int(v) for v in str(args.counts).split(",")]
    args.sides = [int(v) for v in str(args.sides).split(",")]
    if args.worker:
        return worker(args)
    if not args.parent:
        sys.exit("--parent: the baseline is the parent commit's own build")
    import numpy as np
    rows = []
    for rnd in range(args.rounds):
        for side, root in (("parent", os.path.abspath(args.parent)), ("new", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", side, "--root", root, "--round", str(rnd), "--counts", ",".join(map(str, args.counts)),
                   "--sides", ",".join(map(str, args.sides))]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit, cwd=root)
            if p.returncode != 0:                                                 # nothing more runs on the GPU after a failed round
                sys.exit("round %d of side %s ended with status %d" % (rnd, side, p.returncode))
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    rows.append(json.loads(line))
                    if args.raw:
                        with open(args.raw, "a") as f:
                            f.write(line + "\n")
            print("round %d %s done" % (rnd, side), flush=True)
    out = []
    for d in args.sides:
        for count in args.counts:
            rec = dict(workload="closest_correlation", d=d, members=count, rounds=args.rounds)
            for side in ("parent", "new"):
                sel = [r for r in rows if r["side"] == side and r["d"] == d and r["members"] == count]
                t = np.array([r["optimize_s"] for r in sel])
                rec[side] = dict(optimize_s_mean=float(t.mean()), optimize_s_std=float(t.std(ddof=1)) if t.size > 1 else 0.0,
                                 setup_s_mean=float(np.mean([r["setup_s"] for r in sel])), iters_mean=float(np.mean([np.mean(r["iters"]) for r in sel])),
                                 iters_min=int(min(min(r["iters"]) for r in sel)), iters_max=int(max(max(r["iters"]) for r in sel)),
                                 solved=int(min(r["solved"] for r in sel)), own_handle_members=int(sel[0]["own_handle_members"]), kernel_form=sel[0]["kernel_form"])
            diff = rec["parent"]["optimize_s_mean"] - rec["new"]["optimize_s_mean"]
            rec["parent_over_new"] = rec["parent"]["optimize_s_mean"] / rec["new"]["optimize_s_mean"]
            band = 3 * rec["parent"]["optimize_s_std"]
            rec["verdict"] = "one round: no spread" if args.rounds < 2 else ("gain" if diff > band else ("loss" if -diff > band else "no difference shown"))
            out.append(rec)
    out += [r for r in rows if r["side"] == "single_handle"]
    with open(args.out, "w") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
