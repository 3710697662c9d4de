#!/usr/bin/env python
"""bench.py -- ADMM iterations/sec (fp64) of the MI355X-native COSMO hot path on BASELINE.json's configurations.

A "step" is ONE ADMM iteration of the loop body src/solver.jl:140-165 including the termination check every 25 iterations
(the reference's own iter_time definition, src/solver.jl:134,169), with the fixed-work settings of SURVEY 8d: eps_abs = eps_rel
= 0, adaptive_rho_interval = 40, scaling = 10, alpha = 1.6, sigma = 1e-6, rho = 0.1, CG tolerance 1/k^1.5, EmptyAccelerator.

Workloads (--workload):
  cfg5  chordal-decomposed SDP n=50k, 400 PSD cliques d in [20,200] + ZeroSet / Nonnegatives   [the workload north_star's targets are stated on;
        the largest BASELINE configuration, fits one GPU: THE HEADLINE at every N since round 5]
  cfg2  random sparse QP n=100k m=200k nnz(A)=2M, Box cone, CG indirect KKT            [BASELINE configs[1]]
  cfg3  1024 independent SOCPs n=500 m=1000, 50 SecondOrderCones each (one step = one iteration of ALL problems)
  cfg4  closest-correlation SDP, one PsdConeTriangle d=2000
  all   (default) headline line = cfg5; cfg2 / cfg3 / cfg4 measured in the same run and reported under "extra"

Multi-GPU (`python bench.py --gpus N` re-launches itself under torch.distributed.run, one process per GPU, RCCL; a launch that
already comes from torch.distributed.run / torchrun is used as it is):
  headline line at EVERY N = cfg5, ONE problem: N = 1 unsharded; N > 1 its cones and all their rows of A / s / mu / rho sharded over the ranks
  (csrc/rowshard.hip; the loop being sharded: src/convexset.jl:885-891, src/linear_solver/kktsolver_indirect.jl:52-54), "scaling": "strong",
  value = steps / max-over-ranks time of the literal cg! path.  The line carries its own parity evidence at the TOP level (config.parity_*,
  config.comm_selftest: flat scalars next to the nested objects), rank 0's unsharded time of the same problem in the same run, the exchange volume
  per iteration, the measured shardable share f of the 1-GPU iteration and the bound 1 / ((1 - f) + f / N) it implies.
  extra.cfg3_sharded = the batch of 1024 SOCPs sharded over the ranks (no collective), strong.
  extra.cfg2_replicas / cfg4_replicas = N independent replicas (these two do not shard): "scaling": "replicas", value = ONE replica's rate
  (max-over-ranks time) -- never aggregated, never a headline.
  --workload cfgK makes that workload the headline instead (cfg5 / cfg3: sharded, strong; cfg2 / cfg4: replicas, weak, value = N x rate).

Output: ONE JSON line on rank 0 (the driver contract) with `roofline` for the dominant kernel of the headline workload and
`cpu_baseline` (the restated CPU reference timed on a bounded sample: the CG path with 1 thread and all host threads where LAPACK is involved, and --
`cpu_baseline.direct_kkt` -- the reference's DEFAULT direct LDL' KKT solver, the CPU path north_star names), and a compact `summary` as the LAST key
(the driver keeps the tail of the line: all four rates must survive there).

Plain run vs --full: a plain `python bench.py --gpus N --steps K --warmup W` sets up the headline workload, warms up, times the K steps and prints
the line (metric, value, unit, ms_per_step, dtype, config); it runs nothing else.  Everything described above that takes work of its own -- the
roofline timings, cpu_baseline, the other workloads under `extra`, the opt-in variants and Float32 numbers, cfg3's time to solution and, at N > 1,
the parity leg and the unsharded comparison -- runs only with --full (the --no-* options then leave parts of it out again).
--dump-outputs DIR: after the timed steps, the arrays the timed path hands its caller (x, y, s as optimize() returns them) as DIR/<name>.npy,
at most DUMP_LIMIT_BYTES in all; the inputs are seeded, so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

if "--cpu-leg" in sys.argv:          # child process of the all-threads cpu_baseline leg: pin the cores BEFORE OpenBLAS creates its threads
    _cpus = [int(c) for c in sys.argv[sys.argv.index("--cpu-leg-cpus") + 1].split(",")]
    os.sched_setaffinity(0, _cpus)
    os.environ["OPENBLAS_NUM_THREADS"] = os.environ["OMP_NUM_THREADS"] = str(len(_cpus))

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md
F64_MFMA_PEAK_TF = 78.6    # fp64 matrix peak (the guide lists no fp64 row, the vector and matrix fp64 peaks coincide)
# what a register-operand v_mfma_f64_16x16x4_f64 stream sustains on this chip with two waves per SIMD (bench/mfma_lab.hip,
# profiles/r02_mfma_ceiling_and_gemm_lab.txt); reported beside `peak`, never instead of it
F64_MFMA_SUSTAINED_TF = 66.9
METRIC = "ADMM iterations/sec (fp64) at fixed (n,m,nnz,cone)"
DUMP_LIMIT_BYTES = 60 * 10 ** 6     # --dump-outputs: array bytes in all (the .npy headers stay well inside 64 MB)


# ---------------------------------------------------------------------------------------------------------------------
# helpers shared with tests/test_distributed_cpu.py
# ---------------------------------------------------------------------------------------------------------------------
def max_over_ranks(elapsed, dist, device):
    """The bench contract's timing rule: every rank times its own K steps, the job's time is the MAX over the ranks."""
    import torch
    t = torch.tensor([elapsed], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def whole_job_value(world, steps, elapsed):
    """Aggregate throughput of `world` replicas that each did `steps` iterations in `elapsed` seconds (weak scaling)."""
    return world * steps / elapsed


def algorithmic_bytes(n, m, nnzA, nnzP):
    """SURVEY 8d per-launch compulsory bytes (fp64 values 8 B, int32 indices 4 B, every array once)."""
    b_A = 12.0 * nnzA + 4.0 * (m + 1) + 8.0 * n + 8.0 * m
    b_AT = 12.0 * nnzA + 4.0 * (n + 1) + 8.0 * m + 8.0 * n
    b_P = 12.0 * nnzP + 4.0 * (n + 1) + 16.0 * n
    # fused operator kernel c = [P | A'] [v; tmp] + sigma v: both matrices once, one row-pointer + one split array,
    # gather vectors v (n) and tmp (m) once, c written once, v re-read for the sigma term / dot product is cached
    b_op = 12.0 * (nnzA + nnzP) + 8.0 * (n + 1) + 8.0 * (n + m) + 8.0 * n
    b_vec = 8.0 * (8 * n + 13 * m)
    b_cgvec = 8.0 * (10 * n + m)
    return dict(A=b_A, AT=b_AT, P=b_P, op=b_op, vec=b_vec, cgvec=b_cgvec)


def iteration_bytes(ab, kbar):
    """B_iter(K) of SURVEY 8d."""
    return ab["vec"] + (kbar + 2) * (ab["A"] + ab["AT"]) + (kbar + 1) * (ab["P"] + ab["cgvec"])


def psd_useful_flops(d, r=None):
    """F_psd(d, r) of SURVEY 8d: the REFERENCE algorithm's flops for one d x d block (tridiagonalise 4/3 d^3, back-transform 2 d^3,
    SYRK d(d+1) r with r = #positive eigenvalues ~ d/2)."""
    r = d / 2.0 if r is None else r
    return (10.0 / 3.0) * d ** 3 + d * (d + 1.0) * r


# ---------------------------------------------------------------------------------------------------------------------
# --dump-outputs
# ---------------------------------------------------------------------------------------------------------------------
def dump_outputs(dirname, arrays):
    """Write every array as DIR/<name>.npy (float32 stays float32, everything else float64).  Above DUMP_LIMIT_BYTES in all, every array is cut
    to the same fraction of its entries, a sorted sample drawn with a fixed seed: the same positions at every run of the same workload."""
    os.makedirs(dirname, exist_ok=True)
    arrays = {k: np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64) for k, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > DUMP_LIMIT_BYTES:
            keep = a.size * DUMP_LIMIT_BYTES // total
            a = a[np.sort(np.random.default_rng(0).choice(a.size, size=keep, replace=False))]
        np.save(os.path.join(dirname, name + ".npy"), a)


def caller_arrays(md, w_prev, s, mu):
    """x, y, s of one problem from its device iterates, as optimize() returns them (reverse_scaling!, src/scaling.jl:170-179; y = -mu)."""
    x = w_prev[:md.n]
    if md.settings.scaling != 0:
        x, s, mu = md.sm.D * x, md.sm.Einv * s, (md.sm.E * mu) * md.sm.cinv
    return dict(x=x, y=-mu, s=s)


def dump_handle_outputs(ctx, args, model):
    """--dump-outputs of a single-problem workload, read right after the timed steps.  On a sharded handle get_iterates is collective (every
    rank receives the global vectors), so every rank reads and rank 0 writes."""
    if not args.dump_outputs:
        return
    _, w_prev, s, mu = model.handle.get_iterates()
    if ctx.rank == 0:
        dump_outputs(args.dump_outputs, caller_arrays(model, w_prev, s, mu))


class Ctx:
    def __init__(self):
        import torch
        self.torch = torch
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.dist = None
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a MI355X (no CPU fallback)")
        # COSMO_BENCH_TRANSPORT=shm: dry run of the multi-rank path on ONE GPU (every rank on device 0, gloo for the barriers, the
        # host-staged exchange of csrc/comm.hip instead of RCCL, which refuses two ranks on one device).  Functional check only
        # (tests/test_gpu_sharding.py); the line it prints says so and is not a measurement.
        self.shm = os.environ.get("COSMO_BENCH_TRANSPORT", "") == "shm"
        if self.shm:
            self.local_rank = 0
        elif self.world > torch.cuda.device_count():
            raise SystemExit("bench.py: %d ranks but %d visible GPU(s) -- one process per GPU (COSMO_BENCH_TRANSPORT=shm runs a functional "
                             "dry run of the multi-rank path on one GPU)" % (self.world, torch.cuda.device_count()))
        torch.cuda.set_device(self.local_rank)
        if self.world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if self.shm:
                dist.init_process_group(backend="gloo")
            else:
                dist.init_process_group(backend="nccl", device_id=torch.device("cuda", self.local_rank))
            self.dist = dist

    def barrier(self):
        if self.dist is not None:
            self.dist.barrier()
        self.torch.cuda.synchronize()

    def timed(self, fn):
        """barrier + synchronize, run fn (which must drain its stream), synchronize; MAX over the ranks."""
        self.barrier()
        t0 = time.perf_counter()
        fn()
        self.torch.cuda.synchronize()
        el = time.perf_counter() - t0
        self.last_rank_seconds = [el]
        if self.dist is not None:
            every = [None] * self.world
            self.dist.all_gather_object(every, float(el))       # per-rank times: load imbalance must be visible in the line (min / max)
            self.last_rank_seconds = [float(t) for t in every]
            el = max_over_ranks(el, self.dist, "cpu" if self.shm else "cuda")
            self.dist.barrier()
        return el

    def rank_seconds(self):
        t = getattr(self, "last_rank_seconds", None) or [0.0]
        return dict(min=round(min(t), 6), max=round(max(t), 6), per_rank=[round(x, 6) for x in t])

    def all_gather(self, obj):
        if self.dist is None:
            return [obj]
        every = [None] * self.world
        self.dist.all_gather_object(every, obj)
        return every


KKT_CHOICE = {"name": "cg"}


def fixed_work_settings(cj, **kw):
    kkt = cj.CGSingleReductionKKTSolver if KKT_CHOICE["name"] == "cg-sr" else cj.CGIndirectKKTSolver
    base = dict(eps_abs=0.0, eps_rel=0.0, max_iter=10 ** 9, check_infeasibility=10 ** 9, kkt_solver=kkt)
    base.update(kw)
    return cj.Settings(**base)


def oracle_settings(O, iters):
    return O.Settings(kkt_solver="cg", eps_abs=0.0, eps_rel=0.0, max_iter=iters, check_infeasibility=10 ** 9)


def host_threads():
    try:
        return len(os.sched_getaffinity(0))
    except Exception:
        return os.cpu_count() or 1


def _cpulist(text):
    out = set()
    for part in text.strip().split(","):
        if part:
            a, _, b = part.partition("-")
            out.update(range(int(a), int(b or a) + 1))
    return out


def numa_node0_physical_cores(cap=32):
    """One hardware thread per physical core of NUMA node 0 among the CPUs this process may use (the all-threads BLAS leg runs there: spread over
    both sockets / all 256 hardware threads of the GPU host, OpenBLAS' syevr was SLOWER than one thread in round 2).  Returns (cpu ids, description)."""
    allowed = set(os.sched_getaffinity(0))
    try:
        node0 = _cpulist(open("/sys/devices/system/node/node0/cpulist").read()) & allowed
        where = "NUMA node 0"
    except Exception:
        node0, where = set(allowed), "all allowed CPUs (no NUMA information)"
    if not node0:
        node0, where = set(allowed), "all allowed CPUs (node 0 not in the affinity mask)"
    cores = {}
    for c in sorted(node0):
        try:
            key = min(_cpulist(open("/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list" % c).read()))
        except Exception:
            key = c
        cores.setdefault(key, c)
    cpus = sorted(cores.values())[:cap]
    return cpus, "%d physical cores of %s (one hardware thread each; host exposes %d hardware threads)" % (len(cpus), where, len(allowed))


def _native_oracle():
    """The compiled C restatement (oracle/cosmo_oracle_c.c) built -O3 -march=native ON the host whose cores are timed."""
    import subprocess
    from oracle import cosmo_oracle_c as OC
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "native"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    OC.lib(native=True)
    return OC


def compiled_cpu_rate(prob, iters, threads=1):
    """ADMM iterations/s of the compiled C loop (Julia-style CSC SpMVs, serial cone loop, LAPACK ?syevr + BLAS ?syrk projections through SciPy's
    OpenBLAS with `threads` BLAS threads) on a NumPy-oracle workspace (setup = scaling / classification, excluded like the reference's setup!).
    The init step (one KKT solve) is part of iter_time on both sides."""
    from oracle import cosmo_oracle as O
    from tests import util
    from threadpoolctl import threadpool_limits
    OC = _native_oracle()
    ws = O.Workspace(prob["P"], prob["q"], prob["A"], prob["b"], util.oracle_cones(prob["sets"]), oracle_settings(O, iters))
    with threadpool_limits(limits=threads):
        c = OC.run(ws, native=True)
    return dict(rate=c["iter"] / c["iter_time"], iters=c["iter"], secs=c["iter_time"], cg=c["cg_iters_total"] / (c["iter"] + 1.0), proj_secs=c["proj_time"])


def compiled_cpu_baseline(prob, iters, label, workload_key, args, with_all_threads=True, iters_all=None):
    """cpu_baseline of one configuration: the compiled loop with 1 thread (what the tagged reference does outside BLAS) and -- where LAPACK is
    involved -- with the physical cores of one NUMA node as BLAS threads, run in a child process that is pinned to them before OpenBLAS starts."""
    r1 = compiled_cpu_rate(prob, iters, 1)
    out = dict(value=r1["rate"], unit="ADMM iterations/s", cores=1, kind="port",
               sample="compiled C loop (gcc -O3 -march=native; oracle/cosmo_oracle_c.c): %d ADMM iteration(s) + init step of the same %s instance, %.1f s "
                      "(%.1f s of it in the cone projections), 1 thread; mean CG its/solve %.1f" % (r1["iters"], label, r1["secs"], r1["proj_secs"], r1["cg"]))
    if with_all_threads:
        import subprocess
        cpus, where = numa_node0_physical_cores(cap=16)       # 32 threads were slower still (r03_bench_all_v3.json: cfg5 0.037 it/s against 0.153 with one)
        if len(cpus) > 1:
            cmd = [sys.executable, os.path.abspath(__file__), "--cpu-leg", workload_key, "--cpu-leg-cpus", ",".join(map(str, cpus)), "--cpu-leg-iters", str(iters_all or iters)]
            if args.small:
                cmd.append("--small")
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
                rn = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
                out["all_threads"] = dict(value=rn["rate"], cores=len(cpus), sample="%d iteration(s), %.1f s (%.1f s projections), OpenBLAS threads = %s, process pinned to them%s"
                                          % (rn["iters"], rn["secs"], rn["proj_secs"], where,
                                             "" if rn["rate"] >= r1["rate"] else "; SLOWER than one thread: OpenBLAS' threaded syevr / syrk do not scale at these matrix sizes"))
            except Exception as e:
                out["all_threads"] = dict(error="%s: %s" % (type(e).__name__, e))
    return out


def direct_kkt_cpu_baseline(prob, iters, label):
    """cpu_baseline.direct_kkt: the reference's DEFAULT CPU path (north_star: "the reference Julia/QDLDL CPU path") -- QdldlKKTSolver
    (src/linear_solver/kktsolver.jl:285-320): quasi-definite LDL' of [P + sigma I, A'; A, -diag(1/rho)] once (+ once per rho update) and one
    permuted triangular solve pair per ADMM iteration -- inside the same compiled loop (oracle/cosmo_oracle_c.c: the restated QDLDL algorithm, 1 thread
    like QDLDL.jl; projections through LAPACK ?syevr + ?syrk as the reference does).  The first factorisation and the ordering are setup (outside
    iter_time on every side) and reported separately."""
    from oracle import cosmo_oracle as O
    from tests import util
    from threadpoolctl import threadpool_limits
    OC = _native_oracle()
    ws = O.Workspace(prob["P"], prob["q"], prob["A"], prob["b"], util.oracle_cones(prob["sets"]), oracle_settings(O, iters))
    t0 = time.perf_counter()
    cached = os.path.exists(os.path.join(OC.PERM_DIR, "perm_%s.npz" % OC._pattern_key(ws.P, ws.A)))
    perm = OC.kkt_ordering(ws)
    t_ord = time.perf_counter() - t0
    with threadpool_limits(limits=1):
        c = OC.run(ws, native=True, direct=dict(perm=perm, nnz_cap=int(6e8)))
    L = c["ldl"]
    return dict(value=c["iter"] / c["iter_time"], unit="ADMM iterations/s", cores=1, kind="port",
                kkt="QdldlKKTSolver restated (published QDLDL algorithm: etree + up-looking LDL'; QDLDL.jl 0.4.1 / AMD.jl are not vendored in the reference tree)",
                factor_s=round(L["factor_s"] / max(L["n_factor"], 1), 3), n_factor=L["n_factor"], solve_ms=round(1e3 * L["solve_s"] / max(L["n_solve"], 1), 3),
                nnz_L=L["nnz_L"], kkt_dim=int(ws.n + ws.m), ordering_s=round(t_ord, 2),
                ordering="minimum degree: rows of A with <= 1 entry first (no fill), SuperLU MMD(A'+A) on the Schur complement pattern of the rest%s"
                         % (" (read from oracle/kkt_perm/, keyed by the sparsity pattern)" if cached else ""),
                sample="compiled C loop with the direct solve: %d ADMM iteration(s) + init step of the same %s instance, %.1f s of loop time (%.1f s projections, %.2f s "
                       "triangular solves), 1 thread; the first factorisation (%.1f s) is setup, refactorisations at rho updates (%d here) are inside"
                       % (c["iter"], label, c["iter_time"], c["proj_time"], L["solve_s"], L["factor_s"] / max(L["n_factor"], 1), L["n_factor"] - 1))


def direct_kkt_probe_cfg2(prob, cap=int(4e8)):
    """BASELINE config 2 is DEFINED with the CG indirect solver, and for a reason that can be measured: the elimination-tree pass of the QDLDL
    restatement counts the fill of its KKT matrix (uniformly random pattern) under two orderings and stops at `cap` nonzeros."""
    from oracle import cosmo_oracle as O
    from tests import util
    from scipy.sparse.csgraph import reverse_cuthill_mckee
    OC = _native_oracle()
    ws = O.Workspace(prob["P"], prob["q"], prob["A"], prob["b"], util.oracle_cones(prob["sets"]), oracle_settings(O, 1))
    n, m = ws.n, ws.m
    K = OC.kkt_full(ws)
    t0 = time.perf_counter()
    tried = {"rows of A first, then x (what minimum degree does with degree-10 row nodes)": np.concatenate([np.arange(n, n + m), np.arange(n)]).astype(np.int64),
             "reverse Cuthill-McKee of K": np.asarray(reverse_cuthill_mckee(K.tocsr(), symmetric_mode=True), np.int64)}
    res = {k: OC.ldl_nnz(ws, p, cap=cap, native=True) for k, p in tried.items()}
    feasible = any(v >= 0 for v in res.values())
    return dict(feasible=feasible, nnz_L={k: (v if v >= 0 else "> %d" % cap) for k, v in res.items()}, kkt_dim=int(n + m), probe_s=round(time.perf_counter() - t0, 2),
                note=("the LDL' factor of this KKT matrix exceeds %.0e nonzeros (> %.1f GB, > ~1e12 flops per factorisation) under every ordering tried: the Schur "
                      "complement onto x is a uniformly random graph of mean degree ~%d on %d nodes, whose Cholesky factor is essentially dense (%.1e entries); "
                      "the direct path is not a baseline for this configuration -- BASELINE.json itself specifies the CG indirect KKT solver for it"
                      % (cap, 12.0 * cap / 1e9, int(ws.A.nnz / n * (ws.A.nnz / m - 1.0)), n, n * (n + 1) / 2.0)) if not feasible else "fits: see nnz_L")


def _problem_for(key, small):
    import cosmo_jl_amd as cj
    if key == "cfg2":
        return cj.problems.sparse_box_qp(n=10_000, m=20_000, nnz=200_000) if small else cj.problems.sparse_box_qp()
    if key == "cfg4":
        return cj.problems.closest_correlation(d=400 if small else 2000)
    if key == "cfg5":
        return cj.problems.chordal_sdp(**(dict(ncliques=40, n_total=6000, n_zero=100, n_nonneg=500) if small else {}))
    raise ValueError(key)


def cpu_leg_main():
    """`bench.py --cpu-leg cfgK --cpu-leg-cpus a,b,c --cpu-leg-iters N`: the all-threads leg of a cpu_baseline (no GPU involved); affinity and the
    BLAS thread count were fixed at the top of this file, before NumPy / SciPy loaded OpenBLAS."""
    key = sys.argv[sys.argv.index("--cpu-leg") + 1]
    iters = int(sys.argv[sys.argv.index("--cpu-leg-iters") + 1])
    ncpu = len(sys.argv[sys.argv.index("--cpu-leg-cpus") + 1].split(","))
    print(json.dumps(compiled_cpu_rate(_problem_for(key, "--small" in sys.argv), iters, ncpu)), flush=True)


# ---------------------------------------------------------------------------------------------------------------------
# cfg2
# ---------------------------------------------------------------------------------------------------------------------
def bench_cfg2(ctx, args, steps, warmup):
    import cosmo_jl_amd as cj
    prob = cj.problems.sparse_box_qp(n=10_000, m=20_000, nnz=200_000) if args.small else cj.problems.sparse_box_qp()
    st = fixed_work_settings(cj)
    st.device = ctx.local_rank
    model = cj.Model()
    model.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
    cj.model.setup(model)                       # upload + Ruiz scaling on the device (setup!, excluded from iter_time)
    h = model.handle
    n, m, nnzA, nnzP = model.n, model.m, model.A.nnz, model.P.nnz
    h.set_iterates(model.x, model.s, model.mu)
    h.admm_init()
    if args.exact_launches:
        h.set_profiling(2)
    h.admm_iterate_checked(warmup)
    stats0 = h.get_stats()
    elapsed = ctx.timed(lambda: h.admm_iterate_checked(steps))          # returns after the stream has drained (host sync inside)
    stats1 = h.get_stats()
    assert stats1["admm_iters"] - stats0["admm_iters"] == steps
    dump_handle_outputs(ctx, args, model)
    kbar = (stats1["kkt_iters_total"] - stats0["kkt_iters_total"]) / max(1, stats1["kkt_solves"] - stats0["kkt_solves"])
    world = ctx.world
    value = whole_job_value(world, steps, elapsed)
    out = dict(value=value, ms_per_step=1e3 * elapsed / steps, steps=steps, warmup=warmup, scaling="weak")
    rank_seconds = ctx.rank_seconds()
    if ctx.rank != 0:
        return out
    ab = algorithmic_bytes(n, m, nnzA, nnzP)
    if args.full:
        # dominant kernel: the fused [P | A'] operator SpMV of the CG iteration (K-bar launches per ADMM iteration).  Duration: HIP events
        # on the library's stream around R back-to-back launches of exactly that kernel on the live loop state (one event pair per R
        # launches: the ~5 us of an event pair would swamp a 10-20 us kernel; the launch gap IS included, i.e. the number is conservative).
        t_op, bytes_op = min(h.time_spmv(cj._ffi.MAT_OP, 200) for _ in range(3))        # best of three event pairs of 200 launches (one read 21.9 us once: r03_bench_all_v2)
        t_A, bytes_A = min(h.time_spmv(cj._ffi.MAT_A, 200) for _ in range(3))            # all four timed the same way (best of 3 x 200)
        t_AT, bytes_AT = min(h.time_spmv(cj._ffi.MAT_AT, 200) for _ in range(3))
        t_P, bytes_P = min(h.time_spmv(cj._ffi.MAT_P, 200) for _ in range(3))
        achieved = bytes_op / t_op / 1e9
        traffic, traffic_src = None, None
        if not args.small:
            import glob
            for fpmc in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_cfg2_pmc_traffic.json"))):
                try:
                    with open(fpmc) as fh:
                        traffic = json.load(fh)["kernels"]["k_op_apply"]["hbm_bytes_per_launch"]
                    traffic_src = os.path.relpath(fpmc, ROOT)
                except Exception:
                    pass

        def other(b, t):
            return dict(achieved=round(b / t / 1e9, 1), frac=round(b / t / 1e9 / HBM_PEAK_GBS, 4), algorithmic_bytes_per_launch=b, avg_launch_us=round(1e6 * t, 3))
        out["roofline"] = dict(bound="hbm", kernel="k_op_apply (c = [P|A'][v; rho.*(A v)] + sigma v, CSR-stream SpMV)", achieved=round(achieved, 1),
                               peak=HBM_PEAK_GBS, unit="GB/s", frac=round(achieved / HBM_PEAK_GBS, 4), traffic=traffic, traffic_source=traffic_src,
                               algorithmic_bytes_per_launch=bytes_op, avg_launch_us=round(t_op * 1e6, 3), launches_timed=200, timing="best of 3 x 200 back-to-back launches",
                               other={"k_spmv_A_rho (A v)": other(bytes_A, t_A), "k_cg_rhs (A' y)": other(bytes_AT, t_AT), "k_spmv_plain (P x)": other(bytes_P, t_P)})
    b_iter = iteration_bytes(ab, kbar)
    # (`workload` stays under 120 characters: the driver's parsed copy of the line cut the longer string of round 3 in the middle of a word)
    out["config"] = {"workload": "cfg2: random sparse QP n=%d m=%d nnz(A)=%d, Box cone, CG indirect KKT" % (n, m, nnzA),
                     "workload_detail": "nnz(P)=%d; CG tolerance 1/k^1.5, check_termination=25, adaptive_rho_interval=40, Ruiz scaling=10, eps_abs=eps_rel=0 (fixed work), "
                                        "alpha=1.6, sigma=1e-6, rho=0.1, EmptyAccelerator (SURVEY 8d)" % nnzP,
                     "parallelism": "replicas x%d (a single sparse QP does not shard; SURVEY 8e)" % world,
                     "mean_cg_iters_per_admm_iter": round(kbar, 3), "kkt_budget_stalls": stats1["kkt_budget_stalls"],
                     "iteration_roofline_frac": round(b_iter * (value / world) / (HBM_PEAK_GBS * 1e9), 4), "rank_seconds": rank_seconds,
                     "algorithmic_bytes_per_iteration": b_iter}
    if not args.no_cpu_baseline and world == 1:
        def cpu_leg(out=out, prob=prob, value=value):
            out["cpu_baseline"] = compiled_cpu_baseline(prob, args.cpu_sample_iters if not args.small else 200, "cfg2", "cfg2", args, with_all_threads=False)   # no BLAS in this configuration
            out["config"]["gpu_over_cpu"] = round(value / out["cpu_baseline"]["value"], 2)
            try:
                out["cpu_baseline"]["direct_kkt"] = direct_kkt_probe_cfg2(prob)
            except Exception as e:
                out["cpu_baseline"]["direct_kkt"] = dict(error="%s: %s" % (type(e).__name__, e))
        args.deferred.append(cpu_leg)
    h.close()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cfg3: batch of independent SOCPs, sharded over the ranks (no collective)
# ---------------------------------------------------------------------------------------------------------------------
def bench_cfg3(ctx, args, steps, warmup):
    import cosmo_jl_amd as cj
    nprob = 64 if args.small else 1024
    lo, hi = cj.model.shard_range(nprob, ctx.rank, ctx.world)
    probs = [cj.problems.socp(seed=1000 + k) for k in range(lo, hi)]
    st = fixed_work_settings(cj)
    mods = []
    for p in probs:
        md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st); mods.append(md)
    B, _ = cj.model.prepare_batch(mods, ctx.local_rank)
    B.iterate(warmup, with_init=True)
    _, _, kk0 = B.counters()
    elapsed = ctx.timed(lambda: B.iterate(steps))
    _, _, kk1 = B.counters()
    if args.dump_outputs:                                    # every problem of the job, in global order (the shards are contiguous)
        mine = [caller_arrays(md, *B.get_iterates(k)[1:]) for k, md in enumerate(mods)]
        every = [p for part in ctx.all_gather(mine) for p in part]
        if ctx.rank == 0:
            dump_outputs(args.dump_outputs, {key: np.concatenate([p[key] for p in every]) for key in ("x", "y", "s")})
    value = steps / elapsed                                  # one step = one ADMM iteration of ALL problems of the job
    out = dict(value=value, ms_per_step=1e3 * elapsed / steps, steps=steps, warmup=warmup, scaling="strong")
    rank_seconds = ctx.rank_seconds()
    parity = None
    kry_every = ctx.all_gather((kk1 - kk0).astype(np.float64)) if ctx.world > 1 else None
    if ctx.world > 1 and args.full and os.environ.get("COSMO_BENCH_PARITY", "1") != "0":
        # parity evidence inside the N > 1 line: a sample of problems FROM EVERY RANK's shard (its first `per`), iterates after warmup + steps
        # iterations, against ONE single-rank batch of exactly those problems run by rank 0 with the same call sequence.  The problems of a batch are
        # independent (src/solver.jl:140-165 per problem, no exchange), so the expected deviation is 0 (bit-identical).
        per = max(1, min(hi - lo, 32 // ctx.world))
        mine = [(lo + k, B.get_iterates(k)[0]) for k in range(per)]
        every = ctx.all_gather(mine)
        if ctx.rank == 0:
            samp = [kv for part in every for kv in part]
            mods1 = []
            for gk, _ in samp:
                p1 = cj.problems.socp(seed=1000 + gk)
                md = cj.Model(); md.set(p1["P"], p1["q"], p1["A"], p1["b"], p1["sets"], st); mods1.append(md)
            B1, _ = cj.model.prepare_batch(mods1, ctx.local_rank)
            B1.iterate(warmup, with_init=True); B1.iterate(steps)
            dev = 0.0
            for j, (gk, wsh) in enumerate(samp):
                w1 = B1.get_iterates(j)[0]
                d = float(np.max(np.abs(wsh - w1)) / max(np.max(np.abs(w1)), 1e-300))
                dev = max(dev, d if np.isfinite(d) else float("inf"))
            B1.close()
            parity = dict(sharded_vs_single_max_rel_dev=dev, expected_at_most=0.0, ok=bool(dev == 0.0), problems_compared=len(samp),
                          sample="the first %d problem(s) of every rank's shard (global indices %s), w after %d iterations, against a single-rank batch of "
                                 "exactly these problems on rank 0" % (per, [gk for gk, _ in samp][:8] + (["..."] if len(samp) > 8 else []), warmup + steps))
        ctx.barrier()
    if ctx.rank != 0:
        B.close()
        return out
    n, m = mods[0].n, mods[0].m
    nnzA, nnzP = int(np.mean([md.A.nnz for md in mods])), int(np.mean([md.P.nnz for md in mods]))
    kry = (kk1 - kk0).astype(np.float64)                      # Krylov iterations per problem inside the timed steps (device counters)
    kry_all = np.concatenate(kry_every) if kry_every is not None else kry
    out["config"] = {"workload": "cfg3: %d independent SOCPs n=%d m=%d nnz(A)~%d, 50 SecondOrderCone(20) each" % (nprob, n, m, nnzA),
                     "workload_detail": "one step = one ADMM iteration of every problem; one persistent workgroup per problem (csrc/batch.hip)",
                     "parallelism": "batch sharded over %d rank(s), %d problems on rank 0, no collective" % (ctx.world, hi - lo),
                     "problem_iterations_per_s": round(value * nprob, 1), "rank_seconds": rank_seconds, "parity": parity,
                     "krylov_iterations_per_problem_in_timed_steps": dict(mean=round(float(kry.mean()), 1), max=int(kry.max()), min=int(kry.min()),
                                                                          largest_16=[int(v) for v in np.sort(kry)[::-1][:16]]),
                     "us_per_krylov_iteration_of_the_slowest_problem": round(1e6 * elapsed / max(float(kry.max()), 1.0), 3),
                     "kernel": B.kernel_info(),
                     "scaling_model": cfg3_scaling_model(cj, kry_all, elapsed, ctx.world)}
    # What bounds the persistent kernel is the LDS: every Krylov iteration streams the problem's LDS image once through the two sparse passes --
    # A pass: (value 8 B + u16 column + 8 B gathered x) per nonzero; [P | A'] pass: (packed u32 position / row + 8 B value + 8 B gathered y) per
    # nonzero of A and (8 + 2 + 8) per nonzero of P (a diagonal P sits in registers in the sliced image: those bytes are then not read, the formula keeps
    # them).  achieved = MEASURED Krylov iterations of rank 0's problems x those bytes / elapsed, against
    # the chip's LDS read peak (guide: ~150 TB/s for ds_read_b64 at 2.4 GHz).  The batch ends with its slowest problem, so the rate is set by
    # max (not mean) Krylov iterations x the time one workgroup needs per Krylov iteration (`us_per_krylov_iteration_of_the_slowest_problem`): the
    # serial chain of ONE CU's LDS pipe, not the chip's LDS bandwidth.
    lds_bytes_per_krylov = nnzA * (8 + 2 + 8) + nnzA * (2 + 2 + 8 + 8) + nnzP * (8 + 2 + 8) + 8.0 * (4 * n + 2 * m)
    lds_achieved = float(kry.sum()) * lds_bytes_per_krylov / elapsed / 1e9
    LDS_PEAK_GBS = 150000.0
    out["roofline"] = dict(bound="lds", kernel="k_batch_admm_reg (persistent, LDS-resident problem image, register-resident iterates)",
                           achieved=round(lds_achieved, 1), peak=LDS_PEAK_GBS, unit="GB/s", frac=round(lds_achieved / LDS_PEAK_GBS, 4), traffic=None,
                           lds_bytes_per_krylov_iteration_per_problem=lds_bytes_per_krylov, krylov_iterations_timed=int(kry.sum()),
                           note="LDS bytes of the sparse passes x measured Krylov iterations (device counters) / elapsed; HBM is touched at launch and at the checks "
                                "only.  The slowest problem's dependent chain of Krylov iterations, not LDS bandwidth, ends the step (see config)")
    if ctx.world == 1 and args.full and os.environ.get("COSMO_BENCH_TTS", "1") != "0":
        # Time to solution of the whole batch (every problem to the default eps = 1e-5, certificates on) with a tight KKT solve, without and with the
        # reference's default accelerator (AndersonAccelerator, mem 15, safeguarded) running inside the persistent kernels.  Reported, not the metric.
        try:
            tight = cj.with_options(cj.CGIndirectKKTSolver, tol_constant=1e-10, tol_exponent=0.0)
            tts = {}
            for label, stt in (("plain", cj.Settings(kkt_solver=tight)), ("anderson", cj.Settings(kkt_solver=tight, accelerator=cj.AndersonAccelerator))):
                ms = []
                for p in probs:
                    md = cj.Model(); md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], stt); ms.append(md)
                Bt, _ = cj.model.prepare_batch(ms, ctx.local_rank)
                t0 = time.perf_counter(); rs = Bt.optimize(); dt = time.perf_counter() - t0
                its = np.array([r.iter for r in rs])
                tts[label] = dict(seconds=round(dt, 4), solved=int(sum(r.status == 1 for r in rs)), admm_iterations_max=int(its.max()), admm_iterations_sum=int(its.sum()),
                                  krylov_iterations_sum=int(sum(r.kkt_iters_total for r in rs)), safeguarding_iterations=int(sum(r.safeguarding_iter for r in rs)))
                Bt.close()
            tts["note"] = ("cosmo_hip_batch_optimize of all %d problems, eps = 1e-5, CG solved to 1e-10; `anderson` = the reference's default accelerator inside "
                           "the persistent kernels (csrc/batch.hip); wall seconds of the optimize call" % nprob)
            out["config"]["time_to_solution_tight_cg"] = tts
        except Exception as e:                                  # a reported extra must not take the line down
            out["config"]["time_to_solution_tight_cg"] = dict(error="%s: %s" % (type(e).__name__, e))
    if not args.no_cpu_baseline and ctx.world == 1:
        def cpu_leg(out=out, probs=probs):
            from oracle import cosmo_oracle as O
            from tests import util
            OC = _native_oracle()
            nsamp, its, secs = (8 if args.small else 512), 0, 0.0
            for p in probs[:nsamp]:
                ws = O.Workspace(p["P"], p["q"], p["A"], p["b"], util.oracle_cones(p["sets"]), oracle_settings(O, warmup + steps))
                c = OC.run(ws, native=True)
                its += c["iter"]; secs += c["iter_time"]
            out["cpu_baseline"] = dict(value=its / secs / nprob, unit="ADMM iterations/s (of the whole batch)", cores=1, kind="port",
                                       sample="compiled C loop (gcc -O3 -march=native; oracle/cosmo_oracle_c.c), %d problems x %d iterations (+ init step), %.2f s of loop time, "
                                              "scaled to %d problems solved one after the other (the reference's own batch mode)" % (nsamp, warmup + steps, secs, nprob))
        args.deferred.append(cpu_leg)
    B.close()
    return out


def cfg3_scaling_model(cj, kry_all, elapsed, world, slots_per_gpu=256):
    """What bounds a batch step, from the MEASURED per-problem Krylov counts of the timed window: one persistent workgroup per problem and one workgroup per
    CU (the problem's LDS image fills the CU), so a rank's step takes  t_k * max(longest chain on the rank, work of the rank / 256 CU slots)  with t_k = the
    measured seconds per Krylov iteration of the slowest problem.  The straggler's serial chain does not shrink with more GPUs: the bound on the sharded
    speed-up is ~1 as long as  max K_p >> sum K_p / 256  (SURVEY 8e promised "~linear"; this is the measured reason why not)."""
    K = np.asarray(kry_all, dtype=np.float64)
    kmax = max(float(K.max()), 1.0)
    t_k = elapsed / max(float(max(K[lo:hi].max() if hi > lo else 0.0 for lo, hi in (cj.model.shard_range(K.size, r, world) for r in range(world)))), 1.0)
    out = dict(seconds_per_krylov_iteration=round(t_k, 9), longest_chain_krylov_iterations=int(kmax), total_krylov_iterations=int(K.sum()),
               cu_slot_utilisation_this_run=round(float(K.sum()) * t_k / (slots_per_gpu * world * elapsed), 4), predicted={})
    t1 = None
    for N in (1, 2, 4, 8):
        per_rank = [K[lo:hi] for lo, hi in (cj.model.shard_range(K.size, r, N) for r in range(N))]
        tN = t_k * max(max((float(k.max()) if k.size else 0.0), float(k.sum()) / slots_per_gpu) for k in per_rank)
        t1 = tN if N == 1 else t1
        out["predicted"]["%d" % N] = dict(ms_per_window=round(1e3 * tN, 3), chain_limited=bool(all((k.max() if k.size else 0) >= k.sum() / slots_per_gpu for k in per_rank)),
                                         speedup_bound=round(t1 / tN, 3))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cfg4 / cfg5: SDPs (matrix-sign projections on the fp64 matrix cores)
# ---------------------------------------------------------------------------------------------------------------------
_SHM_SEQ = [0]
TRANSPORT_NAME = {0: "none", 1: "rccl", 2: "host-staged shared memory (dry run, one GPU)"}


def _setup_sharding(ctx, model, dist, shard):
    """Communicator + partition of a set-up model (collective).  Returns the known-answer check of the exchange path, taken right after
    comm_init and BEFORE the handle is converted: every N > 1 line carries its own evidence that the collectives deliver the right sums and
    the same bits on every rank (the replicated n-side of the loop relies on that)."""
    import cosmo_jl_amd as cj
    if ctx.shm:
        _SHM_SEQ[0] += 1
        name = [("/cosmo_bench_%d_%d" % (os.getpid(), _SHM_SEQ[0])) if ctx.rank == 0 else None]
        dist.broadcast_object_list(name, src=0)
        model.handle.comm_init_hostshm(ctx.rank, ctx.world, name[0])
    else:
        cj.model._comm_for(model, dist)
    check = comm_known_answer_check(ctx, model.handle, model.n)
    if shard == "rows":
        model.handle.set_row_shard(cj.partition_cones_contiguous(cj.model.row_shard_costs(model.sets), ctx.world))
    else:
        model.handle.set_cone_shard(cj.partition_cones_contiguous(cj.cone_costs(model.sets), ctx.world))
    return check


def comm_known_answer_check(ctx, h, count):
    """cosmo_hip_comm_allreduce_check on every rank (an all-reduce of `count` reals through the loop's own exchange path: an exactly
    representable sum, and a fractional one whose bits must agree on all ranks), combined over the ranks."""
    try:
        mine = h.comm_allreduce_check(count)
        err = None
    except Exception as e:                      # a failing collective is evidence too; the other ranks must not wait for this one forever
        mine, err = None, "%s: %s" % (type(e).__name__, e)
    every = ctx.all_gather((mine, err))
    errs = [e for _, e in every if e]
    res = [r for r, _ in every if r]
    out = dict(count=int(count))
    if errs or not res:
        out["selftest"] = "FAILED: " + "; ".join(errs or ["no result"])
        return out
    v = res[0]["rccl_version_code"]
    out.update(transport_name=TRANSPORT_NAME.get(res[0]["transport"], str(res[0]["transport"])),
               rccl_version=("%d.%d.%d" % (v // 10000, (v // 100) % 100, v % 100)) if v else None,
               exact_sum_mismatches=sum(r["exact_mismatches"] for r in res), fractional_sum_outside_bound=sum(r["inexact_outside_bound"] for r in res),
               result_bits_identical_on_all_ranks=len({r["hash"] for r in res}) == 1)
    bad = out["exact_sum_mismatches"] or out["fractional_sum_outside_bound"] or not out["result_bits_identical_on_all_ranks"]
    out["selftest"] = ("FAILED: known-answer all-reduce of %d reals came back wrong" % count) if bad else "ok"
    return out


def _bits_hash(*arrays):
    import hashlib
    hsh = hashlib.sha256()
    for a in arrays:
        hsh.update(np.ascontiguousarray(a).tobytes())
    return hsh.hexdigest()[:16]


def _run_sdp(ctx, model, steps, warmup, dist=None, shard="rows"):
    import cosmo_jl_amd as cj
    cj.model.setup(model)
    comm_check = None
    if dist is not None and ctx.world > 1:
        comm_check = _setup_sharding(ctx, model, dist, shard)
    h = model.handle
    h.bench_comm_check = comm_check
    h.set_iterates(model.x, model.s, model.mu)
    h.admm_init()
    gpu_prewarm(h)
    h.admm_iterate_checked(warmup)
    s0 = h.get_stats()
    c0 = h.comm_stats_ex()
    h.polar_dataflow_stats(reset=True)                             # event timing of the persistent sign-iteration launch: the timed window only
    elapsed = ctx.timed(lambda: h.admm_iterate_checked(steps))
    s1 = h.get_stats()
    c1 = h.comm_stats_ex()
    assert s1["admm_iters"] - s0["admm_iters"] == steps
    kbar = (s1["kkt_iters_total"] - s0["kkt_iters_total"]) / max(1, s1["kkt_solves"] - s0["kkt_solves"])
    h.bench_comm = dict(c1, bytes_per_iteration=round((c1["bytes"] - c0["bytes"]) / steps, 1),
                        collectives_per_iteration=round((c1["collectives"] - c0["collectives"]) / steps, 3))
    if comm_check is not None:
        h.bench_comm.update(comm_check)
    return h, elapsed, kbar


def cfg5_sharded_parity_leg(ctx, args, prob, iters=12):
    """Parity evidence INSIDE the N > 1 line: the same problem run unsharded on rank 0 and sharded over all ranks, `iters` ADMM iterations with a
    TIGHT CG (tol_constant = 1e-10, tol_exponent = 0: both sides solve every KKT system to ~1e-10, so the iterates are comparable at 1e-7 although
    the summation order of A'y changes with the partition -- the tolerance tests/test_gpu_sharding.py asserts), then
      sharded_vs_single_max_rel_dev = max(|w_sharded - w_single|_inf / |w_single|_inf, same for s)        [expected <= 1e-7]
      ranks_bit_identical: every rank's gathered (w, s) hashes to the same value (the replicated n-side and the all-gathered rows).
    The loop being sharded: src/convexset.jl:885-891 (projections), src/linear_solver/kktsolver_indirect.jl:52-54, 81-83 (the A' / A products)."""
    import cosmo_jl_amd as cj
    st = fixed_work_settings(cj, kkt_solver=cj.with_options(cj.CGIndirectKKTSolver, tol_constant=1e-10, tol_exponent=0.0)); st.device = ctx.local_rank
    ref = None
    if ctx.rank == 0:
        m1 = cj.Model(); m1.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
        cj.model.setup(m1)
        h1 = m1.handle
        h1.set_iterates(m1.x, m1.s, m1.mu); h1.admm_init(); h1.admm_iterate_checked(iters)
        w1, _, s1, _ = h1.get_iterates()
        k1 = h1.get_stats()["kkt_iters_total"]
        ref = (w1, s1, k1)
        h1.close()
    ctx.barrier()
    md = cj.Model(); md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
    cj.model.setup(md)
    _setup_sharding(ctx, md, ctx.dist, args.shard)
    h = md.handle
    h.set_iterates(md.x, md.s, md.mu); h.admm_init(); h.admm_iterate_checked(iters)
    w, _, s, _ = h.get_iterates()                                      # collective: every rank receives the global vectors
    kk = h.get_stats()["kkt_iters_total"]
    h.close()
    hashes = ctx.all_gather(_bits_hash(w, s))
    if ctx.rank != 0:
        return None
    w1, s1, k1 = ref
    dev = max(float(np.max(np.abs(w - w1)) / max(np.max(np.abs(w1)), 1e-300)), float(np.max(np.abs(s - s1)) / max(np.max(np.abs(s1)), 1e-300)))
    if not np.isfinite(dev):
        dev = float("inf")
    return dict(sharded_vs_single_max_rel_dev=dev, expected_at_most=1e-7, ok=bool(dev <= 1e-7 and len(set(hashes)) == 1), ranks_bit_identical=len(set(hashes)) == 1,
                admm_iterations=iters, krylov_iterations=dict(single=int(k1), sharded=int(kk)),
                settings="tight CG (tol_constant 1e-10, tol_exponent 0), otherwise the fixed-work settings of the timed run; w and s compared in the "
                         "infinity norm relative to the single-GPU run of rank 0")


NO_PREWARM = [False]


def gpu_prewarm(h, seconds=0.3):
    """Bring the GPU clocks up before a short timed window: back-to-back launches of the sign iteration's product kernel on the handle's WORK
    matrices (the measurement hook of the library; the next projection overwrites them, no ADMM state is touched)."""
    if NO_PREWARM[0]:          # profiling runs (rocprofv3 --stats): per-kernel averages must come from the loop's own launches
        return
    ps = h.polar_stats()
    which = 1 if ps["batch_cones"] > 0 else (0 if ps["large_cones"] > 0 else None)
    if which is None:
        return
    t, _ = h.time_psd_product(which, 20)
    h.time_psd_product(which, max(20, min(20000, int(seconds / max(t, 1e-6)))))


def shardable_share(h, ms_per_iter, iters=10):
    """Measured split of the 1-GPU iteration: HIP events around every loop kernel (exact-launch mode) give the milliseconds per iteration of the
    projections (shard with the cones) and of the row kernels (k_z, rhs, A' y2, A x_tl / s_tl / w_s, primal check: shard with the rows).  The
    Krylov kernels are inflated in that mode (a host round trip per Krylov iteration), so the shares are taken against `ms_per_iter`, the UNPROFILED
    iteration time of the same handle; what is left is the replicated n-side (CG, dual check).  Returns (f_cones, f_rows, ms by class)."""
    h.set_profiling(1)
    h.admm_iterate_checked(iters)
    kt = h.get_kernel_times()
    h.set_profiling(0)
    if not kt or ms_per_iter <= 0:
        return None, None, {}
    ms = {k: 1e3 * v[0] / iters for k, v in kt.items()}
    proj = sum(v for k, v in ms.items() if k.startswith("proj_"))
    rows = proj + sum(v for k, v in ms.items() if k.startswith(("admm_z", "admm_x_rhs", "spmv_AT", "tail", "check_primal", "rho_apply")))
    return min(proj / ms_per_iter, 0.999), min(rows / ms_per_iter, 0.999), {k: round(v, 4) for k, v in ms.items()}


def float32_extra(ctx, args, prob, st, steps, warmup):
    """The same workload on the Float32 instantiation (libcosmo_hip_f32.so, COSMO.Model{Float32}): reported NEXT to the fp64 number of
    the contract line, never instead of it (`dtype` of this sub-object is "f32")."""
    import cosmo_jl_amd as cj
    m32 = cj.Model(dtype=np.float32)
    m32.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
    h32, el32, k32 = _run_sdp(ctx, m32, steps, warmup)
    ps = h32.polar_stats()
    out = dict(value=steps / el32, ms_per_step=1e3 * el32 / steps, steps=steps, warmup=warmup, dtype="f32", unit="ADMM iterations/s",
               mean_cg_iters_per_admm_iter=round(k32, 3), polar={k: ps[k] for k in ("fallback_rounds", "verified", "unverified")},
               note="same instance and fixed-work settings on libcosmo_hip_f32.so (every kernel instantiated for float, v_mfma_f32_16x16x4_f32 products)")
    h32.close()
    return out


def bench_cfg4(ctx, args, steps, warmup):
    import cosmo_jl_amd as cj
    d = 400 if args.small else 2000
    prob = cj.problems.closest_correlation(d=d)
    st = fixed_work_settings(cj); st.device = ctx.local_rank
    model = cj.Model(); model.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
    h, elapsed, kbar = _run_sdp(ctx, model, steps, warmup)
    dump_handle_outputs(ctx, args, model)
    value = whole_job_value(ctx.world, steps, elapsed)
    out = dict(value=value, ms_per_step=1e3 * elapsed / steps, steps=steps, warmup=warmup, scaling="weak")
    if ctx.rank != 0:
        return out
    ps = h.polar_stats()
    if args.full:
        t_prod, fl = h.time_psd_product(0, 20)
        per_gpu = value / ctx.world
        out["roofline"] = dict(bound="mfma", kernel="k_symm_gemm<EPI, %d, %d> (symmetric product of the sign iteration, v_mfma_f64_16x16x4_f64)" % (ps["tile_side"], ps["k_split"]),
                               achieved=round(fl / t_prod / 1e12, 2), peak=F64_MFMA_PEAK_TF, unit="TFLOP/s", frac=round(fl / t_prod / 1e12 / F64_MFMA_PEAK_TF, 4), traffic=None,
                               peak_sustained_measured=F64_MFMA_SUSTAINED_TF, frac_of_sustained=round(fl / t_prod / 1e12 / F64_MFMA_SUSTAINED_TF, 4),
                               flops_per_launch=fl, avg_launch_us=round(1e6 * t_prod, 2), launches_timed=20,
                               products_per_projection=ps["products_last_large"],
                               performed_tflops_whole_iteration=round(ps["products_last_large"] * fl * per_gpu / 1e12, 2),
                               useful_tflops_reference_algorithm=round(psd_useful_flops(d) * per_gpu / 1e12, 3),
                               useful_frac_of_peak=round(psd_useful_flops(d) * per_gpu / 1e12 / F64_MFMA_PEAK_TF, 4))
    out["config"] = {"workload": "cfg4: closest-correlation SDP, one PsdConeTriangle d=%d (n=%d, m=%d), CG indirect KKT" % (d, model.n, model.m),
                     "parallelism": "replicas x%d (a single cone does not shard; SURVEY 8e)" % ctx.world,
                     "mean_cg_iters_per_admm_iter": round(kbar, 3), "polar": dict({k: ps[k] for k in ("schedule_steps", "fallback_rounds", "verified", "unverified", "err_max_e18")}, lifting_depth=h.polar_depth_stats())}
    if not args.no_cpu_baseline and ctx.world == 1:
        args.deferred.append(lambda out=out, prob=prob: out.__setitem__("cpu_baseline", compiled_cpu_baseline(prob, 16 if not args.small else 20, "cfg4", "cfg4", args,
                                                                                                                iters_all=2 if not args.small else 20)))
    h.close()
    if ctx.world == 1 and not args.no_float32:
        out["float32"] = float32_extra(ctx, args, prob, st, steps, warmup)
    return out


def bench_cfg5(ctx, args, steps, warmup):
    import cosmo_jl_amd as cj
    kw = dict(ncliques=40, n_total=6000, n_zero=100, n_nonneg=500) if args.small else {}
    prob = cj.problems.chordal_sdp(**kw)
    st = fixed_work_settings(cj); st.device = ctx.local_rank
    single, share = None, None
    if ctx.world > 1 and args.full:
        # self-contained speed-up: rank 0 times the UNSHARDED problem first (the other ranks wait at the barrier inside timed()), and measures
        # which share of that iteration shards
        if ctx.rank == 0:
            m1 = cj.Model(); m1.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
            cj.model.setup(m1)
            h1 = m1.handle
            h1.set_iterates(m1.x, m1.s, m1.mu); h1.admm_init(); gpu_prewarm(h1); h1.admm_iterate_checked(warmup)
            ctx.torch.cuda.synchronize()
            t0 = time.perf_counter(); h1.admm_iterate_checked(steps); ctx.torch.cuda.synchronize()
            single = steps / (time.perf_counter() - t0)
            share = shardable_share(h1, 1e3 / single)
            h1.close()
        ctx.barrier()
    model = cj.Model(); model.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
    h, elapsed, kbar = _run_sdp(ctx, model, steps, warmup, dist=ctx.dist, shard=args.shard)
    dump_handle_outputs(ctx, args, model)
    value = steps / elapsed                                                # ONE problem, all ranks work on it: strong scaling
    out = dict(value=value, ms_per_step=1e3 * elapsed / steps, steps=steps, warmup=warmup, scaling="strong")
    rank_seconds = ctx.rank_seconds()
    parity = None
    if ctx.world > 1 and args.full and os.environ.get("COSMO_BENCH_PARITY", "1") != "0":     # (COSMO_BENCH_PARITY=0: throughput only -- for bisecting a failing multi-GPU run)
        try:                                                               # a second communicator next to the timed handle's (both stay valid)
            parity = cfg5_sharded_parity_leg(ctx, args, prob)
        except Exception as e:
            parity = dict(ok=False, error="%s: %s" % (type(e).__name__, e))
    if ctx.rank != 0:
        h.close()
        return out
    ps = h.polar_stats()
    dk = np.asarray(prob["clique_dims"], dtype=np.float64)
    useful = float(np.sum([psd_useful_flops(d) for d in dk]))
    if ctx.world == 1:
        par = "single GPU"
    elif args.shard == "rows":
        par = ("cones AND their rows of A / s / mu / rho sharded over %d ranks (contiguous cone ranges balanced by sum d^3 + 8 rows; n-side CG replicated on the "
               "assembled operator; one RCCL all-reduce of an n-vector per iteration, one more per residual check; csrc/rowshard.hip)" % ctx.world)
    else:
        par = ("cliques sharded over %d ranks (contiguous cone ranges balanced by sum d^3; affine step replicated; one RCCL broadcast group of the "
               "projected slices of s per iteration)" % ctx.world)
    out["config"] = {"workload": "cfg5: chordal SDP n=%d m=%d, %d PSD cliques d in [%d, %d] + Zero/Nonneg rows, CG indirect KKT" % (model.n, model.m, dk.size, dk.min(), dk.max()),
                     "workload_detail": "nnz(A)=%d, PsdConeTriangle cliques, ZeroSet(%d) + Nonnegatives(%d)" % (model.A.nnz, prob["sets"][0].dim, prob["sets"][1].dim),
                     "parallelism": par,
                     "mean_cg_iters_per_admm_iter": round(kbar, 3), "comm": h.bench_comm, "row_shard": h.row_shard_info(), "cg_persist": h.cg_persist_stats(),
                     "cg_assembled_operator": h.fold_stats(), "kkt_solver": h.kkt_recurrence(),
                     "polar": dict({k: ps[k] for k in ("batch_cones", "schedule_steps", "products_last_batch", "fallback_rounds", "verified", "unverified", "err_max_e18")},
                                   lifting_depth=h.polar_depth_stats())}
    if ctx.world > 1:
        out["config"]["rank_seconds"] = rank_seconds
        # the same evidence as FLAT scalars: the driver's parsed copy of the line keeps the scalar entries of `config` (nested objects are dropped there)
        comm = h.bench_comm or {}
        if args.full:                                                      # a plain run has no parity leg: no parity verdict either
            out["config"]["parity"] = parity
            out["config"]["parity_ok"] = bool(parity and parity.get("ok") and comm.get("selftest") == "ok")
            out["config"]["parity_sharded_vs_single_max_rel_dev"] = (parity or {}).get("sharded_vs_single_max_rel_dev")
            out["config"]["parity_expected_at_most"] = 1e-7
            out["config"]["parity_ranks_bit_identical"] = (parity or {}).get("ranks_bit_identical")
        out["config"]["comm_selftest"] = comm.get("selftest")
        out["config"]["comm_transport"] = comm.get("transport_name")
        out["config"]["comm_rccl_version"] = comm.get("rccl_version")
        out["config"]["comm_bytes_per_iteration"] = comm.get("bytes_per_iteration")
        out["config"]["rank_seconds_min_max"] = "%.6f / %.6f" % (rank_seconds["min"], rank_seconds["max"])
    if single is not None:
        out["config"]["single_gpu_same_workload"] = round(single, 3)
        out["config"]["speedup_vs_single_gpu"] = round(value / single, 3)
        if share is not None and share[0] is not None:
            f = share[1] if args.shard == "rows" else share[0]
            out["config"]["shardable_share_of_single_gpu_iteration"] = dict(
                projections=round(share[0], 4), projections_and_row_kernels=round(share[1], 4), used=round(f, 4), ms_per_iteration_by_kernel_class=share[2],
                predicted_speedup_bound=round(1.0 / ((1.0 - f) + f / ctx.world), 3),
                note="f = (event-timed ms per iteration of the kernels that shard) / (unprofiled ms per iteration of the same 1-GPU run); bound "
                     "1 / ((1 - f) + f / N) ignores the exchange and load imbalance; the replicated rest is the n-side CG + dual check")
    # ---- roofline: the kernel class with the largest share of the step's time is named first, the other under `other` ----------------------
    ms_step = 1e3 * elapsed / steps
    products = None
    if args.full and ps["batch_cones"] > 0:
        # the product kernel timed as the IN-LOOP MIX: per repetition one Y = U^2 and the two alpha A B + beta Cin products of a step of the sign
        # iteration with their real operands (time_psd_product mode 2), not back-to-back launches of the cheapest flavour
        t_prod, fl = h.time_psd_product(2, 20)
        t_sq, _ = h.time_psd_product(1, 20)
        own = dk if ctx.world == 1 else None                      # rank 0's cliques only in sharded runs: useful flops not attributed there
        useful_prod = float(np.sum(dk * dk * (dk + 1.0))) if own is not None else None
        nprod = ps["products_last_batch"]
        df = h.polar_dataflow_stats()
        if df["enabled"] and df["timed_launches"] > 0:
            # round 6: the main schedule is ONE persistent dependency-driven launch (k_polar_dataflow); its duration comes from the HIP events the library records
            # around every such launch of the timed window; a "product" below = the launch divided by its number of products
            t_launch, npl = df["avg_launch_seconds"], df["products_per_launch"]
            t_eq = t_launch / npl
            products = dict(bound="mfma", kernel="k_polar_dataflow<4> (the %d products of the sign iteration's main schedule in ONE persistent launch of %d workgroups: per-XCD in-order "
                                                "tile queue, per-cone completion counters, operands read with sc1 loads; tile arithmetic = k_symm_gemm_batch_r<EPI, 4>, same bits)"
                                                % (npl, df["workgroups"]),
                            timing="HIP events recorded by the library around every persistent launch of the timed window (%d launches)" % df["timed_launches"],
                            useful_flops_per_launch=(useful_prod * npl if useful_prod else None), performed_over_useful=(round(fl / useful_prod, 3) if useful_prod else None),
                            useful_frac_per_product=(round(useful_prod / t_eq / 1e12 / F64_MFMA_PEAK_TF, 4) if useful_prod else None),
                            achieved=round(fl / t_eq / 1e12, 2), peak=F64_MFMA_PEAK_TF, unit="TFLOP/s", frac=round(fl / t_eq / 1e12 / F64_MFMA_PEAK_TF, 4), traffic=None,
                            peak_sustained_measured=F64_MFMA_SUSTAINED_TF, frac_of_sustained=round(fl / t_eq / 1e12 / F64_MFMA_SUSTAINED_TF, 4),
                            flops_per_launch=fl * npl, avg_launch_us=round(1e6 * t_launch, 2), us_per_product_equivalent=round(1e6 * t_eq, 2),
                            launches_timed=df["timed_launches"], products_per_projection=nprod, share_of_step=round(1e3 * t_launch / ms_step, 4),
                            launch_per_product_form=dict(avg_launch_us=round(1e6 * t_prod, 2), avg_launch_us_square_only=round(1e6 * t_sq, 2), frac=round(fl / t_prod / 1e12 / F64_MFMA_PEAK_TF, 4),
                                                         note="k_symm_gemm_batch_r<EPI, 4>, one launch per product (COSMO_HIP_POLAR_DATAFLOW=0; still used by the repair rounds): in-loop mix "
                                                              "20 x (Y = U^2, T = c Y^2 + b Y, U' = U T + a U), HIP events"),
                            hbm_algorithmic_bytes_per_launch=(24.0 * float(np.sum(dk * dk)) * npl if own is not None else None),
                            hbm_frac_algorithmic=(round(24.0 * float(np.sum(dk * dk)) / t_eq / 1e9 / HBM_PEAK_GBS, 4) if own is not None else None),
                            useful_tflops_reference_algorithm=round(useful * value / 1e12, 3), useful_frac_of_peak=round(useful * value / 1e12 / F64_MFMA_PEAK_TF, 5))
        else:
            products = dict(bound="mfma", kernel="k_symm_gemm_batch_r<EPI, 4> (ragged block-balanced tiles: one workgroup per list of <= 16 blocks of 16 x 16 of one of rank 0's "
                                                "cliques; upper blocks only on the diagonal; four workgroups per CU, tiles launched by decreasing cost)",
                            timing="in-loop mix: 20 x (Y = U^2, T = c Y^2 + b Y, U' = U T + a U) on the batch's work matrices, HIP events on the library's stream",
                            useful_flops_per_launch=useful_prod, performed_over_useful=(round(fl / useful_prod, 3) if useful_prod else None),
                            useful_frac_per_product=(round(useful_prod / t_prod / 1e12 / F64_MFMA_PEAK_TF, 4) if useful_prod else None),
                            achieved=round(fl / t_prod / 1e12, 2), peak=F64_MFMA_PEAK_TF, unit="TFLOP/s", frac=round(fl / t_prod / 1e12 / F64_MFMA_PEAK_TF, 4), traffic=None,
                            peak_sustained_measured=F64_MFMA_SUSTAINED_TF, frac_of_sustained=round(fl / t_prod / 1e12 / F64_MFMA_SUSTAINED_TF, 4),
                            flops_per_launch=fl, avg_launch_us=round(1e6 * t_prod, 2), avg_launch_us_square_only=round(1e6 * t_sq, 2), launches_timed=60,
                            products_per_projection=nprod, share_of_step=round(nprod * 1e3 * t_prod / ms_step, 4),
                            # the other roof of the same launch: Y = U^2 reads U once and writes Y once (8 B x sum d^2 each); the alpha A B + beta Cin products
                            # read up to three distinct matrices: 2 / 3 / 4 x 8 B x sum d^2 for the three launches of a step => 3 matrices per product on average
                            hbm_algorithmic_bytes_per_launch=(24.0 * float(np.sum(dk * dk)) if own is not None else None),
                            hbm_frac_algorithmic=(round(24.0 * float(np.sum(dk * dk)) / t_prod / 1e9 / HBM_PEAK_GBS, 4) if own is not None else None),
                            useful_tflops_reference_algorithm=round(useful * value / 1e12, 3), useful_frac_of_peak=round(useful * value / 1e12 / F64_MFMA_PEAK_TF, 5))
    krylov = None
    pmc5 = None
    if args.full and not args.small:
        import glob
        for fpmc in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_cfg5_pmc_traffic.json"))):       # committed PMC passes (constants, like cfg2's)
            try:
                with open(fpmc) as fh:
                    pmc5 = (json.load(fh), os.path.relpath(fpmc, ROOT))
            except Exception:
                pass
    if products is not None and pmc5 is not None:
        try:
            kk = pmc5[0]["kernels"]
            if products["kernel"].startswith("k_polar_dataflow"):
                e = kk["k_polar_dataflow<4>"]
                products["traffic"] = round(e["hbm_bytes_per_launch"], 1)
                products["mfma_busy_frac_pmc"] = round(e["mfma_busy_frac"], 4)
            else:
                e0, e1 = kk["k_symm_gemm_batch_r<0, 4>"], kk["k_symm_gemm_batch_r<1, 4>"]
                products["traffic"] = round((e0["hbm_bytes_per_launch"] + 2.0 * e1["hbm_bytes_per_launch"]) / 3.0, 1)      # the in-loop mix: one EPI 0 + two EPI 1 launches
                products["mfma_busy_frac_pmc"] = round((e0["mfma_busy_frac"] + 2.0 * e1["mfma_busy_frac"]) / 3.0, 4)
            products["traffic_source"] = pmc5[1]
        except Exception:
            pass
    if ctx.world == 1 and args.full:
        try:
            t_k, b_k, nl = min(h.time_krylov(200) for _ in range(3))
            fs = h.fold_stats()
            rec = h.kkt_recurrence()                               # the kernel names come from the handle (cosmo_hip_kkt_recurrence)
            krylov = dict(bound="hbm", limited_by="latency: a chain of dependent launches and load round trips, not bandwidth",
                          kernel=("%s: ONE Krylov iteration of the reduced CG solve on the assembled operator M = P + sigma I + A' rho A (%d nonzeros), %d launch(es) [%s]"
                                  % (("k_" + rec.split(", k_", 1)[1]) if ", k_" in rec else rec, fs["nnz"], nl, rec.split(", k_")[0])) if fs["enabled"] else "one Krylov iteration of cg! (%d launches) [%s]" % (nl, rec),
                          achieved=round(b_k / t_k / 1e9, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(b_k / t_k / 1e9 / HBM_PEAK_GBS, 4), traffic=None,
                          algorithmic_bytes_per_launch=b_k, avg_launch_us=round(1e6 * t_k, 3), launches_timed=200,
                          timing="best of 3 x 200 Krylov iterations as the loop enqueues them (captured chain), tolerance 0, HIP events on the library's stream; "
                                 "'launch' = one Krylov iteration = %d dependent kernel(s) incl. the boundaries" % nl,
                          krylov_iterations_per_step=round(kbar, 2), share_of_step=round(kbar * 1e3 * t_k / ms_step, 4),
                          note="a chain of dependent round trips (the eight L2s are invalidated at every kernel boundary, operands come back through the fabric / "
                               "Infinity Cache): the HBM fraction is reported because the contract asks for it; what bounds the pair is launch + load latency")
            if pmc5 is not None and fs["enabled"]:
                key = "krylov_iteration_one_launch" if nl == 1 else "krylov_iteration_pair"
                if key in pmc5[0]:
                    krylov["traffic"] = pmc5[0][key]["hbm_bytes_per_krylov_iteration"]
                    krylov["traffic_source"] = pmc5[1]
        except Exception as e:
            krylov = dict(error="%s: %s" % (type(e).__name__, e))
    cands = [r for r in (krylov, products) if r and "share_of_step" in r]
    if cands:
        cands.sort(key=lambda r: -r["share_of_step"])
        out["roofline"] = dict(cands[0])
        if len(cands) > 1:
            out["roofline"]["other"] = {cands[1]["kernel"].split(" ")[0]: cands[1]}
    elif products:
        out["roofline"] = products
    if not args.no_cpu_baseline and ctx.world == 1:
        def cpu_leg(out=out, prob=prob, value=value):
            cb = compiled_cpu_baseline(prob, 3 if not args.small else 10, "cfg5", "cfg5", args, iters_all=1 if not args.small else 10)
            cb["kkt"] = "CGIndirectKKTSolver (the solver of the GPU path; kktsolver_indirect.jl:36-88)"
            try:
                cb["direct_kkt"] = direct_kkt_cpu_baseline(prob, 10 if not args.small else 20, "cfg5")
                out["config"]["gpu_over_cpu_direct_kkt"] = round(value / cb["direct_kkt"]["value"], 2)
            except Exception as e:
                cb["direct_kkt"] = dict(error="%s: %s" % (type(e).__name__, e))
            out["config"]["gpu_over_cpu"] = round(value / cb["value"], 2)
            out["cpu_baseline"] = cb
        args.deferred.append(cpu_leg)
    if ctx.world == 1:
        h.close()
        if args.full:
            try:
                out["pcg"] = jacobi_pcg_extra(ctx, args, prob, steps, warmup)
            except Exception as e:
                out["pcg"] = dict(error="%s: %s" % (type(e).__name__, e))
        if KKT_CHOICE["name"] == "cg" and not args.no_variants:
            try:
                out["single_reduction_cg"] = single_reduction_extra(ctx, args, prob, steps, warmup, value, kbar)
            except Exception as e:
                out["single_reduction_cg"] = dict(error="%s: %s" % (type(e).__name__, e))
        if not args.no_variants:
            try:
                out["adaptive_lifting_depth"] = adaptive_depth_extra(ctx, args, prob, steps, warmup, value)
            except Exception as e:
                out["adaptive_lifting_depth"] = dict(error="%s: %s" % (type(e).__name__, e))
            try:
                out["eigen_projection"] = eigen_projection_extra(ctx, args, prob, value)
            except Exception as e:
                out["eigen_projection"] = dict(error="%s: %s" % (type(e).__name__, e))
            if not args.small:
                try:
                    out["time_to_solution"] = time_to_solution_extra(ctx, args, prob)
                except Exception as e:
                    out["time_to_solution"] = dict(error="%s: %s" % (type(e).__name__, e))
    if ctx.world == 1 and not args.no_float32:
        out["float32"] = float32_extra(ctx, args, prob, st, steps, warmup)
    h.close()
    return out


def eigen_projection_extra(ctx, args, prob, value_sign):
    """The same workload with the eigendecomposition-based PSD projection the reference performs (src/convexset.jl:163-189, 243-263; north_star's wording of
    a7 / a8) instead of the verified matrix-sign iteration: Settings.psd_projection = 'eigen' = cosmo_hip_set_psd_projection(EIGEN) -- one workgroup per
    clique runs a block one-sided Jacobi eigensolver (csrc/psd.hip), nnz_lambda is counted from the eigenvalues.  A short window (the projections take
    several times longer): the PRICE of that shape on this chip, re-measured by every run."""
    import cosmo_jl_amd as cj
    steps, warmup = (4, 2) if not args.small else (3, 1)
    st = fixed_work_settings(cj, psd_projection="eigen"); st.device = ctx.local_rank
    md = cj.Model(); md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
    h, el, kb = _run_sdp(ctx, md, steps, warmup)
    ps = h.psd_stats() if hasattr(h, "psd_stats") else None
    out = dict(value=round(steps / el, 3), ms_per_step=round(1e3 * el / steps, 6), steps=steps, warmup=warmup, unit="ADMM iterations/s", dtype="f64",
               vs_sign_iteration=round(steps / el / value_sign, 4), mean_cg_iters_per_admm_iter=round(kb, 3), jacobi=ps,
               note="OPT-IN psd_projection='eigen': Jacobi eigendecomposition of every clique (exact nnz_lambda) instead of the verified matrix-sign iteration")
    h.close()
    return out


def adaptive_depth_extra(ctx, args, prob, steps, warmup, value_fixed):
    """The same workload with the per-cone adaptive lifting depth of the sign iteration (COSMO_HIP_POLAR_ADAPT=1; the a-posteriori check and with it
    the error bound of every projection are unchanged) and the compact repair launches of round 5: what VERDICT r04 item 5 asks to be decided by
    measurement.  Same literal cg!, same iterates up to the projections' 64 d eps bound."""
    import cosmo_jl_amd as cj
    os.environ["COSMO_HIP_POLAR_ADAPT"] = "1"
    try:
        st = fixed_work_settings(cj); st.device = ctx.local_rank
        md = cj.Model(); md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
        h, el, kb = _run_sdp(ctx, md, steps, warmup)
        ps, dp = h.polar_stats(), h.polar_depth_stats()
        out = dict(value=round(steps / el, 3), ms_per_step=round(1e3 * el / steps, 6), steps=steps, warmup=warmup, unit="ADMM iterations/s", dtype="f64",
                   vs_fixed_depth=round(steps / el / value_fixed, 4), mean_cg_iters_per_admm_iter=round(kb, 3),
                   polar=dict({k: ps[k] for k in ("products_last_batch", "fallback_rounds", "verified", "unverified", "err_max_e18")}, lifting_depth=dp),
                   note="OPT-IN COSMO_HIP_POLAR_ADAPT=1: every cone runs its own number of lifting steps (joins the batch's schedule late), failed verifications are "
                        "repaired by launches over the failing cones' tiles only, resuming with one more lifting step")
        h.close()
        return out
    finally:
        os.environ.pop("COSMO_HIP_POLAR_ADAPT", None)


def single_reduction_extra(ctx, args, prob, steps, warmup, value_literal, kbar_literal):
    """The same workload with the OPT-IN single-reduction (Chronopoulos-Gear) recurrence (kkt_kind CG_SR): ONE launch per Krylov iteration on the
    assembled operator (csrc/cg_sr.hip: k_sr_M, captured chain, device-side iteration index).  Round 6 measured it as a candidate default for
    assembled operators and rejected it -- slower per iteration (24-byte gathers) and more iterations at tight thresholds; the leg
    stays so that the decision is re-measured by every run."""
    import cosmo_jl_amd as cj
    st = fixed_work_settings(cj, kkt_solver=cj.CGSingleReductionKKTSolver); st.device = ctx.local_rank
    md = cj.Model(); md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
    h, el, kb = _run_sdp(ctx, md, steps, warmup)
    out = dict(value=round(steps / el, 3), ms_per_step=round(1e3 * el / steps, 6), steps=steps, warmup=warmup, unit="ADMM iterations/s", dtype="f64",
               kkt_solver=h.kkt_recurrence(), mean_cg_iters_per_admm_iter=round(kb, 3),
               vs_literal=round((steps / el) / value_literal, 4), krylov_iterations_per_step_minus_literal=round(kb - kbar_literal, 3))
    try:
        t_k, b_k, nl = min(h.time_krylov(200) for _ in range(3))
        out["us_per_krylov_iteration"] = round(1e6 * t_k, 3)
    except Exception as e:
        out["us_per_krylov_iteration"] = "%s: %s" % (type(e).__name__, e)
    h.close()
    return out


def time_to_solution_extra(ctx, args, prob):
    """BASELINE config 5 solved at the reference's DEFAULT settings (src/settings.jl:101-139: eps_abs = eps_rel = 1e-5, adaptive rho, check_termination 25,
    AndersonAccelerator{Type2{QRDecomp}, RestartedMemory} with safeguarding, :136-138) with the CG indirect solver: wall time of COSMO.optimize!'s loop on the
    device, status, iterations.  A side figure: the contract number above is iterations/s on fixed-work settings."""
    import cosmo_jl_amd as cj
    st = cj.Settings(kkt_solver=cj.CGIndirectKKTSolver, accelerator=cj.AndersonAccelerator, max_iter=6000, time_limit=120.0)
    st.device = ctx.local_rank
    md = cj.Model(); md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
    t0 = time.perf_counter(); cj.model.setup(md); t_setup = time.perf_counter() - t0
    gpu_prewarm(md.handle)
    t1 = time.perf_counter(); r = cj.optimize(md); t_solve = time.perf_counter() - t1
    a = md.handle.accel_stats()
    out = dict(status=r.status, seconds=round(t_solve, 3), iter_time_seconds=round(r.times.iter_time, 3), setup_seconds=round(t_setup, 3), iterations=int(r.iter),
               safeguarding_iterations=int(r.safeguarding_iter), objective=float(r.obj_val), r_prim=float(r.info.r_prim), r_dual=float(r.info.r_dual),
               rho_updates=len(r.info.rho_updates) - 1, krylov_iterations=int(r.kkt_iters_total), accelerated_steps=int(a["accelerated"]), declined=int(a["declined"]),
               settings="reference defaults: eps 1e-5, adaptive rho, AndersonAccelerator (mem 15, safeguarded), CGIndirectKKTSolver; max_iter 6000",
               unit="seconds to status (COSMO.optimize! loop on the device)", kkt_solver=md.handle.kkt_recurrence())
    md.handle.close()
    return out


def jacobi_pcg_extra(ctx, args, prob, steps, warmup):
    """The same workload with the OPT-IN Jacobi-preconditioned CG (kkt_kind CG_JACOBI; IterativeSolvers' PCGIterable with Pl = diag of the reduced
    operator): a DIFFERENT Krylov method for the same systems under the same true-residual stopping rule -- the reference passes no preconditioner
    (src/linear_solver/kktsolver_indirect.jl:70), so this number stands NEXT to the literal-cg! contract number, never in its place."""
    import cosmo_jl_amd as cj
    st = fixed_work_settings(cj, kkt_solver=cj.CGJacobiKKTSolver); st.device = ctx.local_rank
    md = cj.Model(); md.set(prob["P"], prob["q"], prob["A"], prob["b"], prob["sets"], st)
    h, el, kb = _run_sdp(ctx, md, steps, warmup)
    out = dict(value=round(steps / el, 3), ms_per_step=round(1e3 * el / steps, 6), steps=steps, warmup=warmup, unit="ADMM iterations/s", dtype="f64",
               kkt_solver="CG, Jacobi-preconditioned (OPT-IN kkt_kind CG_JACOBI; same operator, warm start and stopping rule ||r||_2 <= tol_k / ||rhs||)",
               mean_cg_iters_per_admm_iter=round(kb, 3))
    try:
        t_k, b_k, nl = min(h.time_krylov(200) for _ in range(3))
        out["us_per_krylov_iteration"] = round(1e6 * t_k, 3)
    except Exception as e:
        out["us_per_krylov_iteration"] = "%s: %s" % (type(e).__name__, e)
    h.close()
    return out


BENCH = {"cfg2": bench_cfg2, "cfg3": bench_cfg3, "cfg4": bench_cfg4, "cfg5": bench_cfg5}
# (steps, warmup) of the extra workloads: the iteration WINDOW is part of the workload -- cfg5 needs 169.5 Krylov iterations per ADMM iteration in
# iterations 11-50, 138 in 16-75 and 92 in 51-130 (after the rho update of iteration 40), i.e. 156 / 188 / 264 it/s for the same kernels -- so the
# windows stay those of round 2.  Ten warm-up iterations (60-80 ms) do not bring the clocks of an idling GPU back up (cfg5 read 155 it/s right after
# 10 s of CPU-baseline work against 166-170), so all cpu_baseline legs run AFTER the GPU work (args.deferred) and _run_sdp first spins the product
# kernel for ~0.3 s (gpu_prewarm; no ADMM state is touched)
EXTRA_STEPS = {"cfg2": (40, 10), "cfg3": (100, 25), "cfg4": (40, 10), "cfg5": (40, 10)}
HEADLINE = "cfg5"       # the workload north_star's targets are stated on (">= 10x ... on a 50k-var chordal SDP at 1xMI355X", ">= 6x at 8 GPUs on clique-sharded problems")


def relaunch_under_torchrun(n):
    """`python bench.py --gpus N` without a launcher: replace this process by `python -m torch.distributed.run --nproc-per-node N
    bench.py <same arguments>` (one process per GPU, rendezvous on 127.0.0.1 at a free port).  Rank 0 of that job prints the line."""
    import socket
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL across processes needs it on this driver
    os.environ.setdefault("OMP_NUM_THREADS", "4")
    os.environ["COSMO_BENCH_SELF_LAUNCHED"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush(); sys.stderr.flush()
    os.execv(sys.executable, cmd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", choices=["all", "cfg2", "cfg3", "cfg4", "cfg5"], default=None,
                    help="default: headline cfg5 at every N (N > 1: row-sharded, strong); extras cfg2 / cfg3 / cfg4 at N=1, cfg3_sharded + cfg2 / cfg4 replicas at N>1")
    ap.add_argument("--shard", choices=["rows", "cones"], default="rows",
                    help="cfg5 at N>1: rows = every rank owns its cones AND their rows of A / s / mu / rho, one all-reduce of an n-vector per "
                         "iteration (SURVEY 8e option 2 on a replicated CG); cones = projections only, one broadcast group of s per iteration (option 1)")
    ap.add_argument("--small", action="store_true", help="reduced-size instances (debugging only; not the BASELINE workloads)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extra", action="store_true", help="headline workload only")
    ap.add_argument("--no-variants", action="store_true", help="skip the opt-in variants of cfg5 measured next to the contract number (adaptive lifting depth)")
    ap.add_argument("--no-float32", action="store_true", help="skip the Float32 (libcosmo_hip_f32.so) side numbers of cfg4 / cfg5")
    ap.add_argument("--cpu-sample-iters", type=int, default=5)
    ap.add_argument("--kkt", choices=["cg", "cg-sr"], default="cg",
                    help="cg: the literal cg! recurrence (default, the reference's algorithm; config.kkt_solver names the kernels); cg-sr: opt-in single-reduction CG (csrc/cg_sr.hip)")
    ap.add_argument("--no-prewarm", action="store_true", help="skip the clock warm-up launches of the product kernel (profiling runs: kernel statistics of the loop's own launches only)")
    ap.add_argument("--exact-launches", action="store_true",
                    help="cfg2: synchronise after every Krylov iteration (rocprofv3 runs: every launch does full work)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: rooflines, cpu_baseline, the other workloads (extra), opt-in variants, Float32, cfg3's time to "
                         "solution and, at N > 1, the parity leg and the unsharded comparison (a plain run times the headline workload only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write x, y, s of the headline workload (as optimize() returns them) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full:
        args.no_extra = args.no_cpu_baseline = args.no_variants = args.no_float32 = True

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_under_torchrun(args.gpus)                         # does not return
    args.deferred = []          # cpu_baseline legs: run AFTER all GPU work, so that no timed window follows tens of seconds of GPU idling (clocks)
    ctx = Ctx()
    if ctx.world != max(args.gpus, 1) and ctx.rank == 0:
        print("bench.py: --gpus %d but the launcher started %d rank(s); reporting n_gpus = %d" % (args.gpus, ctx.world, ctx.world), file=sys.stderr)
    KKT_CHOICE["name"] = args.kkt
    NO_PREWARM[0] = bool(args.no_prewarm)
    import cosmo_jl_amd as cj  # noqa: F401
    workload = args.workload or "all"
    head = HEADLINE if workload == "all" else workload
    # N > 1: the headline itself now runs data-path collectives (the row-sharded loop).  If it never returns -- a rank that died while the others wait
    # inside RCCL on the first real multi-GPU execution -- a line must still come out and it must not look like a measurement: value 0, an `error`
    # field, exit code 1 (COSMO_BENCH_HEAD_TIMEOUT seconds, default 900).
    head_dog = None
    if ctx.world > 1:
        import threading as _th

        def head_expired():
            if ctx.rank == 0:
                print(json.dumps({"metric": METRIC, "value": 0.0, "unit": "ADMM iterations/s", "n_gpus": ctx.world, "steps": args.steps, "warmup": args.warmup,
                                  "ms_per_step": None, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
                                  "config": {"workload": "%s (headline did not finish)" % head},
                                  "error": "the %d-rank run of the headline workload did not finish within COSMO_BENCH_HEAD_TIMEOUT = %s s (a hang inside a "
                                           "collective?): NOT a measurement" % (ctx.world, os.environ.get("COSMO_BENCH_HEAD_TIMEOUT", "900"))}), flush=True)
            os._exit(1)
        head_dog = _th.Timer(float(os.environ.get("COSMO_BENCH_HEAD_TIMEOUT", "900")), head_expired)
        head_dog.daemon = True
        head_dog.start()
    res = BENCH[head](ctx, args, args.steps, args.warmup)
    args.dump_outputs = None                                       # the outputs are the headline's: the extras below must not overwrite them
    if head_dog is not None:
        head_dog.cancel()
    extra = {}

    def headline_line():
        out = {"metric": METRIC, "value": round(res["value"], 3), "unit": "ADMM iterations/s", "n_gpus": ctx.world, "steps": res["steps"], "warmup": res["warmup"],
               "ms_per_step": round(res["ms_per_step"], 6), "higher_is_better": True, "scaling": res["scaling"], "vs_baseline": None, "dtype": "f64",
               "data": "synthetic", "config": res.get("config", {}), "roofline": res.get("roofline")}
        # which Krylov recurrence ran comes from the handle (cosmo_hip_kkt_recurrence); workloads that do not report it ran kkt_kind CG
        out["config"].setdefault("kkt_solver", "CGIndirectKKTSolver (--kkt %s)" % args.kkt)
        out["config"]["kkt_solver_requested"] = {"cg": "CGIndirectKKTSolver (kkt_kind CG: the literal cg! recurrence, the reference's algorithm)",
                                                 "cg-sr": "kkt_kind CG_SR: single-reduction (Chronopoulos-Gear) recurrence -- OPT-IN variant, same operator / stopping rule"}[args.kkt]
        out["config"]["launch"] = ("self-launched torch.distributed.run" if os.environ.get("COSMO_BENCH_SELF_LAUNCHED") else
                                   "torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ else "single process")
        if ctx.shm:
            out["data"] = "synthetic; DRY RUN of the multi-rank path: all ranks share one GPU (COSMO_BENCH_TRANSPORT=shm), not a measurement"
        if "cpu_baseline" in res:
            out["cpu_baseline"] = res["cpu_baseline"]
        var = {k: res[k] for k in ("time_to_solution", "single_reduction_cg", "pcg", "adaptive_lifting_depth", "eigen_projection", "float32") if k in res}      # opt-in variants of the headline workload: next to, never instead of, `value`
        if var:
            out["variants"] = var
        if extra:
            out["extra"] = dict(extra)
        return out

    def summary_of(line):
        """Compact digest, LAST key of the line (the driver keeps the tail of stdout): every workload's rate + roofline fraction + CPU baselines."""
        def short(r):
            if not isinstance(r, dict) or "error" in r or "value" not in r:
                return {"error": (r or {}).get("error", "missing")} if isinstance(r, dict) else None
            o = {"value": r["value"], "scaling": r.get("scaling")}
            rf = r.get("roofline") or {}
            if rf:
                o["roofline_frac"] = rf.get("frac"); o["bound"] = rf.get("bound")
            cb = r.get("cpu_baseline") or {}
            if cb:
                o["cpu"] = round(cb["value"], 4) if isinstance(cb.get("value"), float) else cb.get("value")
                dk = cb.get("direct_kkt") or {}
                if "value" in dk:
                    o["cpu_direct_kkt"] = round(dk["value"], 4)
                elif "feasible" in dk:
                    o["cpu_direct_kkt"] = "infeasible (fill)" if not dk["feasible"] else "feasible"
            return o
        sm = {head: short(line)}
        for k, v in (line.get("extra") or {}).items():
            sm[k] = short(v)
        cfgp = line.get("config", {})
        tts = (line.get("variants") or {}).get("time_to_solution") or {}
        if "seconds" in tts:
            sm["cfg5_time_to_solution"] = {"seconds": tts["seconds"], "status": tts["status"], "iterations": tts["iterations"]}
        if ctx.world > 1:
            sm["parity_ok"] = cfgp.get("parity_ok"); sm["speedup_vs_single_gpu"] = cfgp.get("speedup_vs_single_gpu")
        return sm

    # N > 1: the sharded extras are the only part of this program with data-path collectives.  If one of them hangs (a rank that failed while
    # the others wait in a collective), the headline -- measured already -- must still be reported: a watchdog prints the line with what has
    # been collected and ends every rank.  COSMO_BENCH_EXTRA_TIMEOUT seconds for all extras together (default 600).
    watchdog = None
    others = [k for k in ("cfg2", "cfg3", "cfg4", "cfg5") if k != head]
    extra_plan = [(k, k) for k in others] if ctx.world == 1 else \
                 [(k, k + "_sharded") for k in others if k in ("cfg3", "cfg5")] + [(k, k + "_replicas") for k in others if k in ("cfg2", "cfg4")]
    extra_keys = [key for _, key in extra_plan]
    import threading
    line_lock, line_state = threading.Lock(), {"printed": False}

    def print_line_once(extras_override=None):
        """The ONE JSON line of the contract: whoever gets here first (the normal end of main, or rank 0's watchdog) prints it, nobody prints twice."""
        with line_lock:
            if line_state["printed"] or ctx.rank != 0:
                return None
            line_state["printed"] = True
            out = headline_line()
            if extras_override is not None:
                out["extra"] = extras_override
            out["summary"] = summary_of(out)
            print(json.dumps(out), flush=True)
            return out

    if ctx.world > 1 and workload == "all" and not args.no_extra:
        deadline = float(os.environ.get("COSMO_BENCH_EXTRA_TIMEOUT", "600"))

        def expire():
            # Rank 0 prints the headline with a COPY of what has been collected (under the lock that the normal end of main takes too: the line is
            # printed once) and leaves.  The other ranks print nothing and leave `grace` seconds EARLIER than rank 0: a rank that outlives rank 0 would
            # die with an exception inside its next collective and torchrun would report the job as failed; rank 0, if a peer leaves while it is inside a
            # collective, gets an exception that the per-extra try / except below records, and still prints.
            if ctx.rank == 0:
                snap = dict(extra)
                for name in extra_keys:
                    snap.setdefault(name, {"error": "not finished within COSMO_BENCH_EXTRA_TIMEOUT; the headline above was measured before"})
                print_line_once(snap)
            os._exit(0)
        watchdog = threading.Timer(deadline + (float(os.environ.get("COSMO_BENCH_EXTRA_GRACE", "2")) if ctx.rank == 0 else 0.0), expire)
        watchdog.daemon = True
        watchdog.start()
    if workload == "all" and not args.no_extra:
        # N = 1: the other three BASELINE configurations on the one GPU.  N > 1: the batch that shards (strong scaling) and -- explicitly as REPLICAS,
        # one replica's rate, never aggregated -- the two configurations that do not shard.
        for name, key in extra_plan:
            try:
                k, w = EXTRA_STEPS[name]
                r = BENCH[name](ctx, args, k, w)
                if key.endswith("_replicas"):
                    r["value"] = r["value"] / ctx.world; r["scaling"] = "replicas"; r["replicas"] = ctx.world
                    r["note"] = "%d independent replicas, value = ONE replica's rate on the max-over-ranks time (this configuration does not shard; never a headline)" % ctx.world
                r["value"] = round(r["value"], 3); r["ms_per_step"] = round(r["ms_per_step"], 6); r["unit"] = "ADMM iterations/s"
                r["n_gpus"] = ctx.world
                extra[key] = r
            except Exception as e:                                  # an extra workload must not take the headline line down
                extra[key] = {"error": "%s: %s" % (type(e).__name__, e)}
    if watchdog is not None:
        watchdog.cancel()
    for leg in args.deferred:     # the restated CPU reference on bounded samples of the same instances (rank 0 at N = 1 only)
        leg()
    out = print_line_once()
    if ctx.dist is not None:
        try:
            ctx.dist.barrier()
            ctx.dist.destroy_process_group()
        except Exception:           # a peer that left through its watchdog: the line is out already
            pass
    return out


if __name__ == "__main__":
    if "--cpu-leg" in sys.argv:
        cpu_leg_main()
    else:
        main()
