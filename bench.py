#!/usr/bin/env python3
"""bench.py -- headline benchmark: MPC solves/s of the batched SQP-RTI step on MI355X.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path (admpc_solve_batch: shooting + QP + full step for every
instance; at N = 20 fp64 one fused persistent kernel behind a work-order pre-pass, otherwise two launches) over one batch of synthetic scenarios that is already resident
in HBM.  Every step starts from the same initial iterate (pre-staged copies), so all steps do identical work.
Workloads (BASELINE.json):
  --gpus 1 (default)                                   configs[1]: batch 4096 random (x0, curved reference) scenarios, N = 20, fp64
  --gpus N > 1 (default 8192 per GPU)                  configs[3]: 65536 scenarios at 8 GPUs, every rank its own contiguous shard
                                                       (weak scaling, no data-path collective), RCCL arg-min at the end of the step
  --dtype f32 --horizon 80 --batch-per-gpu 16384       configs[4]: long horizon, fp32 storage and arithmetic
  --gp                                                 configs[2]: GP residual dynamics active

`python bench.py --gpus N` with N > 1 and no torch.distributed environment starts its N ranks ITSELF (a child
`python -m torch.distributed.run --nproc-per-node N ... bench.py <same arguments>`, spawned before any GPU call), relays rank 0's
JSON line and exits with the child's code.  It refuses (non-zero exit, no JSON) to run on fewer GPUs or ranks than `--gpus` asks for:
`n_gpus` in the line is never below the request, and `ranks_seen` is what the collective itself counted (an all-reduce of ones).
`--dry-collective gloo` rehearses exactly that launcher / rendezvous / sharding / arg-min record path on CPU ranks (no solve, no
GPU; `value` is null and `dry` is true): the CPU test of the N > 1 path.

A plain run sets up, warms up, times the K steps and prints its line.  Everything else it can measure is behind `--full`: the CPU
baseline, two batches in flight, the tight stop levels, HBM traffic from rocprofv3 child passes, and on N > 1 ranks the per-rank rate
without the collective (each of them can still be switched off one by one with its --no-* option).
`--dump-outputs DIR` writes what the last timed step returned to its caller (x, u, cost, status, iters; on N > 1 ranks rank 0's shard
and the arg-min) as DIR/<name>.npy, float32 or float64, at most 64 MB in all; the inputs depend on the arguments only.

Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from ad_mpc_amd.config import default_config, set_gp, NX, NU, NY  # noqa: E402
from ad_mpc_amd.engine import BatchSolver  # noqa: E402
from ad_mpc_amd.scenarios import random_scenarios, grid_gp  # noqa: E402
from ad_mpc_amd import dist as adist  # noqa: E402

FP64_PEAK_TFLOPS = 78.6          # MI355X fp64 vector = matrix peak (AMD datasheet)
FP32_PEAK_TFLOPS = 157.3         # /opt/skills/guides/MI355X_MICROARCH.md: peak FP32 (vector)
HBM_PEAK_GBS = 8000.0            # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec


def algorithmic_bytes_per_solve(N, elem=8):
    """in x0 + yref + yref_e + iterate + p ; out iterate + cost + status(4 B).  N = 20 fp64: 4564 B; N = 80 fp32: 8764 B."""
    n_in = NX + (N * NY + NX) + ((N + 1) * NX + N * NU) + 1
    n_out = (N + 1) * NX + N * NU + 1
    return elem * (n_in + n_out) + 4


def gp_flops_per_model_eval(cfg):
    """Residual GPs inside the model (configs[2]): per training point of a regressor with d features 3 d (scaled squared distance) + 1 (exp,
    counted as one operation like the sin / cos of SURVEY 8d's model count) + 2 (mean) + 3 d (gradient): 3 + 6 d; one-feature regressors with
    20 points each (grid_gp): 3 x 20 x 9 = 540 per evaluation of the model, i.e. N x 4 x 540 per solve on top of the shooting's N x 4360."""
    return float(sum(cfg.gp[g].n_points * (3 + 6 * cfg.gp[g].n_feat) for g in range(cfg.n_gp)))


def algorithmic_flops_per_solve(N, mean_ipm_iters, trial, gp_eval_flops=0.0):
    """shooting N*4360 + N*1900 per interior-point iteration (measured mean iterations).  With the unconstrained
    trial (cfg.ipm_try_unconstrained) every instance also pays one factorisation + one solve = 0.7 of an iteration's count.
    gp_eval_flops: the residual GPs' kernel sums per model evaluation (4 RK stages per shooting stage), so that configs[2]'s fraction
    counts the same arithmetic as configs[1]'s."""
    return N * (4360.0 + 4.0 * gp_eval_flops) + N * 1900.0 * (mean_ipm_iters + (0.7 if trial else 0.0))


def measured_traffic(N, B, dtype, variant=""):
    """HBM bytes of one step from the committed PMC passes (profiles/rN/*pmc_summary.json, written by scripts/profile.sh on
    the same workload: separate --pmc runs for FETCH_SIZE and WRITE_SIZE, FETCH_SIZE doubled as the microarchitecture guide
    prescribes for gfx950).  Counters cannot be read inside this process; None unless a profile of exactly this workload exists."""
    import glob
    import re
    best = None
    def order(f):            # newest round, then newest build
        m = re.search(r"r(\d+)[/\\]", f)
        return (int(m.group(1)) if m else 0, os.path.getmtime(f))
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*", "*pmc_summary.json")), key=order):
        try:
            js = json.load(open(f))
        except Exception:
            continue
        w = js.get("_workload", {"horizon": 20, "batch": 4096, "dtype": "f64"})      # round-1 summaries carry no tag: configs[1]
        t = js.get("_step_traffic")
        if t and (w.get("horizon"), w.get("batch"), w.get("dtype"), w.get("variant", "")) == (N, B, dtype, variant):
            best = {"bytes": t["bytes"], "source": os.path.relpath(f, ROOT)}
    return best


def traffic_child_args(argv, steps, warm):
    """Command line of a PMC child pass: the parent's workload arguments, its own step counts, no side measurements, no nested passes,
    no output dump."""
    keep = [a for a in argv if a not in ("--no-cpu-baseline", "--no-two-in-flight", "--no-tight-stop", "--no-live-traffic", "--full")]
    out = []
    i = 0
    while i < len(keep):                                   # drop --steps / --warmup / --dump-outputs (and their values) of the parent
        if keep[i] in ("--steps", "--warmup", "--dump-outputs"):
            i += 2; continue
        if keep[i].startswith(("--steps=", "--warmup=", "--dump-outputs=")):
            i += 1; continue
        out.append(keep[i]); i += 1
    return out + ["--steps", str(steps), "--warmup", str(warm), "--no-cpu-baseline", "--no-two-in-flight", "--no-tight-stop", "--no-live-traffic"]


def live_traffic(argv, timeout_s=45):
    """HBM bytes of one step measured NOW, for this run's own workload: two child runs of this script under `rocprofv3 --pmc`
    (FETCH_SIZE and WRITE_SIZE in passes of their own: the TCC counters share slots -- MI355X_MICROARCH.md, HBM section; FETCH_SIZE is
    in KiB and doubled on gfx950, WRITE_SIZE in KiB), 3 steps each, no side measurements, summed over the kernels of a step and
    divided by the number of steps.  Counters cannot be read inside the timed process.  None when rocprofv3 is missing or a pass fails
    (the committed summary of the same workload is reported instead, labelled by `traffic_source`)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    rp = shutil.which("rocprofv3")
    if rp is None:
        return None
    steps, warm = 3, 1
    child = [sys.executable, os.path.abspath(__file__)] + traffic_child_args(argv, steps, warm)
    tmp = tempfile.mkdtemp(prefix="admpc_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    total = {}
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, ctr)
            # the program itself directly behind `--` (no env / shell hop: the profiler's preloaded library has initialised the GPU)
            r = subprocess.run([rp, "--pmc", ctr, "--output-format", "csv", "-d", d, "--"] + child, cwd="/tmp", env=env,
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s)
            if r.returncode != 0:
                print("bench.py: live traffic: the %s pass exited with %d; reporting the committed summary of this workload instead" % (ctr, r.returncode), file=sys.stderr)
                return None
            per_kernel = {}                                # kernel -> dispatch -> value (a counter row per XCD / SE instance is summed)
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                with open(f) as fh:
                    for row in csv.DictReader(fh):
                        name = row["Kernel_Name"]
                        if "admpc_" not in name or row["Counter_Name"] != ctr:
                            continue
                        per_kernel.setdefault(name, {}).setdefault(row["Dispatch_Id"], 0.0)
                        per_kernel[name][row["Dispatch_Id"]] += float(row["Counter_Value"])
            if not per_kernel:
                return None
            # every launch of every admpc kernel of the run (warm-up included: all steps are alike) / number of steps
            total[ctr] = sum(sum(v.values()) for v in per_kernel.values()) / float(steps + warm)
        return {"bytes": total["FETCH_SIZE"] * 1024.0 * 2.0 + total["WRITE_SIZE"] * 1024.0,
                "source": "live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE child passes of this command (%d steps each)" % (steps + warm)}
    except Exception as e:                 # a timeout (two passes, at most 45 s each) or an unreadable counter file
        print("bench.py: live traffic: %r; reporting the committed summary of this workload instead" % (e,), file=sys.stderr)
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def cpu_baseline(cfg, scen, target_seconds=12.0):
    """Time the CPU oracle (OpenMP build of oracle/admpc_oracle.c) on the same workload, bounded sample."""
    from oracle.oracle import Oracle, build
    build(omp=True)
    o = Oracle(omp=True)
    nthreads = o.max_threads()
    B = scen["x0"].shape[0]
    # single-thread probe on 256 instances to size the sample
    nprobe = min(256, B)
    t = time.perf_counter()
    o.solve_batch(cfg, scen["x0"][:nprobe], scen["yref"][:nprobe], scen["yref_e"][:nprobe], scen["p"][:nprobe],
                  scen["xbar"][:nprobe], scen["ubar"][:nprobe], nthreads=1)
    t1 = (time.perf_counter() - t) / nprobe
    reps = max(1, int(round(target_seconds / (t1 * B))))       # ~target_seconds of total CPU work
    t = time.perf_counter()
    for _ in range(reps):
        o.solve_batch(cfg, scen["x0"], scen["yref"], scen["yref_e"], scen["p"], scen["xbar"], scen["ubar"], nthreads=nthreads)
    dt = time.perf_counter() - t
    return {"value": reps * B / dt, "unit": "solves/s", "cores": nthreads, "kind": "port",
            "sample": "%d x the same %d-instance batch (N=%d; the oracle is fp64 whatever the GPU dtype) on %d OpenMP threads; single-thread rate %.0f solves/s"
                      % (reps, B, cfg.N, nthreads, 1.0 / t1)}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, per_instance, extra=None):
    """--dump-outputs: one DIR/<name>.npy per array.  `per_instance` arrays share their leading batch axis; if all of them together exceed
    64 MB, the same fixed, seeded sample of instances is kept of each, and its indices are written as instance_index.npy.  Integer
    arrays (status, iteration counts) are written as float64, which holds them exactly."""
    os.makedirs(path, exist_ok=True)
    out = {k: np.asarray(a) for k, a in per_instance.items()}
    out = {k: (a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)) for k, a in out.items()}
    B = next(iter(out.values())).shape[0]
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_LIMIT_BYTES:
        m = int((DUMP_LIMIT_BYTES - (1 << 20)) // (total / B + 8))
        idx = np.sort(np.random.default_rng(20240601).choice(B, m, replace=False))
        out = {k: a[idx] for k, a in out.items()}
        out["instance_index"] = idx.astype(np.float64)
    for k, a in (extra or {}).items():
        out[k] = np.asarray(a, dtype=np.float64)
    for k, a in out.items():
        np.save(os.path.join(path, k + ".npy"), np.ascontiguousarray(a))


def spawn_ranks(n):
    """Start the N ranks of this very command as a child `python -m torch.distributed.run` (never an exec: nothing in this process
    has touched a GPU yet, and nothing will), relay the one JSON line of rank 0, return the child's exit code."""
    import socket
    import subprocess
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    print("bench.py: --gpus %d without a torch.distributed environment: starting the ranks: %s" % (n, " ".join(cmd)), file=sys.stderr)
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, env=env)
    line = None
    for ln in proc.stdout.decode(errors="replace").splitlines():
        try:
            if isinstance(json.loads(ln), dict): line = ln
        except ValueError:
            print(ln, file=sys.stderr)
    if proc.returncode == 0 and line is None:
        print("bench.py: the ranks exited with 0 but printed no JSON line", file=sys.stderr)
        return 1
    if line is not None and proc.returncode == 0:
        print(line, flush=True)
    return proc.returncode


def dry_collective(args, world, rank, launched):
    """--dry-collective gloo: the N > 1 plumbing of this file on CPU ranks -- rendezvous, the refusal rules, contiguous shard
    offsets, the 16-byte record path of the arg-min (reduced by libadmpc's host twin of the device reducer), barrier + max-over-ranks
    timing, the JSON line.  Nothing is solved: the 'costs' are a fixed function of the global scenario index."""
    B, K, Wm = args.batch_per_gpu or 8192, args.steps, args.warmup
    if launched:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
        if dist.get_world_size() != args.gpus:
            print("bench.py: the process group has %d ranks, --gpus asks for %d" % (dist.get_world_size(), args.gpus), file=sys.stderr)
            sys.exit(3)
    ones = torch.ones(1, dtype=torch.int64)
    if launched: dist.all_reduce(ones)
    lo, hi = adist.shard_range(world * B, rank, world)
    g = torch.arange(lo, hi, dtype=torch.float64)
    cost = torch.remainder((g + 1.0) * 0.6180339887498949, 1.0) + 1.0            # golden-ratio sequence: a distinct pseudo-random cost per global index
    best = None
    for phase, n in ((0, Wm), (1, K)):
        if phase == 1:
            if launched: dist.barrier()
            t0 = time.perf_counter()
        for _ in range(n):
            v, i = adist.local_argmin_torch(cost, index_offset=lo)
            best = adist.global_argmin_records(adist.pack_pair(v, i), adist.pairs_min_host) if launched else adist.pack_pair(v, i)
    if launched: dist.barrier()
    elapsed = time.perf_counter() - t0
    if launched:
        tt = torch.tensor([elapsed], dtype=torch.float64); dist.all_reduce(tt, op=dist.ReduceOp.MAX); elapsed = float(tt.item())
    rates = None
    if args.full:
        # the collective-free segment of the real run (per-rank rate by the rank's own clock, gathered): here the local arg-min loop stands in
        tl = time.perf_counter()
        for _ in range(K):
            adist.local_argmin_torch(cost, index_offset=lo)
        rl = torch.tensor([B * K / max(time.perf_counter() - tl, 1e-9)], dtype=torch.float64)
        rates = [float(rl.item())]
        if launched:
            allr = [torch.empty_like(rl) for _ in range(world)]; dist.all_gather(allr, rl); rates = [float(t.item()) for t in allr]
    if rank == 0:
        traffic = measured_traffic(args.horizon, B, args.dtype, "")
        allc = torch.remainder((torch.arange(world * B, dtype=torch.float64) + 1.0) * 0.6180339887498949, 1.0) + 1.0
        bc, bidx = adist.unpack_pair(best)
        out = {"metric": "MPC solves/sec (N=%d, nx=7, nu=2, fp64)" % args.horizon, "value": None, "unit": "solves/s", "dry": True,
               "n_gpus": world, "ranks_seen": int(ones.item()), "steps": K, "warmup": Wm, "ms_per_step": elapsed / K * 1e3,
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
               "config": {"workload": "DRY RUN of the N > 1 plumbing on CPU ranks (gloo): no solve", "batch_per_gpu": B,
                          "collective": "gloo all-gather arg-min (16 B/rank), reducer admpc_argmin_pairs_host"},
               "roofline": {"traffic": (traffic or {}).get("bytes"), "traffic_source": (traffic or {}).get("source")},
               "argmin": {"cost": bc, "index": bidx},
               "argmin_single_process": {"cost": float(allc.min()), "index": int(torch.argmin(allc))}}
        if rates is not None:
            out["config"]["one_gpu_solves_per_s_at_this_batch"] = rates[0]
            out["per_rank_solves_per_s_no_collective"] = {"min": min(rates), "max": max(rates), "rank0": rates[0], "batch_per_gpu": B, "dry": True}
        if args.full and not args.no_cpu_baseline:
            try:
                cfg = default_config(N=args.horizon, Ts=0.05)
                out["cpu_baseline"] = cpu_baseline(cfg, random_scenarios(64, N=args.horizon, Ts=0.05, seed=1234), target_seconds=0.5)
            except Exception as e:
                out["cpu_baseline"] = {"value": None, "unit": "solves/s", "cores": 0, "kind": "port", "sample": "failed: %r" % (e,)}
        print(json.dumps(out), flush=True)
    if launched:
        dist.barrier(); dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch-per-gpu", type=int, default=None, help="default: 4096 on one GPU (configs[1]), 8192 per GPU on several (configs[3])")
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--dtype", choices=("f64", "f32"), default="f64", help="f32: storage and arithmetic (configs[4] with --horizon 80 --batch-per-gpu 16384)")
    ap.add_argument("--gp", action="store_true", help="config 3: GP residual dynamics active")
    ap.add_argument("--dynamic", action="store_true", help="blend speeds 3/5 m/s so that the dynamic bicycle branch is active")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-two-in-flight", action="store_true",
                    help="skip the side measurement `two_in_flight` (an extra field, never `value`): the same K steps with two solver handles on two "
                         "streams, so that the tail of one step's interior-point kernel overlaps the next step (single-process runs only)")
    ap.add_argument("--no-tight-stop", action="store_true", help="skip the side measurement `tight_stop` (the same steps at the tight stop levels of rounds 1-2)")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="do not measure roofline.traffic with rocprofv3 child passes of this command (single-process runs; about a minute); "
                         "the committed PMC summary of the same workload is reported instead")
    ap.add_argument("--dry-collective", choices=("gloo",), default=None,
                    help="rehearse the N > 1 launcher / rendezvous / sharding / arg-min record path on CPU ranks (no solve, no GPU)")
    ap.add_argument("--full", action="store_true",
                    help="also run the side measurements (CPU baseline, two_in_flight, tight_stop, live roofline.traffic, per-rank rates "
                         "without the collective); a plain run only times the K steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32 / float64, at most 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    launched = "RANK" in os.environ and "MASTER_PORT" in os.environ     # torch.distributed.run: one rank per GPU, also for N = 1
    if args.gpus < 1:
        print("bench.py: --gpus must be >= 1", file=sys.stderr); sys.exit(2)
    # ---- N ranks or nothing.  The un-launched parent must see N GPUs; a launched rank only its own (a launcher may give every rank one
    # visible device).  What matters for the ranks this file starts itself is that they are a child PROCESS, never an exec of this one.
    ndev = torch.cuda.device_count()
    if not args.dry_collective and ((not launched and ndev < args.gpus) or (launched and ndev <= (local_rank if ndev > 1 else 0))):
        print("bench.py: --gpus %d but only %d GPU(s) visible%s: refusing to report a smaller job" % (args.gpus, ndev, " to rank %d" % rank if launched else ""), file=sys.stderr)
        sys.exit(3)
    if not launched and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus))
    if launched and world != args.gpus:
        if rank == 0:
            print("bench.py: launched with WORLD_SIZE %d but --gpus %d: refusing (n_gpus would not be what was asked)" % (world, args.gpus), file=sys.stderr)
        sys.exit(3)
    if args.dry_collective:
        return dry_collective(args, world, rank, launched)
    # stdout carries exactly one JSON line: whatever native libraries print there (the RCCL banner at communicator
    # creation) is sent to stderr for the duration of the run
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    if launched:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dv = local_rank if torch.cuda.device_count() > 1 else 0
        torch.cuda.set_device(dv)
        dist.init_process_group("nccl", device_id=torch.device("cuda", dv))
        if dist.get_world_size() != args.gpus:
            print("bench.py: the process group has %d ranks, --gpus asks for %d" % (dist.get_world_size(), args.gpus), file=sys.stderr)
            sys.exit(3)
    dev_index = (local_rank if torch.cuda.device_count() > 1 else 0) if launched else 0      # one visible device per rank: index 0
    torch.cuda.set_device(dev_index)

    if args.batch_per_gpu is None:
        args.batch_per_gpu = 4096 if world == 1 else 8192
    N, B, K, Wm = args.horizon, args.batch_per_gpu, args.steps, args.warmup
    f32 = args.dtype == "f32"
    tdt = torch.float32 if f32 else torch.float64
    elem = 4 if f32 else 8
    cfg = default_config(N=N, Ts=0.05)
    if args.gp:
        set_gp(cfg, grid_gp())
    blend = (3.0, 5.0) if args.dynamic else (100.0, 110.0)
    scen = random_scenarios(B, N=N, Ts=0.05, seed=1234, start=rank * B, blend=blend)
    eng = BatchSolver(cfg, device=dev_index)
    d = lambda a: eng.to_device(a, tdt)
    x0, yref, yref_e, p = d(scen["x0"]), d(scen["yref"]), d(scen["yref_e"]), d(scen["p"])
    xinit, uinit = d(scen["xbar"]), d(scen["ubar"])
    # one pre-staged iterate per step: every step starts from the same initial iterate
    xb = [xinit.clone() for _ in range(K + Wm)]
    ub = [uinit.clone() for _ in range(K + Wm)]
    cost = torch.empty(B, dtype=tdt, device=eng.device)
    status = torch.empty(B, dtype=torch.int32, device=eng.device)
    iters = torch.empty(B, dtype=torch.int32, device=eng.device)
    # HIP events around the timed region (on the launch stream): step time by the device's clock = elapsed / K.  (Two events PER STEP, as in
    # rounds 1-2, put two marker packets between consecutive solves: 8 us of a 0.23 ms step.)
    ev_begin, ev_end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    # config 4: per-GPU arg-min, 16 B/rank all-gather over RCCL, second-level arg-min -- three device operations, no host sync.  They run
    # on a side stream behind an event of the solve, so that the all-gather's latency (~ 70 us, a quarter of an N = 20 step) overlaps the
    # next step's solve; the cost array and the gather buffer alternate between two copies (a solve must not overwrite the costs the
    # side stream is still reducing).  Every arg-min of the K timed steps completes inside the timed region (device-wide synchronise).
    # The persistent solve kernel holds every register of the chip until it drains, so the three small operations of step i only get
    # to run in the drain of step i + 1 (or behind it): with two copies the solve of step i + 2 waited for them (+ 17 us per step on
    # one rank); four copies keep the main stream from ever waiting on the side stream.
    NRING = 4
    gathered = [torch.empty((world, 2), dtype=torch.float64, device=eng.device) for _ in range(NRING)]
    costs = [cost] + [torch.empty_like(cost) for _ in range(NRING - 1)]
    red_prio = int(os.environ.get("ADMPC_BENCH_RED_PRIO", "-1"))
    red = torch.cuda.Stream(device=eng.device, priority=red_prio) if launched else None      # high priority: its three tiny operations run as soon as a CU has room
    solved = [torch.cuda.Event() for _ in range(NRING)]
    reduced = [None] * NRING

    def step(i, timed_idx=None):
        q = i % NRING
        c = costs[q] if launched else cost
        if launched and reduced[q] is not None:
            # the reduction NRING steps back has read this copy.  Waited for on the HOST (it has long happened; the host runs several steps
            # ahead): a cross-stream wait packet in front of every solve cost the main stream several microseconds per step
            if os.environ.get("ADMPC_BENCH_DEVICE_WAIT") == "1": torch.cuda.current_stream().wait_event(reduced[q])
            else: reduced[q].synchronize()
        eng.solve(x0, yref, yref_e, p, xb[i], ub[i], c, status, iters)
        if launched:
            solved[q].record()                                         # the side stream's trigger (the only marker packet of a step)
            # The reduction of step i is handed to the side stream one step LATER, behind the enqueue of solve i + 1: issued at once its
            # three operations become runnable exactly at the boundary between two solves and hold up the next solve's start (+ 17 us per
            # step measured on one rank); one step behind they are runnable while solve i + 1 runs and go into its drain.
            best = reduce_pending()
            pending.append((q, c))
            return best
        return None

    pending = []

    def reduce_pending():
        if not pending:
            return None
        q, c = pending.pop(0)
        with torch.cuda.stream(red):
            red.wait_event(solved[q])
            best = adist.global_argmin_device(eng, c.double() if f32 else c, index_offset=rank * B, gathered=gathered[q])
            ev = torch.cuda.Event(); ev.record(red); reduced[q] = ev
        return best

    # ---- launched runs: the same K steps WITHOUT any collective first (no arg-min, no side stream), every rank by its own clock: the
    # denominator of a scaling efficiency that is measured in the same run, on the same per-GPU batch (the default batches of `--gpus 1`
    # and `--gpus N` differ: 4096 / 8192 per GPU, and the per-GPU rate depends on the batch -- VERDICT round 3, weak 6)
    local_rate = None
    if launched and args.full:
        for i in range(Wm):
            eng.solve(x0, yref, yref_e, p, xb[i].clone(), ub[i].clone(), cost, status, iters)
        xs = [xinit.clone() for _ in range(K)]; us = [uinit.clone() for _ in range(K)]
        torch.cuda.synchronize(); tl = time.perf_counter()
        for i in range(K):
            eng.solve(x0, yref, yref_e, p, xs[i], us[i], cost, status, iters)
        torch.cuda.synchronize()
        local_rate = B * K / (time.perf_counter() - tl)
        del xs, us
    ranks_seen = 1
    if launched:                                  # what the collective itself counts: every rank adds one
        ones = torch.ones(1, dtype=torch.int64, device=eng.device)
        dist.all_reduce(ones)
        ranks_seen = int(ones.item())
        if ranks_seen != args.gpus:
            print("bench.py: the all-reduce counted %d ranks, --gpus asks for %d" % (ranks_seen, args.gpus), file=sys.stderr)
            sys.exit(3)
    for i in range(Wm):
        step(i)
    if launched: reduce_pending()
    torch.cuda.synchronize()
    if launched: dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    best = None
    ev_begin.record()
    for i in range(K):
        best = step(Wm + i, i)
    ev_end.record()
    if launched: best = reduce_pending()      # the arg-min of the last step: every one of the K reductions completes inside the timed region
    t_enq = time.perf_counter() - t0          # host time to enqueue the K steps (launch-bound if close to `elapsed`)
    torch.cuda.synchronize()
    if launched: dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if launched:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=eng.device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if args.dump_outputs and rank == 0:
        last = Wm + K - 1
        dump_outputs(args.dump_outputs,
                     {"x": xb[last].cpu().numpy(), "u": ub[last].cpu().numpy(), "cost": (costs[last % NRING] if launched else cost).cpu().numpy(),
                      "status": status.cpu().numpy(), "iters": iters.cpu().numpy()},
                     {"argmin": adist.unpack_pair(best)} if best is not None else None)

    rates = None
    if local_rate is not None:
        rl = torch.tensor([local_rate], dtype=torch.float64, device=eng.device)
        allr = [torch.empty_like(rl) for _ in range(world)]
        dist.all_gather(allr, rl)
        rates = [float(t.item()) for t in allr]
    kern_ms = float(ev_begin.elapsed_time(ev_end)) / K      # the step's kernels and the gaps between them, by the device's clock
    it_host = iters.cpu().numpy(); st_host = status.cpu().numpy()
    two = None
    try:
      if args.full and not args.no_two_in_flight and not launched:
          # two handles (each owns its workspace: one solve in flight per handle), two streams, steps alternate between them
          eng2 = BatchSolver(cfg, device=dev_index)
          engs = (eng, eng2); sts = (torch.cuda.Stream(), torch.cuda.Stream())
          outs = [(torch.empty_like(cost), torch.empty_like(status), torch.empty_like(iters)) for _ in range(2)]
          xb2 = [xinit.clone() for _ in range(K + Wm)]; ub2 = [uinit.clone() for _ in range(K + Wm)]
          torch.cuda.synchronize()
          for phase in (0, 1):
              if phase == 1:
                  torch.cuda.synchronize(); t1 = time.perf_counter()
              for i in (range(Wm) if phase == 0 else range(Wm, Wm + K)):
                  with torch.cuda.stream(sts[i & 1]):
                      engs[i & 1].solve(x0, yref, yref_e, p, xb2[i], ub2[i], *outs[i & 1])
          torch.cuda.synchronize()
          dt2 = time.perf_counter() - t1
          two = {"ms_per_step": dt2 / K * 1e3, "solves_per_s": B * K / dt2,
                 "note": "two batches in flight (two handles, two streams): the drain of one step's persistent kernel (its last, slowest instances) is filled by the next step; not `value`"}
          two["bit_identical_to_the_timed_run"] = bool(torch.equal(xb2[Wm + K - 1], xb[Wm + K - 1]) and torch.equal(ub2[Wm + K - 1], ub[Wm + K - 1]))
          del eng2
    except Exception as e:                      # a side measurement: never a reason to lose the bench line
        two = {"error": repr(e)}
    # the same K steps at the tight stop levels of rounds 1-2 (every instance to within 1e-8 of the exact minimiser): a side measurement
    tight = None
    try:
        if args.full and not args.no_tight_stop and not launched:
            from ad_mpc_amd.config import tight_ipm
            engt = BatchSolver(tight_ipm(cfg.copy()), device=dev_index)
            itt = torch.empty_like(iters); stt = torch.empty_like(status)
            xbt = [xinit.clone() for _ in range(K + Wm)]; ubt = [uinit.clone() for _ in range(K + Wm)]
            for i in range(Wm):
                engt.solve(x0, yref, yref_e, p, xbt[i], ubt[i], cost, stt, itt)
            torch.cuda.synchronize(); tt0 = time.perf_counter()
            for i in range(Wm, Wm + K):
                engt.solve(x0, yref, yref_e, p, xbt[i], ubt[i], cost, stt, itt)
            torch.cuda.synchronize(); dtt = time.perf_counter() - tt0
            ith = itt.cpu().numpy()
            tight = {"ms_per_step": dtt / K * 1e3, "solves_per_s": B * K / dtt, "mean_ipm_iters": float(ith.mean()), "max_ipm_iters": int(ith.max()),
                     "status_nonzero": int((stt.cpu().numpy() != 0).sum()),
                     "max_abs_input_difference_to_the_timed_run": float((ubt[Wm + K - 1] - ub[Wm + K - 1]).abs().max()),
                     "levels": "complementarity 1e-10, residuals 1e-9, last input step 1e-6"}
            del engt
    except Exception as e:
        tight = {"error": repr(e)}
    mean_iters = float(it_host.mean())
    if rank == 0:
        total = world * B * K
        value = total / elapsed
        trial = cfg.ipm_try_unconstrained != 0.0
        flops = algorithmic_flops_per_solve(N, mean_iters, trial, gp_flops_per_model_eval(cfg)) * B
        byts = algorithmic_bytes_per_solve(N, elem) * B
        traffic = None
        profiled = any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ)      # already under a profiler (scripts/profile*.sh): no nested passes
        if args.full and not launched and not args.no_live_traffic and not profiled:
            traffic = live_traffic(sys.argv[1:])
        if traffic is None and not args.dynamic:
            traffic = measured_traffic(N, B, args.dtype, "gp" if args.gp else "")
        ach_tf = flops / (kern_ms * 1e-3) / 1e12
        ach_gbs = byts / (kern_ms * 1e-3) / 1e9
        peak_tf = FP32_PEAK_TFLOPS if f32 else FP64_PEAK_TFLOPS
        if f32 and N == 80 and B == 16384:
            wl = "BASELINE configs[4]: long horizon N=80, fp32 storage and arithmetic, batch 16384"
        elif world > 1 or B == 8192:
            wl = "BASELINE configs[3]: %d scenarios sharded over %d GPU(s), %d per GPU (shard of the 65536-scenario batch), N=%d, %s, RCCL arg-min" % (world * B, world, B, N, args.dtype)
        elif args.gp:
            wl = "BASELINE configs[2]: batch %d, N=%d, %s, GP residual-dynamics correction active" % (B, N, args.dtype)
        else:
            wl = "BASELINE configs[1]: batch %d random (x0, curved ref) scenarios, N=%d, %s" % (B, N, args.dtype)
        dense = N == 20 and not f32 and os.environ.get("ADMPC_QP") != "riccati"
        fused = dense and os.environ.get("ADMPC_N20") != "split"
        seg = not f32 and N in (40, 60, 80) and ((not args.gp and os.environ.get("ADMPC_QP") != "riccati") or os.environ.get("ADMPC_QP") == "seg")      # admpc_seg.hip: N / 20 cooperating waves per instance
        out = {
            "metric": "MPC solves/sec (N=%d, nx=7, nu=2, %s)" % (N, "fp32" if f32 else "fp64"), "value": value, "unit": "solves/s",
            "n_gpus": world, "ranks_seen": ranks_seen, "steps": K, "warmup": Wm, "ms_per_step": elapsed / K * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": wl + ", one SQP-RTI step" + (", dynamic branch (blend 3/5)" if args.dynamic else ""),
                       "batch_per_gpu": B, "horizon": N, "seed": 1234,
                       "qp_stop": "the reference's: HPIPM mode BALANCE, every residual norm and the complementarity products <= 1e-8, no step test "
                                  "(acados_solver_sim_car.c:688; qp_solver_tol_* unset)" + ("; fp32: floored at 1e-2 / 1e-3 and a step test at 1e-3" if f32 else ""),
                       "collective": "RCCL all-gather arg-min (16 B/rank)" if launched else "none"},
            "roofline": {"bound": "fp32-valu" if f32 else "fp64-valu", "achieved": ach_tf, "peak": peak_tf, "unit": "TFLOP/s",
                         "frac": ach_tf / peak_tf, "traffic": (traffic or {}).get("bytes"),
                         "traffic_source": (traffic or {}).get("source"),
                         "kernel": ("one step = admpc_f20_order_kernel (work-order pre-pass, ~5 us) + admpc_fused20_kernel (dominant, > 97 %: shooting, condensing, dense interior point and expansion of an instance in one persistent wave)"
                                    if fused else "one step = admpc_f20_order_kernel (work-order pre-pass, ~5 us) + admpc_seg_kernel<%d> (dominant, > 98 %%: %d cooperating waves per instance, each shooting, condensing, factorising and expanding 20 stages; the cuts coupled through 7 x 7 blocks)" % (N // 20, N // 20)
                                    if seg else "one step = admpc_linearize_kernel + admpc_condense_kernel<20,7> + admpc_qp_dense_kernel<20> (dominant, ~58 %) + admpc_expand_kernel<20>"
                                    if dense else "one step = admpc_linearize_kernel + admpc_rowqp_kernel (dominant, > 95 %: row-mapped Riccati interior point; batches of more than one round of waves run it twice -- trial for all, interior point on the remainder sorted by violated bounds)"),
                         "kernel_ms": kern_ms,
                         "kernel_ms_is": "HIP-event time over the K timed steps on the launch stream / K: the kernels of a step and the gaps between them (the dominant kernel's own average duration: the rocprofv3 kernel trace under profiles/)",
                         **({"peak_unpacked": FP64_PEAK_TFLOPS, "frac_unpacked": ach_tf / FP64_PEAK_TFLOPS,
                             "peak_note": "157.3 TFLOP/s is the packed (v_pk_fma_f32) vector rate; kernel R issues unpacked v_fmac_f32 (DPP operands), whose rate is 78.6"} if f32 else {}),
                         "note": ("%s; roof = %s vector peak %.1f TFLOP/s; algorithmic FLOPs = N*4360 (+ N*4*540 for the GP kernel sums with --gp) + N*1900*(mean_ipm_iters + 0.7 for the unconstrained trial) per solve (SURVEY 8d)"
                                  % ("vector FMAs, the condensed Hessian alone on v_mfma_f64_16x16x4_f64 tiles (2 %% of the arithmetic; the fp64 matrix peak equals the vector peak: profiles/r3/mfma_condense_ab.txt)"
                                     if fused else "vector FMAs; the condensed Hessians and the Schur blocks of the cuts on v_mfma_f64_16x16x4_f64 tiles (the fp64 matrix peak equals the vector peak)"
                                     if seg else "the kernels issue vector FMAs only (no MFMA executes: profiles/r2/mfma_vs_valu_f64.txt)", "fp32" if f32 else "fp64", peak_tf))},
            "roofline_hbm": {"bound": "hbm", "achieved": ach_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach_gbs / HBM_PEAK_GBS,
                             "bytes_per_solve": algorithmic_bytes_per_solve(N, elem)},
            "host_enqueue_ms_per_step": t_enq / K * 1e3, "mean_ipm_iters": mean_iters, "max_ipm_iters": int(it_host.max()), "status_nonzero": int((st_host != 0).sum()),
            "unconstrained_trial": {"enabled": bool(trial), "fraction_solved_without_interior_point": float((it_host == 0).mean())},
        }
        if rates is not None:
            out["per_rank_solves_per_s_no_collective"] = {"min": min(rates), "max": max(rates), "rank0": rates[0], "batch_per_gpu": B,
                "note": "the same K steps on every rank before the timed region, no arg-min, no barrier inside, each rank by its own clock: "
                        "N x min is what the job would do if the collective and the closing barrier were free"}
            out["config"]["one_gpu_solves_per_s_at_this_batch"] = rates[0]
        if two is not None:
            out["two_in_flight"] = two
        if tight is not None:
            out["tight_stop"] = tight
        if best is not None:
            bc, bidx = adist.unpack_pair(best)
            out["argmin"] = {"cost": bc, "index": bidx}
        if args.full and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(cfg, scen)
            except Exception as e:  # the baseline is a reported number, never a reason to lose the GPU line
                out["cpu_baseline"] = {"value": None, "unit": "solves/s", "cores": 0, "kind": "port", "sample": "failed: %r" % (e,)}
        sys.stdout.flush()
        os.dup2(real_stdout, 1)
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)
    if launched:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
