"""Vehicles per second of the fleet control step (ad_mpc_amd/fleet.py, admpc_control_step_batch) against the bare solve of the same
batch (admpc_solve_batch on the same references) and against the per-vehicle loop through ROSGPMPC (get_waypoints, resample_vel,
set_reference, optimize: what a host does for each vehicle without the fleet step).

    python scripts/fleet_step.py [--batches 1,64,4096] [--horizons 20,40] [--steps 50] [--warmup 10] [--loop-calls 200]
    python scripts/fleet_step.py --bank [--batches 4096] [--horizons 20,40] [--steps 50] [--warmup 10] [--repeats 5]
    python scripts/fleet_step.py --lane [--batches 4096] [--horizons 20,40] [--steps 50] [--warmup 10] [--repeats 5]
    python scripts/fleet_step.py --rollout 50 [--batches 4096] [--horizons 20,40] [--repeats 5]
    python scripts/fleet_step.py --rollout 50 --observe [--batches 4096] [--horizons 20,40] [--repeats 5]

--bank: the same workloads through a bank of paths (admpc_control_step_bank_batch: set_paths / step_paths) with K = 1 and with K = 8 copies
of the path and round-robin path_of, against the single-path step in the same process, the variants interleaved `repeats` times (one JSON
line per (N, B) with every repeat and the medians); and admpc_argmin_groups at (G, group) = (4096, 4) and (64, 1024) against admpc_argmin
over the same number of entries.

--lane: the step along a route (admpc_control_step_lane_batch: step_route with L = 64) for B vehicles spread along one route of 2000
waypoints, against the single-path step and the bank step (K = 1) for B vehicles at the start of the same route, interleaved as above.

--rollout T: one rollout_route of T closed-loop steps (admpc_rollout_lane_batch: the lane step and the plant kernel, T times, one call)
against T back-to-back step_route calls, for the same B vehicles spread along the route of --lane, seconds per step, interleaved as above;
every repeat starts from the same poses.  The plant kernel's own time is read from a kernel trace of this command in a run of its own
(rocprofv3 --kernel-trace --stats -- python scripts/fleet_step.py --rollout T --repeats 1: the row of admpc_plant_kernel).

--rollout T --observe: the rollout of a controller that does not learn, of one that learns three regressors (placeholder GPs in its
model: the GP kernel paths) without observing, and of the same with every step observed (admpc_rollout_observe_lane_batch: the latch, and
admpc_observe_kernel and admpc_bin_kernel behind every step), seconds per step, interleaved as above; and seconds per fit_gp with its
install on filled bins (8, 32 and 32 points factorised), on a controller of its own.  The kernels' own times are read from a kernel trace of this command in a run of its own (--repeats 1).

One JSON line per (N, B) and one for the per-vehicle loop per N.  Times come from HIP events around `steps` back-to-back steps (fleet,
bare solve) or wall time around `loop-calls` calls (the per-vehicle loop, which synchronises at every call by construction)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ad_mpc_amd import host  # noqa: E402
from ad_mpc_amd.create_ros_ad_mpc import ROSGPMPC  # noqa: E402
from ad_mpc_amd.fleet import FleetController  # noqa: E402

T_HORIZON, OPT_DT = 1.0, 0.01


def path(M=400, ds=0.5):
    s = np.arange(M) * ds
    return s * np.cos(0.3), s * np.sin(0.3) + 2.0 * np.sin(s / 30.0), np.arctan2(np.sin(0.3) + 2.0 / 30.0 * np.cos(s / 30.0), np.cos(0.3) + 0 * s), \
        7.0 + 1.5 * np.sin(s / 20.0)


def poses(B, p, seed=0):
    """Vehicles at the first waypoints of the path (the reference generator lays its window from the path's first waypoint on,
    ref_traj.py:124-131), up to 1 m off it, speeds 5 .. 9 m/s."""
    rng = np.random.default_rng(seed)
    x, y, psi, _ = p
    idx = rng.integers(0, 5, size=B)
    e = rng.uniform(-1.0, 1.0, size=B)
    px, py = x[idx] - e * np.sin(psi[idx]), y[idx] + e * np.cos(psi[idx])
    yaw = psi[idx] + rng.uniform(-0.1, 0.1, size=B)
    return [px, py, yaw, rng.uniform(5.0, 9.0, size=B), rng.uniform(-0.2, 0.2, size=B), rng.uniform(-0.1, 0.1, size=B),
            rng.uniform(-0.05, 0.05, size=B)]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / steps


def fleet_and_bare(N, B, p, steps, warmup):
    fc = FleetController(T_HORIZON, N, OPT_DT, B)
    fc.set_traj(*p)
    ins = [torch.as_tensor(a, dtype=torch.float64, device=fc.device) for a in poses(B, p)]
    t_step = timed(lambda: fc.step(*ins), steps, warmup)
    # the bare solve of the same batch: the references the step assembles, built here with the same host rules
    ref, _, _ = fc._ref.get_waypoints_batch(ins[0], ins[1], ins[2])
    fc._eng.resample_vel(ref[:, 3, :], ins[3], ins[4], fc.ad.acc_max, T_HORIZON / N)
    r = ref.cpu().numpy()
    yaw = ins[2].cpu().numpy()
    yr = np.zeros((B, N, 9)); yr[:, :, 0], yr[:, :, 1], yr[:, :, 3] = r[:, 0], r[:, 1], r[:, 3]
    yr[:, :, 2] = host.yaw_fix(yaw[:, None], r[:, 2])
    ye = yr[:, N - 1, :7].copy()
    x0 = np.stack([a.cpu().numpy() for a in ins], axis=1)
    pp = host.vel_switch(x0[:, 3], fc.ad.blend_min, fc.ad.blend_max)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=fc.device)
    tx0, tyr, tye, tp = d(x0), d(yr), d(ye), d(pp)
    xb, ub = torch.zeros_like(fc.x_opt), torch.zeros_like(fc.w_opt)
    st = torch.empty(B, dtype=torch.int32, device=fc.device)
    t_solve = timed(lambda: fc._eng.solve(tx0, tyr, tye, tp, xb, ub, None, st, None), steps, warmup)
    modes = fc.mode.cpu().numpy()
    fc.close()
    return t_step, t_solve, float(modes.mean())


def bank_against_single(N, B, p, steps, warmup, repeats):
    """Seconds per step of the single-path step, the bank step with K = 1 and with K = 8 (round-robin path_of), interleaved."""
    ins = None
    runs = {}
    for name, K in (("single", 0), ("bank_k1", 1), ("bank_k8", 8)):
        fc = FleetController(T_HORIZON, N, OPT_DT, B)
        if ins is None:
            ins = [torch.as_tensor(a, dtype=torch.float64, device=fc.device) for a in poses(B, p)]
        if K == 0:
            fc.set_traj(*p)
            runs[name] = (fc, lambda fc=fc: fc.step(*ins))
        else:
            fc.set_paths([p] * K)
            path_of = (torch.arange(B, device=fc.device) % K).to(torch.int32)
            runs[name] = (fc, lambda fc=fc, path_of=path_of: fc.step_paths(path_of, *ins))
    times = {name: [] for name in runs}
    for _ in range(repeats):
        for name, (fc, fn) in runs.items():
            times[name].append(timed(fn, steps, warmup))
    for fc, _ in runs.values():
        fc.close()
    return times


def lane_against_bank(N, B, steps, warmup, repeats, M=2000, lane=64):
    """Seconds per step of the single-path step, the bank step (K = 1) and the lane step on one route of M waypoints.  The first two can
    only serve vehicles at the route's start and get those; the lane step gets vehicles spread over the route, 0.3 m off it."""
    p = path(M)
    x, y, psi, _ = p
    rng = np.random.default_rng(1)
    at = rng.integers(0, M - 50, size=B)
    e = 0.3 * (-1.0) ** np.arange(B)
    spread = [x[at] - e * np.sin(psi[at]), y[at] + e * np.cos(psi[at]), psi[at] + rng.uniform(-0.05, 0.05, size=B), rng.uniform(5.0, 9.0, size=B),
              rng.uniform(-0.1, 0.1, size=B), rng.uniform(-0.05, 0.05, size=B), rng.uniform(-0.03, 0.03, size=B)]
    runs, ins = {}, {}
    for name in ("single", "bank_k1", "lane"):
        fc = FleetController(T_HORIZON, N, OPT_DT, B)
        ins[name] = [torch.as_tensor(a, dtype=torch.float64, device=fc.device) for a in (spread if name == "lane" else poses(B, p))]
        zero = torch.zeros(B, dtype=torch.int32, device=fc.device)
        if name == "single":
            fc.set_traj(*p)
            runs[name] = (fc, lambda fc=fc: fc.step(*ins["single"]))
        elif name == "bank_k1":
            fc.set_paths([p])
            runs[name] = (fc, lambda fc=fc, zero=zero: fc.step_paths(zero, *ins["bank_k1"]))
        else:
            fc.set_paths([p])
            runs[name] = (fc, lambda fc=fc, zero=zero: fc.step_route(zero, *ins["lane"], lane=lane))
    times = {name: [] for name in runs}
    for _ in range(repeats):
        for name, (fc, fn) in runs.items():
            times[name].append(timed(fn, steps, warmup))
    share = {name: float(fc.valid.float().mean().item()) for name, (fc, _) in runs.items()}
    for fc, _ in runs.values():
        fc.close()
    return times, share


def route_poses(M, B):
    """The route of M waypoints and B poses 0.3 m beside it, 5 .. 9 m/s."""
    p = path(M)
    x, y, psi, _ = p
    rng = np.random.default_rng(1)
    at = rng.integers(0, M - 50, size=B)
    e = 0.3 * (-1.0) ** np.arange(B)
    return p, [x[at] - e * np.sin(psi[at]), y[at] + e * np.cos(psi[at]), psi[at] + rng.uniform(-0.05, 0.05, size=B), rng.uniform(5.0, 9.0, size=B),
               rng.uniform(-0.1, 0.1, size=B), rng.uniform(-0.05, 0.05, size=B), rng.uniform(-0.03, 0.03, size=B)]


LEARN = [dict(feat=3, out=3, lo=[2.0], hi=[12.0], bins=[8], length_scale=2.0),
         dict(feat=[3, 6], out=4, lo=[2.0, -0.3], hi=[12.0, 0.3], bins=[8, 4], length_scale=[2.0, 0.2]),
         dict(feat=[3, 6], out=5, lo=[2.0, -0.3], hi=[12.0, 0.3], bins=[8, 4], length_scale=[2.0, 0.2])]


def rollout_observed(N, B, T, repeats, M=2000, lane=64):
    """Seconds per step of one rollout_route of T steps: of a controller that does not learn (`nominal`), of one that learns three
    regressors, its placeholder GPs in the model, without observing (`learn`) and observing every step (`observe`); and seconds per
    fit_gp with the install (`fit_install`) on a fourth controller whose bins are all filled (8, 32 and 32 points).  Interleaved, poses and lane_idx sent back before every repeat as in rollout_against_steps."""
    p, spread = route_poses(M, B)
    runs = {}
    for name in ("nominal", "learn", "observe"):
        fc = FleetController(T_HORIZON, N, OPT_DT, B, learn=None if name == "nominal" else LEARN)
        fc.set_paths([p])
        first = [torch.as_tensor(a, dtype=torch.float64, device=fc.device) for a in spread]
        ins = [t.clone() for t in first]
        zero = torch.zeros(B, dtype=torch.int32, device=fc.device)
        fn = lambda fc=fc, ins=ins, zero=zero, obs=name == "observe": fc.rollout_route(zero, *ins, steps=T, lane=lane, observe=obs)
        runs[name] = (fc, fn, first, ins)
    # the fit is timed on a controller of its own, whose rollout is not: every bin of its three regressors holds hand-made statistics
    fitter = FleetController(T_HORIZON, N, OPT_DT, 64, learn=LEARN)
    stats = np.zeros((4, 32, 5))
    for g, d in enumerate(LEARN):
        nb = list(d["bins"])
        for k in range(int(np.prod(nb))):
            idx = np.unravel_index(k, nb)
            z = [d["lo"][i] + (idx[i] + 0.5) * (d["hi"][i] - d["lo"][i]) / nb[i] for i in range(len(nb))]
            stats[g, k, 0], stats[g, k, 1:1 + len(nb)], stats[g, k, 4] = 5.0, 5.0 * np.array(z), 5.0 * np.sin(z[0]) * np.cos(3.0 * z[-1])
    fitter.bins.copy_(torch.as_tensor(stats, device=fitter.device))
    times = {name: [] for name in list(runs) + ["fit_install"]}
    for r in range(repeats + 1):                                   # the first round is the warm-up
        for name, (fc, fn, first, ins) in runs.items():
            fc.reset()
            for t, f in zip(ins, first):
                t.copy_(f)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(a.elapsed_time(b) * 1e-3 / T)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fit_info, fit_installed = fitter.fit_gp(min_count=1)       # filled bins: 8, 32 and 32 points are factorised and installed
        b.record()
        torch.cuda.synchronize()
        if r:
            times["fit_install"].append(a.elapsed_time(b) * 1e-3)
    fc = runs["observe"][0]
    bins, dropped = fc.bins.cpu().numpy(), fc.dropped.cpu().numpy()
    info = {"samples_binned": [float(v) for v in bins[:3, :, 0].sum(axis=1)], "dropped": [int(v) for v in dropped],
            "fit_points": fit_info.cpu().tolist(), "fit_installed": fit_installed.cpu().tolist()}
    fitter.close()
    for fc, _, _, _ in runs.values():
        fc.close()
    return times, info


def rollout_against_steps(N, B, T, repeats, M=2000, lane=64):
    """Seconds per step of one rollout_route of T steps and of T back-to-back step_route calls, on the route and the poses of
    lane_against_bank.  The rollout moves its vehicles, so every repeat copies the first poses back and sends lane_idx back to a search
    of the whole route, for both variants, outside the timed window."""
    p, spread = route_poses(M, B)
    runs = {}
    for name in ("rollout", "step_route"):
        fc = FleetController(T_HORIZON, N, OPT_DT, B)
        fc.set_paths([p])
        first = [torch.as_tensor(a, dtype=torch.float64, device=fc.device) for a in spread]
        ins = [t.clone() for t in first]
        zero = torch.zeros(B, dtype=torch.int32, device=fc.device)
        if name == "rollout":
            fn = lambda fc=fc, ins=ins, zero=zero: fc.rollout_route(zero, *ins, steps=T, lane=lane)
        else:
            def fn(fc=fc, ins=ins, zero=zero):
                for _ in range(T):
                    fc.step_route(zero, *ins, lane=lane)
        runs[name] = (fc, fn, first, ins)
    times = {name: [] for name in runs}
    for r in range(repeats + 1):                                   # the first round is the warm-up
        for name, (fc, fn, first, ins) in runs.items():
            fc.reset()
            for t, f in zip(ins, first):
                t.copy_(f)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(a.elapsed_time(b) * 1e-3 / T)
    fc = runs["rollout"][0]
    counts, tally = fc.counts.cpu().numpy(), fc.tally.cpu().numpy()
    info = {"mpc_share": float(counts[:, 1].mean() / T), "unusable_share": float(counts[:, 2].mean() / T), "max_abs_e_y": float(tally[:, 2].max())}
    for fc, _, _, _ in runs.values():
        fc.close()
    return times, info


def argmin_groups_against_argmin(steps, warmup, repeats):
    """Seconds per call of admpc_argmin_groups at (G, group) and of admpc_argmin over G * group entries."""
    fc = FleetController(T_HORIZON, 20, OPT_DT, 4)
    eng, L = fc._eng, fc.lib
    out = []
    for G, group in ((4096, 4), (64, 1024)):
        cost = torch.rand(G * group, dtype=torch.float64, device=fc.device)
        val, idx = torch.empty(G, dtype=torch.float64, device=fc.device), torch.empty(G, dtype=torch.int64, device=fc.device)
        p = lambda t: t.data_ptr()
        groups = lambda: L.admpc_argmin_groups(eng._h, p(cost), G, group, p(val), p(idx), eng._stream())
        whole = lambda: L.admpc_argmin(eng._h, p(cost), G * group, 0, p(val), p(idx), eng._stream())
        t = {"groups": [], "argmin": []}
        for _ in range(repeats):
            t["groups"].append(timed(groups, steps, warmup)); t["argmin"].append(timed(whole, steps, warmup))
        out.append((G, group, t))
    fc.close()
    return out


def per_vehicle_loop(N, p, calls):
    from ad_mpc_amd.ref_traj import RefTrajectory
    mpc = ROSGPMPC(T_HORIZON, N, OPT_DT)
    rt = RefTrajectory(traj_horizon=N, traj_dt=T_HORIZON / N)
    rt.set_traj(*p)
    ps = poses(calls, p, seed=1)

    def one(i):
        px, py, yaw, vx, vy, r, steer = (float(a[i]) for a in ps)
        wd = rt.get_waypoints(px, py, yaw)
        vel = host.resample_vel(wd["v_ref"], vx, vy, mpc.ad.acc_max, T_HORIZON / N)
        ref = np.zeros([7, N]); ref[0], ref[1], ref[2], ref[3] = wd["x_ref"], wd["y_ref"], wd["psi_ref"], vel
        mpc.set_state([px, py, yaw, vx, vy, r, steer])
        mpc.set_reference(ref.T, np.zeros((N - 1, 2)), False)
        mpc.optimize(0)
    for i in range(min(20, calls)):
        one(i)
    t0 = time.perf_counter()
    for i in range(calls):
        one(i)
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--horizons", default="20,40")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--loop-calls", type=int, default=200)
    ap.add_argument("--bank", action="store_true", help="the bank of paths against the single-path step, and the arg-min per group")
    ap.add_argument("--lane", action="store_true", help="the step along a route against the bank step and the single-path step")
    ap.add_argument("--rollout", type=int, default=0, metavar="T", help="one rollout of T closed-loop steps against T step_route calls")
    ap.add_argument("--observe", action="store_true", help="with --rollout T: the rollout with and without the observation of every step")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    p = path()
    gpu = torch.cuda.get_device_name(0)
    if a.rollout:
        us = lambda ts: [round(t * 1e6, 1) for t in ts]
        med = lambda ts: float(np.median(ts))
        for N in [int(v) for v in a.horizons.split(",")]:
            for B in [int(v) for v in (a.batches if a.batches != "1,64,4096" else "4096").split(",")]:
                if a.observe:
                    t, info = rollout_observed(N, B, a.rollout, a.repeats)
                    print(json.dumps({"what": "fleet_rollout_observe", "N": N, "B": B, "T": a.rollout, "route_waypoints": 2000, "L": 64, "regressors": len(LEARN),
                                      "us": {k: us(v) for k, v in t.items()}, "median_us": {k: round(med(v) * 1e6, 1) for k, v in t.items()},
                                      "spread_us": {k: round((max(v) - min(v)) * 1e6, 1) for k, v in t.items()},
                                      "observe_minus_learn_us": round((med(t["observe"]) - med(t["learn"])) * 1e6, 1),
                                      "learn_minus_nominal_us": round((med(t["learn"]) - med(t["nominal"])) * 1e6, 1), **info, "gpu": gpu}), flush=True)
                    continue
                t, info = rollout_against_steps(N, B, a.rollout, a.repeats)
                print(json.dumps({"what": "fleet_rollout", "N": N, "B": B, "T": a.rollout, "route_waypoints": 2000, "L": 64,
                                  "us_per_step": {k: us(v) for k, v in t.items()}, "median_us": {k: round(med(v) * 1e6, 1) for k, v in t.items()},
                                  "spread_us": {k: round((max(v) - min(v)) * 1e6, 1) for k, v in t.items()},
                                  "rollout_minus_step_route_us": round((med(t["rollout"]) - med(t["step_route"])) * 1e6, 1), **info, "gpu": gpu}),
                      flush=True)
        return
    if a.lane:
        us = lambda ts: [round(t * 1e6, 1) for t in ts]
        med = lambda ts: float(np.median(ts))
        for N in [int(v) for v in a.horizons.split(",")]:
            for B in [int(v) for v in (a.batches if a.batches != "1,64,4096" else "4096").split(",")]:
                t, share = lane_against_bank(N, B, a.steps, a.warmup, a.repeats)
                print(json.dumps({"what": "fleet_step_lane", "N": N, "B": B, "route_waypoints": 2000, "L": 64,
                                  "us_per_step": {k: us(v) for k, v in t.items()}, "median_us": {k: round(med(v) * 1e6, 1) for k, v in t.items()},
                                  "vehicles_per_s": {k: round(B / med(v), 1) for k, v in t.items()},
                                  "lane_rate_over_bank_rate": round(med(t["bank_k1"]) / med(t["lane"]), 4), "valid_share": share, "gpu": gpu}), flush=True)
        return
    if a.bank:
        us = lambda ts: [round(t * 1e6, 1) for t in ts]
        med = lambda ts: float(np.median(ts))
        for N in [int(v) for v in a.horizons.split(",")]:
            for B in [int(v) for v in (a.batches if a.batches != "1,64,4096" else "4096").split(",")]:
                t = bank_against_single(N, B, p, a.steps, a.warmup, a.repeats)
                print(json.dumps({"what": "fleet_step_bank", "N": N, "B": B, "us_per_step": {k: us(v) for k, v in t.items()},
                                  "median_us": {k: round(med(v) * 1e6, 1) for k, v in t.items()},
                                  "vehicles_per_s": {k: round(B / med(v), 1) for k, v in t.items()},
                                  "bank_k1_over_single": round(med(t["bank_k1"]) / med(t["single"]), 4),
                                  "bank_k8_over_single": round(med(t["bank_k8"]) / med(t["single"]), 4), "gpu": gpu}), flush=True)
        for G, group, t in argmin_groups_against_argmin(a.steps, a.warmup, a.repeats):
            print(json.dumps({"what": "argmin_groups", "G": G, "group": group, "us_per_call": {k: us(v) for k, v in t.items()},
                              "median_us": {k: round(med(v) * 1e6, 2) for k, v in t.items()}, "gpu": gpu}), flush=True)
        return
    for N in [int(v) for v in a.horizons.split(",")]:
        t_loop = per_vehicle_loop(N, p, a.loop_calls)
        print(json.dumps({"what": "per_vehicle_rosgpmpc_loop", "N": N, "vehicles_per_s": round(1.0 / t_loop, 1),
                          "us_per_vehicle": round(t_loop * 1e6, 1), "gpu": gpu}), flush=True)
        for B in [int(v) for v in a.batches.split(",")]:
            t_step, t_solve, mode1 = fleet_and_bare(N, B, p, a.steps, a.warmup)
            print(json.dumps({"what": "fleet_step", "N": N, "B": B, "vehicles_per_s": round(B / t_step, 1), "us_per_step": round(t_step * 1e6, 1),
                              "bare_solve_vehicles_per_s": round(B / t_solve, 1), "us_per_bare_solve": round(t_solve * 1e6, 1),
                              "step_over_solve": round(t_step / t_solve, 3), "vs_loop": round(t_loop * B / t_step, 1),
                              "mpc_mode_share": round(mode1, 3), "gpu": gpu}), flush=True)


if __name__ == "__main__":
    main()
