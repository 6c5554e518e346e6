"""Times the quadrotor's closed loop on the device (include/admpc_quad_fleet.h; ad_mpc_amd/quad_fleet.py: QuadFleet.rollout) at B = 4096,
N = 10 and N = 20 (t_horizon 1 s, over-sampling 5, simulation_dt 5e-4: 40 and 20 sub-steps a period), drag on, every vehicle on one long
circle_reference (5 m, 3 m/s) from a start row of its own, 0.2 m off the reference.

Every device figure is a captured graph of STEPS closed-loop steps replayed K times between two HIP events, after a warm-up, repeated R
times: the median per STEP and the 10th and 90th percentile of the R windows, in microseconds.
  rollout       admpc_quad_rollout_batch: window -> RTI step -> plant, the fleet moving on along the circle from replay to replay
  chunk_solve   the window and the solve alone, at the state the rollout left (the state and the index stand still)
  plant         the plant launch alone under w_opt[:, 0] (events around replays of the launch; the kernels' own times come from running
                this script under `rocprofv3 --kernel-trace --stats`, in a run of its own)
  host          the only route without this module: solve on the device, u[0] to the host, a vectorised numpy plant, the next window built
                on the host and uploaded -- host clock around three steps ending in a synchronise, a few repeats

With --noise the simulator's random disturbances (include/admpc_quad_noise.h; noisy and motor_noise both on, the reference's
simulation_disturbances) are measured against the deterministic simulator instead: per horizon two fleets, the same but for the
switches, their `rollout` and `plant` graphs captured once and then measured ALTERNATING, calm, noisy, calm, noisy, ..., three times
each; every figure is the median of the three window medians, with the smallest and the largest of them.  The kernels' own times come from
running the same command under `rocprofv3 --kernel-trace --stats`, in a run of its own.

    python scripts/quad_rollout_time.py [--steps 10] [--replays 10] [--windows 20] [--out FILE] [--noise]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import quad_plant_spec as QS  # noqa: E402  (the vectorised numpy plant of the host route)
from ad_mpc_amd.quad_config import SimQuad  # noqa: E402
from ad_mpc_amd.quad_fleet import QuadFleet  # noqa: E402
from ad_mpc_amd.quad_scenarios import circle_reference  # noqa: E402

B, OVER, ROWS = 4096, 5, 6000


def graph_capture(fn, replays):
    """fn (which enqueues some steps) run once, captured, and replayed `replays` times as a warm-up: the graph."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(replays):
        g.replay()
    torch.cuda.synchronize()
    return g


def graph_time(fn, steps, replays, windows):
    """(median, p10, p90) microseconds per step of fn (which enqueues `steps` steps), captured once and replayed."""
    return graph_measure(graph_capture(fn, replays), steps, replays, windows)


def graph_measure(g, steps, replays, windows):
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / (replays * steps))
    return [float(np.median(out)), float(np.percentile(out, 10)), float(np.percentile(out, 90))]


def host_window(traj, u, idx, N, over):
    """The closed form of the window for a fleet on one trajectory, vectorised: (yref [B,N,17], yref_e [B,13])."""
    M = traj.shape[0]
    L = np.minimum(N + 1, -(-(M - idx) // over))
    j = np.arange(N + 1)[None, :]
    rx = idx[:, None] + np.minimum(j, L[:, None] - 1) * over
    ru = idx[:, None] + np.minimum(j[:, :N], np.maximum(L[:, None] - 2, 0)) * over
    return np.concatenate((traj[rx[:, :N]], u[ru]), axis=2), traj[rx[:, N]]


def host_route(fl, traj, u, steps):
    """`steps` closed-loop steps with the plant and the window on the host; seconds per step."""
    x, idx = fl.x.cpu().numpy(), fl.idx.cpu().numpy().astype(np.int64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        yref, yref_e = host_window(traj, u, idx, fl.N, fl.over)
        fl.yref.copy_(torch.as_tensor(yref)); fl.yref_e.copy_(torch.as_tensor(yref_e)); fl.x.copy_(torch.as_tensor(x))
        fl._eng.solve(fl.x, fl.yref, fl.yref_e, fl.x_opt, fl.w_opt, fl.cost, fl.status, fl.iters)
        u0 = fl.w_opt[:, 0, :].cpu().numpy()                                   # synchronises
        x, _ = QS.step_fleet(fl._plant, x, u0)
        idx = np.minimum(idx + 1, traj.shape[0] - 1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def noise_against_calm(a):
    """--noise: the closed-loop step and the plant launch of a fleet under both disturbances against the deterministic fleet."""
    res = {"case": "B = %d, t_horizon 1 s, over-sampling %d, simulation_dt 5e-4, drag on, circle 5 m at 3 m/s; noisy and motor_noise on against both off" % (B, OVER),
           "steps_per_graph": a.steps, "replays_per_window": a.replays, "windows": a.windows, "alternations": 3,
           "microseconds": "per closed-loop step: median, smallest, largest of the three window medians", "device": torch.cuda.get_device_name(0)}
    rows = 2000 + 2 * a.steps * a.replays * (1 + 3 * a.windows) + 200
    for N in (10, 20):
        rng = np.random.default_rng(0)
        fleets = {"calm": QuadFleet(B, quad=SimQuad(drag=True), n_nodes=N, reference_over_sampling=OVER),
                  "noisy": QuadFleet(B, quad=SimQuad(drag=True, noisy=True, motor_noise=True), n_nodes=N, reference_over_sampling=OVER, noise_seed=1)}
        traj, u = circle_reference(rows, fleets["calm"].control_period, 5.0, 3.0)
        idx0 = rng.integers(0, 2000, B)
        x0 = traj[idx0].copy()
        x0[:, 0:3] += rng.uniform(-0.2, 0.2, (B, 3))
        graphs = {}
        for name, fl in fleets.items():
            fl.set_trajectories([(traj, u)])
            fl.reset(0, idx0, x0)
            graphs[name, "rollout"] = graph_capture(lambda fl=fl: fl.rollout(a.steps), a.replays)

            def plant(fl=fl):
                for _ in range(a.steps):
                    fl.plant_step(fl.w_opt[:, 0, :], fl.scratch_x)

            fl.scratch_x = fl.x.clone()                                            # the plant alone moves a copy, not the fleet
            graphs[name, "plant"] = graph_capture(plant, a.replays)
        r = {"substeps": int(fleets["calm"]._plant.substeps)}
        for what in ("rollout", "plant"):
            meds = {"calm": [], "noisy": []}
            for _ in range(3):
                for name in ("calm", "noisy"):
                    fleets[name].scratch_x.copy_(fleets[name].x)
                    meds[name].append(graph_measure(graphs[name, what], a.steps, a.replays, a.windows)[0])
            for name in ("calm", "noisy"):
                r["%s_%s" % (what, name)] = [float(np.median(meds[name])), min(meds[name]), max(meds[name])]
            r["%s_noisy_over_calm" % what] = r[what + "_noisy"][0] / r[what + "_calm"][0]
        for name, fl in fleets.items():
            torch.cuda.synchronize()
            assert int(fl.idx.max()) < rows - 1 - (N + 1) * OVER, "the fleet ran into the end of the reference"
            r["status_nonzero_steps_" + name] = int(fl.counts[:, 1].sum())
            r["tracking_rmse_mean_" + name] = float(fl.tracking_rmse().mean())
            fl.close()
        res["N%d" % N] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--noise", action="store_true", help="the noisy simulator against the deterministic one, alternating")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_rollout_time.py measures on the GPU"
    if a.noise:
        emit(noise_against_calm(a), a.out)
        return
    res = {"case": "B = %d, t_horizon 1 s, over-sampling %d, simulation_dt 5e-4, drag on, circle 5 m at 3 m/s" % (B, OVER),
           "steps_per_graph": a.steps, "replays_per_window": a.replays, "windows": a.windows, "microseconds": "median, 10th, 90th percentile per closed-loop step",
           "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(0)
    for N in (10, 20):
        fl = QuadFleet(B, quad=SimQuad(drag=True), n_nodes=N, reference_over_sampling=OVER)
        traj, u = circle_reference(ROWS, fl.control_period, 5.0, 3.0)
        fl.set_trajectories([(traj, u)])
        idx0 = rng.integers(0, 2000, B)
        x0 = traj[idx0].copy()
        x0[:, 0:3] += rng.uniform(-0.2, 0.2, (B, 3))
        fl.reset(0, idx0, x0)
        r = {"substeps": int(fl._plant.substeps)}
        r["rollout"] = graph_time(lambda: fl.rollout(a.steps), a.steps, a.replays, a.windows)
        torch.cuda.synchronize()
        assert int(fl.idx.max()) < ROWS - 1 - (N + 1) * OVER, "the fleet ran into the end of the reference"
        r["status_nonzero_steps"] = int(fl.counts[:, 1].sum())
        r["mean_ipm_iters_last_step"] = float(fl.iters.double().mean())
        r["tracking_rmse_mean"] = float(fl.tracking_rmse().mean())

        def chunk_solve():
            for _ in range(a.steps):
                fl.ref_chunk()
                fl._eng.solve(fl.x, fl.yref, fl.yref_e, fl.x_opt, fl.w_opt, fl.cost, fl.status, fl.iters)

        def plant():
            for _ in range(a.steps):
                fl.plant_step(fl.w_opt[:, 0, :])

        r["chunk_solve"] = graph_time(chunk_solve, a.steps, a.replays, a.windows)
        keep = fl.x.clone()
        r["plant"] = graph_time(plant, a.steps, a.replays, a.windows)
        fl.x.copy_(keep)
        host = [host_route(fl, traj, u, 3) for _ in range(a.host_repeats + 1)][1:]          # the first is the warm-up
        r["host"] = [1e6 * h for h in host]
        r["plant_share_of_rollout"] = r["plant"][0] / r["rollout"][0]
        r["host_over_rollout"] = float(np.median(r["host"])) / r["rollout"][0]
        res["N%d" % N] = r
        fl.close()
    emit(res, a.out)


def emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
