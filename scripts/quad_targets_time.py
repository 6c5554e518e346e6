"""Times the target flight on the device (include/admpc_quad_targets.h; ad_mpc_amd/quad_fleet.py: QuadFleet.rollout_targets) against the
flight along a circle (QuadFleet.rollout) at B = 4096, N = 10 and N = 20 (t_horizon 1 s, over-sampling 5, simulation_dt 5e-4: 40 and 20
sub-steps a period), drag on.

Per horizon two fleets of the same vehicle: `circle`, every vehicle on one long circle_reference (5 m, 3 m/s) as
scripts/quad_rollout_time.py flies it, and `targets`, every vehicle from the reference's start state towards random "aggressive" targets
(world radius 3 m, reached within 5 cm, the reference's recovery).  Their graphs of STEPS closed-loop periods are captured once and then
measured ALTERNATING, circle, targets, circle, targets, ..., three times each; every figure is the median of the three window medians,
with the smallest and the largest of them, in microseconds per period.  With --noise both fleets fly the simulator's random disturbances
(noisy and motor_noise on).  The kernels' own times -- admpc_quad_plant_period_kernel<NOISY, L, true> against admpc_quad_plant_kernel, or against
admpc_quad_plant_period_kernel<true, L, false> -- come from running the same command under `rocprofv3 --kernel-trace --stats`, in a run of its own.

    python scripts/quad_targets_time.py [--steps 10] [--replays 10] [--windows 20] [--out FILE] [--noise]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from quad_rollout_time import B, OVER, emit, graph_capture, graph_measure  # noqa: E402  (puts the repository root on sys.path)
from ad_mpc_amd.quad_config import SimQuad  # noqa: E402
from ad_mpc_amd.quad_fleet import QuadFleet  # noqa: E402
from ad_mpc_amd.quad_scenarios import circle_reference  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--noise", action="store_true", help="both fleets under noisy and motor_noise")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_targets_time.py measures on the GPU"
    res = {"case": "B = %d, t_horizon 1 s, over-sampling %d, simulation_dt 5e-4, drag on%s; rollout_targets (aggressive, R = 3 m, 5 cm) against rollout on a "
                   "circle of 5 m at 3 m/s" % (B, OVER, ", noisy and motor_noise on" if a.noise else ""),
           "steps_per_graph": a.steps, "replays_per_window": a.replays, "windows": a.windows, "alternations": 3,
           "microseconds": "per closed-loop period: median, smallest, largest of the three window medians", "device": torch.cuda.get_device_name(0)}
    rows = 2000 + 2 * a.steps * a.replays * (1 + 3 * a.windows) + 200
    quad = lambda: SimQuad(drag=True, noisy=a.noise, motor_noise=a.noise)
    seed = 1 if a.noise else None
    for N in (10, 20):
        rng = np.random.default_rng(0)
        circle = QuadFleet(B, quad=quad(), n_nodes=N, reference_over_sampling=OVER, noise_seed=seed)
        targets = QuadFleet(B, quad=quad(), n_nodes=N, reference_over_sampling=OVER, noise_seed=seed)
        traj, u = circle_reference(rows, circle.control_period, 5.0, 3.0)
        idx0 = rng.integers(0, 2000, B)
        x0 = traj[idx0].copy()
        x0[:, 0:3] += rng.uniform(-0.2, 0.2, (B, 3))
        circle.set_trajectories([(traj, u)])
        circle.reset(0, idx0, x0)
        targets.set_targets(seed=7)
        targets.reset_targets()
        graphs = {"circle": graph_capture(lambda: circle.rollout(a.steps), a.replays),
                  "targets": graph_capture(lambda: targets.rollout_targets(a.steps), a.replays)}
        meds = {"circle": [], "targets": []}
        for _ in range(3):
            for name in ("circle", "targets"):
                meds[name].append(graph_measure(graphs[name], a.steps, a.replays, a.windows)[0])
        r = {"substeps": int(circle._plant.substeps)}
        for name in meds:
            r["rollout_" + name] = [float(np.median(meds[name])), min(meds[name]), max(meds[name])]
        r["targets_over_circle"] = r["rollout_targets"][0] / r["rollout_circle"][0]
        torch.cuda.synchronize()
        assert int(circle.idx.max()) < rows - 1 - (N + 1) * OVER, "the fleet ran into the end of the reference"
        tc = targets.tcounts.cpu().numpy()
        r["periods_flown"] = int(tc[0, 2])
        r["targets_reached"], r["recoveries"], r["status_nonzero_periods"] = int(tc[:, 0].sum()), int(tc[:, 1].sum()), int(tc[:, 3].sum())
        r["status_nonzero_steps_circle"] = int(circle.counts[:, 1].sum())
        # what the two flights ask of the RTI step: the interior-point iterations of the last period's solve
        r["mean_ipm_iters_circle"], r["mean_ipm_iters_targets"] = float(circle.iters.double().mean()), float(targets.iters.double().mean())
        circle.close(); targets.close()
        res["N%d" % N] = r
    emit(res, a.out)


if __name__ == "__main__":
    main()
