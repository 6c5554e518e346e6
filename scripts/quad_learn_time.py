"""Times what learning costs the quadrotor's closed loop on the device (include/admpc_quad_learn.h; ad_mpc_amd/quad_fleet.py: learn=) at
B = 4096, N = 10 and N = 20 (t_horizon 1 s, over-sampling 5, simulation_dt 5e-4), drag on, every vehicle on one long circle_reference
(5 m, 3 m/s) from a start row of its own, 0.2 m off the reference -- the case of scripts/quad_rollout_time.py.

Every figure is a captured graph replayed K times between two HIP events, after a warm-up, repeated R times: the median and the 10th and
90th percentile of the R windows, in microseconds.
  unobserved    rollout(STEPS) of a fleet that learns (placeholder GPs: the GP path of the solve), per closed-loop step
  observed      rollout(STEPS, observe=True): the same with the latch and, behind every step, the observe and bin launches, per step
  observe       the two launches of observe() alone at the state the rollout left, per call
  fit_install   fit_gp(min_count=2) with install on the statistics the observed rollout gathered, per call (two launches)
The kernels' own times come from running this script under `rocprofv3 --kernel-trace --stats`, in a run of its own and without counters.

    python scripts/quad_learn_time.py [--steps 10] [--replays 10] [--windows 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from quad_rollout_time import B, OVER, ROWS, graph_time  # noqa: E402
from ad_mpc_amd.quad_config import SimQuad  # noqa: E402
from ad_mpc_amd.quad_fleet import QuadFleet  # noqa: E402
from ad_mpc_amd.quad_scenarios import circle_reference  # noqa: E402

LEARN = [dict(feat=7 + i, out=7 + i, lo=[-9.0], hi=[9.0], bins=[32], length_scale=2.0, sigma_f=1.0, noise=1e-4, count_noise=1e-2) for i in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_learn_time.py measures on the GPU"
    res = {"case": "B = %d, t_horizon 1 s, over-sampling %d, simulation_dt 5e-4, drag on, circle 5 m at 3 m/s, three regressors of one feature on 32 bins" % (B, OVER),
           "steps_per_graph": a.steps, "replays_per_window": a.replays, "windows": a.windows, "microseconds": "median, 10th, 90th percentile",
           "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(0)
    for N in (10, 20):
        fl = QuadFleet(B, quad=SimQuad(drag=True), n_nodes=N, reference_over_sampling=OVER, learn=LEARN)
        traj, u = circle_reference(ROWS, fl.control_period, 5.0, 3.0)
        fl.set_trajectories([(traj, u)])
        idx0 = rng.integers(0, 2000, B)
        x0 = traj[idx0].copy()
        x0[:, 0:3] += rng.uniform(-0.2, 0.2, (B, 3))
        r = {}
        for name, observe in (("unobserved", False), ("observed", True)):
            fl.reset(0, idx0, x0)
            fl.observe_reset()
            r[name] = graph_time(lambda: fl.rollout(a.steps, observe=observe), a.steps, a.replays, a.windows)
            torch.cuda.synchronize()
            assert int(fl.idx.max()) < ROWS - 1 - (N + 1) * OVER, "the fleet ran into the end of the reference"
        r["status_nonzero_steps"] = int(fl.counts[:, 1].sum())
        r["samples_binned_per_regressor"] = [float(v) for v in fl.bins[:, :, 0].sum(dim=1).cpu()]
        r["dropped"] = [int(v) for v in fl.dropped.cpu()]
        r["observed_over_unobserved"] = r["observed"][0] / r["unobserved"][0]
        bins, dropped = fl.bins.clone(), fl.dropped.clone()
        r["observe"] = graph_time(lambda: fl.observe(), 1, a.replays, a.windows)
        fl.bins.copy_(bins); fl.dropped.copy_(dropped)
        r["fit_install"] = graph_time(lambda: fl.fit_gp(min_count=2), 1, a.replays, a.windows)
        torch.cuda.synchronize()
        r["fit_info"], r["installed"] = [int(v) for v in fl.fit_info.cpu()], [int(v) for v in fl.installed.cpu()]
        res["N%d" % N] = r
        fl.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
