"""Times a clustered GP ensemble in the quadrotor's closed loop (include/admpc_quad_ensemble.h; ad_mpc_amd/quad_ensemble_fleet.py) against
the single-handle loop (QuadFleet) at B = 4096, N = 10 and N = 20 (t_horizon 1 s, over-sampling 5, simulation_dt 5e-4), drag on, every
vehicle on one long circle_reference (5 m, 3 m/s) from a start row of its own, 0.2 m off the reference.

Per horizon five forms, every one with three regressors of 20 points per handle (hand-made statistics, fitted and installed on the
device, the same in every handle):
  plain          QuadFleet.rollout: admpc_quad_rollout_batch, one handle
  k1             QuadEnsembleFleet.rollout with one cluster: the routing launch, the route check and ONE routed solve on top of `plain`
  k4             ... with four clusters on the body-frame v_x (centroids -2.25, -0.75, 0.75, 2.25 m/s: the circle visits all of them):
                 four handles each passing over the whole batch
  k4_observed    `k4` with every step observed: the observe kernel and the ensemble's bin kernel behind the plant
  plain_observed `plain` with every step observed: the observe kernel and admpc_quad_bin_kernel

Every form is a captured graph of STEPS closed-loop steps; the graphs are captured once and then measured ALTERNATING, form after form,
three times each; every figure is the median of the three window medians with the smallest and the largest of them, in microseconds per
closed-loop step.  The kernels' own times (admpc_quad_ensemble_bin_kernel against admpc_quad_bin_kernel, the route kernel) come from
running the same command under `rocprofv3 --kernel-trace --stats`, in a run of its own.

    python scripts/quad_ensemble_time.py [--steps 10] [--replays 10] [--windows 20] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import learn_spec as LS  # noqa: E402  (hand-made statistics of a regressor)
from quad_rollout_time import B, OVER, emit, graph_capture, graph_measure  # noqa: E402
from ad_mpc_amd.quad_config import SimQuad  # noqa: E402
from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet  # noqa: E402
from ad_mpc_amd.quad_fleet import QuadFleet  # noqa: E402
from ad_mpc_amd.quad_scenarios import circle_reference  # noqa: E402

LEARN = [dict(feat=7 + i, out=7 + i, lo=[-4.0], hi=[4.0], bins=[32], length_scale=2.0, sigma_f=1.0, noise=1e-4, count_noise=1e-2) for i in range(3)]
CENT4 = [[-2.25], [-0.75], [0.75], [2.25]]
FORMS = ("plain", "k1", "k4", "k4_observed", "plain_observed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_ensemble_time.py measures on the GPU"
    res = {"case": "B = %d, t_horizon 1 s, over-sampling %d, simulation_dt 5e-4, drag on, circle 5 m at 3 m/s; three regressors of 20 points per handle" % (B, OVER),
           "steps_per_graph": a.steps, "replays_per_window": a.replays, "windows": a.windows, "alternations": 3,
           "microseconds": "per closed-loop step: median, smallest, largest of the three window medians", "device": torch.cuda.get_device_name(0)}
    rows = 2000 + 2 * a.steps * (1 + a.replays * (1 + 3 * a.windows)) + 400          # a fleet flies two of the forms
    for N in (10, 20):
        rng = np.random.default_rng(0)
        kw = dict(quad=SimQuad(drag=True), n_nodes=N, reference_over_sampling=OVER)
        fleets = {"plain": QuadFleet(B, learn=LEARN, **kw),
                  "k1": QuadEnsembleFleet(B, centroids=[[0.0]], feats=[7], learn=[LEARN], **kw),
                  "k4": QuadEnsembleFleet(B, centroids=CENT4, feats=[7], learn=[LEARN] * 4, **kw)}
        traj, u = circle_reference(rows, fleets["plain"].control_period, 5.0, 3.0)
        idx0 = rng.integers(0, 2000, B)
        x0 = traj[idx0].copy()
        x0[:, 0:3] += rng.uniform(-0.2, 0.2, (B, 3))
        stats = np.stack([LS.hand_stats(fleets["plain"]._obs.gp[g], np.random.default_rng(g), 20) for g in range(3)])
        for name, fl in fleets.items():
            fl.set_trajectories([(traj, u)])
            fl.reset(0, idx0, x0)
            fl.bins.copy_(torch.as_tensor(stats if name == "plain" else np.broadcast_to(stats, fl.bins.shape).copy()))
            info, installed = fl.fit_gp()
            assert int(info.min()) == 20 and int(installed.min()) == 1
            fl.observe_reset()
        graphs, owner = {}, {"plain": "plain", "k1": "k1", "k4": "k4", "k4_observed": "k4", "plain_observed": "plain"}
        for form in FORMS:
            fl = fleets[owner[form]]
            graphs[form] = graph_capture(lambda fl=fl, obs=form.endswith("observed"): fl.rollout(a.steps, observe=obs), a.replays)
        meds = {form: [] for form in FORMS}
        for _ in range(3):
            for form in FORMS:
                meds[form].append(graph_measure(graphs[form], a.steps, a.replays, a.windows)[0])
        r = {"substeps": int(fleets["plain"]._plant.substeps)}
        for form in FORMS:
            r[form] = [float(np.median(meds[form])), min(meds[form]), max(meds[form])]
        r["k1_minus_plain"] = r["k1"][0] - r["plain"][0]
        r["k4_over_plain"] = r["k4"][0] / r["plain"][0]
        r["k4_observed_minus_k4"] = r["k4_observed"][0] - r["k4"][0]
        r["plain_observed_minus_plain"] = r["plain_observed"][0] - r["plain"][0]
        torch.cuda.synchronize()
        r["clusters_of_the_last_period_k4"] = np.bincount(fleets["k4"].route.cpu().numpy(), minlength=4).tolist()
        for name, fl in fleets.items():
            assert int(fl.idx.max()) < rows - 1 - (N + 1) * OVER, "the fleet ran into the end of the reference"
            r["status_nonzero_steps_" + name] = int(fl.counts[:, 1].sum())
            r["tracking_rmse_mean_" + name] = float(fl.tracking_rmse().mean())
            fl.close()
        res["N%d" % N] = r
    emit(res, a.out)


if __name__ == "__main__":
    main()
