"""Times the evaluation of the learned GPs on the flight log of include/admpc_quad_eval.h (ad_mpc_amd/quad_ensemble_fleet.py: factor_gp,
evaluate_log) against the route it replaces, at B = 4096 vehicles and 60 logged steps (M = 245 760 records), N = 10, for K = 1, 4 and 8
clusters on the body-frame v_x with three 32-point regressors each: every vehicle on one long circle_reference (5 m, 3 m/s) from a start
row of its own, drag on, the simulator's disturbances on.  The fleet flies its 60 observed and logged steps once; the centroids are then
set to the quantiles of the logged v_x, so that every cluster holds records and the clusters alternate inside a wave; the bins are
hand-filled so that every regressor has all 32 points (the cost of a record depends on n alone).

On the device, as captured graphs replayed (`--replays` per window, `--windows` windows), the forms alternating, three times each:
  factor         admpc_quad_ensemble_factor: one launch, one wave per (cluster, regressor)
  evaluate       evaluate_log(): info zeroed, the evaluate kernel, the one-wave finish
  evaluate_per   evaluate_log(per_record=True): the same with mean and standard deviation of every record written
The route they replace, on the host, three times:
  download       the log to the host
  numpy_predict  tests/quad_eval_spec.py's evaluate in float64 over all records from the device's factors: route, predict, statistics
Every figure is the median of the three with the smallest and the largest.  The kernels' own times come from running
`rocprofv3 --kernel-trace --stats -- python scripts/quad_eval_time.py --brief` in a run of its own (--brief: the device forms only).

    python scripts/quad_eval_time.py [--replays 5] [--windows 10] [--brief] [--clusters 1 4 8] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import learn_spec as LS  # noqa: E402
import quad_eval_spec as EV  # noqa: E402
from quad_clusters_time import LEARN, three  # noqa: E402
from quad_rollout_time import B, OVER, emit, graph_capture, graph_measure  # noqa: E402
from ad_mpc_amd.quad_config import SimQuad  # noqa: E402
from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet  # noqa: E402
from ad_mpc_amd.quad_scenarios import circle_reference  # noqa: E402

T, N = 60, 10
FORMS = ("factor", "evaluate", "evaluate_per")


def one(K, a):
    rng = np.random.default_rng(0)
    fl = QuadEnsembleFleet(B, quad=SimQuad(drag=True, noisy=True, motor_noise=True), n_nodes=N, reference_over_sampling=OVER,
                           centroids=np.linspace(-1.0, 1.0, K).reshape(K, 1) if K > 1 else np.zeros((1, 1)), feats=[7], learn=[LEARN] * K, log_steps=T,
                           noise_seed=1)
    traj, u = circle_reference(2000 + T + 400, fl.control_period, 5.0, 3.0)
    fl.set_trajectories([(traj, u)])
    idx0 = rng.integers(0, 2000, B)
    x0 = traj[idx0].copy()
    x0[:, 0:3] += rng.uniform(-0.2, 0.2, (B, 3))
    fl.reset(0, idx0, x0)
    fl.rollout(T, observe=True, log=True)
    torch.cuda.synchronize()
    log = fl.log.cpu().numpy().reshape(-1, 14)
    ok = log[:, 13] == 1.0
    if K > 1:
        fl.set_centroids(np.quantile(log[ok, 0], (np.arange(K) + 0.5) / K).reshape(K, 1))
    stats = np.stack([np.stack([LS.hand_stats(fl._obs[c].gp[g], rng, 32) for g in range(3)]) for c in range(K)])
    fl.bins.copy_(torch.as_tensor(stats))
    fl.factor_gp()
    calls = {"factor": fl.factor_gp, "evaluate": fl.evaluate_log, "evaluate_per": lambda: fl.evaluate_log(per_record=True)}
    fl.evaluate_log(per_record=True)                                   # the tensor is allocated outside the captures
    graphs = {form: graph_capture(calls[form], a.replays) for form in FORMS}
    meds = {form: [] for form in FORMS}
    for _ in range(3):
        for form in FORMS:
            meds[form].append(graph_measure(graphs[form], 1, a.replays, a.windows)[0])
    r = {form: three(meds[form]) for form in FORMS}
    torch.cuda.synchronize()
    e = fl.evaluation()
    r.update(info=fl.eval_info.cpu().tolist(), points=fl.factor_info.cpu().tolist(), count=e.count.tolist(),
             ratio=(e.total.augmented_rms / e.total.nominal_rms).tolist(), within_3std=e.total.within_3std.tolist(), clipped=e.total.clipped.tolist())
    if not a.brief:
        host = {"download": [], "numpy_predict": []}
        cent = fl._device_centroids()
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = fl.log.cpu().numpy().reshape(-1, 14)
            blocks = fl.factor.cpu().numpy()
            t1 = time.perf_counter()
            want = EV.evaluate(rec, [7], cent, [[EV.unpack(blocks[c, g]) for g in range(3)] for c in range(K)])
            t2 = time.perf_counter()
            host["download"].append((t1 - t0) * 1e6)
            host["numpy_predict"].append((t2 - t1) * 1e6)
        r.update({name: three(v) for name, v in host.items()})
        r["host_route"] = sum(r[name][0] for name in host)
        r["host_route_over_device"] = r["host_route"] / r["evaluate"][0]
        dev = fl.eval_stats.cpu().numpy()
        r["info_equal"] = bool(np.array_equal(want["info"], np.array(r["info"], dtype=np.int32)))
        with np.errstate(all="ignore"):
            r["max_relative_difference_of_the_sums"] = float(np.nanmax(np.abs(dev - want["stats"]) / np.abs(want["stats"])))
    fl.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--brief", action="store_true")
    ap.add_argument("--clusters", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_eval_time.py measures on the GPU"
    res = {"case": "B = %d, %d logged steps (M = %d), N = %d, over-sampling %d, drag on, noisy and motor_noise, circle 5 m at 3 m/s, three 32-point "
                   "regressors per cluster" % (B, T, B * T, N, OVER),
           "replays_per_window": a.replays, "windows": a.windows, "alternations": 3,
           "microseconds": "median, smallest, largest of three", "device": torch.cuda.get_device_name(0)}
    for K in a.clusters:
        res["k%d" % K] = one(K, a)
    emit(res, a.out)


if __name__ == "__main__":
    main()
