"""Times the prune of the flight log and the RDRv drag fit of include/admpc_quad_prune.h (ad_mpc_amd/quad_ensemble_fleet.py: prune_log,
fit_rdrv) against the route they replace, at B = 4096 vehicles and 60 logged steps (M = 245 760 records), K = 1, N = 10: every vehicle on
one long circle_reference (5 m, 3 m/s) from a start row of its own, drag on, the simulator's disturbances on (noisy and motor_noise, the
reference's default data collection).  The fleet flies its 60 observed and logged steps once; everything below works on that log.

On the device, as captured graphs replayed (`--replays` per window, `--windows` windows), the forms alternating, three times each:
  prune          admpc_quad_records_prune at the reference's ModelFitConfig (x_cap 16, 40 bins, thresh 0.001): range, edges, count, mark
  prune_rebin    prune_log() as a fleet calls it: the prune, the bins zeroed, the re-bin of the 60 steps
  rdrv           fit_rdrv() with the install: the block sums, the finish, one install
The route they replace, on the host, three times:
  download       the log to the host
  numpy_prune    tests/quad_prune_spec.py's prune, the vectorised restatement of the reference's prune_dataset
  sklearn_rdrv   LinearRegression(fit_intercept=False) per axis on the kept records, as rdrv_fitting.linear_rdrv_fitting
  upload         the flags back into the device's log
Every figure is the median of the three with the smallest and the largest.  Then the held-out flight: the fleet, with the drag installed,
flies 60 steps from other start rows twice, observed by the nominal model and by the handle that holds the learned drag
(set_observer(learned=True)); the root mean square of the residual y per body axis of either is printed.  The kernels' own times come
from running `rocprofv3 --kernel-trace --stats -- python scripts/quad_prune_time.py --brief` in a run of its own (--brief: the device
forms only, few replays).

    python scripts/quad_prune_time.py [--replays 5] [--windows 10] [--brief] [--out FILE]
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

import quad_prune_spec as PS  # noqa: E402
from quad_clusters_time import LEARN, three  # noqa: E402
from quad_rollout_time import B, OVER, emit, graph_capture, graph_measure  # noqa: E402
from ad_mpc_amd.quad_config import SimQuad  # noqa: E402
from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet  # noqa: E402
from ad_mpc_amd.quad_scenarios import circle_reference  # noqa: E402

T, N = 60, 10
FORMS = ("prune", "prune_rebin", "rdrv")


def rms(fl):
    torch.cuda.synchronize()
    log = fl.log.cpu().numpy().reshape(-1, 14)
    ok = log[:, 13] == 1.0
    return np.sqrt((log[ok, 10:13] ** 2).mean(axis=0)).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--brief", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_prune_time.py measures on the GPU"
    res = {"case": "B = %d, %d logged steps (M = %d), K = 1, N = %d, over-sampling %d, drag on, noisy and motor_noise, circle 5 m at 3 m/s" % (B, T, B * T, N, OVER),
           "replays_per_window": a.replays, "windows": a.windows, "alternations": 3,
           "microseconds": "median, smallest, largest of three", "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(0)
    fl = QuadEnsembleFleet(B, quad=SimQuad(drag=True, noisy=True, motor_noise=True), n_nodes=N, reference_over_sampling=OVER, centroids=np.zeros((1, 1)),
                           feats=[7], learn=[LEARN], log_steps=T, noise_seed=1)
    traj, u = circle_reference(2000 + T + 400, fl.control_period, 5.0, 3.0)
    fl.set_trajectories([(traj, u)])

    def start(seed_rng):
        idx0 = seed_rng.integers(0, 2000, B)
        x0 = traj[idx0].copy()
        x0[:, 0:3] += seed_rng.uniform(-0.2, 0.2, (B, 3))
        fl.reset(0, idx0, x0)

    start(rng)
    fl.rollout(T, observe=True, log=True)
    torch.cuda.synchronize()
    calls = {"prune": lambda: fl.prune_log(rebin=False), "prune_rebin": fl.prune_log, "rdrv": fl.fit_rdrv}
    graphs = {form: graph_capture(calls[form], a.replays) for form in FORMS}
    meds = {form: [] for form in FORMS}
    for _ in range(3):
        for form in FORMS:
            meds[form].append(graph_measure(graphs[form], 1, a.replays, a.windows)[0])
    r = {form: three(meds[form]) for form in FORMS}
    torch.cuda.synchronize()
    r.update(prune_info=fl.prune_info.cpu().tolist(), rdrv_info=fl.rdrv_info.cpu().tolist(), rdrv_installed=fl.rdrv_installed.cpu().tolist(),
             drag=np.diag(fl.learned_rdrv()).tolist())
    r["kept_share"] = r["prune_info"][2] / max(1, r["prune_info"][1])
    if not a.brief:
        from sklearn.linear_model import LinearRegression
        host = {"download": [], "numpy_prune": [], "sklearn_rdrv": [], "upload": []}
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = fl.log.cpu().numpy().reshape(-1, 14)
            t1 = time.perf_counter()
            want = PS.prune(rec, 16.0, 40, 0.001)
            t2 = time.perf_counter()
            kept = want["records"][want["records"][:, 13] == 1.0]
            drag = [float(LinearRegression(fit_intercept=False).fit(kept[:, i, None], kept[:, 10 + i]).coef_[0]) for i in range(3)]
            t3 = time.perf_counter()
            fl.log[:, :, 13].copy_(torch.as_tensor(want["records"][:, 13].reshape(T, B)))
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            for name, dt in zip(("download", "numpy_prune", "sklearn_rdrv", "upload"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                host[name].append(dt * 1e6)
        r.update({name: three(v) for name, v in host.items()})
        r["host_route"] = sum(r[name][0] for name in host)
        r["host_route_over_device"] = r["host_route"] / (r["prune"][0] + r["rdrv"][0])
        r.update(host_info=want["info"].tolist(), host_margin=want["margin"], host_drag=drag,
                 flags_equal=bool(np.array_equal(fl.log.cpu().numpy().reshape(-1, 14)[:, 13], want["records"][:, 13])),
                 max_drag_difference=float(np.abs(np.array(drag) - np.array(r["drag"])).max()))
        # the held-out flight, flown by the handle with the drag installed, observed by the nominal model and by that handle
        held = {}
        for name, learned in (("nominal", False), ("learned", True)):
            start(np.random.default_rng(7))
            fl.reseed(step=10 ** 6)
            fl.set_observer(learned=learned)
            fl.log_reset()
            fl.rollout(T, observe=True, log=True)
            held[name] = rms(fl)
        r["held_out_rms_y"] = held
        r["held_out_ratio"] = [l / n for l, n in zip(held["learned"], held["nominal"])]
    fl.close()
    res["k1"] = r
    emit(res, a.out)


if __name__ == "__main__":
    main()
