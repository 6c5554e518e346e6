"""Times the selection of the GP training points from the flight log, include/admpc_quad_select.h
(ad_mpc_amd/quad_ensemble_fleet.py: select_points), against the re-bin it stands beside and the route it replaces, at B = 4096
vehicles and 60 logged steps (M = 245 760 records), K = 1, 4 and 8 clusters on the body-frame v_x, three one-feature regressors,
N = 10: every vehicle on one long circle_reference (5 m, 3 m/s) from a start row of its own, drag on.  The fleet flies its 60 observed
and logged steps once per K; everything below works on that log.

On the device, as captured graphs replayed (`--replays` per window, `--windows` windows), the forms alternating, three times each:
  select20       select_points(20): the 22 launches of admpc_quad_ensemble_select_points
  select32       select_points(32)
  rebin          rebin(): the bins zeroed and the 60 bin launches of admpc_quad_clusters_rebin
The route the selection replaces, on the host, alternating with the device's select20, three times:
  download       the log to the host
  numpy_select   tests/quad_select_spec.py's select_log at n_points 20
  upload         the rows back into the device's bins
Every figure is the median of the three with the smallest and the largest.  The kernels' own times come from running
`rocprofv3 --kernel-trace --stats -- python scripts/quad_select_time.py --brief` in a run of its own (--brief: K = 4, the device forms
only).

    python scripts/quad_select_time.py [--replays 5] [--windows 10] [--brief] [--out FILE]
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

import quad_select_spec as SS  # noqa: E402
from quad_clusters_time import LEARN, three  # noqa: E402
from quad_rollout_time import B, OVER, emit, graph_capture, graph_measure  # noqa: E402
from ad_mpc_amd.quad_config import SimQuad  # noqa: E402
from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet  # noqa: E402
from ad_mpc_amd.quad_scenarios import circle_reference  # noqa: E402

T, N = 60, 10
FORMS = ("select20", "select32", "rebin")
REGS = [(7, 7), (8, 8), (9, 9)]


def one(K, a):
    cent = np.linspace(-3.0, 0.5, K).reshape(K, 1) if K > 1 else np.array([[-1.5]])
    fl = QuadEnsembleFleet(B, quad=SimQuad(drag=True), n_nodes=N, reference_over_sampling=OVER, centroids=cent, feats=[7],
                           learn=[LEARN] * K, log_steps=T)
    traj, u = circle_reference(2000 + T + 400, fl.control_period, 5.0, 3.0)
    fl.set_trajectories([(traj, u)])
    rng = np.random.default_rng(0)
    idx0 = rng.integers(0, 2000, B)
    x0 = traj[idx0].copy()
    x0[:, 0:3] += rng.uniform(-0.2, 0.2, (B, 3))
    fl.reset(0, idx0, x0)
    fl.rollout(T, observe=True, log=True)
    torch.cuda.synchronize()
    calls = {"select20": lambda: fl.select_points(20), "select32": lambda: fl.select_points(32), "rebin": fl.rebin}
    graphs = {form: graph_capture(calls[form], a.replays) for form in FORMS}
    meds = {form: [] for form in FORMS}
    host = {"download": [], "numpy_select": [], "upload": []}
    for _ in range(3):
        for form in FORMS:
            meds[form].append(graph_measure(graphs[form], 1, a.replays, a.windows)[0])
        if a.brief:
            continue
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec = fl.log.cpu().numpy().reshape(-1, 14)
        t1 = time.perf_counter()
        want = SS.select_log(rec, cent, [7], REGS, [20, 20, 20])
        t2 = time.perf_counter()
        fl.bins.copy_(torch.as_tensor(want[0]))
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        for name, dt in zip(("download", "numpy_select", "upload"), (t1 - t0, t2 - t1, t3 - t2)):
            host[name].append(dt * 1e6)
    r = {form: three(meds[form]) for form in FORMS}
    r["select20_over_rebin"] = r["select20"][0] / r["rebin"][0]
    if not a.brief:
        r.update({name: three(v) for name, v in host.items()})
        r["host_route"] = sum(r[name][0] for name in host)
        r["host_route_over_device"] = r["host_route"] / r["select20"][0]
        graphs["select20"].replay()
        torch.cuda.synchronize()
        r["sel_equal"] = bool(np.array_equal(fl.sel.cpu().numpy(), want[1]))
        r["bins_equal"] = bool(np.array_equal(fl.bins.cpu().numpy().view(np.uint64), want[0].view(np.uint64)))
        r["info"] = fl.select_info.cpu().numpy()[:, :, :3].tolist()
    fl.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--brief", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_select_time.py measures on the GPU"
    res = {"case": "B = %d, %d logged steps (M = %d), three one-feature regressors, N = %d, over-sampling %d, drag on, circle 5 m at 3 m/s" % (B, T, B * T, N, OVER),
           "replays_per_window": a.replays, "windows": a.windows, "alternations": 3,
           "microseconds": "median, smallest, largest of three", "device": torch.cuda.get_device_name(0)}
    for K in ((4,) if a.brief else (1, 4, 8)):
        res["k%d" % K] = one(K, a)
    emit(res, a.out)


if __name__ == "__main__":
    main()
