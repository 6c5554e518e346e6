"""Times the clustering of include/admpc_quad_clusters.h (ad_mpc_amd/quad_ensemble_fleet.py: fit_clusters) against the route it replaces,
at B = 4096 vehicles and 60 logged steps (M = 245 760 records), K = 4 clusters, on d = 1 (the body-frame v_x) and d = 3 (the body-frame
velocity) clustering features: every vehicle on one long circle_reference (5 m, 3 m/s) from a start row of its own, drag on, N = 10.  The
fleet flies its 60 observed and logged steps once; everything below works on that log, from the same poor initial means (the 5 %, 15 %,
50 % and 90 % quantiles of the logged first feature; the other features at their means).

On the device, as captured graphs replayed (`--replays` per window, `--windows` windows), the forms alternating, three times each:
  fit1, fit21    admpc_quad_clusters_fit with max_iter 1 and 21 at tol = 0: pack, start and that many EM iterations; their difference over
                 20 is one EM iteration (an E launch and an M launch), and fit1 less one iteration is the pack and the start
  clusters       fit_clusters() as a fleet calls it: the fit at sklearn's defaults (max_iter 100, tol 1e-3: the iterations behind the
                 convergence return at once), the install, the bins zeroed, the re-bin of the 60 steps
  rebin          the bins zeroed and the re-bin alone
The route it replaces, on the host, three times:
  download       the log to the host
  sklearn        GaussianMixture(4, weights_init, means_init, precisions_init) from the same start (the hard assignment to the nearest
                 initial mean, done in numpy and timed with it), sklearn's defaults otherwise
  upload_rebin   the new centroids uploaded (set_centroids) and a re-flight's worth of binning: `rebin` above (the re-flight itself, 60
                 closed-loop steps, is not counted)
Every figure is the median of the three with the smallest and the largest.  The kernels' own times come from running
`rocprofv3 --kernel-trace --stats -- python scripts/quad_clusters_time.py --brief` in a run of its own (--brief: the device forms only, few
replays).

    python scripts/quad_clusters_time.py [--replays 5] [--windows 10] [--brief] [--out FILE]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import quad_clusters_spec as CS  # noqa: E402  (the start step, for sklearn's *_init)
from quad_rollout_time import B, OVER, emit, graph_capture, graph_measure  # noqa: E402
from ad_mpc_amd.quad_config import SimQuad  # noqa: E402
from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet  # noqa: E402
from ad_mpc_amd.quad_scenarios import circle_reference  # noqa: E402

LEARN = [dict(feat=7 + i, out=7 + i, lo=[-4.0], hi=[4.0], bins=[32], length_scale=2.0, sigma_f=1.0, noise=1e-4, count_noise=1e-2) for i in range(3)]
K, T, N = 4, 60, 10
FORMS = ("fit1", "fit21", "clusters", "rebin")


def three(v):
    return [float(np.median(v)), float(min(v)), float(max(v))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--brief", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_clusters_time.py measures on the GPU"
    res = {"case": "B = %d, %d logged steps (M = %d), K = %d, N = %d, over-sampling %d, drag on, circle 5 m at 3 m/s" % (B, T, B * T, K, N, OVER),
           "replays_per_window": a.replays, "windows": a.windows, "alternations": 3,
           "microseconds": "median, smallest, largest of three", "device": torch.cuda.get_device_name(0)}
    for feats in ([7], [7, 8, 9]):
        d = len(feats)
        rng = np.random.default_rng(0)
        fl = QuadEnsembleFleet(B, quad=SimQuad(drag=True), n_nodes=N, reference_over_sampling=OVER, centroids=np.zeros((K, d)) + np.arange(K)[:, None],
                               feats=feats, learn=[LEARN] * K, log_steps=T)
        traj, u = circle_reference(2000 + T + 400, fl.control_period, 5.0, 3.0)
        idx0 = rng.integers(0, 2000, B)
        x0 = traj[idx0].copy()
        x0[:, 0:3] += rng.uniform(-0.2, 0.2, (B, 3))
        fl.set_trajectories([(traj, u)])
        fl.reset(0, idx0, x0)
        fl.rollout(T, observe=True, log=True)
        torch.cuda.synchronize()
        log = fl.log.cpu().numpy().reshape(-1, 14)
        z = log[log[:, 13] == 1.0][:, [f - 7 for f in feats]]
        poor = np.tile(z.mean(axis=0), (K, 1))
        poor[:, 0] = np.quantile(z[:, 0], [0.05, 0.15, 0.5, 0.9])
        start = torch.as_tensor(poor).to(fl.device)
        fit = lambda it: fl.fit_clusters(max_iter=it, tol=0.0, init=start, install=False, rebin=False)
        calls = {"fit1": lambda: fit(1), "fit21": lambda: fit(21), "clusters": lambda: fl.fit_clusters(init=start), "rebin": fl.rebin}
        graphs = {form: graph_capture(calls[form], a.replays) for form in FORMS}
        meds = {form: [] for form in FORMS}
        for _ in range(3):
            for form in FORMS:
                meds[form].append(graph_measure(graphs[form], 1, a.replays, a.windows)[0])
        r = {form: three(meds[form]) for form in FORMS}
        r["one_iteration"] = (r["fit21"][0] - r["fit1"][0]) / 20.0
        r["pack_and_start"] = r["fit1"][0] - r["one_iteration"]
        graphs["clusters"].replay()
        got = fl.learned_clusters()
        r.update(iterations=got.n_iter, converged=int(got.converged), status=got.status, n_valid=int(fl.gmm_info.cpu()[3]),
                 initial_means=poor.tolist(), centroids=fl.centroids.tolist(), weights=got.weights.tolist())
        if not a.brief:
            from sklearn.mixture import GaussianMixture
            host = {"download": [], "sklearn": [], "upload_rebin": []}
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rec = fl.log.cpu().numpy().reshape(-1, 14)
                t1 = time.perf_counter()
                packed = CS.pack(rec, feats)
                first, info = np.zeros((1 + K, CS.ROW)), np.zeros(4, dtype=np.int32)
                assert CS.start(packed, poor, d, 1e-6, first, info)
                w, m, c, P = CS.unpack(first, d)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    sk = GaussianMixture(K, covariance_type="full", weights_init=w / w.sum(), means_init=m, precisions_init=np.array([p @ p.T for p in P]),
                                         random_state=0).fit(packed[packed[:, 3] == 1.0, :d])
                t2 = time.perf_counter()
                fl.set_centroids(sk.means_[np.argsort(sk.means_[:, 0], kind="stable")])
                fl.rebin()
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                for name, dt in zip(("download", "sklearn", "upload_rebin"), (t1 - t0, t2 - t1, t3 - t2)):
                    host[name].append(dt * 1e6)
            r.update({name: three(v) for name, v in host.items()})
            r["host_route"] = r["download"][0] + r["sklearn"][0] + r["upload_rebin"][0]
            r["host_route_over_clusters"] = r["host_route"] / r["clusters"][0]
            r.update(sklearn_iterations=int(sk.n_iter_), sklearn_centroids=np.sort(sk.means_[:, 0]).tolist(),
                     max_centroid_difference=float(np.abs(fl._device_centroids() - got.means[got.perm]).max()))
        fl.close()
        res["d%d" % d] = r
    emit(res, a.out)


if __name__ == "__main__":
    main()
