"""Times the k-means start of include/admpc_quad_kmeans.h (ad_mpc_amd/quad_ensemble_fleet.py: fit_clusters(init="kmeans")) against the
route it replaces, at B = 4096 vehicles and 60 logged steps (M = 245 760 records), K = 4 clusters, on d = 1 (the body-frame v_x) and
d = 3 (the body-frame velocity): the flight of scripts/quad_clusters_time.py, flown once; everything below works on that log.

On the device, as captured graphs replayed (`--replays` per window, `--windows` windows), the forms alternating, three times each:
  km1, km11      admpc_quad_kmeans_fit with max_iter 1 and 11 at tol = 0: pack, prep, the seeding and that many Lloyd iterations; their
                 difference over the iterations that ran beyond the first (reported; 10 unless the labels stood still sooner, and then a
                 slight overestimate, since it carries the launches that return at once) is one Lloyd iteration (an assign launch and a
                 move launch), and km1 less one iteration is the seeding with pack, prep and the last pass
  clusters       fit_clusters(init="kmeans", seed=0) as a fleet calls it: the k-means at scikit-learn's defaults, the EM at its
                 defaults from the k-means centres, the install, the bins zeroed, the re-bin of the 60 steps
  given          fit_clusters(init=<the k-means centres>): the same chain without the k-means
The route it replaces, on the host, three times, alternating with `clusters`:
  download       the log to the host
  kmeans         sklearn.cluster.KMeans(4, init=<the points the device seeded>, n_init=1) on the records that count
  upload         the centres uploaded (the tensor the EM's init reads)
Every figure is the median of the three with the smallest and the largest.  The kernels' own times come from running
`rocprofv3 --kernel-trace --stats -- python scripts/quad_kmeans_time.py --brief` in a run of its own (--brief: the device forms only, few
replays).

    python scripts/quad_kmeans_time.py [--replays 5] [--windows 10] [--brief] [--out FILE]
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

import quad_clusters_spec as CS  # noqa: E402  (the pack, for the host route)
from quad_clusters_time import K, LEARN, N, T, three  # noqa: E402
from quad_rollout_time import B, OVER, emit, graph_capture, graph_measure  # noqa: E402
from ad_mpc_amd import _lib  # noqa: E402
from ad_mpc_amd.engine import _ptr  # noqa: E402
from ad_mpc_amd.quad_config import SimQuad  # noqa: E402
from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet  # noqa: E402
from ad_mpc_amd.quad_scenarios import circle_reference  # noqa: E402

FORMS = ("km1", "km11", "clusters", "given")
SEED = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--brief", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_kmeans_time.py measures on the GPU"
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
        fl.fit_clusters(init="kmeans", seed=SEED)                                               # allocates the k-means state before any capture
        km = fl.learned_kmeans()
        assert km.status == 0, km
        given = torch.as_tensor(km.centers).to(fl.device)
        M = fl.log_count * fl.B

        def raw(it):
            _lib.check(fl.lib.admpc_quad_kmeans_fit(fl._ens, SEED, 0, it, 0.0, M, _ptr(fl.log), _ptr(fl._packed), _ptr(fl._km_dist), _ptr(fl.km_labels),
                                                    _ptr(fl._km_work), _ptr(fl.km_centers), _ptr(fl.km_idx), _ptr(fl.km_stats), _ptr(fl.km_info), fl._stream()))

        calls = {"km1": lambda: raw(1), "km11": lambda: raw(11), "clusters": lambda: fl.fit_clusters(init="kmeans", seed=SEED),
                 "given": lambda: fl.fit_clusters(init=given)}
        graphs = {form: graph_capture(calls[form], a.replays) for form in FORMS}
        meds = {form: [] for form in FORMS}
        host = {"download": [], "kmeans": [], "upload": []}
        for _ in range(3):
            for form in FORMS:
                meds[form].append(graph_measure(graphs[form], 1, a.replays, a.windows)[0])
            if a.brief:
                continue
            from sklearn.cluster import KMeans
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = fl.log.cpu().numpy().reshape(-1, 14)
            t1 = time.perf_counter()
            packed = CS.pack(rec, feats)
            sk = KMeans(K, init=packed[km.idx, :d], n_init=1).fit(packed[packed[:, 3] == 1.0, :d])
            t2 = time.perf_counter()
            given.copy_(torch.as_tensor(sk.cluster_centers_))
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            for name, dt in zip(("download", "kmeans", "upload"), (t1 - t0, t2 - t1, t3 - t2)):
                host[name].append(dt * 1e6)
        r = {form: three(meds[form]) for form in FORMS}
        graphs["km11"].replay()
        torch.cuda.synchronize()
        ran = int(fl.km_info.cpu()[0])                                                          # fewer than 11 if the run stopped: the launches behind the stop return at once
        r["km11_iterations_run"] = ran
        r["one_lloyd_iteration"] = (r["km11"][0] - r["km1"][0]) / max(ran - 1, 1)
        r["seeding_with_pack_prep_and_last_pass"] = r["km1"][0] - r["one_lloyd_iteration"]
        r["kmeans_whole"] = r["clusters"][0] - r["given"][0]
        graphs["clusters"].replay()
        km, got = fl.learned_kmeans(), fl.learned_clusters()
        r.update(kmeans_iterations=km.n_iter, kmeans_converged=km.converged, kmeans_centres=km.centers.tolist(), seeded_records=km.idx.tolist(),
                 em_iterations=got.n_iter, em_converged=int(got.converged), status=got.status, centroids=fl.centroids.tolist())
        if not a.brief:
            r.update({name: three(v) for name, v in host.items()})
            r["host_route"] = r["download"][0] + r["kmeans"][0] + r["upload"][0]
            r["host_route_over_kmeans_whole"] = r["host_route"] / r["kmeans_whole"]
            r.update(sklearn_iterations=int(sk.n_iter_), max_centre_difference=float(np.abs(sk.cluster_centers_ - km.centers).max()))
        fl.close()
        res["d%d" % d] = r
    emit(res, a.out)


if __name__ == "__main__":
    main()
