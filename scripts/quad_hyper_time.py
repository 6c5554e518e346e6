"""Times the search of the quadrotor's GP hyperparameters on the device (include/admpc_quad_hyper.h; QuadEnsembleFleet.search_gp) at
B = 4096 with three 32-bin regressors per cluster (the body-frame velocity axes, every bin filled: 32 points each), K = 1, 4 and 8
clusters; grid 5 (125 candidates per regressor and round), 10 rounds, the reference's box.

Every device figure is a captured graph replayed several times between two HIP events, after a warm-up, repeated over some windows: the
median per replay.  The two forms of a comparison alternate in one session, three passes; the medians of the three are reported.
  chain_10 / chain_1    admpc_quad_ensemble_search alone from resume = 0 with 10 rounds and with 1: all K * 3 regressors in one chain of
                        launches; a round is (chain_10 - chain_1) / 9
  calls_10 / calls_1    the same work as K calls of admpc_quad_gp_search, one per cluster
  whole                 search_gp(): the search, the re-fit of all clusters in one launch, the K installs
  fit_install           the existing fit_gp at the given values with the install
  host                  what a user without the search does: bins to the host, scipy L-BFGS-B per regressor from the centre of the same box
                        on the same statistics (numpy.linalg.cholesky, the reference's formula), set_quad_gp, K new QuadBatchSolver --
                        host clock, ending in a synchronise, a few repeats

    python scripts/quad_hyper_time.py [--replays 10] [--windows 20] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ad_mpc_amd import _lib, config as _c  # noqa: E402
from ad_mpc_amd.engine import QuadBatchSolver, _ptr  # noqa: E402
from ad_mpc_amd.quad_config import SimQuad, set_quad_gp  # noqa: E402
from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet  # noqa: E402

B = 4096
LEARN = [dict(feat=7 + i, out=7 + i, lo=[-9.0], hi=[9.0], bins=[32], length_scale=2.0, sigma_f=1.0, noise=1e-4, count_noise=1e-2) for i in range(3)]


def filled_stats(K, seed=0):
    """Every bin of the K * 3 regressors: five samples at the bin's centre, a smooth target that differs per cluster and a little noise."""
    rng = np.random.default_rng(seed)
    stats = np.zeros((K, 3, 32, 5))
    z = -9.0 + (np.arange(32) + 0.5) * 18.0 / 32
    for c in range(K):
        for g in range(3):
            stats[c, g, :, 0], stats[c, g, :, 1] = 5.0, 5.0 * z
            stats[c, g, :, 4] = 5.0 * (np.sin(z / (1.0 + 0.25 * c)) * (1.0 + 0.1 * g) + 0.02 * rng.normal(size=32))
    return stats


def graph_time(fn, replays, windows):
    """median seconds per call of fn, captured once and replayed `replays` times per window."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(replays):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / replays)
    return float(np.median(out))


def host_nll(theta, Z, y, counts, count_noise):
    """gp.py:311-313 at exp(theta): length, sigma_f (not squared), noise."""
    v = np.exp(theta)
    d2 = ((Z[:, None] - Z[None, :]) / v[0]) ** 2
    Kmat = v[1] * np.exp(-0.5 * d2) + np.diag(v[2] + count_noise / counts)
    try:
        L = np.linalg.cholesky(Kmat)
    except np.linalg.LinAlgError:
        return 1e300
    w = np.linalg.solve(L, y)
    return float(np.log(np.diag(L)).sum() + 0.5 * w @ w + 0.5 * len(y) * np.log(2.0 * np.pi))


def host_fit(bins, boxes):
    """L-BFGS-B per regressor of one cluster from the centre of its box, and the GP at what it found: (set_quad_gp's dicts, [nll])."""
    from scipy.optimize import minimize
    gps, nlls = [], []
    for g, d in enumerate(LEARN):
        keep = bins[g, :, 0] >= 1
        counts = bins[g, keep, 0]
        Z, t = bins[g, keep, 1] / counts, bins[g, keep, 4] / counts
        ymean = t.mean()
        bounds = [(np.log(boxes[g].lo[s]), np.log(boxes[g].hi[s])) for s in (0, 3, 4)]
        x0 = np.array([0.5 * (a + b) for a, b in bounds])
        res = minimize(host_nll, x0, args=(Z, t - ymean, counts, d["count_noise"]), method="L-BFGS-B", bounds=bounds)
        v = np.exp(res.x)
        Kmat = v[1] * np.exp(-0.5 * ((Z[:, None] - Z[None, :]) / v[0]) ** 2) + np.diag(v[2] + d["count_noise"] / counts)
        gps.append(dict(feat=d["feat"], out=d["out"], Z=Z[:, None], alpha=np.linalg.solve(Kmat, t - ymean), length_scale=v[0], sigma_f=v[1], ymean=ymean))
        nlls.append(float(res.fun))
    return gps, nlls


def host_route(fl, boxes):
    """bins -> host -> host_fit per cluster -> set_quad_gp -> K new QuadBatchSolver; (seconds, [[nll per regressor] per cluster])."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bins = fl.bins.cpu().numpy()
    fits = [host_fit(bins[c], boxes) for c in range(fl.K)]
    engs = [QuadBatchSolver(set_quad_gp(fl._solvers[c].cfg.copy(), fits[c][0]), device=fl.device_index) for c in range(fl.K)]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for e in engs:
        e.close()
    return dt, [f[1] for f in fits]


def measure(K, a):
    cent = np.linspace(-3.0, 3.0, K).reshape(K, 1) if K > 1 else np.zeros((1, 1))
    fl = QuadEnsembleFleet(B, quad=SimQuad(drag=True), n_nodes=10, centroids=cent, feats=[7], learn=[LEARN] * K)
    fl.bins.copy_(torch.as_tensor(filled_stats(K), device=fl.device))
    boxes = _c.search_boxes(LEARN)
    lib, s = fl.lib, fl._stream

    def set_rounds(rounds):
        sp = (_c.AdmpcGpSearchParams * K)(*[_c.AdmpcGpSearchParams(grid=5, rounds=rounds, shrink=0.5, box=boxes) for _ in range(K)])
        _lib.check(lib.admpc_quad_ensemble_set_search(fl._ens, sp))                       # synchronous: outside every capture
        return sp[0]

    def chain():
        _lib.check(lib.admpc_quad_ensemble_search(fl._ens, 1, 0, _ptr(fl.bins), _ptr(fl.hyper), _ptr(fl._nll), _ptr(fl.search_info), s()))

    def calls(sp):
        for c in range(K):
            _lib.check(lib.admpc_quad_gp_search(fl.device_index, C.byref(fl._obs[c]), C.byref(sp), 1, 0, _ptr(fl.bins[c]), _ptr(fl.hyper[c]),
                                                _ptr(fl._nll[c]), _ptr(fl.search_info[c]), s()))

    runs = {k: [] for k in ("chain_10", "calls_10", "chain_1", "calls_1")}
    for _ in range(3):                                                                    # the forms alternate in one session
        for rounds in (10, 1):
            sp = set_rounds(rounds)
            runs["chain_%d" % rounds].append(graph_time(chain, a.replays, a.windows))
            runs["calls_%d" % rounds].append(graph_time(lambda: calls(sp), a.replays, a.windows))
    res = {k: float(np.median(v)) for k, v in runs.items()}
    res["chain_round"], res["calls_round"] = (res["chain_10"] - res["chain_1"]) / 9.0, (res["calls_10"] - res["calls_1"]) / 9.0
    fl.search_gp(grid=5, rounds=10)                                                       # its set_search, outside the capture
    res["whole"] = graph_time(lambda: fl.search_gp(grid=5, rounds=10), a.replays, a.windows)
    res["fit_install"] = graph_time(lambda: fl.fit_gp(), a.replays, a.windows)
    fl.search_gp(grid=5, rounds=10)
    res["device_nll"] = [[h["nll"] for h in cl] for cl in fl.learned_hyper()]
    res["device_info"] = [fl.fit_info.cpu().tolist(), fl.installed.cpu().tolist()]
    host = [host_route(fl, boxes) for _ in range(a.host_repeats + 1)][1:]                  # the first is the warm-up
    res["host_seconds"], res["host_nll"] = [h[0] for h in host], host[-1][1]
    res["whole_over_host"] = res["whole"] / float(np.median(res["host_seconds"]))
    fl.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--clusters", type=int, nargs="*", default=[1, 4, 8])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_hyper_time.py measures on the GPU"
    res = {"case": "B = 4096, three 32-bin regressors per cluster, 32 points each, grid 5: 125 candidates per regressor and round; 10 rounds; "
                   "the reference's box", "replays_per_window": a.replays, "windows": a.windows, "seconds": "medians per call, three alternating passes"}
    for K in a.clusters:
        res["K=%d" % K] = measure(K, a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
