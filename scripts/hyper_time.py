"""Times the search of the GP hyperparameters on the device (include/admpc_hyper.h; FleetController.search_gp) on the three-regressor case
scripts/fleet_step.py times the fit for: every bin filled, 8, 32 and 32 points; grid 5 (125, 625 and 625 candidates a round), 10 rounds,
the reference's box.

Every device figure is a captured graph replayed K times between two HIP events, after a warm-up, repeated R times: the median per
replay and the 10th and 90th percentile of the R windows.
  search_10 / search_1   admpc_gp_search alone from resume = 0 with 10 rounds and with 1; a round is (search_10 - search_1) / 9
  whole                  search_gp(): the search, the re-fit and the install
  fit / fit_install      the existing fit_gp at the given values without and with the install: one candidate per regressor
  host                   what a user without the search does: bins to the host, scipy L-BFGS-B from the centre of the same box on the same
                         statistics (numpy.linalg.cholesky, the reference's formula), set_gp, a new BatchSolver -- host clock, ending in a
                         synchronise, a few repeats

    python scripts/hyper_time.py [--replays 20] [--windows 50] [--out FILE]
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
from ad_mpc_amd.engine import BatchSolver, _ptr  # noqa: E402
from ad_mpc_amd.fleet import FleetController  # noqa: E402

T_HORIZON, OPT_DT = 1.0, 0.01
LEARN = [dict(feat=3, out=3, lo=[2.0], hi=[12.0], bins=[8], length_scale=2.0),
         dict(feat=[3, 6], out=4, lo=[2.0, -0.3], hi=[12.0, 0.3], bins=[8, 4], length_scale=[2.0, 0.2]),
         dict(feat=[3, 6], out=5, lo=[2.0, -0.3], hi=[12.0, 0.3], bins=[8, 4], length_scale=[2.0, 0.2])]


def filled_stats(seed=0):
    """Every bin of the three regressors: five samples at the bin's centre, a smooth target and a little noise (fleet_step.py's, with noise)."""
    rng = np.random.default_rng(seed)
    stats = np.zeros((4, 32, 5))
    for g, d in enumerate(LEARN):
        nb = list(d["bins"])
        for k in range(int(np.prod(nb))):
            idx = np.unravel_index(k, nb)
            z = [d["lo"][i] + (idx[i] + 0.5) * (d["hi"][i] - d["lo"][i]) / nb[i] for i in range(len(nb))]
            stats[g, k, 0], stats[g, k, 1:1 + len(nb)] = 5.0, 5.0 * np.array(z)
            stats[g, k, 4] = 5.0 * (np.sin(z[0]) * np.cos(3.0 * z[-1]) + 0.02 * rng.normal())
    return stats


def graph_time(fn, replays, windows):
    """(median, p10, p90) seconds per call of fn, captured once and replayed `replays` times per window."""
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
    return [float(np.median(out)), float(np.percentile(out, 10)), float(np.percentile(out, 90))]


def host_nll(theta, Z, y, counts, count_noise, nf):
    """gp.py:311-313 at exp(theta): lengths, sigma_f (not squared), noise."""
    v = np.exp(theta)
    d2 = (((Z[:, None, :] - Z[None, :, :]) / v[:nf]) ** 2).sum(axis=2)
    K = v[nf] * np.exp(-0.5 * d2) + np.diag(v[nf + 1] + count_noise / counts)
    try:
        L = np.linalg.cholesky(K)
    except np.linalg.LinAlgError:
        return 1e300
    w = np.linalg.solve(L, y)
    return float(np.log(np.diag(L)).sum() + 0.5 * w @ w + 0.5 * len(y) * np.log(2.0 * np.pi))


def host_fit(bins, boxes):
    """L-BFGS-B per regressor from the centre of its box, and the GP at what it found: (the dicts set_gp takes, [nll per regressor])."""
    from scipy.optimize import minimize
    gps, nlls = [], []
    for g, d in enumerate(LEARN):
        nf = len(np.atleast_1d(d["feat"]))
        keep = bins[g, :, 0] >= 1
        counts = bins[g, keep, 0]
        Z, t = bins[g, keep, 1:1 + nf] / counts[:, None], bins[g, keep, 4] / counts
        ymean = t.mean()
        slots = list(range(nf)) + [3, 4]
        bounds = [(np.log(boxes[g].lo[s]), np.log(boxes[g].hi[s])) for s in slots]
        x0 = np.array([0.5 * (a + b) for a, b in bounds])
        res = minimize(host_nll, x0, args=(Z, t - ymean, counts, d.get("count_noise", 0.0), nf), method="L-BFGS-B", bounds=bounds)
        v = np.exp(res.x)
        d2 = (((Z[:, None, :] - Z[None, :, :]) / v[:nf]) ** 2).sum(axis=2)
        K = v[nf] * np.exp(-0.5 * d2) + np.diag(v[nf + 1] + d.get("count_noise", 0.0) / counts)
        gps.append(dict(feat=d["feat"], out=d["out"], Z=Z, alpha=np.linalg.solve(K, t - ymean), length_scale=v[:nf], sigma_f=v[nf], ymean=ymean))
        nlls.append(float(res.fun))
    return gps, nlls


def host_route(fc, boxes):
    """bins -> host -> host_fit -> set_gp -> a new BatchSolver; (seconds, [nll per regressor])."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gps, nlls = host_fit(fc.bins.cpu().numpy(), boxes)
    eng = BatchSolver(_c.set_gp(fc._eng.cfg.copy(), gps), device=fc.device.index)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    eng.close()
    return dt, nlls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "hyper_time.py measures on the GPU"
    fc = FleetController(T_HORIZON, 20, OPT_DT, 64, learn=LEARN)
    fc.bins.copy_(torch.as_tensor(filled_stats(), device=fc.device))
    obs = fc._observe_params("hyper_time", observing=False)
    boxes = _c.search_boxes(LEARN)

    def search(rounds):
        sp = _c.AdmpcGpSearchParams(grid=5, rounds=rounds, shrink=0.5, box=boxes)
        _lib.check(fc.lib.admpc_gp_search(fc.device.index, C.byref(obs), C.byref(sp), 1, 0, _ptr(fc.bins), _ptr(fc.hyper), _ptr(fc._nll),
                                          _ptr(fc.search_info), fc._eng._stream()))

    res = {"case": "three regressors, 8 / 32 / 32 points, grid 5: 125 / 625 / 625 candidates a round; 10 rounds; the reference's box",
           "replays_per_window": a.replays, "windows": a.windows, "seconds": "median, 10th, 90th percentile per call"}
    res["search_10"] = graph_time(lambda: search(10), a.replays, a.windows)
    res["search_1"] = graph_time(lambda: search(1), a.replays, a.windows)
    res["whole"] = graph_time(lambda: fc.search_gp(grid=5, rounds=10), a.replays, a.windows)
    res["fit"] = graph_time(lambda: fc.fit_gp(install=False), a.replays, a.windows)
    res["fit_install"] = graph_time(lambda: fc.fit_gp(), a.replays, a.windows)
    res["round"] = (res["search_10"][0] - res["search_1"][0]) / 9.0
    res["candidates_per_round"] = 125 + 625 + 625
    res["round_over_candidates_times_fit_per_regressor"] = res["round"] / (res["candidates_per_round"] * res["fit"][0] / 3.0)
    fc.search_gp(grid=5, rounds=10)
    res["device"] = fc.learned_hyper()
    res["device_info"] = [fc.fit_info.cpu().tolist()[:3], fc.installed.cpu().tolist()[:3]]
    host = [host_route(fc, boxes) for _ in range(a.host_repeats + 1)][1:]                  # the first is the warm-up
    res["host"] = {"seconds": [h[0] for h in host], "nll": host[-1][1]}
    res["whole_over_host"] = res["whole"][0] / float(np.median(res["host"]["seconds"]))
    fc.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
