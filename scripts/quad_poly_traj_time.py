"""Times the generation of the quadrotor's random reference trajectories on the device (include/admpc_quad_poly_traj.h;
QuadFleet.generate_polynomial_trajectories) against the host route it replaces, at K = 4096 trajectories: the reference's
random_trajectory for seeds 0 ... 4095 at speed 3.5 m/s, dt the control period (0.02: N = 10, over-sampling 5).

The keyframes (ad_mpc_amd/quad_keyframes.py, numpy on the host) are made once and timed on their own: both routes need them.  Then
three rounds, the device and the host alternating in each.  On the device, `--repeats` calls per round: generate_polynomial_trajectories
by wall clock with a synchronise behind every call (the lengths, the weight matrix, the allocation and the uploads are in it) and the
span of the stream's events around the call; the kernel's own time comes from `rocprofv3 --kernel-trace --stats -- python
scripts/quad_poly_traj_time.py --brief` in a run of its own.  The written bytes are rows * 17 * 8, given per second of the event span
and, with --kernel-us, of the kernel's traced time.  On the host, over `--host-k` trajectories and scaled to K: tests/quad_poly_traj_spec.py's
vectorised numpy rule per trajectory (np.linalg.solve per axis, as the reference does), then set_trajectories.  Every figure is the
median of three with the smallest and the largest.

    python scripts/quad_poly_traj_time.py [--repeats 5] [--host-k 64] [--brief] [--kernel-us T] [--out FILE]
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

import quad_poly_traj_spec as PS  # noqa: E402
from quad_clusters_time import three  # noqa: E402
from quad_rollout_time import emit  # noqa: E402
from ad_mpc_amd.quad_fleet import QuadFleet  # noqa: E402
from ad_mpc_amd.quad_keyframes import random_keyframes  # noqa: E402

K, N, SPEED = 4096, 10, 3.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-k", type=int, default=64)
    ap.add_argument("--brief", action="store_true")
    ap.add_argument("--kernel-us", type=float, default=None, help="the kernel's time from a trace, for the bytes per second it writes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_poly_traj_time.py measures on the GPU"
    res = {"case": "K = %d random trajectories, seeds 0 ... %d, speed %g m/s, dt the control period" % (K, K - 1, SPEED),
           "repeats": a.repeats, "microseconds": "median, smallest, largest of three", "device": torch.cuda.get_device_name(0)}
    t0 = time.perf_counter()
    keys = np.stack([random_keyframes(seed) for seed in range(K)])
    res["host_keyframes_once_us"] = (time.perf_counter() - t0) * 1e6
    fl = QuadFleet(1, n_nodes=N)
    fl.generate_polynomial_trajectories(keys, SPEED)                         # warm-up: the code object, the allocator
    torch.cuda.synchronize()
    M = fl._M.copy()
    nbytes = int(M.sum()) * 17 * 8
    res.update(dt=fl.control_period, rows=int(M.sum()), rows_per_trajectory=[int(M.min()), float(M.mean()), int(M.max())], bytes_written=nbytes)
    quad = PS.TS.DEFAULT_QUAD
    wall, span, host_gen, host_up = [], [], [], []
    trajs = None
    for _ in range(3):
        w, s = [], []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fl.generate_polynomial_trajectories(keys, SPEED)
            e1.record()
            torch.cuda.synchronize()
            w.append((time.perf_counter() - t0) * 1e6); s.append(e0.elapsed_time(e1) * 1e3)
        wall.append(float(np.median(w))); span.append(float(np.median(s)))
        if not a.brief:
            t0 = time.perf_counter()
            trajs = [PS.generate(dict(keys=keys[k], speed=SPEED, dt=fl.control_period, quad=quad)) for k in range(a.host_k)]
            t1 = time.perf_counter()
            fl.set_trajectories(trajs)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host_gen.append((t1 - t0) * 1e6 * K / a.host_k); host_up.append((t2 - t1) * 1e6 * K / a.host_k)
    res.update(generate_wall=three(wall), generate_event_span=three(span),
               write_bandwidth_GBps_over_event_span=nbytes / (three(span)[0] * 1e-6) / 1e9)
    if a.kernel_us:
        res.update(kernel_us_from_trace=a.kernel_us, kernel_write_bandwidth_GBps=nbytes / (a.kernel_us * 1e-6) / 1e9,
                   loop_generator_kernel_write_bandwidth_GBps=952.0)
    if not a.brief:
        res.update(host_numpy_rule_scaled_to_K=three(host_gen), host_set_trajectories_scaled_to_K=three(host_up), host_k=a.host_k)
        res["host_route_over_device"] = (three(host_gen)[0] + three(host_up)[0]) / three(wall)[0]
        fl.generate_polynomial_trajectories(keys[:a.host_k], SPEED)
        worst = 0.0
        for k in range(0, a.host_k, 7):
            t, u = fl.trajectory(k)
            worst = max(worst, float(np.abs(t - trajs[k][0]).max()), float(np.abs(u - trajs[k][1]).max()))
        res["max_difference_device_against_numpy_rule"] = worst
    fl.close()
    emit(res, a.out)


if __name__ == "__main__":
    main()
