"""Times the generation of the quadrotor's reference trajectories on the device (include/admpc_quad_traj.h;
QuadFleet.generate_trajectories) against the host route it replaces, at K = 4096 trajectories of 600 rows: loops and lemniscates
alternating, v_max spread over 2 ... 12 m/s, lin_acc = 0.25 v_max, dt = 0.02 (N = 10, over-sampling 5), radius 5, z 1.

On the device, three times, `--repeats` calls each: generate_trajectories by wall clock with a synchronise behind every call (the
lengths, the allocation and the uploads of the descriptors are in it) and the span of the stream's events around the call (the same call,
the kernel and the uploads; the kernel's own time comes from `rocprofv3 --kernel-trace --stats -- python scripts/quad_traj_time.py
--brief` in a run of its own).  The achieved write bandwidth is K * M * 17 * 8 bytes over the event span.
The host route, once over `--host-k` trajectories and scaled to K: tests/quad_traj_spec.py's vectorised numpy rule per trajectory, then
set_trajectories (the upload trajectory by trajectory).  Every figure is the median of three with the smallest and the largest.

--compare flies the comparative experiment's grid (comparative_experiment.py): loop and lemniscate x v_max {2, 4.5, 7, 9.5, 12},
radius 5, z 1, lin_acc 0.25 v, B = 10 vehicles, T = M steps, N = 10, the nominal model against the perfect and against the drag
simulator, and prints tracking_rmse per cell in the reference's table layout (a row per simulator, a column per speed).  tracking_rmse
counts the error at the start of each step; the reference's last row is the state after the last step.

    python scripts/quad_traj_time.py [--repeats 5] [--host-k 64] [--brief] [--compare] [--out FILE]
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

import quad_traj_spec as TS  # noqa: E402
from quad_clusters_time import three  # noqa: E402
from quad_rollout_time import emit  # noqa: E402
from ad_mpc_amd.quad_config import SimQuad  # noqa: E402
from ad_mpc_amd.quad_fleet import QuadFleet  # noqa: E402

K, N = 4096, 10
SPEEDS = [2.0, 4.5, 7.0, 9.5, 12.0]


def compare():
    out = {}
    for name, drag in (("perfect", False), ("drag", True)):
        fl = QuadFleet(10, quad=SimQuad(drag=drag), n_nodes=N)
        fl.generate_trajectories(["loop"] * 5 + ["lemniscate"] * 5, SPEEDS * 2)
        fl.reset(np.arange(10), 0)
        fl.rollout(int(fl._M[0]))
        torch.cuda.synchronize()
        rmse, counts = fl.tracking_rmse().cpu().numpy(), fl.counts.cpu().numpy()
        out[name] = {"loop": rmse[:5].tolist(), "lemniscate": rmse[5:].tolist(), "steps_with_status": counts[:, 1].tolist(),
                     "steps_with_replaced_input": counts[:, 2].tolist()}
        fl.close()
    print("tracking_rmse [m], nominal model; v_max  " + "  ".join("%7.1f" % v for v in SPEEDS))
    for kind in ("loop", "lemniscate"):
        for name in ("perfect", "drag"):
            print("%-10s %-8s            " % (kind, name) + "  ".join("%7.4f" % v for v in out[name][kind]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-k", type=int, default=64)
    ap.add_argument("--brief", action="store_true")
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_traj_time.py measures on the GPU"
    res = {"case": "K = %d trajectories of 600 rows, loops and lemniscates alternating, v_max 2 ... 12, lin_acc 0.25 v_max, dt 0.02" % K,
           "repeats": a.repeats, "microseconds": "median, smallest, largest of three", "device": torch.cuda.get_device_name(0)}
    if a.compare:
        res["compare"] = compare()
    kinds = [("loop", "lemniscate")[k % 2] for k in range(K)]
    v_max = np.linspace(2.0, 12.0, K).tolist()
    fl = QuadFleet(1, n_nodes=N)
    fl.generate_trajectories(kinds, v_max)                                  # warm-up: the code object, the allocator
    torch.cuda.synchronize()
    M = fl._M
    assert (M == 600).all(), (M.min(), M.max())
    nbytes = int(M.sum()) * 17 * 8
    wall, span = [], []
    for _ in range(3):
        w, s = [], []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fl.generate_trajectories(kinds, v_max)
            e1.record()
            torch.cuda.synchronize()
            w.append((time.perf_counter() - t0) * 1e6); s.append(e0.elapsed_time(e1) * 1e3)
        wall.append(float(np.median(w))); span.append(float(np.median(s)))
    res.update(generate_wall=three(wall), generate_event_span=three(span), bytes_written=nbytes,
               write_bandwidth_GBps_over_event_span=nbytes / (three(span)[0] * 1e-6) / 1e9)
    if not a.brief:
        quad = TS.DEFAULT_QUAD
        host_gen, host_up = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            trajs = [TS.generate(dict(kind=kinds[k], clockwise=True, radius=5.0, z=1.0, lin_acc=0.25 * v_max[k], v_max=v_max[k], dt=fl.control_period,
                                      quad=quad)) for k in range(a.host_k)]
            t1 = time.perf_counter()
            fl.set_trajectories(trajs)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host_gen.append((t1 - t0) * 1e6 * K / a.host_k); host_up.append((t2 - t1) * 1e6 * K / a.host_k)
        res.update(host_numpy_rule_scaled_to_K=three(host_gen), host_set_trajectories_scaled_to_K=three(host_up), host_k=a.host_k)
        res["host_route_over_device"] = (three(host_gen)[0] + three(host_up)[0]) / three(wall)[0]
        fl.generate_trajectories(kinds[:a.host_k], v_max[:a.host_k])
        worst = 0.0
        for k in range(0, a.host_k, 7):
            t, u = fl.trajectory(k)
            worst = max(worst, float(np.abs(t - trajs[k][0]).max()), float(np.abs(u - trajs[k][1]).max()))
        res["max_difference_device_against_numpy_rule"] = worst
    fl.close()
    emit(res, a.out)


if __name__ == "__main__":
    main()
