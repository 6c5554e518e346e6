#!/usr/bin/env python3
"""Generate tests/golden/lane.json: the reference's own RefTrajectory on local lanes cut out of two routes.  TEST INFRASTRUCTURE ONLY.

Runs only where the reference tree is present (ADMPC_REFERENCE, default /root/reference).  As oracle/make_golden.py does, it imports the
reference's ref_traj.py with empty `rosbag` / `rospy` modules in place of the two it imports and never uses.  The lane handed to
set_traj is built here the way include/admpc_lane.h states it -- waypoints i0 .. i0 + L - 1 of the route with the last one repeated,
then the node's clamp (gp_ad_mpc_node.py:344-349) at the vehicle's speed -- and set_traj / get_waypoints are the reference's.  The
file is DATA: the routes, and per lane the reference's trajectory table and its get_waypoints dictionaries."""
import importlib.util
import json
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ADMPC_REFERENCE", "/root/reference")
ACC_MAX = 5.0


def reference_module():
    for name in ("rosbag", "rospy"):
        sys.modules.setdefault(name, types.ModuleType(name))
    path = os.path.join(REF, "data_driven_mpc/ros_gp_mpc/src/ad_mpc/ref_traj.py")
    spec = importlib.util.spec_from_file_location("reference_ref_traj", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def route(M, psi0):
    """Waypoints 0.5 m apart along a path of varying curvature; psi0 = 2.8 makes the yaw cross +-pi."""
    s = 0.5 * np.arange(M)
    psi = psi0 + 0.9 * np.sin(s / 11.0) + 0.01 * s
    x = np.concatenate(([0.0], np.cumsum(np.cos(psi[:-1]) * 0.5))) + 10.0
    y = np.concatenate(([0.0], np.cumsum(np.sin(psi[:-1]) * 0.5))) - 5.0
    return x, y, (psi + np.pi) % (2 * np.pi) - np.pi, 7.0 + 5.0 * np.sin(s / 9.0)


def main():
    mod = reference_module()
    rng = np.random.default_rng(11)
    routes = [route(120, 2.8), route(40, -0.4)]
    # (route, i0, L, H, dt, speed or None): lanes inside the route, ending at its end, one past it, far past it, all padding; a route
    # shorter than the lane; H > L; with and without the clamp; a vehicle at rest
    lanes = [(0, 0, 64, 20, 0.05, (6.0, 0.3)), (0, 30, 34, 20, 0.05, None), (0, 56, 64, 40, 0.025, (9.0, -0.2)), (0, 57, 64, 20, 0.05, (5.0, 0.0)),
             (0, 100, 65, 20, 0.05, (7.5, 0.1)), (0, 119, 34, 10, 0.1, (4.0, 0.0)), (0, 10, 256, 64, 0.05, (8.0, 0.0)),
             (1, 0, 63, 20, 0.05, (0.0, 0.0)), (1, 5, 34, 40, 0.2, None), (1, 12, 64, 3, 0.05, (6.5, 0.2))]
    cases = []
    for k, i0, L, H, dt, speed in lanes:
        x, y, psi, vel = routes[k]
        idx = np.minimum(i0 + np.arange(L), len(x) - 1)
        lx, ly, lpsi, lvel = list(x[idx]), list(y[idx]), list(psi[idx]), list(vel[idx])
        if speed is not None:
            bound = math.sqrt(speed[0] ** 2 + speed[1] ** 2)
            for i in range(L):
                if lvel[i] > bound:
                    lvel[i] = bound
                bound = bound + ACC_MAX * dt * 0.8
        rt = mod.RefTrajectory(traj_horizon=H, traj_dt=dt)
        rt.set_traj(lx, ly, lpsi, lvel)
        poses = []
        for _ in range(3):
            X0, Y0 = x[i0] + rng.normal(0, 0.1), y[i0] + rng.normal(0, 0.1)
            P0 = psi[i0] + rng.normal(0, 0.2) + rng.choice([0, 2 * np.pi, -2 * np.pi])
            w = rt.get_waypoints(X0, Y0, P0)
            poses.append(dict(X=X0, Y=Y0, psi=P0, out={key: (v.tolist() if hasattr(v, "tolist") else bool(v)) for key, v in w.items()}))
        cases.append(dict(route=k, i0=i0, L=L, H=H, dt=dt, speed=speed, acc_max=ACC_MAX, clamp_dt=dt, table=rt.trajectory.tolist(), poses=poses))
    out = dict(source="data_driven_mpc/ros_gp_mpc/src/ad_mpc/ref_traj.py (set_traj, get_waypoints) on lanes cut by scripts/make_golden_lane.py",
               routes=[dict(x=r[0].tolist(), y=r[1].tolist(), psi=r[2].tolist(), vel=r[3].tolist()) for r in routes], cases=cases)
    path = os.path.join(ROOT, "tests", "golden", "lane.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print("%s: %d lanes, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
