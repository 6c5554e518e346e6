"""Writes tests/golden/quad_traj_vectors.json: trajectories by the REFERENCE's own `loop_trajectory`, `lemniscate_trajectory` and
`minimum_snap_trajectory_generator` (utils/trajectories.py:357-561, :128-282), for the machines that have no reference tree.  Per case
the parameters, M, the five phase lengths, the per-column sums of |value| and full rows (13 states, 4 inputs) at rows 0, 1, 2,
M - 3 .. M - 1, the row on either side of each phase boundary and 16 seeded rows; and the five `np.arange` lengths of the reference on a
grid of (dt, v_max, lin_acc) triples.  Data only.

The three functions are taken out of the reference's file at run time (`ast`): its module imports ROS, which they do not need.  Their
namespace is numpy, the reference's `q_dot_q` and `quaternion_inverse`, `load_map_limits_from_file = lambda m: None` and a silent print.

Runs only where the reference tree is present (see gen_quad_plant_golden.py):  python tests/gen_quad_traj_golden.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import gen_quad_plant_golden as GG  # noqa: E402
import gen_quad_targets_golden as GT  # noqa: E402
import quad_traj_spec as TS  # noqa: E402

SRC = os.path.join(GG.REF, "data_driven_mpc", "ros_gp_mpc", "src")
TRAJ = os.path.join(SRC, "utils", "trajectories.py")
UTILS = os.path.join(SRC, "utils", "utils.py")
OUT = os.path.join(HERE, "golden", "quad_traj_vectors.json")
SEED = 0x7A26A1

OTHER_QUAD = {          # a vehicle that is not the simulator's: other inertia, mass, arms, yaw coefficients and rotor force
    "mass": 1.7, "J": [.021, .035, .049], "max_thrust": 13.0,
    "x_f": [0.21, -0.17, -0.19, 0.23], "y_f": [-0.16, -0.22, 0.2, 0.18], "z_l_tau": [-0.011, 0.017, -0.015, 0.012],
}


def cases():
    out = []
    for kind in ("loop", "lemniscate"):
        for v in (2.0, 7.0, 12.0):
            for dt in (0.02, 0.01):
                out.append(dict(kind=kind, clockwise=True, radius=5.0, z=1.0, lin_acc=0.25 * v, v_max=v, dt=dt, quad=TS.DEFAULT_QUAD))
    out.append(dict(kind="loop", clockwise=False, radius=5.0, z=1.0, lin_acc=1.75, v_max=7.0, dt=0.02, quad=TS.DEFAULT_QUAD))
    out.append(dict(kind="lemniscate", clockwise=True, radius=3.5, z=1.6, lin_acc=1.9, v_max=6.0, dt=0.02, quad=TS.DEFAULT_QUAD))
    out.append(dict(kind="loop", clockwise=True, radius=2.25, z=0.8, lin_acc=2.3, v_max=5.0, dt=0.05, quad=TS.DEFAULT_QUAD))
    out.append(dict(kind="lemniscate", clockwise=True, radius=5.0, z=1.0, lin_acc=2.0, v_max=8.0, dt=0.02, quad=OTHER_QUAD))
    out.append(dict(kind="loop", clockwise=True, radius=5.0, z=1.0, lin_acc=2.0, v_max=8.0, dt=0.02, quad=OTHER_QUAD))
    return out


def length_grid():
    """(dt, v_max, lin_acc) triples: quotients that are integers in exact arithmetic, and seeded ones."""
    grid = []
    for dt in (0.02, 0.01, 0.05, 0.1, 0.25):
        for ratio in (2.5, 3.0, 4.0, 6.5):
            for lin_acc in (1.0, 0.7, 3.0):
                grid.append((dt, ratio * lin_acc, lin_acc))
    rng = np.random.RandomState(SEED)
    for _ in range(180):
        dt = float(rng.choice([0.02, 0.01, 0.05, 0.1, 0.25, 0.27, 0.03, 0.007, 1.0 / 30, 1.0 / 60]))
        lin_acc = float(np.round(rng.uniform(0.3, 4.0), 3))
        grid.append((dt, float(np.round(lin_acc * rng.uniform(2.05, 9.0), 3)), lin_acc))
    return grid


def reference_present():
    return os.path.isfile(TRAJ) and os.path.isfile(UTILS)


class _Quad:
    def __init__(self, d):
        self.mass, self.max_thrust = d["mass"], d["max_thrust"]
        self.J, self.x_f, self.y_f, self.z_l_tau = (np.array(d[k], dtype=np.float64) for k in ("J", "x_f", "y_f", "z_l_tau"))


def load_reference():
    ns = {"np": np, "load_map_limits_from_file": lambda m: None, "print": lambda *a, **k: None}
    for name in ("q_dot_q", "quaternion_inverse"):
        GT._function(UTILS, name, ns)
    for name in ("minimum_snap_trajectory_generator", "loop_trajectory", "lemniscate_trajectory"):
        GT._function(TRAJ, name, ns)
    return ns


def run_reference(ns, case):
    f = ns["loop_trajectory" if case["kind"] == "loop" else "lemniscate_trajectory"]
    traj, _, u = f(_Quad(case["quad"]), case["dt"], case["radius"], case["z"], case["lin_acc"], case["clockwise"], False, case["v_max"], None,
                   False)
    return traj, u


def reference_lengths(dt, v_max, lin_acc):
    """The lengths of the five np.arange calls of trajectories.py:396-410, by the same expressions."""
    ramp_up_t = 2
    t_total = 2 * v_max / lin_acc + 2 * ramp_up_t
    coasting_duration = (t_total - 4 * ramp_up_t) / 2
    return [len(np.arange(0, stop, dt)) for stop in (ramp_up_t, coasting_duration, 2 * ramp_up_t, coasting_duration, ramp_up_t)]


def stored_rows(n, rng):
    M = sum(n)
    rows = {0, 1, 2, M - 3, M - 2, M - 1}
    edge = 0
    for p in range(4):
        edge += n[p]
        rows.update((edge - 1, edge))
    rows.update(int(r) for r in rng.randint(0, M, size=16))
    return sorted(rows)


def main():
    if not reference_present():
        sys.exit("no reference tree at %s" % GG.REF)
    ns = load_reference()
    rng = np.random.RandomState(SEED)
    out = {"seed": SEED, "cases": [], "lengths": []}
    for case in cases():
        traj, u = run_reference(ns, case)
        n = reference_lengths(case["dt"], case["v_max"], case["lin_acc"])
        assert traj.shape == (sum(n), 13) and u.shape == (sum(n), 4)
        full = np.concatenate([traj, u], axis=1)
        rows = stored_rows(n, rng)
        out["cases"].append(dict(case, M=int(sum(n)), n=[int(v) for v in n], abs_sums=np.abs(full).sum(axis=0).tolist(), rows=rows,
                                 values=full[rows].tolist()))
    for dt, v_max, lin_acc in length_grid():
        out["lengths"].append([dt, v_max, lin_acc] + [int(v) for v in reference_lengths(dt, v_max, lin_acc)])
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote %s: %d cases, %d length triples, %d bytes" % (OUT, len(out["cases"]), len(out["lengths"]), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
