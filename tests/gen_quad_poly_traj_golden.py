"""Writes tests/golden/quad_poly_traj_vectors.json: keyframes, polynomial coefficients and trajectories by the REFERENCE's own
`random_periodical_trajectory` (utils/keyframe_3d_gen.py), `random_trajectory`, `straight_trajectory` and
`minimum_snap_trajectory_generator` (utils/trajectories.py) and `fit_multi_segment_polynomial_trajectory` / `get_full_traj`
(utils/trajectory_generator.py), for the machines that have no reference tree.  Data only:

  keyframes  per seed the raw curve of random_periodical_trajectory, the adjusted keyframes of random_trajectory:330-338 and the
             coefficients [n_seg][8][4] of fit_multi_segment_polynomial_trajectory (descending powers; the fourth dimension is the yaw's)
  cases      per case its keyframes (a seed of the table above, or the points), speed, dt, vehicle, s, M, the per-column sums of |value| and
             full rows (13 states, 4 inputs) at rows 0, 1, 2, M - 3 .. M - 1, the row on either side of every segment junction and 16
             seeded rows
  rounding   (av_dist, speed, dt, round(av_dist / speed / dt)) as the reference's get_full_traj rounds, ties included

Arrays of doubles are stored as base-85 text of their little-endian bytes ("b85:..."; `unpack` reads them): a third of the size of
decimal digits, and exact.  The functions are taken out of the reference's files at run time (`ast`): its modules import ROS and open
plot windows, which the functions do not need.  It needs scikit-learn, as the reference does.

Runs only where the reference tree is present (see gen_quad_plant_golden.py):  python tests/gen_quad_poly_traj_golden.py"""
import base64
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import gen_quad_plant_golden as GG  # noqa: E402
import gen_quad_targets_golden as GT  # noqa: E402
import gen_quad_traj_golden as GJ  # noqa: E402
import quad_traj_spec as TS  # noqa: E402

SRC = os.path.join(GG.REF, "data_driven_mpc", "ros_gp_mpc", "src", "utils")
TRAJ, UTILS, GEN, KEYS = (os.path.join(SRC, n) for n in ("trajectories.py", "utils.py", "trajectory_generator.py", "keyframe_3d_gen.py"))
OUT = os.path.join(HERE, "golden", "quad_poly_traj_vectors.json")
SEED = 0x90171A
SEEDS = (1, 2, 303, 0, 7, 42, 1234, 9998)
SIZE_CAP = 200 * 1000


def pack(a):
    return "b85:" + base64.b85encode(np.ascontiguousarray(a, dtype="<f8").tobytes()).decode("ascii")


def unpack(s, shape=(-1,)):
    assert s.startswith("b85:")
    return np.frombuffer(base64.b85decode(s[4:]), dtype="<f8").reshape(shape).copy()


def given_keyframes(n_key, rng):
    """A seeded walk: steps of about 1.5 m, above the ground."""
    step = rng.standard_normal((n_key - 1, 3)) * np.array([1.0, 1.0, 0.25])
    step *= (1.5 / np.sqrt((step ** 2).sum(axis=1)))[:, None] * rng.uniform(0.6, 1.4, size=(n_key - 1, 1))
    keys = np.concatenate([np.zeros((1, 3)), np.cumsum(step, axis=0)])
    keys[:, 2] += 3.0 - keys[:, 2].min()
    return np.round(keys, 6)


def cases():
    out = []
    for seed in (1, 2, 303):
        for speed in (2.0, 3.5, 8.0):
            for dt in (0.02, 0.01):
                out.append(dict(kind="random", seed=seed, speed=speed, dt=dt, quad=TS.DEFAULT_QUAD))
    out.append(dict(kind="random", seed=2, speed=3.5, dt=0.02, quad=GJ.OTHER_QUAD))
    out.append(dict(kind="straight", speed=3.0, dt=0.02, quad=TS.DEFAULT_QUAD))
    rng = np.random.RandomState(SEED)
    for n_key in (4, 17, 32):
        out.append(dict(kind="given", keys=given_keyframes(n_key, rng).tolist(), speed=3.0, dt=0.02, quad=TS.DEFAULT_QUAD))
    return out


def rounding_grid():
    """(av_dist, speed, dt): quotients of exactly k + 0.5 (dt and speed powers of two, av_dist = (k + 0.5) speed dt), and seeded ones."""
    grid = []
    for dt in (0.25, 0.125, 0.03125):
        for speed in (1.0, 2.0, 0.5):
            for k in (0, 1, 2, 3, 4, 7, 10, 75, 76):
                grid.append(((k + 0.5) * speed * dt, speed, dt))
    rng = np.random.RandomState(SEED + 1)
    for _ in range(60):
        dt = float(rng.choice([0.02, 0.01, 0.05, 0.1, 1.0 / 30, 0.007]))
        grid.append((float(np.round(rng.uniform(0.05, 6.0), 4)), float(np.round(rng.uniform(0.5, 9.0), 3)), dt))
    return grid


def reference_present():
    return all(os.path.isfile(p) for p in (TRAJ, UTILS, GEN, KEYS))


def load_reference():
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import ExpSineSquared
    ns = {"np": np, "load_map_limits_from_file": lambda m: None, "print": lambda *a, **k: None, "draw_poly": None,
          "GaussianProcessRegressor": GaussianProcessRegressor, "ExpSineSquared": ExpSineSquared}
    for name in ("q_dot_q", "quaternion_inverse"):
        GT._function(UTILS, name, ns)
    for name in ("center_and_scale", "random_periodical_trajectory"):
        GT._function(KEYS, name, ns)
    for name in ("matrix_generation", "multiple_waypoints", "rhs_generation", "fit_multi_segment_polynomial_trajectory", "get_full_traj"):
        GT._function(GEN, name, ns)
    for name in ("minimum_snap_trajectory_generator", "random_trajectory", "straight_trajectory"):
        GT._function(TRAJ, name, ns)
    return ns


def reference_round(av_dist, speed, dt):
    """s as get_full_traj forms it from the av_dt of random_trajectory (trajectories.py:341-342, trajectory_generator.py:99)."""
    return int(round(np.float64(av_dist) / speed / dt))


def adjusted(ns, seed):
    """(raw, adjusted): the curve of random_periodical_trajectory and what random_trajectory:330-338 makes of it, by its expressions."""
    raw, att = ns["random_periodical_trajectory"](random_state=seed, map_limits=None, plot=False)
    assert not att.any()
    pos = raw.copy()
    pos[:, 0] -= pos[0, 0]
    pos[:, 1] -= pos[0, 1]
    min_z = np.min(pos[:, -1])
    if min_z < 0:
        pos[:, -1] = pos[:, -1] + 2 * min_z * np.sign(min_z)
    return raw, pos


def run_reference(ns, case, keys):
    quad = GJ._Quad(case["quad"])
    if case["kind"] == "random":
        traj, _, u = ns["random_trajectory"](quad, case["dt"], case["seed"], case["speed"])
    elif case["kind"] == "straight":
        traj, _, u = ns["straight_trajectory"](quad, case["dt"], case["speed"])
    else:                                               # random_trajectory behind its keyframes, by its own calls
        av_dt = np.mean(np.sqrt(np.sum(np.diff(keys, axis=0) ** 2, axis=1))) / case["speed"]
        poly = ns["fit_multi_segment_polynomial_trajectory"](keys.T, np.zeros(len(keys)))
        full, yaw, t_ref = ns["get_full_traj"](poly, av_dt, case["dt"])
        traj, _, u = ns["minimum_snap_trajectory_generator"](full, yaw, t_ref, quad, None, False)
    return traj, u


def stored_rows(n_seg, s, rng):
    M = n_seg * s + 1
    rows = {0, 1, 2, M - 3, M - 2, M - 1}
    for seg in range(1, n_seg):
        rows.update((seg * s - 1, seg * s))
    rows.update(int(r) for r in rng.randint(0, M, size=16))
    return sorted(rows)


def main():
    if not reference_present():
        sys.exit("no reference tree at %s" % GG.REF)
    ns = load_reference()
    rng = np.random.RandomState(SEED)
    out = {"seed": SEED, "keyframes": [], "cases": [], "rounding": []}
    table = {}
    for seed in SEEDS:
        raw, pos = adjusted(ns, seed)
        table[seed] = pos
        coef = ns["fit_multi_segment_polynomial_trajectory"](pos.T, np.zeros(len(pos)))
        assert coef.shape == (len(pos) - 1, 8, 4) and not coef[:, :, 3].any()
        out["keyframes"].append(dict(seed=seed, raw=pack(raw), adjusted=pack(pos), coefficients=pack(coef)))
    straight = np.zeros((3, 3))
    straight[:, 1] = np.linspace(-3, 3, 3)
    straight[:, 2] = 1
    for case in cases():
        keys = table[case["seed"]] if case["kind"] == "random" else straight if case["kind"] == "straight" else np.array(case["keys"])
        traj, u = run_reference(ns, case, keys)
        n_seg = len(keys) - 1
        s = reference_round(np.mean(np.sqrt(np.sum(np.diff(keys, axis=0) ** 2, axis=1))), case["speed"], case["dt"])
        M = traj.shape[0]
        assert M == n_seg * s + 1 and traj.shape == (M, 13) and u.shape == (M, 4) and np.isfinite(traj).all() and np.isfinite(u).all()
        full = np.concatenate([traj, u], axis=1)
        rows = stored_rows(n_seg, s, rng)
        out["cases"].append(dict(case, s=int(s), M=int(M), abs_sums=pack(np.abs(full).sum(axis=0)), rows=rows, values=pack(full[rows])))
    for av_dist, speed, dt in rounding_grid():
        out["rounding"].append([av_dist, speed, dt, reference_round(av_dist, speed, dt)])
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    size = os.path.getsize(OUT)
    print("wrote %s: %d seeds, %d cases, %d rounding triples, %d bytes" % (OUT, len(SEEDS), len(out["cases"]), len(out["rounding"]), size))
    assert size < SIZE_CAP


if __name__ == "__main__":
    main()
