"""Writes tests/golden/quad_targets_vectors.json: targets sampled by the REFERENCE's own `sample_random_target`
(experiments/point_tracking_and_record.py:82-107) and distances by its `euclidean_dist` (utils/utils.py:262-281), for the machines that
have no reference tree.  Seed, positions, target numbers, uniforms, targets, point pairs and distances only.

np.random's stream is not what include/admpc_quad_targets.h offers; its distributions are.  So `np.random.uniform`, as the reference's
functions see it, is replaced by a feeder that hands out the uniforms of tests/quad_targets_spec.py in the reference's call order --
theta, psi, the radius ("aggressive"), or the three coordinates at once (uniform) -- mapped as numpy maps a uniform number onto
[low, high): low + (high - low) * u.  The two functions are taken out of the reference's files at run time (`ast`): their modules import
casadi, pyquaternion and more, which they do not need.

Runs only where the reference tree is present (see gen_quad_plant_golden.py):  python tests/gen_quad_targets_golden.py"""
import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import gen_quad_plant_golden as GG  # noqa: E402
import quad_targets_spec as TS  # noqa: E402

SRC = os.path.join(GG.REF, "data_driven_mpc", "ros_gp_mpc", "src")
SCRIPT = os.path.join(SRC, "experiments", "point_tracking_and_record.py")
UTILS = os.path.join(SRC, "utils", "utils.py")
OUT = os.path.join(HERE, "golden", "quad_targets_vectors.json")
SEED = 0x7A26E75F00D5
B, R = 24, 3.0


def reference_present():
    return os.path.isfile(SCRIPT) and os.path.isfile(UTILS)


class _Random:
    """np.random for the reference's functions: `uniform` hands out the queued uniforms, mapped onto [low, high) as numpy does."""

    def __init__(self):
        self.queue = []

    def uniform(self, low=0.0, high=1.0, size=None):
        n = int(np.prod(size)) if size is not None else 1
        u = np.array([self.queue.pop(0) for _ in range(n)], dtype=np.float64)
        out = low + (high - low) * u
        return out.reshape(size) if size is not None else out[0]


class _Numpy:
    """numpy as the reference's functions see it: everything numpy's own but `random`."""

    def __init__(self, rnd):
        self.random = rnd

    def __getattr__(self, name):
        return getattr(np, name)


def _function(path, name, namespace):
    """The function `name` of the file at `path`, compiled on its own in `namespace`."""
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    node = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(node) == 1, (path, name)
    exec(compile(ast.Module(body=node, type_ignores=[]), path, "exec"), namespace)
    return namespace[name]


def load_reference():
    """(sample_random_target, euclidean_dist, the feeder)."""
    rnd = _Random()
    ns = {"np": _Numpy(rnd)}
    return _function(SCRIPT, "sample_random_target", ns), _function(UTILS, "euclidean_dist", {"np": np}), rnd


def inputs():
    """(positions [B,3], target numbers [B] uint64): the high counter word is exercised from b = 2 on."""
    rng = np.random.default_rng(77)
    return rng.uniform(-4.0, 4.0, (B, 3)), np.arange(B, dtype=np.uint64) * np.uint64(2 ** 31)


def pairs():
    """Point pairs of the reach test: far, near, on both sides of 0.05, and equal."""
    rng = np.random.default_rng(78)
    p = rng.uniform(-3.0, 3.0, (16, 3))
    step = rng.standard_normal((16, 3))
    step /= np.linalg.norm(step, axis=1, keepdims=True)
    t = p + step * np.array([3.0, 1.0, 0.3, 0.1, 0.0501, 0.0499, 0.05 + 1e-9, 0.05 - 1e-9, 0.04, 0.01, 1e-3, 1e-6, 0.0, 2.0, 0.06, 0.05])[:, None]
    return t, p


def run_reference(sample, rnd, aggressive, P, U):
    out = np.zeros_like(P)
    for b in range(P.shape[0]):
        rnd.queue = [U[b, 0], U[b, 1], U[b, 2]]
        out[b] = np.asarray(sample(P[b].copy(), R, aggressive=aggressive), dtype=np.float64).reshape(3)
        assert not rnd.queue
    return out


def main():
    sample, euclid, rnd = load_reference()
    P, no = inputs()
    U = TS.uniforms(TS.words(SEED, np.arange(B), no))
    t, p = pairs()
    doc = {"seed": SEED, "world_radius": R, "positions": P.tolist(), "target_no": [int(v) for v in no], "uniforms": U.tolist(),
           "aggressive": run_reference(sample, rnd, True, P, U).tolist(), "uniform": run_reference(sample, rnd, False, P, U).tolist(),
           "pair_t": t.tolist(), "pair_p": p.tolist(), "dist": [float(euclid(t[i], p[i])) for i in range(len(t))],
           "within_0.05": [bool(euclid(t[i], p[i], thresh=0.05)) for i in range(len(t))]}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
    print("wrote %s: %d targets per mode, %d point pairs" % (OUT, B, len(t)))


if __name__ == "__main__":
    main()
