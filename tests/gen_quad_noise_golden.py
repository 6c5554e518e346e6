"""Writes tests/golden/quad_noise_vectors.json: noisy plant steps computed by the REFERENCE's own simulator (quad_mpc/quad_3d.py,
`Quadrotor3D.update` with `noisy` and `motor_noise`), for the machines that have no reference tree.  States, inputs, flags, seed, periods
and results only.

np.random's stream is not what include/admpc_quad_noise.h offers; its distributions are.  So `np.random.normal`, as the reference module
sees it, is replaced by a function that hands out the draws of tests/quad_noise_spec.py in the reference's call order -- four scalar
rotor draws (motor_noise), then f_d, then t_d (noisy), per update -- and everything else is the reference's own text.

Runs only where the reference tree is present (see gen_quad_plant_golden.py):  python tests/gen_quad_noise_golden.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import gen_quad_plant_golden as GG  # noqa: E402
import quad_noise_spec as NS  # noqa: E402

OUT = os.path.join(HERE, "golden", "quad_noise_vectors.json")
SEED = 0x5EEDF00D2024
# (noisy, motor_noise, drag, sub-steps): the four switch combinations x drag, at 1 and 40 sub-steps
CASES = [(n, mn, d, s) for n in (False, True) for mn in (False, True) for d in (False, True) for s in (1, 40)]


def periods(B):
    """The period of vehicle b: the high counter word is exercised from b = 2 on."""
    return np.arange(B, dtype=np.uint64) * np.uint64(2 ** 31)


class _Random:
    """np.random for the reference module: `normal` hands out the spec's draws, in the order the reference asks for them."""

    def __init__(self):
        self.queue = []

    def feed(self, z, noisy, motor_noise):
        """z [substeps, 10] -> the calls of `substeps` updates."""
        self.queue = []
        for row in z:
            if motor_noise:
                self.queue += [("scalar", row[i]) for i in range(4)]
            if noisy:
                self.queue += [("vector", row[4:7]), ("vector", row[7:10])]

    def normal(self, loc=0.0, scale=1.0, size=None):
        kind, z = self.queue.pop(0)
        if kind == "scalar":
            assert size is None
            return loc + scale * z
        assert tuple(size) == (3, 1) and loc == 0.0
        return (scale * z)[:, np.newaxis]


class _Numpy:
    """numpy as the reference module sees it: everything numpy's own but `random`."""

    def __init__(self, rnd):
        self.random = rnd

    def __getattr__(self, name):
        return getattr(np, name)


def load_reference():
    """(the reference's quad_3d module with its np.random replaced, the feeder)."""
    ref = GG.load_reference()
    rnd = _Random()
    ref.np = _Numpy(rnd)
    return ref, rnd


def run_reference(ref, rnd, noisy, motor_noise, drag, substeps, X, U, seed=SEED):
    out = np.zeros_like(X)
    p = periods(X.shape[0])
    for b in range(X.shape[0]):
        quad = ref.Quadrotor3D(noisy=noisy, drag=drag, payload=False, motor_noise=motor_noise)
        quad.set_state(X[b].tolist())
        rnd.feed(NS.draws(seed, b, p[b], np.arange(substeps)), noisy, motor_noise)
        for _ in range(substeps):
            quad.update(U[b].copy(), GG.DT)
        assert not rnd.queue
        out[b] = quad.get_state(quaternion=True, stacked=True)
    return out


def main():
    ref, rnd = load_reference()
    X, U = GG.inputs()
    doc = {"dt": GG.DT, "seed": SEED, "periods": [int(v) for v in periods(X.shape[0])], "x": X.tolist(), "u": U.tolist(), "cases": []}
    for noisy, motor_noise, drag, substeps in CASES:
        doc["cases"].append({"noisy": noisy, "motor_noise": motor_noise, "drag": drag, "substeps": substeps,
                             "result": run_reference(ref, rnd, noisy, motor_noise, drag, substeps, X, U).tolist()})
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
    print("wrote %s: %d cases of %d vehicles" % (OUT, len(CASES), X.shape[0]))


if __name__ == "__main__":
    main()
