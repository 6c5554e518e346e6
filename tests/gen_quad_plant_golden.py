"""Writes tests/golden/quad_plant_vectors.json: plant steps computed by the REFERENCE's own simulator (quad_mpc/quad_3d.py,
`Quadrotor3D.update`), for the machines that have no reference tree.  States, inputs, flags and results only.

Runs only where the reference tree is present (ADMPC_REFERENCE, default /root/reference):  python tests/gen_quad_plant_golden.py

The reference module imports `utils.utils`, which needs casadi and pyquaternion; `load_reference` puts a stand-in module in its place that
supplies the five helpers quad_3d.py imports (the restatements of tests/quad_plant_spec.py; quaternion_to_euler is not reached by
`update`).  tests/test_quad_fleet_cpu.py runs the same cases live and holds the numpy spec against them."""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import quad_plant_spec as QS  # noqa: E402

REF = os.environ.get("ADMPC_REFERENCE", "/root/reference")
QUAD_3D = os.path.join(REF, "data_driven_mpc", "ros_gp_mpc", "src", "quad_mpc", "quad_3d.py")
OUT = os.path.join(HERE, "golden", "quad_plant_vectors.json")
DT = 5e-4
# (drag, payload, sub-steps)
CASES = [(False, False, 1), (False, False, 40), (True, False, 1), (True, False, 40), (True, True, 1), (True, True, 40)]


def reference_present():
    return os.path.isfile(QUAD_3D)


def load_reference():
    """The reference's quad_3d module, with the stand-in for utils.utils."""
    def quaternion_to_euler(q):
        raise NotImplementedError("not reached by Quadrotor3D.update")

    def unit_quat(q):
        return 1 / np.sqrt(np.sum(q ** 2)) * q

    def v_dot_q(v, q):
        return QS.rot(q).dot(v)

    saved = {k: sys.modules.get(k) for k in ("utils", "utils.utils")}
    pkg, mod = types.ModuleType("utils"), types.ModuleType("utils.utils")
    for f in (quaternion_to_euler, unit_quat, v_dot_q):
        setattr(mod, f.__name__, f)
    mod.skew_symmetric, mod.quaternion_inverse = QS.skew4, QS.conj
    pkg.utils = mod
    sys.modules["utils"], sys.modules["utils.utils"] = pkg, mod
    try:
        spec = importlib.util.spec_from_file_location("_reference_quad_3d", QUAD_3D)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return m


def inputs():
    """(X [12,13], U [12,4]): finite activations only -- under a NaN the reference's max(min(...)) depends on the argument order -- on both
    sides of [0, 1]; vehicle 5 level with v_y = 0 (one body-frame velocity component exactly 0)."""
    X, U = QS.fleet67(nan_input=False)
    return X[:12].copy(), U[:12].copy()


def run_reference(ref, drag, payload, substeps, X, U):
    out = np.zeros_like(X)
    for b in range(X.shape[0]):
        quad = ref.Quadrotor3D(noisy=False, drag=drag, payload=payload, motor_noise=False)
        quad.set_state(X[b].tolist())
        for _ in range(substeps):
            quad.update(U[b].copy(), DT)
        out[b] = quad.get_state(quaternion=True, stacked=True)
    return out


def main():
    ref = load_reference()
    X, U = inputs()
    doc = {"dt": DT, "x": X.tolist(), "u": U.tolist(), "cases": []}
    for drag, payload, substeps in CASES:
        doc["cases"].append({"drag": drag, "payload": payload, "substeps": substeps, "result": run_reference(ref, drag, payload, substeps, X, U).tolist()})
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
    print("wrote %s: %d cases of %d vehicles" % (OUT, len(CASES), X.shape[0]))


if __name__ == "__main__":
    main()
