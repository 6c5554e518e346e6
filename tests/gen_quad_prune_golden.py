"""Writes tests/golden/quad_prune_vectors.json: the indices the REFERENCE's own `prune_dataset` (utils/utils.py:458-533) keeps of the
seeded fixtures of tests/quad_prune_spec.py, and the drag coefficients its `linear_rdrv_fitting` (model_fitting/rdrv_fitting.py:27-33)
fits to what is kept, for the machines that have no reference tree.  Seeds, parameters, kept-index lists and drag coefficients only: the
fixtures are rebuilt from their seeds.

The two functions are taken out of the reference's files at run time (`ast`, as tests/gen_quad_targets_golden.py does): their modules
import casadi, pyquaternion, joblib and more, which they do not need.  prune_dataset sees numpy and, for the `plot` branch that is never
taken, nothing; linear_rdrv_fitting sees numpy and sklearn's LinearRegression, the class the reference calls.  The reference gets the
CLEAN fixtures (every record takes part): x the body velocities, y the three errors, as GPDataset.prune hands them over
(gp_common.py:101-112).

Runs only where the reference tree is present (see gen_quad_plant_golden.py):  python tests/gen_quad_prune_golden.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import gen_quad_plant_golden as GG  # noqa: E402
import gen_quad_targets_golden as GT  # noqa: E402
import quad_prune_spec as PS  # noqa: E402

SRC = os.path.join(GG.REF, "data_driven_mpc", "ros_gp_mpc", "src")
UTILS = os.path.join(SRC, "utils", "utils.py")
RDRV = os.path.join(SRC, "model_fitting", "rdrv_fitting.py")
OUT = os.path.join(HERE, "golden", "quad_prune_vectors.json")


def reference_present():
    return os.path.isfile(UTILS) and os.path.isfile(RDRV)


def load_reference():
    """(prune_dataset, linear_rdrv_fitting)."""
    from sklearn.linear_model import LinearRegression
    return GT._function(UTILS, "prune_dataset", {"np": np, "plt": None}), \
        GT._function(RDRV, "linear_rdrv_fitting", {"np": np, "LinearRegression": LinearRegression})


def run_case(prune_dataset, fit, kind, M, n_bins, thresh, x_cap, seed):
    """The kept indices and the diagonal of the drag matrix (None where nothing is kept)."""
    v, y = PS.clean(kind, M, seed)
    with np.errstate(all="ignore"):
        kept = np.asarray(prune_dataset(v.copy(), y.copy(), x_cap, n_bins, thresh, False), dtype=np.int64).reshape(-1)
    drag = None
    if kept.size:
        drag = [float(d) for d in np.diag(fit(v[kept], y[kept], np.array([0, 1, 2])))]
    return [int(i) for i in kept], drag


def main():
    prune_dataset, fit = load_reference()
    cases = []
    for kind, M, n_bins, thresh, x_cap, seed in PS.GOLDEN_CASES:
        kept, drag = run_case(prune_dataset, fit, kind, M, n_bins, thresh, x_cap, seed)
        cases.append({"kind": kind, "M": M, "n_bins": n_bins, "thresh": thresh, "x_cap": x_cap, "seed": seed, "kept": kept, "drag": drag})
    with open(OUT, "w") as f:
        json.dump({"cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
