"""Writes tests/golden/quad_select_vectors.json: the indices the REFERENCE's own `distance_maximizing_points_1d`
(utils/utils.py:536-581) picks on the seeded fixtures of tests/quad_select_spec.py, for the machines that have no reference tree.
Seeds, generator parameters, n_points and index lists only: the fixtures are rebuilt from their seeds.

The function is taken out of the reference's file at run time (`ast`, as tests/gen_quad_prune_golden.py does): its module imports
casadi, pyquaternion, joblib and more, which it does not need; it sees numpy alone.  It gets the values as the column [N, 1] that
gp_fitting.py hands it.  Where a bin has no member the reference draws a random record (np.random.choice); the entry of such a bin --
found by the spec's own edges and comparisons -- is stored as -1, and the draw is never compared.

Runs only where the reference tree is present (see gen_quad_plant_golden.py):  python tests/gen_quad_select_golden.py"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import gen_quad_plant_golden as GG  # noqa: E402
import gen_quad_targets_golden as GT  # noqa: E402
import quad_select_spec as SS  # noqa: E402

UTILS = os.path.join(GG.REF, "data_driven_mpc", "ros_gp_mpc", "src", "utils", "utils.py")
OUT = os.path.join(HERE, "golden", "quad_select_vectors.json")


def reference_present():
    return os.path.isfile(UTILS)


def load_reference():
    return GT._function(UTILS, "distance_maximizing_points_1d", {"np": np})


def run_case(pick, kind, N, n, seed):
    """The reference's index per bin, -1 where the spec finds the bin empty."""
    z = SS.values(kind, N, seed)
    np.random.seed(seed)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        got = np.asarray(pick(z.reshape(-1, 1).copy(), n), dtype=np.int64).reshape(-1)
    empty = SS.select_1d(z, n) < 0
    return [-1 if e else int(i) for i, e in zip(got, empty)]


def main():
    pick = load_reference()
    cases = [{"kind": kind, "N": N, "n_points": n, "seed": seed, "index": run_case(pick, kind, N, n, seed)} for kind, N, n, seed in SS.GOLDEN_CASES]
    with open(OUT, "w") as f:
        json.dump({"cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
