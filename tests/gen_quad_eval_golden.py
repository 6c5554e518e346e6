"""Writes tests/golden/quad_eval_vectors.json: what the REFERENCE's own GP prediction gives on the seeded fixtures of
tests/quad_eval_spec.py -- `GPEnsemble.select_gp` (model_fitting/gp.py:738-770) for the cluster of every query, and
`CustomGPRegression.predict` (gp.py:403-444) with `squared_exponential_kernel` (gp.py:81-115, its numpy branch, with
`_check_length_scale`) for the posterior mean and standard deviation -- for the machines that have no reference tree.  Seeds, parameters
and the reference's outputs only: the fixtures are rebuilt from their seeds.

The functions are taken out of the reference's file at run time by `ast`: the module imports casadi, which is not needed -- `cs` is
touched only in isinstance tests, so a stand-in namespace serves.  `self` is a plain object carrying what `fit` leaves (gp.py:361-363):
kernel, x_train, K_inv = inv(K), K_inv_y and y_mean, with K = kernel(x, x) + sigma_n^2 I.

Runs only where the reference tree is present:  python tests/gen_quad_eval_golden.py"""
import ast
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import gen_quad_plant_golden as GG  # noqa: E402
import quad_eval_spec as EV  # noqa: E402

GP_PY = os.path.join(GG.REF, "data_driven_mpc", "ros_gp_mpc", "src", "model_fitting", "gp.py")
OUT = os.path.join(HERE, "golden", "quad_eval_vectors.json")


def reference_present():
    return os.path.isfile(GP_PY)


def _method(tree, cls, name, namespace):
    """Method `name` of class `cls` as a plain function (decorators dropped), compiled on its own in `namespace`."""
    klass = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls]
    assert len(klass) == 1, cls
    node = [n for n in klass[0].body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(node) == 1, (cls, name)
    node[0].decorator_list = []
    exec(compile(ast.Module(body=node, type_ignores=[]), GP_PY, "exec"), namespace)
    return namespace[name]


def load_reference():
    """(kernel(self, x_1, x_2), _check_length_scale, predict(self, x, return_std), select_gp(self, dim, z=...))."""
    from numpy.linalg import inv  # noqa: F401
    from scipy.spatial.distance import cdist, pdist, squareform
    with open(GP_PY) as f:
        tree = ast.parse(f.read(), filename=GP_PY)
    cs = types.SimpleNamespace(MX=type("MX", (), {}), DM=type("DM", (), {}))
    ns = {"np": np, "cs": cs, "cdist": cdist, "pdist": pdist, "squareform": squareform}
    return (_method(tree, "CustomKernelFunctions", "squared_exponential_kernel", ns), _method(tree, "CustomKernelFunctions", "_check_length_scale", ns),
            _method(tree, "CustomGPRegression", "predict", ns), _method(tree, "GPEnsemble", "select_gp", ns))


def run_case(ref, seed, nf, n, K):
    """(idx [200], mu [200], std [200]) of the reference on the fixture of a case."""
    kernel_fn, check, predict, select_gp = ref
    feats, cent, clusters, z = EV.golden_fixture(seed, nf, n, K)
    ens = types.SimpleNamespace(gp_centroids={0: cent})
    idx = np.asarray(select_gp(ens, 0, z=z.T), dtype=np.int64).reshape(-1)
    mu, std = np.zeros(len(z)), np.zeros(len(z))
    for c, (x, y, ymean, length) in enumerate(clusters):
        k = types.SimpleNamespace(params={"l": length, "sigma_f": EV.SIGMA_F}, _check_length_scale=check)
        kernel = lambda a, b, k=k: kernel_fn(k, a, b)
        Kmat = kernel(x, x) + EV.SIGMA_N ** 2 * np.eye(len(x))
        K_inv = np.linalg.inv(Kmat)
        gp = types.SimpleNamespace(kernel=kernel, x_train=x, K_inv=K_inv, K_inv_y=K_inv.dot(y - ymean), y_mean=ymean)
        at = idx == c
        if at.any():
            with np.errstate(invalid="ignore"):
                mu[at], std[at] = predict(gp, z[at], return_std=True)
    return [int(i) for i in idx], [float(v) for v in mu], [float(v) for v in std]


def main():
    ref = load_reference()
    cases = []
    for seed, nf, n, K in EV.GOLDEN_CASES:
        idx, mu, std = run_case(ref, seed, nf, n, K)
        cases.append({"seed": seed, "n_feat": nf, "n": n, "K": K, "sigma_f": EV.SIGMA_F, "sigma_n": EV.SIGMA_N, "idx": idx, "mu": mu, "std": std})
    with open(OUT, "w") as f:
        json.dump({"cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
