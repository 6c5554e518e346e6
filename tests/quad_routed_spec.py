"""The kernel paths of the quadrotor's routed solve (admpc_quad_solve_batch_routed) and the inputs their tests share (TEST INFRASTRUCTURE).

ROUTED_PATHS names every kernel quad_solve can launch with a route, under the names of test_problem_data_quad.PATHS; quad_kernel mirrors
the dispatch of quad_solve (its lines are in batch_regimes.LAUNCH_LINES) and test_quad_routed_paths_cpu.py holds the table against the
launch sites in the source.  `scenario` draws the inputs of one path: what tests/test_quad_routed_paths.py solves on the device is what
the CPU module checks, with the oracle alone, for the conditions that keep a routed comparison from passing vacuously."""
import numpy as np

import quad_ensemble_spec as ES
from ad_mpc_amd.quad_config import default_quad_config, set_quad_gp, QNX, QNU
from ad_mpc_amd.quad_scenarios import random_quad_scenarios

DENSE40, GENERIC, WIDE = ("admpc_quad_solve_kernel<%s>" % p for p in ("Dense40Path", "GenericPath", "WidePath"))
SEG = "admpc_quad_seg_kernel"

# path: (N, environment at the creation of the handles, the kernel quad_solve launches).  The distance between the fp64 and the 80-bit
# oracle on each path's own batch (test_quad_routed_paths_cpu.py measures it) stands beside the path in the table of
# test_quad_routed_paths.py: the figure a bound above 1e-8 would have to come from (`bound`).  No path needs one.
ROUTED_PATHS = {
    "dense40_N10": (10, {}, DENSE40),                             # the control: test_quad_gpu.py and test_batch_regimes.py hold it already
    "generic_N10": (10, {"ADMPC_QUAD_GENERIC": "1"}, GENERIC),
    "generic_N5": (5, {}, GENERIC),
    "generic_N16": (16, {}, GENERIC),
    "wide_N17": (17, {}, WIDE),
    "wide_N24": (24, {}, WIDE),
    "wide_N20": (20, {"ADMPC_QUAD_WIDE": "1"}, WIDE),
    "seg_N20": (20, {}, SEG),
}
# the order the GPU module runs the paths in: a barrier mismatch in a skip branch of a two-wave kernel hangs, and should do so at B = 96
TWO_WAVE_FIRST = ["seg_N20", "wide_N20", "wide_N17", "wide_N24", "generic_N16", "generic_N10", "generic_N5", "dense40_N10"]
assert sorted(TWO_WAVE_FIRST) == sorted(ROUTED_PATHS)

SWITCHES = {"ADMPC_QUAD_GENERIC": "generic", "ADMPC_QUAD_WIDE": "wide20"}      # environment variable: the handle's field it sets


def quad_kernel(N, env):
    """The kernel quad_solve launches for a handle of horizon N created under `env`."""
    generic, wide20 = (env.get(k, "")[:1] == "1" for k in ("ADMPC_QUAD_GENERIC", "ADMPC_QUAD_WIDE"))
    if N == 20 and not wide20:
        return SEG
    if N * QNU > 64:
        return WIDE
    if N * QNU == 40 and not generic:
        return DENSE40
    return GENERIC


FEATS = [7, 13]                                                   # body-frame v_x and the first rotor's input
CENT = np.array([[-1.1, 0.3], [0.0, 0.5], [1.1, 0.7]])
B1 = 96
OFF = {5: 7, 6: -1}                                               # instance: a route that names no cluster
TOL = 1e-8                                                        # test_problem_data_quad._assert_quad_parity: |du|, |dx|; cost 1e-9 relative


def horizon(N):
    return min(0.1 * N, 2.0)


def path_config(path):
    N = ROUTED_PATHS[path][0]
    return default_quad_config(N=N, t_horizon=horizon(N))


def clusters(K=3):
    from test_quad_oracle import quad_gps
    return [quad_gps(seed=c + 1) for c in range(K)]


def cluster_config(cfg, gps):
    cc = cfg.copy(); set_quad_gp(cc, gps)
    return cc


def features(s, seed):
    """The states and inputs the route is selected on: x0 moved by a unit normal draw (unit quaternion), inputs uniform in [0, 1]."""
    B = len(s["x0"])
    rng = np.random.default_rng(seed)
    xs = s["x0"] + rng.standard_normal((B, QNX)); xs[:, 3:7] /= np.linalg.norm(xs[:, 3:7], axis=1, keepdims=True)
    return xs, rng.uniform(0, 1, (B, QNU))


def spec_route(xs, us, cent=CENT, feats=FEATS):
    """(route, smallest gap between the two nearest centroids) by the numpy statement of admpc_quad_select_cluster_batch."""
    z = [ES.z_of_row(np.r_[x, u])[feats] for x, u in zip(xs, us)]
    return np.array([ES.nearest(v, cent) for v in z], dtype=np.int32), min(ES.margin(v, cent) for v in z)


_SCEN = {}


def scenario(path, B=B1):
    """(cfg, s, xs, us, route) of one path; the inputs depend on the horizon alone, so that the two kernels of N = 10 and of N = 20 solve
    the same problems.  route: the spec's, before the out-of-range entries of OFF go in."""
    N = ROUTED_PATHS[path][0]
    if (N, B) not in _SCEN:
        cfg = path_config(path)
        s = random_quad_scenarios(B, cfg, seed=610 + N)
        xs, us = features(s, seed=60 + N)
        route, gap = spec_route(xs, us)
        assert gap >= 1e-6, "a feature within 1e-6 of a cell boundary: draw another seed"
        _SCEN[N, B] = (s, xs, us, route)
    return (path_config(path),) + _SCEN[N, B]


def gp_state(s):
    """A first-node GP state away from x0 (test_quad_oracle.py:test_first_node_gp_state_parameter's)."""
    g = s["x0"].copy(); g[:, 7:10] += 1.5
    return g


def with_off(route):
    r = route.copy()
    for b, v in OFF.items():
        r[b] = v
    return r


def quad_args(s):
    return tuple(s[k] for k in ("x0", "yref", "yref_e", "xbar", "ubar"))


def oracle_routed(oracle, cfg, gps, route, s, gp_state=None, idx=None):
    """The oracle's solve of every in-range instance (of idx, when given) under the GPs of its own cluster: (index array, results)."""
    K = len(gps)
    idx = np.arange(len(route)) if idx is None else np.asarray(idx)
    idx = idx[(route[idx] >= 0) & (route[idx] < K)]
    out = None
    for c in range(K):
        m = idx[route[idx] == c]
        if not len(m):
            continue
        o = oracle.solve_batch(cluster_config(cfg, gps[c]), *(a[m] for a in quad_args(s)), gp_state=None if gp_state is None else gp_state[m], nthreads=16)
        if out is None:
            out = [np.zeros((len(route),) + a.shape[1:], dtype=a.dtype) for a in o]
        for a, b in zip(out, o):
            a[m] = b
    return idx, tuple(a[idx] for a in out)


def bound(gap):
    """The parity bound of a path from its measured distance between the fp64 and the 80-bit oracle: two fp64 evaluation orders are each
    about that far from the 80-bit result (2 x covers their mutual distance), and the drawn set need not be the worst case (2 x more)."""
    return max(TOL, 4.0 * gap)


def assert_parity(g, o, cfg, what, tol=TOL):
    """test_problem_data_quad._assert_quad_parity on routed results: statuses and iteration counts identical, |du| and |dx| within tol, the
    cost within 1e-9 relative, the inputs inside the box."""
    np.testing.assert_array_equal(g[3], o[3], err_msg=what); assert (o[3] == 0).all(), what
    np.testing.assert_array_equal(g[4], o[4], err_msg=what)
    du, dx = np.abs(g[1] - o[1]).max(), np.abs(g[0] - o[0]).max()
    print("ROUTED %-28s %5d instances: max|du| %.1e max|dx| %.1e  bound %.0e" % (what, len(g[0]), du, dx, tol))
    assert du <= tol and dx <= tol, (what, du, dx)
    np.testing.assert_allclose(g[2], o[2], rtol=1e-9, err_msg=what)
    lb, ub = np.array(cfg.lbu[:]), np.array(cfg.ubu[:])
    assert (g[1] >= lb - 1e-9).all() and (g[1] <= ub + 1e-9).all(), what
    return du, dx
