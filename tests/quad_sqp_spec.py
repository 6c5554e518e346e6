"""solver_type "SQP" inside the one-wave solve kernel (include/admpc_quad_sqp.h): the kernel paths, the modes and the inputs their tests
share (TEST INFRASTRUCTURE).

What tests/test_quad_sqp_gpu.py solves on the device is what tests/test_quad_sqp_cpu.py checks, with the oracle alone, for the status
mixes that keep a comparison from passing vacuously, and measures for its bounds.  The inputs are those of
test_quad_gpu.py::test_quad_sqp_mode_on_the_device and quad_ipm_exits_spec.sqp_case: random_quad_scenarios(B, cfg, seed=7, pos_err=0.8,
tilt=0.2, aggressive=0.0), B = 96 at N = 10 and 32 elsewhere, t_horizon = quad_routed_spec.horizon(N)."""
import numpy as np

import quad_routed_spec as Q
from ad_mpc_amd.quad_config import default_quad_config, set_quad_gp
from ad_mpc_amd.quad_scenarios import random_quad_scenarios

# path: (N, environment at the creation of the handle, the instantiation quad_solve_sqp launches)
PATHS = {
    "generic_N2": (2, {}, "GenericPath"),                         # the k >= 1 branch of the adjoint recursion runs once
    "generic_N5": (5, {}, "GenericPath"),
    "dense40_N10": (10, {}, "Dense40Path"),
    "generic_N10": (10, {"ADMPC_QUAD_GENERIC": "1"}, "GenericPath"),
    "generic_N16": (16, {}, "GenericPath"),                       # n = 64: no idle lane
}
BASE_MODES = [(100, 1e-6), (4, 1e-6), (3, 0.0)]                   # (qp_max, tol)
MID_MODE = (30, 1e-6)


def modes(path):
    return BASE_MODES + ([MID_MODE] if PATHS[path][0] != 2 else [])


CASES = [(p,) + m for p in PATHS for m in modes(p)]
HORIZONS = sorted({v[0] for v in PATHS.values()})

# instances with (status 0, status 2) at a limit of L QPs and tol = 1e-6, by the oracle (the fp64 and the 80-bit oracle agree):
# test_quad_sqp_cpu.py holds the oracle against this table
STATUS_MIX = {
    (2, 3): (8, 24), (2, 4): (16, 16), (2, 6): (32, 0),
    (5, 4): (0, 32), (5, 10): (1, 31), (5, 30): (12, 20), (5, 100): (24, 8),
    (10, 4): (0, 96), (10, 10): (4, 92), (10, 30): (21, 75), (10, 100): (51, 45),
    (16, 4): (0, 32), (16, 10): (0, 32), (16, 30): (7, 25), (16, 100): (15, 17),
}
QPS_SWEEP_N2 = range(2, 8)                                        # qps at N = 2: (the smallest L with status 0) - 1
QPS_LIMITS = (10, 30, 100)                                        # qps at N = 5, 10, 16: qps <= L - 1 exactly where the oracle's status at limit L is 0

# The distance between the fp64 and the 80-bit oracle per (N, qp_max, tol): (max |du|, max |dx|, max relative cost distance), measured by
# test_quad_sqp_cpu.py, which holds its own figures at or below twice these.  `bound` turns them into the tolerances of the device tests.
SQP_GAPS = {
    (2, 100, 1e-6): (6.7e-16, 8.9e-16, 4.5e-16), (2, 4, 1e-6): (6.7e-16, 8.9e-16, 4.5e-16), (2, 3, 0.0): (3.4e-16, 8.9e-16, 4.5e-16),
    (5, 100, 1e-6): (1.5e-14, 4.3e-14, 5.6e-16), (5, 4, 1e-6): (2.1e-14, 7.2e-14, 1.1e-15), (5, 3, 0.0): (5.0e-14, 7.2e-14, 8.8e-16),
    (5, 30, 1e-6): (2.5e-14, 7.7e-14, 1.4e-15),
    (10, 100, 1e-6): (8.7e-13, 2.1e-12, 4.2e-14), (10, 4, 1e-6): (9.3e-13, 1.9e-12, 5.4e-14), (10, 3, 0.0): (1.5e-12, 2.5e-12, 3.5e-14),
    (10, 30, 1e-6): (1.4e-12, 5.4e-12, 4.8e-14),
    (16, 100, 1e-6): (3.9e-11, 3.8e-10, 4.4e-12), (16, 4, 1e-6): (5.1e-11, 2.1e-10, 4.2e-12), (16, 3, 0.0): (1.0e-10, 1.4e-10, 4.6e-12),
    (16, 30, 1e-6): (3.7e-11, 3.9e-10, 5.7e-12),
}
# the same for the batch of N = 10 with one GP on the handle and a first-node GP state away from x0, mode MID_MODE (statuses 22 x 0, 74 x 2)
GP_GAP = (8.0e-13, 1.0e-11, 1.4e-13)


def batch(N):
    return 96 if N == 10 else 32


def config(N, mode=None):
    """The configuration of horizon N; with a mode, the fields the oracle and the host loop read it from."""
    cfg = default_quad_config(N=N, t_horizon=Q.horizon(N))
    if mode is not None:
        cfg.sqp_iters, cfg.sqp_tol = mode
    return cfg


_SCEN = {}


def scenario(N):
    """The inputs of horizon N, shared between the calls: they must stay unchanged."""
    if N not in _SCEN:
        _SCEN[N] = random_quad_scenarios(batch(N), config(N), seed=7, pos_err=0.8, tilt=0.2, aggressive=0.0)
    return _SCEN[N]


def gp_config(mode=None):
    """N = 10 with one GP on the handle (the first of test_quad_oracle.quad_gps)."""
    from test_quad_oracle import quad_gps
    cfg = config(10, mode)
    set_quad_gp(cfg, quad_gps(seed=1)[:1])
    return cfg


def gaps(o, o8):
    """(max |du|, max |dx|, max relative cost distance over the finite costs) between two results (x, u, cost, status, iters)."""
    fin = np.isfinite(o[2]) & np.isfinite(o8[2])
    return float(np.abs(o[1] - o8[1]).max()), float(np.abs(o[0] - o8[0]).max()), float((np.abs(o[2] - o8[2])[fin] / np.abs(o8[2][fin])).max())


def bounds(gap, mode):
    """(bound on |du|, bound on |dx|) of a mode against the oracle.  tol == 0: quad_routed_spec.bound of the distance between the two
    oracles and 10 x that (test_quad_ipm_exits.py::test_sqp_mode_away_from_the_shipped_horizon).  tol > 0: the figures of
    test_quad_gpu.py::test_quad_sqp_mode_on_the_device -- 1e-8 / 1e-7 below 100 QPs, 1e-6 / 1e-5 at 100 QPs (converged instances are within
    the tolerance of each other's fixed point, up to a hundred QPs of rounding apart) -- or that bound where it is larger."""
    b = Q.bound(max(gap[0], gap[1]))
    if mode[1] > 0.0:
        b = max(b, 1e-6 if mode[0] == 100 else 1e-8)
    return b, 10.0 * b
