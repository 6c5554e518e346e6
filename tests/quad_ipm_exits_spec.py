"""The inputs that drive the quadrotor's box-QP interior point out of its loop by every way but "converged" (TEST INFRASTRUCTURE).

admpc_quad.hip holds two copies of the loop (admpc_quad_solve_kernel<Dense40Path | GenericPath | WidePath> and admpc_quad_seg_kernel), and
each leaves it through the fallback restart (it >= ADMPC_QUAD_IPM_FALLBACK_ITER = 30: cold start, `--it`, no second-order term from then
on, a budget of ipm_iter_max + 30), through the iteration limit (status 0, the iterate is written) or with status 4.  The restart level is
a compile-time constant, but ipm_mu0 and ipm_iter_max are fields of the configuration: a start far too close to the boundary stalls a share
of ordinary instances, and a small limit ends every instance early.  `case` draws the inputs of one path and one case: what
tests/test_quad_ipm_exits.py solves on the device is what tests/test_quad_ipm_exits_cpu.py checks, with the oracle alone, for the class
counts that keep a comparison from passing vacuously, and measures for its bounds.

The paths, their configurations, their environment and their order are quad_routed_spec's (ROUTED_PATHS, path_config, TWO_WAVE_FIRST).

What an iteration count says (budget ipm_iter_max = 50): the stop test stands in front of the restart test, so an instance that reports
exactly 30 converged at its 30th test and never restarted; a restarted instance redoes pass 30 from the cold start, which cannot pass the
stop test (it would have passed it at pass 0), and so reports MORE than 30.  `restarted` is therefore it > 30; the class counts are held
in that form and in the weaker `it >= 30` form."""
import numpy as np

import quad_routed_spec as Q
from ad_mpc_amd.quad_scenarios import random_quad_scenarios

FALLBACK = 30                                                     # ADMPC_QUAD_IPM_FALLBACK_ITER (include/admpc_quad.h)
B, B_SQP = 64, 32
PATHS = Q.TWO_WAVE_FIRST

# The restart case of every horizon: random_quad_scenarios(64, cfg, seed) at ipm_mu0, everything else as shipped (ipm_iter_max = 50).
# The draw of seed 11 stalls a share of the instances at every horizon, but away from N = 5 every stalled instance of it then runs to the
# extended limit; a census with the fp64 oracle over seeds 11 .. 102 and ipm_mu0 = 1e-3 .. 1e-8 gave these draws, the first of each
# horizon that holds an instance that restarts AND converges.  Classes by the fp64 oracle (the 80-bit oracle gives the same counts):
#   N: (seed, ipm_mu0)      it > 30   of those at 80   restarted and converged (instance: count)   it == 30   it < 30   edge cases: at 29 / 30 / 61
RESTART = {
    5: (11, 1e-8),        #    7          6              62: 76                                       0         57         2 /  1 / 1
    10: (28, 1e-5),       #    9          8              28: 57                                       1         54        11 /  9 / 7
    16: (24, 1e-6),       #   12         11              31: 48                                       2         50        10 /  7 / 4
    17: (48, 1e-6),       #   12         11              13: 56                                       1         51         8 /  6 / 4
    20: (21, 1e-7),       #   15         14              23: 67                                       0         49         2 /  2 / 2
    24: (15, 1e-8),       #   19         18              29: 75                                       1         44         4 /  3 / 2
}
# restart_tight_budget (ipm_iter_max = 35): the instances at 80 above stand at 65, and so does instance 62 of N = 5, 67 of N = 20 and 75
# of N = 24 (7 / 8 / 11 / 11 / 15 / 19 at 65); 28 of N = 10, 31 of N = 16 and 13 of N = 17 converge as above.
LIMIT_SEED = 11                                                   # limit_1 / 3 / 8: the default ipm_mu0, 64 / 64 / 39 .. 61 instances at the limit
LIMITS = {"limit_1": 1, "limit_3": 3, "limit_8": 8}
EDGES = {"edge_29": 29, "edge_30": 30, "edge_31": 31}             # the restart is entered from ipm_iter_max = 31 on: 29 / 30 / 61 iterations
# The edge cases solve the restart draw WITHOUT these instances.  An instance stopped at pass 29 or 30 in the middle of its stall has an
# iterate that rounding moves: the fp64 and the 80-bit oracle agree on its iteration count and are this far apart in max(|du|, |dx|)
# (the larger of ipm_iter_max = 29 and 30; at 31, where they restart and run on to 61, every one of them is within 4e-9).  Listed: every
# instance of the draw with more than 1e-8; a bound that covered them (up to 2e-2) would test nothing.  One pair of evaluation orders
# does not find every such instance: the second measure is the fp64 oracle against itself with ubar moved by at most one unit in the last
# place (`one_ulp`, four draws; the iteration counts stay the same); an instance is listed when either measure is above 1e-8.  The second
# adds three to the first: 17 of N = 16, and 30 and 38 of N = 24 (7e-8 and 2e-7), which the 80-bit oracle happens to leave within 2e-9
# and 5e-9 -- and which the device (WidePath) puts 1e-7 from the fp64 oracle.
EDGE_SKIP = {
    5: [10, 43, 45, 58, 62, 63],                                  # 1e-7 7e-7 2e-7 6e-8 4e-8 3e-6
    10: [44],                                                     # 2e-8
    16: [5, 9, 19, 23, 33, 41,                                    # 5e-8 1e-7 3e-7 8e-4 7e-6 6e-8
         17],                                                     # by the second measure (1.1e-8; 80-bit 1e-9)
    17: [2, 19, 43, 45, 46, 52, 62],                              # 1e-6 7e-8 2e-7 2e-2 4e-8 1e-5 2e-8
    20: [3, 6, 10, 13, 15, 16, 25, 27, 32, 44, 46, 55, 58],       # 3e-7 9e-7 3e-7 1e-6 4e-7 2e-6 2e-6 6e-7 3e-7 2e-7 5e-5 2e-3 5e-8
    24: [0, 2, 3, 5, 16, 19, 21, 22, 29, 37, 41, 46, 54, 57, 60,  # 5e-7 9e-8 8e-8 5e-7 9e-6 1e-7 3e-6 2e-4 4e-7 6e-6 4e-8 2e-7 1e-7 9e-3 5e-6
         30, 38],                                                 # by the second measure
}
EDGE_ITERS = {"edge_29": 29, "edge_30": 30, "edge_31": 31 + FALLBACK}
TIGHT = 35                                                        # restart_tight_budget: the extended limit is 35 + 30, not 80
CASES = ["restart", "limit_1", "limit_3", "limit_8", "edge_29", "edge_30", "edge_31", "restart_tight_budget"]

# The distance between the fp64 and the 80-bit oracle on every case, which agree in status and iteration count on every instance:
# (max |du|, max |dx|, max relative cost distance), measured by test_quad_ipm_exits_cpu.py, which holds its own figures at or below these
# (each its figure rounded up to two digits).  `bounds` turns them into the tolerances of the device tests.
GAPS = {
    (5, "restart"): (7.5e-11, 5.8e-10, 1.7e-12), (5, "restart_tight_budget"): (8.1e-11, 5.0e-10, 4.6e-12),
    (5, "limit_1"): (8.4e-16, 1.1e-14, 9.4e-16), (5, "limit_3"): (1.3e-14, 1.1e-13, 1.4e-15), (5, "limit_8"): (7.2e-14, 1.3e-13, 1.1e-15),
    (5, "edge_29"): (7.1e-11, 5.7e-10, 6.4e-16), (5, "edge_30"): (7.7e-13, 6.2e-12, 7.4e-16), (5, "edge_31"): (4.1e-13, 3.2e-12, 9.8e-15),
    (10, "restart"): (1.6e-12, 1.0e-11, 7.0e-14), (10, "restart_tight_budget"): (1.6e-12, 1.0e-11, 1.3e-14),
    (10, "limit_1"): (2.0e-14, 1.8e-13, 1.2e-14), (10, "limit_3"): (3.6e-13, 2.1e-12, 5.7e-14), (10, "limit_8"): (1.1e-12, 1.8e-12, 1.3e-15),
    (10, "edge_29"): (2.0e-10, 1.6e-09, 3.3e-13), (10, "edge_30"): (5.8e-11, 1.5e-10, 1.1e-13), (10, "edge_31"): (1.6e-12, 1.0e-11, 5.1e-14),
    (16, "restart"): (2.7e-10, 2.6e-09, 1.4e-10), (16, "restart_tight_budget"): (3.0e-10, 3.5e-09, 1.6e-10),
    (16, "limit_1"): (6.1e-13, 5.7e-12, 4.2e-13), (16, "limit_3"): (8.7e-12, 2.5e-11, 5.4e-13), (16, "limit_8"): (5.2e-11, 8.8e-11, 2.7e-15),
    (16, "edge_29"): (3.8e-10, 2.6e-09, 4.2e-12), (16, "edge_30"): (2.3e-10, 4.1e-09, 1.1e-11), (16, "edge_31"): (2.2e-10, 2.6e-09, 4.1e-12),
    (17, "restart"): (1.6e-10, 4.4e-10, 4.8e-12), (17, "restart_tight_budget"): (1.6e-10, 7.1e-10, 2.5e-11),
    (17, "limit_1"): (2.9e-13, 5.0e-12, 5.3e-13), (17, "limit_3"): (1.3e-11, 6.7e-11, 5.6e-13), (17, "limit_8"): (8.0e-11, 1.4e-10, 2.6e-14),
    (17, "edge_29"): (5.5e-10, 7.0e-09, 7.5e-11), (17, "edge_30"): (4.4e-10, 4.0e-09, 3.2e-11), (17, "edge_31"): (2.6e-10, 2.0e-09, 4.9e-11),
    (20, "restart"): (1.4e-09, 6.6e-09, 2.8e-10), (20, "restart_tight_budget"): (2.7e-10, 1.6e-09, 5.4e-11),
    (20, "limit_1"): (1.5e-12, 2.4e-11, 3.9e-12), (20, "limit_3"): (1.3e-10, 1.6e-09, 8.2e-11), (20, "limit_8"): (3.3e-10, 5.5e-10, 5.6e-14),
    (20, "edge_29"): (5.1e-10, 4.1e-09, 3.2e-11), (20, "edge_30"): (4.4e-10, 3.3e-09, 1.3e-11), (20, "edge_31"): (5.1e-10, 1.6e-09, 4.9e-11),
    (24, "restart"): (1.6e-09, 2.8e-09, 1.8e-10), (24, "restart_tight_budget"): (1.6e-09, 8.0e-09, 2.4e-10),
    (24, "limit_1"): (8.3e-13, 8.5e-12, 1.5e-12), (24, "limit_3"): (9.1e-11, 2.5e-10, 4.3e-12), (24, "limit_8"): (5.4e-10, 8.0e-10, 1.9e-14),
    (24, "edge_29"): (1.6e-09, 2.8e-09, 4.6e-12), (24, "edge_30"): (1.6e-09, 2.0e-09, 2.1e-11), (24, "edge_31"): (1.6e-09, 2.0e-09, 9.1e-12),
}
# solver_type "SQP" away from N = 10: (sqp_iters, sqp_tol) -> the same three distances; statuses by the fp64 oracle (the 80-bit oracle's are
# the same): (4, 1e-6) all 2, (3, 0) all 0, (100, 1e-6) 24 x 0 and 8 x 2 at N = 5, 15 x 0 and 17 x 2 at N = 17 and at N = 20
SQP_HORIZONS = {5: "generic_N5", 17: "wide_N17", 20: "seg_N20"}
SQP_MODES = [(4, 1e-6), (3, 0.0), (100, 1e-6)]
SQP_GAPS = {
    (5, 4, 1e-6): (2.1e-14, 7.2e-14, 1.1e-15), (5, 3, 0.0): (5.0e-14, 7.2e-14, 8.8e-16), (5, 100, 1e-6): (1.5e-14, 4.3e-14, 5.6e-16),
    (17, 4, 1e-6): (6.8e-11, 2.0e-10, 3.6e-12), (17, 3, 0.0): (1.0e-10, 1.6e-10, 2.2e-12), (17, 100, 1e-6): (2.2e-10, 1.9e-09, 1.6e-11),
    (20, 4, 1e-6): (3.8e-10, 9.8e-10, 2.2e-11), (20, 3, 0.0): (1.1e-09, 1.8e-09, 1.2e-11), (20, 100, 1e-6): (6.4e-10, 4.6e-09, 4.1e-11),
}

HORIZONS = sorted(RESTART)
assert HORIZONS == sorted({r[0] for r in Q.ROUTED_PATHS.values()})


def path_of(N):
    """A path of horizon N (the inputs and the oracle's results depend on the horizon alone)."""
    return next(p for p in PATHS if Q.ROUTED_PATHS[p][0] == N)


_SCEN = {}


def _draw(N, seed):
    if (N, seed) not in _SCEN:
        _SCEN[N, seed] = random_quad_scenarios(B, Q.path_config(path_of(N)), seed=seed)
    return _SCEN[N, seed]


def case(path, name):
    """(cfg, scenarios) of one path and one case of CASES; the scenarios are shared between the calls and must stay unchanged."""
    N = Q.ROUTED_PATHS[path][0]
    cfg = Q.path_config(path)
    seed, mu0 = RESTART[N]
    if name in LIMITS:
        cfg.ipm_iter_max = LIMITS[name]
        return cfg, _draw(N, LIMIT_SEED)
    cfg.ipm_mu0 = mu0
    s = _draw(N, seed)
    if name in EDGES:
        cfg.ipm_iter_max = EDGES[name]
        keep = np.setdiff1d(np.arange(B), EDGE_SKIP[N])
        s = {k: v[keep] for k, v in s.items()}
    elif name == "restart_tight_budget":
        cfg.ipm_iter_max = TIGHT
    else:
        assert name == "restart", name
    return cfg, s


def restarted(it):
    return np.asarray(it) > FALLBACK


def one_ulp(ubar, draw):
    """ubar with every entry moved by -1, 0 or +1 units in the last place (relative 2^-52), seeded by `draw`."""
    return ubar * (1.0 + 2.0 ** -52 * np.random.default_rng(draw).integers(-1, 2, ubar.shape))


def bounds(N, name):
    """(bound on |du| and |dx|, relative bound on the cost) of a case from its measured distance between the two oracles."""
    du, dx, dc = GAPS[N, name]
    return Q.bound(max(du, dx)), max(1e-9, 4.0 * dc)


def sqp_case(N, iters, tol):
    """solver_type "SQP" away from N = 10: the inputs of test_quad_gpu.py::test_quad_sqp_mode_on_the_device, B = 32."""
    cfg = Q.path_config(SQP_HORIZONS[N])
    s = random_quad_scenarios(B_SQP, cfg, seed=7, pos_err=0.8, tilt=0.2, aggressive=0.0)
    cfg.sqp_iters, cfg.sqp_tol = iters, tol
    return cfg, s


def sqp_bound(N, iters, tol):
    du, dx, dc = SQP_GAPS[N, iters, tol]
    return Q.bound(max(du, dx))


def gaps(o, o8):
    """(max |du|, max |dx|, max relative cost distance) between two results (x, u, cost, status, iters)."""
    return float(np.abs(o[1] - o8[1]).max()), float(np.abs(o[0] - o8[0]).max()), float((np.abs(o[2] - o8[2]) / np.abs(o8[2])).max())
