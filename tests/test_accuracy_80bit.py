"""Every device path against 80-bit arithmetic (the oracles built with ORACLE_LONG_DOUBLE: liboracle_ld.so, libquad_oracle_ld.so).

The parity suite compares each kernel with the fp64 oracle at 1e-8 (N <= 32) / 1e-7; that headroom absorbs two correct evaluation
orders and sits 10^2 .. 10^4 x above what the kernels deliver.  Here each path solves one seeded batch and is held to committed
budgets on its distance from the 80-bit solution, next to the fp64 oracle's own distance:
  (a) the share of instances with the 80-bit oracle's status (0) and iteration count is at least the measured share minus 0.02;
  (b) on those instances the device's median, 99 % quantile and max of the per-instance max |du| and max |dx| are within budget;
  (c) the fp64 oracle's max |du| and max |dx| are within its budget (the CPU yardstick of tests/test_oracle_hygiene.py, per family).
Budgets are at most 4 x the value measured on the MI355X, rounded up to two significant digits; the measured values stand on each
row of BUDGET.  Kernels are bit-wise repeatable and draw-order free, so for a fixed build the numbers are deterministic.  Rows
whose device max budget is not 10 x below the path's parity tolerance are named in KNOWN_WEAK, with the reason.

Further: yaw far from zero (psi + 2 pi K, |psi| up to 1e4: the hand-written Cody-Waite reduction of sincos_small) on kernels F, S
and R, and the shooting of both vehicle models at the edges of their functions (quadrant boundaries of psi, huge psi, steering at
its bounds, every blend value, GP features 10 - 40 length scales from every training point: exp_nonpos in its underflow, denormal
and clamp range), against the 80-bit rk4_sens."""
import math

import numpy as np
import pytest

from ad_mpc_amd.config import default_config, tight_config, set_gp
from ad_mpc_amd.quad_config import default_quad_config, set_quad_gp, QNX, QNU
from ad_mpc_amd.quad_scenarios import random_quad_scenarios
from ad_mpc_amd.scenarios import random_scenarios, grid_gp

pytestmark = pytest.mark.gpu

B_SOLVE = 512
SHARE_MARGIN = 0.02

# ---------------------------------------------------------------------------------------------------------------------------------
# the paths: (vehicle, N, model, blend, environment); blend None: the generator's default (100, 110), i.e. p = 0 everywhere
CAR = {
    "F20_dynamic": (20, "nominal", (3.0, 5.0), {}),
    "R20_dynamic": (20, "nominal", (3.0, 5.0), {"ADMPC_QP": "riccati"}),
    "F20_kinematic": (20, "nominal", (100.0, 110.0), {}),
    "R20_kinematic": (20, "nominal", (100.0, 110.0), {"ADMPC_QP": "riccati"}),
    "F20_q127_tight": (20, "q127_tight", (3.0, 5.0), {}),
    "F20_gp": (20, "gp", None, {}),
    "F20_sqp3": (20, "sqp3", (3.0, 5.0), {}),
    "S40": (40, "nominal", (3.0, 5.0), {}),
    "R40": (40, "nominal", (3.0, 5.0), {"ADMPC_QP": "riccati"}),
    "S60": (60, "nominal", (3.0, 5.0), {}),
    "R60": (60, "nominal", (3.0, 5.0), {"ADMPC_QP": "riccati"}),
    "S80": (80, "nominal", (3.0, 5.0), {}),
    "R80": (80, "nominal", (3.0, 5.0), {"ADMPC_QP": "riccati"}),
    "R40_gp": (40, "gp", None, {}),
    "S40_gp": (40, "gp", None, {"ADMPC_QP": "seg"}),
    "R13": (13, "nominal", (3.0, 5.0), {}),
    "R30": (30, "nominal", (3.0, 5.0), {}),
    "R97": (97, "nominal", (3.0, 5.0), {}),
    "F20_q7_random": (20, "q7_random", (3.0, 5.0), {}),
    "S80_q7_random": (80, "q7_random", (3.0, 5.0), {}),
}
QUAD = {
    "Q10_dense40": (10, "nominal", {}),
    "Q10_generic": (10, "nominal", {"ADMPC_QUAD_GENERIC": "1"}),
    "Q5_generic": (5, "nominal", {}),
    "Q13_generic": (13, "nominal", {}),
    "Q17_wide": (17, "nominal", {}),
    "Q24_wide": (24, "nominal", {}),
    "Q20_wide": (20, "nominal", {"ADMPC_QUAD_WIDE": "1"}),
    "Q20_seg": (20, "nominal", {}),
    "Q20_seg_gp": (20, "gp", {}),
    "Q20_seg_drag": (20, "drag", {}),
    "Q10_random": (10, "random", {}),
}
# a path that only an environment variable selects: its bits must differ from the default path's on the same inputs
SIBLING = {"R20_dynamic": "F20_dynamic", "R20_kinematic": "F20_kinematic", "R40": "S40", "R60": "S60", "R80": "S80",
           "S40_gp": "R40_gp", "Q10_generic": "Q10_dense40", "Q20_wide": "Q20_seg"}

# (min share of identical iteration counts, device |du| (median, 99 %, max), device |dx| (median, 99 %, max), fp64 oracle max (|du|, |dx|));
# below each row the values measured on the MI355X (512 instances, seed 100; the quadrotor seed 100 + N)
BUDGET = {
    "F20_dynamic": (0.98, (1.1e-13, 5.2e-13, 6.4e-13), (8.4e-14, 2.3e-13, 2.9e-13), (6.4e-13, 2.9e-13)),
    #   measured: share 1.0000; |du| 2.6e-14 / 1.3e-13 / 1.6e-13; |dx| 2.1e-14 / 5.7e-14 / 7.1e-14; fp64 |du| 1.6e-13, |dx| 7.1e-14
    "R20_dynamic": (0.98, (1.1e-13, 5.2e-13, 6.4e-13), (8.4e-14, 2.4e-13, 2.9e-13), (6.4e-13, 2.9e-13)),
    #   measured: share 1.0000; |du| 2.6e-14 / 1.3e-13 / 1.6e-13; |dx| 2.1e-14 / 6.0e-14 / 7.1e-14; fp64 |du| 1.6e-13, |dx| 7.1e-14
    "F20_kinematic": (0.98, (1.1e-13, 5.2e-13, 6.8e-13), (6.0e-14, 2.3e-13, 2.9e-13), (6.8e-13, 2.9e-13)),
    #   measured: share 1.0000; |du| 2.6e-14 / 1.3e-13 / 1.7e-13; |dx| 1.5e-14 / 5.7e-14 / 7.1e-14; fp64 |du| 1.7e-13, |dx| 7.1e-14
    "R20_kinematic": (0.98, (1.0e-13, 5.2e-13, 6.8e-13), (5.6e-14, 2.3e-13, 2.9e-13), (6.8e-13, 2.9e-13)),
    #   measured: share 1.0000; |du| 2.5e-14 / 1.3e-13 / 1.7e-13; |dx| 1.4e-14 / 5.7e-14 / 7.1e-14; fp64 |du| 1.7e-13, |dx| 7.1e-14
    "F20_q127_tight": (0.98, (1.0e-13, 4.4e-13, 7.2e-13), (8.4e-14, 2.3e-13, 2.8e-13), (5.6e-13, 2.8e-13)),
    #   measured: share 1.0000; |du| 2.5e-14 / 1.1e-13 / 1.8e-13; |dx| 2.1e-14 / 5.7e-14 / 6.8e-14; fp64 |du| 1.4e-13, |dx| 6.8e-14
    "F20_gp": (0.98, (1.6e-13, 4.4e-11, 1.8e-10), (1.2e-13, 4.4e-10, 1.3e-09), (6.0e-13, 2.2e-11)),
    #   measured: share 1.0000; |du| 3.9e-14 / 1.1e-11 / 4.4e-11; |dx| 2.8e-14 / 1.1e-10 / 3.2e-10; fp64 |du| 1.5e-13, |dx| 5.3e-12
    "F20_sqp3": (0.98, (2.9e-14, 1.6e-13, 1.9e-13), (2.9e-14, 8.4e-14, 8.4e-14), (2.0e-13, 8.4e-14)),
    #   measured: share 1.0000; |du| 7.1e-15 / 3.9e-14 / 4.7e-14; |dx| 7.1e-15 / 2.1e-14 / 2.1e-14; fp64 |du| 4.8e-14, |dx| 2.1e-14
    "S40": (0.98, (2.0e-13, 5.6e-12, 2.8e-10), (1.3e-13, 6.0e-13, 2.8e-11), (4.0e-12, 6.4e-13)),
    #   measured: share 1.0000; |du| 5.0e-14 / 1.4e-12 / 7.0e-11; |dx| 3.2e-14 / 1.5e-13 / 6.9e-12; fp64 |du| 1.0e-12, |dx| 1.6e-13
    "R40": (0.98, (1.9e-13, 1.0e-12, 2.3e-12), (1.2e-13, 4.0e-13, 4.8e-13), (4.0e-12, 6.4e-13)),
    #   measured: share 1.0000; |du| 4.6e-14 / 2.5e-13 / 5.6e-13; |dx| 2.8e-14 / 1.0e-13 / 1.2e-13; fp64 |du| 1.0e-12, |dx| 1.6e-13
    "S60": (0.98, (2.9e-13, 2.4e-11, 4.4e-10), (6.0e-13, 1.6e-11, 3.1e-11), (4.0e-11, 3.9e-12)),
    #   measured: share 1.0000; |du| 7.2e-14 / 6.0e-12 / 1.1e-10; |dx| 1.5e-13 / 4.0e-12 / 7.6e-12; fp64 |du| 1.0e-11, |dx| 9.7e-13
    "R60": (0.98, (2.0e-13, 9.6e-13, 9.6e-12), (1.3e-13, 4.4e-13, 1.4e-12), (4.0e-11, 3.9e-12)),
    #   measured: share 1.0000; |du| 4.8e-14 / 2.4e-13 / 2.4e-12; |dx| 3.1e-14 / 1.1e-13 / 3.5e-13; fp64 |du| 1.0e-11, |dx| 9.7e-13
    "S80": (0.98, (3.5e-13, 1.4e-10, 3.6e-09), (1.4e-12, 6.4e-11, 3.6e-10), (2.1e-10, 2.6e-11)),
    #   measured: share 1.0000; |du| 8.7e-14 / 3.3e-11 / 9.0e-10; |dx| 3.4e-13 / 1.6e-11 / 8.9e-11; fp64 |du| 5.1e-11, |dx| 6.3e-12
    "R80": (0.98, (2.1e-13, 1.1e-12, 6.0e-11), (1.6e-13, 5.6e-13, 8.0e-12), (2.1e-10, 2.6e-11)),
    #   measured: share 1.0000; |du| 5.2e-14 / 2.7e-13 / 1.5e-11; |dx| 3.9e-14 / 1.4e-13 / 2.0e-12; fp64 |du| 5.1e-11, |dx| 6.3e-12
    "R40_gp": (0.98, (3.2e-13, 5.6e-09, 1.2e-08), (2.3e-13, 2.2e-06, 4.0e-06), (1.4e-08, 3.7e-06)),
    #   measured: share 1.0000; |du| 8.0e-14 / 1.4e-09 / 3.0e-09; |dx| 5.6e-14 / 5.3e-07 / 1.0e-06; fp64 |du| 3.3e-09, |dx| 9.1e-07
    "S40_gp": (0.98, (3.9e-13, 2.5e-06, 3.4e-06), (3.4e-13, 3.7e-02, 6.8e-02), (1.4e-08, 3.7e-06)),
    #   measured: share 1.0000; |du| 9.7e-14 / 6.2e-07 / 8.3e-07; |dx| 8.5e-14 / 9.1e-03 / 1.7e-02; fp64 |du| 3.3e-09, |dx| 9.1e-07
    "R13": (0.98, (4.4e-14, 2.0e-13, 2.6e-13), (7.2e-14, 1.8e-13, 1.8e-13), (2.6e-13, 1.8e-13)),
    #   measured: share 1.0000; |du| 1.1e-14 / 4.9e-14 / 6.3e-14; |dx| 1.8e-14 / 4.3e-14 / 4.3e-14; fp64 |du| 6.4e-14, |dx| 4.3e-14
    "R30": (0.98, (1.8e-13, 1.1e-12, 1.4e-10), (1.2e-13, 3.8e-13, 1.0e-11), (2.4e-10, 1.8e-11)),
    #   measured: share 1.0000; |du| 4.3e-14 / 2.6e-13 / 3.3e-11; |dx| 2.8e-14 / 9.4e-14 / 2.5e-12; fp64 |du| 5.9e-11, |dx| 4.5e-12
    "R97": (0.98, (2.3e-13, 3.2e-12, 1.2e-09), (2.0e-13, 8.4e-13, 1.4e-10), (3.3e-09, 3.6e-10)),
    #   measured: share 1.0000; |du| 5.7e-14 / 7.9e-13 / 3.0e-10; |dx| 5.0e-14 / 2.1e-13 / 3.3e-11; fp64 |du| 8.2e-10, |dx| 8.9e-11
    "Q10_dense40": (0.98, (2.7e-13, 4.8e-12, 6.8e-12), (1.1e-12, 8.4e-12, 1.2e-11), (8.4e-12, 1.5e-11)),
    #   measured: share 1.0000; |du| 6.6e-14 / 1.2e-12 / 1.7e-12; |dx| 2.6e-13 / 2.1e-12 / 2.8e-12; fp64 |du| 2.1e-12, |dx| 3.6e-12
    "Q10_generic": (0.98, (2.3e-13, 4.8e-12, 6.4e-12), (9.2e-13, 8.8e-12, 1.1e-11), (8.4e-12, 1.5e-11)),
    #   measured: share 1.0000; |du| 5.7e-14 / 1.2e-12 / 1.6e-12; |dx| 2.3e-13 / 2.2e-12 / 2.7e-12; fp64 |du| 2.1e-12, |dx| 3.6e-12
    "Q5_generic": (0.98, (4.4e-15, 1.7e-13, 2.1e-13), (2.6e-14, 2.8e-13, 3.4e-13), (2.2e-13, 3.8e-13)),
    #   measured: share 1.0000; |du| 1.1e-15 / 4.1e-14 / 5.1e-14; |dx| 6.5e-15 / 7.0e-14 / 8.5e-14; fp64 |du| 5.5e-14, |dx| 9.5e-14
    "Q13_generic": (0.98, (2.9e-12, 3.7e-11, 5.2e-11), (8.8e-12, 6.4e-11, 8.8e-11), (4.8e-11, 8.0e-11)),
    #   measured: share 1.0000; |du| 7.1e-13 / 9.2e-12 / 1.3e-11; |dx| 2.2e-12 / 1.6e-11 / 2.2e-11; fp64 |du| 1.2e-11, |dx| 2.0e-11
    "Q17_wide": (0.98, (4.8e-11, 3.0e-10, 4.4e-10), (1.3e-10, 6.4e-10, 7.6e-10), (4.0e-10, 6.8e-10)),
    #   measured: share 1.0000; |du| 1.2e-11 / 7.4e-11 / 1.1e-10; |dx| 3.1e-11 / 1.6e-10 / 1.9e-10; fp64 |du| 9.9e-11, |dx| 1.7e-10
    "Q24_wide": (0.98, (1.5e-09, 5.2e-09, 8.0e-09), (2.5e-09, 8.0e-09, 1.2e-08), (6.4e-09, 9.6e-09)),
    #   measured: share 1.0000; |du| 3.6e-10 / 1.3e-09 / 2.0e-09; |dx| 6.1e-10 / 2.0e-09 / 3.0e-09; fp64 |du| 1.6e-09, |dx| 2.4e-09
    "Q20_wide": (0.98, (2.5e-10, 1.3e-09, 2.2e-09), (5.2e-10, 2.0e-09, 2.4e-09), (2.7e-09, 2.6e-09)),
    #   measured: share 1.0000; |du| 6.1e-11 / 3.2e-10 / 5.5e-10; |dx| 1.3e-10 / 5.0e-10 / 5.9e-10; fp64 |du| 6.7e-10, |dx| 6.3e-10
    "Q20_seg": (0.98, (2.2e-12, 5.2e-11, 9.2e-11), (6.0e-12, 3.5e-09, 6.0e-09), (2.7e-09, 2.6e-09)),
    #   measured: share 1.0000; |du| 5.5e-13 / 1.3e-11 / 2.3e-11; |dx| 1.5e-12 / 8.7e-10 / 1.5e-09; fp64 |du| 6.7e-10, |dx| 6.3e-10
    "Q20_seg_gp": (0.98, (2.1e-12, 2.3e-11, 4.8e-11), (6.4e-12, 1.4e-09, 3.2e-09), (2.0e-09, 2.4e-09)),
    #   measured: share 1.0000; |du| 5.1e-13 / 5.7e-12 / 1.2e-11; |dx| 1.6e-12 / 3.5e-10 / 8.0e-10; fp64 |du| 4.8e-10, |dx| 5.8e-10
    "Q20_seg_drag": (0.98, (2.2e-12, 4.8e-11, 1.0e-10), (5.6e-12, 2.8e-09, 6.0e-09), (1.4e-09, 2.3e-09)),
    #   measured: share 1.0000; |du| 5.3e-13 / 1.2e-11 / 2.5e-11; |dx| 1.4e-12 / 6.8e-10 / 1.5e-09; fp64 |du| 3.3e-10, |dx| 5.6e-10
    "F20_q7_random": (0.98, (7.2e-14, 4.8e-13, 1.3e-10), (8.4e-14, 2.9e-13, 1.9e-11), (4.4e-12, 6.4e-13)),
    #   measured: share 1.0000; |du| 1.8e-14 / 1.2e-13 / 3.2e-11; |dx| 2.1e-14 / 7.1e-14 / 4.8e-12; fp64 |du| 1.1e-12, |dx| 1.6e-13
    "S80_q7_random": (0.98, (7.2e-13, 5.2e-09, 3.6e-07), (5.6e-12, 8.0e-10, 4.8e-08), (2.7e-08, 3.7e-09)),
    #   measured: share 1.0000; |du| 1.8e-13 / 1.3e-09 / 9.0e-08; |dx| 1.4e-12 / 2.0e-10 / 1.2e-08; fp64 |du| 6.7e-09, |dx| 9.1e-10
    "Q10_random": (0.98, (1.8e-13, 1.8e-12, 3.4e-12), (6.0e-13, 4.0e-12, 8.8e-12), (3.5e-12, 6.4e-12)),
    #   measured: share 1.0000; |du| 4.5e-14 / 4.3e-13 / 8.3e-13; |dx| 1.5e-13 / 1.0e-12 / 2.2e-12; fp64 |du| 8.7e-13, |dx| 1.6e-12
}
# Rows whose device max budget (|du| or |dx|) is not 10 x below the parity tolerance (1e-8 for N <= 32 and the quadrotor, 1e-7 above):
# known weaknesses of the suite, each with its reason.
KNOWN_WEAK = {
    "F20_gp": "kernel F on GP models: |du| 4.4e-11 and |dx| 3.2e-10 against 1.5e-13 and 5.3e-12 for the fp64 oracle, whose stage-wise "
              "recursion does not share the loss; condensing 20 stages of the GP-augmented dynamics (its unstable lateral mode) costs the "
              "digits, as for kernel S at N = 40.  Not conditioning of the problem: a fix should bring it within 10 x of the oracle",
    "R40_gp": "conditioning shared with the fp64 oracle (|du| 3.3e-9, |dx| 9.1e-7 there): the unstable lateral mode of the GP model",
    "S40_gp": "the known-bad case (kernel S on GP models, 300 x / 1.7e4 x kernel R's |du| / |dx|); the budget pins today's value so that "
              "it cannot get worse.  A fix should tighten it to within 10 x of kernel R's row",
    "Q20_wide": "the quadrotor at N >= 20 is as far from 80-bit in the fp64 oracle (|du| 6.7e-10): conditioning of the condensed QP",
    "Q24_wide": "as Q20_wide (fp64 oracle |du| 1.6e-9, |dx| 2.4e-9)",
    "Q20_seg": "|dx| 1.5e-9 (2.4 x the fp64 oracle's 6.3e-10) while |du| is 30 x closer to 80-bit than the oracle: the states are "
               "expanded through 20 stages of the same ill-conditioned dynamics",
    "Q20_seg_gp": "as Q20_seg",
    "Q20_seg_drag": "as Q20_seg",
    "S80_q7_random": "kernel S at N = 80 as in the S80 row (device max |du| 18 x the fp64 oracle's there, 13 x here) on a draw whose "
                     "problem is 100 x worse conditioned than the shipped one (fp64 oracle |du| 6.7e-9 against 5.1e-11): the device is "
                     "9.0e-8 from 80-bit, inside the 1e-7 parity tolerance but not 10 x below it",
}


def _parity_tol(name):
    n = CAR[name][0] if name in CAR else 0
    return 1e-7 if n > 32 else 1e-8


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def car_oracles():
    from oracle.oracle import Oracle
    return Oracle(omp=True), Oracle(variant="ld")


@pytest.fixture(scope="module")
def quad_oracles():
    from oracle.quad_oracle import QuadOracle
    return QuadOracle(), QuadOracle(variant="ld")


@pytest.fixture(scope="module")
def runs():
    return {}


def _car_cfg(N, model):
    if model == "q7_random":                  # a fixed draw of tests/test_gpu_parity.py:random_q7_problem (kernels F / S, qmask 7)
        from test_gpu_parity import random_q7_problem
        return random_q7_problem(np.random.default_rng([80, N]), N)
    if model == "q127_tight":
        return tight_config(N=N, q=(10.0, 10.0, 100.0, 2.0, 3.0, 4.0, 5.0))
    cfg = default_config(N=N, sqp_iters=3 if model == "sqp3" else 1)
    if model == "gp":
        set_gp(cfg, grid_gp())
    return cfg


def _quad_cfg(N, model):
    if model == "random":                     # a fixed draw of tests/test_problem_data_quad.py:random_quad_problem
        from test_problem_data_quad import random_quad_problem
        return random_quad_problem(np.random.default_rng([80, N]), N)
    cfg = default_quad_config(N=N, t_horizon=0.1 * N)
    if model == "gp":
        from test_quad_oracle import quad_gps
        set_quad_gp(cfg, quad_gps())
    elif model == "drag":
        cfg.rdrv[0], cfg.rdrv[1], cfg.rdrv[2] = -0.35, -0.25, -0.1
    return cfg


def _with_env(monkeypatch, env, make):
    for k in ("ADMPC_QP", "ADMPC_QUAD_GENERIC", "ADMPC_QUAD_WIDE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return make()
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


def _car_run(name, runs, car_oracles, monkeypatch):
    """(device, fp64 oracle, 80-bit oracle) results of path `name`; the oracle solves are shared by paths on the same inputs."""
    from ad_mpc_amd.engine import BatchSolver
    N, model, blend, env = CAR[name]
    key = ("car", N, model, blend)
    cfg = _car_cfg(N, model)
    if key not in runs:
        kw = {} if blend is None else dict(blend=blend)
        s = random_scenarios(B_SOLVE, N=N, Ts=cfg.Ts, seed=100, **kw)
        a = (cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
        runs[key] = (s, car_oracles[0].solve_batch(*a, nthreads=16), car_oracles[1].solve_batch(*a))
    s, o64, o80 = runs[key]

    def dev():
        eng = BatchSolver(cfg, device=0)
        g = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
        eng.close()
        return g
    if name not in runs:
        runs[name] = _with_env(monkeypatch, env, dev)
    return runs[name], o64, o80


def _quad_run(name, runs, quad_oracles, monkeypatch):
    from ad_mpc_amd.engine import QuadBatchSolver
    N, model, env = QUAD[name]
    key = ("quad", N, model)
    cfg = _quad_cfg(N, model)
    if key not in runs:
        s = random_quad_scenarios(B_SOLVE, cfg, seed=100 + N)
        a = (cfg, s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"])
        runs[key] = (s, quad_oracles[0].solve_batch(*a, nthreads=16), quad_oracles[1].solve_batch(*a, nthreads=16))
    s, o64, o80 = runs[key]

    def dev():
        eng = QuadBatchSolver(cfg, device=0)
        g = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"])
        eng.close()
        return g
    if name not in runs:
        runs[name] = _with_env(monkeypatch, env, dev)
    return runs[name], o64, o80


def _distance(g, t):
    """Instances where g has the 80-bit oracle's status 0 and iteration count, and there per instance max |du|, max |dx|."""
    same = (g[3] == t[3]) & (g[4] == t[4]) & (t[3] == 0)
    B = len(same)
    du = np.abs(g[1] - t[1]).reshape(B, -1).max(axis=1)[same]
    dx = np.abs(g[0] - t[0]).reshape(B, -1).max(axis=1)[same]
    return same, du, dx


def _q(v):
    return np.median(v), np.quantile(v, 0.99), v.max()


def _check(name, g, o64, o80, g_sibling=None):
    same, du, dx = _distance(g, o80)
    _, du64, dx64 = _distance(o64, o80)
    share = same.mean()
    mu, mx = _q(du), _q(dx)
    print("ACC %-15s share %.4f  device |du| %.1e / %.1e / %.1e  |dx| %.1e / %.1e / %.1e  fp64 max |du| %.1e |dx| %.1e"
          % ((name, share) + mu + mx + (du64.max(), dx64.max())))
    if g_sibling is not None:                                     # the environment variable did select another kernel
        assert (g[1] != g_sibling[1]).any() or (g[0] != g_sibling[0]).any(), name
    assert name in BUDGET, "no budget for " + name
    b_share, b_u, b_x, (b_u64, b_x64) = BUDGET[name]
    assert share >= b_share, (name, share)
    for what, got, lim in (("du", mu, b_u), ("dx", mx, b_x)):
        for stat, v, l in zip(("median", "99%", "max"), got, lim):
            assert v <= l, "%s: device |%s| %s %.3e above the budget %.2e" % (name, what, stat, v, l)
    assert du64.max() <= b_u64 and dx64.max() <= b_x64, (name, du64.max(), dx64.max())


@pytest.mark.parametrize("name", list(CAR))
def test_car_path_against_80_bit(name, runs, car_oracles, monkeypatch):
    g, o64, o80 = _car_run(name, runs, car_oracles, monkeypatch)
    sib = _car_run(SIBLING[name], runs, car_oracles, monkeypatch)[0] if name in SIBLING else None
    _check(name, g, o64, o80, sib)


@pytest.mark.parametrize("name", list(QUAD))
def test_quad_path_against_80_bit(name, runs, quad_oracles, monkeypatch):
    g, o64, o80 = _quad_run(name, runs, quad_oracles, monkeypatch)
    sib = _quad_run(SIBLING[name], runs, quad_oracles, monkeypatch)[0] if name in SIBLING else None
    _check(name, g, o64, o80, sib)


def test_budgets_cover_every_path():
    assert set(BUDGET) == set(CAR) | set(QUAD)
    for name, (_, bu, bx, _) in BUDGET.items():
        assert (max(bu[2], bx[2]) * 10 > _parity_tol(name)) == (name in KNOWN_WEAK), name


# ---------------------------------------------------------------------------------------------------------------------------------
# yaw far from zero: psi + 2 pi K in x0, xbar, yref and yref_e; the problem is the same one, its inputs rounded at |psi| ~ 2 pi K
YAW_K = (10, 1000, 1600)
YAW_PATH = {"F20": 20, "S40": 40, "R30": 30}           # the default path of each horizon
# device max |du|, max |dx| from 80-bit on the shifted batch (256 instances, seed 300), per K: 4 x the measured value.  The distance grows
# with |psi| eps in the fp64 oracle alike (same column, "fp64"): the inputs and every stage state carry psi at its ulp (1.8e-12 at 1e4).
YAW_BUDGET = {                         # measured: device |du|, |dx|;  fp64 oracle |du|, |dx|
    "F20": {0: (5.6e-13, 2.6e-13),     # 1.4e-13, 6.4e-14;  2.3e-13, 6.4e-14
            10: (9.2e-13, 1.4e-12),    # 2.3e-13, 3.4e-13;  2.3e-13, 3.4e-13
            1000: (5.2e-11, 9.6e-11),  # 1.3e-11, 2.4e-11;  1.3e-11, 2.4e-11
            1600: (1.2e-10, 2.0e-10)},  # 2.8e-11, 4.9e-11;  2.8e-11, 4.9e-11
    "S40": {0: (3.0e-11, 8.4e-12),     # 7.4e-12, 2.1e-12;  2.9e-13, 1.3e-13
            10: (1.2e-11, 2.2e-12),    # 2.8e-12, 5.3e-13;  1.1e-12, 5.0e-13
            1000: (2.6e-10, 2.2e-10),  # 6.3e-11, 5.5e-11;  6.3e-11, 5.5e-11
            1600: (6.4e-10, 4.8e-10)},  # 1.6e-10, 1.2e-10;  1.6e-10, 1.2e-10
    "R30": {0: (1.2e-12, 4.0e-13),     # 2.8e-13, 1.0e-13;  2.8e-13, 1.0e-13
            10: (3.6e-12, 1.9e-12),    # 9.0e-13, 4.6e-13;  9.1e-13, 4.5e-13
            1000: (1.8e-10, 1.5e-10),  # 4.5e-11, 3.6e-11;  4.5e-11, 3.6e-11
            1600: (4.8e-10, 2.7e-10)},  # 1.2e-10, 6.6e-11;  1.2e-10, 6.6e-11
}


def _shift_yaw(s, K):
    t = {k: v.copy() for k, v in s.items()}
    d = 2 * math.pi * K
    t["x0"][:, 2] += d; t["xbar"][:, :, 2] += d; t["yref"][:, :, 2] += d; t["yref_e"][:, 2] += d
    return t


@pytest.mark.parametrize("path", list(YAW_PATH))
def test_large_yaw_against_80_bit(path, car_oracles):
    """Statuses and iteration counts of the unshifted batch, and the distance from 80-bit within YAW_BUDGET at every K."""
    from ad_mpc_amd.engine import BatchSolver
    N = YAW_PATH[path]
    cfg = default_config(N=N)
    s0 = random_scenarios(256, N=N, seed=300, blend=(3.0, 5.0))
    eng = BatchSolver(cfg, device=0)
    run = lambda s: eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    g0 = run(s0)
    res = []
    for K in (0,) + YAW_K:
        s = _shift_yaw(s0, K)
        g = run(s)
        a = (cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
        o80 = car_oracles[1].solve_batch(*a)
        same, du, dx = _distance(g, o80)
        _, du64, dx64 = _distance(car_oracles[0].solve_batch(*a, nthreads=16), o80)
        psi = np.abs(s["x0"][:, 2]).max()
        print("YAW %s K %4d |psi| <= %.0f  share %.3f  device max |du| %.1e |dx| %.1e   fp64 max |du| %.1e |dx| %.1e"
              % (path, K, psi, same.mean(), du.max(), dx.max(), du64.max(), dx64.max()))
        res.append((K, g, same.mean(), psi, du.max(), dx.max()))
    eng.close()
    for K, g, share, psi, du, dx in res:
        np.testing.assert_array_equal(g[3], g0[3]); np.testing.assert_array_equal(g[4], g0[4])
        assert share >= res[0][2] - SHARE_MARGIN, (path, K, share)
        bu, bx = YAW_BUDGET[path][K]
        assert du <= bu and dx <= bx, (path, K, du, dx)


# ---------------------------------------------------------------------------------------------------------------------------------
# shooting at the edges of the model functions; per entry: device error <= SHOOT_FACTOR x the fp64 oracle's + 1e-13 max(1, |ref|)
SHOOT_FACTOR = 8.0


def _assert_shooting(tag, got, ref64, ref80):
    err = np.abs(got - ref80); err64 = np.abs(ref64 - ref80)
    lim = SHOOT_FACTOR * err64 + 1e-13 * np.maximum(1.0, np.abs(ref80))
    worst = np.unravel_index(np.argmax(err / lim), err.shape)
    print("SHOOT %-28s max device err %.1e  fp64 err %.1e  worst ratio to the bound %.3f" % (tag, err.max(), err64.max(), (err / lim).max()))
    assert np.isfinite(got).all(), tag
    assert (err <= lim).all(), (tag, worst, got[worst], ref80[worst], ref64[worst])


def _car_edge_states():
    """Rows (x, u, p): psi at k pi/4 and 1..3 ulp either side (k = -8 .. 8), psi = theta + 2 pi K; steering at -ubx, 0, +ubx in turn;
    p cycling through the golden set's blend values 0, 0.3, 1."""
    rng = np.random.default_rng(11)
    psis = []
    for k in range(-8, 9):
        c = k * math.pi / 4
        psis.append(c)
        lo = hi = c
        for _ in range(3):
            lo = np.nextafter(lo, -np.inf); hi = np.nextafter(hi, np.inf)
            psis += [lo, hi]
    for K in YAW_K:
        for th in (-2.5, -0.7, 0.0, 0.4, 1.9, math.pi / 4, -math.pi / 2):
            psis.append(th + 2 * math.pi * K)
    cfg = default_config(N=2)
    steer = (cfg.lbx_delta, 0.0, cfg.ubx_delta)
    rows = []
    for i, psi in enumerate(psis):
        x = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), psi, rng.uniform(2, 15), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3),
                      steer[i % 3]])
        u = np.array([rng.uniform(-10, 5), rng.uniform(-3, 3)])
        rows.append((x, u, (0.0, 0.3, 1.0)[(i // 3) % 3]))
    return rows


def _far_gp():
    """Three 1-D GPs on v_x, v_y, r whose 20 training points sit in a narrow interval below each feature: see _gp_tail_states."""
    return [dict(feat=3, out=3, Z=np.linspace(1.0, 2.0, 20), alpha=np.linspace(-0.4, 0.5, 20), length_scale=0.2, sigma_f=1.0, ymean=0.01),
            dict(feat=4, out=4, Z=np.linspace(-1.3, -1.0, 20), alpha=np.linspace(0.3, -0.2, 20), length_scale=0.02, sigma_f=0.7, ymean=0.0),
            dict(feat=5, out=5, Z=np.linspace(-2.2, -1.9, 20), alpha=np.linspace(-0.1, 0.2, 20), length_scale=0.03, sigma_f=1.2, ymean=-0.02)]


# distances (in length scales) from the nearest training point: exp(-d^2 / 2) is 2e-22 at 10, denormal for 37.7 < d < 38.6, and
# below the ldexp clamp of exp_nonpos (2^-1100) from 39.05
GP_TAIL_D = (10.0, 20.0, 30.0, 37.0, 37.8, 38.1, 38.4, 38.7, 39.2, 40.0)


def _gp_tail_states():
    rng = np.random.default_rng(12)
    rows = []
    for i, d in enumerate(GP_TAIL_D):
        for j in range(3):
            x = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-3, 3),
                          2.0 + 0.2 * d, -1.0 + 0.02 * GP_TAIL_D[(i + j) % len(GP_TAIL_D)], -1.9 + 0.03 * GP_TAIL_D[(i + 2 * j) % len(GP_TAIL_D)],
                          rng.uniform(-0.5, 0.5)])
            rows.append((x, np.array([rng.uniform(-10, 5), rng.uniform(-3, 3)]), (0.0, 0.3, 1.0)[j]))
    return rows


def _car_shoot(cfg, rows, oracles):
    import torch
    from ad_mpc_amd.engine import BatchSolver
    B = len(rows)
    xbar = np.zeros((B, 3, 7)); ubar = np.zeros((B, 2, 2)); p = np.zeros(B)
    for b, (x, u, pb) in enumerate(rows):
        xbar[b, :] = x; ubar[b, :] = u; p[b] = pb
    eng = BatchSolver(cfg, device=0)
    out = eng.shoot(eng.to_device(xbar), eng.to_device(ubar), eng.to_device(p))
    torch.cuda.synchronize()
    got = [t.cpu().numpy()[:, 0] for t in out]
    eng.close()
    ref = [[np.stack(v) for v in zip(*(o.rk4_sens(cfg, x, u, pb, cfg.Ts) for x, u, pb in rows))] for o in oracles]
    return got, ref[0], ref[1]


def test_car_shooting_at_the_edges(car_oracles):
    cfg = default_config(N=2)
    got, r64, r80 = _car_shoot(cfg, _car_edge_states(), car_oracles)
    for nm, a, b, c in zip(("phi", "A", "B"), got, r64, r80):
        _assert_shooting("car edges " + nm, a, b, c)


def test_car_shooting_in_the_gp_tails(car_oracles):
    cfg = default_config(N=2)
    set_gp(cfg, _far_gp())
    rows = _gp_tail_states()
    got, r64, r80 = _car_shoot(cfg, rows, car_oracles)
    for nm, a, b, c in zip(("phi", "A", "B"), got, r64, r80):
        _assert_shooting("car GP tails " + nm, a, b, c)
    # the GP terms are really evaluated: far from the training points every GP mean is its ymean
    nominal = default_config(N=2)
    x, u, pb = rows[0]
    f_gp = car_oracles[1].f(cfg, x, u, pb); f_nom = car_oracles[1].f(nominal, x, u, pb)
    assert abs((f_gp - f_nom)[3] - 0.01) < 1e-12 and abs((f_gp - f_nom)[5] + 0.02) < 1e-12


def test_quad_shooting_in_the_gp_tails(quad_oracles):
    """GP features 10 - 40 length scales from every training point in the quadrotor's residual (z = body-frame velocity), nodes with
    the integrated state and node 0 with its GP-state parameter (the initial state)."""
    import torch
    from ad_mpc_amd.engine import QuadBatchSolver
    cfg = default_quad_config()
    l = (0.1, 0.05, 0.08)
    gps = [dict(feat=7 + i, out=7 + i, Z=np.linspace(-3.0, -2.5, 15) + 0.1 * i, alpha=np.linspace(-0.3, 0.4, 15), length_scale=l[i],
                sigma_f=1.0, ymean=0.01 * (i + 1)) for i in range(3)]
    set_quad_gp(cfg, gps)
    rng = np.random.default_rng(13)
    N = cfg.N
    rows = []
    for i, d in enumerate(GP_TAIL_D):
        for j in range(2):
            x = np.zeros(QNX)
            x[0:3] = rng.uniform(-2, 2, 3); x[3] = 1.0                          # identity attitude: the body-frame velocity is v
            for c in range(3):
                dd = GP_TAIL_D[(i + j * (c + 1)) % len(GP_TAIL_D)]
                x[7 + c] = -2.5 + 0.1 * c + l[c] * dd
            x[10:13] = rng.uniform(-0.2, 0.2, 3)
            rows.append((x, rng.uniform(0.2, 0.8, QNU)))
    B = len(rows)
    xbar = np.stack([np.repeat(x[None], N + 1, axis=0) for x, _ in rows]); ubar = np.stack([np.repeat(u[None], N, axis=0) for _, u in rows])
    eng = QuadBatchSolver(cfg, device=0)
    d_ = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    out = eng.shoot(d_(xbar), d_(ubar))
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in out]
    eng.close()
    for k, tag in ((0, "node 0 (GP state)"), (1, "node 1")):
        got = [t[:, k] for t in out]
        refs = [[np.stack(v) for v in zip(*(o.rk4_sens(cfg, x, u, cfg.Ts, gpx=x if k == 0 else None) for x, u in rows))] for o in quad_oracles]
        for nm, a, b, c in zip(("phi", "A", "B"), got, refs[0], refs[1]):
            _assert_shooting("quad GP tails %s %s" % (tag, nm), a, b, c)
    nominal = default_quad_config()
    x, u = rows[0]
    fg = quad_oracles[1].f(cfg, x, u); fn = quad_oracles[1].f(nominal, x, u)
    np.testing.assert_allclose((fg - fn)[7:10], [0.01, 0.02, 0.03], atol=1e-12)
