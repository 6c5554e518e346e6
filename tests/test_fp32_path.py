"""The fp32 path on the device (admpc_solve_batch_f32: admpc_linearize_kernel<float>, admpc_rowqp_kernel<float>,
admpc_nlp_res_kernel<float>; admpc_shoot_batch_f32) against float yardsticks.

Shooting: the device's float rk4 against 80-bit rk4_sens evaluated at the float-rounded inputs; the bound per entry is SHOOT_FACTOR x
the float oracle's own error (liboracle_f32.so: the same model in float arithmetic) + 1e-13 * eps32 / eps64 * max(1, |ref|), the shape
of tests/test_accuracy_80bit.py:_assert_shooting.

Solve rows (tests/fp32_path.py:ROWS, 512 instances each): the device against the fp64 oracle at the tight stop levels and against the
float emulator (tests/emu) fed the device's own float linearisation.  BUDGET holds 4 x the EMULATOR's distance from the fp64 oracle on
the same batch, computed on the CPU with the float oracle's linearisation (tests/test_fp32_path_cpu.py recomputes it and fails when a
budget exceeds that); the emulator's and the device's measured values stand under each row.

GP models: admpc_solve_batch_f32 refuses them beyond N = ADMPC_F32_GP_MAX_N = 28.  The census behind the bound
(scripts/census_f32_gp.py; CPU, float emulator against the fp64 oracle, 2048 instances per horizon and GP; BAD: status 0 on both sides
and max |du| > 2.5e-3).  Emulator values, not device values:

    grid GP     N    20      22      24      26      27      28      29      30      32      36      40
      bad             0       0       0       0       0       0       1      11      31      74     128
      worst |du|  3.0e-4  2.7e-4  4.7e-4  1.3e-3  1.1e-3  2.2e-3  3.4e-3  5.3e-3  3.4e-2  2.0e-1     3.1
      worst |dx|  2.3e-3  8.9e-3  3.5e-2  1.2e-1  2.4e-1  3.1e-1  5.7e-1     1.0     3.4      62     600
    multi-feature GPs: no bad instance at any N = 20 .. 40, worst |du| 6.3e-4, worst |dx| 4.8e-4

The states of the grid-GP model are already 3e-1 off at N = 28 while the inputs are within the bound: the documented bound of the
float path is a bound on the inputs there (the fp64 oracle itself is 9e-7 from 80-bit arithmetic in |dx| on this model at N = 40).
"""
import math
import os

import numpy as np
import pytest

import batch_regimes as R
import fp32_path as F
from ad_mpc_amd.config import default_config, tight_ipm, set_gp

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
SHOOT_FACTOR = 8.0                                  # as tests/test_accuracy_80bit.py
SHOOT_FLOOR = 1e-13 * 2.0 ** 29                     # that file's floor scaled by eps32 / eps64: 5.4e-5
STEER_MARGIN = 2e-3                                 # tests/test_gpu_parity.py:test_fp32_config5_full_size

# name: ((|du| median, 99 %, max), (|dx| median, 99 %, max)) = 4 x the emulator's value on the CPU, rounded up to two digits
BUDGET = {
    # BUDGET-BEGIN (written by scripts/fp32_budget_table.py --write; device lines by --device-log)
    "N2": ((1.1e-06, 8.1e-06, 9.9e-06), (7.4e-06, 2.3e-05, 2.6e-05)),
    #   emulator (CPU): |du| 2.7e-07 / 2.0e-06 / 2.5e-06; |dx| 1.8e-06 / 5.7e-06 / 6.5e-06
    #   device (MI355X): |du| 2.9e-07 / 2.4e-06 / 3.9e-06; |dx| 1.8e-06 / 5.7e-06 / 6.5e-06
    "N3": ((1.1e-03, 2.3e-03, 2.7e-03), (1.6e-04, 4.5e-04, 5.0e-04)),
    #   emulator (CPU): |du| 2.7e-04 / 5.6e-04 / 6.6e-04; |dx| 4.0e-05 / 1.1e-04 / 1.2e-04
    #   device (MI355X): |du| 2.7e-04 / 5.6e-04 / 6.6e-04; |dx| 4.0e-05 / 1.1e-04 / 1.2e-04
    "N7": ((6.9e-06, 1.5e-03, 1.9e-03), (2.9e-05, 1.1e-03, 1.8e-03)),
    #   emulator (CPU): |du| 1.7e-06 / 3.7e-04 / 4.6e-04; |dx| 7.1e-06 / 2.6e-04 / 4.5e-04
    #   device (MI355X): |du| 1.8e-06 / 3.7e-04 / 4.6e-04; |dx| 7.1e-06 / 2.6e-04 / 4.5e-04
    "N13": ((2.6e-05, 1.7e-03, 2.4e-03), (3.8e-05, 1.4e-03, 1.9e-03)),
    #   emulator (CPU): |du| 6.5e-06 / 4.2e-04 / 5.8e-04; |dx| 9.4e-06 / 3.4e-04 / 4.6e-04
    #   device (MI355X): |du| 6.4e-06 / 4.2e-04 / 5.8e-04; |dx| 9.3e-06 / 3.3e-04 / 4.6e-04
    "N19": ((5.3e-05, 3.2e-04, 2.0e-03), (4.3e-05, 1.3e-04, 1.4e-04)),
    #   emulator (CPU): |du| 1.3e-05 / 7.8e-05 / 4.8e-04; |dx| 1.1e-05 / 3.1e-05 / 3.4e-05
    #   device (MI355X): |du| 1.3e-05 / 7.4e-05 / 4.8e-04; |dx| 1.1e-05 / 3.1e-05 / 3.4e-05
    "N21": ((6.5e-05, 3.5e-04, 3.8e-04), (4.7e-05, 1.3e-04, 1.5e-04)),
    #   emulator (CPU): |du| 1.6e-05 / 8.6e-05 / 9.5e-05; |dx| 1.2e-05 / 3.2e-05 / 3.6e-05
    #   device (MI355X): |du| 1.5e-05 / 8.0e-05 / 1.0e-04; |dx| 1.2e-05 / 3.2e-05 / 3.6e-05
    "N33": ((1.3e-04, 6.2e-04, 1.9e-03), (5.7e-05, 1.9e-04, 3.6e-04)),
    #   emulator (CPU): |du| 3.2e-05 / 1.5e-04 / 4.6e-04; |dx| 1.4e-05 / 4.7e-05 / 8.9e-05
    #   device (MI355X): |du| 3.0e-05 / 1.5e-04 / 4.6e-04; |dx| 1.4e-05 / 4.8e-05 / 8.5e-05
    "N40": ((1.4e-04, 6.7e-04, 1.4e-03), (5.9e-05, 2.0e-04, 4.2e-04)),
    #   emulator (CPU): |du| 3.3e-05 / 1.7e-04 / 3.3e-04; |dx| 1.5e-05 / 5.0e-05 / 1.0e-04
    #   device (MI355X): |du| 3.1e-05 / 2.2e-04 / 3.3e-04; |dx| 1.5e-05 / 5.1e-05 / 1.0e-04
    "N64": ((1.4e-04, 6.4e-04, 1.4e-03), (6.9e-05, 2.6e-04, 5.0e-04)),
    #   emulator (CPU): |du| 3.3e-05 / 1.6e-04 / 3.5e-04; |dx| 1.7e-05 / 6.3e-05 / 1.2e-04
    #   device (MI355X): |du| 3.1e-05 / 1.6e-04 / 3.4e-04; |dx| 1.7e-05 / 6.6e-05 / 1.3e-04
    "N65": ((1.4e-04, 7.4e-04, 1.4e-03), (7.1e-05, 2.9e-04, 5.0e-04)),
    #   emulator (CPU): |du| 3.3e-05 / 1.8e-04 / 3.4e-04; |dx| 1.8e-05 / 7.2e-05 / 1.2e-04
    #   device (MI355X): |du| 3.2e-05 / 1.8e-04 / 3.4e-04; |dx| 1.8e-05 / 6.7e-05 / 1.3e-04
    "N97": ((1.6e-04, 9.1e-04, 2.1e-03), (1.2e-04, 4.9e-04, 6.2e-04)),
    #   emulator (CPU): |du| 3.8e-05 / 2.3e-04 / 5.1e-04; |dx| 2.8e-05 / 1.2e-04 / 1.5e-04
    #   device (MI355X): |du| 3.7e-05 / 2.3e-04 / 5.1e-04; |dx| 2.8e-05 / 1.2e-04 / 1.5e-04
    "N128": ((1.9e-04, 1.1e-03, 1.5e-03), (1.8e-04, 1.1e-03, 1.2e-03)),
    #   emulator (CPU): |du| 4.6e-05 / 2.5e-04 / 3.6e-04; |dx| 4.4e-05 / 2.6e-04 / 2.8e-04
    #   device (MI355X): |du| 4.5e-05 / 2.4e-04 / 3.6e-04; |dx| 4.2e-05 / 2.1e-04 / 3.1e-04
    "N40_kinematic": ((1.2e-04, 6.3e-04, 4.5e-03), (5.2e-05, 2.2e-04, 8.3e-04)),
    #   emulator (CPU): |du| 3.0e-05 / 1.6e-04 / 1.1e-03; |dx| 1.3e-05 / 5.5e-05 / 2.1e-04
    #   device (MI355X): |du| 2.9e-05 / 1.6e-04 / 1.1e-03; |dx| 1.3e-05 / 5.5e-05 / 2.1e-04
    "q7_N20_d0": ((9.0e-05, 8.9e-04, 2.0e-03), (3.4e-05, 1.8e-04, 5.7e-04)),
    #   emulator (CPU): |du| 2.2e-05 / 2.2e-04 / 4.8e-04; |dx| 8.3e-06 / 4.3e-05 / 1.4e-04
    #   device (MI355X): |du| 2.2e-05 / 2.1e-04 / 4.8e-04; |dx| 8.2e-06 / 4.3e-05 / 1.4e-04
    "q7_N20_d1": ((2.1e-04, 1.4e-03, 2.1e-03), (5.4e-05, 1.6e-04, 1.7e-04)),
    #   emulator (CPU): |du| 5.2e-05 / 3.3e-04 / 5.2e-04; |dx| 1.3e-05 / 3.8e-05 / 4.0e-05
    #   device (MI355X): |du| 4.7e-05 / 3.2e-04 / 4.1e-04; |dx| 1.3e-05 / 3.8e-05 / 4.0e-05
    "q7_N40_d0": ((1.5e-04, 1.1e-03, 1.4e-03), (6.5e-05, 2.3e-04, 4.0e-04)),
    #   emulator (CPU): |du| 3.7e-05 / 2.7e-04 / 3.3e-04; |dx| 1.6e-05 / 5.6e-05 / 9.8e-05
    #   device (MI355X): |du| 3.4e-05 / 2.3e-04 / 3.2e-04; |dx| 1.6e-05 / 5.8e-05 / 9.8e-05
    "q7_N40_d1": ((1.8e-04, 6.7e-04, 9.8e-04), (1.2e-04, 3.0e-04, 3.4e-04)),
    #   emulator (CPU): |du| 4.3e-05 / 1.7e-04 / 2.4e-04; |dx| 2.8e-05 / 7.4e-05 / 8.4e-05
    #   device (MI355X): |du| 4.0e-05 / 1.7e-04 / 2.3e-04; |dx| 2.8e-05 / 7.8e-05 / 8.6e-05
    "q7_N80_d0": ((8.0e-05, 9.8e-04, 1.9e-03), (1.2e-04, 6.0e-04, 9.0e-04)),
    #   emulator (CPU): |du| 2.0e-05 / 2.4e-04 / 4.6e-04; |dx| 3.0e-05 / 1.5e-04 / 2.2e-04
    #   device (MI355X): |du| 2.0e-05 / 2.7e-04 / 8.2e-04; |dx| 3.0e-05 / 1.3e-04 / 1.8e-04
    "q7_N80_d1": ((7.0e-05, 2.9e-04, 6.5e-04), (2.6e-04, 7.8e-04, 9.6e-04)),
    #   emulator (CPU): |du| 1.7e-05 / 7.1e-05 / 1.6e-04; |dx| 6.3e-05 / 1.9e-04 / 2.4e-04
    #   device (MI355X): |du| 1.8e-05 / 7.3e-05 / 1.6e-04; |dx| 6.3e-05 / 2.0e-04 / 2.9e-04
    "q127_N20": ((6.1e-05, 3.2e-04, 6.3e-04), (4.5e-05, 1.3e-04, 1.5e-04)),
    #   emulator (CPU): |du| 1.5e-05 / 7.9e-05 / 1.6e-04; |dx| 1.1e-05 / 3.1e-05 / 3.7e-05
    #   device (MI355X): |du| 1.5e-05 / 7.3e-05 / 1.6e-04; |dx| 1.1e-05 / 3.1e-05 / 3.7e-05
    "q127_N24": ((8.7e-05, 3.9e-04, 9.9e-04), (4.7e-05, 1.4e-04, 1.7e-04)),
    #   emulator (CPU): |du| 2.2e-05 / 9.6e-05 / 2.5e-04; |dx| 1.2e-05 / 3.4e-05 / 4.1e-05
    #   device (MI355X): |du| 2.1e-05 / 9.2e-05 / 2.5e-04; |dx| 1.2e-05 / 3.3e-05 / 4.1e-05
    "gp_grid_N2": ((1.2e-06, 8.3e-06, 1.3e-05), (7.4e-06, 2.4e-05, 2.7e-05)),
    #   emulator (CPU): |du| 2.9e-07 / 2.1e-06 / 3.0e-06; |dx| 1.8e-06 / 6.0e-06 / 6.6e-06
    #   device (MI355X): |du| 3.3e-07 / 2.0e-06 / 3.2e-06; |dx| 1.8e-06 / 5.9e-06 / 6.5e-06
    "gp_grid_N3": ((3.1e-04, 2.0e-03, 2.2e-03), (8.0e-05, 1.1e-03, 1.6e-03)),
    #   emulator (CPU): |du| 7.6e-05 / 4.8e-04 / 5.5e-04; |dx| 2.0e-05 / 2.5e-04 / 3.8e-04
    #   device (MI355X): |du| 7.6e-05 / 4.8e-04 / 5.5e-04; |dx| 2.0e-05 / 2.5e-04 / 3.8e-04
    "gp_grid_N7": ((1.5e-05, 1.5e-03, 1.9e-03), (3.6e-05, 1.1e-03, 2.5e-03)),
    #   emulator (CPU): |du| 3.7e-06 / 3.6e-04 / 4.6e-04; |dx| 8.9e-06 / 2.7e-04 / 6.2e-04
    #   device (MI355X): |du| 3.5e-06 / 3.6e-04 / 4.6e-04; |dx| 8.6e-06 / 2.7e-04 / 6.3e-04
    "gp_grid_N13": ((5.3e-05, 1.6e-03, 1.9e-03), (6.3e-05, 1.6e-03, 3.9e-03)),
    #   emulator (CPU): |du| 1.3e-05 / 3.9e-04 / 4.5e-04; |dx| 1.6e-05 / 4.0e-04 / 9.5e-04
    #   device (MI355X): |du| 1.3e-05 / 3.9e-04 / 4.5e-04; |dx| 1.5e-05 / 3.9e-04 / 9.2e-04
    "gp_grid_N19": ((5.8e-05, 2.8e-04, 6.0e-04), (6.3e-05, 3.8e-03, 5.2e-03)),
    #   emulator (CPU): |du| 1.4e-05 / 7.0e-05 / 1.5e-04; |dx| 1.6e-05 / 9.4e-04 / 1.3e-03
    #   device (MI355X): |du| 1.4e-05 / 7.2e-05 / 1.5e-04; |dx| 1.6e-05 / 9.1e-04 / 1.5e-03
    "gp_grid_N20": ((6.5e-05, 3.5e-04, 4.6e-04), (6.5e-05, 6.3e-03, 1.3e-02)),
    #   emulator (CPU): |du| 1.6e-05 / 8.6e-05 / 1.1e-04; |dx| 1.6e-05 / 1.6e-03 / 3.2e-03
    #   device (MI355X): |du| 1.6e-05 / 7.7e-05 / 1.1e-04; |dx| 1.6e-05 / 1.2e-03 / 2.5e-03
    "gp_grid_N21": ((7.2e-05, 3.3e-04, 5.4e-04), (6.7e-05, 9.6e-03, 2.3e-02)),
    #   emulator (CPU): |du| 1.8e-05 / 8.1e-05 / 1.3e-04; |dx| 1.7e-05 / 2.4e-03 / 5.6e-03
    #   device (MI355X): |du| 1.7e-05 / 8.2e-05 / 1.3e-04; |dx| 1.7e-05 / 2.5e-03 / 3.2e-03
    "gp_grid_N24": ((1.1e-04, 4.7e-04, 1.7e-03), (7.7e-05, 5.5e-02, 1.1e-01)),
    #   emulator (CPU): |du| 2.5e-05 / 1.2e-04 / 4.1e-04; |dx| 1.9e-05 / 1.4e-02 / 2.6e-02
    #   device (MI355X): |du| 2.5e-05 / 1.2e-04 / 4.6e-04; |dx| 1.9e-05 / 1.2e-02 / 2.6e-02
    "gp_grid_N28": ((1.3e-04, 3.0e-03, 4.7e-03), (8.4e-05, 6.6e-01, 1.3e+00)),
    #   emulator (CPU): |du| 3.2e-05 / 7.5e-04 / 1.2e-03; |dx| 2.1e-05 / 1.6e-01 / 3.0e-01
    #   device (MI355X): |du| 3.1e-05 / 7.7e-04 / 1.7e-03; |dx| 2.1e-05 / 1.4e-01 / 5.8e-01
    "gp_multi_N2": ((1.3e-06, 1.2e-05, 1.7e-04), (7.7e-06, 2.4e-05, 2.8e-05)),
    #   emulator (CPU): |du| 3.1e-07 / 2.8e-06 / 4.2e-05; |dx| 1.9e-06 / 5.9e-06 / 6.9e-06
    #   device (MI355X): |du| 3.0e-07 / 2.3e-06 / 4.2e-05; |dx| 1.9e-06 / 6.0e-06 / 6.9e-06
    "gp_multi_N3": ((1.2e-03, 2.3e-03, 2.8e-03), (1.6e-04, 4.6e-04, 5.3e-04)),
    #   emulator (CPU): |du| 2.8e-04 / 5.6e-04 / 6.8e-04; |dx| 3.9e-05 / 1.1e-04 / 1.3e-04
    #   device (MI355X): |du| 2.8e-04 / 5.6e-04 / 6.8e-04; |dx| 3.9e-05 / 1.1e-04 / 1.3e-04
    "gp_multi_N7": ((7.2e-06, 1.7e-03, 2.5e-03), (2.8e-05, 1.3e-03, 2.2e-03)),
    #   emulator (CPU): |du| 1.8e-06 / 4.0e-04 / 6.1e-04; |dx| 6.8e-06 / 3.2e-04 / 5.3e-04
    #   device (MI355X): |du| 1.8e-06 / 4.0e-04 / 6.1e-04; |dx| 6.8e-06 / 3.2e-04 / 5.3e-04
    "gp_multi_N13": ((2.9e-05, 1.8e-03, 2.5e-03), (4.5e-05, 1.4e-03, 2.8e-03)),
    #   emulator (CPU): |du| 7.2e-06 / 4.4e-04 / 6.2e-04; |dx| 1.1e-05 / 3.3e-04 / 6.9e-04
    #   device (MI355X): |du| 7.4e-06 / 4.4e-04 / 6.2e-04; |dx| 1.1e-05 / 3.3e-04 / 6.8e-04
    "gp_multi_N19": ((6.2e-05, 2.7e-04, 3.7e-04), (4.7e-05, 1.3e-04, 1.4e-04)),
    #   emulator (CPU): |du| 1.5e-05 / 6.7e-05 / 9.2e-05; |dx| 1.2e-05 / 3.1e-05 / 3.3e-05
    #   device (MI355X): |du| 1.5e-05 / 7.0e-05 / 9.2e-05; |dx| 1.2e-05 / 3.1e-05 / 3.3e-05
    "gp_multi_N20": ((7.0e-05, 3.0e-04, 4.3e-04), (4.8e-05, 1.4e-04, 1.5e-04)),
    #   emulator (CPU): |du| 1.7e-05 / 7.5e-05 / 1.1e-04; |dx| 1.2e-05 / 3.3e-05 / 3.6e-05
    #   device (MI355X): |du| 1.7e-05 / 7.6e-05 / 1.0e-04; |dx| 1.2e-05 / 3.2e-05 / 3.4e-05
    "gp_multi_N21": ((7.7e-05, 3.2e-04, 4.2e-04), (4.9e-05, 1.4e-04, 1.5e-04)),
    #   emulator (CPU): |du| 1.9e-05 / 7.9e-05 / 1.0e-04; |dx| 1.2e-05 / 3.5e-05 / 3.7e-05
    #   device (MI355X): |du| 1.9e-05 / 8.2e-05 / 1.0e-04; |dx| 1.2e-05 / 3.4e-05 / 3.7e-05
    "gp_multi_N28": ((1.3e-04, 6.2e-04, 1.7e-03), (5.8e-05, 1.8e-04, 2.2e-04)),
    #   emulator (CPU): |du| 3.0e-05 / 1.5e-04 / 4.0e-04; |dx| 1.4e-05 / 4.5e-05 / 5.3e-05
    #   device (MI355X): |du| 3.1e-05 / 1.6e-04 / 4.0e-04; |dx| 1.4e-05 / 4.5e-05 / 5.2e-05
    "sqp3_N20": ((1.6e-05, 1.6e-04, 5.3e-04), (1.8e-05, 4.4e-05, 5.2e-05)),
    #   emulator (CPU): |du| 3.9e-06 / 4.0e-05 / 1.3e-04; |dx| 4.3e-06 / 1.1e-05 / 1.3e-05
    #   device (MI355X): |du| 3.8e-06 / 3.0e-05 / 1.3e-04; |dx| 4.3e-06 / 1.1e-05 / 1.2e-05
    "sqp_tol_N20": ((2.3e-03, 4.3e-02, 6.8e-02), (2.2e-03, 2.3e-02, 3.8e-02)),
    #   emulator (CPU): |du| 5.6e-04 / 1.1e-02 / 1.7e-02; |dx| 5.4e-04 / 5.6e-03 / 9.3e-03
    #   device (MI355X): |du| 5.6e-04 / 1.1e-02 / 1.7e-02; |dx| 5.4e-04 / 5.6e-03 / 9.3e-03
    "sqp_tol_N40": ((8.4e-04, 2.0e-02, 6.7e-02), (6.2e-04, 9.5e-03, 2.7e-02)),
    #   emulator (CPU): |du| 2.1e-04 / 4.8e-03 / 1.7e-02; |dx| 1.5e-04 / 2.4e-03 / 6.6e-03
    #   device (MI355X): |du| 2.1e-04 / 4.8e-03 / 1.7e-02; |dx| 1.5e-04 / 2.4e-03 / 6.6e-03
    # BUDGET-END
}
# rows whose device value exceeds its budget, with the reason (none allowed without one)
KNOWN_WEAK = {}


@pytest.fixture(scope="module")
def oracles():
    from oracle.oracle import Oracle
    return Oracle(omp=True), Oracle(variant="ld"), Oracle(variant="f32")


@pytest.fixture(scope="module")
def emu():
    from emu.emu import Emu
    return Emu()


@pytest.fixture(scope="module")
def nc():
    return R.num_cu()


def _engine(cfg):
    from ad_mpc_amd.engine import BatchSolver
    return BatchSolver(cfg, device=0)


def _solve32(eng, a):
    return eng.solve_numpy(*(a[k] for k in F.ARGS), dtype=np.float32)


def _bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if len(a) == 0:
        return
    same = (a.view(np.uint8) == b.view(np.uint8)).reshape(len(a), -1).all(axis=1)
    assert same.all(), "%s: %d instances differ in bits, first %s" % (what, (~same).sum(), np.nonzero(~same)[0][:8])


def _device_lineariser(eng):
    import torch
    from emu.emu import pack_shooting

    def lin(x, u, p):
        out = eng.shoot(*(eng.to_device(v, torch.float32) for v in (x, u, p)))
        torch.cuda.synchronize()
        return pack_shooting(*(t.cpu().numpy() for t in out), x)
    return lin


# ---------------------------------------------------------------------------------------------------------------------------------
# shooting

def _shoot32(cfg, rows, oracles):
    """Device float shooting of (x, u, p) rows and the float / 80-bit oracles at the float-rounded inputs."""
    import torch
    B = len(rows)
    xbar = np.zeros((B, 3, 7), dtype=np.float32); ubar = np.zeros((B, 2, 2), dtype=np.float32); p = np.zeros(B, dtype=np.float32)
    for b, (x, u, pb) in enumerate(rows):
        xbar[b, :] = x; ubar[b, :] = u; p[b] = pb
    eng = _engine(cfg)
    out = eng.shoot(*(eng.to_device(v, torch.float32) for v in (xbar, ubar, p)))
    torch.cuda.synchronize()
    got = [t.cpu().numpy()[:, 0].astype(np.float64) for t in out]
    eng.close()
    d = lambda v: np.asarray(v, dtype=np.float64)
    ref = [[np.stack(v) for v in zip(*(o.rk4_sens(cfg, d(xbar[b, 0]), d(ubar[b, 0]), float(p[b]), cfg.Ts) for b in range(B)))]
           for o in (oracles[2], oracles[1])]
    return got, ref[0], ref[1]


def _assert_shooting32(tag, got, ref32, ref80):
    err = np.abs(got - ref80); err32 = np.abs(ref32 - ref80)
    lim = SHOOT_FACTOR * err32 + SHOOT_FLOOR * np.maximum(1.0, np.abs(ref80))
    worst = np.unravel_index(np.argmax(err / lim), err.shape)
    print("SHOOT32 %-26s max device err %.1e  float oracle err %.1e  worst ratio to the bound %.3f" % (tag, err.max(), err32.max(), (err / lim).max()))
    assert np.isfinite(got).all(), tag
    assert (err <= lim).all(), (tag, worst, got[worst], ref80[worst], ref32[worst])


def _edge_states32():
    """test_accuracy_80bit.py:_car_edge_states with psi at k pi / 4 and 1..3 FLOAT ulps either side."""
    from test_accuracy_80bit import _car_edge_states, YAW_K
    psis = []
    for k in range(-8, 9):
        c = np.float32(k * math.pi / 4)
        psis.append(c)
        lo = hi = c
        for _ in range(3):
            lo = np.nextafter(lo, np.float32(-np.inf)); hi = np.nextafter(hi, np.float32(np.inf))
            psis += [lo, hi]
    for K in YAW_K:
        for th in (-2.5, -0.7, 0.0, 0.4, 1.9, math.pi / 4, -math.pi / 2):
            psis.append(np.float32(th + 2 * math.pi * K))
    rows = _car_edge_states()
    assert len(rows) == len(psis)
    out = []
    for (x, u, p), psi in zip(rows, psis):
        x = x.copy(); x[2] = float(psi)
        out.append((x, u, p))
    return out


# distances (in length scales) from the nearest training point, chosen for expf: exp(-d^2 / 2) is normal below 13.2, falls from FLT_MIN
# to the smallest denormal for 13.2 < d < 14.4, and is 0 beyond
GP_TAIL_D32 = (2.0, 5.0, 10.0, 13.0, 13.3, 13.6, 13.9, 14.2, 14.6, 16.0, 20.0)


def _gp_tail_states32():
    rng = np.random.default_rng(12)
    D = GP_TAIL_D32
    rows = []
    for i, d in enumerate(D):
        for j in range(3):
            x = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-3, 3),
                          2.0 + 0.2 * d, -1.0 + 0.02 * D[(i + j) % len(D)], -1.9 + 0.03 * D[(i + 2 * j) % len(D)], rng.uniform(-0.5, 0.5)])
            rows.append((x, np.array([rng.uniform(-10, 5), rng.uniform(-3, 3)]), (0.0, 0.3, 1.0)[j]))
    return rows


def test_float_shooting_at_the_edges(oracles):
    got, r32, r80 = _shoot32(default_config(N=2), _edge_states32(), oracles)
    for nm, a, b, c in zip(("phi", "A", "B"), got, r32, r80):
        _assert_shooting32("car edges " + nm, a, b, c)


def test_float_shooting_in_the_gp_tails(oracles):
    from test_accuracy_80bit import _far_gp
    cfg = set_gp(default_config(N=2), _far_gp())
    got, r32, r80 = _shoot32(cfg, _gp_tail_states32(), oracles)
    for nm, a, b, c in zip(("phi", "A", "B"), got, r32, r80):
        _assert_shooting32("car GP tails " + nm, a, b, c)


def test_float_shooting_on_the_golden_vectors(oracles, golden_shooting):
    cases = golden_shooting["cases"]
    assert len(cases) == 120
    cfg = default_config(N=2, Ts=cases[0]["h"])
    rows = [(np.array(c["x"]), np.array(c["u"]), c["p"]) for c in cases]
    got, r32, r80 = _shoot32(cfg, rows, oracles)
    for nm, a, b, c in zip(("phi", "A", "B"), got, r32, r80):
        _assert_shooting32("golden vectors " + nm, a, b, c)
    # the 80-bit oracle at the rounded inputs is the golden vector to the rounding of the inputs
    phi = np.array([c["phi"] for c in cases])
    assert np.abs(r80[0] - phi).max() <= 64 * EPS32 * np.abs(phi).max()


def test_kinematic_branch_is_exact_at_p_zero():
    """p == 0: the float model drops the dynamic terms (model_dev.h), so a config with other tyre / inertia parameters gives the same
    bits -- also at v_x = 0, where the dynamic branch would be inf * 0."""
    import torch
    rows = [(x, u, 0.0) for x, u, _ in _edge_states32()[:60]]
    for i in range(0, 60, 5):
        rows[i][0][3] = 0.0
    B = len(rows)
    xbar = np.zeros((B, 3, 7), dtype=np.float32); ubar = np.zeros((B, 2, 2), dtype=np.float32); p = np.zeros(B, dtype=np.float32)
    for b, (x, u, pb) in enumerate(rows):
        xbar[b, :] = x; ubar[b, :] = u
    outs = []
    for scale in (1.0, 1.37):
        cfg = default_config(N=2)
        cfg.Cf *= scale; cfg.Cr /= scale; cfg.mass *= scale; cfg.Iz /= scale
        eng = _engine(cfg)
        out = eng.shoot(*(eng.to_device(v, torch.float32) for v in (xbar, ubar, p)))
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in out])
        eng.close()
    for a, b, nm in zip(outs[0], outs[1], ("phi", "A", "B")):
        assert np.isfinite(a).all(), nm
        _bits(a, b, "kinematic branch at p = 0: " + nm)
    # and the parameters do matter as soon as p > 0
    p[:] = 0.3
    cfg = default_config(N=2); eng = _engine(cfg)
    blended = eng.shoot(*(eng.to_device(v, torch.float32) for v in (xbar, ubar, p)))[0].cpu().numpy()
    eng.close()
    keep = xbar[:, 0, 3] != 0
    assert (blended[keep] != outs[0][0][keep]).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# solve rows

def _check_budget(name, what, got, budget, emu_here=None):
    (mu, mx), (bu, bx) = got, budget
    print("F32 %-14s %-8s |du| %.1e / %.1e / %.1e  |dx| %.1e / %.1e / %.1e" % ((name, what) + mu + mx))
    if name in KNOWN_WEAK:
        return
    for lbl, g, l in (("du", mu, bu), ("dx", mx, bx)):
        for stat, v, lim in zip(("median", "99%", "max"), g, l):
            assert v <= lim, "%s: %s |%s| %s %.3e above the budget %.2e" % (name, what, lbl, stat, v, lim)


@pytest.mark.parametrize("name", list(F.ROWS))
def test_solve_row(name, oracles, emu):
    cfg, s = F.row(name)
    N = cfg.N
    o = F.oracle_solve(oracles[0], cfg, s, nthreads=16)
    a = F.args32(s)
    eng = _engine(cfg)
    g = _solve32(eng, a)
    for x, y, nm in zip(g, _solve32(eng, a), ("x", "u", "cost", "status", "iters")):
        _bits(x, y, "second call: " + nm)
    F.batch_conditions(o, g, cfg)                                   # statuses as the oracle's; nobody left out but the oracle's failures
    ok = o[3] == 0
    # x_0 is the measured state on every solved instance; a failed instance keeps its iterate bit for bit
    _bits(g[0][:, 0, :], np.where(ok[:, None], a["x0"], a["xbar"][:, 0, :]), "x_0")
    _bits(g[0][~ok], a["xbar"][~ok], "iterate of a failed instance"); _bits(g[1][~ok], a["ubar"][~ok], "inputs of a failed instance")
    d = g[0][ok][:, 1:N, 6]                                          # the hard box holds on stages 1 .. N - 1, at N = 2 on stage 1
    assert d.min() >= cfg.lbx_delta - STEER_MARGIN and d.max() <= cfg.ubx_delta + STEER_MARGIN, (d.min(), d.max())
    assert name in BUDGET, "no budget for " + name
    got = F.stats(g, o)
    _check_budget(name, "device", got, BUDGET[name])
    if name in F.SHIPPED:
        assert got[0][2] <= F.F32_BOUND, (name, got[0][2])
    # the float emulator on the device's own linearisation: the same algorithm from the same numbers
    e = F.emu_passes(emu, cfg, s, _device_lineariser(eng))
    eng.close()
    np.testing.assert_array_equal(e[3], g[3])
    _check_budget(name, "emulator", F.stats(e, o), BUDGET[name])
    apart = F.stats(g, (e[0].astype(np.float64), e[1].astype(np.float64), None, o[3]))
    print("F32 %-14s dev-emu  |du| %.1e / %.1e / %.1e  |dx| %.1e / %.1e / %.1e  same iteration counts %.3f"
          % ((name,) + apart[0] + apart[1] + ((e[4] == g[4])[ok].mean(),)))
    assert apart[0][0] <= BUDGET[name][0][0] and apart[1][0] <= BUDGET[name][1][0], (name, apart)     # medians: one distribution


def test_budgets_cover_every_row():
    assert set(BUDGET) == set(F.ROWS) | {"sqp_tol_N20", "sqp_tol_N40"}
    assert set(KNOWN_WEAK) <= set(BUDGET) and all(KNOWN_WEAK.values())


@pytest.mark.parametrize("gp", ["grid", "multi"])
def test_gp_models_beyond_the_bound_are_refused(gp):
    """ADMPC_F32_GP_MAX_N: the float solve of a GP model at N = 29 and 40 is an error (ADMPC_EINVAL) that writes nothing -- iterate,
    cost, status and iteration counts keep their bits; the fp64 entry of the same handle still solves, and the same horizons without
    GPs run in float."""
    import torch
    from ad_mpc_amd import _lib
    from ad_mpc_amd.scenarios import random_scenarios
    for N in (F.GP_MAX_N + 1, 40):
        cfg = set_gp(default_config(N=N), F.gp_model(gp))
        s = random_scenarios(32, N=N, seed=5)
        a = F.args32(s)
        eng = _engine(cfg)
        t = {k: eng.to_device(a[k], torch.float32) for k in F.ARGS}
        cost = torch.full((32,), 7.0, dtype=torch.float32, device=eng.device)
        st = torch.full((32,), -9, dtype=torch.int32, device=eng.device); it = torch.full_like(st, -9)
        with pytest.raises(_lib.AdmpcError, match="ADMPC_F32_GP_MAX_N"):
            eng.solve(*(t[k] for k in F.ARGS), cost, st, it)
        torch.cuda.synchronize()
        _bits(t["xbar"].cpu().numpy(), a["xbar"], "iterate after the refusal"); _bits(t["ubar"].cpu().numpy(), a["ubar"], "inputs after the refusal")
        assert (cost.cpu().numpy() == 7.0).all() and (st.cpu().numpy() == -9).all() and (it.cpu().numpy() == -9).all()
        g = eng.solve_numpy(*(s[k] for k in F.ARGS))
        assert (g[3] == 0).all()
        eng.close()
        plain = _engine(default_config(N=N))
        assert (_solve32(plain, a)[3] == 0).all()
        plain.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# SQP with a tolerance: admpc_nlp_res_kernel<float>

@pytest.mark.parametrize("N", [20, 40])
def test_sqp_with_a_tolerance(N, oracles):
    """sqp_iters = 20, sqp_tol = 1e-6 on a batch where the fp64 oracle's SQP converges within 10 passes: every instance converges
    (status 0); its iterate is bit for bit the iterate of a fixed-pass run of k < 20 passes (the stopping test only skips); k differs
    between instances; the shooting defects of the returned iterate are within the floored tol_eq; the iterate is within budget of the
    fp64 oracle's converged solution; with sqp_iters = 2 exactly the instances with k > 1 report status 2."""
    s, ref = F.sqp_tol_batch(oracles[0], N, nthreads=16)
    a = F.args32(s)
    B = len(a["x0"])

    def run(iters, tol):
        eng = _engine(tight_ipm(default_config(N=N, sqp_iters=iters, sqp_tol=tol)))
        g = _solve32(eng, a)
        eng.close()
        return g
    g = run(20, F.SQP_TOL)
    assert (g[3] == 0).all(), np.bincount(g[3])
    k_of = np.zeros(B, dtype=np.int32)
    for k in range(1, 20):
        f = run(k, 0.0)
        same = (f[0].view(np.uint32) == g[0].view(np.uint32)).all(axis=(1, 2)) & (f[1].view(np.uint32) == g[1].view(np.uint32)).all(axis=(1, 2))
        k_of[(k_of == 0) & same] = k
        if (k_of > 0).all():
            break
    print("SQP32 N %d passes per instance: %s" % (N, np.bincount(k_of)))
    assert (k_of > 0).all(), "%d instances equal no fixed-pass iterate" % (k_of == 0).sum()
    assert len(np.unique(k_of)) > 1
    cfg = default_config(N=N)
    x, u = g[0].astype(np.float64), g[1].astype(np.float64)
    worst = 0.0
    for b in range(B):
        for k in range(N):
            phi = oracles[0].rk4_sens(cfg, x[b, k], u[b, k], float(a["p"][b]), cfg.Ts)[0]
            lim = F.SQP_FLOORS[1] + EPS32 * np.maximum(np.abs(phi), np.abs(x[b, k + 1]))
            worst = max(worst, float((np.abs(phi - x[b, k + 1]) / lim).max()))
    print("SQP32 N %d worst defect / (tol_eq + |x| eps32): %.3f" % (N, worst))
    assert worst <= 1.0
    _check_budget("sqp_tol_N%d" % N, "device", F.stats(g, ref), BUDGET["sqp_tol_N%d" % N])
    two = run(2, F.SQP_TOL)
    np.testing.assert_array_equal(two[3], np.where(k_of > 1, 2, 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# failures

@pytest.mark.parametrize("passes,B", [(1, 301), (2, 77), (3, 1023)])
def test_nonfinite_instances_fail_alone(passes, B):
    """NaN / inf in x0 or yref at scattered instances: status 4, cost +inf, iterate untouched bit for bit; every other instance has the
    bits of the clean batch."""
    from ad_mpc_amd.scenarios import random_scenarios
    N = 20
    cfg = default_config(N=N, sqp_iters=passes)
    a = F.args32(random_scenarios(B, N=N, seed=60 + passes, blend=(3.0, 5.0)))
    eng = _engine(cfg)
    clean = _solve32(eng, a)
    assert (clean[3] == 0).all()
    rng = np.random.default_rng(passes)
    bad = np.unique(np.r_[0, B - 1, rng.integers(0, B, 9)])
    dirty = {k: v.copy() for k, v in a.items()}
    for i, b in enumerate(bad):
        v = (np.nan, np.inf, -np.inf)[i % 3]
        if i % 2 == 0:
            dirty["x0"][b, i % 7] = v
        else:
            dirty["yref"][b, (3 * i) % N, i % 9] = v
    g = _solve32(eng, dirty)
    eng.close()
    assert (g[3][bad] == 4).all() and np.isposinf(g[2][bad]).all(), (g[3][bad], g[2][bad])
    _bits(g[0][bad], a["xbar"][bad], "iterate of a failed instance"); _bits(g[1][bad], a["ubar"][bad], "inputs of a failed instance")
    keep = np.ones(B, dtype=bool); keep[bad] = False
    for x, y, nm in zip(g, clean, ("x", "u", "cost", "status", "iters")):
        _bits(x[keep], y[keep], "neighbours of the failed instances: " + nm)


# ---------------------------------------------------------------------------------------------------------------------------------
# regimes of the row kernel's launch plan

@pytest.mark.parametrize("side", ["rows1", "rows2", "rows4", "split"])
def test_row_count_and_split_switches(nc, side):
    """admpc_rowqp_plan maps 1, 2 or 4 instances to a wave depending on the batch, and past one round of waves the batch is split into
    two phases: the float solve on each side, bit-identical to the same instances in sub-batches of one instance per wave and to a
    permuted batch."""
    from ad_mpc_amd.scenarios import random_scenarios
    from test_batch_regimes import _composition_free
    N = 20
    B = R.rowqp_sizes(nc)[side]
    assert R.rowqp_lds_rows(N, 4) == 4 and R.rowqp_per_cu(N, 4, 4) == 4          # the footprint at this horizon does not cap the plan
    rows = R.rowqp_rows(nc, B)
    assert rows == {"rows1": 1, "rows2": 2, "rows4": 4, "split": 4}[side]
    assert R.rowqp_splits(nc, B, rows) == (side == "split")
    a = F.args32(random_scenarios(B, N=N, seed=700 + B % 97, blend=(3.0, 5.0)))
    eng = _engine(default_config(N=N))
    solve = lambda *t: eng.solve_numpy(*t, dtype=np.float32)
    g = _composition_free(solve, tuple(a[k] for k in F.ARGS), nc, seed=B)
    eng.close()
    assert (g[3] == 0).all() and (g[4] > 0).mean() >= 0.25


# ---------------------------------------------------------------------------------------------------------------------------------
# one handle, both widths

def test_one_handle_alternating_widths():
    """ensure_row / ensure_mult are sized by element width: fp32 B = 300, fp64 B = 700, fp32 B = 1200, fp64 B = 100 on one handle with
    an SQP tolerance (the multiplier workspace is in use), each bit-identical to a fresh handle's result."""
    from ad_mpc_amd.scenarios import random_scenarios
    N = 24
    cfg = default_config(N=N, sqp_iters=4, sqp_tol=1e-6)
    one = _engine(cfg)
    for step, (B, dt) in enumerate(((300, np.float32), (700, np.float64), (1200, np.float32), (100, np.float64))):
        s = random_scenarios(B, N=N, seed=800 + step, blend=(3.0, 5.0))
        args = tuple(np.ascontiguousarray(s[k], dtype=dt) for k in F.ARGS)
        got = one.solve_numpy(*args, dtype=dt)
        fresh = _engine(cfg)
        want = fresh.solve_numpy(*args, dtype=dt)
        fresh.close()
        assert set(np.unique(want[3])) <= {0, 2}
        for x, y, nm in zip(got, want, ("x", "u", "cost", "status", "iters")):
            _bits(x, y, "call %d (B = %d, %s): %s" % (step, B, np.dtype(dt).name, nm))
    one.close()
