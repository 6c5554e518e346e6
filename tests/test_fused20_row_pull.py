"""Kernel F (admpc_fused20.hip), phase D: H is pulled into registers unmasked (the diagonal term through LDS where that is exact), the
mat-vec's row comes without presets, the complementarity and step stop tests are wave votes and the per-stage scans run five steps.
The paths of phase D that tests/test_fused20_rhs_row.py does not drive, against the oracle under the suite's rule for this path
(identical statuses and iteration counts, solutions within 1e-8), at B = 64 and B = 1:
  - an iteration limit that is reached: the loop ends on its bound with the next iteration's H in flight;
  - the GP configuration;
  - a steering box tight enough that some instance needs eight or more iterations (seeds picked with the oracle alone: the assertion
    on the oracle's iteration counts holds without a GPU);
  - one instance of 64 with a non-finite x0: status and untouched iterate as the oracle gives them, its 63 neighbours as without it.
The cases name nothing this change adds: they hold for the kernel before it as well.
"""
import numpy as np
import pytest

from ad_mpc_amd.config import default_config, set_gp
from ad_mpc_amd.scenarios import random_scenarios, grid_gp
from test_gpu_parity import _assert_parity, TOL

pytestmark = pytest.mark.gpu

CAR = ("x0", "yref", "yref_e", "p", "xbar", "ubar")
BLEND = (3.0, 5.0)


def _args(s):
    return tuple(s[k] for k in CAR)


def _iteration_limit():
    cfg = default_config(N=20); cfg.ipm_iter_max = 2
    return cfg, 2, lambda o, B: (o[4] == 2).sum() >= (B + 3) // 4


def _gp():
    cfg = default_config(N=20); set_gp(cfg, grid_gp())
    return cfg, 2, lambda o, B: (o[4] >= 4).sum() >= (B + 3) // 4


def _tight_steering():
    cfg = default_config(N=20); cfg.lbx_delta, cfg.ubx_delta = -0.05, 0.05
    return cfg, 1, lambda o, B: (o[4] >= 8).sum() >= (B + 3) // 4


CASES = {"iteration_limit": _iteration_limit, "gp": _gp, "tight_steering": _tight_steering}


@pytest.mark.parametrize("B", [64, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_parity_on_the_paths_of_phase_d(gpu_engine_factory, oracle_omp, case, B):
    cfg, seed, reached = CASES[case]()
    s = random_scenarios(B, N=20, seed=seed, blend=BLEND)
    g = gpu_engine_factory(cfg).solve_numpy(*_args(s))
    o = oracle_omp.solve_batch(cfg, *_args(s), nthreads=16)
    print("%s B %d: iterations %s" % (case, B, np.bincount(o[4]).tolist()))
    assert (o[3] == 0).all() and reached(o, B)
    _assert_parity(g, o, TOL)


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_one_non_finite_x0_among_64(gpu_engine_factory, oracle_omp, bad):
    cfg = default_config(N=20)
    s = random_scenarios(64, N=20, seed=1234, blend=BLEND)
    k = 17
    sb = {key: v.copy() for key, v in s.items()}
    sb["x0"][k, 1] = bad
    eng = gpu_engine_factory(cfg)
    g0 = eng.solve_numpy(*_args(s))
    g = eng.solve_numpy(*_args(sb))
    o = oracle_omp.solve_batch(cfg, *_args(sb), nthreads=16)
    assert o[3][k] != 0 and (np.delete(o[3], k) == 0).all() and (np.delete(o[4], k) > 0).any()
    _assert_parity(g, o, TOL)                                            # statuses on all 64, iterations and solutions on the 63
    assert np.isinf(g[2][k]) and np.isinf(o[2][k])
    np.testing.assert_array_equal(o[0][k], sb["xbar"][k]); np.testing.assert_array_equal(o[1][k], sb["ubar"][k])
    np.testing.assert_array_equal(g[0][k], sb["xbar"][k]); np.testing.assert_array_equal(g[1][k], sb["ubar"][k])      # the iterate stays as it is
    for a, b, name in zip(g, g0, ("x", "u", "cost", "status", "iters")):                                                    # the neighbours: the same bytes
        a, b = np.ascontiguousarray(np.delete(a, k, axis=0)), np.ascontiguousarray(np.delete(b, k, axis=0))
        assert a.tobytes() == b.tobytes(), name
