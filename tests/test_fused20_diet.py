"""Kernel F (admpc_fused20.hip): the per-lane LDS addresses and masks of the condensing chain (phase C) and of the expansion (phase E) are
formed once per instance, and the expansion's lanes >= 7 get their exact 0.0 from operands they read as zeros instead of a select.  No
arithmetic changed, so the cases are the paths that use what moved, against the oracle under the suite's rule for this path (identical
statuses and iteration counts, solutions within 1e-8), at B = 64 and B = 1:
  - every state weighted: the kernel's second instantiation, two MFMA steps per stage with their own operand addresses;
  - the default weights, with at least a quarter of the instances at three or more iterations;
  - the blend speeds (3, 5): the dynamic branch of the model (every case below runs there);
  - the GP configuration;
  - a warm start that is abandoned (ipm_warm_restart = 0.999, the C ABI admits [0, 1): by the oracle's iteration counts with and without
    the rule, every instance of the draw that iterates restarts);
  - the conservative restart (ipm_fallback_iter = 2);
  - one instance of 64 with x0 = inf: status, untouched iterate and infinite cost as the oracle's, the neighbours' bytes as without it
    (the expansion's lanes >= 7 and its 21 tests for a non-finite dx).
The seed is picked with the oracle alone; every case is guarded by an assertion on the oracle's own counts that holds without a GPU.
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
SEED = 2            # the oracle iterates on instance 0 of this draw in every configuration below (B = 1 is that instance)


def _args(s):
    return tuple(s[k] for k in CAR)


def _quarter(B):
    return (B + 3) // 4


def _q127():
    return default_config(N=20, q=(10.0, 10.0, 100.0, 1.0, 2.0, 3.0, 4.0)), lambda o, B, ref: (o[4] >= 3).sum() >= _quarter(B)


def _default():
    return default_config(N=20), lambda o, B, ref: (o[4] >= 3).sum() >= _quarter(B)


def _gp():
    cfg = default_config(N=20); set_gp(cfg, grid_gp())
    return cfg, lambda o, B, ref: (o[4] >= 3).sum() >= _quarter(B)


def _warm_abandoned():
    cfg = default_config(N=20); cfg.ipm_warm_restart = 0.999
    # ref: the oracle with the rule off.  The restart costs iterations: every instance that iterates at all has abandoned its warm start
    return cfg, lambda o, B, ref: ((o[4] != ref[4]) == (ref[4] > 0)).all() and (ref[4] > 0).sum() >= _quarter(B)


def _fallback():
    cfg = default_config(N=20); cfg.ipm_fallback_iter = 2.0
    return cfg, lambda o, B, ref: (o[4] > 2).sum() >= _quarter(B)                 # past the iteration at which the restart runs


CASES = {"q127": _q127, "default": _default, "gp": _gp, "warm_abandoned": _warm_abandoned, "fallback": _fallback}


@pytest.mark.parametrize("B", [64, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_parity_on_the_paths_the_hoisted_addresses_serve(gpu_engine_factory, oracle_omp, case, B):
    cfg, reached = CASES[case]()
    s = random_scenarios(B, N=20, seed=SEED, blend=BLEND)
    g = gpu_engine_factory(cfg).solve_numpy(*_args(s))
    o = oracle_omp.solve_batch(cfg, *_args(s), nthreads=16)
    off = default_config(N=20); off.ipm_warm_restart = 0.0
    ref = oracle_omp.solve_batch(off, *_args(s), nthreads=16)
    print("%s B %d: iterations %s" % (case, B, np.bincount(o[4]).tolist()))
    assert (o[3] == 0).all() and reached(o, B, ref)
    _assert_parity(g, o, TOL)


def test_one_infinite_x0_among_64(gpu_engine_factory, oracle_omp):
    cfg = default_config(N=20)
    s = random_scenarios(64, N=20, seed=SEED, blend=BLEND)
    k = 41
    sb = {key: v.copy() for key, v in s.items()}
    sb["x0"][k, 0] = np.inf
    eng = gpu_engine_factory(cfg)
    g0 = eng.solve_numpy(*_args(s))
    g = eng.solve_numpy(*_args(sb))
    o = oracle_omp.solve_batch(cfg, *_args(sb), nthreads=16)
    assert o[3][k] != 0 and (np.delete(o[3], k) == 0).all() and (np.delete(o[4], k) >= 3).sum() >= 16
    _assert_parity(g, o, TOL)                                            # statuses on all 64, iterations and solutions on the 63
    assert np.isinf(g[2][k]) and np.isinf(o[2][k])
    np.testing.assert_array_equal(o[0][k], sb["xbar"][k]); np.testing.assert_array_equal(o[1][k], sb["ubar"][k])
    np.testing.assert_array_equal(g[0][k], sb["xbar"][k]); np.testing.assert_array_equal(g[1][k], sb["ubar"][k])      # the iterate stays as it is
    for a, b, name in zip(g, g0, ("x", "u", "cost", "status", "iters")):                                                    # the neighbours: the same bytes
        a, b = np.ascontiguousarray(np.delete(a, k, axis=0)), np.ascontiguousarray(np.delete(b, k, axis=0))
        assert a.tobytes() == b.tobytes(), name
