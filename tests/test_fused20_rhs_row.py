"""Kernel F (admpc_fused20.hip), phase D: the trial's right-hand side -g0 and the predictor's right-hand side ride through the
factorisation as row 40 of the Newton matrix (dense40.h, dense40_factorise with a right-hand-side row) and those two solves run the
backward substitution only; the corrector keeps the whole solve.  The cases below are the ways an instance reaches the two call
sites -- the trial alone, the predictor behind a failed trial (warm start), the predictor from a cold start, the fallback restart
(a `continue` in front of the factorisation, with a right-hand side already published), an abandoned warm start, the tight stopping
test, the second instantiation of the kernel -- against the oracle under the suite's rule for this path: identical statuses and
iteration counts, solutions within 1e-8.  Then what must not depend on anything but the instance: two solves on one handle, and two
draw orders of a batch larger than the grid, give the same bytes.
"""
import numpy as np
import pytest

import batch_regimes as R
from ad_mpc_amd.config import default_config, tight_config
from ad_mpc_amd.scenarios import random_scenarios
from test_gpu_parity import _assert_parity, TOL

pytestmark = pytest.mark.gpu

CAR = ("x0", "yref", "yref_e", "p", "xbar", "ubar")
SEED = 1234
BLENDS = [(100.0, 110.0), (3.0, 5.0)]


def _args(s):
    return tuple(s[k] for k in CAR)


def _default():
    return default_config(N=20)


def _no_trial():
    cfg = default_config(N=20).copy(); cfg.ipm_try_unconstrained = 0.0
    return cfg


def _fallback():                        # test_gpu_parity.test_fallback_mode
    cfg = tight_config(N=20); cfg.ipm_fallback_iter = 3.0
    return cfg


def _warm_abandoned():                  # test_gpu_parity.test_blocked_warm_start_is_abandoned
    cfg = tight_config(N=20); cfg.ipm_warm_restart = 0.99
    return cfg


def _tight():
    return tight_config(N=20)


def _q127():                            # all seven state weights: the kernel's second instantiation
    return default_config(N=20, q=(10.0, 10.0, 100.0, 1.0, 2.0, 3.0, 4.0))


CONFIGS = {"default": _default, "no_trial": _no_trial, "fallback": _fallback, "warm_abandoned": _warm_abandoned, "tight": _tight, "q127": _q127}


@pytest.mark.parametrize("B", [64, 1])
@pytest.mark.parametrize("blend", BLENDS, ids=["blend100", "blend3"])
@pytest.mark.parametrize("case", list(CONFIGS))
def test_parity_at_both_call_sites(gpu_engine_factory, oracle_omp, case, blend, B):
    cfg = CONFIGS[case]()
    s = random_scenarios(B, N=20, seed=SEED, blend=blend)
    g = gpu_engine_factory(cfg).solve_numpy(*_args(s))
    o = oracle_omp.solve_batch(cfg, *_args(s), nthreads=16)
    it = o[4]
    print("%s blend %s B %d: iterations %s" % (case, blend, B, np.bincount(it).tolist()))
    assert (o[3] == 0).all()
    if case == "default" and B == 64:
        assert (it == 0).any() and (it > 0).any()            # the trial solves some, the others iterate: both call sites run
    if case == "no_trial":
        assert (it >= 1).all()                               # every instance takes the predictor path, from a cold start
    if case == "fallback" and B == 64 and blend == BLENDS[1]:
        assert (it > 3).any()                                # the restart is reached
    if case == "warm_abandoned" and B == 64 and blend == BLENDS[1]:
        off = cfg.copy(); off.ipm_warm_restart = 0.0
        assert (oracle_omp.solve_batch(off, *_args(s), nthreads=16)[4] != it).any()      # somebody's warm start is abandoned
    _assert_parity(g, o, TOL)


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert a.tobytes() == b.tobytes(), what


def test_two_solves_on_one_handle_give_the_same_bytes(gpu_engine_factory):
    s = random_scenarios(64, N=20, seed=SEED, blend=BLENDS[1])
    eng = gpu_engine_factory(default_config(N=20))
    g1 = eng.solve_numpy(*_args(s))
    g2 = eng.solve_numpy(*_args(s))
    assert (g1[4] == 0).any() and (g1[4] > 0).any()
    for k, name in enumerate(("x", "u", "cost", "status", "iters")):
        _bits(g1[k], g2[k], name)


def test_two_draw_orders_past_the_grid_give_the_same_bytes(gpu_engine_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nc = R.num_cu()
    B = R.f_past(nc)                                         # the smallest batch the suite uses beyond eight waves per CU
    assert R.work_ordered(R.f_grid(nc, B), B)
    s = random_scenarios(B, N=20, seed=SEED, blend=BLENDS[1])
    eng = gpu_engine_factory(default_config(N=20))
    g = eng.solve_numpy(*_args(s))
    perm = np.random.default_rng(SEED).permutation(B)
    gp = eng.solve_numpy(*tuple(a[perm] for a in _args(s)))
    assert (g[4] == 0).any() and (g[4] > 0).any()
    for k, name in enumerate(("x", "u", "cost", "status", "iters")):
        _bits(g[k][perm], gp[k], "permuted batch: " + name)
