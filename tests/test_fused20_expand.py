"""Kernel F (admpc_fused20.hip), phase E: the state expansion dx_{k+1} = A_k dx_k + B_k du_k + b_k runs on operands that were read
from LDS one stage ahead of the stage that uses them, and every lane stores its dx_k (lanes that hold no state into a dump area).
The cases below are the ways an instance reaches or leaves that phase -- a batch inside the grid and one past it (the next ticket is
drawn inside the phase), instances the trial solves next to instances that iterate, the iteration limit (the last fetch of H is in
flight into the buffer the phase writes), a non-finite instance that never gets there, and a later SQP pass that skips finished
instances -- against the oracle: identical statuses and iteration counts, solutions within the suite's tolerance for this path.
"""
import numpy as np
import pytest

import batch_regimes as R
from ad_mpc_amd.config import default_config
from ad_mpc_amd.scenarios import random_scenarios
from test_gpu_parity import _assert_parity, TOL

pytestmark = pytest.mark.gpu

CAR = ("x0", "yref", "yref_e", "p", "xbar", "ubar")


@pytest.fixture(scope="module")
def nc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return R.num_cu()


def _args(s):
    return tuple(s[k] for k in CAR)


@pytest.mark.parametrize("size", ["1", "3", "65", "past_grid"])
def test_expansion_parity_inside_and_past_the_grid(gpu_engine_factory, oracle_omp, nc, size):
    """B = 1, 3, 65: one instance per wave, no tickets.  Past the grid: every wave draws its next ticket at the top of phase E and
    resolves it behind the recursion.  From 65 on the batch mixes instances the trial solves with instances that iterate."""
    B = R.f_past(nc) if size == "past_grid" else int(size)
    assert R.work_ordered(R.f_grid(nc, B), B) == (size == "past_grid")
    cfg = default_config(N=20)
    s = random_scenarios(B, N=20, seed=4100 + B, blend=(3.0, 5.0))
    g = gpu_engine_factory(cfg).solve_numpy(*_args(s))
    o = oracle_omp.solve_batch(cfg, *_args(s), nthreads=16)
    assert (o[3] == 0).all()
    if B >= 65:
        assert (o[4] == 0).sum() >= 8 and (o[4] > 0).sum() >= 8
    _assert_parity(g, o, TOL)


def test_iteration_limit_reaches_the_expansion_with_a_fetch_in_flight(gpu_engine_factory, oracle_omp):
    """ipm_iter_max = 1: the interior point leaves its loop behind the first corrector, whose last substitution has just issued the
    fetch of H for an iteration that never comes -- into the buffer phase E writes du and dx to."""
    cfg = default_config(N=20).copy()
    cfg.ipm_iter_max = 1
    s = random_scenarios(65, N=20, seed=4200, blend=(3.0, 5.0))
    g = gpu_engine_factory(cfg).solve_numpy(*_args(s))
    o = oracle_omp.solve_batch(cfg, *_args(s), nthreads=16)
    assert (o[4] == 1).sum() >= 8 and (o[4] == 0).sum() >= 8 and o[4].max() == 1
    _assert_parity(g, o, TOL)


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_non_finite_x0_fails_alone(gpu_engine_factory, oracle_omp, value):
    cfg = default_config(N=20)
    s = random_scenarios(9, N=20, seed=4300, blend=(3.0, 5.0))
    s["x0"] = s["x0"].copy()
    s["x0"][4, 1] = value
    g = gpu_engine_factory(cfg).solve_numpy(*_args(s))
    o = oracle_omp.solve_batch(cfg, *_args(s), nthreads=16)
    ok = np.ones(9, dtype=bool); ok[4] = False
    assert g[3][4] == 4 and np.isposinf(g[2][4])
    np.testing.assert_array_equal(g[0][4], s["xbar"][4]); np.testing.assert_array_equal(g[1][4], s["ubar"][4])
    assert (g[3][ok] == 0).all()
    _assert_parity(g, o, TOL)


def test_later_sqp_passes_skip_finished_instances(gpu_engine_factory, oracle_omp, nc):
    """Three SQP passes in one call, past the grid: passes two and three run with first_pass = 0 and skip what failed in the first
    (status 4, cost +inf, iterate as it came in); the others are expanded three times.  (Tolerance of the suite's SQP cases: three
    full Newton steps on top of each other.)"""
    B = R.f_past(nc)
    cfg = default_config(N=20, sqp_iters=3)
    good = random_scenarios(B - 8, N=20, seed=4400, blend=(3.0, 5.0))
    bad = random_scenarios(8, N=20, seed=3, blend=(3.0, 5.0), init="zeros")            # zeros iterate with p > 0: non-finite model
    s = {k: np.concatenate([good[k][:20], bad[k], good[k][20:]]) for k in good}
    g = gpu_engine_factory(cfg).solve_numpy(*_args(s))
    o = oracle_omp.solve_batch(cfg, *_args(s), nthreads=16)
    np.testing.assert_array_equal(g[3], o[3])
    failed = g[3] != 0
    assert failed[20:28].any() and not failed[:20].any() and (~failed).sum() >= B - 8
    assert np.isposinf(g[2][failed]).all()
    np.testing.assert_array_equal(g[0][failed], s["xbar"][failed]); np.testing.assert_array_equal(g[1][failed], s["ubar"][failed])
    ok = ~failed
    np.testing.assert_array_equal(g[4][ok], o[4][ok])
    assert np.abs(g[1][ok] - o[1][ok]).max() <= 1e-7 and np.abs(g[0][ok] - o[0][ok]).max() <= 1e-7
    np.testing.assert_allclose(g[2][ok], o[2][ok], rtol=1e-9, atol=1e-9)
