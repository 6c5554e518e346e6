"""Kernel F (admpc_fused20.hip) keeps H in a per-wave slot of global memory while its factor holds the one LDS buffer they share, and
fetches it back by LDS-DMA in front of iteration 0 (behind the trial) and behind the corrector's last substitution of every iteration.
Every path that reaches a factorisation or the residual's mat-vec must find H in LDS; each case below drives one of them at a batch
past the persistent grid (every wave draws several instances, so a slot is rewritten while the previous instance's lines may still
be in the CU's vector L1), against the oracle: identical statuses and iteration counts, solutions within the suite's tolerance.
"""
import numpy as np
import pytest

import batch_regimes as R
from ad_mpc_amd.config import default_config, tight_config, set_gp
from ad_mpc_amd.scenarios import random_scenarios, grid_gp
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


def _case(name):
    """(config, scenario keywords, a check on the oracle's output that the case reaches its path)"""
    if name == "many_iterations":
        return tight_config(N=20), {"blend": (3.0, 5.0)}, lambda o, B: (o[4] >= 8).sum() >= 16
    if name == "warm_restart":            # alpha < 0.99 at iteration 0 of a warm start: cold start behind the corrector's fetch
        cfg = tight_config(N=20); cfg.ipm_warm_restart = 0.99
        return cfg, {"blend": (3.0, 5.0)}, None
    if name == "fallback_restart":        # the restart at iteration 3 takes the path without a factorisation behind the fetch
        cfg = tight_config(N=20); cfg.ipm_fallback_iter = 3.0
        return cfg, {"blend": (3.0, 5.0)}, lambda o, B: (o[4] > 3).sum() >= B // 4
    if name == "iteration_limit":         # the loop ends on its bound with the next iteration's fetch in flight
        cfg = tight_config(N=20); cfg.ipm_iter_max = 4; cfg.ipm_fallback_iter = 0.0
        return cfg, {"blend": (3.0, 5.0)}, lambda o, B: (o[4] == 4).sum() >= B // 4
    if name == "no_trial":                # no trial: H is never overwritten before iteration 0
        cfg = tight_config(N=20); cfg.ipm_try_unconstrained = 0.0
        return cfg, {"blend": (3.0, 5.0)}, lambda o, B: (o[4] > 0).all()
    if name == "gp":
        cfg = default_config(N=20); set_gp(cfg, grid_gp())
        return cfg, {"blend": (3.0, 5.0)}, lambda o, B: (o[4] > 0).sum() >= 16
    raise ValueError(name)


@pytest.mark.parametrize("name", ["many_iterations", "warm_restart", "fallback_restart", "iteration_limit", "no_trial", "gp"])
def test_h_slot_paths_past_the_grid(gpu_engine_factory, oracle_omp, nc, name):
    B = R.f_past(nc)
    assert R.work_ordered(R.f_grid(nc, B), B)
    cfg, kw, reached = _case(name)
    s = random_scenarios(B, N=20, seed=2024, **kw)
    g = gpu_engine_factory(cfg).solve_numpy(*_args(s))
    o = oracle_omp.solve_batch(cfg, *_args(s), nthreads=16)
    if name == "warm_restart":
        off = cfg.copy(); off.ipm_warm_restart = 0.0
        assert (oracle_omp.solve_batch(off, *_args(s), nthreads=16)[4] != o[4]).sum() >= B // 20
    else:
        assert reached(o, B)
    _assert_parity(g, o, TOL)


@pytest.mark.parametrize("model", ["plain", "gp"])
def test_two_handles_interleaved_on_two_streams_give_the_bits_of_one(gpu_engine_factory, nc, model):
    """Slots belong to a handle: two handles whose launches interleave on two streams return the bits of one handle solving the same
    batches one after the other (batches past the grid: every wave of both launches rewrites its slot several times)."""
    import torch
    cfg = default_config(N=20)
    if model == "gp":
        set_gp(cfg, grid_gp())
    B = R.f_past(nc)
    sc = [random_scenarios(B, N=20, seed=700 + i, blend=(3.0, 5.0)) for i in range(4)]
    e0, e1 = gpu_engine_factory(cfg), gpu_engine_factory(cfg)
    ref = [e0.solve_numpy(*_args(s)) for s in sc]
    d = e0.to_device
    dev = [[d(s[k]) for k in CAR] for s in sc]
    outs = [(torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"),
             torch.empty(B, dtype=torch.int32, device="cuda")) for _ in sc]
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    torch.cuda.synchronize()
    for i, a in enumerate(dev):
        with torch.cuda.stream(streams[i & 1]):
            (e0, e1)[i & 1].solve(a[0], a[1], a[2], a[3], a[4], a[5], *outs[i])
    torch.cuda.synchronize()
    for i, a in enumerate(dev):
        got = (a[4].cpu().numpy(), a[5].cpu().numpy(), outs[i][0].cpu().numpy(), outs[i][1].cpu().numpy(), outs[i][2].cpu().numpy())
        for k, (x, r) in enumerate(zip(got, ref[i])):
            x, r = np.ascontiguousarray(x), np.ascontiguousarray(r)
            assert x.dtype == r.dtype and x.shape == r.shape
            assert (x.view(np.uint8) == r.view(np.uint8)).all(), "batch %d, output %d: bits differ" % (i, k)
    assert (ref[0][4] > 0).any()
