"""Parity tests proper: the HIP path, called through the C ABI (libadmpc.so), against the CPU oracle on
identical seeded inputs, against the committed golden fixtures, and through size-independent properties
at BASELINE's full batch sizes.

Stated tolerances (written in the assertions below):
  shooting quantities         <= 1e-11 relative (reference golden vectors)
  fp64 solve, N <= 32         |u - u_oracle|, |x - x_oracle| <= 1e-8 absolute   (measured 1e-13 .. 2e-12)
  fp64 solve, N  > 32         <= 1e-7 absolute                                   (measured 2e-10 .. 4e-8)
  fp32 solve (configs[4])     <= 2e-3 absolute on inputs of size 10 (2e-4 of the input range; measured 5e-4)
  status identical, interior-point iteration counts IDENTICAL on every committed input (fp64).
Why the long horizons get 1e-7: the last iterations of the interior point run with slacks of active hard bounds at the
rounding level of the states (1e-16); the ratio test of those iterations amplifies last-bit differences between two correct
evaluation orders into a step length of 0.90 instead of 0.999999 on an update of size 2e-7.
"""
import ctypes as C
import os
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from ad_mpc_amd.config import default_config, tight_config, set_gp, AdmpcConfig  # noqa: E402
from ad_mpc_amd.scenarios import random_scenarios, straight_scenario, assemble, grid_gp  # noqa: E402

TOL = 1e-8
TOL_LONG = 1e-7


def tol_for(N):
    return TOL if N <= 32 else TOL_LONG


def _solve_both(eng, oracle, cfg, s, nthreads=1):
    g = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    o = oracle.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], nthreads=nthreads)
    return g, o


def _assert_parity(g, o, tol=TOL):
    """Same Newton steps on both sides: identical status, identical interior-point iteration counts, solutions within `tol`."""
    x, u, cost, st, it = g; xo, uo, co, so, io = o
    np.testing.assert_array_equal(st, so)
    ok = so == 0
    np.testing.assert_array_equal(it[ok], io[ok])
    assert np.abs(u[ok] - uo[ok]).max(initial=0.0) <= tol, np.abs(u[ok] - uo[ok]).max()
    assert np.abs(x[ok] - xo[ok]).max(initial=0.0) <= tol, np.abs(x[ok] - xo[ok]).max()
    np.testing.assert_allclose(cost[ok], co[ok], rtol=1e-9, atol=1e-9)


def test_shooting_against_reference_golden_vectors(gpu_engine_factory, golden_shooting):
    """H0/H1 on the GPU against vectors from the reference's compiled CasADi code."""
    import torch
    cases = golden_shooting["cases"]
    cfg = default_config(N=2, Ts=cases[0]["h"])
    eng = gpu_engine_factory(cfg)
    B = len(cases)
    xbar = np.zeros((B, 3, 7)); ubar = np.zeros((B, 2, 2)); p = np.zeros(B)
    for b, c in enumerate(cases):
        xbar[b, 0] = c["x"]; xbar[b, 1] = c["x"]; ubar[b, 0] = c["u"]; ubar[b, 1] = c["u"]; p[b] = c["p"]
    phi, A, Bm = eng.shoot(eng.to_device(xbar), eng.to_device(ubar), eng.to_device(p))
    torch.cuda.synchronize()
    phi, A, Bm = phi.cpu().numpy(), A.cpu().numpy(), Bm.cpu().numpy()
    for b, c in enumerate(cases):
        for k in (0, 1):
            np.testing.assert_allclose(phi[b, k], np.array(c["phi"]), rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(A[b, k], np.array(c["A"]), rtol=1e-11, atol=1e-13)
            np.testing.assert_allclose(Bm[b, k], np.array(c["B"]), rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("N,B,blend,init", [
    (20, 256, (100.0, 110.0), "x0"), (20, 256, (3.0, 5.0), "x0"), (20, 64, (100.0, 110.0), "zeros"),
    (40, 64, (3.0, 5.0), "x0"), (32, 16, (3.0, 5.0), "x0"), (33, 16, (3.0, 5.0), "x0"), (64, 8, (100.0, 110.0), "x0"),
    (2, 8, (3.0, 5.0), "x0"), (5, 1, (3.0, 5.0), "x0"),
])
def test_solve_parity_with_oracle(gpu_engine_factory, oracle, N, B, blend, init):
    cfg = default_config(N=N)
    s = random_scenarios(B, N=N, seed=1234, blend=blend, init=init)
    g, o = _solve_both(gpu_engine_factory(cfg), oracle, cfg, s)
    assert (o[3] == 0).all()
    _assert_parity(g, o, tol_for(N))


def test_both_qp_kernels_agree_at_n20(gpu_engine_factory, oracle, monkeypatch):
    """N = 20 has two device paths: the condensed dense-LDL' pipeline (default) and the row-mapped Riccati kernel R
    (ADMPC_QP=riccati, the path of every other horizon and of every fp32 solve).  Both must match the oracle."""
    cfg = tight_config(N=20)
    s = random_scenarios(512, N=20, seed=77, blend=(3.0, 5.0))
    o = oracle.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    g_dense = gpu_engine_factory(cfg).solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    monkeypatch.setenv("ADMPC_QP", "riccati")
    g_ric = gpu_engine_factory(cfg).solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    # and once more with the unconstrained trial switched off on both sides
    cfg_r = cfg.copy(); cfg_r.ipm_try_unconstrained = 0.0
    o_r = oracle.solve_batch(cfg_r, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    g_ric0 = gpu_engine_factory(cfg_r).solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    monkeypatch.delenv("ADMPC_QP")
    _assert_parity(g_dense, o)
    _assert_parity(g_ric, o)
    _assert_parity(g_ric0, o_r)
    assert (g_ric[4] == 0).mean() > 0.3 and (g_ric0[4] >= 4).all()
    assert np.abs(g_dense[1] - g_ric[1]).max() <= TOL


def test_unconstrained_trial_on_and_off(gpu_engine_factory, oracle):
    """cfg.ipm_try_unconstrained: instances whose inequality-free minimiser is feasible skip the interior point (iters = 0).
    Both settings return the same solution; the skip set is the oracle's; it is a majority of the config-2 scenarios."""
    s = random_scenarios(1024, N=20, seed=1234)
    on = tight_config(N=20); off = on.copy(); off.ipm_try_unconstrained = 0.0
    assert on.ipm_try_unconstrained == 1.0
    g_on, o_on = _solve_both(gpu_engine_factory(on), oracle, on, s)
    g_off, o_off = _solve_both(gpu_engine_factory(off), oracle, off, s)
    _assert_parity(g_on, o_on); _assert_parity(g_off, o_off)
    np.testing.assert_array_equal(g_on[4] == 0, o_on[4] == 0)
    assert (g_on[4] == 0).mean() > 0.4 and (g_off[4] >= 4).all()
    assert np.abs(g_on[1] - g_off[1]).max() <= 1e-9 and np.abs(g_on[0] - g_off[0]).max() <= 1e-9


@pytest.mark.parametrize("N", [20, 24, 40])
def test_warm_start_from_the_unconstrained_minimiser(gpu_engine_factory, oracle, N):
    """cfg.ipm_warm_thr: after a failed trial the interior point starts from the inequality-free minimiser (default) or from
    the zero step (0).  Same solution either way, oracle parity for both, and fewer iterations with the warm start --
    on the condensed path (N = 20) and on the Riccati path (N = 24, 40)."""
    s = random_scenarios(512, N=N, seed=4321, blend=(3.0, 5.0))
    warm = tight_config(N=N); cold = warm.copy(); cold.ipm_warm_thr = 0.0
    assert warm.ipm_warm_thr == 0.01
    g_w, o_w = _solve_both(gpu_engine_factory(warm), oracle, warm, s)
    g_c, o_c = _solve_both(gpu_engine_factory(cold), oracle, cold, s)
    _assert_parity(g_w, o_w, tol_for(N)); _assert_parity(g_c, o_c, tol_for(N))
    np.testing.assert_array_equal(g_w[4] == 0, g_c[4] == 0)                 # the trial decides the same way
    assert np.abs(g_w[1] - g_c[1]).max() <= 1e-7 and np.abs(g_w[0] - g_c[0]).max() <= 1e-7
    ipm = g_c[4] > 0
    assert ipm.any() and g_w[4][ipm].mean() < 0.9 * g_c[4][ipm].mean()
    bad = cold.copy(); bad.ipm_warm_thr = -1.0
    h = C.c_void_p(0)
    from ad_mpc_amd import _lib
    assert _lib.load().admpc_create(C.byref(bad), 0, C.byref(h)) == -1


def test_blocked_warm_start_is_abandoned(gpu_engine_factory, oracle_omp):
    """cfg.ipm_warm_restart on the device: forced (0.99) through the condensed pipeline (N = 20) and kernel R (N = 40), then the default
    on the whole N = 80 batch it was introduced for (24 of 2048 instances restart; maximum 24 -> 19 iterations)."""
    for N, B in ((20, 512), (40, 256)):
        cfg = tight_config(N=N); cfg.ipm_warm_restart = 0.99
        s = random_scenarios(B, N=N, seed=21, blend=(3.0, 5.0))
        g, o = _solve_both(gpu_engine_factory(cfg), oracle_omp, cfg, s, nthreads=8)
        off = cfg.copy(); off.ipm_warm_restart = 0.0
        assert (oracle_omp.solve_batch(off, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], nthreads=8)[4] != o[4]).sum() >= B // 10
        _assert_parity(g, o, tol_for(N))
    N = 80
    cfg = tight_config(N=N)
    s = random_scenarios(2048, N=N, seed=1234)
    g, o = _solve_both(gpu_engine_factory(cfg), oracle_omp, cfg, s, nthreads=8)
    # every instance, iteration for iteration (round 3: the oracle's stopping test takes the stationarity residual through the same
    # (1 - alpha) law as the kernel instead of re-evaluating it on its rounding floor; instances 1167 and 1799 used to differ by one)
    assert (o[3] == 0).all()
    _assert_parity(g, o, tol_for(N))
    assert o[4].max() <= 19 and g[4].max() <= 19
    off = cfg.copy(); off.ipm_warm_restart = 0.0
    slow = oracle_omp.solve_batch(off, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], nthreads=8)
    assert slow[4].max() >= 24 and 10 <= (slow[4] != o[4]).sum() <= 100 and np.abs(slow[1] - o[1]).max() <= 1e-7


def test_fallback_mode(gpu_engine_factory, oracle_omp):
    """cfg.ipm_fallback_iter on the device: forced (3) through the condensed pipeline (N = 20) and kernel R (N = 40, 24), then the default
    on the batches that hold the four known cycling instances (tests/test_rowqp_emu.py CYCLING): every instance of those batches
    converges, iteration for iteration with the oracle."""
    from test_rowqp_emu import CYCLING
    for N, B in ((20, 512), (40, 256), (24, 130)):
        cfg = tight_config(N=N); cfg.ipm_fallback_iter = 3.0
        s = random_scenarios(B, N=N, seed=33, blend=(3.0, 5.0))
        g, o = _solve_both(gpu_engine_factory(cfg), oracle_omp, cfg, s, nthreads=8)
        assert (o[4] > 3).sum() >= B // 4 and (o[4] <= 3).sum() >= 1
        _assert_parity(g, o, tol_for(N))
    for N, B, kw, seed in ((40, 4096, {"blend": (3.0, 5.0)}, 2), (80, 2048, {}, 4), (80, 2048, {"blend": (3.0, 5.0)}, 4)):
        cfg = tight_config(N=N)
        s = random_scenarios(B, N=N, seed=seed, **kw)
        g, o = _solve_both(gpu_engine_factory(cfg), oracle_omp, cfg, s, nthreads=8)
        np.testing.assert_array_equal(g[3], o[3]); assert (o[3] == 0).all()
        for n_, b_, kw_, seed_, idx, its in CYCLING:
            if (n_, b_, kw_, seed_) == (N, B, kw, seed):
                assert g[4][idx] == o[4][idx] == its
        assert g[4].max() < cfg.ipm_iter_max + 30 and o[4].max() < cfg.ipm_iter_max + 30      # nobody runs out of iterations
        _assert_parity(g, o, tol_for(N))                        # no exceptions: identical iteration counts on every instance


def test_split_batches_give_the_bits_of_one_launch(gpu_engine_factory, oracle_omp, monkeypatch):
    """Kernel R runs batches of more than one round of waves in two phases (trial for all; interior point for the deferred
    instances, ordered by the number of bounds their trial minimiser violates).  ADMPC_ROWQP_SPLIT=1 / 0 force / forbid it: every
    output must be bit-identical either way -- fp64 and fp32, odd batch sizes, converged SQP with its per-instance stop, the
    multiplier snapshot -- and equal to the oracle's."""
    import torch
    def run(cfg, s, mode, dtype=np.float64):
        monkeypatch.setenv("ADMPC_ROWQP_SPLIT", mode)
        return gpu_engine_factory(cfg).solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], dtype=dtype)
    for N, B in ((40, 701), (24, 130), (80, 257), (3, 9)):
        cfg = default_config(N=N)
        s = random_scenarios(B, N=N, seed=50 + N, blend=(3.0, 5.0))
        one, two = run(cfg, s, "0"), run(cfg, s, "1")
        for a, b in zip(one, two):
            np.testing.assert_array_equal(a, b)
        _assert_parity(two, oracle_omp.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], nthreads=8), tol_for(N))
        if N in (40, 80):
            for a, b in zip(run(cfg, s, "0", np.float32), run(cfg, s, "1", np.float32)):
                np.testing.assert_array_equal(a, b)
    # converged SQP: instances freeze one by one, later steps skip them in both phases
    cfg = default_config(N=40); cfg.sqp_iters = 6; cfg.sqp_tol = 1e-6
    s = random_scenarios(300, N=40, seed=8)
    for a, b in zip(run(cfg, s, "0"), run(cfg, s, "1")):
        np.testing.assert_array_equal(a, b)
    # multiplier snapshot (admpc_solve_batch_ex): deferred rows must not write theirs in the first phase
    cfg = default_config(N=40)
    s = random_scenarios(200, N=40, seed=9, blend=(3.0, 5.0))
    outs = []
    for mode in ("0", "1"):
        monkeypatch.setenv("ADMPC_ROWQP_SPLIT", mode)
        eng = gpu_engine_factory(cfg)
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
        x, u = d(s["xbar"]), d(s["ubar"])
        pi, ineq = eng.solve_with_multipliers(d(s["x0"]), d(s["yref"]), d(s["yref_e"]), d(s["p"]), x, u)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (x, u, pi, ineq)])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    monkeypatch.delenv("ADMPC_ROWQP_SPLIT")


def test_full_size_n40_b8192_split_by_default(gpu_engine_factory, oracle_omp):
    """N = 40 at the shard size of configs[3]: two rounds of waves, so the batch takes the two-phase path by default.  Every
    instance against the oracle."""
    N, B = 40, 8192
    cfg = default_config(N=N)
    s = random_scenarios(B, N=N, seed=4321)
    g, o = _solve_both(gpu_engine_factory(cfg), oracle_omp, cfg, s, nthreads=16)
    _assert_parity(g, o, tol_for(N))
    assert (o[4] == 0).mean() > 0.3 and o[4].max() >= 12


def test_all_state_weights_nonzero(gpu_engine_factory, oracle):
    """The shipped weights only track x, y, psi (specialised condensing kernel); with velocity / yaw-rate / steering weights
    the general instantiation runs.  N = 20 (condensed path) and N = 24 (Riccati path) against the oracle."""
    for N in (20, 24):
        cfg = default_config(N=N, q=(10.0, 10.0, 100.0, 1.0, 2.0, 3.0, 4.0))
        s = random_scenarios(128, N=N, seed=99, blend=(3.0, 5.0))
        g, o = _solve_both(gpu_engine_factory(cfg), oracle, cfg, s)
        assert (o[3] == 0).all()
        _assert_parity(g, o)


def _random_problem(rng, N):
    """Problem data away from the shipped values: every weight, asymmetric bounds and L1 penalties, sampling time, terminal scale,
    vehicle parameters (SURVEY Appendix A lists the fields the reference sets; all of them reach the kernels through AdmpcConfig)."""
    q = tuple(float(v) for v in np.r_[rng.uniform(5, 20, 2), rng.uniform(50, 150), rng.uniform(0.0, 3.0, 4)])
    r = (float(rng.uniform(0.5, 2.0)), float(rng.uniform(50, 150)))
    cfg = default_config(N=N, Ts=float(rng.uniform(0.03, 0.08)), q=q, r=r, terminal_scale=float(10 ** rng.uniform(-6, -2)))
    cfg.lbu[0], cfg.ubu[0] = float(-rng.uniform(4, 10)), float(rng.uniform(2, 5))
    cfg.lbu[1], cfg.ubu[1] = float(-rng.uniform(0.3, 0.6)), float(rng.uniform(0.3, 0.6))
    cfg.lbx_delta, cfg.ubx_delta = float(-rng.uniform(0.35, 0.5)), float(rng.uniform(0.35, 0.5))
    cfg.zl, cfg.zu = float(rng.uniform(5, 20)), float(rng.uniform(5, 20))
    cfg.mass *= float(rng.uniform(0.8, 1.2)); cfg.Iz *= float(rng.uniform(0.8, 1.2)); cfg.L_F *= float(rng.uniform(0.9, 1.1))
    cfg.L_R *= float(rng.uniform(0.9, 1.1)); cfg.Cf *= float(rng.uniform(0.8, 1.2)); cfg.Cr *= float(rng.uniform(0.8, 1.2))
    return cfg


def random_q7_problem(rng, N):
    """Problem data away from the shipped values that keeps the shipped weight PATTERN: only x, y and psi carry weights (W[3..6] =
    We[3..6] = 0), so admpc_create picks the qmask-7 instantiation of kernels F and S.  W[0], W[1], W[2] independent; Ts in [0.02, 0.1];
    input weights; terminal scale in [1e-6, 1e-2]; asymmetric input, steering-rate and steering boxes; zl != zu; all six vehicle
    parameters within 30 % of the shipped ones."""
    q = (float(rng.uniform(2, 30)), float(rng.uniform(2, 30)), float(rng.uniform(20, 200)), 0.0, 0.0, 0.0, 0.0)
    r = (float(rng.uniform(0.3, 3.0)), float(rng.uniform(20, 200)))
    cfg = default_config(N=N, Ts=float(rng.uniform(0.02, 0.1)), q=q, r=r, terminal_scale=float(10 ** rng.uniform(-6, -2)))
    cfg.lbu[0], cfg.ubu[0] = float(-rng.uniform(3, 10)), float(rng.uniform(1.5, 6))
    cfg.lbu[1], cfg.ubu[1] = float(-rng.uniform(0.3, 1.0)), float(rng.uniform(0.3, 1.0))
    cfg.lbx_delta, cfg.ubx_delta = float(-rng.uniform(0.25, 0.55)), float(rng.uniform(0.25, 0.55))
    cfg.zl, cfg.zu = float(rng.uniform(3, 30)), float(rng.uniform(3, 30))
    for f in ("mass", "L_F", "L_R", "Iz", "Cf", "Cr"):
        setattr(cfg, f, getattr(cfg, f) * float(rng.uniform(0.7, 1.3)))
    assert all(cfg.W[c] == 0.0 and cfg.We[c] == 0.0 for c in range(3, 7)) and cfg.W[0] != cfg.W[1]
    return cfg


@pytest.mark.parametrize("N", [13, 20, 40, 60, 80])
def test_randomised_problem_data(gpu_engine_factory, oracle_omp, N):
    """Five random problem descriptions per horizon (weights, asymmetric bounds and slack penalties, sampling time, terminal scale,
    vehicle parameters), 96 scenarios each, against the oracle: the general-weight instantiation of kernel F at N = 20 and of kernel S
    at N = 40, 60 and 80, kernel R at N = 13.  Same statuses and iteration counts, 1e-8 / 1e-7."""
    rng = np.random.default_rng(100 + N)
    for trial in range(5):
        cfg = _random_problem(rng, N)
        s = random_scenarios(96, N=N, seed=int(rng.integers(1 << 30)), blend=(3.0, 5.0))
        g, o = _solve_both(gpu_engine_factory(cfg), oracle_omp, cfg, s, nthreads=8)
        assert (o[3] == 0).mean() >= 0.9
        _assert_parity(g, o, tol_for(N))


def test_bitwise_repeatability(gpu_engine_factory):
    """Instances are independent and every wave's arithmetic is fixed, so repeated solves must agree bit for bit -- for any
    batch size and whatever the scheduler's draw order.  Small batches matter: a wave that is alone on its SIMD gets no
    accidental wait states from a neighbour, which is how an instruction hazard inside the hand-written assembly (a v_readlane
    directly behind the v_fma_f64 that writes its source) once showed up as 1e-15 run-to-run noise."""
    cfg = default_config(N=20)
    for B, seed in ((6, 3), (40, 5), (700, 7)):
        s = random_scenarios(B, N=20, seed=seed, blend=(3.0, 5.0))
        eng = gpu_engine_factory(cfg)
        ref = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
        for _ in range(25):
            g = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
            for a, b in zip(g, ref):
                np.testing.assert_array_equal(a, b)


def test_ordered_batches_on_one_handle_are_draw_order_free(gpu_engine_factory, oracle_omp):
    """More instances than persistent waves (B > 8 per CU): the work-order pre-pass, the ticket counter, the per-wave table of the bin
    counts and the ticket drawn ahead under the expansion are all in play.  DIFFERENT batches solved one after another on ONE handle (the
    two scheduler states alternate, nothing of a launch may leak into the next) must each give the bits a fresh handle gives, run after
    run, and the oracle's answer."""
    cfg = default_config(N=20)
    eng = gpu_engine_factory(cfg)
    for B, seed, blend in ((2500, 11, (3.0, 5.0)), (4096, 12, (100.0, 110.0)), (2049, 13, (3.0, 5.0)), (5000, 14, (100.0, 110.0))):
        s = random_scenarios(B, N=20, seed=seed, blend=blend)
        args = (s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
        g = eng.solve_numpy(*args)
        fresh = gpu_engine_factory(cfg).solve_numpy(*args)
        again = eng.solve_numpy(*args)
        for a, b, c in zip(g, fresh, again):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a, c)
        if B == 2500:
            o = oracle_omp.solve_batch(cfg, *args, nthreads=16)
            _assert_parity(g, o, tol_for(20))


@pytest.mark.parametrize("N,B", [(24, 300), (40, 64), (40, 1500), (64, 600), (20, 5000)])
def test_row_kernel_repeatable_and_ticket_order_free(gpu_engine_factory, oracle_omp, N, B, monkeypatch):
    """Kernel R draws quadruples of instances from a ticket counter and runs one to four instances per wave depending on the
    batch: more instances than resident row slots must give the same bits as any other draw order, run after run, and the
    oracle's answer.  (N = 20 forced onto kernel R as well.)"""
    monkeypatch.setenv("ADMPC_QP", "riccati")
    cfg = default_config(N=N)
    s = random_scenarios(B, N=N, seed=77, blend=(3.0, 5.0))
    eng = gpu_engine_factory(cfg)
    ref = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    for _ in range(4):
        g = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
        for a, b in zip(g, ref):
            np.testing.assert_array_equal(a, b)
    o = oracle_omp.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], nthreads=16)
    _assert_parity(ref, o, tol_for(N))


@pytest.mark.parametrize("N", [2, 3, 7, 19, 21, 27, 28, 32, 33, 40, 45, 46, 64, 65, 80, 96, 97, 128])
def test_horizon_sweep_row_kernel(gpu_engine_factory, oracle_omp, N, monkeypatch):
    """(Round 4: N = 40 / 60 / 80 run the segmented condensed kernel by default -- tests/test_seg_gpu.py; this sweep keeps kernel R at
    those horizons too, ADMPC_QP=riccati.)
    Every horizon class of kernel R (odd and even, the LDS budgets of 4, 2 and 1 instances per wave, the maximum N = 128):
    status and iteration counts equal to the oracle's for every instance, solutions within the stated tolerance, bit-wise
    repeatable.  (The former scripts/sweep_horizons.py, now a test; the old stage-wise kernel this replaces gave run-to-run
    different results on some of these horizons.)"""
    B = 600 if N <= 46 else (200 if N <= 80 else 64)
    monkeypatch.setenv("ADMPC_QP", "riccati")
    cfg = default_config(N=N)
    s = random_scenarios(B, N=N, seed=1000 + N, blend=(3.0, 5.0))
    eng = gpu_engine_factory(cfg)
    g = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    g2 = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    for a, b in zip(g, g2):
        np.testing.assert_array_equal(a, b)
    o = oracle_omp.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], nthreads=16)
    assert (o[3] == 0).all()
    _assert_parity(g, o, tol_for(N))


def test_full_size_n40_b4096_every_instance(gpu_engine_factory, oracle_omp):
    """The reference's shipped horizon (launch/gp_ad_mpc.launch:6-7, N = 40, T = 2 s) at the full batch size: every one of
    the 4096 instances against the oracle."""
    cfg = default_config(N=40)
    s = random_scenarios(4096, N=40, seed=1234, blend=(3.0, 5.0))
    g = gpu_engine_factory(cfg).solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    o = oracle_omp.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], nthreads=16)
    assert (o[3] == 0).all() and g[4].max() < cfg.ipm_iter_max
    _assert_parity(g, o, TOL_LONG)


def test_full_size_shard_8192_every_instance(gpu_engine_factory, oracle_omp):
    """BASELINE configs[3] on one of its eight GPUs: the 8192-instance shard of the 65536 scenarios (shard 5), N = 20, every
    instance against the oracle; the generator gives instance i the same data whatever the sharding."""
    from ad_mpc_amd.dist import shard_range
    cfg = default_config(N=20)
    lo, hi = shard_range(65536, 5, 8)
    assert hi - lo == 8192
    s = random_scenarios(hi - lo, N=20, seed=1234, start=lo)
    g = gpu_engine_factory(cfg).solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    o = oracle_omp.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], nthreads=16)
    assert (o[3] == 0).all()
    _assert_parity(g, o, TOL)


def test_fp32_config5_full_size(gpu_engine_factory, oracle_omp):
    """BASELINE configs[4]: N = 80, B = 16384, fp32 storage and arithmetic, against the fp64 oracle: identical status, every
    instance converged before iter_max, |u - u_oracle| <= 1.5e-3 absolute at worst and <= 5e-4 for 99 % of the instances (inputs range over
    [-10, 5], states over tens of metres), costs to 1e-3 relative; bit-wise repeatable."""
    N, B = 80, 16384
    cfg = default_config(N=N)
    s = random_scenarios(B, N=N, seed=1234)
    eng = gpu_engine_factory(cfg)
    g = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], dtype=np.float32)
    g2 = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], dtype=np.float32)
    for a, b in zip(g, g2):
        np.testing.assert_array_equal(a, b)
    o = oracle_omp.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], nthreads=16)
    np.testing.assert_array_equal(g[3], o[3])
    assert (g[3] == 0).all()
    assert g[4].max() < cfg.ipm_iter_max and o[4].max() < cfg.ipm_iter_max
    # measured on this batch: max 7.1e-4, 99.9 % of the instances within 4.9e-4, 99 % within 2.3e-4 (inputs), states 2.2e-4 -- asserted with a
    # factor 2; over twelve more batches of the same size (scripts/census_f32_margin.py, 196 608 instances) the quantiles are the same and
    # the single worst instance is 1.78e-3, which is what the 2.5e-3 of DESIGN section 9 bounds with 40 % to spare
    du = np.abs(g[1] - o[1]).max(axis=(1, 2))
    assert du.max() <= 1.5e-3 and np.quantile(du, 0.999) <= 1e-3 and np.quantile(du, 0.99) <= 5e-4, (du.max(), np.quantile(du, 0.999), np.quantile(du, 0.99))
    assert np.abs(g[0] - o[0]).max() <= 1e-3, np.abs(g[0] - o[0]).max()
    np.testing.assert_allclose(g[2], o[2], rtol=1e-3)
    np.testing.assert_array_equal(g[0][:, 0, :], s["x0"].astype(np.float32))          # x_0 pinned to the measured state
    assert np.abs(g[0][:, 1:N, 6]).max() <= 0.52 + 2e-3                                # steering inside its hard bound


@pytest.mark.parametrize("N,blend", [(20, (3.0, 5.0)), (40, (100.0, 110.0)), (5, (3.0, 5.0))])
def test_fp32_small_cases(gpu_engine_factory, oracle, N, blend):
    """fp32 path on small batches of both model branches (p = 1 dynamic, p = 0 kinematic where the fp32 build drops the
    1e-99-guarded dynamic terms), tolerance as above."""
    cfg = default_config(N=N)
    s = random_scenarios(96, N=N, seed=1234, blend=blend)
    g = gpu_engine_factory(cfg).solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], dtype=np.float32)
    o = oracle.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    np.testing.assert_array_equal(g[3], o[3])
    assert np.abs(g[1] - o[1]).max() <= 2e-3 and np.abs(g[0] - o[0]).max() <= 2e-3


def test_mehrotra_limit_cycle_instance(gpu_engine_factory, oracle):
    """Scenario 10474 of the config-5 batch drove the unguarded predictor-corrector into a limit cycle (mu with period 4 until
    iter_max = 50, in the oracle and on the device alike).  With the centring safeguard (ADMPC_IPM_BLOCKED_STEP, include/admpc.h)
    it converges in 14 iterations: same count and same answer on the device, fp64 and fp32."""
    N = 80
    cfg = default_config(N=N)
    s = random_scenarios(1, N=N, seed=1234, start=10474)
    eng = gpu_engine_factory(cfg)
    g = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    o = oracle.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    assert o[3][0] == 0 and o[4][0] < 20
    _assert_parity(g, o, TOL_LONG)
    g32 = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], dtype=np.float32)
    assert g32[3][0] == 0 and g32[4][0] < 30 and np.abs(g32[1] - o[1]).max() <= 2e-3


def test_full_size_batch_4096(gpu_engine_factory, oracle):
    """BASELINE configs[1] at full size: direct parity for every instance plus size-independent properties."""
    cfg = default_config(N=20)
    s = random_scenarios(4096, N=20, seed=1234)
    eng = gpu_engine_factory(cfg)
    g, o = _solve_both(eng, oracle, cfg, s)
    assert (g[3] == 0).all()
    _assert_parity(g, o)
    x, u = g[0], g[1]
    # property 1: x_0 is pinned to the measured state; steering stays inside its hard bound on stages 1..N-1
    np.testing.assert_array_equal(x[:, 0, :], s["x0"])
    assert np.abs(x[:, 1:20, 6]).max() <= 0.52 + 1e-8
    # property 2: the step reduces the objective of the (already feasible) initial iterate? not guaranteed for RTI;
    # instead: idempotence at convergence -- after 30 more full SQP steps one further RTI step is a no-op
    cfg2 = cfg.copy(); cfg2.sqp_iters = 30
    eng2 = gpu_engine_factory(cfg2)
    xc, uc, cc, sc, _ = eng2.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], x, u)
    ok = sc == 0
    assert ok.all()
    x1, u1, c1, s1, _ = eng.solve_numpy(s["x0"][ok], s["yref"][ok], s["yref_e"][ok], s["p"][ok], xc[ok], uc[ok])
    conv = np.abs(u1 - uc[ok]).reshape(ok.sum(), -1).max(1)
    assert conv.max() < 1e-6 and np.quantile(conv, 0.99) < 1e-8
    # property 3: a converged iterate satisfies the nonlinear dynamics (multiple-shooting gaps closed)
    import torch
    phi, _, _ = eng.shoot(eng.to_device(x1), eng.to_device(u1), eng.to_device(s["p"][ok]))
    torch.cuda.synchronize()
    gaps = np.abs(phi.cpu().numpy() - x1[:, 1:, :]).reshape(ok.sum(), -1).max(1)
    assert gaps.max() < 1e-6 and np.quantile(gaps, 0.99) < 1e-8


def test_kat_acados_iterate_on_gpu(gpu_engine_factory, golden_kat):
    """Solver pin on the GPU: the reference's converged acados iterate is a fixed point of one RTI step and the
    limit of a cold-started SQP."""
    k = golden_kat
    N = k["N"]
    cfg = default_config(N=N, Ts=k["Ts"], terminal_scale=k["terminal_scale"])
    X, U = np.array(k["X"]), np.array(k["U"])
    x0, yref, ye = np.array(k["x0"]), np.array(k["yref"]), np.array(k["yref_e"])
    eng = gpu_engine_factory(cfg)
    x, u, cost, st, it = eng.solve_numpy(x0[None], yref[None], ye[None], np.array([0.0]), X[None], U[None])
    assert st[0] == 0 and np.abs(u[0] - U).max() < 1e-8 and np.abs(x[0] - X).max() < 1e-8
    assert abs(cost[0] - 11.5810534473) < 1e-8
    cfg2 = cfg.copy(); cfg2.sqp_iters = 15
    x, u, cost, st, it = gpu_engine_factory(cfg2).solve_numpy(x0[None], yref[None], ye[None], np.array([0.0]),
                                                              np.zeros((1, N + 1, 7)), np.zeros((1, N, 2)))
    assert st[0] == 0 and np.abs(u[0] - U).max() < 1e-8 and np.abs(x[0] - X).max() < 1e-8


def test_second_stored_iterate_dynamic_branch_on_gpu(gpu_engine_factory, oracle, golden_kat_mid_rti):
    """The reference's second stored acados iterate (solve_iteration.json, dynamic branch) on the device path, with the statement
    of tests/test_oracle_solver.py::_mid_rti_statement, and equal to the oracle on the same inputs to 1e-7."""
    from test_oracle_solver import _mid_rti_statement
    k = golden_kat_mid_rti
    _, u = _mid_rti_statement(lambda cfg, *a: gpu_engine_factory(cfg).solve_numpy(*a), k)
    cfg = default_config(N=k["N"], Ts=k["Ts"], terminal_scale=k["terminal_scale"]); cfg.sqp_iters = 30
    o = oracle.solve_batch(cfg, np.array(k["x0"])[None], np.array(k["yref"])[None], np.array(k["yref_e"])[None], np.array([k["p"]]),
                           np.array(k["X"])[None], np.array(k["U"])[None])
    assert np.abs(u - o[1]).max() <= 1e-7


@pytest.mark.parametrize("tight", [True, False])
@pytest.mark.parametrize("N,B", [(20, 48), (40, 32), (80, 16)])
def test_kkt_residuals_of_the_device_output(gpu_engine_factory, N, B, tight):
    """Optimality evidence on the DEVICE output, independent of any CPU solver: the step and the multipliers that
    admpc_solve_batch_ex returns (pi, slacks, inequality multipliers) satisfy the KKT conditions of the QP of the RTI step --
    linearised dynamics, stationarity in states / inputs / slack variables, primal and dual feasibility, complementarity --
    evaluated in numpy (tests/kkt_check.py) with the linearisation the device's own shooting entry returns.  The QP is strictly
    convex in the inputs, so a KKT point IS its minimiser."""
    import torch
    from kkt_check import kkt_residuals_from_multipliers
    cfg = tight_config(N=N) if tight else default_config(N=N)          # tight levels of rounds 1-2 / the reference's (HPIPM BALANCE: 1e-8)
    s = random_scenarios(B, N=N, seed=77, blend=(3.0, 5.0))
    eng = gpu_engine_factory(cfg)
    d = eng.to_device
    xb, ub = d(s["xbar"]).clone(), d(s["ubar"]).clone()
    phi, A, Bm = eng.shoot(d(s["xbar"]), d(s["ubar"]), d(s["p"]))
    st = torch.empty(B, dtype=torch.int32, device=eng.device); it = torch.empty_like(st)
    pi, ineq = eng.solve_with_multipliers(d(s["x0"]), d(s["yref"]), d(s["yref_e"]), d(s["p"]), xb, ub, None, st, it)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and (it.cpu().numpy() > 0).sum() >= B // 4          # the interior point really ran
    phi, A, Bm, xn, un, pi, ineq = (t.cpu().numpy() for t in (phi, A, Bm, xb, ub, pi, ineq))
    worst = {}
    for i in range(B):
        r = kkt_residuals_from_multipliers(cfg, s["x0"][i], s["yref"][i], s["yref_e"][i], s["xbar"][i], s["ubar"][i], A[i], Bm[i], phi[i],
                                           xn[i], un[i], pi[i], ineq[i])
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), float(v))
    tol = 1e-7 if N <= 40 else 1e-6
    assert worst["dyn"] <= 1e-9 and worst["x0"] <= 1e-12, worst
    for k in ("stat_x", "stat_x0", "stat_u", "stat_s", "slack_consistency", "prim", "dual"):
        assert worst[k] <= tol, (k, worst)
    assert worst["comp"] <= (1e-9 if tight else 1e-8), worst


def test_gp_residual_config3(gpu_engine_factory, oracle):
    cfg = default_config(N=20); set_gp(cfg, grid_gp())
    s = random_scenarios(256, N=20, seed=1234, blend=(3.0, 5.0))
    g, o = _solve_both(gpu_engine_factory(cfg), oracle, cfg, s)
    _assert_parity(g, o)
    base = oracle.solve_batch(default_config(N=20), s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    assert np.abs(base[1] - o[1]).max() > 1e-3       # the GP really changes the answer


def test_gp_residual_config3_full_size(gpu_engine_factory, oracle_omp):
    """BASELINE configs[2] at its full size: batch 4096 with the GP residual-dynamics correction active (grid_gp: three 1-D
    regressors on v_x, v_y, psi_dot), every instance against the oracle on OpenMP threads -- identical status and interior-point
    iteration counts, solutions within 1e-8 -- for the shipped blend speeds (kinematic branch) and for the 3 / 5 m/s blend that
    switches the dynamic bicycle branch on."""
    cfg = default_config(N=20); set_gp(cfg, grid_gp())
    eng = gpu_engine_factory(cfg)
    for kw in ({}, {"blend": (3.0, 5.0)}):
        s = random_scenarios(4096, N=20, seed=1234, **kw)
        g, o = _solve_both(eng, oracle_omp, cfg, s, nthreads=16)
        assert (o[3] == 0).all()
        _assert_parity(g, o)


def test_gp_residual_at_the_shipped_horizon(gpu_engine_factory, oracle_omp):
    """N = 40 (the reference's shipped horizon) WITH the GP residual: the one family whose states sit above the 1e-7 of the other
    long-horizon tests, with its own stated tolerance: inputs <= 1e-7, states <= 1e-5, identical statuses and
    iteration counts.  The GP-augmented linearised dynamics has an unstable lateral mode: the expansion x_{k+1} = A_k dx_k + B_k du_k + b_k
    amplifies the rounding-level disagreement of the inputs (1e-10 .. 1e-11) by ~1e5 over 40 stages; the worst entry is always v_y at the
    last stage (profiles/r3/gp_n40_state_amplification.txt: 2.4e-6 over five seeds).  A condition number of the expansion, in the
    reference's own formulation as much as here -- stated, not hidden.  The device path is kernel R: with GP residuals in the model the
    segmented condensed kernel is not the default at N = 40 (eliminating 20 stages at a time through such dynamics costs digits the
    stage-wise recursion keeps: 3e-6 in the inputs on this batch -- admpc_create)."""
    cfg = default_config(N=40); set_gp(cfg, grid_gp())
    s = random_scenarios(4096, N=40, seed=100)
    o = oracle_omp.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], nthreads=16)
    assert (o[3] == 0).all()
    for qp in (None, "riccati"):                      # the default IS kernel R here: bit-identical results
        if qp: os.environ["ADMPC_QP"] = qp
        try:
            g = gpu_engine_factory(cfg).solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
        finally:
            os.environ.pop("ADMPC_QP", None)
        if qp is None: g_default = g
        else: np.testing.assert_array_equal(g[1], g_default[1])
        np.testing.assert_array_equal(g[3], o[3]); np.testing.assert_array_equal(g[4], o[4])
        du = np.abs(g[1] - o[1]).max(); dx = np.abs(g[0] - o[0]).max()
        assert du <= 1e-7 and dx <= 1e-5, (qp, du, dx)
        worst = np.unravel_index(np.argmax(np.abs(g[0] - o[0])), g[0].shape)
        assert dx <= 1e-7 or worst[1] >= 30, worst             # what exceeds the plain tolerance sits at the end of the horizon


def _multi_feature_gps(seed=8):
    """Three regressors with 3, 2 and 1 features (states and inputs mixed, one length scale per feature)."""
    rng = np.random.default_rng(seed)
    Z3 = np.c_[rng.uniform(2, 14, 28), rng.uniform(-0.3, 0.3, 28), rng.uniform(-4, 4, 28)]
    Z2 = np.c_[rng.uniform(-0.5, 0.5, 20), rng.uniform(-0.5, 0.5, 20)]
    return [dict(feat=[3, 6, 7], out=3, Z=Z3, alpha=0.15 * rng.standard_normal(28), length_scale=[2.5, 0.25, 2.0], sigma_f=0.9, ymean=0.02),
            dict(feat=[4, 8], out=4, Z=Z2, alpha=0.1 * rng.standard_normal(20), length_scale=[0.3, 0.4], sigma_f=1.1, ymean=-0.01),
            dict(feat=5, out=5, Z=np.linspace(-0.4, 0.4, 16), alpha=0.1 * rng.standard_normal(16), length_scale=0.2, sigma_f=1.0, ymean=0.0)]


@pytest.mark.parametrize("N", [20, 40])
def test_multi_feature_gp_residual(gpu_engine_factory, oracle_omp, N):
    """Residual GPs over up to three features with an anisotropic length scale (gp.py:81-138): shooting (state, A, B) against the
    oracle's RK4 with analytic GP gradients at 1e-11 relative, then the solve on the condensed pipeline (N = 20) and kernel R (N = 40)."""
    import torch
    cfg = default_config(N=N); set_gp(cfg, _multi_feature_gps())
    s = random_scenarios(128, N=N, seed=77, blend=(3.0, 5.0))
    eng = gpu_engine_factory(cfg)
    phi, A, Bm = eng.shoot(eng.to_device(s["xbar"]), eng.to_device(s["ubar"]), eng.to_device(s["p"]))
    torch.cuda.synchronize()
    phi, A, Bm = phi.cpu().numpy(), A.cpu().numpy(), Bm.cpu().numpy()
    for b in range(0, 128, 17):
        for k in (0, N // 2, N - 1):
            po, Ao, Bo = oracle_omp.rk4_sens(cfg, s["xbar"][b, k], s["ubar"][b, k], s["p"][b], cfg.Ts)
            for got, ref in ((phi[b, k], po), (A[b, k], Ao), (Bm[b, k], Bo)):
                assert np.abs(got - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max())
    g, o = _solve_both(eng, oracle_omp, cfg, s, nthreads=8)
    _assert_parity(g, o, tol_for(N))
    base = oracle_omp.solve_batch(default_config(N=N), s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], nthreads=8)
    assert np.abs(base[1] - o[1]).max() > 1e-3       # the GPs really change the answer


def test_active_slack_and_steering_bound(gpu_engine_factory, oracle):
    cfg = default_config()
    x0, xref, uref = straight_scenario(N=cfg.N, Ts=cfg.Ts, v=5.0)
    rows = []
    for y, d0, v in [(-10.0, 0.5, 3.0), (6.0, 0.5, 14.0), (4.0, -0.5, 6.0), (-6.0, 0.5, 14.0), (0.0, 0.6, 5.0), (0.0, -0.7, 9.0)]:
        x = x0.copy(); x[1] = y; x[6] = d0; x[3] = v; rows.append(x)
    X0 = np.array(rows); B = len(rows)
    s = assemble(X0, np.repeat(xref[None], B, 0), np.repeat(uref[None], B, 0))
    g, o = _solve_both(gpu_engine_factory(cfg), oracle, cfg, s)
    _assert_parity(g, o)
    assert (g[1][:, :, 0] > 5.0 + 1.0).any()                       # soft bound violated through the slack
    assert np.abs(g[0][:, 1:20, 6]).max() <= 0.52 + 1e-8           # hard bound respected, even from an infeasible x0


def test_failure_status_and_untouched_iterate(gpu_engine_factory, oracle):
    cfg = default_config()
    s = random_scenarios(8, seed=3, blend=(3.0, 5.0), init="zeros")
    g, o = _solve_both(gpu_engine_factory(cfg), oracle, cfg, s)
    np.testing.assert_array_equal(g[3], o[3])
    bad = g[3] != 0
    assert bad.any() and (g[3][bad] == 4).all() and np.isinf(g[2][bad]).all()
    np.testing.assert_array_equal(g[0][bad], s["xbar"][bad]); np.testing.assert_array_equal(g[1][bad], s["ubar"][bad])


def test_odd_batch_sizes_and_mixed_failures_over_sqp_iterations(gpu_engine_factory, oracle):
    """Batch sizes around the wave / persistent-grid boundaries (1, 63..65, just above 2048 = one instance per resident wave),
    and a three-step SQP in which some instances fail in the first step: they must be skipped by every later kernel
    (linearise, condense, interior point, expand), keep status 4 / cost inf / their iterate, and not disturb the others."""
    cfg = default_config(N=20)
    for B in (1, 63, 64, 65, 2049, 2500):
        s = random_scenarios(B, N=20, seed=100 + B, blend=(3.0, 5.0))
        g, o = _solve_both(gpu_engine_factory(cfg), oracle, cfg, s)
        assert (g[3] == 0).all()
        _assert_parity(g, o)
    cfg3 = default_config(N=20, sqp_iters=3)
    good = random_scenarios(40, N=20, seed=11, blend=(3.0, 5.0))
    bad = random_scenarios(8, N=20, seed=3, blend=(3.0, 5.0), init="zeros")            # zeros iterate with p > 0: non-finite model
    s = {k: np.concatenate([good[k][:20], bad[k], good[k][20:]]) for k in good}
    g, o = _solve_both(gpu_engine_factory(cfg3), oracle, cfg3, s)
    np.testing.assert_array_equal(g[3], o[3])
    failed = g[3] != 0
    assert failed.any() and (~failed).sum() >= 40
    assert np.isinf(g[2][failed]).all()
    np.testing.assert_array_equal(g[0][failed], s["xbar"][failed]); np.testing.assert_array_equal(g[1][failed], s["ubar"][failed])
    ok = ~failed
    assert np.abs(g[1][ok] - o[1][ok]).max() <= 1e-7 and np.abs(g[0][ok] - o[0][ok]).max() <= 1e-7


def test_one_engine_growing_and_shrinking_batches(gpu_engine_factory, oracle):
    """The workspace (linearisation, Hessians, scheduler lists) is sized by the largest batch seen; a solver handle must give
    the same answers when batches grow and shrink between calls."""
    cfg = default_config(N=20)
    eng = gpu_engine_factory(cfg)
    for B in (40, 3000, 7, 4500, 300):
        s = random_scenarios(B, N=20, seed=500 + B, blend=(3.0, 5.0))
        g = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
        o = oracle.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
        _assert_parity(g, o)


@pytest.mark.parametrize("N,split", [(20, None), (40, "1")])
def test_solve_is_capturable_in_a_hip_graph(gpu_engine_factory, monkeypatch, N, split):
    """admpc_solve_batch is launches only (no allocation, no copy, no synchronisation after admpc_reserve): it can be
    captured into a hipGraph on the caller's stream and replayed; the replay reproduces the eager result bit for bit.
    N = 20: the four kernels of the condensed pipeline; N = 40 with the split forced: linearise, trial launch, sort, second launch."""
    import torch
    if split: monkeypatch.setenv("ADMPC_ROWQP_SPLIT", split)
    cfg = default_config(N=N)
    s = random_scenarios(300, N=N, seed=21, blend=(3.0, 5.0))
    eng = gpu_engine_factory(cfg)
    d = eng.to_device
    x0, yref, yref_e, p = d(s["x0"]), d(s["yref"]), d(s["yref_e"]), d(s["p"])
    xb0, ub0 = d(s["xbar"]), d(s["ubar"])
    xb, ub = xb0.clone(), ub0.clone()
    cost = torch.empty(300, dtype=torch.float64, device=eng.device)
    st = torch.empty(300, dtype=torch.int32, device=eng.device); it = torch.empty_like(st)
    eng.solve(x0, yref, yref_e, p, xb, ub, cost, st, it)              # eager (also reserves the workspace)
    torch.cuda.synchronize()
    ref = (xb.clone(), ub.clone(), cost.clone(), st.clone(), it.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    xb.copy_(xb0); ub.copy_(ub0)
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.solve(x0, yref, yref_e, p, xb, ub, cost, st, it)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        xb.copy_(xb0); ub.copy_(ub0); cost.zero_(); st.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip((xb, ub, cost, st, it), ref):
            assert torch.equal(a, b)


@pytest.mark.parametrize("N", [20, 40])
def test_two_handles_on_two_streams(gpu_engine_factory, N):
    """One solve in flight per handle -- two handles, two streams: independent batches overlap on the device (the second fills the tail of
    the first; bench.py's `two_in_flight`) and every result is bit-identical to the same solves issued one after the other."""
    import torch
    cfg = default_config(N=N)
    B = 1500
    sc = [random_scenarios(B, N=N, seed=300 + i, blend=(3.0, 5.0)) for i in range(4)]
    e0, e1 = gpu_engine_factory(cfg), gpu_engine_factory(cfg)
    ref = [e0.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"]) for s in sc]
    d = e0.to_device
    dev = [[d(s[k]) for k in ("x0", "yref", "yref_e", "p", "xbar", "ubar")] for s in sc]
    outs = [(torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")) for _ in sc]
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    torch.cuda.synchronize()
    for i, a in enumerate(dev):
        with torch.cuda.stream(streams[i & 1]):
            (e0, e1)[i & 1].solve(a[0], a[1], a[2], a[3], a[4], a[5], *outs[i])
    torch.cuda.synchronize()
    for i, a in enumerate(dev):
        got = (a[4].cpu().numpy(), a[5].cpu().numpy(), outs[i][0].cpu().numpy(), outs[i][1].cpu().numpy(), outs[i][2].cpu().numpy())
        for g, r in zip(got, ref[i]):
            np.testing.assert_array_equal(g, r)


def test_batches_beyond_4_gb_are_solved_in_chunks(gpu_engine_factory, monkeypatch):
    """Kernel R addresses its arrays with 32-bit offsets; the library used to refuse batches whose largest array passes 4 GB
    ("split it").  Now it splits them itself.  (a) A forced chunk size (ADMPC_ROWQP_CHUNK) gives the bits of the one-launch solve, fp64
    with multipliers and fp32, odd sizes, converged SQP; (b) a real N = 128 batch of 101 000 instances (4.4 GB of linearisation)
    equals the solves of its two halves, bit for bit, and every instance converges."""
    import torch
    for N, B, chunk in ((40, 1000, 333), (24, 257, 64)):
        cfg = default_config(N=N, sqp_iters=3, sqp_tol=1e-9)
        s = random_scenarios(B, N=N, seed=61, blend=(3.0, 5.0))
        ref = gpu_engine_factory(cfg).solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
        ref32 = gpu_engine_factory(cfg).solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], dtype=np.float32)
        monkeypatch.setenv("ADMPC_ROWQP_CHUNK", str(chunk))
        eng = gpu_engine_factory(cfg)
        got = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
        got32 = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], dtype=np.float32)
        d = eng.to_device
        xb, ub = d(s["xbar"]).clone(), d(s["ubar"]).clone()
        pi, ineq = eng.solve_with_multipliers(d(s["x0"]), d(s["yref"]), d(s["yref_e"]), d(s["p"]), xb, ub)
        monkeypatch.delenv("ADMPC_ROWQP_CHUNK")
        xb1, ub1 = d(s["xbar"]).clone(), d(s["ubar"]).clone()
        pi1, ineq1 = gpu_engine_factory(cfg).solve_with_multipliers(d(s["x0"]), d(s["yref"]), d(s["yref_e"]), d(s["p"]), xb1, ub1)
        torch.cuda.synchronize()
        for a, b in zip(got + got32, ref + ref32):
            np.testing.assert_array_equal(a, b)
        ok = torch.as_tensor(got[3] != 4, device=eng.device)          # a failed instance has no multipliers (its records stay unwritten)
        assert int(ok.sum()) >= B - B // 50
        assert torch.equal(pi[ok], pi1[ok]) and torch.equal(ineq[ok], ineq1[ok]) and torch.equal(xb, xb1)
    N, B = 128, 101000
    cfg = default_config(N=N)
    eng = gpu_engine_factory(cfg)
    assert B * (N + 1) * 42 * 8 > 2 ** 32
    base = random_scenarios(1000, N=N, seed=62)
    rep = lambda a: torch.as_tensor(a, device=eng.device).repeat((B // 1000,) + (1,) * (a.ndim - 1)).contiguous()
    t = {k: rep(base[k]) for k in ("x0", "yref", "yref_e", "p", "xbar", "ubar")}
    t["p"] = t["p"] * 0.0 + torch.linspace(0.0, 1.0, B, device=eng.device, dtype=torch.float64)        # every instance its own blend: no two alike
    xb, ub = t["xbar"].clone(), t["ubar"].clone()
    st = torch.empty(B, dtype=torch.int32, device=eng.device); it = torch.empty_like(st); cost = torch.empty(B, dtype=torch.float64, device=eng.device)
    eng.solve(t["x0"], t["yref"], t["yref_e"], t["p"], xb, ub, cost, st, it)
    h = B // 2
    for lo, hi in ((0, h), (h, B)):
        xh, uh = t["xbar"][lo:hi].clone(), t["ubar"][lo:hi].clone()
        sh = torch.empty(hi - lo, dtype=torch.int32, device=eng.device); ih = torch.empty_like(sh); ch = torch.empty(hi - lo, dtype=torch.float64, device=eng.device)
        eng.solve(t["x0"][lo:hi].contiguous(), t["yref"][lo:hi].contiguous(), t["yref_e"][lo:hi].contiguous(), t["p"][lo:hi].contiguous(), xh, uh, ch, sh, ih)
        torch.cuda.synchronize()
        assert torch.equal(xh, xb[lo:hi]) and torch.equal(uh, ub[lo:hi]) and torch.equal(sh, st[lo:hi]) and torch.equal(ih, it[lo:hi]) and torch.equal(ch, cost[lo:hi])
    assert int((st != 0).sum()) == 0 and int(it.max()) < cfg.ipm_iter_max + 30          # nobody runs out of iterations (fallback budget included)


def test_empty_batch_and_argument_errors(gpu_engine_factory):
    import torch
    from ad_mpc_amd import _lib
    cfg = default_config()
    eng = gpu_engine_factory(cfg)
    L = eng.lib
    z = C.c_void_p(0)
    assert L.admpc_solve_batch(eng._h, 0, z, z, z, z, z, z, z, z, z, z) == 0            # B = 0 is a no-op
    assert L.admpc_solve_batch(eng._h, 4, z, z, z, z, z, z, z, z, z, z) == -1           # null arrays -> EINVAL
    assert b"null" in L.admpc_last_error()
    assert L.admpc_solve_batch(eng._h, -1, z, z, z, z, z, z, z, z, z, z) == -1
    bad = cfg.copy(); bad.N = 1
    h = C.c_void_p(0)
    assert L.admpc_create(C.byref(bad), 0, C.byref(h)) == -1
    bad = cfg.copy(); bad.n_gp = 1; bad.gp[0].out = 0; bad.gp[0].n_feat = 1; bad.gp[0].feat[0] = 3
    assert L.admpc_create(C.byref(bad), 0, C.byref(h)) == -1
    assert L.admpc_create(C.byref(cfg), 99, C.byref(h)) == -2                           # no such device
    with pytest.raises(ValueError):
        eng.solve(torch.zeros(3, 7), torch.zeros(3, 20, 9), torch.zeros(3, 7), torch.zeros(3), torch.zeros(3, 21, 7), torch.zeros(3, 20, 2))


def test_two_level_argmin_through_a_process_group(gpu_engine_factory):
    """The N-GPU arg-min path of bench.py / config 4 on the one GPU of the box: admpc_argmin into a 16-byte record,
    all-gather (RCCL, one rank), admpc_argmin_pairs; and the second level alone on hand-made records of 8 'ranks'."""
    import torch
    import torch.distributed as dist
    from ad_mpc_amd import dist as adist
    eng = gpu_engine_factory(default_config())
    rng = np.random.default_rng(3)
    cost = rng.uniform(1.0, 2.0, size=5000); cost[[17, 4000]] = 0.5; cost[100] = np.nan
    tc = eng.to_device(cost)
    pair = eng.argmin_pair(tc, index_offset=70000)
    assert adist.unpack_pair(pair) == (0.5, 70017)
    vals = np.array([3.0, np.nan, 1.25, 7.0, 1.25, np.inf, 2.0, 1.25])
    idxs = np.array([5, 1, 900, 3, 40, 2, 6, 41], dtype=np.int64)
    rec = np.stack([vals, idxs.view(np.float64)], axis=1)
    assert adist.unpack_pair(eng.argmin_pairs(eng.to_device(rec))) == (1.25, 40)
    allbad = np.stack([np.full(3, np.nan), np.array([9, 4, 6], dtype=np.int64).view(np.float64)], axis=1)
    v, i = adist.unpack_pair(eng.argmin_pairs(eng.to_device(allbad)))
    assert v == np.inf and i == 4
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        out = adist.global_argmin_device(eng, tc, index_offset=70000)
        assert adist.unpack_pair(out) == (0.5, 70017)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("N", [20, 40])
def test_sqp_mode_stops_on_tolerance(gpu_engine_factory, oracle, N):
    """cfg.sqp_tol on the device (acados' residual test in front of every QP but the first; kernel R at both horizons): per-instance
    stop inside one admpc_solve_batch call, same statuses as the oracle (0 converged, 2 at the step limit, 4 failed), same iterates."""
    s = random_scenarios(48, N=N, seed=11, blend=(3.0, 5.0))
    bad = random_scenarios(4, N=N, seed=3, blend=(3.0, 5.0), init="zeros")          # non-finite model: status 4 in the first step
    s = {k: np.concatenate([s[k][:20], bad[k], s[k][20:]]) for k in s}
    good_idx = np.r_[0:20, 24:52]
    for iters in (30, 2):
        cfg = default_config(N=N, sqp_iters=iters, sqp_tol=1e-6)
        g, o = _solve_both(gpu_engine_factory(cfg), oracle, cfg, s)
        np.testing.assert_array_equal(g[3], o[3])
        assert set(np.unique(g[3][good_idx])) <= ({0, 4} if iters == 30 else {2, 4}) and (g[3][good_idx] != 4).sum() >= 40
        okm = g[3] != 4
        good = np.ones(len(okm), dtype=bool); good[20:24] = False      # the four non-finite-model instances carry garbage until they fail
        good &= okm & (np.abs(o[0]).max(axis=(1, 2)) < 1e3) & (np.abs(o[1]).max(axis=(1, 2)) < 1e3)   # full Newton steps without a line search
        assert good.sum() >= 40                                        # may diverge: finite garbage on both sides, not comparable
        assert np.abs(g[1][good] - o[1][good]).max() <= 1e-7 and np.abs(g[0][good] - o[0][good]).max() <= 1e-7
        assert np.isfinite(g[2][good]).all() and np.isinf(g[2][~okm]).all()
        first = ~okm & (o[0] == s["xbar"]).all(axis=(1, 2))          # failed in the very first step (in the oracle): iterate untouched
        np.testing.assert_array_equal(g[0][first], s["xbar"][first])
        if N == 20:
            assert first.sum() == (~okm).sum() == 4


@pytest.mark.parametrize("N", [20, 40])
def test_nlp_residuals_on_the_device_and_the_sqp_stop(gpu_engine_factory, oracle, N):
    """acados' SQP stopping test on the device (admpc_nlp_res_kernel behind admpc_nlp_residuals_batch and inside every SQP solve with a
    tolerance).  (a) After one RTI step the four residuals the device forms at the NEW iterate with the multipliers it returned equal
    the oracle's restatement on the same data, and an independent numpy statement with the device's own shooting; the dynamics rows
    really are non-zero there (the linearisation moved).  (b) A solve with sqp_tol stops exactly when they are within tolerance:
    status 0 <=> all four <= sqp_tol at the returned iterate with the returned multipliers; at the step limit (status 2) at least
    one is above."""
    import torch
    from kkt_check import nlp_residuals_numpy
    B = 64
    s = random_scenarios(B, N=N, seed=21, blend=(3.0, 5.0))
    cfg = default_config(N=N)
    eng = gpu_engine_factory(cfg)
    d = eng.to_device
    args = [d(s[k]) for k in ("x0", "yref", "yref_e", "p")]
    xb, ub = d(s["xbar"]).clone(), d(s["ubar"]).clone()
    st = torch.empty(B, dtype=torch.int32, device=eng.device)
    pi, ineq = eng.solve_with_multipliers(*args, xb, ub, None, st, None)
    res = eng.nlp_residuals(*args, xb, ub, pi, ineq)
    phi, A, Bm = eng.shoot(xb, ub, args[3])
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    res, xn, un, pin, iqn, phi, A, Bm = (t.cpu().numpy() for t in (res, xb, ub, pi, ineq, phi, A, Bm))
    for i in range(B):
        want = oracle.nlp_residuals(cfg, s["x0"][i], s["yref"][i], s["yref_e"][i], s["p"][i], xn[i], un[i], pin[i], iqn[i])
        assert np.all(np.abs(res[i] - want) <= 1e-9 * (1.0 + np.abs(want))), (i, res[i], want)
        if i < 8:
            ind = nlp_residuals_numpy(cfg, s["x0"][i], s["yref"][i], s["yref_e"][i], xn[i], un[i], A[i], Bm[i], phi[i], pin[i], iqn[i])
            assert np.all(np.abs(res[i] - ind) <= 1e-9 * (1.0 + np.abs(ind))), (i, res[i], ind)
    assert np.median(res[:, 0]) > 1e-6 and np.median(res[:, 1]) > 1e-6 and res[:, 2].max() <= 1e-7 and res[:, 3].max() <= 1e-7
    for iters, want_status in ((30, 0), (2, 2)):
        cfg2 = default_config(N=N, sqp_iters=iters, sqp_tol=1e-6)
        eng2 = gpu_engine_factory(cfg2)
        xb, ub = d(s["xbar"]).clone(), d(s["ubar"]).clone()
        pi, ineq = eng2.solve_with_multipliers(*args, xb, ub, None, st, None)
        res = eng2.nlp_residuals(*args, xb, ub, pi, ineq)
        torch.cuda.synchronize()
        stn, res = st.cpu().numpy(), res.cpu().numpy()
        ok = np.abs(xb.cpu().numpy()).max(axis=(1, 2)) < 1e3            # full Newton steps without a line search may diverge
        assert ok.sum() >= B - 8 and (stn[ok] == want_status).sum() >= ok.sum() - 4, (iters, np.unique(stn, return_counts=True))
        conv = res.max(axis=1) <= 1e-6
        assert conv[stn == 0].all()                                      # stopped <=> the test passed at the returned iterate
        if want_status == 2:
            assert (~conv[ok]).sum() >= ok.sum() - 4                     # two QPs do not get there (the last iterate is never tested: acados' loop)


def test_argmin_global_through_the_c_abi_with_an_rccl_communicator(gpu_engine_factory):
    """admpc_argmin_global: what a C++ host binds for the cross-GPU winner -- an ncclComm_t goes in, the library
    does local arg-min, ncclAllGather (16 B per rank) and the second-level arg-min on the caller's stream.  One-rank communicator
    built here through RCCL's own C API."""
    import torch
    eng = gpu_engine_factory(default_config())
    rccl = C.CDLL("librccl.so")

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_byte * 128)]
    uid = UniqueId()
    assert rccl.ncclGetUniqueId(C.byref(uid)) == 0
    comm = C.c_void_p(0)
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    assert rccl.ncclCommInitRank(C.byref(comm), 1, uid, 0) == 0
    try:
        rng = np.random.default_rng(3)
        cost = rng.uniform(1.0, 2.0, size=8192); cost[[17, 4000]] = 0.5; cost[100] = np.nan
        tc = eng.to_device(cost)
        val = torch.empty(1, dtype=torch.float64, device=eng.device); idx = torch.empty(1, dtype=torch.int64, device=eng.device)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = eng.lib.admpc_argmin_global(eng._h, C.c_void_p(tc.data_ptr()), 8192, 5 * 8192, comm, C.c_void_p(val.data_ptr()), C.c_void_p(idx.data_ptr()), st)
        assert rc == 0, eng.lib.admpc_last_error()
        torch.cuda.synchronize()
        assert val.item() == 0.5 and idx.item() == 5 * 8192 + 17
        assert eng.lib.admpc_argmin_global(eng._h, C.c_void_p(tc.data_ptr()), 8192, 0, C.c_void_p(0), C.c_void_p(val.data_ptr()), C.c_void_p(idx.data_ptr()), st) == -1
    finally:
        rccl.ncclCommDestroy.argtypes = [C.c_void_p]
        rccl.ncclCommDestroy(comm)


@pytest.mark.parametrize("with_gp", [False, True])
def test_iterate_shift_matches_oracle(gpu_engine_factory, oracle, with_gp):
    """admpc_shift_batch (SURVEY 8f-3 option): the moved stages are copies (bit-exact), the rolled-out terminal state
    agrees with the oracle's RK4 step to 1e-12 relative."""
    import torch
    cfg = default_config(N=20)
    if with_gp:
        set_gp(cfg, grid_gp())
    s = random_scenarios(67, N=20, seed=11, blend=(3.0, 5.0))          # 67: not a multiple of the 21 instances per wave
    eng = gpu_engine_factory(cfg)
    X, U, _, st, _ = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    d = eng.to_device
    for rollout in (False, True):
        tx, tu = d(X).clone(), d(U).clone()
        eng.shift(tx, tu, d(s["p"]), rollout=rollout)
        torch.cuda.synchronize()
        gx, gu = tx.cpu().numpy(), tu.cpu().numpy()
        ox, ou = oracle.shift_batch(cfg, X, U, s["p"], rollout=rollout)
        assert np.array_equal(gu, ou) and np.array_equal(gx[:, :20], ox[:, :20])
        if rollout:
            assert np.abs(gx[:, 20] - ox[:, 20]).max() <= 1e-12 * max(1.0, np.abs(ox[:, 20]).max())
            assert np.abs(gx[:, 20] - X[:, 20]).max() > 1e-3
        else:
            assert np.array_equal(gx[:, 20], ox[:, 20])
    with pytest.raises(ValueError):
        eng.shift(d(X), d(U), None, rollout=True)
    eng.shift(d(X[:0]), d(U[:0]), d(s["p"][:0]))                        # empty batch: no launch
    L = eng.lib
    assert L.admpc_shift_batch(eng._h, 3, C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), 0, C.c_void_p(0)) == -1      # null arrays
    assert L.admpc_argmin_pairs(eng._h, C.c_void_p(0), 0, C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)) == -1
    if not with_gp:                                                     # the shortest and a long horizon, dynamic branch
        for N, B in ((2, 5), (64, 9)):
            c2 = default_config(N=N)
            s2 = random_scenarios(B, N=N, seed=12, blend=(3.0, 5.0))
            e2 = gpu_engine_factory(c2)
            X2 = s2["xbar"] + np.random.default_rng(1).normal(size=s2["xbar"].shape) * 0.01
            U2 = s2["ubar"] + np.random.default_rng(2).normal(size=s2["ubar"].shape) * 0.1
            tx, tu = e2.to_device(X2).clone(), e2.to_device(U2).clone()
            e2.shift(tx, tu, e2.to_device(s2["p"]), rollout=True)
            torch.cuda.synchronize()
            ox, ou = oracle.shift_batch(c2, X2, U2, s2["p"], rollout=True)
            assert np.array_equal(tu.cpu().numpy(), ou) and np.array_equal(tx.cpu().numpy()[:, :N], ox[:, :N])
            assert np.abs(tx.cpu().numpy()[:, N] - ox[:, N]).max() <= 1e-12 * max(1.0, np.abs(ox[:, N]).max())


def test_argmin_kernel(gpu_engine_factory):
    import torch
    eng = gpu_engine_factory(default_config())
    rng = np.random.default_rng(0)
    for B in (1, 2, 63, 64, 255, 256, 257, 4096, 8192):
        c = rng.uniform(0, 100, B)
        if B > 4:
            c[B // 2] = c.min(); c[1] = np.nan; c[3] = np.inf         # tie with a later index, NaN, inf
        v, i = eng.argmin(eng.to_device(c), index_offset=1000)
        torch.cuda.synchronize()
        cc = np.where(np.isnan(c), np.inf, c)
        assert v.item() == cc.min() and i.item() == 1000 + int(np.argmin(cc))
    v, i = eng.argmin(eng.to_device(np.array([np.inf, np.nan])), 7)
    assert math.isinf(v.item()) and i.item() == 7


def test_argmin_rules_table_on_the_device_reducers(gpu_engine_factory):
    """tests/argmin_spec.py -- the table tests/test_dist_gloo.py runs against the host reducer of the world-size-2 gloo path --
    against the device kernels: admpc_argmin_pairs on every case, admpc_argmin on the cost-array cases and on every case whose
    records carry consecutive indices, and the library's host twin once more in this process (same answers, bit for bit)."""
    import torch
    from ad_mpc_amd import dist as adist
    from tests import argmin_spec as spec
    eng = gpu_engine_factory(default_config())

    def records(recs):
        a = np.empty((len(recs), 2)); a[:, 0] = [c for c, _ in recs]
        a[:, 1] = np.array([i for _, i in recs], dtype=np.int64).view(np.float64)
        return a
    for name, recs, want in spec.CASES:
        rec = records(recs)
        dev = adist.unpack_pair(eng.argmin_pairs(eng.to_device(rec)))
        host = adist.unpack_pair(adist.pairs_min_host(torch.from_numpy(rec)))
        assert dev == want and host == want, (name, dev, host, want)
        if spec.consecutive((name, recs, want)):
            v, i = eng.argmin(eng.to_device(rec[:, 0].copy()), index_offset=recs[0][1])
            assert (v.item(), i.item()) == want, name
    for name, costs, off, want in spec.ARRAY_CASES:
        v, i = eng.argmin(eng.to_device(np.array(costs)), index_offset=off)
        assert (v.item(), i.item()) == want, (name, v.item(), i.item(), want)
        assert adist.unpack_pair(eng.argmin_pair(eng.to_device(np.array(costs)), index_offset=off)) == want, name


def test_epilogue_kernel_matches_host_logic(gpu_engine_factory):
    import torch
    from ad_mpc_amd import host
    cfg = default_config()
    eng = gpu_engine_factory(cfg)
    s = random_scenarios(64, seed=5)
    x, u, *_ = eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
    x[3, :, 1] += 30.0; x[7, 4, 0] += 30.0          # make two instances invalid
    ref = s["xref"][:, :, :2].copy()
    ack, valid = eng.epilogue(eng.to_device(x), eng.to_device(u), eng.to_device(ref))
    torch.cuda.synchronize()
    ack, valid = ack.cpu().numpy(), valid.cpu().numpy()
    for b in range(64):
        assert bool(valid[b]) == host.is_valid_command(x[b], s["xref"][b])
        exp = np.array(host.ackermann_fields(x[b], u[b].reshape(-1)), dtype=np.float32)
        np.testing.assert_array_equal(ack[b], exp)
    assert not valid[3] and not valid[7] and 0 < valid.sum() < 64


def test_long_horizons_fp64(gpu_engine_factory, oracle_omp):
    """Horizon of BASELINE configs[4] (N = 80, T = 4 s) and the maximum N = 128, in fp64, in this process (kernel R has no
    private segment: the child process the old stage-wise kernel needed is gone)."""
    for N, B in [(80, 512), (128, 128)]:
        cfg = default_config(N=N)
        s = random_scenarios(B, N=N, seed=1234, blend=(3.0, 5.0))
        g = gpu_engine_factory(cfg).solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])
        o = oracle_omp.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"], nthreads=16)
        assert (o[3] == 0).all()
        _assert_parity(g, o, TOL_LONG)


@pytest.mark.parametrize("N", [20, 40])
def test_reference_stop_levels_on_the_device(gpu_engine_factory, oracle_omp, N):
    """The default stop levels (HPIPM BALANCE's 1e-8 on every residual norm and on the complementarity products, no step test: the
    reference's setting) against the tight levels of rounds 1-2 on the full bench batch, both on the device and both against the oracle at
    the same levels: identical statuses and iteration counts either way; the default levels never need more iterations, the slowest
    instance three (N = 20) / four (N = 40) fewer; the steps agree to 1e-6 for 98 % (N = 40: 94 %) of the instances, to 2e-5 for 99 % and to
    2.4e-4 at worst (instances with a nearly degenerate bound pair: error ~ sqrt(mu) -- the accuracy the reference's own QP solver delivers there)."""
    s = random_scenarios(4096, N=N, seed=1234)
    res = {}
    for name, cfg in (("ref", default_config(N=N)), ("tight", tight_config(N=N))):
        g, o = _solve_both(gpu_engine_factory(cfg), oracle_omp, cfg, s, nthreads=16)
        _assert_parity(g, o, tol_for(N))
        res[name] = g
    a, t = res["ref"], res["tight"]
    assert (a[3] == 0).all() and (a[4] <= t[4]).all() and a[4].max() <= t[4].max() - 3 and a[4].mean() <= 0.88 * t[4].mean()
    dev = np.abs(a[1] - t[1]).max(axis=(1, 2))
    assert dev.max() <= 5e-4 and np.quantile(dev, 0.99) <= 2e-5 and np.quantile(dev, 0.9) <= 1e-6
