"""The simulator's random disturbances on the device (include/admpc_quad_noise.h; ad_mpc_amd/quad_fleet.py: noise_seed=).

The generator's words are compared bit for bit with the numpy spec (tests/quad_noise_spec.py) and the normals at a bound worked out from
the libraries' errors.  The noisy plant step is compared with the spec -- which tests/test_quad_noise_cpu.py holds against the
reference's own simulator at 1e-15 -- and with the reference-made golden vectors at the plant's bound, substeps * 1e-12 relative to
max(1, |ref|).  The noisy rollout is compared bit for bit with the loop it replaces, and with the CPU closed loop of the oracle's solve
and the spec's noisy plant."""
import ctypes as C
import json

import numpy as np
import pytest

import gen_quad_noise_golden as NG
import gen_quad_plant_golden as GG
import quad_learn_spec as QL
import quad_noise_spec as NS
import quad_plant_spec as QS
import test_quad_fleet_gpu as TQ
from test_quad_fleet_gpu import RTOL, _bits, _close, _dev, _host, _p, _stream

pytestmark = pytest.mark.gpu

SEED = NG.SEED
SWITCHES = [(False, False), (True, False), (False, True), (True, True)]           # (noisy, motor_noise)


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _plant(drag, substeps):
    from ad_mpc_amd.quad_config import SimQuad, quad_plant_params
    p = quad_plant_params(SimQuad(drag=drag), GG.DT, GG.DT)
    p.substeps = substeps
    return p


def _noise(noisy=True, motor_noise=True, seed=SEED):
    from ad_mpc_amd.quad_config import SimQuad, quad_noise_params
    return quad_noise_params(SimQuad(noisy=noisy, motor_noise=motor_noise), GG.DT, seed)


def _periods(B):
    return np.arange(B, dtype=np.uint64) * np.uint64(2 ** 31)


def _run_plant(L, plant, noise, X, U, p):
    """One period on copies of the inputs: (the new states [B,13], noise_step afterwards [B] uint64).  Both switches off: the
    deterministic entry, which is what the noise entries tell such a caller to use."""
    import torch
    x, u = _dev(X), _dev(U)
    step = _dev(np.asarray(p, dtype=np.uint64).view(np.int64))
    if not (noise.noisy or noise.motor_noise):
        rc = L.admpc_quad_plant_step_batch(C.byref(plant), 0, X.shape[0], _p(u), 4, _p(x), _stream())
    else:
        rc = L.admpc_quad_plant_step_noise_batch(C.byref(plant), C.byref(noise), 0, X.shape[0], _p(u), 4, _p(x), _p(step), _stream())
    assert rc == 0, L.admpc_last_error()
    torch.cuda.synchronize()
    return _host(x), _host(step).view(np.uint64)


# ---- 1. the draws -------------------------------------------------------------------------------------------------------------------

def test_draws_equal_the_spec():
    """B = 67, 40 sub-steps, noise_step = arange(67) * 2^31, so that the high counter word is exercised.  The words bit for bit; the
    normals within 16 * 2^-52 * max(1, r), r from the spec: log, sin and cos are within 2 ulp in both libraries, sqrt is exact and two
    products follow -- about 6 ulp of r -- with a margin of 2.5.  Measured on the MI355X: see DESIGN.md section 7."""
    import torch
    L = TQ._lib()
    B, S = 67, 40
    p = _periods(B)
    assert (p >> np.uint64(32)).max() > 0
    step = _dev(p.view(np.int64))
    z = torch.full((B, S, 10), float("nan"), dtype=torch.float64, device="cuda:0")
    raw = torch.zeros((B, S, 10), dtype=torch.int64, device="cuda:0")
    noise = _noise()
    assert L.admpc_quad_noise_draw_batch(C.byref(noise), 0, B, S, _p(step), _p(z), _p(raw), _stream()) == 0, L.admpc_last_error()
    want_raw = NS.words(SEED, np.arange(B)[:, None], p[:, None], np.arange(S)[None, :])
    want, r = NS.normals(want_raw)
    _bits(_host(raw).view(np.uint64), want_raw, "the generator's words")
    got = _host(z)
    ratio = np.abs(got - want) / (16 * 2.0 ** -52 * np.maximum(1.0, np.repeat(r, 2, axis=-1)))
    print("draws: largest |z - spec| = %.3g, over its bound %.3g, in ulp of max(1, r) %.3g" % (np.abs(got - want).max(), ratio.max(), 16 * ratio.max()))
    assert np.isfinite(got).all() and ratio.max() <= 1.0
    _bits(_host(step).view(np.uint64), p, "noise_step after the draw call")
    z2 = torch.empty_like(z)                                        # without raw; one switch off: all ten are written all the same
    one = _noise(noisy=False)
    assert L.admpc_quad_noise_draw_batch(C.byref(one), 0, B, S, _p(step), _p(z2), None, _stream()) == 0
    _bits(_host(z2), got, "the draws do not depend on the switches")


# ---- 2. the plant against the spec and the golden vectors ---------------------------------------------------------------------------

_SPEC = {}


def _spec67(noisy, motor_noise, drag, substeps):
    key = (noisy, motor_noise, drag, substeps)
    if key not in _SPEC:
        X, U = QS.fleet67()
        _SPEC[key] = NS.step_batch(_plant(drag, substeps), _noise(noisy, motor_noise), X, U, _periods(67))
    return _SPEC[key]


@pytest.mark.parametrize("substeps", [1, 40])
@pytest.mark.parametrize("drag", [False, True])
@pytest.mark.parametrize("noisy,motor_noise", SWITCHES)
def test_noisy_plant_matches_the_spec_and_the_golden_vectors(noisy, motor_noise, drag, substeps):
    """QS.fleet67 with its NaN activation, vehicle b in period b * 2^31.  Bound: substeps * 1e-12 * max(1, |ref|), the plant's; the
    draws' own error is orders of magnitude below it.  Then the twelve vehicles of tests/golden/quad_noise_vectors.json against what the
    reference's own simulator gave under the same draws."""
    L = TQ._lib()
    X, U = QS.fleet67()
    plant, noise = _plant(drag, substeps), _noise(noisy, motor_noise)
    p = _periods(67)
    want, replaced = _spec67(noisy, motor_noise, drag, substeps)
    assert replaced.sum() == 1 and replaced[9]
    got, after = _run_plant(L, plant, noise, X, U, p)
    what = "noisy=%s motor_noise=%s drag=%s substeps=%d" % (noisy, motor_noise, drag, substeps)
    _close(got, want, substeps * RTOL, "noisy plant, " + what)
    with open(NG.OUT) as f:
        doc = json.load(f)
    case = [c for c in doc["cases"] if (c["noisy"], c["motor_noise"], c["drag"], c["substeps"]) == (noisy, motor_noise, drag, substeps)]
    assert len(case) == 1 and doc["dt"] == plant.dt and doc["seed"] == SEED
    Xg, Ug, pg = np.array(doc["x"]), np.array(doc["u"]), np.array(doc["periods"], dtype=np.uint64)
    _close(_run_plant(L, plant, noise, Xg, Ug, pg)[0], np.array(case[0]["result"]), substeps * RTOL, "golden vectors, " + what)
    if not (noisy or motor_noise):
        return
    _bits(after, p + np.uint64(1), "noise_step advanced by exactly 1")
    again, after2 = _run_plant(L, plant, noise, X, U, after)
    assert np.abs(again - got).max() > 1e-9, "a second call draws other numbers"
    _bits(after2, p + np.uint64(2), "noise_step after the second call")
    _bits(_run_plant(L, plant, noise, X, U, p)[0], got, "the same call from the same counters")
    other = _noise(noisy, motor_noise, seed=SEED + 1)
    assert np.abs(_run_plant(L, plant, other, X, U, p)[0] - got).max() > 1e-9, "another key draws other numbers"
    calm = _noise(noisy, motor_noise)
    calm.force_std = calm.torque_std = calm.motor_std = calm.motor_bias = 0.0
    _close(_run_plant(L, plant, calm, X, U, p)[0], TQ._spec67(drag, False, substeps)[0], substeps * RTOL, "all scales 0 against the deterministic plant, " + what)


# ---- 3. past the grid ---------------------------------------------------------------------------------------------------------------

def test_noisy_plant_past_the_grid():
    """B = 4096 * 64 + 301 with one sub-step, both switches and drag on: one lane per vehicle, the stride loop runs and the last wave is
    partial.  Every vehicle draws its own numbers, so the last 301 vehicles and every 997th are held against the spec."""
    L = TQ._lib()
    B = QS.PAST_THE_GRID
    X, U = QS.fleet67()
    t = np.arange(B) % 67
    plant, noise = _plant(True, 1), _noise()
    p = np.full(B, 5, dtype=np.uint64)
    got, after = _run_plant(L, plant, noise, X[t], U[t], p)
    assert (after == 6).all()
    sample = np.unique(np.concatenate([np.arange(0, B, 997), np.arange(B - 301, B)]))
    assert sample.max() == B - 1 and (sample >= 4096 * 64).sum() >= 301
    want = np.stack([NS.step(plant, noise, X[b % 67], U[b % 67], b, 5)[0] for b in sample])
    _close(got[sample], want, RTOL, "noisy plant past the grid, the sample")
    assert len({got[b].tobytes() for b in range(0, 67 * 50, 67)}) == 50                      # the same vehicle 50 times over: 50 results


@pytest.mark.parametrize("B,substeps", [(NS.WIDE_MAX, 13), (NS.WIDE_MAX + 1, 5)])
def test_noisy_plant_on_both_sides_of_the_mapping_threshold(B, substeps):
    """The largest fleet that gets four lanes a vehicle (16 vehicles a block, chunks of 10 sub-steps: 13 sub-steps are a whole and a
    partial chunk) and the smallest that gets one (chunks of 2: 5 sub-steps are two and a partial one).  The first and the last 70
    vehicles and every 997th against the spec."""
    L = TQ._lib()
    per = 64 // NS.WIDE_LANES
    assert NS.LDS_DOUBLES // (per * 10) == 10 and NS.LDS_DOUBLES // (64 * 10) == 2 and NS.WIDE_MAX % per == 0
    X, U = QS.fleet67()
    t = np.arange(B) % 67
    plant, noise = _plant(True, substeps), _noise()
    p = np.arange(B, dtype=np.uint64) % np.uint64(5)
    got, after = _run_plant(L, plant, noise, X[t], U[t], p)
    _bits(after, p + np.uint64(1), "noise_step")
    sample = np.unique(np.concatenate([np.arange(70), np.arange(0, B, 997), np.arange(B - 70, B)]))
    want = np.stack([NS.step(plant, noise, X[b % 67], U[b % 67], b, p[b])[0] for b in sample])
    _close(got[sample], want, substeps * RTOL, "noisy plant at B = %d" % B)


# ---- 4. the rollout against the loop it replaces ------------------------------------------------------------------------------------

def _fleet(B, N, trajs, traj_of, idx0, x0, learn=None, seed=SEED):
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    fl = QuadFleet(B, quad=SimQuad(drag=True, noisy=True, motor_noise=True), n_nodes=N, learn=learn, noise_seed=seed)
    fl.set_trajectories(trajs)
    fl.reset(traj_of, idx0, x0)
    return fl


def _python_loop(fl, trajs, T, observe=False):
    """The loop the noisy rollout replaces: window, solve, noisy plant step under w_opt[:, 0], index update (and observe), each a call
    of its own; the tally and the counts by the spec.  Returns (traj [T+1,B,13], u [T,B,4], tally, counts)."""
    import torch
    B = fl.B
    pos = torch.empty((B, 3), dtype=torch.float64, device=fl.device)
    tally, counts = np.zeros((B, 3)), np.zeros((B, 3), dtype=np.int32)
    traj, us = [_host(fl.x)], []
    traj_of = _host(fl.traj_of)
    if observe:
        fl.observe_latch()
    for _ in range(T):
        fl.ref_chunk(pos_ref=pos)
        fl._eng.solve(fl.x, fl.yref, fl.yref_e, fl.x_opt, fl.w_opt, fl.cost, fl.status, fl.iters)
        u0, st, pr, x = _host(fl.w_opt)[:, 0, :].copy(), _host(fl.status), _host(pos), _host(fl.x)
        for b in range(B):
            QS.tally_step(tally[b], counts[b], pr[b], x[b], st[b], not np.isfinite(u0[b]).all())
        fl.plant_step(fl.w_opt[:, 0, :])
        fl.idx.copy_(torch.as_tensor(QS.next_idx(trajs, traj_of, _host(fl.idx))))
        if observe:
            fl.observe()
        us.append(u0); traj.append(_host(fl.x))
    return np.stack(traj), np.stack(us), tally, counts


@pytest.mark.parametrize("N,B,T", [(10, 67, 6), (20, 33, 3)])
def test_noisy_rollout_equals_the_loop_it_replaces(N, B, T):
    """The vehicles of test_rollout_equals_the_loop_it_replaces, both switches and drag on.  The rollout equals the Python loop of
    ref_chunk, solve, noisy plant_step and idx advance bit for bit in x, idx, the iterate, tally, counts, traj and u, and noise_step is T.
    Then the observed form (one feature per axis) against observe_latch, the same loop and observe, in samples, bins and dropped."""
    trajs = TQ._circles(N, 3.0)
    traj_of = (np.arange(B) % 2).astype(np.int32)
    idx0 = np.where(traj_of == 1, 6, (np.arange(B) * 3) % 110).astype(np.int32)
    x0 = TQ._start(trajs, traj_of, idx0, seed=N)
    for learn in (None, QL.EXP_LEARN):
        whole, loop, calm = (_fleet(B, N, trajs, traj_of, idx0, x0, learn=learn) for _ in range(3))
        try:
            out = whole.rollout(T, record=True, observe=learn is not None)
            traj, us, tally, counts = _python_loop(loop, trajs, T, observe=learn is not None)
            got, want = TQ._state(whole), TQ._state(loop)
            for k in ("x", "idx", "x_opt", "w_opt", "status", "yref", "yref_e", "cost", "iters"):
                _bits(got[k], want[k], k)
            _bits(_host(out.traj), traj, "traj_out"); _bits(_host(out.u), us, "u_out")
            _bits(got["tally"], tally, "tally"); _bits(got["counts"], counts, "counts")
            for fl in (whole, loop):
                assert (_host(fl.noise_step) == T).all()
            assert (got["counts"] == [T, 0, 0]).all() and np.abs(traj[T] - traj[0])[:, 0:3].max() > 0.05
            if learn is not None:
                for k in ("samples", "bins", "dropped", "_prev"):
                    _bits(_host(getattr(whole, k)), _host(getattr(loop, k)), k)
                assert (_host(whole.bins)[:, :, 0].sum(axis=1) + _host(whole.dropped)[:3] == B * T).all()
            # the same fleet under another key flies another trajectory; u_out is the raw first input of the iterate
            calm.reseed(SEED + 1)
            assert np.abs(_host(calm.rollout(T).x) - got["x"]).max() > 1e-7
            _bits(us[T - 1], got["w_opt"][:, 0, :], "u_out stays the raw ubar[b][0]")
        finally:
            for fl in (whole, loop, calm):
                fl.close()


# ---- 5. graph -----------------------------------------------------------------------------------------------------------------------

def test_captured_noisy_rollout_draws_fresh_numbers_at_every_replay():
    """rollout(3) at B = 67 captured and replayed twice WITHOUT a reset in between: the counters live on the device, so the two replays
    equal six eager steps bit for bit, and the second replay's disturbances are not the first's."""
    import torch
    N, B, T = 10, 67, 3
    trajs = TQ._circles(N, 3.0)
    traj_of = (np.arange(B) % 2).astype(np.int32)
    idx0 = np.where(traj_of == 1, 2, (np.arange(B) * 5) % 100).astype(np.int32)
    x0 = TQ._start(trajs, traj_of, idx0, seed=81)
    eager, graphed = (_fleet(B, N, trajs, traj_of, idx0, x0) for _ in range(2))
    try:
        graphed.rollout(T)                                          # every kernel has run once before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = graphed.rollout(T, record=True)
        graphed.reset(traj_of, idx0, x0); graphed.reseed(step=0)
        ref = eager.rollout(2 * T, record=True)
        rt, ru = _host(ref.traj), _host(ref.u)
        for r in range(2):
            g.replay()
            _bits(_host(out.traj), rt[r * T:(r + 1) * T + 1], "traj at replay %d" % r); _bits(_host(out.u), ru[r * T:(r + 1) * T], "u at replay %d" % r)
        want, got = TQ._state(eager), TQ._state(graphed)
        for k in TQ.STATE + ("tally", "cost", "iters"):
            _bits(got[k], want[k], "%s after two replays" % k)
        assert (_host(graphed.noise_step) == 2 * T).all() and (want["counts"] == [2 * T, 0, 0]).all()
        z0 = graphed.noise_draws()
        graphed.reseed(step=0)
        assert z0.shape == (B, 40, 10) and np.abs(graphed.noise_draws() - z0).max() > 1.0       # period 6 against period 0
        z3 = graphed.noise_draws(substeps=3)
        _bits(z3, np.ascontiguousarray(graphed.noise_draws()[:, :3]), "the draws of a sub-step do not depend on how many there are")
        assert np.abs(z3 - NS.draws(SEED, np.arange(B)[:, None], 0, np.arange(3)[None, :])).max() <= 16 * 2.0 ** -52 * 8.66
    finally:
        eager.close(); graphed.close()


# ---- 6. the noisy rollout against the CPU closed loop -------------------------------------------------------------------------------

def _cpu_loop(oracle, cfg, plant, noise, trajs, traj_of, idx0, x0, T, over):
    """The oracle's RTI step and the spec's noisy plant in closed loop, period t drawing with counter t: (traj [T+1,B,13], status [T,B])."""
    B, N = len(traj_of), cfg.N
    x, idx = np.array(x0), np.array(idx0)
    xbar, ubar = np.zeros((B, N + 1, 13)), np.zeros((B, N, 4))
    traj, sts = [x.copy()], []
    for t in range(T):
        yref, yref_e, _ = QS.chunk_batch(trajs, traj_of, idx, N, over)
        xbar, ubar, _, st, _ = oracle.solve_batch(cfg, x, yref, yref_e, xbar, ubar)
        x, _ = NS.step_fleet(plant, noise, x, ubar[:, 0, :], t)
        idx = QS.next_idx(trajs, traj_of, idx)
        traj.append(x.copy()); sts.append(st.copy())
    return np.stack(traj), np.stack(sts)


def test_noisy_rollout_follows_the_cpu_closed_loop():
    """test_rollout_follows_the_cpu_closed_loop's N = 10 case with both switches on: the CPU loop flies the spec's noisy step_fleet under
    the same draws.  Statuses identical; states within 1e-8 * T * S, S measured as that test measures it (under the same disturbances)."""
    from ad_mpc_amd.quad_scenarios import circle_reference
    from oracle.quad_oracle import QuadOracle
    N, speed, T, B, over = 10, 3.0, 25, 8, 5
    dt = 1.0 / (N * over)
    trajs = [circle_reference(120, dt, 5.0, speed)]
    traj_of = np.zeros(B, dtype=np.int32)
    idx0 = np.array([0, 0, 95, 95, 0, 0, 95, 95], dtype=np.int32)
    x0 = np.stack([trajs[0][0][i] for i in idx0])
    x0[[1, 3, 5, 7], 0:3] += 0.3 * np.array([1.0, -1.0, 0.5])
    x0[4:, 7:10] *= 0.9
    fl = _fleet(B, N, trajs, traj_of, idx0, x0)
    try:
        oracle = QuadOracle()
        cpu, sts = _cpu_loop(oracle, fl.cfg, fl._plant, fl._noise, trajs, traj_of, idx0, x0, T, over)
        moved = x0.copy(); moved[:, 0:3] += 1e-8; moved[:, 7:10] += 1e-8
        S = max(1.0, float(np.abs(_cpu_loop(oracle, fl.cfg, fl._plant, fl._noise, trajs, traj_of, idx0, moved, T, over)[0] - cpu).max() / 1e-8))
        calm = TQ._cpu_loop(oracle, fl.cfg, fl._plant, trajs, traj_of, idx0, x0, T, over)[0]
        got, dev_st = [_host(fl.x)], []
        for _ in range(T):
            fl.step()
            got.append(_host(fl.x)); dev_st.append(_host(fl.status))
        got, dev_st = np.stack(got), np.stack(dev_st)
    finally:
        fl.close()
    err = float(np.abs(got - cpu).max())
    print("noisy closed loop: sensitivity S = %.3f, max |device - CPU loop| = %.3g (bound %.3g), against the calm loop %.3g"
          % (S, err, 1e-8 * T * S, np.abs(cpu - calm).max()))
    assert np.array_equal(dev_st, sts) and (sts == 0).all()
    assert err <= 1e-8 * T * S
    assert np.abs(cpu - calm).max() > 1e-3                                                       # the disturbances act on the loop


# ---- 7. the reference's set-up end to end -------------------------------------------------------------------------------------------

def test_the_reference_set_up_flies_learns_and_flies_again_on_the_device():
    """SimpleSimConfig.simulation_disturbances -- noisy, drag, motor_noise -- at B = 64: an observed rollout, fit_gp, a second rollout;
    nothing comes to the host in between.  The motor bias is in what the GPs learn: the vertical residual's samples are negative on
    average (the rotors deliver less than commanded)."""
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    N, B, T = 10, 64, 10
    trajs = TQ._circles(N, 3.0)[:1]
    fl = QuadFleet(B, quad=SimQuad(drag=True, noisy=True, motor_noise=True), n_nodes=N, learn=QL.EXP_LEARN, noise_seed=11)
    try:
        fl.set_trajectories(trajs)
        fl.reset(np.zeros(B, dtype=np.int32), (np.arange(B) * 3) % 100)
        fl.rollout(T, observe=True)
        info, installed = fl.fit_gp()
        fl.rollout(2)
        assert (_host(fl.noise_step) == T + 2).all() and (_host(fl.counts) == [T + 2, 0, 0]).all()
        assert (_host(info) >= 1).all() and _host(installed).tolist() == [1, 1, 1]
        samples = _host(fl.samples)
        assert (samples[:, 13] == 1.0).all() and samples[:, 12].mean() < 0.0
    finally:
        fl.close()
    plain = QuadFleet(2, quad=SimQuad(drag=True), noise_seed=5)                                  # a quad without disturbances ignores the seed
    try:
        assert plain.noise_step is None and plain._noise is None
        with pytest.raises(ValueError, match="deterministic"):
            plain.reseed(1)
        with pytest.raises(ValueError, match="deterministic"):
            plain.noise_draws()
    finally:
        plain.close()
