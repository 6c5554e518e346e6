"""The plant step and the rollout on the device (include/admpc_plant.h; ad_mpc_amd/fleet.py: set_plant, plant_step, rollout_route).

The plant step is compared with its numpy restatement (tests/plant_spec.py: one oracle RK4 step per sub-step) at 1e-12 relative to
max(1, |ref|), element by element -- the bound test_iterate_shift_matches_oracle holds this model step to; over M sub-steps the bound is
that one summed over the sub-steps and carried through the chain's own Jacobians.  The rollout is compared bit for bit with the loop it
replaces, a second controller driven from Python by step_route and plant_step; its tally and counts with the spec's accumulation."""
import ctypes as C

import numpy as np
import pytest

import lane_spec as LS
import path_bank as PB
import plant_spec as PS
import test_lane_gpu as TL                      # the road, the poses beside it, the controller's STATE list, the bit comparison

pytestmark = pytest.mark.gpu

T_HORIZON = TL.T_HORIZON
RTOL = 1e-12
_dev, _p, _bits = TL._dev, TL._p, TL._bits


def _plant(**kw):
    from ad_mpc_amd.config import AdmpcPlantParams
    d = dict(dt=0.05, blend_min=3.0, blend_max=5.0, brake_acc=-10.0, v_min=0.0, substeps=1, reserved=0)
    d.update(kw)
    return AdmpcPlantParams(**d)


def _cfg(with_gp):
    from ad_mpc_amd.config import default_config, set_gp
    from ad_mpc_amd.scenarios import grid_gp
    cfg = default_config(N=20)
    return set_gp(cfg, grid_gp()) if with_gp else cfg


def _fleet67():
    """(X [67,7], ack float32 [67,4], mode int32 [67]): the states of random_scenarios(67, blend=(3, 5)), so that p takes 0, 1 and values
    between; MPC and brake records mixed, one mode that is neither; accelerations and steering rates on both sides of every bound; a
    non-finite field under mode 1; two vehicles whose steering runs into its bound."""
    from ad_mpc_amd.scenarios import random_scenarios
    X = random_scenarios(67, N=20, seed=21, blend=(3.0, 5.0))["x0"].copy()
    rng = np.random.default_rng(22)
    mode = (np.arange(67) % 3 != 2).astype(np.int32)
    mode[5] = 2
    ack = np.zeros((67, 4), dtype=np.float32)
    ack[:, 0], ack[:, 2] = X[:, 6], X[:, 3]
    ack[:, 3] = rng.uniform(-14.0, 8.0, size=67)
    ack[:, 1] = rng.uniform(-4.5, 4.5, size=67)
    ack[7, 3], ack[9, 1] = np.nan, np.inf
    mode[[7, 9, 10, 12, 13]] = 1
    X[10, 6], ack[10, 1] = 0.5, 2.0
    X[12, 6], ack[12, 1] = -0.5, -4.0
    ack[13, 3], ack[13, 1] = 7.0, -3.5
    X[14, 3], mode[14] = 2.7, 0                                                       # brakes down to the floor of test 1
    return X, ack, mode


def _run_plant(eng, plant, X, ack, mode, calls=1):
    """admpc_plant_step_batch `calls` times on copies of the inputs: the new states [B,7]."""
    import torch
    st = [_dev(X[:, i]) for i in range(7)]
    a, m = _dev(ack, torch.float32), _dev(mode, torch.int32)
    for _ in range(calls):
        rc = eng.lib.admpc_plant_step_batch(eng._h, C.byref(plant), X.shape[0], _p(a), _p(m), *[_p(t) for t in st], eng._stream())
        assert rc == 0, eng.lib.admpc_last_error()
    torch.cuda.synchronize()
    return np.stack([t.cpu().numpy() for t in st], axis=1)


def _spec(oracle, cfg, plant, X, ack, mode, clear=True):
    out = [PS.step(oracle, cfg, plant, X[b], ack[b], mode[b], clear=clear) for b in range(X.shape[0])]
    return np.stack([o[0] for o in out]), np.array([PS.chain_gain(o[1]) for o in out])


def _close(got, want, bound, what):
    ratio = np.abs(got - want) / (bound * np.maximum(1.0, np.abs(want)))
    print("%s: largest |device - spec| over its bound: %.3g" % (what, ratio.max()))
    assert not np.isnan(got).any() and ratio.max() <= 1.0, (what, ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))


# ---- 1. one sub-step against the oracle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_gp", [False, True])
def test_one_sub_step_matches_the_spec(gpu_engine_factory, oracle, with_gp):
    """B = 67 (no multiple of the 21 vehicles of a block), dt = 0.05, M = 1, v_min = 2.5 so that the slow braking vehicles reach it."""
    cfg = _cfg(with_gp)
    X, ack, mode = _fleet67()
    plant = _plant(v_min=2.5)
    p = PS.blend(X[:, 3], 3.0, 5.0)
    assert (p == 0).any() and (p == 1).any() and ((p > 0) & (p < 1)).any() and set(mode.tolist()) == {0, 1, 2}
    for col, lo, hi in ((3, cfg.lbu[0], cfg.ubu[0]), (1, cfg.lbu[1], cfg.ubu[1])):
        v = ack[mode == 1, col]
        assert (v < lo).any() and (v > hi).any() and ((v > lo) & (v < hi)).any()
    want, _ = _spec(oracle, cfg, plant, X, ack, mode)
    assert (want[[10, 12], 6] == [cfg.ubx_delta, cfg.lbx_delta]).all() and (want[:, 3] == 2.5).any() and (want[:, 3] > 2.5).any()
    eng = gpu_engine_factory(cfg)
    try:
        got = _run_plant(eng, plant, X, ack, mode)
    finally:
        eng.close()
    _close(got, want, RTOL, "one sub-step, gp=%s" % with_gp)
    brake = ~((mode == 1) & np.isfinite(ack[:, 3]) & np.isfinite(ack[:, 1]))
    assert brake.sum() > 20 and np.array_equal(got[brake & (np.abs(X[:, 6]) < 0.45), 6], X[brake & (np.abs(X[:, 6]) < 0.45), 6])    # steering held
    assert np.abs(got - X).max() > 1e-2


# ---- 2. sub-steps -------------------------------------------------------------------------------------------------------------------

def test_sub_steps_chain_and_stay_within_the_summed_bound(gpu_engine_factory, oracle):
    """dt = 0.1 and M = 4 against four calls with M = 1 and dt = 0.025 (h is the same double in both forms), bit for bit, and against the
    spec within M * G * 1e-12.  The band (8, 8.5) with every speed at least 1.4 m/s away keeps p at 0 or 1 through the period, so the four
    calls, which take p anew, use the p of the one.  The four calls also wrap the yaw four times; (yaw + pi) - pi returns yaw itself only
    where yaw + pi is exact, which holds for -2 pi <= yaw <= -pi / 2 (Sterbenz), so every yaw is laid into [-2.9, -1.7] and the spec
    asserts that it stays inside [-3, -pi / 2] after every sub-step: |yaw| < 3 throughout, and the wrap moves no bit."""
    cfg = _cfg(True)
    X, ack, mode = _fleet67()
    X[:, 2] = -2.9 + 1.2 * (X[:, 2] + np.pi) / (2.0 * np.pi)
    X[:, 3] = np.where((X[:, 3] > 6.5) & (X[:, 3] < 10.0), X[:, 3] + 4.0, X[:, 3])
    ack[7, 3], ack[9, 1] = 1.0, 0.5                                                    # finite, so that the inputs cannot differ either
    M = 4
    one, quarter = _plant(dt=0.1, substeps=M, blend_min=8.0, blend_max=8.5), _plant(dt=0.025, substeps=1, blend_min=8.0, blend_max=8.5)
    assert one.dt / M == quarter.dt
    want, G = _spec(oracle, cfg, one, X, ack, mode)
    x = X.copy()
    for _ in range(M):                                                                 # the chain of the four calls, by the spec
        p = PS.blend(x[:, 3], 8.0, 8.5)
        assert ((p == 0) | (p == 1)).all() and (x[:, 2] >= -3.0).all() and (x[:, 2] <= -np.pi / 2).all()
        x, _ = _spec(oracle, cfg, quarter, x, ack, mode)
    assert (x[:, 2] >= -3.0).all() and (x[:, 2] <= -np.pi / 2).all() and np.array_equal(x, want)
    assert set(PS.blend(X[:, 3], 8.0, 8.5).tolist()) == {0.0, 1.0}
    eng = gpu_engine_factory(cfg)
    try:
        got = _run_plant(eng, one, X, ack, mode)
        chained = _run_plant(eng, quarter, X, ack, mode, calls=M)
    finally:
        eng.close()
    _bits(got, chained, "one call with M = 4 against four calls with M = 1")
    bound = (M * G * RTOL)[:, None]
    print("G: %.3f .. %.3f" % (G.min(), G.max()))
    _close(got, want, bound, "four sub-steps")


# ---- 3. past the grid ---------------------------------------------------------------------------------------------------------------

def test_plant_step_past_the_grid(gpu_engine_factory):
    """B = 4096 * 21 + 301: the stride loop runs and the last block is partial.  The 67 vehicles of test 1 tiled (4096 * 21 is no multiple
    of 67, so a block's second round holds other vehicles than its first): vehicle b ends as vehicle b mod 67."""
    cfg = _cfg(True)
    X, ack, mode = _fleet67()
    B = PS.PAST_THE_GRID
    assert B == 4096 * 21 + 301 and (4096 * 21) % 67 != 0
    t = np.arange(B) % 67
    eng = gpu_engine_factory(cfg)
    try:
        got = _run_plant(eng, _plant(v_min=2.5), X[t], ack[t], mode[t])
        small = _run_plant(eng, _plant(v_min=2.5), X, ack, mode)
    finally:
        eng.close()
    _bits(got, got[:67][t], "vehicle b against vehicle b mod 67")
    _bits(got[:67], small, "the first 67 against the batch of 67")


# ---- 4. the rollout against the loop it replaces ------------------------------------------------------------------------------------

def _poses(pose):
    return [_dev(np.ascontiguousarray(a)) for a in pose]


def _host(tensors):
    import torch
    torch.cuda.synchronize()
    return np.stack([t.cpu().numpy() for t in tensors])


def _lane_err(fc, path_of, ins, lane=64, back=8, ahead=64):
    """out_err [B,3] of the generator for the poses `ins`, on a COPY of the controller's lane_idx: what the next step_route will see."""
    import torch
    from ad_mpc_amd.config import AdmpcLaneParams
    B, N = fc.B, fc.N
    ref = torch.empty((B, 6, N), dtype=torch.float64, device=fc.device)
    err = torch.empty((B, 3), dtype=torch.float64, device=fc.device)
    stop = torch.empty((B,), dtype=torch.int32, device=fc.device)
    idx = fc.lane_idx.clone()
    prm = AdmpcLaneParams(L=lane, back=back, ahead=ahead)
    rc = fc.lib.admpc_waypoints_lane_batch(fc._bank, C.byref(prm), B, _p(path_of), _p(idx), *[_p(t) for t in ins[:5]], fc._prm.resample,
                                           fc._prm.acc_max, fc._prm.resample_dt, _p(ref), _p(err), _p(stop), fc._eng._stream())
    assert rc == 0, fc.lib.admpc_last_error()
    torch.cuda.synchronize()
    return err.cpu().numpy()


@pytest.mark.parametrize("N,B,T", [(20, 16, 6), (40, 8, 3)])
def test_rollout_equals_the_loop_of_step_route_and_plant_step(N, B, T):
    """Three controllers from the same poses on the curved road of 600 waypoints, threshold 2 (brake records first, MPC commands after):
    `loop` is driven from Python by step_route and plant_step, `single` by T rollouts of one step (accumulate), `whole` by one rollout
    of T steps (record).  State, poses and trajectory bit for bit; tally and counts against the spec's accumulation of the generator's
    own errors."""
    import torch
    road = TL._road()
    at = np.linspace(3, 500, B).astype(int)
    pose = TL._along(road, at, seed=N)
    tk = _dev(np.zeros(B, dtype=np.int32), torch.int32)
    fcs = [TL._controller(N, B, threshold=2) for _ in range(3)]
    loop, single, whole = fcs
    try:
        for fc in fcs:
            fc.set_paths([road])
            fc.set_plant(dt=T_HORIZON / N, substeps=2)
        pl, ps, pw = _poses(pose), _poses(pose), _poses(pose)
        out = whole.rollout_route(tk, *pw, steps=T, record=True)
        tally, counts = np.zeros((B, 3)), np.zeros((B, 3), dtype=np.int32)
        traj = [pose.copy()]
        for t in range(T):
            err = _lane_err(loop, tk, pl)
            loop.step_route(tk, *pl)
            st = TL._state(loop)
            for b in range(B):
                PS.tally_step(tally[b], counts[b], err[b], st["mode"][b], st["status"][b], st["valid"][b])
            loop.plant_step(*pl)
            traj.append(_host(pl))
            r = single.rollout_route(tk, *ps, steps=1, accumulate=t > 0)
            assert r.traj is None and r.tally is single.tally and r.counts is single.counts
            want, got = TL._state(loop), TL._state(single)
            for k in TL.STATE:
                _bits(got[k], want[k], "%s after step %d" % (k, t))
            _bits(_host(ps), traj[-1], "poses after step %d" % t)
            _bits(single.tally.cpu().numpy(), tally, "tally after step %d" % t)
            _bits(single.counts.cpu().numpy(), counts, "counts after step %d" % t)
        want, got = TL._state(loop), TL._state(whole)
        for k in TL.STATE:
            _bits(got[k], want[k], "%s at the end" % k)
        _bits(_host(pw), traj[-1], "poses at the end")
        _bits(out.traj.cpu().numpy(), np.stack(traj), "traj")
        _bits(out.tally.cpu().numpy(), tally, "tally"); _bits(out.counts.cpu().numpy(), counts, "counts")
        assert (counts[:, 0] == T).all() and (counts[:, 1] == T - 1).all() and (counts[:, 2] == 0).all(), counts
        assert (tally[:, 2] > 0.2).all() and np.abs(traj[-1] - traj[0])[:2].max() > 0.3          # 0.3 m beside the road at first; they moved
    finally:
        for fc in fcs:
            fc.close()


# ---- 5. graph -----------------------------------------------------------------------------------------------------------------------

def test_captured_rollout_replays_the_eager_result():
    import torch
    N, B, T = 20, 12, 3
    road = TL._road()
    at = np.linspace(0, 480, B).astype(int)
    poses = [TL._along(road, at + 9 * r, seed=30 + r) for r in range(2)]
    tk = _dev(np.zeros(B, dtype=np.int32), torch.int32)
    eager, graphed = TL._controller(N, B, threshold=1), TL._controller(N, B, threshold=1)
    try:
        for fc in (eager, graphed):
            fc.set_paths([road])
            fc.set_plant(dt=T_HORIZON / N)
        ins = _poses(poses[0])
        graphed.rollout_route(tk, *ins, steps=T)                                   # every kernel has run once before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = graphed.rollout_route(tk, *ins, steps=T, record=True)
        for r in range(2):
            eager.reset(); graphed.reset()
            pe = _poses(poses[r])
            ref = eager.rollout_route(tk, *pe, steps=T, record=True)
            for i in range(7):
                ins[i].copy_(torch.as_tensor(poses[r][i], device=graphed.device))
            g.replay()
            want, got = TL._state(eager), TL._state(graphed)
            for k in TL.STATE:
                _bits(got[k], want[k], "%s at replay %d" % (k, r))
            _bits(_host(ins), _host(pe), "poses at replay %d" % r)
            for k in ("tally", "counts", "traj"):
                _bits(getattr(out, k).cpu().numpy(), getattr(ref, k).cpu().numpy(), "%s at replay %d" % (k, r))
            assert (want["mode"] == 1).all() and (ref.counts.cpu().numpy() == [T, T, 0]).all()
    finally:
        eager.close(); graphed.close()


# ---- 6. a plant that is not the model -----------------------------------------------------------------------------------------------

def test_kinematic_controller_drives_a_dynamic_plant():
    """The controller predicts with the kinematic model (the shipped band 100 .. 110 m/s), the plant is dynamic at these speeds (band
    3 .. 5, four sub-steps per period of T_HORIZON / N).  No bound on the tracking error; its maximum is printed."""
    import torch
    N, B, T = 20, 16, 40
    road = TL._road()
    route = TL._spec_route(road)
    at = np.linspace(3, 480, B).astype(int)
    pose = TL._along(road, at, seed=40)
    pose[3] = np.random.default_rng(41).uniform(6.0, 10.0, size=B)
    tk = _dev(np.zeros(B, dtype=np.int32), torch.int32)
    fc = TL._controller(N, B, threshold=3)
    try:
        fc.set_paths([road])
        fc.set_plant(dt=T_HORIZON / N, substeps=4, blend_min=3.0, blend_max=5.0)
        assert fc._prm.blend_min == 100.0 and fc._prm.blend_max == 110.0
        ins = _poses(pose)
        out = fc.rollout_route(tk, *ins, steps=T, record=True)
        st = TL._state(fc)
        tally, counts, traj, last = out.tally.cpu().numpy(), out.counts.cpu().numpy(), out.traj.cpu().numpy(), _host(ins)
    finally:
        fc.close()
    print("dynamic plant under the kinematic controller: max |e_y| = %.4f m, rms e_y = %.4f m" % (tally[:, 2].max(), np.sqrt(tally[:, 0].max() / T)))
    assert (st["status"] == 0).all() and (st["mode"] == 1).all() and (st["valid"] == 1).all()
    assert (counts == [T, T - 2, 0]).all(), counts                  # every status 0 and valid; every record after the gate's warm-up an MPC command
    assert np.isfinite(tally).all() and (tally >= 0).all() and np.isfinite(traj).all()
    assert np.array_equal(traj[T], last) and np.array_equal(traj[0], pose)
    idx = np.full(B, -1)
    for t in range(T):                                               # the spec's chain of nearest waypoints over the poses the steps saw
        nxt = np.array([LS.nearest(route[1], route[2], traj[t, 0, b], traj[t, 1, b], idx[b], 8, 64) for b in range(B)])
        assert (nxt >= idx).all(), t
        idx = nxt
    assert np.array_equal(st["lane_idx"], idx) and (idx > at).all(), (st["lane_idx"], idx, at)
    gap = np.abs(last.T - st["x_opt"][:, 1, :]).max(axis=1)
    assert (gap > 1e-6).all(), gap                                    # the plant did not do what the controller predicted


# ---- 7. best_of on a closed-loop score ----------------------------------------------------------------------------------------------

def test_best_of_on_a_closed_loop_score():
    import torch
    N, V, Cn, T = 20, 8, 4, 5
    B = V * Cn
    road = TL._road()
    roads = [TL._road(off=1.5), road, TL._road(off=-1.0), TL._road(off=60.0)]
    at = np.linspace(40, 480, V).astype(int)
    pose = np.repeat(TL._along(road, at, seed=50), Cn, axis=1)
    tk = _dev(np.tile(np.arange(Cn, dtype=np.int32), V), torch.int32)
    fc = TL._controller(N, B, threshold=1)
    try:
        fc.set_paths(roads)
        fc.set_plant(dt=T_HORIZON / N)
        with pytest.raises(ValueError, match="step_paths"):
            fc.best_of(Cn)
        out = fc.rollout_route(tk, *_poses(pose), steps=T)
        score = torch.where(out.counts[:, 2] > 0, torch.full_like(out.tally[:, 0], float("inf")), out.tally[:, 0])
        val, idx = fc.best_of(Cn, cost=score)
        torch.cuda.synchronize()
        sc = score.cpu().numpy()
        ev, ei = PB.group_argmin(sc, Cn)
        _bits(val.cpu().numpy(), ev, "val"); _bits(idx.cpu().numpy(), ei, "idx")
        assert np.isfinite(ev).all() and (ei % Cn != 3).all() and np.isposinf(sc.reshape(V, Cn)[:, 3]).all()
        assert (out.counts.cpu().numpy()[:, 0] == T).all() and np.isfinite(sc.reshape(V, Cn)[:, 1]).all()
        val, idx = fc.best_of(Cn)                                              # without it: the last step's cost, as before
        torch.cuda.synchronize()
        ev, ei = PB.group_argmin(fc.cost.cpu().numpy(), Cn)
        _bits(val.cpu().numpy(), ev, "val of the last step's cost"); _bits(idx.cpu().numpy(), ei, "idx of the last step's cost")
        with pytest.raises(ValueError):
            fc.best_of(Cn, cost=score[:B - 1].contiguous())
        with pytest.raises(ValueError):
            fc.best_of(Cn, cost=score.to(torch.float32))
    finally:
        fc.close()


# ---- 8. a vehicle without a route ---------------------------------------------------------------------------------------------------

def test_a_vehicle_without_a_route_brakes_and_leaves_its_neighbours_alone():
    import torch
    N, B, T, lost = 20, 8, 4, 3
    road = TL._road()
    at = np.linspace(10, 400, B).astype(int)
    pose = TL._along(road, at, seed=60)
    dt, brake = T_HORIZON / N, -4.0
    res = []
    for k in (7, 0):                                                           # vehicle `lost` on a route the bank does not hold, then on the road
        path_of = np.zeros(B, dtype=np.int32)
        path_of[lost] = k
        fc = TL._controller(N, B, threshold=1)
        try:
            fc.set_paths([road])
            fc.set_plant(dt=dt, brake_acc=brake)
            ins = _poses(pose)
            out = fc.rollout_route(_dev(path_of, torch.int32), *ins, steps=T, record=True)
            res.append((TL._state(fc), _host(ins), out.tally.cpu().numpy(), out.counts.cpu().numpy(), out.traj.cpu().numpy()))
        finally:
            fc.close()
    (st, last, tally, counts, traj), good = res
    assert st["lane_idx"][lost] == -1 and (tally[lost] == 0).all() and counts[lost].tolist() == [T, 0, T]
    assert st["status"][lost] == 4 and st["mode"][lost] == 0 and np.isposinf(st["cost"][lost])
    # the kinematic model under the brake record: v_x' = brake_acc exactly, the steering held
    assert abs(last[3, lost] - (pose[3, lost] + T * dt * brake)) < 1e-12 and last[6, lost] == pose[6, lost]
    assert (np.diff(traj[:, 3, lost]) < 0).all()
    others = np.arange(B) != lost
    assert counts[others].tolist() == [[T, T, 0]] * (B - 1) and good[3][lost].tolist() == [T, T, 0]
    for k in TL.STATE:
        _bits(st[k][others], good[0][k][others], k)
    _bits(last[:, others], good[1][:, others], "poses")
    _bits(tally[others], good[2][others], "tally"); _bits(counts[others], good[3][others], "counts")
    _bits(traj[:, :, others], good[4][:, :, others], "traj")


# ---- 9. arguments -------------------------------------------------------------------------------------------------------------------

def test_argument_errors_and_the_plant_of_another_model(gpu_engine_factory):
    import torch
    from ad_mpc_amd.fleet import FleetLaneStep, FleetRollout
    N, B = 20, 6
    road = TL._road(M=200)
    pose = TL._along(road, np.linspace(5, 100, B).astype(int), seed=70)
    tk = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    fc = TL._controller(N, B, threshold=1)
    gp = gpu_engine_factory(_cfg(True))
    L = fc.lib
    try:
        assert fc._plant.dt == TL.OPT_DT and fc._plant.brake_acc == fc.ad.acc_min and fc._plant.substeps == 1        # the defaults of set_plant
        assert (fc._plant.blend_min, fc._plant.blend_max) == (fc._prm.blend_min, fc._prm.blend_max)
        for kw in (dict(dt=0.0), dict(dt=float("nan")), dict(substeps=0), dict(substeps=65), dict(blend_min=5.0, blend_max=5.0), dict(brake_acc=1.0),
                   dict(v_min=-1.0), dict(model=fc)):
            with pytest.raises(ValueError, match="set_plant"):
                fc.set_plant(**kw)
        ins = _poses(pose)
        with pytest.raises(ValueError, match="set_paths"):
            fc.rollout_route(tk, *ins, steps=2)
        fc.set_paths([road])
        for kw in (dict(steps=2, lane=33), dict(steps=2, back=-1), dict(steps=-1), dict(steps=4097)):
            with pytest.raises(ValueError, match="rollout_route"):
                fc.rollout_route(tk, *ins, **kw)
        with pytest.raises(ValueError, match="int32"):
            fc.rollout_route(tk.to(torch.int64), *ins, steps=2)
        with pytest.raises(ValueError, match="shape"):
            fc.plant_step(*ins[:6], ins[6][:5].contiguous())
        r = fc.rollout_route(tk, *ins, steps=0, record=True)                      # no step: nothing moves, slot 0 holds the poses
        assert isinstance(r, FleetRollout) and r._fields == FleetLaneStep._fields + ("tally", "counts", "traj")
        _bits(_host(ins), pose, "poses after a rollout of no step"); _bits(r.traj.cpu().numpy()[0], pose, "slot 0")
        assert (fc.lane_idx.cpu().numpy() == -1).all() and (fc.counts.cpu().numpy() == 0).all()

        # the C ABI behind a real solver and bank: the new arguments are refused behind the lane step's own
        from ad_mpc_amd.config import AdmpcLaneParams
        ok = AdmpcLaneParams(L=64, back=8, ahead=64)

        def call(**over):
            a = dict(s=fc._eng._h, model=None, plant=C.byref(fc._plant), B=B, T=2, tk=_p(tk), work=_p(fc._work), tally=_p(fc.tally), counts=_p(fc.counts))
            a.update(over)
            return L.admpc_rollout_lane_batch(a["s"], fc._bank, C.byref(ok), C.byref(fc._prm), a["model"], a["plant"], a["B"], a["T"], a["tk"],
                                              _p(fc.lane_idx), *[_p(t) for t in ins], _p(fc.x_opt), _p(fc.w_opt), _p(fc.safe_count), _p(fc.prev_u),
                                              _p(fc.has_valid), a["work"], _p(fc.ack), _p(fc.mode), _p(fc.valid), _p(fc.status), _p(fc.cost),
                                              a["tally"], a["counts"], None, fc._eng._stream())

        def refused(rc, words):
            assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

        before = TL._state(fc)
        refused(call(plant=None), "plant parameters are not set")
        refused(call(B=-1), "negative batch")
        other = TL._controller(40, B)
        refused(call(s=other._eng._h), "H must equal")
        other.close()
        refused(call(tk=C.c_void_p(0)), "admpc_rollout_lane_batch: null array")
        refused(call(work=C.c_void_p(0)), "admpc_rollout_lane_batch: null array")
        refused(call(T=-1), "T must be in [0, 4096]")
        refused(call(T=4097), "T must be in [0, 4096]")
        refused(call(tally=C.c_void_p(0)), "null tally or counts")
        refused(call(counts=C.c_void_p(0)), "null tally or counts")
        assert call(B=0) == 0 and call(T=0) == 0 and call(T=0, tally=C.c_void_p(0)) == 0
        refused(L.admpc_plant_step_batch(gp._h, C.byref(fc._plant), B, None, _p(fc.mode), *[_p(t) for t in ins], None), "null array")
        assert L.admpc_plant_step_batch(gp._h, C.byref(fc._plant), 0, None, None, *([None] * 7), None) == 0
        after = TL._state(fc)
        for k in TL.STATE:
            _bits(after[k], before[k], "%s after refused calls" % k)
        _bits(_host(ins), pose, "poses after refused calls")

        # set_plant(model=...): the plant integrates that solver's vehicle and GP, the controller keeps its own
        fc.set_plant(dt=0.05, blend_min=3.0, blend_max=5.0)
        fc.rollout_route(tk, *ins, steps=2)
        start = _host(ins)
        own, theirs = _poses(start), _poses(start)
        fc.plant_step(*own)
        fc.set_plant(dt=0.05, blend_min=3.0, blend_max=5.0, model=gp)
        fc.plant_step(*theirs)
        torch.cuda.synchronize()
        direct = _run_plant(gp, fc._plant, start.T.copy(), fc.ack.cpu().numpy(), fc.mode.cpu().numpy())
        _bits(_host(theirs), np.ascontiguousarray(direct.T), "plant_step with another model against the library call on that model")
        assert np.abs(_host(theirs) - _host(own))[3:6].max() > 1e-6              # the GP residual acts on v_x, v_y and the yaw rate
    finally:
        fc.close(); gp.close()
