"""The quadrotor's closed loop on the device (include/admpc_quad_fleet.h; ad_mpc_amd/quad_fleet.py).

The window is a gather and is compared bit for bit with its numpy spec (tests/quad_plant_spec.py).  The plant step is compared with the
spec -- which tests/test_quad_fleet_cpu.py holds against the reference's own simulator at 1e-15 -- and with the reference-made golden
vectors at substeps * 1e-12 relative to max(1, |ref|), element by element: the per-sub-step bound tests/test_plant_gpu.py holds the
car's plant to, summed over the sub-steps.  The rollout is compared bit for bit with the loop it replaces, driven from Python by the
window, the solve, the plant step and the index update; and with the CPU closed loop of the oracle's solve and the spec's plant."""
import ctypes as C
import json

import numpy as np
import pytest

import gen_quad_plant_golden as GG
import quad_plant_spec as QS

pytestmark = pytest.mark.gpu

RTOL = 1e-12
PLANTS = [(False, False), (True, False), (True, True)]          # (drag, payload)


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
    return t if dtype is None else t.to(dtype)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = got.view(np.uint8).reshape(-1) == want.view(np.uint8).reshape(-1)
    assert same.all(), (what, int((~same).sum()), "bytes differ")


def _lib():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ad_mpc_amd import _lib as L
    return L.load()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _plant(drag=False, payload=False, substeps=1, dt=GG.DT):
    from ad_mpc_amd.quad_config import SimQuad, quad_plant_params
    p = quad_plant_params(SimQuad(drag=drag, payload=payload), dt, dt)
    p.substeps = substeps
    return p


class _Bank:
    """A trajectory bank of the library over host arrays [(traj, u), ...]."""

    def __init__(self, L, trajs):
        self.L, self.trajs = L, [(np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)) for t, u in trajs]
        K = len(self.trajs)
        M = (C.c_int32 * K)(*[t.shape[0] for t, _ in self.trajs])
        tp = (C.c_void_p * K)(*[t.ctypes.data for t, _ in self.trajs])
        up = (C.c_void_p * K)(*[u.ctypes.data for _, u in self.trajs])
        self.h = C.c_void_p(0)
        assert L.admpc_quad_traj_bank_create(0, K, M, tp, up, C.byref(self.h)) == 0, L.admpc_last_error()

    def chunk(self, traj_of, idx, N, over, pos=True):
        import torch
        B = len(traj_of)
        yref = torch.full((B, N, 17), 7.0, dtype=torch.float64, device="cuda:0")
        yref_e = torch.full((B, 13), 7.0, dtype=torch.float64, device="cuda:0")
        pos_ref = torch.full((B, 3), 7.0, dtype=torch.float64, device="cuda:0") if pos else None
        tk, ix = _dev(traj_of, torch.int32), _dev(idx, torch.int32)
        rc = self.L.admpc_quad_ref_chunk_batch(self.h, B, N, over, _p(tk), _p(ix), _p(yref), _p(yref_e), _p(pos_ref), _stream())
        assert rc == 0, self.L.admpc_last_error()
        torch.cuda.synchronize()
        return yref, yref_e, pos_ref

    def close(self):
        self.L.admpc_quad_traj_bank_destroy(self.h)


def _random_bank(Ms, seed=5):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((M, 13)), rng.standard_normal((M, 4))) for M in Ms]


def _run_plant(L, plant, X, U, stride=4):
    """admpc_quad_plant_step_batch on copies of the inputs: the new states [B,13]."""
    import torch
    x = _dev(X)
    if stride == 4:
        u = _dev(U)
    else:
        u = torch.full((X.shape[0], stride), float("nan"), dtype=torch.float64, device="cuda:0")
        u[:, :4] = _dev(U)
    rc = L.admpc_quad_plant_step_batch(C.byref(plant), 0, X.shape[0], _p(u), stride, _p(x), _stream())
    assert rc == 0, L.admpc_last_error()
    return _host(x)


def _close(got, want, bound, what):
    ratio = np.abs(got - want) / (bound * np.maximum(1.0, np.abs(want)))
    print("%s: largest |device - reference| over its bound: %.3g" % (what, ratio.max()))
    assert not np.isnan(got).any() and ratio.max() <= 1.0, (what, ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))


_SPEC = {}


def _spec67(drag, payload, substeps):
    """The spec's result for the 67 vehicles of QS.fleet67, computed once per plant."""
    key = (drag, payload, substeps)
    if key not in _SPEC:
        X, U = QS.fleet67()
        _SPEC[key] = QS.step_batch(_plant(drag, payload, substeps), X, U)
    return _SPEC[key]


# ---- 1. the window ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,over", [(10, 1), (10, 5), (20, 1), (20, 5)])
def test_window_equals_the_spec_bit_for_bit(N, over):
    """B = 67 on K = 3 trajectories of 7 (shorter than one window), 61 and 120 rows; idx spread over each, M - 1 included; vehicle 11 on a
    trajectory the bank does not hold, vehicle 12 below it, vehicles 13 and 14 with idx = M and -1: NaN rows, the neighbours untouched."""
    L = _lib()
    trajs = _random_bank((7, 61, 120))
    Ms = np.array([7, 61, 120])
    B = 67
    traj_of = (np.arange(B) % 3).astype(np.int32)
    idx = np.array([min(Ms[traj_of[b]] - 1, int(round((b // 3) / 21.0 * (Ms[traj_of[b]] - 1)))) for b in range(B)], dtype=np.int32)
    traj_of[11], traj_of[12] = 3, -1
    idx[13], idx[14] = Ms[traj_of[13]], -1
    for k in range(3):
        assert (idx[traj_of == k] == Ms[k] - 1).any() and (idx[traj_of == k] == 0).any()
    bank = _Bank(L, trajs)
    try:
        yref, yref_e, pos = [_host(t) for t in bank.chunk(traj_of, idx, N, over)]
        only = bank.chunk(traj_of, idx, N, over, pos=False)
    finally:
        bank.close()
    want = QS.chunk_batch(trajs, traj_of, idx, N, over)
    for got, w, what in zip((yref, yref_e, pos), want, ("yref", "yref_e", "pos_ref")):
        assert np.array_equal(np.isnan(got), np.isnan(w)), what
        _bits(np.nan_to_num(got, nan=-1.0), np.nan_to_num(w, nan=-1.0), what)
    lost = [11, 12, 13, 14]
    assert np.isnan(yref[lost]).all() and np.isnan(yref_e[lost]).all() and np.isnan(pos[lost]).all()
    assert np.isnan(yref).reshape(B, -1).any(axis=1).sum() == 4
    _bits(np.nan_to_num(_host(only[0]), nan=-1.0), np.nan_to_num(yref, nan=-1.0), "yref without pos_ref")
    assert only[2] is None


# ---- 2. the plant against the spec and the golden vectors ---------------------------------------------------------------------------

@pytest.mark.parametrize("substeps", [1, 40])
@pytest.mark.parametrize("drag,payload", PLANTS)
def test_plant_matches_the_spec_and_the_golden_vectors(drag, payload, substeps):
    """B = 67 (no multiple of the 64 vehicles of a wave): activations on both sides of [0, 1], one NaN activation (vehicle 9), one
    body-frame velocity component exactly 0 (vehicle 5).  Bound: substeps * 1e-12 * max(1, |ref|).  The chain's Jacobian gain is not
    carried: this input set does not need it -- the largest ratio, printed below, was 2.3e-4 on the MI355X.  Then the same plant on the
    twelve vehicles of tests/golden/quad_plant_vectors.json against what the reference's own simulator gave, at the same bound."""
    L = _lib()
    X, U = QS.fleet67()
    assert (U[np.isfinite(U)] < 0).any() and (U[np.isfinite(U)] > 1).any() and np.isnan(U[9, 2]) and np.isnan(U).sum() == 1
    assert QS.rot(QS.conj(X[5, 3:7])).dot(X[5, 7:10])[1] == 0.0
    plant = _plant(drag, payload, substeps)
    want, replaced = _spec67(drag, payload, substeps)
    assert replaced.sum() == 1 and replaced[9]
    got = _run_plant(L, plant, X, U)
    _close(got, want, substeps * RTOL, "plant, drag=%s payload=%s substeps=%d" % (drag, payload, substeps))
    assert np.abs(got - X).max() > 1e-4
    _bits(_run_plant(L, plant, X, U), got, "a second call on the same inputs")
    _bits(_run_plant(L, plant, X, U, stride=40), got, "rows of u 40 doubles apart")
    with open(GG.OUT) as f:
        doc = json.load(f)
    case = [c for c in doc["cases"] if (c["drag"], c["payload"], c["substeps"]) == (drag, payload, substeps)]
    assert len(case) == 1 and doc["dt"] == plant.dt
    Xg, Ug = np.array(doc["x"]), np.array(doc["u"])
    _close(_run_plant(L, plant, Xg, Ug), np.array(case[0]["result"]), substeps * RTOL, "golden vectors of the reference's simulator")


# ---- 3. past the grid ---------------------------------------------------------------------------------------------------------------

def test_plant_and_window_past_the_grid():
    """B = 4096 * 64 + 301 with one sub-step: the plant's stride loop runs and its last wave is partial.  The 67 vehicles of test 2 tiled
    (4096 * 64 is no multiple of 67): vehicle b ends as vehicle b mod 67, and a sample -- the first, the last, those around the stride
    boundary -- is held against the spec.  The window at the same B covers its grid of 4096 * 256 threads 46 times; its vehicles repeat
    with period 21, and the sample around every thread-stride boundary's first vehicle is held against the spec."""
    import torch
    L = _lib()
    B = QS.PAST_THE_GRID
    assert B == 4096 * 64 + 301 and (4096 * 64) % 67 != 0
    X, U = QS.fleet67()
    t = np.arange(B) % 67
    plant = _plant(True, True, 1)
    got = _run_plant(L, plant, X[t], U[t])
    _bits(got, got[:67][t], "vehicle b against vehicle b mod 67")
    want, _ = _spec67(True, True, 1)
    sample = np.array([0, 1, 63, 64, 4096 * 64 - 1, 4096 * 64, 4096 * 64 + 1, 4096 * 64 + 63, 4096 * 64 + 64, B - 1])
    _close(got[sample], want[sample % 67], RTOL, "past the grid, the sample")

    N, over = 10, 5
    trajs = _random_bank((7, 61, 120))
    traj_of = (np.arange(B) % 3).astype(np.int32)
    idx = ((np.arange(B) // 3) % 7).astype(np.int32)
    W = N * 17 + 13 + 3
    cover = QS.CHUNK_GRID * QS.CHUNK_THREADS
    assert B * W > 40 * cover
    sample = np.unique(np.concatenate([[0, 1, B - 2, B - 1]] + [[r * cover // W - 1, r * cover // W, r * cover // W + 1] for r in range(1, B * W // cover + 1)]))
    sample = sample[sample < B]
    bank = _Bank(L, trajs)
    try:
        yref, yref_e, pos = bank.chunk(traj_of, idx, N, over)
        period = torch.arange(B, device="cuda:0") % 21
        for a in (yref, yref_e, pos):
            assert torch.equal(a, a[:21][period])
        pick = torch.as_tensor(sample, device="cuda:0")
        got = [_host(a[pick]) for a in (yref, yref_e, pos)]
    finally:
        bank.close()
    for g, w, what in zip(got, QS.chunk_batch(trajs, traj_of[sample], idx[sample], N, over), ("yref", "yref_e", "pos_ref")):
        _bits(g, w, "%s past the grid" % what)


# ---- 4. the rollout against the loop it replaces ------------------------------------------------------------------------------------

STATE = ("x", "idx", "x_opt", "w_opt", "status", "yref", "yref_e", "counts")


def _state(fl):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(fl, k).cpu().numpy() for k in STATE + ("tally", "cost", "iters")}


def _fleet(B, N, trajs, traj_of, idx0, x0, drag=True):
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    fl = QuadFleet(B, quad=SimQuad(drag=drag), n_nodes=N)
    fl.set_trajectories(trajs)
    fl.reset(traj_of, idx0, x0)
    return fl


def _circles(N, speed):
    from ad_mpc_amd.quad_scenarios import circle_reference
    dt = 1.0 / (N * 5)
    return [circle_reference(120, dt, 5.0, speed), circle_reference(9, dt, 4.0, speed, z=1.5)]


def _start(trajs, traj_of, idx0, seed):
    """The row idx0 of each vehicle's trajectory (that of trajectory 0 for a vehicle without one), moved by up to 0.3 m."""
    rng = np.random.default_rng(seed)
    x0 = np.stack([trajs[k if 0 <= k < len(trajs) else 0][0][i] for k, i in zip(traj_of, idx0)])
    x0[:, 0:3] += rng.uniform(-0.3, 0.3, (len(traj_of), 3))
    return x0


def _python_loop(fl, trajs, T):
    """The loop the rollout replaces, on the controller `fl`: window, solve, plant step under w_opt[:, 0], index update, each a call of its
    own; the tally and the counts by the spec.  Returns (traj [T+1,B,13], u [T,B,4], tally, counts)."""
    import torch
    B = fl.B
    pos = torch.empty((B, 3), dtype=torch.float64, device=fl.device)
    tally, counts = np.zeros((B, 3)), np.zeros((B, 3), dtype=np.int32)
    traj, us = [_host(fl.x)], []
    traj_of = _host(fl.traj_of)
    for _ in range(T):
        fl.ref_chunk(pos_ref=pos)
        fl._eng.solve(fl.x, fl.yref, fl.yref_e, fl.x_opt, fl.w_opt, fl.cost, fl.status, fl.iters)
        u0, st, pr, x = _host(fl.w_opt)[:, 0, :].copy(), _host(fl.status), _host(pos), _host(fl.x)
        for b in range(B):
            QS.tally_step(tally[b], counts[b], pr[b], x[b], st[b], not np.isfinite(u0[b]).all())
        fl.plant_step(fl.w_opt[:, 0, :])
        fl.idx.copy_(torch.as_tensor(QS.next_idx(trajs, traj_of, _host(fl.idx))))
        us.append(u0); traj.append(_host(fl.x))
    fl.counts.copy_(torch.as_tensor(counts))
    return np.stack(traj), np.stack(us), tally, counts


@pytest.mark.parametrize("N,B,T", [(10, 67, 6), (20, 33, 3)])
def test_rollout_equals_the_loop_it_replaces(N, B, T):
    """Vehicles on a circle of 120 rows and on one of 9 rows (started at row 6, they reach M - 1 = 8 and hold there); vehicle 3 on a
    trajectory the bank does not hold: status 4 on every step, its iterate untouched, counted, and -- against a third controller on which
    it has a trajectory -- its neighbours not affected.  N = 20 runs the two-wave kernel."""
    trajs = _circles(N, 3.0)
    traj_of = (np.arange(B) % 2).astype(np.int32)
    idx0 = np.where(traj_of == 1, 6, (np.arange(B) * 3) % 110).astype(np.int32)
    lost = 3
    x0 = _start(trajs, traj_of, idx0, seed=N)
    traj_of[lost] = 5
    good_of = traj_of.copy(); good_of[lost] = 1
    whole, loop, good = (_fleet(B, N, trajs, k, idx0, x0) for k in (traj_of, traj_of, good_of))
    try:
        out = whole.rollout(T, record=True)
        ref = good.rollout(T, record=True)
        traj, us, tally, counts = _python_loop(loop, trajs, T)
        got, want, other = _state(whole), _state(loop), _state(good)
        for k in STATE:
            nan = np.isnan(want[k]) if want[k].dtype == np.float64 else None
            if nan is not None and nan.any():
                assert np.array_equal(np.isnan(got[k]), nan), k
                _bits(np.nan_to_num(got[k], nan=-1.0), np.nan_to_num(want[k], nan=-1.0), k)
            else:
                _bits(got[k], want[k], k)
        _bits(_host(out.traj), traj, "traj_out"); _bits(_host(out.u), us, "u_out")
        _bits(got["tally"], tally, "tally against the spec's accumulation over the loop")
        ok = np.arange(B) != lost
        e = np.linalg.norm(_window_pos(trajs, traj_of, idx0, T) - traj[:T, :, 0:3], axis=2)[:, ok]             # [T,B-1], by numpy
        want_tally = np.stack([e.sum(0), (e ** 2).sum(0), e.max(0)], axis=1)
        assert (np.abs(got["tally"][ok] - want_tally) <= 1e-14 * np.abs(want_tally)).all()
        assert (got["tally"][lost] == 0).all() and got["counts"][lost].tolist() == [T, T, 0] and got["status"][lost] == 4
        assert (got["x_opt"][lost] == 0).all() and (got["w_opt"][lost] == 0).all()               # the iterate of a vehicle without a window
        assert got["idx"][lost] == idx0[lost] and np.isnan(got["yref"][lost]).all()
        assert (got["counts"][ok] == [T, 0, 0]).all() and (got["tally"][ok, 2] > 0.01).all()
        held = ok & (traj_of == 1)
        assert (got["idx"][held] == 8).all() and (idx0[held] + T > 8).all() and (got["idx"][ok & (traj_of == 0)] == idx0[ok & (traj_of == 0)] + T).all()
        assert np.abs(traj[T] - traj[0])[ok, 0:3].max() > 0.05
        for k in STATE + ("tally",):                                                             # the neighbours of the lost vehicle
            _bits(got[k][ok], other[k][ok], "%s of the neighbours" % k)
        _bits(_host(out.traj)[:, ok], _host(ref.traj)[:, ok], "traj_out of the neighbours")
        assert other["counts"][lost].tolist() == [T, 0, 0]
        rm = _host(whole.tracking_rmse())
        assert np.array_equal(rm[ok], got["tally"][ok, 0] / T) and rm[lost] == 0.0
    finally:
        for fl in (whole, loop, good):
            fl.close()


def _window_pos(trajs, traj_of, idx0, T):
    """[T,B,3]: the position of row idx of every step, idx advancing by one and holding at M - 1 (NaN rows never enter: the caller masks)."""
    out = np.zeros((T, len(traj_of), 3))
    idx = np.array(idx0)
    for t in range(T):
        for b, k in enumerate(traj_of):
            out[t, b] = trajs[k][0][idx[b], :3] if 0 <= k < len(trajs) else np.nan
        idx = QS.next_idx(trajs, traj_of, idx)
    return out


# ---- 5. the rollout against the CPU closed loop -------------------------------------------------------------------------------------

def _cpu_loop(oracle, cfg, plant, trajs, traj_of, idx0, x0, T, over):
    """The oracle's RTI step and the spec's plant in closed loop: (traj [T+1,B,13], status [T,B], iters [T,B])."""
    B, N = len(traj_of), cfg.N
    x, idx = np.array(x0), np.array(idx0)
    xbar, ubar = np.zeros((B, N + 1, 13)), np.zeros((B, N, 4))
    traj, sts, its = [x.copy()], [], []
    for _ in range(T):
        yref, yref_e, _ = QS.chunk_batch(trajs, traj_of, idx, N, over)
        xbar, ubar, _, st, it = oracle.solve_batch(cfg, x, yref, yref_e, xbar, ubar)
        x, _ = QS.step_fleet(plant, x, ubar[:, 0, :])
        idx = QS.next_idx(trajs, traj_of, idx)
        traj.append(x.copy()); sts.append(st.copy()); its.append(it.copy())
    return np.stack(traj), np.stack(sts), np.stack(its)


@pytest.mark.parametrize("N,speed", [(10, 3.0), (20, 6.0)])
def test_rollout_follows_the_cpu_closed_loop(N, speed):
    """8 vehicles on circle_reference(120, control_period, 5.0, speed), drag on: start offsets 0 and 0.3 m * (1, -1, 0.5), start rows 0 and
    95 (the truncated windows are crossed), two of each.  T = 25.  Statuses identical on every step.  The states stay within
    1e-8 * T * S of the CPU loop's: 1e-8 is the project's device-against-oracle parity of one solve for N <= 32, and S, measured here, is
    the closed loop's own sensitivity -- the largest change of the CPU trajectory per unit change of the start, for a start moved by 1e-8
    in position and velocity, floored at 1."""
    from ad_mpc_amd.quad_scenarios import circle_reference
    from oracle.quad_oracle import QuadOracle
    T, B, over = 25, 8, 5
    dt = 1.0 / (N * over)
    trajs = [circle_reference(120, dt, 5.0, speed)]
    traj_of = np.zeros(B, dtype=np.int32)
    idx0 = np.array([0, 0, 95, 95, 0, 0, 95, 95], dtype=np.int32)
    x0 = np.stack([trajs[0][0][i] for i in idx0])
    x0[[1, 3, 5, 7], 0:3] += 0.3 * np.array([1.0, -1.0, 0.5])
    x0[4:, 7:10] *= 0.9                                                                          # the second pair of each starts slower
    fl = _fleet(B, N, trajs, traj_of, idx0, x0)
    try:
        oracle = QuadOracle()
        cpu, sts, its = _cpu_loop(oracle, fl.cfg, fl._plant, trajs, traj_of, idx0, x0, T, over)
        moved = x0.copy(); moved[:, 0:3] += 1e-8; moved[:, 7:10] += 1e-8
        S = max(1.0, float(np.abs(_cpu_loop(oracle, fl.cfg, fl._plant, trajs, traj_of, idx0, moved, T, over)[0] - cpu).max() / 1e-8))
        got, dev_st = [_host(fl.x)], []
        for _ in range(T):
            fl.step()
            got.append(_host(fl.x)); dev_st.append(_host(fl.status))
        got, dev_st = np.stack(got), np.stack(dev_st)
    finally:
        fl.close()
    err = float(np.abs(got - cpu).max())
    print("N = %d: closed-loop sensitivity S = %.3f, IPM iterations %d .. %d, max |device - CPU loop| = %.3g (bound %.3g)"
          % (N, S, its.min(), its.max(), err, 1e-8 * T * S))
    assert np.array_equal(dev_st, sts) and (sts == 0).all()
    assert err <= 1e-8 * T * S
    assert np.abs(got[T] - got[0])[:, 0:3].max() > 0.5


# ---- 6. graph -----------------------------------------------------------------------------------------------------------------------

def test_captured_rollout_replays_the_eager_result():
    """rollout(T = 3) at B = 67 captured with torch.cuda.graph (its own side stream) and replayed twice from re-seeded inputs.  The chain
    is linear: window, solve, plant, three times."""
    import torch
    N, B, T = 10, 67, 3
    trajs = _circles(N, 3.0)
    traj_of = (np.arange(B) % 2).astype(np.int32)
    seeds = []
    for r in range(2):
        idx0 = np.where(traj_of == 1, 4 + r, (np.arange(B) * 5 + 11 * r) % 110).astype(np.int32)
        seeds.append((idx0, _start(trajs, traj_of, idx0, seed=80 + r)))
    eager, graphed = (_fleet(B, N, trajs, traj_of, *seeds[0]) for _ in range(2))
    try:
        graphed.rollout(T)                                          # every kernel has run once before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = graphed.rollout(T, record=True)
        for r in range(2):
            eager.reset(traj_of, *seeds[r]); graphed.reset(traj_of, *seeds[r])
            ref = eager.rollout(T, record=True)
            g.replay()
            want, got = _state(eager), _state(graphed)
            for k in STATE + ("tally", "cost", "iters"):
                _bits(got[k], want[k], "%s at replay %d" % (k, r))
            _bits(_host(out.traj), _host(ref.traj), "traj at replay %d" % r); _bits(_host(out.u), _host(ref.u), "u at replay %d" % r)
            assert (want["counts"] == [T, 0, 0]).all() and np.array_equal(_host(ref.traj)[0], seeds[r][1])
    finally:
        eager.close(); graphed.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_in_their_order_and_the_no_ops():
    """Every refusal the header lists, naming its argument, in the listed order (a call that breaks two rules is refused for the first);
    nothing on the device moves.  The bank on another device needs a second GPU and is not exercised here."""
    import torch
    from ad_mpc_amd.engine import QuadBatchSolver
    from ad_mpc_amd.quad_config import default_quad_config
    N, B = 10, 5
    trajs = _circles(N, 3.0)
    traj_of = np.zeros(B, dtype=np.int32)
    idx0 = np.arange(B, dtype=np.int32)
    fl = _fleet(B, N, trajs, traj_of, idx0, None)
    sqp_cfg = default_quad_config(); sqp_cfg.sqp_iters = 3
    sqp = QuadBatchSolver(sqp_cfg)
    L = fl.lib
    null = C.c_void_p(0)
    try:
        def roll(**over):
            a = dict(s=fl._eng._h, bank=fl._bank, plant=C.byref(fl._plant), over=5, B=B, T=2, traj_of=_p(fl.traj_of), idx=_p(fl.idx), x=_p(fl.x),
                     status=_p(fl.status), tally=_p(fl.tally), counts=_p(fl.counts))
            a.update(over)
            return L.admpc_quad_rollout_batch(a["s"], a["bank"], a["plant"], a["over"], a["B"], a["T"], a["traj_of"], a["idx"], a["x"], _p(fl.x_opt),
                                              _p(fl.w_opt), _p(fl.yref), _p(fl.yref_e), _p(fl.cost), a["status"], _p(fl.iters), a["tally"],
                                              a["counts"], None, None, fl._stream())

        def refused(rc, words):
            assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

        bad = fl._plant.copy(); bad.substeps = 0
        before = _state(fl)
        refused(roll(s=null, bank=null), "null solver")
        refused(roll(s=sqp._h, bank=null), "sqp_iters > 1")
        refused(roll(bank=null, plant=None), "null bank")
        refused(roll(plant=None, over=0), "plant parameters are not set")
        refused(roll(plant=C.byref(bad), over=0), "substeps must be in [1, 1024]")
        refused(roll(over=0, B=-1), "over must be at least 1")
        refused(roll(B=-1, T=-1), "negative batch")
        refused(roll(T=-1, x=null), "T must be in [0, 4096]")
        refused(roll(T=4097), "T must be in [0, 4096]")
        for k in ("traj_of", "idx", "x", "status"):
            refused(roll(tally=null, **{k: null}), "admpc_quad_rollout_batch: null array")
        refused(roll(tally=null), "null tally or counts")
        refused(roll(counts=null), "null tally or counts")
        assert roll(B=0, x=null) == 0 and roll(T=0, x=null, tally=null) == 0

        chunk = lambda bank=fl._bank, B=B, N=N, over=5, yref=_p(fl.yref): L.admpc_quad_ref_chunk_batch(
            bank, B, N, over, _p(fl.traj_of), _p(fl.idx), yref, _p(fl.yref_e), None, fl._stream())
        refused(chunk(bank=null, B=-1), "null bank")
        refused(chunk(B=-1, N=1), "negative batch")
        refused(chunk(N=1, over=0), "N must be in [2, 24]")
        refused(chunk(N=25), "N must be in [2, 24]")
        refused(chunk(over=0, yref=null), "over must be at least 1")
        refused(chunk(yref=null), "null array")
        assert chunk(B=0, yref=null) == 0

        plant = lambda p=C.byref(fl._plant), dev=0, B=B, u=_p(fl.w_opt), stride=N * 4: L.admpc_quad_plant_step_batch(p, dev, B, u, stride, _p(fl.x), fl._stream())
        refused(plant(p=None, B=-1), "plant parameters are not set")
        refused(plant(p=C.byref(bad), B=-1), "substeps must be in [1, 1024]")
        refused(plant(B=-1, u=null), "negative batch")
        refused(plant(u=null, stride=3), "null array")
        refused(plant(stride=3), "u_stride must be at least 4")
        assert plant(dev=99) == -2 and b"no such device" in L.admpc_last_error()
        assert plant(B=0, u=null) == 0

        h = C.c_void_p(0)
        x = np.zeros((2, 13)); u = np.zeros((2, 4))
        tp, up = (C.c_void_p * 1)(x.ctypes.data), (C.c_void_p * 1)(u.ctypes.data)
        refused(L.admpc_quad_traj_bank_create(0, 1, None, tp, up, C.byref(h)), "null argument")
        refused(L.admpc_quad_traj_bank_create(0, 0, (C.c_int32 * 1)(2), tp, up, C.byref(h)), "K must be at least 1")
        refused(L.admpc_quad_traj_bank_create(0, 1, (C.c_int32 * 1)(0), tp, up, C.byref(h)), "M >= 1")
        refused(L.admpc_quad_traj_bank_create(0, 1, (C.c_int32 * 1)(2), (C.c_void_p * 1)(None), up, C.byref(h)), "null trajectory")
        assert L.admpc_quad_traj_bank_create(99, 1, (C.c_int32 * 1)(2), tp, up, C.byref(h)) == -2 and not h.value
        L.admpc_quad_traj_bank_destroy(None)

        dev, n, sq = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        assert L.admpc_quad_solver_info(sqp._h, C.byref(dev), C.byref(n), C.byref(sq)) == 0 and (dev.value, n.value, sq.value) == (0, 10, 3)
        after = _state(fl)
        for k in STATE + ("tally",):
            _bits(after[k], before[k], "%s after refused calls" % k)

        # the Python layer
        with pytest.raises(ValueError, match="rollout"):
            fl.rollout(-1)
        with pytest.raises(ValueError, match="rollout"):
            fl.rollout(4097)
        with pytest.raises(ValueError, match="plant_step"):
            fl.plant_step(fl.w_opt[:, 0, :3])
        with pytest.raises(ValueError, match="x0 is needed"):
            fl.reset(np.full(B, 7), 0)
        r = fl.rollout(0, record=True)
        _bits(_host(r.traj)[0], before["x"], "slot 0 of a rollout of no step")
        assert r.u.shape == (0, B, 4) and (_host(fl.counts) == 0).all()
        from ad_mpc_amd.quad_fleet import QuadFleet
        fresh = QuadFleet(2)
        try:
            with pytest.raises(ValueError, match="set_trajectories"):
                fresh.rollout(1)
        finally:
            fresh.close()
    finally:
        fl.close(); sqp.close()
