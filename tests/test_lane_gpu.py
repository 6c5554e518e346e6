"""The fleet step along a route on the device (include/admpc_lane.h; ad_mpc_amd/fleet.py: step_route).

The generator is compared with its numpy / scipy restatement (tests/lane_spec.py, pinned to the reference's own RefTrajectory by
test_lane_cpu.py): the six rows and out_err to atol 1e-12, the tolerance test_ref_traj.py uses for this kernel family; stop and
lane_idx exactly.  Chosen poses lie at least 0.2 m from every perpendicular bisector between the nearest waypoint and another one (its
neighbours first of all; checked with the spec), so that the nearest index cannot hinge on rounding; the tie cases use exactly representable coordinates.  The step is compared
with the EXISTING admpc_control_step_bank_batch run on a bank that holds, as path b, the lane table the spec builds for vehicle b."""
import ctypes as C

import numpy as np
import pytest

import lane_spec as LS
import path_bank as PB

pytestmark = pytest.mark.gpu

T_HORIZON, OPT_DT = 1.0, 0.01
ATOL = 1e-12
ACC_MAX = 3.0
STATE = ("ack", "mode", "status", "valid", "x_opt", "w_opt", "safe_count", "prev_u", "has_valid", "cost", "lane_idx")


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _lib():
    import torch  # noqa: F401  torch's HIP runtime is loaded before libadmpc.so, the order ad_mpc_amd.engine loads them in
    from ad_mpc_amd import _lib
    return _lib.load()


def _wrap(a):
    return (a + np.pi) % (2.0 * np.pi) - np.pi


def _curved(M, psi0, ds=0.5, seed=0.0):
    """(vel, x, y, psi): waypoints ds apart, varying curvature; psi0 = 2.8 makes the yaw cross +-pi within the first 40 waypoints."""
    s = ds * np.arange(M)
    psi = psi0 + 0.9 * np.sin(s / 11.0 + seed) + 0.01 * s
    x = np.concatenate(([0.0], np.cumsum(np.cos(psi[:-1]) * ds))) + 3.0
    y = np.concatenate(([0.0], np.cumsum(np.sin(psi[:-1]) * ds))) - 7.0
    return 7.0 + 4.0 * np.sin(s / 9.0 + seed), x, y, _wrap(psi)


def _beside(route, i, e):
    """The point e m to the left of waypoint i."""
    _, x, y, psi = route
    return x[i] - e * np.sin(psi[i]), y[i] + e * np.cos(psi[i])


def _bank_of_routes(routes, H, dt):
    """A bank whose paths carry the four columns the lane generator reads (the other three are placeholders).  (handle, keep-alive)."""
    from ad_mpc_amd.config import AdmpcPath
    L = _lib()
    dev = [[_dev(c) for c in r] for r in routes]
    descs = (AdmpcPath * len(dev))()
    for d, (vel, x, y, psi) in zip(descs, dev):
        d.M, d.H, d.dt = int(x.shape[0]), H, dt
        d.vel, d.x, d.y, d.psi, d.psi_unwrapped, d.cdist, d.curv = [c.data_ptr() for c in (vel, x, y, psi, psi, x, y)]
    import torch
    torch.cuda.synchronize()
    bank = C.c_void_p(0)
    assert L.admpc_path_bank_create(0, len(dev), descs, C.byref(bank)) == 0, L.admpc_last_error()
    return bank, dev


def _generate(bank, H, L_, back, ahead, path_of, lane_idx, X, Y, P, vx, vy, clamp, dt):
    import torch
    from ad_mpc_amd.config import AdmpcLaneParams
    L = _lib()
    B = len(X)
    ref = torch.full((B, 6, H), 7.0, dtype=torch.float64, device="cuda:0")
    err = torch.full((B, 3), 7.0, dtype=torch.float64, device="cuda:0")
    stop = torch.full((B,), 7, dtype=torch.int32, device="cuda:0")
    idx = _dev(lane_idx, torch.int32)
    ins = [_dev(path_of, torch.int32), idx] + [_dev(a) for a in (X, Y, P, vx, vy)]
    prm = AdmpcLaneParams(L=L_, back=back, ahead=ahead)
    rc = L.admpc_waypoints_lane_batch(bank, C.byref(prm), B, *[_p(t) for t in ins], 1 if clamp else 0, ACC_MAX, dt, _p(ref), _p(err), _p(stop), None)
    assert rc == 0, L.admpc_last_error()
    torch.cuda.synchronize()
    return ref.cpu().numpy(), err.cpu().numpy(), stop.cpu().numpy(), idx.cpu().numpy()


def _expect(routes, H, L_, back, ahead, path_of, lane_idx, X, Y, P, vx, vy, clamp, dt, loose=()):
    """The spec per vehicle; every pose not listed in `loose` is checked to lie 0.2 m clear of the bisectors of its search range."""
    out = []
    for b in range(len(X)):
        r = routes[path_of[b]]
        if b not in loose:
            assert LS.bisector_clearance(r[1], r[2], X[b], Y[b], lane_idx[b], back, ahead) >= 0.2, b
        out.append(LS.waypoints(r, lane_idx[b], X[b], Y[b], P[b], L_, back, ahead, H, dt, (vx[b], vy[b]) if clamp else None, ACC_MAX, dt))
    return out


def _compare(got, want):
    ref, err, stop, idx = got
    for b, (i0, r, e, st) in enumerate(want):
        np.testing.assert_allclose(ref[b], r, rtol=0, atol=ATOL, err_msg="out_ref of vehicle %d" % b)
        np.testing.assert_allclose(err[b], e, rtol=0, atol=ATOL, err_msg="out_err of vehicle %d" % b)
        assert stop[b] == st and idx[b] == i0, (b, stop[b], st, idx[b], i0)


# ---- 1. the generator: shapes, the route's end ------------------------------------------------------------------------------------

GEN_ROUTES = [_curved(400, 2.8), _curved(40, -0.4, seed=1.0), _curved(20, 1.0, seed=2.0)]


def _gen_fleet(L_):
    """Vehicles 0.3 m beside chosen waypoints: inside route 0 (where its yaw crosses +-pi, and further on), the lane ending exactly at the
    route's end, one past it, far past it, all padding (i0 = M - 1); routes shorter than the lane; one vehicle at rest."""
    M = len(GEN_ROUTES[0][1])
    where = [(0, 0), (0, 20), (0, 37), (0, M - L_), (0, M - L_ + 1), (0, M - 5), (0, M - 1), (1, 3), (1, 39), (2, 0), (2, 10), (0, 150)]
    rng = np.random.default_rng(L_)
    path_of = np.array([k for k, _ in where], dtype=np.int32)
    X, Y = np.array([_beside(GEN_ROUTES[k], i, 0.3 * (-1) ** n) for n, (k, i) in enumerate(where)]).T
    P = np.array([GEN_ROUTES[k][3][i] for k, i in where]) + rng.uniform(-0.2, 0.2, size=len(where))
    P[2] += 2 * np.pi; P[5] -= 2 * np.pi
    vx, vy = rng.uniform(5.0, 9.0, size=len(where)), rng.uniform(-0.2, 0.2, size=len(where))
    vx[1] = vy[1] = 0.0
    return where, path_of, X, Y, P, vx, vy


@pytest.mark.parametrize("L_,H", [(L_, H) for L_ in (34, 63, 64, 65, 256) for H in (3, 20, 64)] + [(34, 40)])
def test_generator_against_the_spec(L_, H):
    """Lanes below, at and above a wave (stride loops), H on both sides of L (H = 40 > L = 34: the speeds are padded with 0.01), with and
    without the clamp, global search."""
    dt = T_HORIZON / H
    where, path_of, X, Y, P, vx, vy = _gen_fleet(L_)
    start = np.full(len(X), -1, dtype=np.int32)
    bank, keep = _bank_of_routes(GEN_ROUTES, H, dt)
    try:
        stops = set()
        for clamp in (True, False):
            want = _expect(GEN_ROUTES, H, L_, 8, 64, path_of, start, X, Y, P, vx, vy, clamp, dt)
            assert [w[0] for w in want] == [i for _, i in where]
            got = _generate(bank, H, L_, 8, 64, path_of, start, X, Y, P, vx, vy, clamp, dt)
            _compare(got, want)
            stops |= set(got[2].tolist())
            assert got[2][6] == 1                                     # the lane that is all padding has reached the route's end
            if clamp:
                assert got[0][1, 4, 0] == 0.0                         # the vehicle at rest: its first abscissa is dt * 0
        assert stops == {0, 1}
    finally:
        _lib().admpc_path_bank_destroy(bank)


# ---- 2. the search ----------------------------------------------------------------------------------------------------------------

def _eight(M=400, a=40.0):
    """A figure-eight that crosses itself between waypoints 199 | 200 and 399 | 0."""
    t = (np.arange(M) + 0.5) * 2 * np.pi / M
    x, y = a * np.sin(t), a * np.sin(t) * np.cos(t)
    return np.full(M, 6.0), x, y, _wrap(np.arctan2(np.gradient(y), np.gradient(x)))


def _line(M=100):
    m = np.arange(M, dtype=np.float64)
    return 6.0 + np.cos(m / 5.0), m.copy(), np.zeros(M), np.zeros(M)


def test_search_window_ties_and_ends():
    H, L_ = 20, 64
    dt = T_HORIZON / H
    routes = [_eight(), _line()]
    ML = 100
    # (route, lane_idx, X, Y): see each line
    cases = [
        (0, 195, 0.25, 0.6),        # 0 at the crossing, on the branch of waypoint 200: the window's answer, though waypoint 0 is nearer
        (0, -1, 0.25, 0.6),         # 1 the same pose searched globally: waypoint 0
        (1, -1, 3.5, 1.0),          # 2 an exact tie between waypoints 3 and 4: the first
        (1, 12, 3.5, 1.0),          # 3 the same with the window [4, 76]: waypoint 4
        (1, -1, 63.5, -2.0),        # 4 a tie between the last waypoint of the scan's first pass and the first of its second: 63
        (1, ML - 3, 98.0, 0.3),     # 5 lane_idx + ahead past M
        (1, ML + 50, 97.0, 0.3),    # 6 lane_idx >= M: the window [M - 1 - back, M - 1]
        (1, 2, 1.0, 0.3),           # 7 lane_idx - back below 0
        (1, 17, np.nan, 0.0),       # 8 a non-finite pose: the first index of the window
        (1, -1, np.nan, 0.0),       # 9 and of the route
        (1, 40, 30.0, 0.3),         # 10 the vehicle is behind its window [32, 104]: the window's edge
        (0, 300, *_beside(routes[0], 310, 0.3)),     # 11 an ordinary advance
    ]
    loose = (2, 3, 4, 8, 9)
    path_of = np.array([c[0] for c in cases], dtype=np.int32)
    start = np.array([c[1] for c in cases], dtype=np.int32)
    X, Y = np.array([c[2] for c in cases]), np.array([c[3] for c in cases])
    P = np.array([0.3, 0.3, 0.1, -0.1, 0.0, 0.0, 6.4, 0.0, 0.0, 0.0, np.nan, 0.2])         # vehicle 10: a non-finite yaw as well
    vx, vy = np.full(len(cases), 6.5), np.zeros(len(cases))
    bank, keep = _bank_of_routes(routes, H, dt)
    try:
        want = _expect(routes, H, L_, 8, 64, path_of, start, X, Y, P, vx, vy, True, dt, loose)
        assert [w[0] for w in want] == [200, 0, 3, 4, 63, 98, 97, 1, 9, 0, 32, 310]
        _compare(_generate(bank, H, L_, 8, 64, path_of, start, X, Y, P, vx, vy, True, dt), want)
        # back = ahead = 0: the answer is min(lane_idx, M - 1) wherever the vehicle is; a negative lane_idx still searches the route
        want = _expect(routes, H, L_, 0, 0, path_of, start, X, Y, P, vx, vy, True, dt, range(len(cases)))
        assert [w[0] for w in want] == [195, 0, 3, 12, 63, ML - 3, ML - 1, 2, 17, 0, 40, 300]
        _compare(_generate(bank, H, L_, 0, 0, path_of, start, X, Y, P, vx, vy, True, dt), want)
    finally:
        _lib().admpc_path_bank_destroy(bank)


# ---- 3. past the grid ---------------------------------------------------------------------------------------------------------------

def test_generator_past_the_grid_with_invalid_routes():
    """B = the grid + 37: vehicle b and b + 4096 share a workgroup, on different routes.  48 distinct vehicles are tiled over the batch
    (4096 is no multiple of 48, so the two differ); every 89th path_of is outside the bank: NaN rows, stop 0, lane_idx untouched."""
    H, L_, B, D = 20, 64, LS.GRID + 37, 48
    dt = T_HORIZON / H
    rng = np.random.default_rng(5)
    k = (np.arange(D) * 5 % 3).astype(np.int32)
    at = np.array([rng.integers(0, len(GEN_ROUTES[j][1])) for j in k])
    X, Y = np.array([_beside(GEN_ROUTES[j], i, 0.3) for j, i in zip(k, at)]).T
    P = np.array([GEN_ROUTES[j][3][i] for j, i in zip(k, at)]) + rng.uniform(-0.2, 0.2, size=D)
    vx, vy = rng.uniform(5.0, 9.0, size=D), rng.uniform(-0.2, 0.2, size=D)
    start = np.where(np.arange(D) % 2 == 0, -1, np.maximum(at - 5, 0)).astype(np.int32)
    want = _expect(GEN_ROUTES, H, L_, 8, 64, k, start, X, Y, P, vx, vy, True, dt)
    assert [w[0] for w in want] == at.tolist()
    t = np.arange(B) % D
    path_of, first = k[t].copy(), start[t].copy()
    bad = np.arange(B) % 89 == 13
    path_of[bad] = np.where(np.arange(bad.sum()) % 2 == 0, -1, len(GEN_ROUTES))
    first[bad] = 1234
    bank, keep = _bank_of_routes(GEN_ROUTES, H, dt)
    try:
        ref, err, stop, idx = _generate(bank, H, L_, 8, 64, path_of, first, X[t], Y[t], P[t], vx[t], vy[t], True, dt)
    finally:
        _lib().admpc_path_bank_destroy(bank)
    assert bad[LS.GRID:].any() and np.isnan(ref[bad]).all() and np.isnan(err[bad]).all() and (stop[bad] == 0).all() and (idx[bad] == 1234).all()
    good = np.nonzero(~bad)[0]
    for name, got, j in (("out_ref", ref, 1), ("out_err", err, 2)):
        exp = np.stack([want[i][j] for i in range(D)])[t[good]]
        np.testing.assert_allclose(got[good], exp, rtol=0, atol=ATOL, err_msg=name)
    assert np.array_equal(stop[good], np.array([w[3] for w in want])[t[good]]) and np.array_equal(idx[good], at[t[good]])


# ---- 4. the step ----------------------------------------------------------------------------------------------------------------------

def _road(M=600, ds=0.5, off=0.0):
    """(x, y, psi, vel) as set_paths takes a path: a gentle wiggle about a line; `off` m to its left."""
    s = np.arange(M) * ds
    x, y = s * np.cos(0.3), s * np.sin(0.3) + 2.0 * np.sin(s / 30.0)
    psi = np.arctan2(np.sin(0.3) + 2.0 / 30.0 * np.cos(s / 30.0), np.cos(0.3) + 0 * s)
    return x - off * np.sin(psi), y + off * np.cos(psi), psi, 7.0 + 1.5 * np.sin(s / 20.0)


def _spec_route(road):
    x, y, psi, vel = road
    return vel, x, y, psi


def _along(road, at, seed):
    """[7][B]: vehicles 0.3 m off the road at the waypoints `at`, 5 .. 9 m/s."""
    rng = np.random.default_rng(seed)
    B = len(at)
    e = 0.3 * (-1.0) ** np.arange(B)
    x, y, psi, _ = road
    return np.stack([x[at] - e * np.sin(psi[at]), y[at] + e * np.cos(psi[at]), psi[at] + rng.uniform(-0.05, 0.05, size=B), rng.uniform(5.0, 9.0, size=B),
                     rng.uniform(-0.1, 0.1, size=B), rng.uniform(-0.05, 0.05, size=B), rng.uniform(-0.03, 0.03, size=B)])


def _controller(N, B, **kw):
    from ad_mpc_amd.fleet import FleetController
    return FleetController(T_HORIZON, N, OPT_DT, B, **kw)


def _state(fc):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(fc, k).cpu().numpy().copy() for k in STATE}


def _step_route(fc, path_of, pose, **kw):
    import torch
    fc.step_route(_dev(path_of, torch.int32), *[_dev(a) for a in pose], **kw)
    return _state(fc)


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


@pytest.mark.parametrize("N", [20, 40])
def test_step_route_equals_the_bank_step_on_the_specs_lanes(N):
    """70 vehicles along a 600-waypoint route.  step_route against the existing bank step (resample = 0) on a bank whose path b is the
    lane table of the spec for vehicle b; and the contrast: under step_paths on the route itself every vehicle beyond waypoint 100 gets
    the window of the route's start and an invalid prediction."""
    import torch
    from ad_mpc_amd.config import AdmpcPath
    B, L_ = 70, 64
    road = _road()
    route = _spec_route(road)
    at = np.linspace(0, 550, B).astype(int)
    pose = _along(road, at, seed=N)
    zero = np.zeros(B, dtype=np.int32)
    new, old, plain = _controller(N, B, threshold=1), _controller(N, B, threshold=1, resample=False), _controller(N, B, threshold=1)
    new.set_paths([road]); plain.set_paths([road])
    dt = T_HORIZON / N
    # the bank of the spec's lanes, descriptors built directly from the spec's columns
    tabs = []
    for b in range(B):
        assert LS.bisector_clearance(route[1], route[2], pose[0, b], pose[1, b]) >= 0.2
        i0 = LS.nearest(route[1], route[2], pose[0, b], pose[1, b])
        assert i0 == at[b]
        tabs.append(LS.lane_table(route, i0, L_, (pose[3, b], pose[4, b]), new.ad.acc_max, dt))
    cols = [[_dev(c) for c in LS.columns(t)] for t in tabs]
    descs = (AdmpcPath * B)()
    for d, cs in zip(descs, cols):
        d.M, d.H, d.dt = L_, N, dt
        d.vel, d.x, d.y, d.psi, d.psi_unwrapped, d.cdist, d.curv = [c.data_ptr() for c in cs]
    torch.cuda.synchronize()
    bank = C.c_void_p(0)
    assert old.lib.admpc_path_bank_create(0, B, descs, C.byref(bank)) == 0, old.lib.admpc_last_error()
    old._bank, old.n_paths = bank, B                                       # close() destroys it
    got = _step_route(new, zero, pose, lane=L_)
    old.step_paths(_dev(np.arange(B, dtype=np.int32)), *[_dev(a) for a in pose])
    want = _state(old)
    plain.step_paths(_dev(zero), *[_dev(a) for a in pose])
    today = _state(plain)
    try:
        assert np.array_equal(got["lane_idx"], at)
        for k in ("status", "valid", "mode"):
            assert np.array_equal(got[k], want[k]), k
        tol = 1e-8 if N <= 32 else 1e-7                                     # the project's parity bound
        np.testing.assert_allclose(got["x_opt"], want["x_opt"], rtol=0, atol=tol)
        np.testing.assert_allclose(got["w_opt"], want["w_opt"], rtol=0, atol=tol)
        np.testing.assert_allclose(got["ack"], want["ack"], rtol=2.4e-7, atol=1e-7)       # 2 float32 ulps: 1e-8 in double can cross a rounding boundary
        assert np.array_equal(np.isposinf(got["cost"]), np.isposinf(want["cost"])) and not np.isnan(got["cost"]).any()
        fin = np.isfinite(want["cost"])
        np.testing.assert_allclose(got["cost"][fin], want["cost"][fin], rtol=1e-9, atol=0)
        # the contrast
        far = at > 100
        assert far.sum() > 50 and (today["valid"][far] == 0).all(), today["valid"]
        assert (got["status"] == 0).all() and (got["valid"] == 1).all() and (got["mode"] == 1).all()
    finally:
        for fc in (new, old, plain):
            fc.close()


def test_closed_loop_and_best_of_along_the_route():
    """30 steps with the next pose taken from the prediction's stage 1: lane_idx follows the spec's index, never goes back and has
    advanced for every vehicle; after the gate's warm-up (threshold 3) every record is an MPC command.  Then V = 8 vehicles x C = 4
    candidate routes (the road, two neighbouring lanes of it and one 60 m away): best_of picks the arg-min of the step's costs."""
    import torch
    N, B, T, back, ahead = 20, 16, 30, 8, 64
    road = _road()
    route = _spec_route(road)
    at = np.linspace(3, 520, B).astype(int)
    pose = _along(road, at, seed=3)
    zero = np.zeros(B, dtype=np.int32)
    fc = _controller(N, B, threshold=3)
    fc.set_paths([road])
    prev = np.full(B, -1)
    try:
        for t in range(T):
            got = _step_route(fc, zero, pose, back=back, ahead=ahead)
            want = np.array([LS.nearest(route[1], route[2], pose[0, b], pose[1, b], prev[b], back, ahead) for b in range(B)])
            assert np.array_equal(got["lane_idx"], want), t
            assert (got["lane_idx"] >= prev).all() and (got["status"] == 0).all(), t
            if t >= 2:
                assert (got["mode"] == 1).all(), (t, got["mode"])
            prev = got["lane_idx"].copy()
            pose = np.ascontiguousarray(got["x_opt"][:, 1, :].T)
        assert (prev > at).all(), (prev, at)
    finally:
        fc.close()
    V, Cn = 8, 4
    B = V * Cn
    roads = [_road(off=1.5), road, _road(off=-1.0), _road(off=60.0)]
    at = np.linspace(40, 500, V).astype(int)
    pose = np.repeat(_along(road, at, seed=4), Cn, axis=1)
    path_of = np.tile(np.arange(Cn, dtype=np.int32), V)
    fc = _controller(N, B)
    fc.set_paths(roads)
    try:
        got = _step_route(fc, path_of, pose)
        val, idx = fc.best_of(Cn)
        torch.cuda.synchronize()
        ev, ei = PB.group_argmin(got["cost"], Cn)
        _bits(val.cpu().numpy(), ev, "val"); _bits(idx.cpu().numpy(), ei, "idx")
        assert np.isfinite(ev).all() and (ei % Cn != 3).all() and np.isposinf(got["cost"].reshape(V, Cn)[:, 3]).all()
        assert (got["status"].reshape(V, Cn)[:, :3] == 0).all() and (got["valid"].reshape(V, Cn)[:, 1] == 1).all()
        for c in range(Cn):                                                   # every candidate lane was cut at its own route's nearest waypoint
            r = _spec_route(roads[c])
            assert got["lane_idx"].reshape(V, Cn)[:, c].tolist() == [LS.nearest(r[1], r[2], pose[0, v * Cn], pose[1, v * Cn]) for v in range(V)]
    finally:
        fc.close()


# ---- 5. capture, reset, refusals ------------------------------------------------------------------------------------------------------

def test_captured_step_route_replays_the_eager_result():
    import torch
    N, B, T = 20, 24, 3
    road = _road()
    at = np.linspace(0, 500, B).astype(int)
    poses = [_along(road, at + 2 * t, seed=6) for t in range(T)]
    path_of = np.zeros(B, dtype=np.int32)
    eager, graphed = _controller(N, B, threshold=1), _controller(N, B, threshold=1)
    eager.set_paths([road]); graphed.set_paths([road])
    try:
        ref = [_step_route(eager, path_of, poses[t]) for t in range(T)]
        dev = graphed.device
        ins = [torch.zeros(B, dtype=torch.float64, device=dev) for _ in range(7)]
        tk = _dev(path_of, torch.int32)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            graphed.step_route(tk, *ins)
        graphed.lane_idx.fill_(-1)
        for t in range(T):
            for i in range(7):
                ins[i].copy_(torch.as_tensor(poses[t][i], device=dev))
            g.replay()
            got = _state(graphed)
            for k in got:
                _bits(got[k], ref[t][k], "%s at replay %d" % (k, t))
        assert np.array_equal(ref[-1]["lane_idx"], at + 2 * (T - 1)) and (ref[-1]["mode"] == 1).all()
    finally:
        eager.close(); graphed.close()


def test_reset_sends_the_masked_vehicles_back_to_a_global_search():
    N, B = 20, 8
    road = _road()
    route = _spec_route(road)
    at = np.linspace(0, 300, B).astype(int)
    zero = np.zeros(B, dtype=np.int32)
    fc = _controller(N, B)
    fc.set_paths([road])
    try:
        assert (fc.lane_idx.cpu().numpy() == -1).all() and str(fc.lane_idx.dtype) == "torch.int32"
        got = _step_route(fc, zero, _along(road, at, seed=7))
        assert np.array_equal(got["lane_idx"], at)
        mask = np.arange(B) % 2 == 0
        fc.reset(mask)
        after = _state(fc)
        assert (after["lane_idx"][mask] == -1).all() and np.array_equal(after["lane_idx"][~mask], at[~mask])
        assert (after["safe_count"][mask] == 0).all() and (after["safe_count"][~mask] == 1).all()
        far = _along(road, at + 200, seed=8)                                   # 200 waypoints on: outside every window
        got = _step_route(fc, zero, far)
        want = [LS.nearest(route[1], route[2], far[0, b], far[1, b], -1 if mask[b] else at[b], 8, 64) for b in range(B)]
        assert got["lane_idx"].tolist() == want
        assert np.array_equal(got["lane_idx"][mask], at[mask] + 200) and np.array_equal(got["lane_idx"][~mask], at[~mask] + 64)
        fc.reset()
        assert (fc.lane_idx.cpu().numpy() == -1).all()
    finally:
        fc.close()


def test_argument_errors():
    import torch
    from ad_mpc_amd.config import AdmpcLaneParams
    from ad_mpc_amd.fleet import FleetLaneStep, FleetPathStep
    N, B = 20, 6
    fc = _controller(N, B)
    z = [torch.zeros(B, dtype=torch.float64, device=fc.device) for _ in range(7)]
    tk = torch.zeros(B, dtype=torch.int32, device=fc.device)
    L = fc.lib
    try:
        with pytest.raises(ValueError, match="set_paths"):
            fc.step_route(tk, *z)
        fc.set_paths([_road(M=100)])
        with pytest.raises(ValueError, match="step_paths"):
            fc.best_of(3)
        for kw in (dict(lane=33), dict(lane=257), dict(back=-1), dict(ahead=-1)):
            with pytest.raises(ValueError, match="lane must be"):
                fc.step_route(tk, *z, **kw)
        with pytest.raises(ValueError, match="int32"):
            fc.step_route(tk.to(torch.int64), *z)
        with pytest.raises(ValueError, match="shape"):
            fc.step_route(tk, *z[:6], z[6][:5].contiguous())
        torch.cuda.synchronize()
        assert (fc.lane_idx.cpu().numpy() == -1).all()                          # no refused call reached the device
        r = fc.step_route(tk, *z, lane=34, back=0, ahead=0)
        assert isinstance(r, FleetLaneStep) and r._fields == FleetPathStep._fields + ("lane_idx",) and r.lane_idx is fc.lane_idx
        val, idx = fc.best_of(2)
        assert val.shape == (3,)
        torch.cuda.synchronize()
        assert (fc.lane_idx.cpu().numpy() == 0).all()

        # the C ABI behind a real bank and solver: the bank step's refusals, behind those of the lane
        ok = AdmpcLaneParams(L=64, back=8, ahead=64)

        def call(**over):
            a = dict(s=fc._eng._h, bank=fc._bank, lane=C.byref(ok), prm=C.byref(fc._prm), B=B, tk=_p(tk), idx=_p(fc.lane_idx), ins=[_p(t) for t in z],
                     work=_p(fc._work))
            a.update(over)
            return L.admpc_control_step_lane_batch(a["s"], a["bank"], a["lane"], a["prm"], a["B"], a["tk"], a["idx"], *a["ins"], _p(fc.x_opt),
                                                   _p(fc.w_opt), _p(fc.safe_count), _p(fc.prev_u), _p(fc.has_valid), a["work"], _p(fc.ack),
                                                   _p(fc.mode), _p(fc.valid), _p(fc.status), _p(fc.cost), fc._eng._stream())

        def refused(rc, words):
            assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

        before = _state(fc)
        refused(call(lane=None), "lane parameters")
        refused(call(lane=C.byref(AdmpcLaneParams(L=300, back=8, ahead=64))), "[34, 256]")
        refused(call(idx=C.c_void_p(0)), "null lane_idx")
        refused(call(bank=None), "bank is not set")
        refused(call(s=None), "null solver / params")
        refused(call(prm=None), "null solver / params")
        refused(call(B=-1), "negative batch")
        refused(call(tk=C.c_void_p(0)), "null array")
        refused(call(work=C.c_void_p(0)), "null array")
        other = _controller(40, B)
        refused(call(s=other._eng._h), "H must equal")
        other.close()
        refused(L.admpc_waypoints_lane_batch(fc._bank, C.byref(ok), B, None, _p(fc.lane_idx), *[_p(t) for t in z[:5]], 1, 3.0, 0.05, _p(fc._work), _p(fc._work),
                                             _p(tk), None), "null array")
        refused(L.admpc_waypoints_lane_batch(fc._bank, C.byref(ok), -1, _p(tk), _p(fc.lane_idx), *[_p(t) for t in z[:5]], 1, 3.0, 0.05, _p(fc._work),
                                             _p(fc._work), _p(tk), None), "negative batch")
        assert call(B=0) == 0
        after = _state(fc)
        for k in STATE:
            _bits(after[k], before[k], "%s after refused calls" % k)
        assert call() == 0
        torch.cuda.synchronize()
    finally:
        fc.close()
