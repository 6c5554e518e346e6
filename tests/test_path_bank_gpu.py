"""A path per vehicle and the best of C candidate paths (include/admpc_fleet.h; ad_mpc_amd/fleet.py: set_paths, step_paths, best_of).

Almost every statement reads "bit-identical to what the single-path code gives for the same vehicle": the waypoints against
admpc_waypoints_batch with the vehicle's path alone, the step against a single-path FleetController fed the same poses in the same
slots, the cost against admpc_solve_batch on the inputs the step assembled, the arg-min per group against admpc_argmin called per
group and against the numpy restatement of the rule (path_bank.group_argmin, itself held to tests/argmin_spec.py on the CPU)."""
import ctypes as C

import numpy as np
import pytest

import batch_regimes as R
import path_bank as PB
from test_fleet_step import T_HORIZON, OPT_DT, _path, _poses, _wrap
from test_fleet_step_edges import _path_east, _poses_east

pytestmark = pytest.mark.gpu

STATE = ("ack", "mode", "status", "valid", "x_opt", "w_opt", "safe_count", "prev_u", "has_valid")


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _lib():
    from ad_mpc_amd import _lib
    return _lib.load()


# ---- 1. waypoints against the bank -----------------------------------------------------------------------------------------------

def _columns(M, seed):
    """The seven columns of a path of M waypoints, straight from numpy (RefTrajectory.set_traj smooths the curvature with a filter that
    needs more than 33 waypoints; the generator itself takes M >= 2).  Waypoints 1 m apart in x at y = seed, so that a pose at
    x = m + 0.5 is equidistant from waypoints m and m + 1."""
    m = np.arange(M, dtype=np.float64)
    x, y = m.copy(), np.full(M, float(seed))
    psi = _wrap(0.05 * m + 3.0)                                           # crosses +-pi: the unwrap runs
    seg = np.sqrt(np.diff(x) ** 2 + np.diff(y) ** 2)
    cdist = np.concatenate(([0.0], np.cumsum(seg)))
    return [6.0 + np.cos(m / 5.0 + seed), x, y, psi, np.unwrap(psi), cdist, 0.01 * np.sin(m / 3.0)]


BANK_M = (2, 7, 65, 400)


def _make_bank(cols_per_path, H, dt):
    """(bank handle, the device columns per path).  The caller destroys the bank."""
    from ad_mpc_amd.config import AdmpcPath
    L = _lib()
    dev = [[_dev(c) for c in cols] for cols in cols_per_path]
    descs = (AdmpcPath * len(dev))()
    for d, cols in zip(descs, dev):
        d.M, d.H, d.dt = int(cols[0].shape[0]), H, dt
        d.vel, d.x, d.y, d.psi, d.psi_unwrapped, d.cdist, d.curv = [c.data_ptr() for c in cols]
    import torch
    torch.cuda.synchronize()
    bank = C.c_void_p(0)
    rc = L.admpc_path_bank_create(0, len(dev), descs, C.byref(bank))
    assert rc == 0, L.admpc_last_error()
    return bank, dev


def _waypoint_poses(B, path_of, seed):
    rng = np.random.default_rng(seed)
    M = np.array(BANK_M)[path_of]
    X = rng.uniform(-1.0, 1.0, size=B) + rng.integers(0, 70, size=B) % M
    Y = path_of + rng.uniform(-1.5, 1.5, size=B)
    P = rng.uniform(-3.5, 3.5, size=B)
    return X, Y, P


def _check_waypoints(H, B, path_of, X, Y, P):
    import torch
    L = _lib()
    dt = T_HORIZON / H
    bank, dev = _make_bank([_columns(M, k) for k, M in enumerate(BANK_M)], H, dt)
    try:
        tX, tY, tP, tk = _dev(X), _dev(Y), _dev(P), _dev(path_of, torch.int32)
        ref = torch.full((B, 6, H), 7.0, dtype=torch.float64, device="cuda:0")
        err = torch.full((B, 3), 7.0, dtype=torch.float64, device="cuda:0")
        stop = torch.full((B,), 7, dtype=torch.int32, device="cuda:0")
        assert L.admpc_waypoints_bank_batch(bank, B, _p(tk), _p(tX), _p(tY), _p(tP), _p(ref), _p(err), _p(stop), None) == 0, L.admpc_last_error()
        torch.cuda.synchronize()
        ref, err, stop = ref.cpu().numpy(), err.cpu().numpy(), stop.cpu().numpy()
        for k, M in enumerate(BANK_M):
            sel = np.nonzero(path_of == k)[0]
            assert len(sel) > 0
            n = len(sel)
            r1 = torch.empty((n, 6, H), dtype=torch.float64, device="cuda:0")
            e1 = torch.empty((n, 3), dtype=torch.float64, device="cuda:0")
            s1 = torch.empty(n, dtype=torch.int32, device="cuda:0")
            pose = [_dev(a[sel]) for a in (X, Y, P)]
            assert L.admpc_waypoints_batch(0, M, H, dt, n, *[_p(c) for c in dev[k]], *[_p(a) for a in pose], _p(r1), _p(e1), _p(s1), None) == 0, \
                L.admpc_last_error()
            torch.cuda.synchronize()
            _bits(ref[sel], r1.cpu().numpy(), "out_ref of the vehicles on path %d (M = %d)" % (k, M))
            _bits(err[sel], e1.cpu().numpy(), "out_err of the vehicles on path %d" % k)
            _bits(stop[sel], s1.cpu().numpy(), "out_stop of the vehicles on path %d" % k)
        return ref, err, stop
    finally:
        L.admpc_path_bank_destroy(bank)


@pytest.mark.parametrize("H", [3, 20, 64])
def test_waypoints_of_a_bank_equal_the_single_path_kernel(H):
    """K = 4 paths of M = 2 (the minimum), 7 (M < H at H = 20 and 64: the first H speeds are padded with 0.01), 65 (one past the stride
    of the nearest-point scan) and 400; 37 poses with mixed path_of, among them poses equidistant from two waypoints (the first index
    wins), one non-finite pose (index 0) and two indices outside the bank (NaN rows, stop 0, nothing else touched)."""
    B = 37
    path_of = (np.arange(B) * 7 % 4).astype(np.int32)
    X, Y, P = _waypoint_poses(B, path_of, seed=H)
    assert path_of[[4, 7, 11, 6, 10, 5]].tolist() == [0, 1, 1, 2, 2, 3]
    for b, m in ((4, 0), (7, 3), (11, 5), (6, 30), (10, 63), (5, 200)):        # on the path's line, half way between waypoints m and m + 1;
        X[b], Y[b] = m + 0.5, float(path_of[b])                                 # 63 / 64: the two belong to different passes of the scan
    X[20], Y[21], P[22] = np.nan, np.inf, np.nan
    bad = [13, 29]
    full = path_of.copy()
    ref, err, stop = _check_waypoints(H, B, path_of, X, Y, P)
    assert np.isfinite(ref[[4, 5, 6, 7, 10, 11]]).all() and not np.isfinite(ref[20]).all()
    # indices outside the bank: the same call once more with two of them; those rows are NaN / 0, every other row keeps its bits
    import torch
    L = _lib()
    full[bad[0]], full[bad[1]] = -1, len(BANK_M)
    bank, dev = _make_bank([_columns(M, k) for k, M in enumerate(BANK_M)], H, T_HORIZON / H)
    try:
        r2 = torch.full((B, 6, H), 7.0, dtype=torch.float64, device="cuda:0")
        e2 = torch.full((B, 3), 7.0, dtype=torch.float64, device="cuda:0")
        s2 = torch.full((B,), 7, dtype=torch.int32, device="cuda:0")
        ins = [_dev(full, torch.int32), _dev(X), _dev(Y), _dev(P)]
        assert L.admpc_waypoints_bank_batch(bank, B, *[_p(a) for a in ins], _p(r2), _p(e2), _p(s2), None) == 0
        torch.cuda.synchronize()
    finally:
        L.admpc_path_bank_destroy(bank)
    r2, e2, s2 = r2.cpu().numpy(), e2.cpu().numpy(), s2.cpu().numpy()
    keep = np.ones(B, dtype=bool); keep[bad] = False
    assert np.isnan(r2[bad]).all() and np.isnan(e2[bad]).all() and (s2[bad] == 0).all()
    _bits(r2[keep], ref[keep], "out_ref next to an invalid index"); _bits(e2[keep], err[keep], "out_err"); _bits(s2[keep], stop[keep], "out_stop")


def test_waypoints_of_a_bank_past_the_grid():
    """B above the 4096 workgroups of the launch: vehicle b and b + 4096 share a workgroup, each with its own path."""
    B = R.WAYPOINTS_PAST
    assert R.waypoints_grid(B) < B
    path_of = (np.arange(B) * 5 % 4).astype(np.int32)
    path_of[4096:] = (path_of[4096:] + 1) % 4                                  # the two vehicles of a workgroup are on different paths
    X, Y, P = _waypoint_poses(B, path_of, seed=1)
    _check_waypoints(20, B, path_of, X, Y, P)


# ---- 2. the step against the bank ------------------------------------------------------------------------------------------------

def _controller(N, B, **kw):
    from ad_mpc_amd.fleet import FleetController
    return FleetController(T_HORIZON, N, OPT_DT, B, **kw)


def _state(fc):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(fc, k).cpu().numpy().copy() for k in STATE + ("cost",)}


def _step_paths(fc, path_of, pose):
    import torch
    fc.step_paths(_dev(path_of, torch.int32), *[_dev(a) for a in pose])
    return _state(fc)


def _step(fc, pose):
    fc.step(*[_dev(a) for a in pose])
    return _state(fc)


def _lane(path, off):
    """The path moved `off` m to its left."""
    x, y, psi, v = path
    return x - off * np.sin(psi), y + off * np.cos(psi), psi, v


@pytest.mark.parametrize("N", [20, 40])
def test_a_bank_of_one_path_is_the_old_step(N):
    B, T = 32, 3
    path = _path_east()
    poses = _poses_east(B, T, seed=41, leave=(1, 2))                         # valid predictions at step 0, invalid ones after them at step 1
    old, new = _controller(N, B), _controller(N, B)
    old.set_traj(*path); new.set_paths([path])
    zero = np.zeros(B, dtype=np.int32)
    seen_valid = 0
    for t in range(T):
        a, b = _step(old, poses[t]), _step_paths(new, zero, poses[t])
        for k in STATE:
            _bits(a[k], b[k], "%s at step %d" % (k, t))
        seen_valid += int(a["valid"].sum())
    assert 0 < seen_valid < B * T and a["has_valid"].any()
    old.close(); new.close()


@pytest.mark.parametrize("N", [20, 40])
def test_three_paths_mixed_equal_three_single_path_fleets(N):
    """B = 48 on K = 3 paths (towards -x, towards +x, and a lane 1.5 m to the left of the latter), three steps.  The vehicles with
    path_of == k are bit-identical to a single-path fleet of the same B on path k fed the same poses in the same slots; cost[b] is the cost
    admpc_solve_batch returns for the inputs the step assembled for b, and +inf exactly where status != 0 or valid == 0."""
    import torch
    B, T = 48, 3
    paths = [_path(), _path_east(), _lane(_path_east(), 1.5)]
    path_of = (np.arange(B) * 5 % 3).astype(np.int32)
    west, east = _poses(B, T, seed=42, leave=(1, 2)), _poses_east(B, T, seed=43, leave=(1, 2))
    poses = np.where((path_of == 0)[None, None, :], west, east)
    poses[2, 0, 17] = np.nan                                                    # a failed solve at the last step
    mixed, single = _controller(N, B), [_controller(N, B) for _ in paths]
    aux = _controller(N, B)                                                     # a second handle for the bare solves
    mixed.set_paths(paths)
    for fc, p in zip(single, paths):
        fc.set_traj(*p)
    masked = finite = 0
    for t in range(T):
        xb, ub = mixed.x_opt.clone(), mixed.w_opt.clone()                       # the iterate the step starts from
        got = _step_paths(mixed, path_of, poses[t])
        for k, fc in enumerate(single):
            ref = _step(fc, poses[t])
            sel = path_of == k
            for key in STATE:
                _bits(got[key][sel], ref[key][sel], "%s of the vehicles on path %d at step %d" % (key, k, t))
        x0, yref, yref_e, p = [v.clone() for v in PB.step_work_views(mixed._work, B, N)]
        cost = torch.empty(B, dtype=torch.float64, device=mixed.device)
        st = torch.empty(B, dtype=torch.int32, device=mixed.device)
        aux._eng.solve(x0, yref, yref_e, p, xb, ub, cost, st, None)
        torch.cuda.synchronize()
        cost, st = cost.cpu().numpy(), st.cpu().numpy()
        _bits(st, got["status"], "status of the bare solve at step %d" % t)
        _bits(xb.cpu().numpy(), got["x_opt"], "x_opt of the bare solve at step %d" % t)
        out = (got["status"] != 0) | (got["valid"] == 0)
        assert np.isposinf(got["cost"][out]).all(), "cost where status != 0 or valid == 0, step %d" % t
        _bits(got["cost"][~out], cost[~out], "cost of the usable vehicles at step %d" % t)
        assert np.isfinite(cost[(got["status"] == 0)]).all()
        masked += int(((got["status"] == 0) & (got["valid"] == 0)).sum()); finite += int((~out).sum())
    assert got["status"][17] == 4 and np.isposinf(got["cost"][17])
    assert masked > 0 and finite > 0, (masked, finite)                         # both sides of the mask occurred
    for fc in [mixed, aux] + single:
        fc.close()


@pytest.mark.parametrize("N", [20, 40])
def test_an_invalid_path_index_fails_its_vehicle_alone(N):
    """path_of = -1 and = K on two vehicles of 16, after two healthy steps: those two end the step as a vehicle whose solve failed, the other
    14 as in the same run without the invalid entries."""
    B, T, bad = 16, 3, [2, 9]
    paths = [_path_east(), _lane(_path_east(), 1.5)]
    path_of = (np.arange(B) % 2).astype(np.int32)
    poses = _poses_east(B, T, seed=44)
    fa, fb = _controller(N, B), _controller(N, B)
    fa.set_paths(paths); fb.set_paths(paths)
    for t in range(2):
        a, b = _step_paths(fa, path_of, poses[t]), _step_paths(fb, path_of, poses[t])
    assert (b["status"][bad] == 0).all() and b["safe_count"][bad].tolist() == [2, 2]          # healthy so far
    assert np.abs(b["x_opt"][bad]).max() > 0
    broken = path_of.copy(); broken[bad[0]], broken[bad[1]] = -1, len(paths)
    a, c = _step_paths(fa, path_of, poses[2]), _step_paths(fb, broken, poses[2])
    assert c["status"][bad].tolist() == [4, 4] and c["mode"][bad].tolist() == [0, 0] and c["valid"][bad].tolist() == [0, 0]
    assert np.isposinf(c["cost"][bad]).all() and c["safe_count"][bad].tolist() == [0, 0]
    for k in ("x_opt", "w_opt", "prev_u", "has_valid"):
        _bits(c[k][bad], b[k][bad], "%s of the vehicles with an invalid index" % k)
    steer = poses[2][6][bad].astype(np.float32)
    _bits(c["ack"][bad], np.stack([steer, np.zeros(2, np.float32), np.zeros(2, np.float32), np.full(2, np.float32(-1e5))], axis=1), "brake record")
    keep = np.ones(B, dtype=bool); keep[bad] = False
    for k in STATE + ("cost",):
        _bits(c[k][keep], a[k][keep], "%s of the other vehicles" % k)
    fa.close(); fb.close()


@pytest.mark.parametrize("N", [20, 40])
def test_captured_step_paths_and_best_of_replay_bit_identical(N):
    import torch
    V, Cn, T = 16, 3, 3
    B = V * Cn
    paths = [_path_east(), _lane(_path_east(), 1.5), _lane(_path_east(), -1.0)]
    path_of = np.tile(np.arange(Cn, dtype=np.int32), V)
    poses = np.repeat(_poses_east(V, T, seed=45), Cn, axis=2)
    eager, graphed = _controller(N, B), _controller(N, B)
    eager.set_paths(paths); graphed.set_paths(paths)
    ref = []
    for t in range(T):
        r = _step_paths(eager, path_of, poses[t])
        val, idx = eager.best_of(Cn)
        torch.cuda.synchronize()
        r["val"], r["idx"] = val.cpu().numpy().copy(), idx.cpu().numpy().copy()
        ref.append(r)
    dev = graphed.device
    ins = [torch.zeros(B, dtype=torch.float64, device=dev) for _ in range(7)]
    tk = _dev(path_of, torch.int32)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        graphed.step_paths(tk, *ins)
        val, idx = graphed.best_of(Cn)
    for t in range(T):
        for i in range(7):
            ins[i].copy_(torch.as_tensor(poses[t][i], device=dev))
        g.replay()
        got = _state(graphed)
        got["val"], got["idx"] = val.cpu().numpy(), idx.cpu().numpy()
        for k in got:
            _bits(got[k], ref[t][k], "%s at replay %d" % (k, t))
    eager.close(); graphed.close()


# ---- 3. the arg-min per group ----------------------------------------------------------------------------------------------------

def _group_costs(G, group, seed):
    """Costs drawn from a few values, so that ties are everywhere: +inf, NaN, -0.0 / 0.0 among them; one all-NaN and one all-+inf group."""
    rng = np.random.default_rng(seed)
    pool = np.array([1.0, 1.0, 2.5, -0.0, 0.0, np.inf, np.nan, -3.5, 1e300, 7.0])
    c = pool[rng.integers(0, len(pool), size=(G, group))]
    c[rng.random(size=G) < 0.3] += 10.0                                          # groups without the common minimum
    if G >= 5:
        c[1], c[G - 1] = np.nan, np.inf
        c[2, :] = 0.0; c[2, group // 2:] = -0.0                                   # 0.0 in front of -0.0: the first wins with its own bits
        c[3, :] = -0.0; c[3, group // 2:] = 0.0
    return c.reshape(-1)


def _argmin_groups(eng, cost, G, group):
    import torch
    L = eng.lib
    val = torch.full((max(G, 1),), 7.0, dtype=torch.float64, device=eng.device)
    idx = torch.full((max(G, 1),), 7, dtype=torch.int64, device=eng.device)
    rc = L.admpc_argmin_groups(eng._h, _p(cost), G, group, _p(val), _p(idx), None)
    torch.cuda.synchronize()
    return rc, val.cpu().numpy()[:G], idx.cpu().numpy()[:G]


@pytest.fixture(scope="module")
def engine():
    from ad_mpc_amd.config import default_config
    from ad_mpc_amd.engine import BatchSolver
    eng = BatchSolver(default_config(N=20), device=0)
    yield eng
    eng.close()


@pytest.mark.parametrize("group", [1, 3, 16, 17, 64, 65, 200])
def test_argmin_groups_against_the_rule_and_against_admpc_argmin(engine, group):
    """Group sizes on both sides of the packing switch (16 / 17) and of a wave (64 / 65), below it and well above; G = 1, 5 and one value past
    the largest grid.  val and idx are bit-identical to the numpy restatement for every group and to admpc_argmin called on the group with
    the group's offset (every group for the small G, 64 groups around the grid's edge for the large one)."""
    import torch
    for G in (1, 5, PB.groups_past(group)):
        variants = [_group_costs(G, group, seed=G + group)]
        if G == 1:
            variants += [np.full(group, np.nan), np.full(group, np.inf)]
        for c in variants:
            cost = _dev(c)
            rc, val, idx = _argmin_groups(engine, cost, G, group)
            assert rc == 0, engine.lib.admpc_last_error()
            ev, ei = PB.group_argmin(c, group)
            _bits(val, ev, "val, G = %d" % G); _bits(idx, ei, "idx, G = %d" % G)
            assert ((idx // group) == np.arange(G)).all()
            per = PB.groups_per_round(group)
            pick = range(G) if G <= 5 else sorted({0, 1, 2, 3, G - 2, G - 1} | set(range(per - 29, per + 29)))
            one_v = torch.empty(len(pick), dtype=torch.float64, device=engine.device)
            one_i = torch.empty(len(pick), dtype=torch.int64, device=engine.device)
            for j, g in enumerate(pick):
                assert engine.lib.admpc_argmin(engine._h, C.c_void_p(cost.data_ptr() + 8 * g * group), group, g * group,
                                               C.c_void_p(one_v.data_ptr() + 8 * j), C.c_void_p(one_i.data_ptr() + 8 * j), None) == 0
            torch.cuda.synchronize()
            _bits(val[list(pick)], one_v.cpu().numpy(), "val against admpc_argmin, G = %d" % G)
            _bits(idx[list(pick)], one_i.cpu().numpy(), "idx against admpc_argmin, G = %d" % G)


# ---- 4. end to end: V vehicles x C candidate paths ---------------------------------------------------------------------------------

def test_best_of_three_candidate_paths_end_to_end():
    """V = 8 vehicles x C = 3 candidates at N = 20, instance b = v * C + c.  Candidates 0 and 1 are two lanes of one road, candidate 2 lies
    60 m away, where is_valid_command fails.  idx[v] is the numpy arg-min of the masked costs of group v; candidate 2 never wins; and in
    the first steps, where safe_count < 10 and so mode is 0 everywhere, every vehicle has a finite winner -- the reason why the mask
    uses status and valid, not mode."""
    import torch
    N, V, Cn, T = 20, 8, 3, 3
    B = V * Cn
    road = _path_east()
    paths = [road, _lane(road, 1.5), _lane(road, 60.0)]
    rng = np.random.default_rng(46)
    pose = np.zeros((7, V))
    s, e = rng.uniform(0.5, 2.0, size=V), np.linspace(-0.4, 1.9, V)                   # between and beside the two lanes
    h = np.arctan2(3.0 / 40.0 * np.cos(s / 40.0), 1.0)
    pose[0], pose[1] = s - e * np.sin(h), 3.0 * np.sin(s / 40.0) + e * np.cos(h)
    pose[2], pose[3] = h + rng.uniform(-0.03, 0.03, size=V), rng.uniform(6.0, 9.0, size=V)
    path_of = np.tile(np.arange(Cn, dtype=np.int32), V)
    fc = _controller(N, B)
    fc.set_paths(paths)
    winners = set()
    for t in range(T):
        pose[0] += 0.08 * np.cos(h); pose[1] += 0.08 * np.sin(h)
        got = _step_paths(fc, path_of, np.repeat(pose, Cn, axis=1))
        val, idx = fc.best_of(Cn)
        torch.cuda.synchronize()
        val, idx = val.cpu().numpy(), idx.cpu().numpy()
        assert (got["mode"] == 0).all() and (got["safe_count"] <= t + 1).all()          # the warm-up of the gate
        assert (got["status"].reshape(V, Cn)[:, :2] == 0).all()
        cost = got["cost"].reshape(V, Cn)
        assert np.isposinf(cost[:, 2]).all() and (got["valid"].reshape(V, Cn)[:, 2] == 0).all()
        masked = np.where((got["status"] != 0) | (got["valid"] == 0), np.inf, got["cost"]).reshape(V, Cn)
        _bits(masked, cost, "the step's mask at step %d" % t)
        np.testing.assert_array_equal(idx, np.arange(V) * Cn + np.argmin(masked, axis=1))
        _bits(val, masked[np.arange(V), np.argmin(masked, axis=1)], "val at step %d" % t)
        assert np.isfinite(val).all(), "a vehicle without a finite winner at step %d: %s" % (t, val)
        assert (idx % Cn != 2).all()
        winners |= set((idx % Cn).tolist())
    assert winners == {0, 1}, winners                                                  # both lanes win for some vehicle
    with pytest.raises(ValueError, match="multiple"):
        fc.best_of(5)
    fc.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_of_the_c_abi_leave_the_outputs_untouched():
    import torch
    from ad_mpc_amd.config import AdmpcPath
    L = _lib()
    dt = T_HORIZON / 20
    cols = [[_dev(c) for c in _columns(M, k)] for k, M in enumerate((40, 50))]

    def descs(**over):
        d = (AdmpcPath * 2)()
        for k in range(2):
            d[k].M, d[k].H, d[k].dt = int(cols[k][0].shape[0]), 20, dt
            d[k].vel, d[k].x, d[k].y, d[k].psi, d[k].psi_unwrapped, d[k].cdist, d[k].curv = [c.data_ptr() for c in cols[k]]
        for name, v in over.items():
            setattr(d[1], name, v)
        return d

    def refused(rc, words, code=-1):
        assert rc == code, (rc, L.admpc_last_error())
        assert words in L.admpc_last_error().decode(), L.admpc_last_error()

    bank = C.c_void_p(0)
    refused(L.admpc_path_bank_create(0, 0, descs(), C.byref(bank)), "K >= 1")
    refused(L.admpc_path_bank_create(0, -3, descs(), C.byref(bank)), "K >= 1")
    refused(L.admpc_path_bank_create(0, 2, descs(M=1), C.byref(bank)), "M >= 2")
    for col in ("vel", "x", "y", "psi", "psi_unwrapped", "cdist", "curv"):
        refused(L.admpc_path_bank_create(0, 2, descs(**{col: None}), C.byref(bank)), "seven columns")
    refused(L.admpc_path_bank_create(0, 2, descs(H=21), C.byref(bank)), "differs from path 0")
    refused(L.admpc_path_bank_create(0, 2, descs(dt=dt * 2), C.byref(bank)), "differs from path 0")
    d = descs(); d[0].dt = d[1].dt = 0.0
    refused(L.admpc_path_bank_create(0, 2, d, C.byref(bank)), "dt > 0")
    d = descs(); d[0].dt = d[1].dt = -dt
    refused(L.admpc_path_bank_create(0, 2, d, C.byref(bank)), "dt > 0")
    refused(L.admpc_path_bank_create(0, 2, None, C.byref(bank)), "null")
    refused(L.admpc_path_bank_create(torch.cuda.device_count() + 3, 2, descs(), C.byref(bank)), "device", code=-2)
    refused(L.admpc_path_bank_create(-1, 2, descs(), C.byref(bank)), "device", code=-2)
    assert bank.value is None                                                    # no refused call wrote the handle
    assert L.admpc_path_bank_create(0, 2, descs(), C.byref(bank)) == 0 and bank.value
    b21 = C.c_void_p(0)
    d = descs(); d[0].H = d[1].H = 21
    assert L.admpc_path_bank_create(0, 2, d, C.byref(b21)) == 0

    # the step
    fc = _controller(20, 4)
    z = [torch.zeros(4, dtype=torch.float64, device=fc.device) for _ in range(7)]
    tk = torch.zeros(4, dtype=torch.int32, device=fc.device)
    outs = (fc.x_opt, fc.w_opt, fc.safe_count, fc.prev_u, fc.has_valid, fc.ack, fc.mode, fc.valid, fc.status, fc.cost)
    for o in outs:
        o.fill_(3)
    before = [o.cpu().numpy().copy() for o in outs]

    def call(h=None, **over):
        a = dict(s=(h or fc)._eng._h, bank=bank, prm=C.byref(fc._prm), B=4, tk=_p(tk), ins=[_p(t) for t in z], work=_p(fc._work), cost=_p(fc.cost))
        a.update(over)
        return L.admpc_control_step_bank_batch(a["s"], a["bank"], a["prm"], a["B"], a["tk"], *a["ins"], _p(fc.x_opt), _p(fc.w_opt), _p(fc.safe_count),
                                               _p(fc.prev_u), _p(fc.has_valid), a["work"], _p(fc.ack), _p(fc.mode), _p(fc.valid), _p(fc.status),
                                               a["cost"], fc._eng._stream())

    refused(call(bank=b21), "H must equal")
    refused(call(bank=None), "bank is not set")
    refused(call(prm=None), "null solver / params")
    refused(call(s=None), "null solver / params")
    refused(call(B=-1), "negative batch")
    refused(call(tk=C.c_void_p(0)), "null array")
    refused(call(ins=[_p(z[0])] * 6 + [C.c_void_p(0)]), "null array")
    refused(call(work=C.c_void_p(0)), "null array")
    long_h = _controller(80, 4)
    refused(call(h=long_h), "[3, 64]")
    refused(L.admpc_waypoints_bank_batch(None, 4, _p(tk), _p(z[0]), _p(z[1]), _p(z[2]), _p(fc._work), _p(fc._work), _p(tk), None), "null bank")
    refused(L.admpc_waypoints_bank_batch(bank, 4, None, _p(z[0]), _p(z[1]), _p(z[2]), _p(fc._work), _p(fc._work), _p(tk), None), "null array")
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        _bits(o.cpu().numpy(), b, "an output of a refused step")
    for o in outs:
        o.zero_()
    assert call(cost=C.c_void_p(0)) == 0                                         # cost may be NULL; the well-formed call goes through
    assert call() == 0
    torch.cuda.synchronize()

    # the arg-min per group
    cost = torch.zeros(12, dtype=torch.float64, device=fc.device)
    val = torch.full((4,), 7.0, dtype=torch.float64, device=fc.device)
    idx = torch.full((4,), 7, dtype=torch.int64, device=fc.device)
    h = fc._eng._h
    refused(L.admpc_argmin_groups(h, _p(cost), -1, 3, _p(val), _p(idx), None), "G >= 0")
    refused(L.admpc_argmin_groups(h, _p(cost), 4, 0, _p(val), _p(idx), None), "group >= 1")
    refused(L.admpc_argmin_groups(h, _p(cost), 4, 3, None, _p(idx), None), "null output")
    refused(L.admpc_argmin_groups(h, _p(cost), 4, 3, _p(val), None, None), "null output")
    refused(L.admpc_argmin_groups(h, None, 4, 3, _p(val), _p(idx), None), "null cost")
    refused(L.admpc_argmin_groups(None, _p(cost), 4, 3, _p(val), _p(idx), None), "solver")
    assert L.admpc_argmin_groups(h, _p(cost), 0, 3, _p(val), _p(idx), None) == 0        # G == 0: a no-op
    torch.cuda.synchronize()
    assert (val.cpu().numpy() == 7.0).all() and (idx.cpu().numpy() == 7).all()
    L.admpc_path_bank_destroy(bank); L.admpc_path_bank_destroy(b21)
    fc.close(); long_h.close()


def test_refusals_of_the_host_mirror():
    import torch
    fc = _controller(20, 6)
    z = [torch.zeros(6, dtype=torch.float64, device=fc.device) for _ in range(7)]
    tk = torch.zeros(6, dtype=torch.int32, device=fc.device)
    with pytest.raises(ValueError, match="set_paths"):
        fc.step_paths(tk, *z)
    with pytest.raises(ValueError):
        fc.set_paths([])
    fc.set_paths([_path_east()])
    with pytest.raises(ValueError, match="step_paths"):
        fc.best_of(3)                                                            # nothing to reduce yet
    with pytest.raises(ValueError, match="int32"):
        fc.step_paths(tk.to(torch.int64), *z)
    with pytest.raises(ValueError, match="shape"):
        fc.step_paths(tk[:5].contiguous(), *z)
    with pytest.raises(ValueError, match="shape"):
        fc.step_paths(tk.view(6, 1), *z)
    r = fc.step_paths(tk, *z)
    assert r._fields == ("ack", "mode", "status", "valid", "x_opt", "w_opt", "cost") and r.cost.shape == (6,)
    from ad_mpc_amd.fleet import FleetStep
    assert FleetStep._fields == r._fields[:-1]
    for g in (4, 5, 0, -2):
        with pytest.raises(ValueError, match="multiple"):
            fc.best_of(g)
    val, idx = fc.best_of(2)
    assert val.shape == (3,) and idx.dtype == torch.int64
    torch.cuda.synchronize()
    fc.close()
    assert fc._bank is None                                                      # close() destroyed the bank
