"""The edges of the fleet's control step (admpc_control_step_batch, ad_mpc_amd/csrc/admpc_step.hip): every kind of horizon in [3, 64],
verdicts on both sides of every threshold of the distance test, the parameters of the step, and a fleet past the command kernel's grid.

Oracle and comparison are those of test_fleet_step.py: one independent host pipeline per vehicle (_HostFleet) that solves through
admpc_solve_batch at B = 1, integers equal, the Ackermann record bit-equal as float32, x_opt / w_opt within 1e-12 (_compare).  Every
"the sequence contains ..." condition below is asserted on the HOST oracle's results."""
import math

import numpy as np
import pytest

import batch_regimes as R
from test_fleet_step import _path, _poses, _on_path, _wrap, _HostFleet, _fleet, _compare, _dev_step

pytestmark = pytest.mark.gpu

KEYS = ("status", "mode", "valid", "safe", "ack", "x", "u")


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _run(fc, host, poses):
    """Every step of `poses` through the fleet and the host pipelines, compared; the host's results per step."""
    out = []
    for t in range(poses.shape[0]):
        ref = host.step(poses[t])
        _compare(t, _dev_step(fc, poses[t]), ref)
        out.append(ref)
    return out


def _path_east(M=400, ds=0.5):
    """_path() mirrored: towards +x.  A fresh controller's iterate is all zeros, a vehicle at rest with yaw 0, so only with a heading near 0
    is the very first prediction close to the window; on _path(), heading near +-pi, no vehicle has a valid prediction at step 0."""
    s = np.arange(M) * ds
    return s, 3.0 * np.sin(s / 40.0), np.arctan2(3.0 / 40.0 * np.cos(s / 40.0), np.ones(M)), 8.0 + 2.0 * np.sin(s / 25.0)


def _poses_east(B, T, **kw):
    """The poses of _poses, mirrored with the path."""
    poses = _poses(B, T, **kw)
    poses[:, 0] *= -1.0; poses[:, 2] = _wrap(np.pi - poses[:, 2])
    return poses


# ---- 1. the horizons

@pytest.mark.parametrize("N", [3, 4, 13, 33, 60, 63, 64])
def test_horizon_sweep(N, monkeypatch):
    """N = 3 (two input-reference rows, the least room for pad_reference and the fallback w[0:2] = prev[2:4]), 4, 13, 33 and 63 run kernel R,
    60 kernel S with three waves, 64 has N + 1 = 65 slots on the command kernel's 64 lanes (the trailing zero of path_close beyond the wave)."""
    B, T = 32, 12
    path = _path()
    poses = _poses(B, T, leave=(6, 9))                     # vehicles 5, 13, 21, 29 leave the path at steps 6 .. 8, after valid steps
    host = _HostFleet(N, B, path, threshold=3)
    res = _run(_fleet(N, B, path, threshold=3), host, poses)
    p = np.array([r["p"] for r in res])
    assert any((r["mode"] == 1).any() for r in res) and any((r["valid"] == 0).any() for r in res)
    assert host.fallbacks > 0 and ((p > 0) & (p < 1)).any()
    if N == 60:
        # the default kernel of this horizon is the segmented one (as test_seg_gpu.py:test_default_kernel_by_horizon finds it out: the bits
        # of the two kernels differ), so that this case cannot become another case of kernel R unnoticed
        got = {}
        for qp in (None, "seg", "riccati"):
            monkeypatch.delenv("ADMPC_QP", raising=False)
            if qp:
                monkeypatch.setenv("ADMPC_QP", qp)
            got[qp] = _dev_step(_fleet(N, B, path), poses[0])
        monkeypatch.delenv("ADMPC_QP", raising=False)
        _bits(got[None]["x"], got["seg"]["x"], "default kernel at N = 60: x_opt"); _bits(got[None]["u"], got["seg"]["u"], "default kernel at N = 60: w_opt")
        assert (got["seg"]["u"] != got["riccati"]["u"]).any()


# ---- 2. verdicts on both sides of every threshold

V_PATH = 8.0            # the speed of _path() at its start: the window's slot h lies V_PATH * (h + 1) / N m along the path


def _pose(s, e, dyaw, vx):
    px, py, h = _on_path(s, e)
    return (px, py, float(_wrap(h + dyaw)), vx, 0.0, 0.0, 0.0)


def verdict_poses(N, lateral, heading, lag):
    """[7][B] (constant over the steps).  Three groups along _path(), each vehicle level with the window's first slot at the path's speed:
    lateral   a uniform offset e [m] across the path: every distance about e (mean = 3, max = 4)
    heading   on the path with a heading error [rad]: the distance grows along the horizon, the last slot (which `valid` counts and
              `healthy` does not) is the largest
    lag       on the path, L [m] behind the window: the window's first slots lead from the vehicle's own position to the path
              (ref_traj.py:160-161), the far corner is where it gets there, and the vehicle never catches up"""
    s0 = V_PATH / N
    rows = [_pose(s0, e, 0.0, V_PATH) for e in lateral] + [_pose(s0, 0.0, a, V_PATH) for a in heading] + [_pose(s0 - L, 0.0, 0.0, V_PATH) for L in lag]
    return np.array(rows).T


def distance_stats(x_opt, rx, ry, n):
    """mean, unbiased variance and max of the n slots of the distance test (the last one 0), in exact summation; rx, ry: the node's window."""
    d = [math.hypot(rx[i] - x_opt[i, 0], ry[i] - x_opt[i, 1]) for i in range(n - 1)] + [0.0]
    mean = math.fsum(d) / n
    return mean, math.fsum((v - mean) ** 2 for v in d) / (n - 1), max(d)


# chosen, with the CPU oracle's solve in place of the device's, so that the host oracle meets the conditions asserted below: at step 1 the last slot of the heading group passes 4 m near 0.59 rad
# at N = 20 and near 0.48 rad at N = 64, where two neighbouring slots are 0.07 m apart (hence the narrow sweep there)
VERDICT_SWEEPS = {
    20: dict(lateral=np.linspace(2.0, 4.5, 22), heading=np.linspace(0.50, 0.70, 21), lag=np.linspace(3.0, 5.0, 21)),
    64: dict(lateral=np.linspace(2.0, 4.5, 22), heading=np.linspace(0.455, 0.505, 21), lag=np.linspace(3.0, 5.0, 21)),
}


@pytest.mark.parametrize("N", [20, 64])
def test_verdicts_on_both_sides_of_the_thresholds(N):
    """64 vehicles whose distances to the window sweep across mean = 3 and max = 4, over the N + 1 slots of `valid` and the N slots of
    `healthy` (and so `mode`: threshold = 1, every step with status 0 and a healthy prediction commands)."""
    B, T = 64, 3
    path = _path()
    pose = verdict_poses(N, **VERDICT_SWEEPS[N])
    assert pose.shape == (7, B)
    res = _run(_fleet(N, B, path, threshold=1), _HostFleet(N, B, path, threshold=1), np.repeat(pose[None], T, axis=0))
    valid, healthy = np.array([r["valid"] for r in res]), np.array([r["healthy"] for r in res])
    assert (valid == 1).any() and (valid == 0).any(), "valid: one verdict only"
    assert (healthy == 1).any() and (healthy == 0).any(), "healthy: one verdict only"
    assert (valid != healthy).any(), "the N + 1-slot test and the N-slot test agree everywhere"
    groups = (slice(0, 22), slice(22, 43), slice(43, 64))
    for g in groups:                                       # every group has vehicles on both sides
        assert len(np.unique(valid[:, g])) == 2, g


def jog_path(J, M=400, ds=0.25, v=30.0, at=15.0):
    """Straight towards -x at v m/s, with one sideways step of J m after `at` m: the first half of a 1 s window lies on one line, the rest
    on another.  Distances to a vehicle that drives straight on are then two-valued, which is what it takes for the spread to decide:
    with every distance below 4 a ramp has a variance of 4 * 4 / 12 = 1.33 at the most."""
    k = int(round(at / ds))
    x = -np.concatenate((np.arange(k + 1) * ds, at + np.arange(M - k - 1) * ds))
    y = np.concatenate((np.zeros(k + 1), np.full(M - k - 1, float(J))))
    psi = np.arctan2(np.gradient(y), np.gradient(x))
    return x, y, psi, np.full(M, v)


JOG_STEP, JOG_OFFSETS = 3.0, np.linspace(-0.15, 0.05, 32)     # at step 1 the variance passes 2 near -0.05 m, by 0.009 from one vehicle to the next (CPU oracle)


def jog_poses(N, e, v=30.0):
    return np.array([(-v / N, float(y), math.pi, v, 0.0, 0.0, 0.0) for y in e]).T


def test_variance_and_the_65th_slot_decide():
    """N = 64 on a path with a sideways step: the distances are two-valued and the spread decides, with vehicles that have mean < 3 and
    max < 4 on both sides of variance = 2.  The sweep is dense enough for vehicle-steps where the 65th slot decides, the trailing zero that
    has no lane: variance >= 2 only with its (0 - mean)^2.  Found from the host oracle's x_opt in exact summation.  (At N = 20 no offset
    on such a path brings the variance to 2 while the maximum stays below 4: the horizon there has no case of this kind.)"""
    N, B, T = 64, 32, 3
    path = jog_path(JOG_STEP)
    pose = jog_poses(N, JOG_OFFSETS)
    res = _run(_fleet(N, B, path, threshold=1), _HostFleet(N, B, path, threshold=1), np.repeat(pose[None], T, axis=0))
    by_var = {0: 0, 1: 0}
    slot65 = 0
    for r in res:
        for b in range(B):
            for n, key in ((N + 1, "valid"), (N, "healthy")):
                mean, var, mx = distance_stats(r["x"][b], r["ref"][b][:, 0], r["ref"][b][:, 1], n)
                if mean < 2.9 and mx < 3.9 and abs(var - 2.0) > 1e-9:
                    assert r[key][b] == int(var < 2.0), (b, n, mean, var, mx)
                    by_var[int(var < 2.0)] += 1
                    if n == N + 1 and var >= 2.0 and var - mean * mean / (n - 1) < 2.0 - 1e-9:
                        slot65 += 1
    assert by_var[0] > 0 and by_var[1] > 0, by_var
    assert slot65 > 0, "no vehicle-step where the 65th slot decides"


# ---- 3. parameters

def _speed_window(fc):
    """The window's speeds after the clamp, [B][N]: row 3 of the step's reference block [B][6][N], the first region of its workspace."""
    B, N = fc.B, fc.N
    return fc._work[:B * 6 * N].view(B, 6, N)[:, 3].cpu().numpy()


def test_resample_off():
    """The problem of ROSGPMPC puts no weight on the speed (Q_DIAG_ROS[3] = 0), so the clamp cannot show in x_opt, w_opt or the command: the
    switch is held to the host where it acts, on the speeds of the window that the step hands to the solve."""
    N, B, T = 20, 16, 6
    path = _path()
    poses = _poses(B, T, seed=21)
    off, on = _fleet(N, B, path, resample=False), _fleet(N, B, path)
    h_off, h_on = _HostFleet(N, B, path, resample=False), _HostFleet(N, B, path)
    differs = np.zeros(B, dtype=bool)
    for t in range(T):
        r_off, r_on = h_off.step(poses[t]), h_on.step(poses[t])
        _compare(t, _dev_step(off, poses[t]), r_off)
        _compare(t, _dev_step(on, poses[t]), r_on)
        v_off, v_on = _speed_window(off), _speed_window(on)
        np.testing.assert_allclose(v_off, r_off["ref"][:, :, 3], rtol=0, atol=1e-12, err_msg="unclamped speeds at step %d" % t)
        np.testing.assert_allclose(v_on, r_on["ref"][:, :, 3], rtol=0, atol=1e-12, err_msg="clamped speeds at step %d" % t)
        differs |= (r_off["ref"][:, :, 3] != r_on["ref"][:, :, 3]).any(axis=1)
    assert differs.any() and not differs.all(), "the clamp acts on every vehicle or on none"


@pytest.mark.parametrize("threshold", [0, 1])
def test_threshold_0_and_1(threshold):
    """At 0 and at 1 the first step with status 0 and a healthy prediction commands, step 0 included; a failed solve resets the count."""
    N, B, T = 20, 16, 6
    path = _path_east()
    poses = _poses_east(B, T, seed=22)
    bad = 1
    poses[3, 0:2, bad] = np.nan                                          # a failed solve for one vehicle at step 3
    res = _run(_fleet(N, B, path, threshold=threshold), _HostFleet(N, B, path, threshold=threshold), poses)
    assert (res[0]["mode"] == 1).any() and (res[0]["mode"] == 0).any()
    assert res[2]["mode"][bad] == 1 and res[3]["status"][bad] == 4 and res[3]["mode"][bad] == 0 and res[3]["safe"][bad] == 0
    assert res[4]["mode"][bad] == 1 and res[4]["safe"][bad] == 1


@pytest.mark.parametrize("band", [None, (3.0, 5.0)])
def test_ends_of_the_blend_band(band):
    """v_x at blend_min and blend_max, one ulp outside and one ulp inside either: p is exactly 0 and exactly 1 at the ends and beyond."""
    from ad_mpc_amd import config as c
    N, B, T = 20, 16, 6
    lo, hi = band or (c.BLEND_MIN, c.BLEND_MAX)
    vx = [lo, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), hi, np.nextafter(hi, np.inf), np.nextafter(hi, -np.inf), 0.5 * (lo + hi)]
    path = _path()
    poses = _poses(B, T, seed=23)
    poses[:, 3, :len(vx)] = vx
    kw = {} if band is None else dict(blend_min=lo, blend_max=hi)
    res = _run(_fleet(N, B, path, **kw), _HostFleet(N, B, path, blend=band), poses)
    for r in res:
        p = r["p"]
        assert p[0] == 0.0 and p[1] == 0.0 and 0.0 < p[2] < 1e-12 and p[3] == 1.0 and p[4] == 1.0 and 1.0 - 1e-12 < p[5] < 1.0 and p[6] == 0.5, p[:7]


def test_yaw_fix_branches_and_yaw_zero():
    """Paths whose heading is 0.001 rad from +-pi.  yaw == 0.0 (and yaws too small to matter): neither branch may fire.  yaw just above 0
    with a heading just above -pi: + 2 pi; yaw just below 0 with a heading just below +pi: - 2 pi.  One host fleet per case, so that the
    branches are counted apart; every vehicle of a case takes its branch at every step."""
    N, T = 20, 4
    s = np.arange(400) * 0.5
    up = (-s, 0.001 * s, np.full(400, math.atan2(0.001, -1.0)), np.full(400, 8.0))       # heading pi - 0.001
    down = (-s, -0.001 * s, np.full(400, math.atan2(-0.001, -1.0)), np.full(400, 8.0))   # heading -pi + 0.001
    off = [0.002, 0.05, 0.3, 1.0]
    still = [0.0, -0.0, 1e-300, -1e-300]
    cases = (("yaw 0 on up", up, still, 0, 0), ("yaw 0 on down", down, still, 0, 0), ("plus", down, off, 1, 0),
             ("minus", up, [-v for v in off], 0, 1), ("same side", up, off, 0, 0))
    for name, path, yaws, plus, minus in cases:
        B = len(yaws)
        poses = np.zeros((T, 7, B))
        for t in range(T):
            poses[t, 0], poses[t, 1], poses[t, 2], poses[t, 3] = -0.4 - 0.1 * t, 0.2, yaws, 8.0
        host = _HostFleet(N, B, path)
        _run(_fleet(N, B, path), host, poses)
        assert (host.yaw_fix["plus"], host.yaw_fix["minus"]) == (plus * T * B, minus * T * B), (name, host.yaw_fix)


# ---- 4. past the command kernel's grid

def test_fleet_step_past_the_command_grid():
    """B = 65536 + 300 at N = 3: the command kernel's stride loop (vehicle b and b + 65536 share a workgroup, each with its own prev_u,
    has_valid and safe_count) and the assemble kernel's B * (N + 1) index.  Bitwise equal to two fresh fleets of B / 2 (below the grid:
    no stride), 64 vehicles equal to the host pipelines."""
    N, B, T = 3, R.COMMAND_PAST, 2
    half = B // 2
    assert R.command_grid(B) < B and R.command_grid(half) == half and 2 * half == B
    path = _path_east()                                     # valid predictions at step 0 already, so that two steps reach the fallback
    poses = _poses_east(B, T, seed=31, leave=(1, 2))        # vehicles 5, 13, .. leave the path at step 1: the fallback reads prev_u
    bad = 65536 + 150
    poses[1, 0:2, bad] = np.nan
    pick = np.array(sorted({0, 65535, 65536, B - 1, bad - 1, bad, bad + 1} | set(np.linspace(3, B - 7, 57).astype(int).tolist())))
    assert len(pick) == 64
    big, parts = _fleet(N, B, path, threshold=1), [_fleet(N, half, path, threshold=1) for _ in range(2)]
    host = _HostFleet(N, len(pick), path, threshold=1)
    last_valid_u = [None] * len(pick)
    for t in range(T):
        dev = _dev_step(big, poses[t])
        for i, fc in enumerate(parts):
            sl = slice(i * half, (i + 1) * half)
            sub = _dev_step(fc, poses[t][:, sl])
            for k in KEYS:
                _bits(dev[k][sl], sub[k], "step %d, half %d: %s" % (t, i, k))
        ref = host.step(poses[t][:, pick])
        _compare(t, {k: v[pick] for k, v in dev.items()}, ref)
        for j in range(len(pick)):
            if ref["valid"][j]:
                last_valid_u[j] = ref["u"][j].copy()
    for k, (a, b) in (("prev_u", (big.prev_u, [p.prev_u for p in parts])), ("has_valid", (big.has_valid, [p.has_valid for p in parts]))):
        _bits(a.cpu().numpy(), np.concatenate([p.cpu().numpy() for p in b]), k)
    # after step 2, as test_gate_reset_and_fallback: the count of the host, the previous VALID inputs, and whether there are any
    safe, pu, hv = big.safe_count.cpu().numpy()[pick], big.prev_u.cpu().numpy()[pick], big.has_valid.cpu().numpy()[pick]
    np.testing.assert_array_equal(safe, ref["safe"])
    j_bad = int(np.where(pick == bad)[0][0])
    assert ref["status"][j_bad] == 4 and safe[j_bad] == 0 and ref["mode"][j_bad] == 0
    for j in range(len(pick)):
        assert hv[j] == (last_valid_u[j] is not None), pick[j]
        if last_valid_u[j] is not None:
            np.testing.assert_allclose(pu[j], last_valid_u[j], rtol=0, atol=1e-12, err_msg="prev_u of vehicle %d" % pick[j])
    assert 0 < hv.sum() < len(pick) and host.fallbacks > 0
