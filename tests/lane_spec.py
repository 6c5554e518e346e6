"""The lane generator of include/admpc_lane.h restated in numpy / scipy (TEST INFRASTRUCTURE): where the lane starts, the cut with the
last waypoint repeated, the node's clamp, set_traj on the lane (serial cdist, compute_curvature with scipy's filtfilt), and
oracle.ref_traj_oracle.get_waypoints on that table.  tests/golden/lane.json (scripts/make_golden_lane.py: the reference's own
RefTrajectory on the same lanes) pins it in test_lane_cpu.py; test_lane_gpu.py compares the device against it."""
import math

import numpy as np
from scipy.signal import filtfilt

from oracle.ref_traj_oracle import get_waypoints

L_MIN, L_MAX = 34, 256
GRID = 4096                                                           # admpc_lane.hip: LANE_GRID
KEYS = ("x_ref", "y_ref", "psi_ref", "v_ref", "cdist_ref", "curv_ref")      # the rows of out_ref, in order


def search_range(M, lane_idx, back, ahead):
    """[lo, hi] of the waypoints that are searched: the whole route for a negative lane_idx, else the window around min(lane_idx, M - 1)."""
    if lane_idx < 0:
        return 0, M - 1
    i = min(int(lane_idx), M - 1)
    return max(0, i - back), min(M - 1, i + ahead)


def nearest(x, y, X0, Y0, lane_idx=-1, back=0, ahead=0):
    """First index of the smallest sqrt(dx^2 + dy^2) over the searched range; its first index where every distance is NaN."""
    lo, hi = search_range(len(x), lane_idx, back, ahead)
    with np.errstate(invalid="ignore"):
        d = np.sqrt((x[lo:hi + 1] - X0) ** 2 + (y[lo:hi + 1] - Y0) ** 2)
    if np.isnan(d).all():
        return lo
    return lo + int(np.nanargmin(d))


def bisector_clearance(x, y, X0, Y0, lane_idx=-1, back=0, ahead=0):
    """Distance of the pose from the nearest perpendicular bisector between the nearest waypoint of the searched range and any other
    waypoint of it -- its neighbours, and whatever else of the route comes close (a waypoint that coincides with the nearest one has
    none).  The bisectors between two waypoints of which neither is the nearest cannot change the answer and are left out.  Well above
    rounding -> the nearest index cannot hinge on it."""
    lo, hi = search_range(len(x), lane_idx, back, ahead)
    i0 = nearest(x, y, X0, Y0, lane_idx, back, ahead)
    ox, oy = np.delete(x[lo:hi + 1], i0 - lo), np.delete(y[lo:hi + 1], i0 - lo)
    ab = np.hypot(ox - x[i0], oy - y[i0])
    keep = ab > 0
    if not keep.any():
        return np.inf
    d0, dm = (X0 - x[i0]) ** 2 + (Y0 - y[i0]) ** 2, (X0 - ox) ** 2 + (Y0 - oy) ** 2
    return float(np.min(np.abs(dm - d0)[keep] / (2.0 * ab[keep])))


def cut(route, i0, L):
    """Waypoints i0 .. i0 + L - 1 of the route (vel, x, y, psi), the last one repeated past its end."""
    vel, x, y, psi = (np.asarray(c, dtype=np.float64) for c in route)
    idx = np.minimum(i0 + np.arange(L), len(x) - 1)
    return vel[idx].copy(), x[idx].copy(), y[idx].copy(), psi[idx].copy()


def clamp(vel, vx, vy, acc_max, clamp_dt):
    """The node's clamp of a lane at the vehicle's speed: the bound grows by repeated addition."""
    vel = np.array(vel, dtype=np.float64)
    bound = math.sqrt(vx * vx + vy * vy)
    for i in range(len(vel)):
        if vel[i] > bound:
            vel[i] = bound
        bound = bound + acc_max * clamp_dt * 0.8
    return vel


def filtfilt_restated(x):
    """scipy's filtfilt(ones(11) / 11, 1, x) in plain numpy: odd extension by 33 samples, the 11-tap mean forwards from the steady
    state of its first sample (ten copies of it in front), the same backwards, the middle len(x) samples."""
    x = np.asarray(x, dtype=np.float64)
    ext = np.concatenate((2.0 * x[0] - x[33:0:-1], x, 2.0 * x[-1] - x[-2:-35:-1]))

    def mean11(v):
        w = np.concatenate((np.full(10, v[0]), v))
        out = np.zeros(len(v))
        for t in range(10, -1, -1):                                   # oldest tap first
            out = w[10 - t:10 - t + len(v)] / 11.0 + out if t < 10 else w[10 - t:10 - t + len(v)] / 11.0
        return out
    return mean11(mean11(ext)[::-1])[::-1][33:-33]


def curvature(cdist, psi, filt=None):
    """compute_curvature of the reference; `filt` replaces scipy's filtfilt."""
    raw = np.diff(np.unwrap(psi)) / np.maximum(np.diff(cdist), 0.1)
    raw = np.insert(raw, len(raw), raw[-1])
    return filtfilt(np.ones((11,)) / 11, 1, raw) if filt is None else filt(raw)


def table(vel, x, y, psi, filt=None):
    """set_traj on a lane: [vel, x, y, psi, cdist, curv], the arc length summed serially."""
    cd = [0.0]
    for i in range(1, len(x)):
        cd.append(math.sqrt((x[i] - x[i - 1]) ** 2 + (y[i] - y[i - 1]) ** 2) + cd[-1])
    cd = np.array(cd)
    return np.column_stack((vel, x, y, psi, cd, curvature(cd, psi, filt)))


def lane_table(route, i0, L, speed=None, acc_max=0.0, clamp_dt=0.0, filt=None):
    """The table of the lane that begins at waypoint i0; speed = (vx, vy) clamps it, None does not."""
    vel, x, y, psi = cut(route, i0, L)
    if speed is not None:
        vel = clamp(vel, speed[0], speed[1], acc_max, clamp_dt)
    return table(vel, x, y, psi, filt)


def waypoints(route, lane_idx, X0, Y0, P0, L, back, ahead, H, dt, speed=None, acc_max=0.0, clamp_dt=0.0):
    """One vehicle: (i0, ref [6, H], err [3], stop)."""
    i0 = nearest(np.asarray(route[1], dtype=np.float64), np.asarray(route[2], dtype=np.float64), X0, Y0, lane_idx, back, ahead)
    with np.errstate(invalid="ignore"):
        w = get_waypoints(lane_table(route, i0, L, speed, acc_max, clamp_dt), H, dt, X0, Y0, P0)
    return i0, np.stack([w[k] for k in KEYS]), np.array([w["s0"], w["e_y0"], w["e_psi0"]]), int(w["stop"])


def columns(tab):
    """The seven device columns of a path whose table is `tab` (what RefTrajectory.set_traj uploads)."""
    return [tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3], np.unwrap(tab[:, 3]), tab[:, 4], tab[:, 5]]
