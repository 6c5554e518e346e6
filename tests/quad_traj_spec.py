"""The numpy restatement of the rule of include/admpc_quad_traj.h: the reference's ``loop_trajectory`` / ``lemniscate_trajectory``
(utils/trajectories.py:357-561) behind ``minimum_snap_trajectory_generator`` (:128-282), non-yawing branch, no map limits -- vectorised,
with the float type and the scan as parameters -- and the forward error bound the tests hold the device and the float64 spec against.

A case is a dict: kind ("loop" / "lemniscate"), clockwise, radius, z, lin_acc, v_max, dt, and ``quad``: mass, J [3], x_f, y_f, z_l_tau [4],
max_thrust.  Nothing here reads the reference tree or the library."""
import math

import numpy as np

U64 = 2.0 ** -53                 # the unit round-off of float64
TILE, WAVE = 256, 64             # the kernel's scan structure
MAX_M = 16384                    # ADMPC_QUAD_TRAJ_MAX_M
GRAVITY = 9.81                   # trajectories.py:154

DEFAULT_QUAD = {                 # the simulator's vehicle (quad_3d.py:39-75)
    "mass": 1.0, "J": [.03, .03, .06], "max_thrust": 20.0,
    "x_f": [math.cos(math.pi / 4) * 0.235 * s for s in (1, -1, -1, 1)],
    "y_f": [math.cos(math.pi / 4) * 0.235 * s for s in (-1, -1, 1, 1)],
    "z_l_tau": [-0.013, 0.013, -0.013, 0.013],
}


def lengths(dt, case):
    """The five np.arange lengths, ceil((stop - 0) / dt) in double: the stops are 2, coasting, 4, coasting, 2."""
    t_total = 2 * float(case["v_max"]) / float(case["lin_acc"]) + 2 * 2
    coasting = (t_total - 4 * 2) / 2
    return [max(0, int(math.ceil(stop / float(dt)))) for stop in (2.0, coasting, 4.0, coasting, 2.0)]


def kernel_scan(v):
    """The inclusive scan as the kernel forms it (include/admpc_quad_traj.h, THE SCAN): tiles of 256, a Hillis-Steele scan per 64 lanes,
    the totals of the waves in front summed serially, out = carry + (waves_before + v), the carry the tile's last lane."""
    v = np.asarray(v)
    M = v.shape[0]
    out = np.zeros_like(v)
    carry = v.dtype.type(0)
    for r0 in range(0, M, TILE):
        t = np.zeros(TILE, dtype=v.dtype)
        t[:min(TILE, M - r0)] = v[r0:r0 + TILE]
        t = t.reshape(TILE // WAVE, WAVE).copy()
        d = 1
        while d < WAVE:
            nxt = t.copy()
            nxt[:, d:] = t[:, :-d] + t[:, d:]
            t, d = nxt, d * 2
        res = np.empty_like(t)
        for m in range(TILE // WAVE):
            if m == 0:
                r = t[0]
            else:
                before = t[0, -1]
                for mm in range(1, m):
                    before = before + t[mm, -1]
                r = before + t[m]
            res[m] = carry + r
        res = res.reshape(-1)
        carry = res[-1]
        out[r0:r0 + TILE] = res[:min(TILE, M - r0)]
    return out


def _qmul(q, r):
    """q_dot_q of utils.py:341 on rows."""
    qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rw, rx, ry, rz = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    return np.stack([rw * qw - rx * qx - ry * qy - rz * qz,
                     rw * qx + rx * qw - ry * qz + rz * qy,
                     rw * qy + rx * qz + ry * qw - rz * qx,
                     rw * qz - rx * qy + ry * qx + rz * qw], axis=1)


def _gradient(f):
    """np.gradient(f, axis=0): central inside, one-sided at both ends."""
    g = np.empty_like(f)
    g[1:-1] = (f[2:] - f[:-2]) / f.dtype.type(2.0)
    g[0] = f[1] - f[0]
    g[-1] = f[-1] - f[-2]
    return g


def _rates(q, dt):
    inv = q * np.array([1, -1, -1, -1], dtype=q.dtype)
    return q.dtype.type(2.0) * _qmul(inv, _gradient(q) / dt)[:, 1:]


def arm_matrix(quad, ft=np.float64):
    return np.array([quad["y_f"], [-v for v in quad["x_f"]], quad["z_l_tau"], [1.0] * 4], dtype=ft)


def _solve(a, b, ft):
    """Rows of solve(a, b[i]); float64 through LAPACK as the reference does, any other type by Gauss-Jordan with partial pivoting."""
    if ft is np.float64:
        return np.linalg.solve(a, b.T).T
    n = a.shape[0]
    w = np.concatenate([a.astype(ft), b.T.astype(ft)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(w[c:, c])))
        w[[c, p]] = w[[p, c]]
        w[c] = w[c] / w[c, c]
        for r in range(n):
            if r != c:
                w[r] = w[r] - w[r, c] * w[c]
    return w[:, n:].T


def alpha(case, ft=np.float64):
    """Step 1: the angular acceleration of every row."""
    dt = ft(case["dt"])
    n = lengths(case["dt"], case)
    a = ft(case["lin_acc"]) / ft(case["radius"])
    q4 = ft(np.pi) / ft(4.0)                                             # the double pi of the reference, whatever ft is
    t = lambda m: np.arange(m).astype(ft) * dt
    ramp = a * np.sin(q4 * t(n[0])) ** 2
    al = np.concatenate([ramp, np.ones(n[1], dtype=ft) * a, a * np.cos(q4 * t(n[2])), -np.ones(n[3], dtype=ft) * a,
                         (a * np.sin(q4 * t(n[4])) ** 2) - a])
    return al if case["clockwise"] else -al


def generate(case, ft=np.float64, scan=np.cumsum, parts=False):
    """(traj [M,13], u [M,4]) in ``ft``; with ``parts`` also a dict of the intermediates the error bound reads."""
    quad = case["quad"]
    dt, R, z = ft(case["dt"]), ft(case["radius"]), ft(case["z"])
    al = alpha(case, ft)
    w = scan(al) * dt
    ang = scan(w) * dt
    s, c = np.sin(ang), np.cos(ang)
    zero = np.zeros_like(ang)
    if case["kind"] == "loop":
        pos = np.stack([R * s, R * c, zero + z], axis=1)
        vel = np.stack([R * w * c, -(R * w * s), zero], axis=1)
        acc = np.stack([R * (al * c - w ** 2 * s), -R * (al * s + w ** 2 * c), zero], axis=1)
    else:
        pos = np.stack([R * c, R * (s * c), zero + z], axis=1)
        vel = np.stack([-R * (w * s), R * (w * c ** 2 - w * s ** 2), zero], axis=1)
        acc = np.stack([-R * (al * s + w ** 2 * c),
                        R * (al * c ** 2 - ft(2.0) * w ** 2 * c * s - al * s ** 2 - ft(2.0) * w ** 2 * s * c), zero], axis=1)
    thrust = acc + np.array([0, 0, ft(GRAVITY)], dtype=ft)
    z_b = thrust / np.sqrt(thrust[:, 0] ** 2 + thrust[:, 1] ** 2 + thrust[:, 2] ** 2)[:, None]
    f_t = ft(quad["mass"]) * (z_b[:, 0] * thrust[:, 0] + z_b[:, 1] * thrust[:, 1] + z_b[:, 2] * thrust[:, 2])
    q = ft(0.5) * np.stack([ft(1.0) + z_b[:, 2], -z_b[:, 1], z_b[:, 0], zero], axis=1)
    q = q / np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2 + q[:, 2] ** 2 + q[:, 3] ** 2)[:, None]
    w0 = _rates(q, dt)
    term = -w0[:, 2] * dt
    term[0] = 0
    yaw = scan(term)
    corr = np.stack([np.cos(yaw / ft(2.0)), zero, zero, np.sin(yaw / ft(2.0))], axis=1)
    qn = _qmul(q, corr)
    qn[0] = q[0]
    rate = _rates(qn, dt)
    rate[0] = w0[0]
    rate_dot = _gradient(rate) / dt
    J = np.array(quad["J"], dtype=ft)
    cross = np.stack([(J[2] - J[1]) * rate[:, 2] * rate[:, 1], (J[0] - J[2]) * rate[:, 0] * rate[:, 2],
                      (J[1] - J[0]) * rate[:, 1] * rate[:, 0]], axis=1)
    tau = rate_dot * J[None, :] + cross
    b = np.concatenate([tau, f_t[:, None]], axis=1)
    u = _solve(arm_matrix(quad, ft), b, ft) / ft(quad["max_thrust"])
    traj = np.concatenate([pos, qn, vel, rate], axis=1)
    x0, y0 = traj[0, 0], traj[0, 1]
    traj[:, 0] -= x0
    traj[:, 1] -= y0
    if not parts:
        return traj, u
    return traj, u, {"alpha": al, "w": w, "thrust": thrust, "q_dot": _gradient(q) / dt, "qn_dot": _gradient(qn) / dt, "w0": w0, "rate": rate,
                     "rate_dot": rate_dot, "b": b, "u": u}


GROUPS = {"position": slice(0, 3), "quaternion": slice(3, 7), "velocity": slice(7, 10), "rate": slice(10, 13)}


def scan_depth(M, how):
    """The largest number of additions a term passes through on its way into a partial sum.  "kernel": per tile 6 steps in the wave, at
    most 2 for the waves in front, 1 to join them, 1 for the carry: 10 per tile on the chain of carries.  "serial": np.cumsum, M - 1."""
    return 10 * ((M + TILE - 1) // TILE) if how == "kernel" else max(M - 1, 1)


def error_bound(case, how="kernel"):
    """The first-order forward error bound of every column group, {"position", "quaternion", "velocity", "rate", "input"} -> float, for
    a float64 evaluation of the rule whose scans have depth ``scan_depth(M, how)``, against exact arithmetic on the same float64 data.
    The derivation is DESIGN.md's (the trajectory generator's section); every quantity of the trajectory it reads (sums of |alpha| and
    |w|, the largest |w|, thrust, quaternion derivative, rate, rate derivative and right-hand side) comes from the longdouble spec.  u is
    2^-53; sin and cos are taken at 2 ulp and sqrt at 1 ulp (4 u and 2 u relative), the figures of the HIP math documentation for
    double precision; numpy's are not worse.  Higher-order terms are covered by the factor 2 at the end."""
    ld = np.longdouble
    _, _, p = generate(case, ft=ld, parts=True)
    M = len(p["alpha"])
    D = scan_depth(M, how)
    u_, dt, R = U64, float(case["dt"]), float(case["radius"])
    quad = case["quad"]
    a = float(case["lin_acc"]) / R
    T = M * dt
    sum_alpha = float(np.sum(np.abs(p["alpha"]))) * dt
    sum_w = float(np.sum(np.abs(p["w"]))) * dt
    wmax = float(np.max(np.abs(p["w"])))
    # step 1: t = j dt and pi / 4 * t round once each (|argument| <= pi), sin / cos 4 u, the square, the product with a, a itself, "- a"
    e_alpha = (2 * math.pi + 4 + 3 + 1 + 1) * u_ * a
    # step 2: a sum of depth D errs by D u sum|terms|; the terms' own errors add up; the product with dt rounds once
    e_w = (D + 1) * u_ * sum_alpha + T * e_alpha
    e_th = (D + 1) * u_ * sum_w + T * e_w
    # step 3: |d sin|, |d cos| <= e_th + 4 u
    e_sc = e_th + 4 * u_
    e_pos = 2 * (R * (2 * e_sc + 3 * u_)) + 2 * R * u_                   # R s c at worst; the shift subtracts row 0's error and rounds
    e_vel = R * (e_w + 3 * wmax * e_sc + 6 * u_ * wmax)
    e_acc = R * (e_alpha + 3 * a * e_sc + 4 * wmax * e_w + 6 * wmax ** 2 * e_sc + 10 * u_ * (a + 4 * wmax ** 2))
    # step 4: |thrust| >= 9.81; normalising divides the error by it; the sum of squares, sqrt (2 u) and the division round
    tmax = float(np.max(np.sqrt(np.sum(p["thrust"] ** 2, axis=1))))
    e_zb = 1.5 * e_acc / GRAVITY + 5 * u_
    e_ft = float(quad["mass"]) * (tmax * (2 * e_zb + 4 * u_) + 1.5 * e_acc)
    e_q = 1.5 * e_zb + 8 * u_                                            # the vector before normalising has norm >= sqrt(1/2)
    # steps 5 .. 7: a difference quotient divides by dt (one-sided: both neighbours' errors in full); a quaternion product is bilinear
    qd = float(np.max(np.sqrt(np.sum(p["q_dot"] ** 2, axis=1))))
    qnd = float(np.max(np.sqrt(np.sum(p["qn_dot"] ** 2, axis=1))))
    e_qd = 2 * e_q / dt + 3 * u_ * qd
    e_w0 = 4 * e_q * qd + 4 * e_qd + 10 * u_ * qd
    sum_yaw = float(np.sum(np.abs(p["w0"][1:, 2]))) * dt
    e_yaw = (D + 1) * u_ * sum_yaw + T * e_w0
    e_qn = 2 * e_q + 1.5 * (e_yaw / 2 + 4 * u_) + 5 * u_
    dmax = max(qd, qnd)
    e_qnd = 2 * e_qn / dt + 3 * u_ * dmax
    e_rate = 4 * e_qn * dmax + 4 * e_qnd + 10 * u_ * dmax
    # step 8: the second quotient, the torque, the 4 x 4 solve (its own error: 8 cond(A) u of the solution)
    rmax = float(np.max(np.abs(p["rate"])))
    rdmax = float(np.max(np.abs(p["rate_dot"])))
    J = [float(v) for v in quad["J"]]
    dJ = max(abs(J[2] - J[1]), abs(J[0] - J[2]), abs(J[1] - J[0]))
    e_rd = 2 * e_rate / dt + 3 * u_ * rdmax
    e_tau = max(J) * e_rd + dJ * 2 * rmax * e_rate + 4 * u_ * (max(J) * rdmax + dJ * rmax ** 2)
    A = arm_matrix(quad)
    Ai = np.abs(np.linalg.inv(A))
    e_b = np.array([e_tau, e_tau, e_tau, e_ft])
    bmax = np.max(np.abs(p["b"]).astype(np.float64), axis=0)
    umax = float(np.max(np.abs(p["u"])))
    e_u = float(np.max(Ai @ e_b + 6 * u_ * (Ai @ bmax))) / float(quad["max_thrust"]) + (8 * np.linalg.cond(A) + 2) * u_ * umax
    return {k: 2 * v for k, v in {"position": e_pos, "quaternion": e_qn, "velocity": e_vel, "rate": e_rate, "input": e_u}.items()}


def group_errors(traj, u, traj_ref, u_ref):
    """The largest absolute difference per column group."""
    err = {k: float(np.max(np.abs(np.asarray(traj, dtype=np.longdouble)[:, s] - traj_ref[:, s]))) for k, s in GROUPS.items()}
    err["input"] = float(np.max(np.abs(np.asarray(u, dtype=np.longdouble) - u_ref)))
    return err


def find_case(target_M, dts, ratios):
    """(dt, ratio, n) of the first pair in the grid whose lengths add up to ``target_M`` with n2 >= 1; None if there is none."""
    for dt in dts:
        for r in ratios:
            n = lengths(dt, {"v_max": r, "lin_acc": 1.0})
            if n[1] >= 1 and sum(n) == target_M:
                return dt, r, n
    return None
