"""The numpy restatement of the rule of include/admpc_quad_poly_traj.h: the reference's ``random_trajectory`` / ``straight_trajectory``
behind their keyframes (utils/trajectories.py:307-354) -- ``fit_multi_segment_polynomial_trajectory`` and ``get_full_traj``
(utils/trajectory_generator.py:91-213, 255-265) in front of ``minimum_snap_trajectory_generator`` (trajectories.py:128-282, non-yawing
branch, no map limits) -- with the float type and the route to the coefficients as parameters, and the forward error bounds the tests hold
the device and the float64 spec against.

A case is a dict: ``keys`` [n_key][3], ``speed``, ``dt`` and ``quad`` (mass, J [3], x_f, y_f, z_l_tau [4], max_thrust).  The two routes:
  "solve"    np.linalg.solve(M_fit, b) per axis, as the reference does (float64), Gauss-Jordan in any other type
  "weights"  c = W p with W = M_fit^-1 S from a longdouble elimination rounded to float64, the sum in index order: the device's route
In float64 the sampling uses the reference's own numpy calls (np.arange, np.polyder, np.polyval); in longdouble t1 is the exact
2 j / s - 1 and compress the exact 2 / (s dt) of the float64 data, rounded once.  Nothing here reads the reference tree or the library."""
import math

import numpy as np

import quad_traj_spec as TS

U64 = TS.U64
GRAVITY = TS.GRAVITY
MAX_M = TS.MAX_M
MIN_KEYS, MAX_KEYS = 3, 32
_FALL = np.array([[math.factorial(a) // math.factorial(a - k) if a >= k else 0 for a in range(8)] for k in range(3)], dtype=np.float64)


# -- the fit ---------------------------------------------------------------------------------------------------------------------------
def _monomials(ts):
    """[8][8]: row d the d-th derivative of 1, t, .., t^7 at ts (matrix_generation)."""
    return np.array([[(math.factorial(a) // math.factorial(a - d)) * ts ** (a - d) if a >= d else 0.0 for a in range(8)] for d in range(8)])


def fit_matrix(n_seg):
    """multiple_waypoints(n_seg), n_seg >= 2: position and three derivatives at both ends, position and continuity of six derivatives
    at every inner keyframe.  Its entries are integers: exact in every float type."""
    lo, hi = _monomials(-1.0), _monomials(1.0)
    m = np.zeros((8 * n_seg, 8 * n_seg))
    m[0:4, 0:8] = lo[:4]
    for i in range(n_seg - 1):
        m[8 * i + 4:8 * i + 11, 8 * i:8 * i + 8] = hi[:7]
        m[8 * i + 5:8 * i + 11, 8 * i + 8:8 * i + 16] = -lo[1:7]
        m[8 * i + 11, 8 * i + 8:8 * i + 16] = lo[0]
    i = n_seg - 1
    m[8 * i + 4:8 * i + 8, 8 * i:8 * i + 8] = hi[:4]
    return m


def scatter(n_key):
    """S [8 n_seg][n_key]: rhs_generation(x) = S x."""
    n = n_key - 1
    s = np.zeros((8 * n, n_key))
    s[0, 0] = 1
    s[8 * n - 4, n] = 1
    for i in range(1, n):
        s[8 * (i - 1) + 4, i] = 1
        s[8 * (i - 1) + 11, i] = 1
    return s


def _gauss_jordan(a, b, ft):
    n = a.shape[0]
    w = np.concatenate([a.astype(ft), b.astype(ft)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(w[c:, c])))
        if p != c:
            w[[c, p]] = w[[p, c]]
        w[c] = w[c] / w[c, c]
        f = w[:, c].copy()
        f[c] = 0
        w -= f[:, None] * w[c][None, :]
    return w[:, n:]


_W = {}


def weights(n_key, ft=np.longdouble):
    """W = M_fit^-1 S [8 n_seg][n_key] by Gauss-Jordan with partial pivoting in ``ft`` (cached)."""
    if (n_key, ft) not in _W:
        _W[n_key, ft] = _gauss_jordan(fit_matrix(n_key - 1), scatter(n_key), ft)
    return _W[n_key, ft]


def fit_cond(n_key):
    return float(np.linalg.cond(fit_matrix(n_key - 1)))


def coefficients(keys, ft=np.float64, route="solve"):
    """[n_seg][8][3], ascending powers (the reference's, before its fliplr)."""
    p = np.asarray(keys, dtype=np.float64)
    n_key = p.shape[0]
    if route == "weights":
        w = weights(n_key).astype(np.float64).astype(ft)         # rounded to double once, as the device's copy is
        c = w[:, 0, None] * p[0].astype(ft)[None, :]
        for m in range(1, n_key):
            c = c + w[:, m, None] * p[m].astype(ft)[None, :]
    elif ft is np.float64:
        m_fit, s = fit_matrix(n_key - 1), scatter(n_key)
        c = np.stack([np.linalg.solve(m_fit, s @ p[:, ax]) for ax in range(3)], axis=1)
    else:
        c = weights(n_key, ft) @ p.astype(ft)
    return c.reshape(n_key - 1, 8, 3)


# -- the lengths -----------------------------------------------------------------------------------------------------------------------
def av_dist(keys):
    p = np.asarray(keys, dtype=np.float64)
    return np.mean(np.sqrt(np.sum(np.diff(p, axis=0) ** 2, axis=1)))


def lengths(dt, keys, speed):
    """(s, M): s = round(av_dist / speed / dt) as Python rounds a float64 (ties to even), M = n_seg s + 1."""
    s = int(round(av_dist(keys) / speed / dt))
    return s, (len(keys) - 1) * s + 1


def speed_for(keys, s, dt):
    """The speed at which the keyframes get s rows per segment: av_dist / (s dt)."""
    return float(av_dist(keys) / (s * dt))


# -- the sampling ----------------------------------------------------------------------------------------------------------------------
def sample(case, ft=np.float64, route="solve"):
    """(pos, vel, acc) [M,3] each, and the coefficients."""
    dt = float(case["dt"])
    s, M = lengths(dt, case["keys"], case["speed"])
    c = coefficients(case["keys"], ft, route)
    n_seg = c.shape[0]
    out = np.zeros((3, M, 3), dtype=ft)
    if ft is np.float64:
        T = s * dt
        t_vec = np.arange(0, T * (n_seg + 1) - 1e-5, T)
        row = 0
        for seg in range(n_seg):
            tau = np.arange(t_vec[seg], t_vec[seg + 1] + 1e-5, dt)
            t1 = (tau - t_vec[seg]) / (t_vec[seg + 1] - t_vec[seg]) * 2 - 1
            compress = 2 / np.diff(t_vec)[seg]
            n = len(t1) - (1 if seg < n_seg - 1 else 0)
            for k in range(3):
                for ax in range(3):
                    out[k, row:row + n, ax] = (np.polyval(np.polyder(c[seg, ::-1, ax], k), t1) * (compress ** k))[:n]
            row += n
        assert row == M, (row, M)
    else:
        i = np.arange(M)
        seg = np.minimum(i // s, n_seg - 1)
        j = i - seg * s
        t1 = ft(2) * j.astype(ft) / ft(s) - ft(1)
        compress = ft(2) / (ft(s) * ft(dt))
        for k in range(3):
            for ax in range(3):
                d = c[:, :, ax] * _FALL[k].astype(ft)[None, :]               # the k-th derivative's coefficients at power a - k
                y = np.zeros(M, dtype=ft)
                for a in range(7, k - 1, -1):
                    y = y * t1 + d[seg, a]
                out[k, :, ax] = y * compress ** k
    return out[0], out[1], out[2], c


def generate(case, ft=np.float64, route="solve", scan=np.cumsum, parts=False):
    """(traj [M,13], u [M,4]) in ``ft``; with ``parts`` also a dict of the intermediates the error bound reads.  From the thrust on these
    are the lines of quad_traj_spec.generate (steps 4 .. 9 of include/admpc_quad_traj.h), repeated here because that function takes its
    accelerations from a loop or a lemniscate and is not to be changed."""
    quad = case["quad"]
    dt = ft(case["dt"])
    pos, vel, acc, c = sample(case, ft, route)
    zero = np.zeros(pos.shape[0], dtype=ft)
    thrust = acc + np.array([0, 0, ft(GRAVITY)], dtype=ft)
    z_b = thrust / np.sqrt(thrust[:, 0] ** 2 + thrust[:, 1] ** 2 + thrust[:, 2] ** 2)[:, None]
    f_t = ft(quad["mass"]) * (z_b[:, 0] * thrust[:, 0] + z_b[:, 1] * thrust[:, 1] + z_b[:, 2] * thrust[:, 2])
    q = ft(0.5) * np.stack([ft(1.0) + z_b[:, 2], -z_b[:, 1], z_b[:, 0], zero], axis=1)
    q = q / np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2 + q[:, 2] ** 2 + q[:, 3] ** 2)[:, None]
    w0 = TS._rates(q, dt)
    term = -w0[:, 2] * dt
    term[0] = 0
    yaw = scan(term)
    corr = np.stack([np.cos(yaw / ft(2.0)), zero, zero, np.sin(yaw / ft(2.0))], axis=1)
    qn = TS._qmul(q, corr)
    qn[0] = q[0]
    rate = TS._rates(qn, dt)
    rate[0] = w0[0]
    rate_dot = TS._gradient(rate) / dt
    J = np.array(quad["J"], dtype=ft)
    cross = np.stack([(J[2] - J[1]) * rate[:, 2] * rate[:, 1], (J[0] - J[2]) * rate[:, 0] * rate[:, 2],
                      (J[1] - J[0]) * rate[:, 1] * rate[:, 0]], axis=1)
    tau = rate_dot * J[None, :] + cross
    b = np.concatenate([tau, f_t[:, None]], axis=1)
    u = TS._solve(TS.arm_matrix(quad, ft), b, ft) / ft(quad["max_thrust"])
    traj = np.concatenate([pos, qn, vel, rate], axis=1)
    x0, y0 = traj[0, 0], traj[0, 1]
    traj[:, 0] -= x0
    traj[:, 1] -= y0
    if not parts:
        return traj, u
    return traj, u, {"c": c, "pos": pos, "vel": vel, "acc": acc, "thrust": thrust, "z_b": z_b, "q_dot": TS._gradient(q) / dt,
                     "qn_dot": TS._gradient(qn) / dt, "w0": w0, "rate": rate, "rate_dot": rate_dot, "b": b, "u": u}


GROUPS = TS.GROUPS
group_errors = TS.group_errors


# -- the bounds ------------------------------------------------------------------------------------------------------------------------
def _bound(case, e_c, how):
    """The first-order forward error bound of every column group for a float64 evaluation of the rule whose coefficients err by ``e_c``
    [n_seg][8][3] and whose yaw scan has depth TS.scan_depth(M, how), against exact arithmetic on the same float64 data.  Every quantity
    of the trajectory it reads comes from the longdouble spec (weights route).  Errors of vectors are bounds of their 2-norm (the sum of
    the three axes' bounds); sqrt is taken at 1 ulp, sin and cos at 2 ulp.  Higher-order terms are covered by the factor 2 at the end."""
    _, _, p = generate(case, ft=np.longdouble, route="weights", parts=True)
    u_, dt = U64, float(case["dt"])
    quad = case["quad"]
    c = np.abs(p["c"]).astype(np.float64)                                      # [n_seg][8][3]
    n_seg = c.shape[0]
    s, M = lengths(dt, case["keys"], case["speed"])
    D = TS.scan_depth(M, how)
    T = M * dt
    compress = 2.0 / (s * dt)
    # step 2: t0 + j dt errs by (n_seg + 2) u T (the product, the sum, the difference; t0 itself cancels), t_next - t0 by (2 n_seg + 2) u T
    # (two products, the difference, T = s dt): N / D * 2 - 1 errs by 2 ((n_seg + 2) + (2 n_seg + 2)) u + 4 u; compress by (2 n_seg + 3) u
    e_t1 = (6 * n_seg + 12) * u_
    e = []
    for k, name in enumerate(("pos", "vel", "acc")):
        f = _FALL[k][None, :, None]                                            # a! / (a - k)!
        slope = np.array([max(a - k, 0) for a in range(8)], dtype=np.float64)[None, :, None]
        # step 3 at |t1| <= 1: the coefficients' own error; Horner of degree 7 (2 * 7 u sum|d_i|) with the k products of polyder and the product
        # with compress^k (4 u more); |p'| <= sum (a - k) |d_a| times the error of t1; compress^k errs by k (2 n_seg + 4) u of the value
        per_axis = np.max(np.sum(f * e_c + (2 * 7 + 4) * u_ * f * c + e_t1 * f * slope * c, axis=1), axis=0) * compress ** k
        per_axis = per_axis + k * (2 * n_seg + 4) * u_ * np.max(np.abs(p[name]).astype(np.float64), axis=0)
        e.append(float(np.sum(per_axis)))
    e_pos0, e_vel, e_acc = e
    e_pos = 2 * e_pos0 + 2 * u_ * float(np.max(np.abs(p["pos"])))             # the shift subtracts row 0's error and rounds
    # step 4, as quad_traj_spec.error_bound has it, with two generalisations: |thrust| >= tmin instead of >= 9.81 (the loop's acc.z is 0,
    # here it is not, and its sum with 9.81 rounds), and the vector under the quaternion's normalisation has norm sqrt((1 + z_b.z) / 2) >=
    # qmin instead of >= sqrt(1/2)
    tnorm = np.sqrt(np.sum(p["thrust"] ** 2, axis=1)).astype(np.float64)
    tmax, tmin = float(np.max(tnorm)), float(np.min(tnorm))
    qmin = float(np.min(np.sqrt((1 + p["z_b"][:, 2]) / 2)))
    e_thr = e_acc + u_ * tmax
    e_zb = 1.5 * e_thr / tmin + 5 * u_
    e_ft = float(quad["mass"]) * (tmax * (2 * e_zb + 4 * u_) + 1.5 * e_thr)
    e_q = 1.5 * e_zb * (math.sqrt(0.5) / qmin) + 8 * u_
    # steps 5 .. 8: the lines of quad_traj_spec.error_bound
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
    rmax = float(np.max(np.abs(p["rate"])))
    rdmax = float(np.max(np.abs(p["rate_dot"])))
    J = [float(v) for v in quad["J"]]
    dJ = max(abs(J[2] - J[1]), abs(J[0] - J[2]), abs(J[1] - J[0]))
    e_rd = 2 * e_rate / dt + 3 * u_ * rdmax
    e_tau = max(J) * e_rd + dJ * 2 * rmax * e_rate + 4 * u_ * (max(J) * rdmax + dJ * rmax ** 2)
    A = TS.arm_matrix(quad)
    Ai = np.abs(np.linalg.inv(A))
    e_b = np.array([e_tau, e_tau, e_tau, e_ft])
    bmax = np.max(np.abs(p["b"]).astype(np.float64), axis=0)
    umax = float(np.max(np.abs(p["u"])))
    e_u = float(np.max(Ai @ e_b + 6 * u_ * (Ai @ bmax))) / float(quad["max_thrust"]) + (8 * np.linalg.cond(A) + 2) * u_ * umax
    return {k: 2 * v for k, v in {"position": e_pos, "quaternion": e_qn, "velocity": e_vel, "rate": e_rate, "input": e_u}.items()}


def error_bound(case, how="kernel"):
    """The bound for the weights route (the device, the float64 spec): a coefficient is a sum of n_key products of W, itself rounded
    once, with a keyframe coordinate: (n_key + 2) u sum |W| |p|."""
    p = np.abs(np.asarray(case["keys"], dtype=np.float64))
    n_key = p.shape[0]
    e_c = (n_key + 2) * U64 * (np.abs(weights(n_key)).astype(np.float64) @ p)
    return _bound(case, e_c.reshape(n_key - 1, 8, 3), how)


def route_bound(case, how="serial"):
    """The bound for the solve route, and so for the difference of the two routes: LAPACK's solution of the 8 n_seg system errs by
    8 cond(M_fit) u max|c| per coefficient, the form quad_traj_spec.error_bound uses for the 4 x 4 solve, pushed through the same tail."""
    c = coefficients(case["keys"], np.longdouble, "weights")
    e_c = np.full(c.shape, 8 * fit_cond(len(case["keys"])) * U64 * float(np.max(np.abs(c))))
    return _bound(case, e_c, how)
