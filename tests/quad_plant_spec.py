"""The plant step, the reference window and the tally of include/admpc_quad_fleet.h restated in numpy (TEST INFRASTRUCTURE), one vehicle
at a time, in the operation order of the reference's simulator (quad_mpc/quad_3d.py:175-287 with the helpers of utils/utils.py) and with
the numpy primitives it uses (3 x 3 and 4 x 4 `dot`, `np.sum`, `u.dot`), so that tests/test_quad_fleet_cpu.py can hold it against the
live `Quadrotor3D.update` at 1e-15."""
import numpy as np

GRID, LANES = 4096, 64                                               # admpc_quad_fleet.hip: QP_GRID and the block of the plant kernel
PAST_THE_GRID = GRID * LANES + 301                                   # 262 445 vehicles: the plant's stride loop runs
CHUNK_GRID, CHUNK_THREADS = 4096, 256                                # QC_GRID, QC_THREADS: one thread per double written


def rot(q):
    """q_to_rot_mat (utils.py:323-338)."""
    qw, qx, qy, qz = q[0], q[1], q[2], q[3]
    return np.array([[1 - 2 * (qy ** 2 + qz ** 2), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                     [2 * (qx * qy + qw * qz), 1 - 2 * (qx ** 2 + qz ** 2), 2 * (qy * qz - qw * qx)],
                     [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx ** 2 + qy ** 2)]])


def conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def skew4(w):
    """skew_symmetric (utils.py:392-404): the 4 x 4 form."""
    return np.array([[0, -w[0], -w[1], -w[2]],
                     [w[0], 0, w[2], -w[1]],
                     [w[1], -w[2], 0, w[0]],
                     [w[2], w[1], -w[0], 0]])


def activations(plant, u):
    """(thrusts [4] in N, replaced): the clip of quad_3d.py:184-194; a non-finite activation becomes u_min and is reported."""
    a, replaced = np.zeros(4), False
    for i in range(4):
        ui = np.float64(u[i])
        if not np.isfinite(ui):
            a[i], replaced = plant.u_min, True
        else:
            a[i] = max(min(ui, plant.u_max), plant.u_min)
    return a * plant.max_thrust, replaced


def deriv(plant, s, f):
    """[f_pos, f_att, f_vel, f_rate] at s = [p, q, v, w] (arrays of 3, 4, 3, 3) under the thrusts f."""
    p, q, v, w = s
    mass = plant.mass
    g = np.array([[0.0], [0.0], [plant.g]])
    J = np.array(plant.J[:])
    xf, yf, zt = np.array(plant.x_f[:]), np.array(plant.y_f[:]), np.array(plant.z_l_tau[:])
    f_att = 1 / 2 * skew4(w).dot(q)
    a_thrust = np.array([[0], [0], [np.sum(f)]]) / mass
    if plant.drag:
        rd = np.array(plant.rotor_drag[:])[:, np.newaxis]
        v_b = rot(conj(q)).dot(v)[:, np.newaxis]
        a_drag = -plant.aero_drag * v_b ** 2 * np.sign(v_b) / mass
        a_drag -= rd * v_b / mass
        a_drag = rot(q).dot(a_drag)
    else:
        a_drag = np.zeros((3, 1))
    a_payload = -plant.payload_mass * g / mass
    f_vel = np.squeeze(-g + a_payload + a_drag + rot(q).dot(a_thrust + np.zeros((3, 1)) / mass))
    f_rate = np.array([1 / J[0] * (f.dot(yf) + 0.0 + (J[1] - J[2]) * w[1] * w[2]),
                       1 / J[1] * (-f.dot(xf) + 0.0 + (J[2] - J[0]) * w[2] * w[0]),
                       1 / J[2] * (f.dot(zt) + 0.0 + (J[0] - J[1]) * w[0] * w[1])])
    return [v, f_att, f_vel, f_rate]


def update(plant, s, f):
    """One Quadrotor3D.update: classic RK4 with step plant.dt, then unit_quat (utils.py:299-312)."""
    dt = plant.dt
    k1 = deriv(plant, s, f)
    k2 = deriv(plant, [s[i] + dt / 2 * k1[i] for i in range(4)], f)
    k3 = deriv(plant, [s[i] + dt / 2 * k2[i] for i in range(4)], f)
    k4 = deriv(plant, [s[i] + dt * k3[i] for i in range(4)], f)
    s = [s[i] + dt * (1.0 / 6.0 * k1[i] + 2.0 / 6.0 * k2[i] + 2.0 / 6.0 * k3[i] + 1.0 / 6.0 * k4[i]) for i in range(4)]
    s[1] = 1 / np.sqrt(np.sum(s[1] ** 2)) * s[1]
    return s


def step(plant, x, u):
    """One control period for one vehicle: (the new state [13], whether an activation was replaced)."""
    x = np.array(x, dtype=np.float64)
    f, replaced = activations(plant, u)
    s = [x[0:3].copy(), x[3:7].copy(), x[7:10].copy(), x[10:13].copy()]
    for _ in range(int(plant.substeps)):
        s = update(plant, s, f)
    return np.concatenate(s), replaced


def step_batch(plant, X, U):
    out = [step(plant, X[b], U[b]) for b in range(X.shape[0])]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out])


def chunk(traj, u, idx, N, over):
    """(yref [N,17], yref_e [13], pos_ref [3]) of include/admpc_quad_fleet.h's closed form; NaN where idx is outside [0, M)."""
    M = traj.shape[0]
    if not 0 <= idx < M:
        return np.full((N, 17), np.nan), np.full(13, np.nan), np.full(3, np.nan)
    L = min(N + 1, -(-(M - idx) // over))
    yref = np.zeros((N, 17))
    for j in range(N):
        yref[j, :13] = traj[idx + min(j, L - 1) * over]
        yref[j, 13:] = u[idx + min(j, max(L - 2, 0)) * over]
    return yref, traj[idx + min(N, L - 1) * over].copy(), traj[idx, :3].copy()


def chunk_batch(bank, traj_of, idx, N, over):
    """The windows of a fleet: bank = [(traj, u), ...]; a traj_of outside the bank gives NaN rows."""
    B = len(traj_of)
    yref, yref_e, pos = np.full((B, N, 17), np.nan), np.full((B, 13), np.nan), np.full((B, 3), np.nan)
    for b in range(B):
        if 0 <= traj_of[b] < len(bank):
            yref[b], yref_e[b], pos[b] = chunk(bank[traj_of[b]][0], bank[traj_of[b]][1], int(idx[b]), N, over)
    return yref, yref_e, pos


def next_idx(bank, traj_of, idx):
    """idx <- min(idx + 1, M - 1) where the vehicle has a window; the others keep theirs."""
    out = np.array(idx, dtype=np.int32)
    for b in range(len(out)):
        if 0 <= traj_of[b] < len(bank):
            M = bank[traj_of[b]][0].shape[0]
            if 0 <= out[b] < M:
                out[b] = min(out[b] + 1, M - 1)
    return out


def tally_step(tally, counts, pos_ref, x, status, replaced):
    """One step of the rollout's sums for one vehicle, in place: tally float64 [3], counts int32 [3]; x the state at the START of the step."""
    e = np.asarray(pos_ref, dtype=np.float64) - np.asarray(x, dtype=np.float64)[0:3]
    with np.errstate(all="ignore"):
        n2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    if np.isfinite(n2):
        n = np.sqrt(n2)
        tally[0] = tally[0] + n
        tally[1] = tally[1] + n2
        tally[2] = max(tally[2], n)
    counts[0] += 1
    counts[1] += 1 if int(status) != 0 else 0
    counts[2] += 1 if replaced else 0


def random_states(B, seed, tilt=0.5):
    """[B,13]: positions, unit quaternions up to `tilt` rad off level, velocities to 6 m/s, body rates to 2 rad/s."""
    rng = np.random.default_rng(seed)
    X = np.zeros((B, 13))
    X[:, 0:3] = rng.uniform(-3, 3, (B, 3))
    ax = rng.standard_normal((B, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = rng.uniform(0, tilt, B)
    X[:, 3] = np.cos(ang / 2); X[:, 4:7] = ax * np.sin(ang / 2)[:, None]
    X[:, 7:10] = rng.uniform(-6, 6, (B, 3)); X[:, 10:13] = rng.uniform(-2, 2, (B, 3))
    return X


def fleet67(nan_input=True):
    """(X [67,13], U [67,4]) of the plant tests: activations on both sides of [0, 1] and inside; vehicle 5 level (q = 1) with v_y = 0, so
    that one body-frame velocity component is exactly 0; vehicle 9 with one NaN activation (nan_input)."""
    X = random_states(67, 31)
    rng = np.random.default_rng(32)
    U = rng.uniform(-0.3, 1.3, (67, 4))
    U[0] = [0.2, 0.4, 0.6, 0.8]
    X[5, 3:7] = [1.0, 0.0, 0.0, 0.0]; X[5, 8] = 0.0
    if nan_input:
        U[9, 2] = np.nan
    return X, U


def step_fleet(plant, X, U):
    """The same period for a whole fleet at once, vectorised over the vehicles (elementwise formulas instead of the 3 x 3 products, so
    the last bits differ from `step`): the plant of the CPU closed loop, where a tolerance of 1e-8 is at stake and not 1e-15.
    Returns (the new states [B,13], replaced [B])."""
    X = np.array(X, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    bad = ~np.isfinite(U)
    F = np.where(bad, plant.u_min, np.clip(np.where(bad, 0.0, U), plant.u_min, plant.u_max)) * plant.max_thrust
    J, m = np.array(plant.J[:]), plant.mass
    az = F.sum(1) / m
    ty, tx, tz = F @ np.array(plant.y_f[:]), F @ np.array(plant.x_f[:]), F @ np.array(plant.z_l_tau[:])
    rd = np.array(plant.rotor_drag[:])

    def R(q):
        qw, qx, qy, qz = q.T
        return np.stack([np.stack([1 - 2 * (qy ** 2 + qz ** 2), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)], 1),
                         np.stack([2 * (qx * qy + qw * qz), 1 - 2 * (qx ** 2 + qz ** 2), 2 * (qy * qz - qw * qx)], 1),
                         np.stack([2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx ** 2 + qy ** 2)], 1)], 1)

    def f(S):
        q, v, w = S[:, 3:7], S[:, 7:10], S[:, 10:13]
        k = np.zeros_like(S)
        k[:, 0:3] = v
        k[:, 3] = 0.5 * (-w[:, 0] * q[:, 1] - w[:, 1] * q[:, 2] - w[:, 2] * q[:, 3])
        k[:, 4] = 0.5 * (w[:, 0] * q[:, 0] + w[:, 2] * q[:, 2] - w[:, 1] * q[:, 3])
        k[:, 5] = 0.5 * (w[:, 1] * q[:, 0] - w[:, 2] * q[:, 1] + w[:, 0] * q[:, 3])
        k[:, 6] = 0.5 * (w[:, 2] * q[:, 0] + w[:, 1] * q[:, 1] - w[:, 0] * q[:, 2])
        Rm = R(q)
        acc = Rm[:, :, 2] * az[:, None]
        if plant.drag:
            vb = np.einsum("bji,bj->bi", Rm, v)
            ab = -plant.aero_drag * vb ** 2 * np.sign(vb) / m - rd * vb / m
            acc = acc + np.einsum("bij,bj->bi", Rm, ab)
        acc[:, 2] += -plant.g - plant.payload_mass * plant.g / m
        k[:, 7:10] = acc
        k[:, 10] = (ty + (J[1] - J[2]) * w[:, 1] * w[:, 2]) / J[0]
        k[:, 11] = (-tx + (J[2] - J[0]) * w[:, 2] * w[:, 0]) / J[1]
        k[:, 12] = (tz + (J[0] - J[1]) * w[:, 0] * w[:, 1]) / J[2]
        return k

    dt = plant.dt
    for _ in range(int(plant.substeps)):
        k1 = f(X); k2 = f(X + dt / 2 * k1); k3 = f(X + dt / 2 * k2); k4 = f(X + dt * k3)
        X = X + dt * (k1 / 6 + k2 / 3 + k3 / 3 + k4 / 6)
        X[:, 3:7] /= np.sqrt((X[:, 3:7] ** 2).sum(1))[:, None]
    return X, bad.any(1)
