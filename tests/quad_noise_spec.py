"""The draws and the noisy plant step of include/admpc_quad_noise.h restated in numpy (TEST INFRASTRUCTURE): Philox4x32-10, the uniforms
and the Box-Muller transform as the header spells them, and `Quadrotor3D.update` under `noisy` and `motor_noise` (quad_mpc/quad_3d.py:
187-202, 271, 284-286) built on tests/quad_plant_spec.py, in the reference's operation order, so that tests/test_quad_noise_cpu.py can
hold it against the live simulator at 1e-15 with the spec's draws handed to it in place of np.random.normal's."""
import numpy as np

import quad_plant_spec as QS

WIDE_MAX, WIDE_LANES, LDS_DOUBLES = 8192, 4, 1600                    # admpc_quad_plant.hip: QN_WIDE_MAX, QN_LANES, QN_LDS_DOUBLES
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)
TWO_PI = 6.283185307179586


def philox4x32_10(counter, key):
    """counter: four arrays (or numbers) of 32-bit words, key: two; returns the four output words as uint64 arrays holding 32 bits."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]              # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c


def words(seed, b, p, m):
    """raw [..., 10] uint64: the ten w words (w0, w1 of j = 0 .. 4) of vehicle(s) b in period(s) p at sub-step(s) m (broadcast)."""
    b, p, m = np.broadcast_arrays(np.asarray(b, dtype=np.uint64), np.asarray(p, dtype=np.uint64), np.asarray(m, dtype=np.uint64))
    key = (int(seed) & 0xffffffff, int(seed) >> 32)
    out = np.zeros(b.shape + (10,), dtype=np.uint64)
    for j in range(5):
        o = philox4x32_10((b, p & MASK, p >> np.uint64(32), np.uint64(8) * m + np.uint64(j)), key)
        out[..., 2 * j] = o[0] | o[1] << np.uint64(32)
        out[..., 2 * j + 1] = o[2] | o[3] << np.uint64(32)
    return out


def normals(raw):
    """(z [..., 10], r [..., 5]) of the words raw [..., 10]: every operation rounded on its own, as numpy does."""
    u = ((raw >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u[..., 0::2]))
    a = TWO_PI * u[..., 1::2]
    z = np.empty(raw.shape)
    z[..., 0::2] = r * np.cos(a)
    z[..., 1::2] = r * np.sin(a)
    return z, r


def draws(seed, b, p, m):
    """z [..., 10]: the ten standard normals of vehicle b in period p at sub-step m."""
    return normals(words(seed, b, p, m))[0]


def deriv(plant, s, f, f_d, t_d):
    """quad_plant_spec.deriv with the disturbance force f_d [3,1] in f_vel (:271) and the torque t_d [3,1] in f_rate (:284-286)."""
    p, q, v, w = s
    mass = plant.mass
    g = np.array([[0.0], [0.0], [plant.g]])
    J = np.array(plant.J[:])
    xf, yf, zt = np.array(plant.x_f[:]), np.array(plant.y_f[:]), np.array(plant.z_l_tau[:])
    f_att = 1 / 2 * QS.skew4(w).dot(q)
    a_thrust = np.array([[0], [0], [np.sum(f)]]) / mass
    if plant.drag:
        rd = np.array(plant.rotor_drag[:])[:, np.newaxis]
        v_b = QS.rot(QS.conj(q)).dot(v)[:, np.newaxis]
        a_drag = -plant.aero_drag * v_b ** 2 * np.sign(v_b) / mass
        a_drag -= rd * v_b / mass
        a_drag = QS.rot(q).dot(a_drag)
    else:
        a_drag = np.zeros((3, 1))
    a_payload = -plant.payload_mass * g / mass
    f_vel = np.squeeze(-g + a_payload + a_drag + QS.rot(q).dot(a_thrust + f_d / mass))
    f_rate = np.array([1 / J[0] * (f.dot(yf) + t_d[0] + (J[1] - J[2]) * w[1] * w[2]),
                       1 / J[1] * (-f.dot(xf) + t_d[1] + (J[2] - J[0]) * w[2] * w[0]),
                       1 / J[2] * (f.dot(zt) + t_d[2] + (J[0] - J[1]) * w[0] * w[1])]).squeeze()
    return [v, f_att, f_vel, f_rate]


def update(plant, noise, s, a, z):
    """One Quadrotor3D.update under the clipped activations a [4] and the ten normals z of this sub-step."""
    if noise.motor_noise:
        f = np.zeros(4)
        for i in range(4):
            std = noise.motor_std * np.sqrt(a[i])
            n = noise.motor_bias * (a[i] / noise.motor_ref) ** 2 + std * z[i]          # np.random.normal(loc, scale) is loc + scale * z
            f[i] = max(min(a[i] - n, plant.u_max), plant.u_min) * plant.max_thrust
    else:
        f = a * plant.max_thrust
    if noise.noisy:
        f_d, t_d = (noise.force_std * z[4:7])[:, np.newaxis], (noise.torque_std * z[7:10])[:, np.newaxis]
    else:
        f_d, t_d = np.zeros((3, 1)), np.zeros((3, 1))
    dt = plant.dt
    k1 = deriv(plant, s, f, f_d, t_d)
    k2 = deriv(plant, [s[i] + dt / 2 * k1[i] for i in range(4)], f, f_d, t_d)
    k3 = deriv(plant, [s[i] + dt / 2 * k2[i] for i in range(4)], f, f_d, t_d)
    k4 = deriv(plant, [s[i] + dt * k3[i] for i in range(4)], f, f_d, t_d)
    s = [s[i] + dt * (1.0 / 6.0 * k1[i] + 2.0 / 6.0 * k2[i] + 2.0 / 6.0 * k3[i] + 1.0 / 6.0 * k4[i]) for i in range(4)]
    s[1] = 1 / np.sqrt(np.sum(s[1] ** 2)) * s[1]
    return s


def step(plant, noise, x, u, b, p):
    """One control period of vehicle b in period p: (the new state [13], whether an activation was replaced)."""
    x = np.array(x, dtype=np.float64)
    replaced = QS.activations(plant, u)[1]
    a = np.array([plant.u_min if not np.isfinite(np.float64(u[i])) else max(min(np.float64(u[i]), plant.u_max), plant.u_min) for i in range(4)])
    S = int(plant.substeps)
    z = draws(noise.seed, b, p, np.arange(S))
    s = [x[0:3].copy(), x[3:7].copy(), x[7:10].copy(), x[10:13].copy()]
    for m in range(S):
        s = update(plant, noise, s, a, z[m])
    return np.concatenate(s), replaced


def step_batch(plant, noise, X, U, p):
    """Vehicles 0 .. B-1 of a batch, each in its period p[b] (a number: the same for all)."""
    p = np.broadcast_to(np.asarray(p, dtype=np.uint64), (X.shape[0],))
    out = [step(plant, noise, X[b], U[b], b, p[b]) for b in range(X.shape[0])]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out])


def step_fleet(plant, noise, X, U, p):
    """The same period for a whole fleet at once, vectorised over the vehicles as quad_plant_spec.step_fleet is (elementwise formulas:
    the last bits differ from `step`): the plant of the CPU closed loop.  Returns (the new states [B,13], replaced [B])."""
    X = np.array(X, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    B = X.shape[0]
    bad = ~np.isfinite(U)
    A = np.where(bad, plant.u_min, np.clip(np.where(bad, 0.0, U), plant.u_min, plant.u_max))
    J, mass = np.array(plant.J[:]), plant.mass
    yf, xf, zt = np.array(plant.y_f[:]), np.array(plant.x_f[:]), np.array(plant.z_l_tau[:])
    rd = np.array(plant.rotor_drag[:])
    p = np.broadcast_to(np.asarray(p, dtype=np.uint64), (B,))
    S = int(plant.substeps)
    Z = draws(noise.seed, np.arange(B)[:, None], p[:, None], np.arange(S)[None, :])            # [B, S, 10]

    def R(q):
        qw, qx, qy, qz = q.T
        return np.stack([np.stack([1 - 2 * (qy ** 2 + qz ** 2), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)], 1),
                         np.stack([2 * (qx * qy + qw * qz), 1 - 2 * (qx ** 2 + qz ** 2), 2 * (qy * qz - qw * qx)], 1),
                         np.stack([2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx ** 2 + qy ** 2)], 1)], 1)

    dt = plant.dt
    for m in range(S):
        z = Z[:, m]
        if noise.motor_noise:
            n = noise.motor_bias * (A / noise.motor_ref) ** 2 + noise.motor_std * np.sqrt(A) * z[:, 0:4]
            F = np.clip(A - n, plant.u_min, plant.u_max) * plant.max_thrust
        else:
            F = A * plant.max_thrust
        fd = noise.force_std * z[:, 4:7] if noise.noisy else np.zeros((B, 3))
        td = noise.torque_std * z[:, 7:10] if noise.noisy else np.zeros((B, 3))
        push = fd / mass
        push[:, 2] += F.sum(1) / mass
        ty, tx, tz = F @ yf + td[:, 0], -(F @ xf) + td[:, 1], F @ zt + td[:, 2]

        def f(Sx):
            q, v, w = Sx[:, 3:7], Sx[:, 7:10], Sx[:, 10:13]
            k = np.zeros_like(Sx)
            k[:, 0:3] = v
            k[:, 3] = 0.5 * (-w[:, 0] * q[:, 1] - w[:, 1] * q[:, 2] - w[:, 2] * q[:, 3])
            k[:, 4] = 0.5 * (w[:, 0] * q[:, 0] + w[:, 2] * q[:, 2] - w[:, 1] * q[:, 3])
            k[:, 5] = 0.5 * (w[:, 1] * q[:, 0] - w[:, 2] * q[:, 1] + w[:, 0] * q[:, 3])
            k[:, 6] = 0.5 * (w[:, 2] * q[:, 0] + w[:, 1] * q[:, 1] - w[:, 0] * q[:, 2])
            Rm = R(q)
            acc = np.einsum("bij,bj->bi", Rm, push)
            if plant.drag:
                vb = np.einsum("bji,bj->bi", Rm, v)
                ab = -plant.aero_drag * vb ** 2 * np.sign(vb) / mass - rd * vb / mass
                acc = acc + np.einsum("bij,bj->bi", Rm, ab)
            acc[:, 2] += -plant.g - plant.payload_mass * plant.g / mass
            k[:, 7:10] = acc
            k[:, 10] = (ty + (J[1] - J[2]) * w[:, 1] * w[:, 2]) / J[0]
            k[:, 11] = (tx + (J[2] - J[0]) * w[:, 2] * w[:, 0]) / J[1]
            k[:, 12] = (tz + (J[0] - J[1]) * w[:, 0] * w[:, 1]) / J[2]
            return k

        k1 = f(X); k2 = f(X + dt / 2 * k1); k3 = f(X + dt / 2 * k2); k4 = f(X + dt * k3)
        X = X + dt * (k1 / 6 + k2 / 3 + k3 / 3 + k4 / 6)
        X[:, 3:7] /= np.sqrt((X[:, 3:7] ** 2).sum(1))[:, None]
    return X, bad.any(1)
