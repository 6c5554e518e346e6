"""Synthetic quadrotor scenarios: random states around hover, position / velocity targets, a hover-input iterate."""
import numpy as np

from .quad_config import QNX, QNU, QNY


def hover_input(cfg):
    return cfg.mass * cfg.g / (4.0 * cfg.max_thrust)


def random_quad_scenarios(B, cfg, seed=0, pos_err=1.5, tilt=0.3, aggressive=0.25):
    """x0: random position error, small random attitude (unit quaternion), velocity and body rates; reference: hover at the origin
    (a fraction `aggressive` of the instances gets a far target so that inputs saturate); iterate: x0 held, hover inputs."""
    rng = np.random.default_rng(seed)
    N = cfg.N
    x0 = np.zeros((B, QNX))
    x0[:, 0:3] = rng.uniform(-pos_err, pos_err, (B, 3))
    ax = rng.standard_normal((B, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = rng.uniform(0, tilt, B)
    x0[:, 3] = np.cos(ang / 2); x0[:, 4:7] = ax * np.sin(ang / 2)[:, None]
    x0[:, 7:10] = rng.uniform(-1, 1, (B, 3)); x0[:, 10:13] = rng.uniform(-0.5, 0.5, (B, 3))
    far = rng.uniform(size=B) < aggressive
    x0[far, 0:3] *= 6.0
    yref = np.zeros((B, N, QNY)); yref[:, :, 3] = 1.0; yref[:, :, QNX:] = hover_input(cfg)
    yref_e = np.zeros((B, QNX)); yref_e[:, 3] = 1.0
    xbar = np.repeat(x0[:, None, :], N + 1, axis=1)
    ubar = np.full((B, N, QNU), hover_input(cfg)) + rng.uniform(-0.02, 0.02, (B, N, QNU))
    return dict(x0=x0, yref=yref, yref_e=yref_e, xbar=xbar, ubar=ubar)


def circle_reference(M, dt, radius, speed, z=1.0, quad=None):
    """A flat-output reference for the closed loop (ad_mpc_amd/quad_fleet.py): M rows, dt apart, of a horizontal circle of `radius` at
    height z flown at constant `speed` with yaw 0 -- the role of the reference's ``loop_trajectory``, which needs ROS to import.  Returns
    (traj [M,13], u [M,4]): position; attitude from the thrust direction (z_b along a + g e_z, x_b in the world's x-z plane); velocity;
    body rates from the jerk; feed-forward activations from the rotor allocation matrix of `quad` (None: the vehicle of quad_3d.py)
    with the body torques J w' + w x J w (w' by a central difference of the analytic rates)."""
    from .quad_config import SimQuad
    quad = SimQuad() if quad is None else quad
    g = float(np.asarray(quad.g, dtype=np.float64).reshape(-1)[-1])
    J = np.asarray(quad.J, dtype=np.float64)
    om = float(speed) / float(radius)

    def frame(t):
        c, s = np.cos(om * t), np.sin(om * t)
        a = np.array([-radius * om ** 2 * c, -radius * om ** 2 * s, 0.0])
        j = np.array([radius * om ** 3 * s, -radius * om ** 3 * c, 0.0])
        f = a + np.array([0.0, 0.0, g])
        thrust = np.linalg.norm(f)
        zb = f / thrust
        yb = np.cross(zb, np.array([1.0, 0.0, 0.0])); yb /= np.linalg.norm(yb)
        xb = np.cross(yb, zb)
        hw = (j - zb.dot(j) * zb) / thrust
        return thrust, xb, yb, zb, np.array([-hw.dot(yb), hw.dot(xb), 0.0])

    traj, u = np.zeros((M, QNX)), np.zeros((M, QNU))
    alloc = np.stack([np.ones(4), np.asarray(quad.y_f, dtype=np.float64), -np.asarray(quad.x_f, dtype=np.float64),
                      np.asarray(quad.z_l_tau, dtype=np.float64)])
    h = 1e-5
    for i in range(M):
        t = i * float(dt)
        c, s = np.cos(om * t), np.sin(om * t)
        thrust, xb, yb, zb, w = frame(t)
        R = np.stack([xb, yb, zb], axis=1)
        qw = 0.5 * np.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2])
        q = np.array([qw, (R[2, 1] - R[1, 2]) / (4 * qw), (R[0, 2] - R[2, 0]) / (4 * qw), (R[1, 0] - R[0, 1]) / (4 * qw)])
        traj[i, 0:3] = [radius * c, radius * s, z]
        traj[i, 3:7] = q / np.linalg.norm(q)
        traj[i, 7:10] = [-radius * om * s, radius * om * c, 0.0]
        traj[i, 10:13] = w
        wdot = (frame(t + h)[4] - frame(t - h)[4]) / (2 * h)
        tau = J * wdot + np.cross(w, J * w)
        u[i] = np.linalg.solve(alloc, np.array([quad.mass * thrust, tau[0], tau[1], tau[2]])) / float(quad.max_thrust)
    return traj, u
