"""CPU anchors of the problem-data tests (tests/test_problem_data.py, tests/test_problem_data_quad.py).

Both oracles are restatements of the reference's models that the golden vectors pin only at the shipped vehicle.  Here one numpy
statement of each ODE, written from the reference's equations (ad_3d_optimizer.py:280-310, quad_3d_optimizer.py:358-393), checks
oracle.f / QuadOracle.f at random parameters (1e-13 relative) and the oracles' ERK4 step and its sensitivities against a numpy ERK4
with central differences -- so a field the two C restatements misread the same way (J[0] for J[1], x_f for y_f, L_F for L_R) fails
here.  Then source pins: the rules the GPU modules rely on to reach the kernels they claim.
"""
import os
import re

import numpy as np
import pytest

from ad_mpc_amd.config import default_config
from ad_mpc_amd.quad_config import QNU

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ad_mpc_amd", "csrc")


def car_ode(cfg, x, u, p):
    """Dynamic bicycle model blended with the kinematic one by the switch p (ad_3d_optimizer.py:280-310)."""
    psi, vx, vy, r, dl = x[2], x[3], x[4], x[5], x[6]
    v = vx + 1e-99
    front = 2 * cfg.Cf * (dl - (vy + cfg.L_F * r) / v)            # lateral tyre forces
    rear = 2 * cfg.Cr * (cfg.L_R * r - vy) / v
    L = cfg.L_F + cfg.L_R
    dyn = np.array([u[0] - front * np.sin(dl) / cfg.mass + vy * r,
                    (rear + front * np.cos(dl)) / cfg.mass - vx * r,
                    (cfg.L_F * front * np.cos(dl) - cfg.L_R * rear) / cfg.Iz])
    kin = np.array([u[0], (u[1] * vx + dl * u[0]) * cfg.L_R / L, (u[1] * vx + dl * u[0]) / L])
    return np.r_[vx * np.cos(psi) - vy * np.sin(psi), vx * np.sin(psi) + vy * np.cos(psi), r, p * dyn + (1 - p) * kin, u[1]]


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])


def _rotate(q, v):
    """v_dot_q (utils.py:315-338): R(q) v with R(q) = I + 2 w [e]x + 2 [e]x^2, q = (w, e) -- the rotation of a unit quaternion, applied
    as that formula to the slightly non-unit quaternions inside an integration step."""
    e = np.asarray(q[1:]); ex = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
    return (np.eye(3) + 2 * q[0] * ex + 2 * ex @ ex) @ v


def quad_ode(cfg, x, u):
    """Rigid body with four rotors (quad_3d_optimizer.py:358-393; g and the linear drag diag(rdrv) of the body-frame velocity as
    configured): p' = v, q' = q (0, w) / 2, v' = R(q) (0, 0, T / m) - (0, 0, g) + R(q) D R(q)' v, J w' = torques - w x J w."""
    q, v, w = x[3:7], x[7:10], x[10:13]
    f = cfg.max_thrust * np.asarray(u)
    J = np.array(cfg.J[:])
    qi = q * np.array([1, -1, -1, -1])
    vdot = _rotate(q, np.array([0.0, 0.0, f.sum() / cfg.mass])) - np.array([0.0, 0.0, cfg.g])
    vdot = vdot + _rotate(q, np.array(cfg.rdrv[:]) * _rotate(qi, v))
    tau = np.array([f @ np.array(cfg.y_f[:]), -f @ np.array(cfg.x_f[:]), f @ np.array(cfg.z_l_tau[:])])
    wdot = (tau - np.cross(w, J * w)) / J
    return np.r_[v, 0.5 * _qmul(q, np.r_[0.0, w]), vdot, wdot]


def erk4(f, x, u, h):
    k1 = f(x, u); k2 = f(x + h / 2 * k1, u); k3 = f(x + h / 2 * k2, u); k4 = f(x + h * k3, u)
    return x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)


def fd_sens(f, x, u, h, eps=1e-6):
    """Central differences of the ERK4 step in x and u."""
    A = np.empty((len(x), len(x))); B = np.empty((len(x), len(u)))
    for j in range(len(x)):
        e = np.zeros(len(x)); e[j] = eps
        A[:, j] = (erk4(f, x + e, u, h) - erk4(f, x - e, u, h)) / (2 * eps)
    for j in range(len(u)):
        e = np.zeros(len(u)); e[j] = eps
        B[:, j] = (erk4(f, x, u + e, h) - erk4(f, x, u - e, h)) / (2 * eps)
    return A, B


def random_car(rng):
    cfg = default_config(N=20, Ts=float(rng.uniform(0.02, 0.1)))
    for k in ("mass", "L_F", "L_R", "Iz", "Cf", "Cr"):
        setattr(cfg, k, getattr(cfg, k) * float(rng.uniform(0.7, 1.3)))
    return cfg


def random_car_point(rng):
    x = np.r_[rng.uniform(-50, 50, 2), rng.uniform(-np.pi, np.pi), rng.uniform(2, 15), rng.uniform(-0.5, 0.5, 2), rng.uniform(-0.4, 0.4)]
    return x, np.r_[rng.uniform(-5, 3), rng.uniform(-1, 1)], float(rng.choice([0.0, 1.0, rng.uniform()]))


def test_car_oracle_model_at_random_vehicles():
    from oracle.oracle import Oracle
    o = Oracle()
    rng = np.random.default_rng(5)
    for _ in range(40):
        cfg = random_car(rng)
        x, u, p = random_car_point(rng)
        want = car_ode(cfg, x, u, p)
        assert np.abs(o.f(cfg, x, u, p) - want).max() <= 1e-13 * np.abs(want).max()
        phi, A, B = o.rk4_sens(cfg, x, u, p, cfg.Ts)
        f = lambda xx, uu: car_ode(cfg, xx, uu, p)
        want = erk4(f, x, u, cfg.Ts)
        assert np.abs(phi - want).max() <= 1e-13 * np.abs(want).max()
        Afd, Bfd = fd_sens(f, x, u, cfg.Ts)
        assert np.abs(A - Afd).max() <= 1e-7 * max(1.0, np.abs(Afd).max()) and np.abs(B - Bfd).max() <= 1e-7 * max(1.0, np.abs(Bfd).max())


def random_quad(rng, plus=False):
    from test_problem_data_quad import random_quad_problem
    cfg = random_quad_problem(rng, 10, plus=plus, drag=bool(rng.integers(2)))
    return cfg


def random_quad_point(rng):
    q = rng.standard_normal(4); q /= np.linalg.norm(q)
    x = np.r_[rng.uniform(-3, 3, 3), q, rng.uniform(-2, 2, 3), rng.uniform(-1.5, 1.5, 3)]
    return x, rng.uniform(0, 1, 4)


@pytest.mark.parametrize("plus", [False, True])
def test_quad_oracle_model_at_random_vehicles(plus):
    from oracle.quad_oracle import QuadOracle
    o = QuadOracle()
    rng = np.random.default_rng(6 + plus)
    for _ in range(40):
        cfg = random_quad(rng, plus)
        x, u = random_quad_point(rng)
        want = quad_ode(cfg, x, u)
        assert np.abs(o.f(cfg, x, u) - want).max() <= 1e-13 * np.abs(want).max()
        phi, A, B = o.rk4_sens(cfg, x, u, cfg.Ts)
        f = lambda xx, uu: quad_ode(cfg, xx, uu)
        want = erk4(f, x, u, cfg.Ts)
        assert np.abs(phi - want).max() <= 1e-13 * np.abs(want).max()
        Afd, Bfd = fd_sens(f, x, u, cfg.Ts)
        assert np.abs(A - Afd).max() <= 1e-7 * max(1.0, np.abs(Afd).max()) and np.abs(B - Bfd).max() <= 1e-7 * max(1.0, np.abs(Bfd).max())


def test_quad_model_restatement_sees_every_field():
    """The numpy statement is not blind to the fields the GPU module draws: J[0] <-> J[1], x_f <-> y_f, a sign of z_l_tau and g all
    change the derivative at a generic point."""
    rng = np.random.default_rng(9)
    cfg = random_quad(rng)
    x, u = random_quad_point(rng)
    base = quad_ode(cfg, x, u)
    for edit in ("J", "arms", "ztau", "g"):
        c = cfg.copy()
        if edit == "J":
            c.J[0], c.J[1] = cfg.J[1], cfg.J[0]
        elif edit == "arms":
            for i in range(4):
                c.x_f[i], c.y_f[i] = cfg.y_f[i], cfg.x_f[i]
        elif edit == "ztau":
            c.z_l_tau[0] = -cfg.z_l_tau[0]
        else:
            c.g = cfg.g + 0.1
        assert np.abs(quad_ode(c, x, u) - base).max() > 1e-6, edit


# ---------------------------------------------------------------------------------------------------------------------------------
def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_qmask_rule_is_the_one_the_generator_relies_on():
    """tests/test_gpu_parity.py:random_q7_problem reaches the qmask-7 instantiation of kernels F and S by keeping W[3..6] = We[3..6] = 0;
    that is admpc_create's rule."""
    src = _read("admpc_kernels.hip")
    assert re.search(r"s->qmask = 7;\s*\n\s*for \(int c = 3; c < NX; \+\+c\) if \(cfg->W\[c\] != 0\.0 \|\| cfg->We\[c\] != 0\.0\) s->qmask = 127;", src)
    assert "s->use_dense = (cfg->N == 20)" in src


def test_quad_dispatch_maps_each_tested_horizon_to_its_kernel():
    """tests/test_problem_data_quad.py:PATHS names a kernel per (N, environment); admpc_quad.hip:quad_solve decides it this way."""
    from test_problem_data_quad import PATHS
    src = _read("admpc_quad.hip")
    body = src[src.index("static int quad_solve("):]
    body = body[:body.index("\n}")]
    assert "const bool seg20 = s->cfg.N == 20 && !s->wide20;" in body
    assert "else if (s->cfg.N * QU > 64)" in body and "admpc_quad_solve_kernel<WidePath>" in body
    assert "else if (s->cfg.N * QU == 40 && !s->generic)" in body and "admpc_quad_solve_kernel<Dense40Path>" in body
    assert 's->generic = e && e[0] == \'1\'' in src and 's->wide20 = e && e[0] == \'1\'' in src
    assert re.search(r'getenv\("ADMPC_QUAD_GENERIC"\)', src) and re.search(r'getenv\("ADMPC_QUAD_WIDE"\)', src)

    def kernel(N, env):                                  # the rule above, restated
        if N == 20 and env.get("ADMPC_QUAD_WIDE") != "1":
            return "seg"
        if N * QNU > 64:
            return "wide"
        return "dense40" if N * QNU == 40 and env.get("ADMPC_QUAD_GENERIC") != "1" else "generic"
    for name, (N, env, _) in PATHS.items():
        assert name.startswith(kernel(N, env) + "_"), name
