"""ctypes mirror of include/admpc_quad.h (AdmpcQuadConfig) and the shipped quadrotor problem
(acados_models/my_quad_acados_ocp.json, src/quad_mpc/quad_3d.py:40-74); of include/admpc_quad_fleet.h (AdmpcQuadPlantParams), the
simulator's vehicle (src/quad_mpc/quad_3d.py:22-95); of include/admpc_quad_learn.h (AdmpcQuadObserveParams), the regressors a fleet
learns on the device; of include/admpc_quad_noise.h (AdmpcQuadNoiseParams), the simulator's random disturbances; of
include/admpc_quad_targets.h (AdmpcQuadTargetParams), the targets a fleet chases."""
import ctypes as C
import math

import numpy as np

from .config import AdmpcGp, AdmpcGpBins, GP_MAX_FEAT, GP_MAX_POINTS, learn_bins

QNX, QNU, QNY, QUAD_MAX_N, QUAD_GP_MAX = 13, 4, 17, 24, 3


class AdmpcQuadConfig(C.Structure):
    _fields_ = [
        ("N", C.c_int32), ("ipm_iter_max", C.c_int32), ("Ts", C.c_double),
        ("W", C.c_double * QNY), ("We", C.c_double * QNX),
        ("lbu", C.c_double * QNU), ("ubu", C.c_double * QNU),
        ("mass", C.c_double), ("J", C.c_double * 3), ("max_thrust", C.c_double),
        ("x_f", C.c_double * 4), ("y_f", C.c_double * 4), ("z_l_tau", C.c_double * 4), ("g", C.c_double), ("rdrv", C.c_double * 3),
        ("ipm_mu0", C.c_double), ("ipm_thr0", C.c_double), ("ipm_tol_comp", C.c_double), ("ipm_tol_res", C.c_double),
        ("sqp_tol", C.c_double),
        ("n_gp", C.c_int32), ("sqp_iters", C.c_int32), ("gp", AdmpcGp * QUAD_GP_MAX),
    ]

    def copy(self):
        c = AdmpcQuadConfig()
        C.memmove(C.byref(c), C.byref(self), C.sizeof(self))
        return c


def default_quad_config(N=10, t_horizon=1.0):
    """my_quad_acados_ocp.json: N = 10, tf = 1 s, W = diag(10,10,10, 0,.1,.1,.1, .05 x 6, .1 x 4), W_e = 0, 0 <= u <= 1;
    vehicle of quad_3d.py ('x' configuration)."""
    if not (2 <= N <= QUAD_MAX_N):
        raise ValueError("N must be in [2, %d]" % QUAD_MAX_N)
    c = AdmpcQuadConfig()
    c.N, c.ipm_iter_max, c.Ts = int(N), 50, float(t_horizon) / N
    for i, v in enumerate([10.0] * 3 + [0.0] + [0.1] * 3 + [0.05] * 6 + [0.1] * 4):
        c.W[i] = v
    for i in range(QNX):
        c.We[i] = 0.0
    for i in range(QNU):
        c.lbu[i], c.ubu[i] = 0.0, 1.0
    c.mass, c.max_thrust, c.g = 1.0, 20.0, 9.81
    c.J[0], c.J[1], c.J[2] = 0.03, 0.03, 0.06
    h = math.cos(math.pi / 4) * (0.47 / 2)
    for i, (xf, yf, zt) in enumerate(zip((h, -h, -h, h), (-h, -h, h, h), (-0.013, 0.013, -0.013, 0.013))):
        c.x_f[i], c.y_f[i], c.z_l_tau[i] = xf, yf, zt
    c.ipm_mu0, c.ipm_thr0 = 1.0, 0.1
    c.sqp_iters, c.sqp_tol = 1, 0.0                 # SQP_RTI (the shipped solver_type); "SQP": sqp_iters 100, sqp_tol 1e-6 (my_quad_acados_ocp.json:2075-2080)
    c.ipm_tol_comp, c.ipm_tol_res = 1e-8, 1e-8      # the reference's levels: HPIPM mode BALANCE (acados_models/my_quad_acados_ocp.json leaves qp_solver_tol_* unset); tight_quad_ipm: 1e-10 / 1e-9
    return c


def set_quad_gp(cfg, gps):
    """Residual GPs of the quadrotor (quad_3d_optimizer.py:289-327).  ``gps``: dicts as for ``config.set_gp``; ``feat`` indexes
    z = [x with the velocity in the body frame (13); u (4)], ``out`` in {7, 8, 9} is the body-frame acceleration component."""
    from .config import AdmpcConfig, set_gp
    gps = list(gps)
    if len(gps) > QUAD_GP_MAX:
        raise ValueError("at most %d GPs" % QUAD_GP_MAX)
    tmp = AdmpcConfig()
    set_gp(tmp, gps)                              # fills AdmpcGp entries (same struct)
    for g, d in enumerate(gps):
        feats = [int(f) for f in np.atleast_1d(d["feat"]).reshape(-1)]
        if not (7 <= int(d["out"]) <= 9) or any(not (7 <= f < QNX + QNU) for f in feats):
            raise ValueError("quadrotor GP: out must be in {7, 8, 9}, features in [7, 17) (body-frame velocity, body rates, inputs)")
        C.memmove(C.byref(cfg.gp[g]), C.byref(tmp.gp[g]), C.sizeof(AdmpcGp))
    cfg.n_gp = len(gps)
    return cfg


def tight_quad_ipm(cfg):
    """The stop levels of earlier rounds (complementarity 1e-10, residual 1e-9), in place; returns cfg."""
    cfg.ipm_tol_comp, cfg.ipm_tol_res = 1e-10, 1e-9
    return cfg


def tight_quad_config(*a, **kw):
    return tight_quad_ipm(default_quad_config(*a, **kw))


class AdmpcQuadPlantParams(C.Structure):
    """include/admpc_quad_fleet.h: the SIMULATOR's vehicle (Quadrotor3D), passed by value into the plant kernel."""
    _fields_ = [
        ("dt", C.c_double), ("mass", C.c_double), ("J", C.c_double * 3), ("max_thrust", C.c_double),
        ("x_f", C.c_double * 4), ("y_f", C.c_double * 4), ("z_l_tau", C.c_double * 4), ("g", C.c_double),
        ("rotor_drag", C.c_double * 3), ("aero_drag", C.c_double), ("payload_mass", C.c_double),
        ("u_min", C.c_double), ("u_max", C.c_double),
        ("substeps", C.c_int32), ("drag", C.c_int32),
    ]

    def copy(self):
        c = AdmpcQuadPlantParams()
        C.memmove(C.byref(c), C.byref(self), C.sizeof(self))
        return c


class AdmpcQuadNoiseParams(C.Structure):
    """include/admpc_quad_noise.h: the key of the generator, the two switches, the scales of the reference's distributions."""
    _fields_ = [("seed", C.c_uint64), ("noisy", C.c_int32), ("motor_noise", C.c_int32), ("force_std", C.c_double), ("torque_std", C.c_double),
                ("motor_bias", C.c_double), ("motor_ref", C.c_double), ("motor_std", C.c_double)]


class AdmpcQuadTargetParams(C.Structure):
    """include/admpc_quad_targets.h: the key of the targets' generator, how the next target is found, when one counts as reached and
    when a vehicle is recovered."""
    _fields_ = [("seed", C.c_uint64), ("mode", C.c_int32), ("n_preset", C.c_int32), ("world_radius", C.c_double), ("thresh", C.c_double),
                ("v_max", C.c_double), ("max_iters", C.c_int32), ("pad", C.c_int32)]


TARGET_MODES = {"preset": 0, "aggressive": 1, "uniform": 2}


class AdmpcQuadTrajSpec(C.Structure):
    """include/admpc_quad_traj.h: one generated reference trajectory, a loop or a lemniscate that ramps to v_max and back."""
    _fields_ = [("kind", C.c_int32), ("clockwise", C.c_int32), ("radius", C.c_double), ("z", C.c_double), ("lin_acc", C.c_double),
                ("v_max", C.c_double)]


TRAJ_KINDS = {"loop": 0, "lemniscate": 1}
QUAD_TRAJ_MAX_M = 16384     # ADMPC_QUAD_TRAJ_MAX_M


def quad_traj_specs(kind, v_max, radius=5.0, z=1.0, lin_acc=None, clockwise=True):
    """(AdmpcQuadTrajSpec * K) of ``QuadFleet.generate_trajectories``'s arguments, each a scalar or a length-K sequence (K: the longest;
    a scalar goes to all).  ``lin_acc=None`` is 0.25 * v_max, the comparative experiment's choice.  A kind that is not "loop" or
    "lemniscate" and sequences of different lengths are ValueErrors; the values themselves are the library's to refuse."""
    cols = {"kind": kind, "v_max": v_max, "radius": radius, "z": z, "lin_acc": lin_acc, "clockwise": clockwise}
    seq = {k: (list(v) if isinstance(v, (list, tuple, np.ndarray)) else None) for k, v in cols.items()}
    lens = {len(v) for v in seq.values() if v is not None}
    if len(lens) > 1 or 0 in lens:
        raise ValueError("quad_traj_specs: the sequences among the arguments must have one length, at least 1")
    K = lens.pop() if lens else 1
    col = {k: (seq[k] if seq[k] is not None else [cols[k]] * K) for k in cols}
    specs = (AdmpcQuadTrajSpec * K)()
    for k in range(K):
        if col["kind"][k] not in TRAJ_KINDS:
            raise ValueError("quad_traj_specs: kind must be one of %s" % sorted(TRAJ_KINDS))
        s = specs[k]
        s.kind, s.clockwise = TRAJ_KINDS[col["kind"][k]], 1 if col["clockwise"][k] else 0
        s.v_max, s.radius, s.z = float(col["v_max"][k]), float(col["radius"][k]), float(col["z"][k])
        s.lin_acc = 0.25 * s.v_max if col["lin_acc"][k] is None else float(col["lin_acc"][k])
    return specs


QUAD_POLY_TRAJ_KEYS = (3, 32)     # ADMPC_QUAD_POLY_TRAJ_MIN_KEYS, ADMPC_QUAD_POLY_TRAJ_MAX_KEYS


def quad_poly_traj_args(keyframes, speed):
    """(keys float64 [K,n_key,3] C-contiguous, speed float64 [K]) of ``QuadFleet.generate_polynomial_trajectories``'s arguments:
    keyframes [K,n_key,3] or [n_key,3] (K: the speed's length then, or 1), speed a scalar or a length-K sequence.  Shapes that do not fit
    are ValueErrors; the values themselves are the library's to refuse (include/admpc_quad_poly_traj.h)."""
    keys = np.array(keyframes, dtype=np.float64)
    sp = np.array(speed, dtype=np.float64)
    if sp.ndim > 1 or keys.ndim not in (2, 3) or keys.shape[-1] != 3 or keys.shape[-2] < 1:
        raise ValueError("quad_poly_traj_args: keyframes are [K,n_key,3] or [n_key,3], speed a scalar or [K]")
    if keys.ndim == 2:
        keys = np.broadcast_to(keys, (sp.shape[0] if sp.ndim else 1,) + keys.shape)
    K = keys.shape[0]
    if K < 1 or (sp.ndim == 1 and sp.shape[0] != K):
        raise ValueError("quad_poly_traj_args: speed must be a scalar or have one entry per trajectory, at least one")
    return np.ascontiguousarray(keys), np.ascontiguousarray(np.broadcast_to(sp, (K,)))


def quad_target_params(mode="aggressive", world_radius=3.0, thresh=0.05, v_max=14.0, max_iters=100, seed=None, n_preset=0):
    """AdmpcQuadTargetParams with the reference's constants (point_tracking_and_record.py:112, :204, :255); every refusal of the header
    is a ValueError here.  ``seed`` (0 .. 2^64 - 1) is needed by the two random modes."""
    if mode not in TARGET_MODES:
        raise ValueError("quad_target_params: mode must be one of %s" % sorted(TARGET_MODES))
    world_radius, thresh, v_max = float(world_radius), float(thresh), float(v_max)
    if not (world_radius > 0 and math.isfinite(world_radius)):
        raise ValueError("quad_target_params: world_radius must be positive and finite")
    if not (thresh > 0 and math.isfinite(thresh)):
        raise ValueError("quad_target_params: thresh must be positive and finite")
    if math.isnan(v_max):
        raise ValueError("quad_target_params: v_max must not be NaN")
    if int(max_iters) != max_iters or not 0 <= int(max_iters) < 2 ** 31:
        raise ValueError("quad_target_params: max_iters must be an integer in [0, 2^31)")
    t = AdmpcQuadTargetParams()
    t.mode = TARGET_MODES[mode]
    if t.mode == 0:
        if not 1 <= int(n_preset) < 2 ** 31:
            raise ValueError("quad_target_params: mode 'preset' needs at least one preset target per vehicle")
        t.n_preset, seed = int(n_preset), 0 if seed is None else seed
    elif seed is None:
        raise ValueError("quad_target_params: mode '%s' needs a seed" % mode)
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError("quad_target_params: seed must be in [0, 2^64)")
    t.seed, t.world_radius, t.thresh, t.v_max, t.max_iters = int(seed), world_radius, thresh, v_max, int(max_iters)
    return t


class AdmpcQuadObserveParams(C.Structure):
    """include/admpc_quad_learn.h: the period between two states, the RK4 sub-steps of the prediction, the regressors to learn."""
    _fields_ = [("dt", C.c_double), ("substeps", C.c_int32), ("n_gp", C.c_int32), ("gp", AdmpcGpBins * QUAD_GP_MAX)]


QUAD_REC = 14       # doubles per sample record: v_b (3), body rates (3), activations (4), y (3), the flag


def quad_learn_bins(learn):
    """The AdmpcGpBins of QuadFleet(learn=...): ``config.learn_bins`` with the quadrotor's ranges -- feat in 7 .. 16 (an index into
    z = [x with the velocity in the body frame; u], or a list of up to 3), out in 7 .. 9, at most QUAD_GP_MAX regressors."""
    return learn_bins(learn, feat_range=(7, QNX + QNU - 1), out_range=(7, 9), gp_max=QUAD_GP_MAX)


def select_request(blocks, n_points=None):
    """``n_points`` of ``QuadEnsembleFleet.select_points`` checked as admpc_quad_ensemble_select_points checks it
    (include/admpc_quad_select.h), for the K blocks ``blocks`` of a fleet that learns ([(AdmpcGpBins array, n_gp)] of
    ``ensemble_layout``): a scalar, one value per regressor, or None for each regressor's nbins.  Returns QUAD_GP_MAX ints, the
    entries past n_gp zero.  Raises ValueError; needs no GPU."""
    n = blocks[0][1]
    for bins, _ in blocks:
        if any(int(bins[g].n_feat) != 1 for g in range(n)):
            raise ValueError("select_points: a regressor with more than one feature: the selection is offered for one-feature regressors")
    most = [min(GP_MAX_POINTS, min(int(bins[g].nb[0]) * int(bins[g].nb[1]) * int(bins[g].nb[2]) for bins, _ in blocks)) for g in range(n)]
    if n_points is None:
        want = list(most)
    else:
        want = np.atleast_1d(np.asarray(n_points)).reshape(-1)
        if want.size == 1:
            want = np.repeat(want, n)
        if want.size != n:
            raise ValueError("select_points: n_points must be a scalar or one value per regressor (%d)" % n)
        if any(int(w) != w for w in want):
            raise ValueError("select_points: n_points must be whole numbers")
        want = [int(w) for w in want]
    for g in range(n):
        if not 1 <= want[g] <= most[g]:
            raise ValueError("select_points: n_points of regressor %d must be in 1 .. %d (min(32, its nbins)), got %d" % (g, most[g], want[g]))
    return want + [0] * (QUAD_GP_MAX - n)


class SimQuad:
    """The attributes of the reference's ``Quadrotor3D`` (quad_3d.py:22-95) that the plant reads, with its values: the vehicle of
    ``quad_plant_params(None, ...)`` and of the tests."""

    def __init__(self, drag=False, payload=False, noisy=False, motor_noise=False):
        self.max_thrust = 20
        self.max_input_value, self.min_input_value = 1, 0
        self.J = np.array([.03, .03, .06])
        self.mass = 1.0
        self.length = 0.47 / 2
        h = np.cos(np.pi / 4) * self.length
        self.x_f = np.array([h, -h, -h, h])
        self.y_f = np.array([-h, -h, h, h])
        self.c = 0.013
        self.z_l_tau = np.array([-self.c, self.c, -self.c, self.c])
        self.g = np.array([[0], [0], [9.81]])
        self.rotor_drag_xy, self.rotor_drag_z = 0.3, 0.0
        self.aero_drag = 0.08
        self.drag, self.noisy, self.motor_noise = drag, noisy, motor_noise
        self.payload_mass = 0.3 * payload


def quad_substeps(simulation_dt, control_period):
    """The sub-steps of one control period as trajectory_test.py:114-119 counts them: ``while t < control_period: t += simulation_dt``
    in floating point (40 at N = 10, 20 at N = 20, 80 at N = 5 with t_horizon 1 s, over-sampling 5 and simulation_dt 5e-4)."""
    simulation_dt, control_period = float(simulation_dt), float(control_period)
    if not (simulation_dt > 0 and math.isfinite(simulation_dt) and math.isfinite(control_period)):
        raise ValueError("simulation_dt must be positive and finite, control_period finite")
    t, n = 0.0, 0
    while t < control_period:
        t += simulation_dt
        n += 1
        if n > 1024:
            raise ValueError("more than 1024 sub-steps per control period")
    if n < 1:
        raise ValueError("control_period must be positive")
    return n


def quad_is_noisy(quad):
    return quad is not None and bool(getattr(quad, "noisy", False) or getattr(quad, "motor_noise", False))


def quad_noise_params(quad, simulation_dt, seed):
    """AdmpcQuadNoiseParams of a ``Quadrotor3D``-shaped object: its switches ``noisy`` and ``motor_noise``, the reference's constants
    (quad_3d.py:190-199: f_d and t_d with std 10 * dt per sub-step; a rotor's error with mean 0.1 * (u / 1.3)^2 and std 0.02 * sqrt(u))
    and the generator's key ``seed`` (0 .. 2^64 - 1)."""
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError("quad_noise_params: seed must be in [0, 2^64)")
    n = AdmpcQuadNoiseParams()
    n.seed = int(seed)
    n.noisy, n.motor_noise = int(bool(getattr(quad, "noisy", False))), int(bool(getattr(quad, "motor_noise", False)))
    n.force_std = n.torque_std = 10 * float(simulation_dt)
    n.motor_bias, n.motor_ref, n.motor_std = 0.1, 1.3, 0.02
    return n


def quad_plant_params(quad, simulation_dt, control_period, allow_noise=False):
    """AdmpcQuadPlantParams of a ``Quadrotor3D``-shaped object (None: ``SimQuad()``): mass, J, max_thrust, x_f, y_f, z_l_tau, g (a scalar
    or the reference's 3 x 1 vector), drag, rotor_drag_xy / rotor_drag_z, aero_drag, payload_mass, min_input_value / max_input_value.
    The random disturbances are not the plant parameters' business: ``noisy`` or ``motor_noise`` set raises NotImplementedError unless
    the caller says with ``allow_noise`` that it flies them through ``quad_noise_params`` and the entries of include/admpc_quad_noise.h."""
    if quad is None:
        quad = SimQuad()
    if quad_is_noisy(quad) and not allow_noise:
        raise NotImplementedError("the simulator's random disturbances (noisy, motor_noise: np.random per sub-step) are not offered by the deterministic "
                                  "plant on the device: give QuadFleet a noise_seed (include/admpc_quad_noise.h)")
    p = AdmpcQuadPlantParams()
    p.dt, p.substeps = float(simulation_dt), quad_substeps(simulation_dt, control_period)
    p.mass, p.max_thrust = float(quad.mass), float(quad.max_thrust)
    p.g = float(np.asarray(quad.g, dtype=np.float64).reshape(-1)[-1])
    for i in range(3):
        p.J[i] = float(quad.J[i])
    for i in range(4):
        p.x_f[i], p.y_f[i], p.z_l_tau[i] = float(quad.x_f[i]), float(quad.y_f[i]), float(quad.z_l_tau[i])
    p.drag = 1 if getattr(quad, "drag", False) else 0
    p.rotor_drag[0] = p.rotor_drag[1] = float(getattr(quad, "rotor_drag_xy", 0.0))
    p.rotor_drag[2] = float(getattr(quad, "rotor_drag_z", 0.0))
    p.aero_drag, p.payload_mass = float(getattr(quad, "aero_drag", 0.0)), float(getattr(quad, "payload_mass", 0.0))
    p.u_min, p.u_max = float(getattr(quad, "min_input_value", 0.0)), float(getattr(quad, "max_input_value", 1.0))
    return p
