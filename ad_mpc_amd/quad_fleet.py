"""A fleet of quadrotors in closed loop on the device (include/admpc_quad_fleet.h): the loop of the reference's
``experiments/trajectory_test.py`` -- slide a window over an over-sampled reference trajectory, one RTI step, apply the first input to the
simplified simulator for ``control_period / simulation_dt`` sub-steps -- for B vehicles, T steps per call, with a tally of the tracking
error.  Built on ``QuadBatchSolver``; the OCP is shaped as ``Quad3DOptimizer`` shapes it (weight expansion for the quaternion, the
vehicle's constants, the linear drag, one cluster of residual GPs).  With ``learn`` the fleet fits those GPs itself, on the device, from
the steps it has flown (include/admpc_quad_learn.h: observe -> bin -> fit -> install; the side it shares with the car's fleet is
learning.py's), and searches their hyperparameters there (include/admpc_quad_hyper.h: ``search_gp`` -> re-fit -> install, ``learned_hyper``; learning.py's
as well).  With ``noise_seed`` and a vehicle whose ``noisy`` or ``motor_noise`` is set, the plant is the simulator under its random
disturbances (include/admpc_quad_noise.h).  With ``set_targets`` the fleet flies the reference's other experiment,
``experiments/point_tracking_and_record.py``: every vehicle chases random target points, reached within a threshold that is tested after
every simulator sub-step, and is recorded over the time it really flew (include/admpc_quad_targets.h).  ``generate_trajectories`` makes the
reference's loop and lemniscate trajectories on the device (include/admpc_quad_traj.h), ``generate_random_trajectories`` and
``generate_polynomial_trajectories`` its random and any other trajectories through keyframes (include/admpc_quad_poly_traj.h);
``set_trajectories`` uploads any others."""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .engine import QuadBatchSolver, _ptr
from .learning import FleetLearning, FleetSearch, placeholder_gps
from .quad_config import (QNX, QNU, QNY, QUAD_GP_MAX, QUAD_REC, AdmpcQuadObserveParams, default_quad_config, quad_is_noisy, quad_learn_bins,
                          quad_noise_params, quad_plant_params, quad_poly_traj_args, quad_target_params, quad_traj_specs, set_quad_gp)
from .quad_keyframes import random_keyframes

QuadRollout = namedtuple("QuadRollout", ("x", "idx", "tally", "counts", "traj", "u"))
QuadTargetRollout = namedtuple("QuadTargetRollout", ("x", "target", "target_no", "tcounts", "traj", "u", "nsub", "targets"))
START_STATE = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)      # point_tracking_and_record.py:115
T_MAX = 4096


def fleet_quad_config(quad=None, t_horizon=1.0, n_nodes=10, q_cost=None, r_cost=None, gp_regressors=None, rdrv_d_mat=None):
    """The AdmpcQuadConfig ``Quad3DOptimizer`` builds from the same arguments (quad_3d_optimizer.py:29-207), SQP_RTI."""
    from .quad_3d_optimizer import QuadGPEnsemble
    if q_cost is None:
        q_cost = np.array([10, 10, 10, 0.1, 0.1, 0.1, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05])
    if r_cost is None:
        r_cost = np.array([0.1, 0.1, 0.1, 0.1])
    cfg = default_quad_config(N=int(n_nodes), t_horizon=float(t_horizon))
    q_cost = np.asarray(q_cost, dtype=np.float64)
    q_diagonal = np.concatenate((q_cost[:3], np.mean(q_cost[3:6])[np.newaxis], q_cost[3:]))       # :140-143
    for i in range(QNX):
        cfg.W[i], cfg.We[i] = float(q_diagonal[i]), 0.0
    for m in range(QNU):
        cfg.W[QNX + m] = float(np.asarray(r_cost)[m])
    if quad is not None:
        cfg.mass, cfg.max_thrust = float(quad.mass), float(quad.max_thrust)
        for i in range(3):
            cfg.J[i] = float(quad.J[i])
        for i in range(4):
            cfg.x_f[i], cfg.y_f[i], cfg.z_l_tau[i] = float(quad.x_f[i]), float(quad.y_f[i]), float(quad.z_l_tau[i])
        lo = getattr(quad, "min_u", getattr(quad, "min_input_value", 0.0)); hi = getattr(quad, "max_u", getattr(quad, "max_input_value", 1.0))
        for m in range(QNU):
            cfg.lbu[m], cfg.ubu[m] = float(lo), float(hi)
    if rdrv_d_mat is not None:
        d = np.asarray(rdrv_d_mat, dtype=np.float64)
        if d.shape != (3, 3) or np.abs(d - np.diag(np.diag(d))).max() != 0.0:
            raise ValueError("rdrv_d_mat must be a 3 x 3 diagonal matrix (quad_3d_optimizer.py:364-381)")
        for i in range(3):
            cfg.rdrv[i] = float(d[i, i])
    if gp_regressors is not None:
        if isinstance(gp_regressors, QuadGPEnsemble):
            if gp_regressors.n_models > 1:
                raise NotImplementedError("clustered GP ensembles are not served by this rollout (one handle drives the whole fleet): "
                                          "QuadEnsembleFleet (quad_ensemble_fleet.py) flies and learns them")
            gp_regressors = gp_regressors.clusters[0]
        set_quad_gp(cfg, list(gp_regressors))
    return cfg


def fleet_solver_type(who, solver_type, n_nodes, sqp, offered=("SQP_RTI", "SQP")):
    """The checks of a fleet's ``solver_type`` and ``sqp`` that come before a handle exists; returns (qp_max, tol) for "SQP", else None."""
    if solver_type not in ("SQP_RTI", "SQP"):
        raise ValueError('%s: solver_type must be "SQP_RTI" or "SQP" (quad_3d_optimizer.py:203), got %r' % (who, solver_type))
    if solver_type not in offered:
        raise ValueError('%s: solver_type "SQP" is not served for clustered GP ensembles (include/admpc_quad_sqp.h: routed solves)' % who)
    if solver_type == "SQP_RTI":
        return None
    if int(n_nodes) > 16:
        raise ValueError('%s: solver_type "SQP" is served up to n_nodes = 16 (include/admpc_quad_sqp.h), got %d' % (who, int(n_nodes)))
    qp_max, tol = sqp
    if not 2 <= int(qp_max) <= 10000 or not float(tol) >= 0.0:
        raise ValueError("%s: sqp must be (qp_max in [2, 10000], tol >= 0)" % who)
    return int(qp_max), float(tol)


class QuadFleet(FleetLearning):
    """B quadrotors, each on one of K reference trajectories.  State on the device: ``x`` [B,13], ``idx`` [B] int32 (the sliding index),
    ``traj_of`` [B] int32, the persistent never-shifted iterate ``x_opt`` [B,N+1,13] / ``w_opt`` [B,N,4], the window ``yref`` / ``yref_e``,
    ``cost`` / ``status`` / ``iters`` of the last step, ``tally`` [B,3] (sum |e|, sum |e|^2, max |e|) and ``counts`` [B,3] int32 (steps,
    steps with status != 0, steps with a replaced activation).

    ``learn``: a list of regressors to learn (quad_config.quad_learn_bins: feat in 7 .. 16, out in 7 .. 9, lo, hi, bins, length_scale,
    sigma_f, noise, count_noise).  With it the controller's handle is created with placeholder GPs of no points, which fit_gp overwrites
    on the device; a second, nominal handle (no GP, same vehicle, same rdrv) predicts for observe; the observation's period is the
    control period, predicted in ``observe_substeps`` RK4 steps.  ``samples`` [B,14], ``bins`` [3,32,5] and ``dropped`` [4] are the
    record, the statistics and the counts of include/admpc_quad_learn.h.  Such a fleet is created as a ``QuadLearningFleet`` (below),
    which adds ``search_gp`` and ``learned_hyper`` (include/admpc_quad_hyper.h).

    ``noise_seed``: the key of the disturbances' generator.  With it and a quad whose ``noisy`` or ``motor_noise`` is set, ``plant_step``
    and ``rollout``, observed or not, go through the entries of include/admpc_quad_noise.h, and ``noise_step`` [B] int64 holds every
    vehicle's period counter (zeros at first; the 64 bits are the header's uint64).  A quad without disturbances ignores the seed; a quad
    with them and no seed is refused.

    ``solver_type``: "SQP_RTI" (one QP per period) or "SQP", the setting of the reference's point-tracking controllers: up to
    ``sqp[0]`` QPs per period, every vehicle until acados' stopping test passes at ``sqp[1]``, inside the solve kernel
    (include/admpc_quad_sqp.h; n_nodes <= 16).  It is set on the controller's handle, not on the nominal observer; ``counts[:, 1]`` and
    ``tcounts[:, 3]`` then count the periods that ended at the limit of QPs (status 2) as well.  ``terminal_cost``: the terminal weights
    are the stage weights of the state (quad_3d_optimizer.py:84), whatever the solver type."""
    _FIT, _INSTALL, _GP_CAP, _REC, _EMPTY, _NOUN = "admpc_quad_gp_fit", "admpc_quad_gp_install", QUAD_GP_MAX, QUAD_REC, 7, "fleet"

    def __new__(cls, *args, **kw):
        """``QuadFleet(..., learn=[...])`` creates a ``QuadLearningFleet``, the fleet with ``search_gp`` and ``learned_hyper``; every
        other class is created as it is asked for."""
        learn = kw.get("learn", args[11] if len(args) > 11 else None)
        return object.__new__(QuadLearningFleet if cls is QuadFleet and learn is not None else cls)

    def __init__(self, B, quad=None, t_horizon=1.0, n_nodes=10, q_cost=None, r_cost=None, simulation_dt=5e-4, reference_over_sampling=5,
                 gp_regressors=None, rdrv_d_mat=None, device=0, learn=None, observe_substeps=1, noise_seed=None, solver_type="SQP_RTI",
                 terminal_cost=False, sqp=(100, 1e-6)):
        sqp = fleet_solver_type("QuadFleet", solver_type, n_nodes, sqp)
        self._init_plant(B, quad, t_horizon, n_nodes, simulation_dt, reference_over_sampling, noise_seed)
        if learn is not None:                                                              # every refusal before a handle exists
            learn = [dict(d) for d in learn]
            bins, n_gp = quad_learn_bins(learn)                                            # ValueError on bad bins
            if gp_regressors is not None:
                raise ValueError("QuadFleet: learn and gp_regressors exclude each other: a fleet that learns starts from placeholder GPs")
            if not 1 <= int(observe_substeps) <= 64:
                raise ValueError("QuadFleet: observe_substeps must be in [1, 64]")
        cfg = fleet_quad_config(quad, t_horizon, n_nodes, q_cost, r_cost, gp_regressors, rdrv_d_mat)
        if terminal_cost:
            for i in range(QNX):
                cfg.We[i] = cfg.W[i]
        if learn is not None:
            self._nominal = QuadBatchSolver(cfg, device=device)
            cfg = set_quad_gp(cfg.copy(), placeholder_gps(learn))
        self._eng = QuadBatchSolver(cfg, device=device)
        self.solver_type = solver_type
        if sqp is not None:
            self._eng.set_sqp(*sqp)
        self._alloc_state([self._eng])
        if learn is not None:
            obs = AdmpcQuadObserveParams(dt=self.control_period, substeps=int(observe_substeps), n_gp=n_gp, gp=bins)
            self._alloc_learning(learn, n_gp, obs, (self.B, QNX))

    def _init_plant(self, B, quad, t_horizon, n_nodes, simulation_dt, reference_over_sampling, noise_seed):
        """The sizes, the simulator's vehicle and its disturbances: everything here is refused before a handle exists."""
        self.B, self.N, self.over = int(B), int(n_nodes), int(reference_over_sampling)
        if self.B < 1 or self.over < 1:
            raise ValueError("QuadFleet: B and reference_over_sampling must be at least 1")
        self.control_period = float(t_horizon) / (self.N * self.over)                      # trajectory_test.py: t_horizon / (n_mpc_nodes * over)
        flies_noise = quad_is_noisy(quad) and noise_seed is not None
        self._plant = quad_plant_params(quad, simulation_dt, self.control_period, allow_noise=flies_noise)    # refuses noisy / motor_noise without a seed before a handle exists
        self._noise = quad_noise_params(quad, simulation_dt, noise_seed) if flies_noise else None
        self.noise_step = None
        self._learn = self._nominal = None
        self._tp, self._targets_started = None, False

    def _alloc_state(self, engines):
        """The fleet's tensors on the device of ``_eng``, and one eager solve on every handle that will solve in the loop."""
        self.lib, self.device, self.device_index, self.cfg = self._eng.lib, self._eng.device, self._eng.device_index, self._eng.cfg
        self._bank, self._M = None, None
        B, N, dev = self.B, self.N, self.device
        f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
        self.x, self.x_opt, self.w_opt = f64(B, QNX), f64(B, N + 1, QNX), f64(B, N, QNU)
        self.yref, self.yref_e = f64(B, N, QNY), f64(B, QNX)
        self.cost, self.status, self.iters = f64(B), i32(B), i32(B)
        self.tally, self.counts = f64(B, 3), i32(B, 3)
        self.traj_of, self.idx = i32(B), i32(B)
        if self._noise is not None:
            self.noise_step = torch.zeros(B, dtype=torch.int64, device=dev)
        # one eager solve: the N = 20 handle allocates its slot buffer at its first solve, so a later graph capture of rollout() is legal
        self.x[:, 3] = 1.0
        self.yref[:, :, 3] = 1.0; self.yref_e[:, 3] = 1.0
        for eng in engines:
            eng.solve(self.x, self.yref, self.yref_e, f64(B, N + 1, QNX), f64(B, N, QNU))
        torch.cuda.synchronize(dev)

    # -- lifetime ---------------------------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_bank", None):
            self.lib.admpc_quad_traj_bank_destroy(self._bank)
            self._bank = None
        if getattr(self, "_eng", None):
            self._eng.close()
        if getattr(self, "_nominal", None):
            self._nominal.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return self._eng._stream()

    # -- the references ---------------------------------------------------------------------------------------------------------------
    def set_trajectories(self, trajectories):
        """[(traj [M,13], u [M,4]), ...]: the over-sampled reference trajectories (one row per control period) and their inputs."""
        tr = [(np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)) for t, u in trajectories]
        if not tr:
            raise ValueError("set_trajectories: at least one trajectory")
        for t, u in tr:
            if t.ndim != 2 or t.shape[1] != QNX or u.shape != (t.shape[0], QNU) or t.shape[0] < 1:
                raise ValueError("set_trajectories: every trajectory is (traj [M,13], u [M,4]) with M >= 1")
        K = len(tr)
        M = (C.c_int32 * K)(*[t.shape[0] for t, _ in tr])
        tp = (C.c_void_p * K)(*[t.ctypes.data for t, _ in tr])
        up = (C.c_void_p * K)(*[u.ctypes.data for _, u in tr])
        h = C.c_void_p(0)
        _lib.check(self.lib.admpc_quad_traj_bank_create(self.device_index, K, M, tp, up, C.byref(h)))
        if self._bank:
            torch.cuda.synchronize(self.device)
            self.lib.admpc_quad_traj_bank_destroy(self._bank)
        self._bank, self._M, self._traj = h, np.array([t.shape[0] for t, _ in tr]), tr

    def generate_trajectories(self, kind, v_max, radius=5.0, z=1.0, lin_acc=None, clockwise=True):
        """K reference trajectories generated on the device (admpc_quad_traj_bank_generate of include/admpc_quad_traj.h): the
        reference's ``loop_trajectory`` / ``lemniscate_trajectory`` (``kind`` "loop" or "lemniscate") that ramp to ``v_max`` and back,
        one row per control period, for this fleet's vehicle.  Every argument is a scalar or a length-K sequence; ``lin_acc=None`` is
        0.25 * v_max.  Replaces the bank as ``set_trajectories`` does; no host copy is kept (``trajectory(k)`` reads one back).  The
        generation is enqueued on the current stream: work enqueued on it later sees the finished bank."""
        specs = quad_traj_specs(kind, v_max, radius, z, lin_acc, clockwise)
        K = len(specs)
        h = C.c_void_p(0)
        _lib.check(self.lib.admpc_quad_traj_bank_generate(self.device_index, K, specs, C.byref(self._plant), self.control_period, self._stream(),
                                                          C.byref(h)))
        self._take_generated(h, K)

    def generate_polynomial_trajectories(self, keyframes, speed):
        """K reference trajectories through keyframes generated on the device (admpc_quad_poly_traj_bank_generate of
        include/admpc_quad_poly_traj.h): the piecewise degree-7 polynomial the reference's ``random_trajectory`` and
        ``straight_trajectory`` fit through their position keyframes, flown at the average ``speed``, one row per control period, for this
        fleet's vehicle.  ``keyframes`` [K,n_key,3] or [n_key,3] (3 <= n_key <= 32), ``speed`` a scalar or a length-K sequence.  Replaces the
        bank as ``generate_trajectories`` does: no host copy is kept, ``reset`` takes its start rows from the device, and the generation
        is enqueued on the current stream."""
        keys, sp = quad_poly_traj_args(keyframes, speed)
        K = keys.shape[0]
        dbl = C.POINTER(C.c_double)
        h = C.c_void_p(0)
        _lib.check(self.lib.admpc_quad_poly_traj_bank_generate(self.device_index, K, keys.shape[1], keys.ctypes.data_as(dbl), sp.ctypes.data_as(dbl),
                                                               C.byref(self._plant), self.control_period, self._stream(), C.byref(h)))
        self._take_generated(h, K)

    def generate_random_trajectories(self, seeds, speed):
        """The reference's ``random_trajectory(quad, control_period, seed, speed)`` (map_name=None) for every seed of ``seeds`` (a number or
        a sequence): ``random_keyframes(seed)`` on the host, then ``generate_polynomial_trajectories``."""
        seeds = np.atleast_1d(np.asarray(seeds))
        self.generate_polynomial_trajectories(np.stack([random_keyframes(int(sd)) for sd in seeds]), speed)

    def _take_generated(self, h, K):
        """The generated bank h of K trajectories replaces the fleet's bank; its lengths are read from the library."""
        if self._bank:
            torch.cuda.synchronize(self.device)
            self.lib.admpc_quad_traj_bank_destroy(self._bank)
        M = (C.c_int32 * K)()
        _lib.check(self.lib.admpc_quad_traj_bank_info(h, None, None, M))
        self._bank, self._M, self._traj = h, np.array(M[:], dtype=np.int64), None

    def trajectory(self, k):
        """(traj [M,13], u [M,4]) of trajectory k of the bank as numpy arrays (admpc_quad_traj_bank_copy).  Synchronises."""
        self._need_bank("trajectory")
        k = int(k)
        if not 0 <= k < len(self._M):
            raise ValueError("trajectory: k must be in [0, K)")
        M = int(self._M[k])
        traj, u = np.empty((M, QNX)), np.empty((M, QNU))
        dbl = C.POINTER(C.c_double)
        _lib.check(self.lib.admpc_quad_traj_bank_copy(self._bank, k, traj.ctypes.data_as(dbl), u.ctypes.data_as(dbl)))
        return traj, u

    def _need_bank(self, who):
        if not self._bank:
            raise ValueError("%s: call set_trajectories or generate_trajectories first" % who)

    def reset(self, traj_of, idx0=0, x0=None):
        """Vehicle b follows trajectory traj_of[b] from row idx0 (a number or [B]); it starts at x0 [B,13] or, as the reference does, at
        that row of its trajectory.  The iterate, the tally and the counts are zeroed.  ``noise_step`` is NOT touched: a fleet that is reset
        goes on drawing fresh disturbances; ``reseed`` starts the stream over."""
        self._need_bank("reset")
        tk = np.broadcast_to(np.asarray(traj_of, dtype=np.int64), (self.B,))
        i0 = np.broadcast_to(np.asarray(idx0, dtype=np.int64), (self.B,))
        if x0 is None:
            if (tk < 0).any() or (tk >= len(self._M)).any() or (i0 < 0).any() or (i0 >= self._M[tk]).any():
                raise ValueError("reset: x0 is needed for a vehicle whose traj_of or idx0 is out of range")
            if self._traj is not None:
                x0 = np.stack([self._traj[k][0][i] for k, i in zip(tk, i0)])
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            if x0.shape != (self.B, QNX):
                raise ValueError("reset: x0 must be [B,13]")
        self.traj_of.copy_(torch.as_tensor(tk.astype(np.int32)))
        self.idx.copy_(torch.as_tensor(i0.astype(np.int32)))
        if x0 is not None:
            self.x.copy_(torch.as_tensor(x0))
        else:                                                                              # a generated bank has no host copy
            _lib.check(self.lib.admpc_quad_traj_rows_batch(self._bank, self.B, _ptr(self.traj_of), _ptr(self.idx), _ptr(self.x), None,
                                                           self._stream()))
        for t in (self.x_opt, self.w_opt, self.tally, self.counts, self.cost, self.status, self.iters):
            t.zero_()

    def ref_chunk(self, pos_ref=None):
        """The window of every vehicle at its idx into yref / yref_e (admpc_quad_ref_chunk_batch); pos_ref [B,3] if given."""
        self._need_bank("ref_chunk")
        if pos_ref is not None:
            self._eng._chk(pos_ref, (self.B, 3))
        _lib.check(self.lib.admpc_quad_ref_chunk_batch(self._bank, self.B, self.N, self.over, _ptr(self.traj_of), _ptr(self.idx), _ptr(self.yref),
                                                       _ptr(self.yref_e), _ptr(pos_ref), self._stream()))

    # -- the plant --------------------------------------------------------------------------------------------------------------------
    def _u_stride(self, who, u, B):
        """The row stride of the activations u, a float64 [B,4] view with unit inner stride; a single row has no stride to speak of."""
        if u.dtype != torch.float64 or u.device != self.device or tuple(u.shape) != (B, QNU) or u.stride(1) != 1 or (B > 1 and u.stride(0) < QNU):
            raise ValueError("%s: u must be float64 [B,4] on the fleet's device with unit inner stride" % who)
        return u.stride(0) if B > 1 else QNU

    def plant_step(self, u, x=None):
        """One control period of the simulator under u [B,4] (or any float64 view with rows of 4 and a row stride, such as
        ``w_opt[:, 0, :]``), in place on x (default: the fleet's state)."""
        x = self.x if x is None else x
        self._eng._chk(x, (x.shape[0], QNX))
        Bx = x.shape[0]
        stride = self._u_stride("plant_step", u, Bx)
        if self._noise is not None:
            if Bx > self.B:
                raise ValueError("plant_step: under the disturbances x has at most the fleet's B rows (row b draws with noise_step[b])")
            _lib.check(self.lib.admpc_quad_plant_step_noise_batch(C.byref(self._plant), C.byref(self._noise), self.device_index, Bx,
                                                                  C.c_void_p(u.data_ptr()), stride, _ptr(x), _ptr(self.noise_step), self._stream()))
            return
        _lib.check(self.lib.admpc_quad_plant_step_batch(C.byref(self._plant), self.device_index, Bx, C.c_void_p(u.data_ptr()), stride, _ptr(x),
                                                        self._stream()))

    # -- the closed loop --------------------------------------------------------------------------------------------------------------
    def rollout(self, T, record=False, observe=False):
        """T closed-loop steps (admpc_quad_rollout_batch): no host synchronisation.  Returns QuadRollout(x, idx, tally, counts, traj, u):
        the fleet's own tensors, and with record traj [T+1,B,13] (slot t: the state at the start of step t) and u [T,B,4].  `observe`:
        every step is observed, as observe_latch before the first and observe behind each would (admpc_quad_rollout_observe_batch;
        needs ``learn``).  Under the disturbances both forms are admpc_quad_rollout_noise_batch, and noise_step advances by T."""
        self._need_bank("rollout")
        if observe:
            self._learns("rollout")
        T, traj, u = self._records("rollout", T, record)
        args = self._rollout_args(self._eng._h, T, traj, u)
        if self._noise is not None:
            watch = (self._observer._h, C.byref(self._obs), _ptr(self._prev), _ptr(self.samples), _ptr(self.bins), _ptr(self.dropped)) if observe \
                else (None,) * 6
            _lib.check(self.lib.admpc_quad_rollout_noise_batch(*args, *watch, C.byref(self._noise), _ptr(self.noise_step), self._stream()))
        elif observe:
            _lib.check(self.lib.admpc_quad_rollout_observe_batch(*args, self._observer._h, C.byref(self._obs), _ptr(self._prev), _ptr(self.samples),
                                                                 _ptr(self.bins), _ptr(self.dropped), self._stream()))
        else:
            _lib.check(self.lib.admpc_quad_rollout_batch(*args, self._stream()))
        return QuadRollout(self.x, self.idx, self.tally, self.counts, traj, u)

    def _rollout_args(self, solver, T, traj, u):
        """The arguments every rollout entry shares, admpc_quad_rollout_batch's up to u_out."""
        return (solver, self._bank, C.byref(self._plant), self.over, self.B, T, _ptr(self.traj_of), _ptr(self.idx), _ptr(self.x),
                _ptr(self.x_opt), _ptr(self.w_opt), _ptr(self.yref), _ptr(self.yref_e), _ptr(self.cost), _ptr(self.status), _ptr(self.iters),
                _ptr(self.tally), _ptr(self.counts), _ptr(traj), _ptr(u))

    def _records(self, who, T, record):
        """T checked, and with record the tensors traj [T+1,B,13] and u [T,B,4] (else None, None)."""
        T = int(T)
        if T < 0 or T > T_MAX:
            raise ValueError("%s: T must be in [0, %d]" % (who, T_MAX))
        traj = u = None
        if record:
            traj = torch.empty((T + 1, self.B, QNX), dtype=torch.float64, device=self.device)
            u = torch.empty((T, self.B, QNU), dtype=torch.float64, device=self.device)
            if T == 0:
                traj[0].copy_(self.x)
        return T, traj, u

    def step(self):
        """One closed-loop step."""
        return self.rollout(1)

    # -- flying to targets (include/admpc_quad_targets.h) --------------------------------------------------------------------------------
    def _targets_offered(self, who):
        """A fleet that cannot chase targets says so here."""

    def _chases(self, who, started=True):
        self._targets_offered(who)
        if self._tp is None:
            raise ValueError("%s: call set_targets first" % who)
        if started and not self._targets_started:
            raise ValueError("%s: call reset_targets first" % who)

    def set_targets(self, mode="aggressive", world_radius=3.0, thresh=0.05, v_max=14.0, max_iters=100, seed=None, presets=None):
        """How the fleet chases targets (point_tracking_and_record.py; the defaults are the reference's): ``mode`` "aggressive" (the next
        target is sampled away from where the vehicle stands), "uniform" (in the world box) or "preset" (``presets`` [n,3] for all
        vehicles or [B,n,3]); a target counts as reached within ``thresh``; a vehicle with a velocity component above ``v_max`` or more
        than ``max_iters`` periods on one target is put back on its target.  ``seed`` is the key of the targets' generator, needed by
        the two random modes.  Every refusal is a ValueError, raised before any device call.  State: ``target`` [B,3], ``target_no`` [B]
        int64 (the 64 bits are the header's uint64), ``n_iter`` [B], ``fast`` [B], ``tcounts`` [B,5] (targets reached, recoveries,
        periods flown, periods with status != 0, periods with a replaced activation) and ``nsub`` [B] (the sub-steps of the last
        period).  ``reset_targets`` starts the flight."""
        self._targets_offered("set_targets")
        pre, n_preset = None, 0
        if mode == "preset":
            if presets is None:
                raise ValueError("set_targets: mode 'preset' needs presets [n,3] or [B,n,3]")
            pre = np.asarray(presets, dtype=np.float64)
            if pre.ndim == 2:
                pre = np.broadcast_to(pre, (self.B,) + pre.shape)
            if pre.ndim != 3 or pre.shape[0] != self.B or pre.shape[1] < 1 or pre.shape[2] != 3:
                raise ValueError("set_targets: presets must be [n,3] or [B,n,3] with n >= 1")
            pre, n_preset = np.ascontiguousarray(pre), pre.shape[1]
        elif presets is not None:
            raise ValueError("set_targets: presets come with mode 'preset'")
        tp = quad_target_params(mode, world_radius, thresh, v_max, max_iters, seed, n_preset)
        z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device=self.device)
        self.target, self.target_no = z(self.B, 3, dtype=torch.float64), z(self.B, dtype=torch.int64)
        self.n_iter, self.fast, self.tcounts, self.nsub = z(self.B), z(self.B), z(self.B, 5), z(self.B)
        self._presets = None if pre is None else torch.as_tensor(pre).to(self.device)
        self._tp, self._targets_started = tp, False

    def reset_targets(self, x0=None):
        """The fleet starts at x0 [B,13] or [13] (default: the reference's start state, level at the origin); the iterate and the
        targets' counters are zeroed, ``fast`` is taken from x0 and target number 0 is installed (admpc_quad_targets_reset_batch).
        ``noise_step`` is NOT touched, as in ``reset``."""
        self._chases("reset_targets", started=False)
        x0 = np.asarray(START_STATE if x0 is None else x0, dtype=np.float64)
        if x0.shape not in ((QNX,), (self.B, QNX)):
            raise ValueError("reset_targets: x0 must be [13] or [B,13]")
        self.x.copy_(torch.as_tensor(np.broadcast_to(x0, (self.B, QNX)).copy()))
        for t in (self.x_opt, self.w_opt, self.cost, self.status, self.iters):
            t.zero_()
        _lib.check(self.lib.admpc_quad_targets_reset_batch(C.byref(self._tp), self.device_index, self.B, _ptr(self.x), _ptr(self._presets),
                                                           _ptr(self.target), _ptr(self.target_no), _ptr(self.n_iter), _ptr(self.fast),
                                                           _ptr(self.tcounts), self._stream()))
        self._targets_started = True

    def target_window(self):
        """The recovery of every vehicle that has run away, then the point reference of every vehicle into yref / yref_e
        (admpc_quad_target_window_batch).  A fleet that learns has the recovered state latched for its next observation."""
        self._chases("target_window")
        prev = self._prev if self._learn is not None else None
        _lib.check(self.lib.admpc_quad_target_window_batch(C.byref(self._tp), self.device_index, self.B, self.N, _ptr(self.x), _ptr(self.target),
                                                           _ptr(self.target_no), _ptr(self.n_iter), _ptr(self.fast), _ptr(self.tcounts),
                                                           _ptr(prev), _ptr(self.yref), _ptr(self.yref_e), self._stream()))

    def plant_step_targets(self, u=None):
        """One control period of the simulator towards the targets, stopped for a vehicle at the sub-step at which it reaches
        (admpc_quad_plant_target_step_batch): ``nsub``, the counters, ``fast`` and, at a reach, the next target in the same launch.
        u [B,4] (a float64 view with rows of 4 and a row stride); default ``w_opt[:, 0, :]``, and then ``status`` of the solve that left
        it is counted in ``tcounts``.  Under the disturbances ``noise_step`` advances by 1."""
        self._chases("plant_step_targets")
        status = self.status if u is None else None
        u = self.w_opt[:, 0, :] if u is None else u
        stride = self._u_stride("plant_step_targets", u, self.B)
        noise = None if self._noise is None else C.byref(self._noise)
        _lib.check(self.lib.admpc_quad_plant_target_step_batch(C.byref(self._plant), C.byref(self._tp), noise, self.device_index, self.B,
                                                               C.c_void_p(u.data_ptr()), stride, _ptr(self.x), _ptr(status), _ptr(self._presets),
                                                               _ptr(self.target), _ptr(self.target_no), _ptr(self.n_iter), _ptr(self.fast),
                                                               _ptr(self.tcounts), _ptr(self.nsub), _ptr(self.noise_step), self._stream()))

    def observe_targets(self, u=None):
        """``observe`` over the time every vehicle really flew in the last period, ``nsub`` sub-steps (admpc_quad_observe_var_batch)."""
        self._chases("observe_targets")
        self._learns("observe_targets")
        u = self.w_opt[:, 0, :] if u is None else u
        stride = self._u_stride("observe_targets", u, self.B)
        _lib.check(self.lib.admpc_quad_observe_var_batch(self._observer._h, C.byref(self._plant), C.byref(self._obs), self.B, C.c_void_p(u.data_ptr()),
                                                         stride, _ptr(self.x), _ptr(self._prev), _ptr(self.nsub), _ptr(self.samples),
                                                         _ptr(self.bins), _ptr(self.dropped), self._stream()))

    def rollout_targets(self, T, record=False, observe=False):
        """T periods of the target flight (admpc_quad_rollout_targets_batch): recovery and window -> RTI step -> plant with the reach test,
        and with `observe` (needs ``learn``) a latch first and the observation of the flown time behind every period.  No host
        synchronisation.  Returns QuadTargetRollout(x, target, target_no, tcounts, traj, u, nsub, targets): the fleet's own tensors, and
        with record traj [T+1,B,13], u [T,B,4], nsub [T,B] int32 and targets [T,B,3] (the target in force during the period)."""
        self._chases("rollout_targets")
        if observe:
            self._learns("rollout_targets")
        T, traj, u = self._records("rollout_targets", T, record)
        nsub = targets = None
        if record:
            nsub = torch.empty((T, self.B), dtype=torch.int32, device=self.device)
            targets = torch.empty((T, self.B, 3), dtype=torch.float64, device=self.device)
        watch = (self._observer._h, C.byref(self._obs), _ptr(self._prev), _ptr(self.samples), _ptr(self.bins), _ptr(self.dropped)) if observe \
            else (None,) * 6
        noise = None if self._noise is None else C.byref(self._noise)
        _lib.check(self.lib.admpc_quad_rollout_targets_batch(
            self._eng._h, C.byref(self._plant), C.byref(self._tp), self.B, T, _ptr(self.x), _ptr(self.x_opt), _ptr(self.w_opt), _ptr(self.yref),
            _ptr(self.yref_e), _ptr(self.cost), _ptr(self.status), _ptr(self.iters), _ptr(self._presets), _ptr(self.target), _ptr(self.target_no),
            _ptr(self.n_iter), _ptr(self.fast), _ptr(self.tcounts), _ptr(self.nsub), _ptr(traj), _ptr(u), _ptr(nsub), _ptr(targets), *watch,
            noise, _ptr(self.noise_step), self._stream()))
        return QuadTargetRollout(self.x, self.target, self.target_no, self.tcounts, traj, u, nsub, targets)

    # -- the disturbances (include/admpc_quad_noise.h) ---------------------------------------------------------------------------------
    def _noisy(self, who):
        if self._noise is None:
            raise ValueError("%s: this fleet flies the deterministic simulator (a quad with noisy or motor_noise and a noise_seed make it noisy)" % who)

    def reseed(self, seed=None, step=0):
        """Sets the generator's key (None: keeps it) and fills ``noise_step`` with ``step`` (a number or [B]): the same call sequence
        after the same reseed draws the same numbers.  The fill is asynchronous on the current stream; the key is read at each call, so a
        captured graph keeps the key it was captured with."""
        self._noisy("reseed")
        if seed is not None:
            if not 0 <= int(seed) < 2 ** 64:
                raise ValueError("reseed: seed must be in [0, 2^64)")
            self._noise.seed = int(seed)
        self.noise_step.copy_(torch.as_tensor(np.broadcast_to(np.asarray(step, dtype=np.int64), (self.B,)).copy()))

    def noise_draws(self, substeps=None):
        """z [B, substeps, 10] on the host: the ten standard normals of every sub-step of the period the fleet flies NEXT
        (admpc_quad_noise_draw_batch; ``substeps`` defaults to the plant's).  ``noise_step`` is not advanced.  Synchronises."""
        self._noisy("noise_draws")
        S = int(self._plant.substeps if substeps is None else substeps)
        if not 1 <= S <= 1024:
            raise ValueError("noise_draws: substeps must be in [1, 1024]")
        z = torch.empty((self.B, S, 10), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.admpc_quad_noise_draw_batch(C.byref(self._noise), self.device_index, self.B, S, _ptr(self.noise_step), _ptr(z), None,
                                                        self._stream()))
        return z.cpu().numpy()

    def tracking_rmse(self):
        """trajectory_test.py:137's figure per vehicle: the mean of the position error norms over the steps taken (tally[:, 0] / steps);
        NaN for a vehicle that has taken no step.  A device tensor [B]."""
        return self.tally[:, 0] / self.counts[:, 0].to(torch.float64)

    # -- learning the body-frame residual GPs (include/admpc_quad_learn.h): what the quadrotor adds to learning.py's FleetLearning ------
    def observe_latch(self):
        """Takes the fleet's state as the one the next observe will predict from.  Asynchronous on the current stream."""
        self._learns("observe_latch")
        _lib.check(self.lib.admpc_quad_observe_latch_batch(self.device_index, self.B, _ptr(self.x), _ptr(self._prev), self._stream()))

    def observe(self, u=None):
        """The fleet's state one control period after the latched one, under the activations u [B,4] (a float64 view with rows of 4 and
        a row stride; default ``w_opt[:, 0, :]``, what the rollout's plant applies): what the observer's model did not predict of the
        body-frame velocity, per second, goes into ``samples`` and from there into ``bins`` and ``dropped``; the state is latched for the
        next call.  Asynchronous on the current stream."""
        self._learns("observe")
        u = self.w_opt[:, 0, :] if u is None else u
        stride = self._u_stride("observe", u, self.B)
        _lib.check(self.lib.admpc_quad_observe_batch(self._observer._h, C.byref(self._plant), C.byref(self._obs), self.B, C.c_void_p(u.data_ptr()),
                                                     stride, _ptr(self.x), _ptr(self._prev), _ptr(self.samples), _ptr(self.bins),
                                                     _ptr(self.dropped), self._stream()))


class QuadLearningFleet(FleetSearch, QuadFleet):
    """What ``QuadFleet(..., learn=[...])`` creates: the fleet that learns, with the search of the hyperparameters of its residual GPs
    on the device (include/admpc_quad_hyper.h; learning.py's ``FleetSearch``, which the car's controller shares): ``search_gp(min_count,
    grid, rounds, shrink, bounds, resume, install)`` -> re-fit -> install and ``learned_hyper()``, with the car's signatures and return
    values; ``hyper`` [3,16] and ``search_info`` [3,2] are the search's state.  ``learned_gps()`` reports the found length scales and
    sigma_f after a search, the given ones again after a later ``fit_gp``."""
    _SEARCH, _REFIT = "admpc_quad_gp_search", "admpc_quad_gp_refit"
