"""The control step of a fleet: pose in, Ackermann command out, for B vehicles on one global path
(include/admpc.h: admpc_control_step_batch; csrc/admpc_step.hip), or with a path per vehicle out of a bank of paths and the best of
every group of candidates (include/admpc_fleet.h: admpc_control_step_bank_batch, admpc_argmin_groups), or along a route of that bank,
wherever on it the vehicle is (include/admpc_lane.h: admpc_control_step_lane_batch), or closes the loop on the device: a plant step under
the record just issued, and T steps of controller and plant per call (include/admpc_plant.h: admpc_plant_step_batch,
admpc_rollout_lane_batch), or learns the residual GP of its model from the steps it has taken, on the device (include/admpc_learn.h:
observe -> bin -> fit -> install; the side it shares with the quadrotor's fleet is learning.py's), and searches the hyperparameters of
that GP on the device (include/admpc_hyper.h: search -> re-fit -> install; search_gp and learned_hyper are learning.py's too).

``FleetController`` solves the problem of ``ROSGPMPC(point_reference=False)`` (create_ros_ad_mpc.py:41-101: SQP_RTI, Q_DIAG_ROS /
R_DIAG_ROS) for every vehicle, and does per step what the reference node does per pose message (gp_ad_mpc_node.py:389-438 ->
run_mpc :160-230): reference window, speed clamp, the padded references, the solve, the validity test, the fallback command of
run_optimization, the Ackermann record and the node's gate.  Everything runs on the device as one chain of launches on the current
stream; the per-vehicle state the node carries from call to call (the iterate, safe_count, the previous valid inputs) lives in device
tensors of this object.

One deliberate deviation: the node clamps the speed of the GLOBAL path once per waypoint message, at the speed the vehicle had then
(:351-368).  Vehicles at different speeds cannot share that, so each step clamps each vehicle's local window at its current speed
(admpc_resample_vel_batch); ``resample=False`` turns the clamp off.  ``step_route`` does not deviate here: it cuts a local lane per
vehicle out of the route, as the node's waypoint message carries one, and clamps that lane as the node does.
"""
import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import config as _c
from .ad_3d import AD3D
from .ad_3d_optimizer import ocp_config
from .config import AdmpcLaneParams, AdmpcObserveParams, AdmpcPath, AdmpcPlantParams, AdmpcStepParams, GP_MAX, NX, NU
from .engine import BatchSolver, _ptr
from .learning import FleetSearch, placeholder_gps
from .ref_traj import RefTrajectory

SAFE_COUNT_THRESHOLD = 10          # consecutive successes before the node issues an MPC command (gp_ad_mpc_node.py:62)


class FleetStep(NamedTuple):
    """Device tensors of one step; they are the controller's own buffers and are overwritten by the next step."""
    ack: torch.Tensor          # float32 [B,4]: steering_angle, steering_angle_velocity, speed, acceleration
    mode: torch.Tensor         # int32 [B]: 1 = MPC command, 0 = the auxiliary controller's brake record
    status: torch.Tensor       # int32 [B]: acados status of the solve (0 success, 4 failure)
    valid: torch.Tensor        # int32 [B]: is_valid_command of the prediction against the padded target
    x_opt: torch.Tensor        # float64 [B,N+1,7]: the iterate (view of the controller's state)
    w_opt: torch.Tensor        # float64 [B,N,2]


class FleetPathStep(NamedTuple):
    """FleetStep of a step against the bank of paths (step_paths), with the objective of every solve."""
    ack: torch.Tensor
    mode: torch.Tensor
    status: torch.Tensor
    valid: torch.Tensor
    x_opt: torch.Tensor
    w_opt: torch.Tensor
    cost: torch.Tensor         # float64 [B]: objective of the solve; +inf where status != 0 or valid == 0 (NOT where mode == 0: admpc_fleet.h)


class FleetLaneStep(NamedTuple):
    """FleetPathStep of a step along a route (step_route), with the waypoint at which every vehicle's lane began."""
    ack: torch.Tensor
    mode: torch.Tensor
    status: torch.Tensor
    valid: torch.Tensor
    x_opt: torch.Tensor
    w_opt: torch.Tensor
    cost: torch.Tensor
    lane_idx: torch.Tensor     # int32 [B]: the nearest waypoint of the route, where the lane was cut; the next step searches around it


class FleetRollout(NamedTuple):
    """FleetLaneStep of the last step of a rollout (rollout_route), with what the closed loop did over its steps."""
    ack: torch.Tensor
    mode: torch.Tensor
    status: torch.Tensor
    valid: torch.Tensor
    x_opt: torch.Tensor
    w_opt: torch.Tensor
    cost: torch.Tensor
    lane_idx: torch.Tensor
    tally: torch.Tensor        # float64 [B,3]: sum of e_y^2, sum of e_psi^2, max |e_y| over the steps (the generator's tracking errors)
    counts: torch.Tensor       # int32 [B,3]: steps taken, steps with an MPC command, unusable steps (status != 0 or valid == 0)
    traj: torch.Tensor         # float64 [steps+1,7,B] or None: the poses at the start of every step, and the final ones


class FleetController(FleetSearch):
    _FIT, _INSTALL, _GP_CAP, _REC, _EMPTY, _NOUN = "admpc_gp_fit", "admpc_gp_install", GP_MAX, 10, 3, "controller"
    _SEARCH, _REFIT = "admpc_gp_search", "admpc_gp_refit"

    def __init__(self, t_horizon, n_mpc_nodes, opt_dt, B, device=0, resample=True, threshold=SAFE_COUNT_THRESHOLD, blend_min=None,
                 blend_max=None, learn=None):
        """``blend_min`` / ``blend_max`` (None: the vehicle's, ad_3d.py) are the ends of the speed band of vel_switch.  ``learn``: a list
        of regressors to learn (config.learn_bins: feat, out, lo, hi, bins, length_scale, sigma_f, noise, count_noise).  With it the
        engine is created with placeholder GPs of no points, which fit_gp overwrites on the device; a second, nominal engine (no GP, same
        vehicle) predicts for observe.  At N = 40 a controller that learns runs kernel R where one that does not runs kernel S
        (include/admpc_learn.h)."""
        N, B = int(n_mpc_nodes), int(B)
        if B < 1:
            raise ValueError("B must be positive")
        self.ad = ad = AD3D(noisy=False, noisy_input=False)            # create_ros_ad_mpc.py:26-38
        if blend_min is not None:
            ad.blend_min = float(blend_min)
        if blend_max is not None:
            ad.blend_max = float(blend_max)
        cfg = ocp_config(ad, t_horizon, N, np.array(_c.Q_DIAG_ROS), np.array(_c.R_DIAG_ROS), "SQP_RTI")
        self._learn = None
        if learn is not None:
            learn = [dict(d) for d in learn]
            bins, n_gp = _c.learn_bins(learn)                            # ValueError on bad bins, before anything is created
            self._nominal = BatchSolver(cfg, device=device)
            cfg = _c.set_gp(cfg.copy(), placeholder_gps(learn))
        self._eng = eng = BatchSolver(cfg, device=device)
        self.lib, self.device = eng.lib, eng.device
        self.N, self.B, self.opt_dt = N, B, opt_dt
        dt = float(t_horizon) / N                                         # traj_dt and the clamp's dt (gp_ad_mpc_node.py:55, :95)
        self._ref = RefTrajectory(traj_horizon=N, traj_dt=dt, device=device)
        self._path = AdmpcPath(M=0, H=N, dt=dt)
        self._prm = AdmpcStepParams(blend_min=ad.blend_min, blend_max=ad.blend_max, acc_max=ad.acc_max, resample_dt=dt,
                                    resample=1 if resample else 0, threshold=int(threshold))
        _lib.check(self.lib.admpc_reserve(eng._h, B))                     # every later step is allocation-free (graph capture)
        nbytes = C.c_size_t(0)
        _lib.check(self.lib.admpc_control_step_workspace(eng._h, B, C.byref(nbytes)))
        z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=self.device)
        self._work = z(-(-nbytes.value // 8))
        self.x_opt, self.w_opt = z(B, N + 1, NX), z(B, N, NU)            # the iterate: all zeros, as a fresh solver's
        self.safe_count = z(B, dtype=torch.int32)
        self.prev_u, self.has_valid = z(B, N, NU), z(B, dtype=torch.int32)
        self.ack = z(B, 4, dtype=torch.float32)
        self.mode, self.valid, self.status = z(B, dtype=torch.int32), z(B, dtype=torch.int32), z(B, dtype=torch.int32)
        self.cost = z(B)                                                  # step_paths; best_of reduces it into the two below
        self._best_val, self._best_idx = z(B), z(B, dtype=torch.int64)
        self.lane_idx = torch.full((B,), -1, dtype=torch.int32, device=self.device)      # step_route; -1: search the whole route
        self._bank, self._stepped_paths, self.n_paths = None, False, 0
        self.tally, self.counts = z(B, 3), z(B, 3, dtype=torch.int32)    # rollout_route
        self._plant_model = None
        self.set_plant()
        if learn is not None:
            obs = AdmpcObserveParams(dt=0.0, blend_min=ad.blend_min, blend_max=ad.blend_max, substeps=1, n_gp=n_gp, gp=bins)
            self._alloc_learning(learn, n_gp, obs, (NX, B))

    def _drop_bank(self):
        if getattr(self, "_bank", None):
            self.lib.admpc_path_bank_destroy(self._bank)
        self._bank, self._stepped_paths, self.n_paths = None, False, 0

    def close(self):
        self._drop_bank()
        for eng in (getattr(self, "_eng", None), getattr(self, "_nominal", None)):
            if eng is not None:
                eng.close()

    def __del__(self):
        try:
            self._drop_bank()
        except Exception:
            pass

    def set_traj(self, x_ref, y_ref, psi_ref, vel_ref):
        """The global path every vehicle follows (RefTrajectory.set_traj, ref_traj.py:67-86)."""
        self._ref.set_traj(x_ref, y_ref, psi_ref, vel_ref)
        cols = self._ref._cols
        p = self._path
        p.M = int(self._ref.trajectory.shape[0])
        p.vel, p.x, p.y, p.psi, p.psi_unwrapped, p.cdist, p.curv = [c.data_ptr() for c in cols]

    def _poses(self, *ins):
        """The seven pose tensors of a call, checked (float64 [B] on the device), as the pointers the library takes."""
        for t in ins:
            self._eng._chk(t, (self.B,))
        return [_ptr(t) for t in ins]

    def _outs(self):
        """The iterate, the state carried from step to step, the workspace and the record: the ten pointers every step entry takes."""
        return (_ptr(self.x_opt), _ptr(self.w_opt), _ptr(self.safe_count), _ptr(self.prev_u), _ptr(self.has_valid), _ptr(self._work),
                _ptr(self.ack), _ptr(self.mode), _ptr(self.valid), _ptr(self.status))

    def _lane(self, who, lane, back, ahead):
        prm = AdmpcLaneParams(L=int(lane), back=int(back), ahead=int(ahead))
        if not 34 <= prm.L <= 256 or prm.back < 0 or prm.ahead < 0:
            raise ValueError("%s: lane must be in [34, 256], back and ahead must not be negative" % who)
        return prm

    def step(self, x, y, yaw, vx, vy, yaw_rate, steer):
        """One control step for every vehicle: float64 [B] device tensors in.  Asynchronous on the current stream; returns FleetStep."""
        poses = self._poses(x, y, yaw, vx, vy, yaw_rate, steer)
        _lib.check(self.lib.admpc_control_step_batch(self._eng._h, C.byref(self._path), C.byref(self._prm), self.B, *poses, *self._outs(),
                                                     self._eng._stream()))
        return FleetStep(self.ack, self.mode, self.status, self.valid, self.x_opt, self.w_opt)

    def set_paths(self, paths):
        """A bank of global paths, a list of (x_ref, y_ref, psi_ref, vel_ref), each prepared as set_traj prepares the one path
        (RefTrajectory.set_traj, ref_traj.py:67-86).  step_paths lays vehicle b against paths[path_of[b]].  Allocates and synchronises."""
        paths = list(paths)
        if not paths:
            raise ValueError("set_paths needs at least one path")
        rt = RefTrajectory(traj_horizon=self.N, traj_dt=self._path.dt, device=self.device.index)
        descs, keep = (AdmpcPath * len(paths))(), []
        for d, p in zip(descs, paths):
            rt.set_traj(*p)
            keep.append(rt._cols)                                         # alive until the bank has copied them
            d.M, d.H, d.dt = int(rt.trajectory.shape[0]), self.N, self._path.dt
            d.vel, d.x, d.y, d.psi, d.psi_unwrapped, d.cdist, d.curv = [c.data_ptr() for c in rt._cols]
        torch.cuda.synchronize(self.device)                               # the columns were uploaded on torch's stream
        bank = C.c_void_p(0)
        _lib.check(self.lib.admpc_path_bank_create(self.device.index, len(paths), descs, C.byref(bank)))
        self._drop_bank()
        self._bank, self.n_paths = bank, len(paths)

    def step_paths(self, path_of, x, y, yaw, vx, vy, yaw_rate, steer):
        """step() with a path per vehicle: path_of int32 [B] device tensor of indices into the paths of set_paths.  A vehicle whose index
        is outside the bank ends the step as one whose solve failed (status 4, brake record, cost +inf).  Returns FleetPathStep."""
        if self._bank is None:
            raise ValueError("step_paths: no bank of paths, call set_paths first")
        self._eng._chk(path_of, (self.B,), torch.int32)
        poses = self._poses(x, y, yaw, vx, vy, yaw_rate, steer)
        _lib.check(self.lib.admpc_control_step_bank_batch(self._eng._h, self._bank, C.byref(self._prm), self.B, _ptr(path_of), *poses,
                                                          *self._outs(), _ptr(self.cost), self._eng._stream()))
        self._stepped_paths = True
        return FleetPathStep(self.ack, self.mode, self.status, self.valid, self.x_opt, self.w_opt, self.cost)

    def step_route(self, path_of, x, y, yaw, vx, vy, yaw_rate, steer, lane=64, back=8, ahead=64):
        """step_paths for vehicles anywhere along their route: every step cuts a local lane of `lane` waypoints (34 .. 256) out of route
        path_of[b], beginning at the waypoint nearest to the vehicle, clamps its speeds at the vehicle's speed (``resample``), tabulates it
        as set_traj does and lays the reference window on it (include/admpc_lane.h).  The nearest waypoint is searched over the whole
        route on a vehicle's first step (lane_idx -1) and from `back` waypoints behind to `ahead` waypoints in front of the last answer
        afterwards.  Returns FleetLaneStep; best_of works as after step_paths."""
        if self._bank is None:
            raise ValueError("step_route: no bank of paths, call set_paths first")
        prm = self._lane("step_route", lane, back, ahead)
        self._eng._chk(path_of, (self.B,), torch.int32)
        poses = self._poses(x, y, yaw, vx, vy, yaw_rate, steer)
        _lib.check(self.lib.admpc_control_step_lane_batch(self._eng._h, self._bank, C.byref(prm), C.byref(self._prm), self.B, _ptr(path_of),
                                                          _ptr(self.lane_idx), *poses, *self._outs(), _ptr(self.cost), self._eng._stream()))
        self._stepped_paths = True
        return FleetLaneStep(self.ack, self.mode, self.status, self.valid, self.x_opt, self.w_opt, self.cost, self.lane_idx)

    def set_plant(self, dt=None, substeps=1, blend_min=None, blend_max=None, brake_acc=None, v_min=0.0, model=None):
        """The plant of plant_step and rollout_route (include/admpc_plant.h): a command is held for `dt` (None: opt_dt) and the model is
        integrated over it in `substeps` RK4 steps, blended over the plant's own speed band (None: the controller's); a brake record
        decelerates at `brake_acc` (None: the vehicle's acc_min) and v_x never falls below `v_min`.  `model`: a BatchSolver whose vehicle
        constants, bounds and GP residual the plant uses in place of the controller's own."""
        prm = AdmpcPlantParams(dt=float(self.opt_dt if dt is None else dt),
                               blend_min=float(self._prm.blend_min if blend_min is None else blend_min),
                               blend_max=float(self._prm.blend_max if blend_max is None else blend_max),
                               brake_acc=float(self.ad.acc_min if brake_acc is None else brake_acc), v_min=float(v_min),
                               substeps=int(substeps), reserved=0)
        if not (prm.dt > 0 and np.isfinite(prm.dt)) or not prm.blend_max > prm.blend_min or not prm.brake_acc <= 0 or not prm.v_min >= 0 \
                or not 1 <= prm.substeps <= 64:
            raise ValueError("set_plant: dt must be positive and finite, blend_max above blend_min, brake_acc <= 0, v_min >= 0, "
                             "substeps in [1, 64]")
        if model is not None and (not isinstance(model, BatchSolver) or model.device != self.device):
            raise ValueError("set_plant: model must be a BatchSolver on %s" % self.device)
        self._plant, self._plant_model = prm, model

    def plant_step(self, x, y, yaw, vx, vy, yaw_rate, steer):
        """Advances the seven float64 [B] device tensors in place by one period of the plant (set_plant) under the controller's last
        ack and mode.  Asynchronous on the current stream."""
        poses = self._poses(x, y, yaw, vx, vy, yaw_rate, steer)
        model = self._plant_model if self._plant_model is not None else self._eng
        _lib.check(self.lib.admpc_plant_step_batch(model._h, C.byref(self._plant), self.B, _ptr(self.ack), _ptr(self.mode), *poses,
                                                   self._eng._stream()))

    def rollout_route(self, path_of, x, y, yaw, vx, vy, yaw_rate, steer, steps, lane=64, back=8, ahead=64, record=False, accumulate=False,
                      observe=False):
        """`steps` closed-loop steps on the device in one call: step_route, then the plant step on the pose tensors, which are advanced
        in place; no host round trip between the steps.  ``tally`` and ``counts`` are the controller's own tensors, zeroed on the current
        stream at the start of the call unless `accumulate`; `record` also returns the poses of every step.  `observe`: every step is
        observed as observe_latch before the first and observe behind each would (needs ``learn``).  Returns FleetRollout; best_of works
        as after step_route."""
        if self._bank is None:
            raise ValueError("rollout_route: no bank of paths, call set_paths first")
        prm = self._lane("rollout_route", lane, back, ahead)
        T = int(steps)
        if not 0 <= T <= 4096:
            raise ValueError("rollout_route: steps must be in [0, 4096]")
        self._eng._chk(path_of, (self.B,), torch.int32)
        poses = self._poses(x, y, yaw, vx, vy, yaw_rate, steer)
        if not accumulate:
            self.tally.zero_()
            self.counts.zero_()
        traj = torch.empty((T + 1, NX, self.B), dtype=torch.float64, device=self.device) if record else None
        if record and T == 0:
            for i, t in enumerate((x, y, yaw, vx, vy, yaw_rate, steer)):
                traj[0, i].copy_(t)
        model = self._plant_model._h if self._plant_model is not None else None
        args = (self._eng._h, self._bank, C.byref(prm), C.byref(self._prm), model, C.byref(self._plant), self.B, T,
                _ptr(path_of), _ptr(self.lane_idx), *poses, *self._outs(), _ptr(self.cost), _ptr(self.tally), _ptr(self.counts),
                _ptr(traj) if record else None)
        if observe:
            obs = self._observe_params("rollout_route")
            _lib.check(self.lib.admpc_rollout_observe_lane_batch(*args, self._observer._h, C.byref(obs), _ptr(self._prev), _ptr(self.samples),
                                                                 _ptr(self.bins), _ptr(self.dropped), self._eng._stream()))
        else:
            _lib.check(self.lib.admpc_rollout_lane_batch(*args, self._eng._stream()))
        self._stepped_paths = True
        return FleetRollout(self.ack, self.mode, self.status, self.valid, self.x_opt, self.w_opt, self.cost, self.lane_idx, self.tally,
                            self.counts, traj)

    # -- learning the residual GP (include/admpc_learn.h): what the car adds to learning.py's FleetLearning -------------------------------
    def _observe_params(self, who, observing=True):
        """The parameters of an observation as things stand: the plant's period and sub-steps, the controller's own speed band.  A call
        that observes is refused when the plant model's input bounds are not the controller's."""
        self._learns(who)
        pm = self._plant_model if observing else None
        if pm is not None and (list(pm.cfg.lbu) != list(self._eng.cfg.lbu) or list(pm.cfg.ubu) != list(self._eng.cfg.ubu)):
            raise ValueError("%s: the plant model's input bounds lbu / ubu differ from the controller's: the inputs the plant applied "
                             "cannot be told from the record" % who)
        o = self._obs
        o.dt, o.substeps, o.blend_min, o.blend_max = self._plant.dt, self._plant.substeps, self._prm.blend_min, self._prm.blend_max
        return o

    def observe_latch(self, x, y, yaw, vx, vy, yaw_rate, steer):
        """Takes the poses the next observe will predict from.  Asynchronous on the current stream."""
        self._observe_params("observe_latch")
        poses = self._poses(x, y, yaw, vx, vy, yaw_rate, steer)
        _lib.check(self.lib.admpc_observe_latch_batch(self.device.index, self.B, *poses, _ptr(self._prev), self._eng._stream()))

    def observe(self, x, y, yaw, vx, vy, yaw_rate, steer):
        """The poses one plant period after the latched ones, under the controller's last ack and mode: what the observer's model did not
        predict of v_x, v_y and the yaw rate, per second, goes into ``samples`` [B,10] and from there into ``bins`` [4,32,5] (count, feature
        sums, target sum per bin) and ``dropped`` [5]; the poses are latched for the next call.  Asynchronous on the current stream."""
        obs = self._observe_params("observe")
        poses = self._poses(x, y, yaw, vx, vy, yaw_rate, steer)
        _lib.check(self.lib.admpc_observe_batch(self._observer._h, C.byref(self._plant), C.byref(obs), self.B, _ptr(self.ack), _ptr(self.mode),
                                                *poses, _ptr(self._prev), _ptr(self.samples), _ptr(self.bins), _ptr(self.dropped),
                                                self._eng._stream()))

    def best_of(self, group, cost=None):
        """The cheapest usable candidate of every group of `group` consecutive instances of the last step_paths or step_route (instance b = v * group + c
        for vehicle v and candidate c): (val float64 [B / group], idx int64 [B / group]) device tensors, idx into the batch, so the command
        of vehicle v is ack[idx[v]].  A group without a usable candidate gives (+inf, its first instance).  `cost`, a float64 [B] device
        tensor, takes the place of the last step's cost: candidates can be chosen by a closed-loop score of rollout_route, for instance
        tally[:, 0] with +inf where counts[:, 2] > 0.  Asynchronous; the tensors are the controller's own and are overwritten by the next
        call."""
        group = int(group)
        if group < 1 or self.B % group != 0:
            raise ValueError("best_of: B = %d is not a multiple of group = %d" % (self.B, group))
        if not self._stepped_paths:
            raise ValueError("best_of: no step_paths yet")
        if cost is None:
            cost = self.cost
        else:
            self._eng._chk(cost, (self.B,))
        G = self.B // group
        val, idx = self._best_val[:G], self._best_idx[:G]
        _lib.check(self.lib.admpc_argmin_groups(self._eng._h, _ptr(cost), G, group, _ptr(val), _ptr(idx), self._eng._stream()))
        return val, idx

    def step_numpy(self, x, y, yaw, vx, vy, yaw_rate, steer):
        """step() with host arrays in and host copies out (synchronises)."""
        d = lambda a: torch.as_tensor(np.array(np.broadcast_to(np.asarray(a, dtype=np.float64), (self.B,))), device=self.device)
        r = self.step(*[d(a) for a in (x, y, yaw, vx, vy, yaw_rate, steer)])
        torch.cuda.current_stream(self.device).synchronize()
        return FleetStep(*[t.cpu().numpy() for t in r])

    def reset(self, mask=None):
        """Selected vehicles (bool [B], host or device; None: all) start over as a freshly created controller: zero iterate, no
        previous valid inputs, safe_count 0 -- what re-creating the solver in reset_mpc_optimizer would give (gp_ad_mpc_node.py:154-158) --
        and, for step_route, a search of the whole route (lane_idx -1)."""
        if mask is None:
            m = slice(None)
        else:
            m = torch.as_tensor(np.asarray(mask) if not isinstance(mask, torch.Tensor) else mask, device=self.device).to(torch.bool)
            if tuple(m.shape) != (self.B,):
                raise ValueError("mask must have shape (%d,)" % self.B)
        for t in (self.x_opt, self.w_opt, self.safe_count, self.prev_u, self.has_valid):
            t[m] = 0
        self.lane_idx[m] = -1
