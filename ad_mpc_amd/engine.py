"""Batch solve engine: thin host wrapper over the C ABI (include/admpc.h).

torch is used only as the carrier of device memory and streams; every number is produced by the
HIP kernels in libadmpc.so.  All tensors are float64 / int32, contiguous, on the solver's device.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .config import NX, NU, NY, default_config, set_gp
from .quad_config import QNX, QNU, QNY, default_quad_config, set_quad_gp


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def packed_layout(fields_in, fields_out):
    """Layout of a staging buffer: every field of ``(name, shape)`` on a 32-double (256-byte) boundary, like an allocation of its own, the
    inputs first.  Returns ({name: (offset, count)} in doubles, the length of the input part, the total length)."""
    off, o = {}, 0
    for k, shp in tuple(fields_in) + tuple(fields_out):
        n = int(np.prod(shp)); off[k] = (o, n); o += -(-n // 32) * 32
    return off, (off[fields_out[0][0]][0] if fields_out else o), o


class PackedIO:
    """Staging for a single-instance solve through the reference-shaped host classes: every input in ONE pinned host buffer / ONE device buffer
    (each field on a 256-byte boundary, handed to the engine as a contiguous view or as its address), every float output behind them, the status
    words in a pair of int32 -- a solve is one copy up, the kernels, one copy down (+ the status pair), one stream synchronisation.  (A tensor per
    field, each with a copy of its own, was 0.2 ms of a 0.58 ms control step of the car.)"""

    def __init__(self, device, fields_in, fields_out, n_int=2):
        self.device = device
        self.shape = {k: tuple(shp) for k, shp in tuple(fields_in) + tuple(fields_out)}
        self.off, self.n_in, o = packed_layout(fields_in, fields_out)
        self.hbuf = torch.zeros(o, dtype=torch.float64).pin_memory(); self.dbuf = torch.zeros(o, dtype=torch.float64, device=device)
        self.hint = torch.zeros(n_int, dtype=torch.int32).pin_memory(); self.dint = torch.zeros(n_int, dtype=torch.int32, device=device)
        self.h, self.hi = self.hbuf.numpy(), self.hint.numpy()
        # device addresses, computed once: of every field (a caller of the C ABI needs no view per call) and of the int32 words
        self.ptr = {k: C.c_void_p(self.dbuf.data_ptr() + 8 * o) for k, (o, n) in self.off.items()}
        self.iptr = tuple(C.c_void_p(self.dint.data_ptr() + 4 * i) for i in range(n_int))

    def put(self, k, a):
        o, n = self.off[k]; self.h[o:o + n] = np.asarray(a, dtype=np.float64).reshape(-1)

    def dev(self, k):
        o, n = self.off[k]; return self.dbuf[o:o + n].view(self.shape[k])

    def take(self, k):
        o, n = self.off[k]; return self.h[o:o + n].reshape(self.shape[k]).copy()

    def upload(self):
        self.dbuf[:self.n_in].copy_(self.hbuf[:self.n_in], non_blocking=True)

    def download(self, first):
        """Everything from field `first` on comes back (the iterate is updated in place: it sits at the end of the inputs), then one synchronisation."""
        o = self.off[first][0]
        self.hbuf[o:].copy_(self.dbuf[o:], non_blocking=True); self.hint.copy_(self.dint, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()


class _Handle:
    """A library handle on one device: created from a config by the library function named ``create``, destroyed by ``destroy``."""

    def __init__(self, create, destroy, cfg, device):
        if not torch.cuda.is_available():
            raise _lib.AdmpcError("no HIP device visible: the AD-MPC engine has no CPU fallback")
        self.lib = _lib.load()
        self.cfg = cfg.copy()
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        self._destroy = getattr(self.lib, destroy)
        h = C.c_void_p(0)
        _lib.check(getattr(self.lib, create)(C.byref(self.cfg), self.device_index, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def N(self):
        return int(self.cfg.N)

    def to_device(self, a, dtype=torch.float64):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=self.device).contiguous()

    def _chk(self, t, shape, dtype=torch.float64):
        if t.dtype != dtype or not t.is_contiguous() or t.device != self.device or tuple(t.shape) != tuple(shape):
            raise ValueError("expected contiguous %s tensor of shape %s on %s, got %s %s on %s"
                             % (dtype, tuple(shape), self.device, t.dtype, tuple(t.shape), t.device))

    def _chk_outputs(self, B, dt, cost, status, iters):
        if cost is not None: self._chk(cost, (B,), dt)
        if status is not None: self._chk(status, (B,), torch.int32)
        if iters is not None: self._chk(iters, (B,), torch.int32)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


class BatchSolver(_Handle):
    """One solver object per (config, device).  Replaces the AcadosOcpSolver object of
    ad_3d_optimizer.py:209 for a whole batch of independent MPC instances."""

    def __init__(self, cfg=None, device=0):
        super().__init__("admpc_create", "admpc_destroy", cfg if cfg is not None else default_config(), device)

    def _chk_solve(self, B, dt, x0, yref, yref_e, p, xbar, ubar, cost=None, status=None, iters=None):
        """The arguments every solve entry of the car shares."""
        N = self.N
        self._chk(x0, (B, NX), dt); self._chk(yref, (B, N, NY), dt); self._chk(yref_e, (B, NX), dt); self._chk(p, (B,), dt)
        self._chk(xbar, (B, N + 1, NX), dt); self._chk(ubar, (B, N, NU), dt)
        self._chk_outputs(B, dt, cost, status, iters)

    # -- the hot path --------------------------------------------------------------------------
    def solve(self, x0, yref, yref_e, p, xbar, ubar, cost=None, status=None, iters=None):
        """One SQP-RTI step for every instance, in place on xbar/ubar (device tensors).  Asynchronous.
        The dtype of x0 selects the path: float64 (admpc_solve_batch) or float32 (admpc_solve_batch_f32, storage and compute)."""
        B = x0.shape[0]
        dt = x0.dtype
        if dt not in (torch.float64, torch.float32):
            raise ValueError("x0 must be float64 or float32")
        self._chk_solve(B, dt, x0, yref, yref_e, p, xbar, ubar, cost, status, iters)
        fn = self.lib.admpc_solve_batch if dt == torch.float64 else self.lib.admpc_solve_batch_f32
        _lib.check(fn(self._h, B, _ptr(x0), _ptr(yref), _ptr(yref_e), _ptr(p), _ptr(xbar), _ptr(ubar),
                      _ptr(cost), _ptr(status), _ptr(iters), self._stream()))

    def solve_with_multipliers(self, x0, yref, yref_e, p, xbar, ubar, cost=None, status=None, iters=None):
        """admpc_solve_batch_ex (float64): the step plus pi [B,N+1,7] and ineq [B,N,20] (see include/admpc.h)."""
        N = self.N
        B = x0.shape[0]
        self._chk_solve(B, torch.float64, x0, yref, yref_e, p, xbar, ubar, cost, status, iters)
        pi = torch.empty((B, N + 1, NX), dtype=torch.float64, device=self.device)
        ineq = torch.empty((B, N, 20), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.admpc_solve_batch_ex(self._h, B, _ptr(x0), _ptr(yref), _ptr(yref_e), _ptr(p), _ptr(xbar), _ptr(ubar),
                                                 _ptr(cost), _ptr(status), _ptr(iters), _ptr(pi), _ptr(ineq), self._stream()))
        return pi, ineq

    def nlp_residuals(self, x0, yref, yref_e, p, xbar, ubar, pi, ineq):
        """admpc_nlp_residuals_batch: [B,4] = (res_stat, res_eq, res_ineq, res_comp) of acados' SQP stopping test at the iterate
        (xbar, ubar) with the multipliers solve_with_multipliers returned for it (AcadosOcpSolver.get_residuals())."""
        N = self.N
        B = x0.shape[0]
        self._chk_solve(B, torch.float64, x0, yref, yref_e, p, xbar, ubar)
        self._chk(pi, (B, N + 1, NX)); self._chk(ineq, (B, N, 20))
        res = torch.empty((B, 4), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.admpc_nlp_residuals_batch(self._h, B, _ptr(x0), _ptr(yref), _ptr(yref_e), _ptr(p), _ptr(xbar), _ptr(ubar),
                                                      _ptr(pi), _ptr(ineq), _ptr(res), self._stream()))
        return res

    def solve_numpy(self, x0, yref, yref_e, p, xbar, ubar, dtype=np.float64):
        """Convenience for tests / the single-instance shims: host arrays in, host arrays out
        (x, u, cost, status, iters).  dtype=np.float32 runs the fp32 path."""
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        d = lambda a: self.to_device(a, tdt)
        x0 = np.asarray(x0, dtype=dtype).reshape(-1, NX)
        B, N = x0.shape[0], self.N
        tx0 = d(x0); tyr = d(np.asarray(yref, dtype=dtype).reshape(B, N, NY)); tye = d(np.asarray(yref_e, dtype=dtype).reshape(B, NX))
        tp = d(np.asarray(p, dtype=dtype).reshape(B))
        tx = d(np.asarray(xbar, dtype=dtype).reshape(B, N + 1, NX)).clone(); tu = d(np.asarray(ubar, dtype=dtype).reshape(B, N, NU)).clone()
        cost = torch.empty(B, dtype=tdt, device=self.device)
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        iters = torch.empty(B, dtype=torch.int32, device=self.device)
        self.solve(tx0, tyr, tye, tp, tx, tu, cost, status, iters)
        torch.cuda.synchronize(self.device)
        return tx.cpu().numpy(), tu.cpu().numpy(), cost.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy()

    def shoot(self, xbar, ubar, p):
        """H1 only: phi [B,N,7], A [B,N,7,7], B [B,N,7,2] (device tensors).  The dtype of xbar selects the instantiation: float64
        (admpc_shoot_batch) or float32 (admpc_shoot_batch_f32)."""
        N = self.N
        B = xbar.shape[0]
        dt = xbar.dtype
        if dt not in (torch.float64, torch.float32):
            raise ValueError("xbar must be float64 or float32")
        self._chk(xbar, (B, N + 1, NX), dt); self._chk(ubar, (B, N, NU), dt); self._chk(p, (B,), dt)
        phi = torch.empty((B, N, NX), dtype=dt, device=self.device)
        A = torch.empty((B, N, NX, NX), dtype=dt, device=self.device)
        Bm = torch.empty((B, N, NX, NU), dtype=dt, device=self.device)
        fn = self.lib.admpc_shoot_batch if dt == torch.float64 else self.lib.admpc_shoot_batch_f32
        _lib.check(fn(self._h, B, _ptr(xbar), _ptr(ubar), _ptr(p), _ptr(phi), _ptr(A), _ptr(Bm), self._stream()))
        return phi, A, Bm

    def shift(self, xbar, ubar, p=None, rollout=True):
        """Receding-horizon shift of the iterate, in place (the reference itself never shifts).
        rollout: new terminal state by one model step under the last input (needs p), else a copy."""
        N = self.N
        B = xbar.shape[0]
        self._chk(xbar, (B, N + 1, NX)); self._chk(ubar, (B, N, NU))
        if rollout:
            if p is None:
                raise ValueError("shift(rollout=True) needs the blend parameter p")
            self._chk(p, (B,))
        _lib.check(self.lib.admpc_shift_batch(self._h, B, _ptr(xbar), _ptr(ubar), _ptr(p if rollout else None), 1 if rollout else 0,
                                              self._stream()))

    def argmin(self, cost, index_offset=0):
        """Local arg-min over a device cost vector -> (val tensor[1], idx tensor[1] int64), ties -> lowest index."""
        B = cost.shape[0]
        self._chk(cost, (B,))
        val = torch.empty(1, dtype=torch.float64, device=self.device)
        idx = torch.empty(1, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.admpc_argmin(self._h, _ptr(cost), B, int(index_offset), _ptr(val), _ptr(idx), self._stream()))
        return val, idx

    def argmin_pair(self, cost, index_offset=0, pair=None):
        """admpc_argmin with value and index written next to each other: a float64[2] tensor whose second element carries
        the bits of the int64 global index -- the 16-byte record that is all-gathered across GPUs."""
        B = cost.shape[0]
        self._chk(cost, (B,))
        if pair is None:
            pair = torch.empty(2, dtype=torch.float64, device=self.device)
        self._chk(pair, (2,))
        _lib.check(self.lib.admpc_argmin(self._h, _ptr(cost), B, int(index_offset), C.c_void_p(pair.data_ptr()),
                                         C.c_void_p(pair.data_ptr() + 8), self._stream()))
        return pair

    def argmin_pairs(self, pairs, out=None):
        """Second level: float64[W,2] gathered records -> float64[2] record of the winner (admpc_argmin_pairs)."""
        W = pairs.shape[0]
        self._chk(pairs, (W, 2))
        if out is None:
            out = torch.empty(2, dtype=torch.float64, device=self.device)
        self._chk(out, (2,))
        _lib.check(self.lib.admpc_argmin_pairs(self._h, _ptr(pairs), W, C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 8),
                                               self._stream()))
        return out

    def epilogue(self, xopt, uopt, xref_xy):
        """Validity bit + Ackermann record per instance."""
        N = self.N
        B = xopt.shape[0]
        self._chk(xopt, (B, N + 1, NX)); self._chk(uopt, (B, N, NU)); self._chk(xref_xy, (B, N + 1, 2))
        ack = torch.empty((B, 4), dtype=torch.float32, device=self.device)
        valid = torch.empty(B, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.admpc_epilogue_batch(self._h, B, _ptr(xopt), _ptr(uopt), _ptr(xref_xy), _ptr(ack), _ptr(valid), self._stream()))
        return ack, valid

    def actuation(self, xopt, uopt, xref_xy, status, steer_meas, safe_count, threshold=10, cost=None):
        """The node's post-solve branch per slot: validity, consecutive-success gate (safe_count is updated in
        place), steering command or brake fallback.  Returns (ack float32 [B,4], mode int32 [B], valid int32 [B]); with `cost`
        given, the cost of every slot that issues no MPC command is set to +inf in place (arg-min over valid candidates)."""
        N = self.N
        B = xopt.shape[0]
        self._chk(xopt, (B, N + 1, NX)); self._chk(uopt, (B, N, NU)); self._chk(xref_xy, (B, N + 1, 2))
        self._chk(status, (B,), torch.int32); self._chk(steer_meas, (B,)); self._chk(safe_count, (B,), torch.int32)
        if cost is not None: self._chk(cost, (B,))
        ack = torch.empty((B, 4), dtype=torch.float32, device=self.device)
        mode = torch.empty(B, dtype=torch.int32, device=self.device)
        valid = torch.empty(B, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.admpc_actuation_batch(self._h, B, _ptr(xopt), _ptr(uopt), _ptr(xref_xy), _ptr(status), _ptr(steer_meas), _ptr(safe_count),
                                                  int(threshold), _ptr(cost), _ptr(ack), _ptr(mode), _ptr(valid), self._stream()))
        return ack, mode, valid

    def resample_vel(self, vel_ref, vx, vy, acc_max, dt):
        """gp_ad_mpc_node.py:344-349 on B rows at once, in place: vel_ref float64 [B,H] (may be a strided row view with unit inner stride)."""
        B, H = vel_ref.shape
        if vel_ref.dtype != torch.float64 or vel_ref.stride(1) != 1 or vel_ref.device != self.device:
            raise ValueError("vel_ref: float64 [B,H] on the solver's device with unit inner stride")
        self._chk(vx, (B,)); self._chk(vy, (B,))
        ld = vel_ref.stride(0) if B > 1 else H
        _lib.check(self.lib.admpc_resample_vel_batch(self.device_index, B, H, int(ld), _ptr(vx), _ptr(vy), float(acc_max), float(dt),
                                                     C.c_void_p(vel_ref.data_ptr()), self._stream()))


class _Ensemble:
    """One handle per cluster on one device, the centroids K x d in the features ``feats``; selection and routing are HIP kernels of the
    library (no gather / scatter, no host synchronisation): every handle runs over the whole batch and leaves the instances of the other
    clusters alone.  A subclass names its model: _SOLVER, _DIMS = (nx, nu) and _SELECT, the library's selection function."""

    def __init__(self, cfgs, centroids, feats, device):
        self.solvers = [self._SOLVER(c, device=device) for c in cfgs]
        s0 = self.solvers[0]
        self.lib, self.device, self.device_index, self.N = s0.lib, s0.device, s0.device_index, s0.N
        cent = np.ascontiguousarray(np.asarray(centroids, dtype=np.float64).reshape(len(self.solvers), -1))
        self._cent = torch.as_tensor(cent, device=self.device).contiguous()      # K x d
        feats = [int(f) for f in np.atleast_1d(feats)]
        self._feats = (C.c_int32 * len(feats))(*feats)
        self._handles = (C.c_void_p * len(self.solvers))(*[sv._h for sv in self.solvers])

    def close(self):
        for s in self.solvers:
            s.close()

    def _stream(self):
        return self.solvers[0]._stream()

    def select(self, x_sel, u_sel, route=None):
        """Cluster of every instance from the state [B,nx] / input [B,nu] the caller selects on (the reference passes the reference state
        and the input target): nearest centroid of the ensemble's features, ties to the lowest index.  float64 device tensors in (row
        views such as ubar[:, 0, :] are welcome), int32 [B] device tensor out.  Asynchronous."""
        B = x_sel.shape[0]
        sv = self.solvers[0]
        nx, nu = self._DIMS
        x_sel, u_sel = x_sel.contiguous(), u_sel.contiguous()
        sv._chk(x_sel, (B, nx)); sv._chk(u_sel, (B, nu))
        if route is None:
            route = torch.empty(B, dtype=torch.int32, device=self.device)
        sv._chk(route, (B,), torch.int32)
        _lib.check(getattr(self.lib, self._SELECT)(self.device_index, B, len(self._feats), self._feats, _ptr(x_sel), _ptr(u_sel),
                                                   int(self._cent.shape[0]), _ptr(self._cent), _ptr(route), self._stream()))
        return route

    def _route(self, gp_ind, B):
        """The cluster index per instance as the library takes it: int32 [B] (int64 is converted)."""
        if gp_ind.dtype != torch.int32:
            gp_ind = gp_ind.to(torch.int32)
        self.solvers[0]._chk(gp_ind, (B,), torch.int32)
        return gp_ind


class EnsembleBatchSolver(_Ensemble):
    """Clustered GP ensembles (reference: one AcadosOcpSolver per cluster, quad_3d_optimizer.py:207, chosen per
    solve by GPEnsemble.select_gp, :452 / :491).  One engine handle per cluster; selection and routing are
    admpc_select_cluster_batch and admpc_solve_batch_routed.  ``ensemble``: gp_loader.GPEnsemble."""
    _SOLVER, _DIMS, _SELECT = BatchSolver, (NX, NU), "admpc_select_cluster_batch"

    def __init__(self, cfg, ensemble, device=0):
        self.ensemble = ensemble
        cfgs = [cfg.copy() for _ in range(ensemble.n_models)]
        for cc, gps in zip(cfgs, ensemble.clusters):
            set_gp(cc, gps)
        super().__init__(cfgs, ensemble.centroids, ensemble.feats, device)

    def solve(self, gp_ind, x0, yref, yref_e, p, xbar, ubar, cost=None, status=None, iters=None):
        """BatchSolver.solve with a cluster index per instance (int32 device tensor, e.g. from `select`; int64 is converted).  In place
        on xbar / ubar.  Asynchronous.  An index outside [0, K) gives status 4 and cost +inf for that instance."""
        B = x0.shape[0]
        gp_ind = self._route(gp_ind, B)
        self.solvers[0]._chk_solve(B, torch.float64, x0, yref, yref_e, p, xbar, ubar, cost, status, iters)
        _lib.check(self.lib.admpc_solve_batch_routed(self._handles, len(self.solvers), B, _ptr(gp_ind), _ptr(x0), _ptr(yref), _ptr(yref_e), _ptr(p),
                                                     _ptr(xbar), _ptr(ubar), _ptr(cost), _ptr(status), _ptr(iters), self._stream()))


class QuadBatchSolver(_Handle):
    """The second vehicle model (include/admpc_quad.h): one SQP-RTI step of the reference's quadrotor MPC for a batch.
    Replaces the AcadosOcpSolver of quad_3d_optimizer.py:207 for B independent instances."""

    def __init__(self, cfg=None, device=0):
        super().__init__("admpc_quad_create", "admpc_quad_destroy", cfg if cfg is not None else default_quad_config(), device)

    def _chk_solve(self, B, x0, yref, yref_e, xbar, ubar, cost=None, status=None, iters=None, gp_state=None):
        """The arguments every solve entry of the quadrotor shares."""
        N = self.N
        self._chk(x0, (B, QNX)); self._chk(yref, (B, N, QNY)); self._chk(yref_e, (B, QNX)); self._chk(xbar, (B, N + 1, QNX)); self._chk(ubar, (B, N, QNU))
        self._chk_outputs(B, torch.float64, cost, status, iters)
        if gp_state is not None: self._chk(gp_state, (B, QNX))

    def solve(self, x0, yref, yref_e, xbar, ubar, cost=None, status=None, iters=None, gp_state=None):
        """In place on xbar [B,N+1,13] / ubar [B,N,4] (float64 device tensors).  Asynchronous.  gp_state [B,13]: the first node's GP
        state (run_optimization's gp_regression_state); None: the initial state x0, the reference's default."""
        B = x0.shape[0]
        self._chk_solve(B, x0, yref, yref_e, xbar, ubar, cost, status, iters, gp_state)
        _lib.check(self.lib.admpc_quad_solve_batch_ex(self._h, B, _ptr(x0), _ptr(yref), _ptr(yref_e), _ptr(gp_state), _ptr(xbar), _ptr(ubar),
                                                      _ptr(cost), _ptr(status), _ptr(iters), self._stream()))

    def set_sqp(self, qp_max=100, tol=1e-6):
        """solver_type "SQP" inside the solve kernel (include/admpc_quad_sqp.h): from here on ``solve`` and every rollout on this handle
        take up to ``qp_max`` QPs per instance, each instance until acados' stopping test passes at ``tol`` (0.0: no test, ``qp_max``
        QPs).  ``qp_max <= 1`` turns the mode off.  Host state: set it before a graph capture.  The defaults are the reference's."""
        _lib.check(self.lib.admpc_quad_set_sqp(self._h, int(qp_max), float(tol)))

    @property
    def sqp(self):
        """(qp_max, tol) of ``set_sqp``; (0, 0.0): the mode is off."""
        q, t = C.c_int32(0), C.c_double(0.0)
        _lib.check(self.lib.admpc_quad_get_sqp(self._h, C.byref(q), C.byref(t)))
        return int(q.value), float(t.value)

    def solve_sqp(self, x0, yref, yref_e, xbar, ubar, cost=None, status=None, iters=None, gp_state=None, qps=None):
        """``solve`` on a handle whose SQP mode is on (``set_sqp``), with qps [B] int32: the QPs started per instance.  status: 0 converged,
        2 the limit of QPs reached (the iterate is valid), 4 a failed QP (the iterate is the one before it).  Asynchronous."""
        B = x0.shape[0]
        self._chk_solve(B, x0, yref, yref_e, xbar, ubar, cost, status, iters, gp_state)
        if qps is not None: self._chk(qps, (B,), torch.int32)
        _lib.check(self.lib.admpc_quad_solve_batch_sqp(self._h, B, _ptr(x0), _ptr(yref), _ptr(yref_e), _ptr(gp_state), _ptr(xbar), _ptr(ubar),
                                                       _ptr(cost), _ptr(status), _ptr(iters), _ptr(qps), self._stream()))

    def shoot(self, xbar, ubar, gp_state=None):
        N, B = self.N, xbar.shape[0]
        self._chk(xbar, (B, N + 1, QNX)); self._chk(ubar, (B, N, QNU))
        if gp_state is not None: self._chk(gp_state, (B, QNX))
        phi = torch.empty((B, N, QNX), dtype=torch.float64, device=self.device)
        A = torch.empty((B, N, QNX, QNX), dtype=torch.float64, device=self.device)
        Bm = torch.empty((B, N, QNX, QNU), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.admpc_quad_shoot_batch_ex(self._h, B, _ptr(xbar), _ptr(ubar), _ptr(gp_state), _ptr(phi), _ptr(A), _ptr(Bm), self._stream()))
        return phi, A, Bm

    def solve_numpy(self, x0, yref, yref_e, xbar, ubar, gp_state=None):
        """Host arrays in, host arrays out: (x, u, cost, status, iters)."""
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=self.device)
        B = np.asarray(x0).shape[0]
        tx, tu = d(xbar).clone(), d(ubar).clone()
        cost = torch.empty(B, dtype=torch.float64, device=self.device); st = torch.empty(B, dtype=torch.int32, device=self.device); it = torch.empty(B, dtype=torch.int32, device=self.device)
        self.solve(d(x0), d(yref), d(yref_e), tx, tu, cost, st, it, gp_state=None if gp_state is None else d(gp_state))
        torch.cuda.synchronize(self.device)
        return tx.cpu().numpy(), tu.cpu().numpy(), cost.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()


class QuadEnsembleBatchSolver(_Ensemble):
    """Clustered GP ensembles of the quadrotor (reference: one AcadosOcpSolver per cluster, quad_3d_optimizer.py:207, chosen per solve
    from the reference state by GPEnsemble.select_gp, :446-452 / :485-491).  One handle per cluster; selection and routing are
    admpc_quad_select_cluster_batch and admpc_quad_solve_batch_routed.  ``clusters[c]``: the ``set_quad_gp`` list of cluster c;
    ``centroids`` K x d in the features ``feats`` (indices into z = [x with the velocity in the body frame; u]).  ``select`` takes the
    reference state with its world-frame velocity: the kernel rotates it to the body frame as the reference does before select_gp."""
    _SOLVER, _DIMS, _SELECT = QuadBatchSolver, (QNX, QNU), "admpc_quad_select_cluster_batch"

    def __init__(self, cfg, clusters, centroids, feats, device=0):
        cfgs = [cfg.copy() for _ in clusters]
        for cc, gps in zip(cfgs, clusters):
            set_quad_gp(cc, gps)
        super().__init__(cfgs, centroids, feats, device)
        if self._cent.shape[1] != len(self._feats):
            raise ValueError("centroids must be K x len(feats)")

    def solve(self, gp_ind, x0, yref, yref_e, xbar, ubar, cost=None, status=None, iters=None, gp_state=None):
        """QuadBatchSolver.solve with a cluster index per instance (int32 device tensor).  In place on xbar / ubar.  Asynchronous.
        An index outside [0, K) gives status 4 and cost +inf for that instance."""
        B = x0.shape[0]
        gp_ind = self._route(gp_ind, B)
        self.solvers[0]._chk_solve(B, x0, yref, yref_e, xbar, ubar, cost, status, iters, gp_state)
        _lib.check(self.lib.admpc_quad_solve_batch_routed(self._handles, len(self.solvers), B, _ptr(gp_ind), _ptr(x0), _ptr(yref), _ptr(yref_e), _ptr(gp_state),
                                                          _ptr(xbar), _ptr(ubar), _ptr(cost), _ptr(status), _ptr(iters), self._stream()))
