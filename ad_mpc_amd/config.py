"""ctypes mirror of ``AdmpcConfig`` / ``AdmpcGp`` (include/admpc.h) plus the reference's shipped values.

Every default cites the reference line it comes from (paths relative to
``data_driven_mpc/ros_gp_mpc`` of HMCL-UNIST/AD_MPC).
"""
import ctypes as C

import numpy as np

NX, NU, NY = 7, 2, 9
MAX_N = 128
GP_MAX = 4
GP_MAX_POINTS = 32
GP_MAX_FEAT = 3


class AdmpcGp(C.Structure):
    _fields_ = [
        ("n_feat", C.c_int32),
        ("feat", C.c_int32 * GP_MAX_FEAT),
        ("out", C.c_int32),
        ("n_points", C.c_int32),
        ("sigma_f", C.c_double),
        ("inv_l2", C.c_double * GP_MAX_FEAT),
        ("ymean", C.c_double),
        ("Z", (C.c_double * GP_MAX_POINTS) * GP_MAX_FEAT),
        ("alpha", C.c_double * GP_MAX_POINTS),
    ]


class AdmpcConfig(C.Structure):
    _fields_ = [
        ("N", C.c_int32),
        ("ipm_iter_max", C.c_int32),
        ("sqp_iters", C.c_int32),
        ("n_gp", C.c_int32),
        ("Ts", C.c_double),
        ("W", C.c_double * NY),
        ("We", C.c_double * NX),
        ("lbu", C.c_double * NU),
        ("ubu", C.c_double * NU),
        ("lbx_delta", C.c_double),
        ("ubx_delta", C.c_double),
        ("zl", C.c_double),
        ("zu", C.c_double),
        ("mass", C.c_double),
        ("L_F", C.c_double),
        ("L_R", C.c_double),
        ("Iz", C.c_double),
        ("Cf", C.c_double),
        ("Cr", C.c_double),
        ("ipm_mu0", C.c_double),
        ("ipm_thr0", C.c_double),
        ("ipm_tol_comp", C.c_double),
        ("ipm_tol_res", C.c_double),
        ("ipm_tol_step", C.c_double),
        ("ipm_try_unconstrained", C.c_double),
        ("ipm_warm_thr", C.c_double),
        ("ipm_warm_restart", C.c_double),
        ("ipm_fallback_iter", C.c_double),
        ("sqp_tol", C.c_double),
        ("gp", AdmpcGp * GP_MAX),
    ]

    def copy(self):
        other = AdmpcConfig()
        C.memmove(C.byref(other), C.byref(self), C.sizeof(AdmpcConfig))
        return other


class AdmpcPath(C.Structure):
    """The global path of admpc_control_step_batch (include/admpc.h): device columns as admpc_waypoints_batch reads them."""
    _fields_ = [("M", C.c_int32), ("H", C.c_int32), ("dt", C.c_double)] + \
        [(k, C.c_void_p) for k in ("vel", "x", "y", "psi", "psi_unwrapped", "cdist", "curv")]


class AdmpcStepParams(C.Structure):
    _fields_ = [("blend_min", C.c_double), ("blend_max", C.c_double), ("acc_max", C.c_double), ("resample_dt", C.c_double),
                ("resample", C.c_int32), ("threshold", C.c_int32)]


class AdmpcLaneParams(C.Structure):
    """The lane of admpc_control_step_lane_batch (include/admpc_lane.h): L waypoints in [34, 256], the search window in waypoints."""
    _fields_ = [("L", C.c_int32), ("back", C.c_int32), ("ahead", C.c_int32)]


class AdmpcPlantParams(C.Structure):
    """The plant of admpc_plant_step_batch / admpc_rollout_lane_batch (include/admpc_plant.h): the period a command is held for, the
    plant's own speed band, the acceleration under a brake record, the floor of v_x, the RK4 sub-steps per period (1 .. 64)."""
    _fields_ = [("dt", C.c_double), ("blend_min", C.c_double), ("blend_max", C.c_double), ("brake_acc", C.c_double), ("v_min", C.c_double),
                ("substeps", C.c_int32), ("reserved", C.c_int32)]


class AdmpcGpBins(C.Structure):
    """One regressor to learn (include/admpc_learn.h): its features and output row as in AdmpcGp, the grid of bins over the features
    (product of nb at most GP_MAX_POINTS), and the fixed hyperparameters of the fit."""
    _fields_ = [("n_feat", C.c_int32), ("feat", C.c_int32 * GP_MAX_FEAT), ("out", C.c_int32), ("nb", C.c_int32 * GP_MAX_FEAT),
                ("lo", C.c_double * GP_MAX_FEAT), ("hi", C.c_double * GP_MAX_FEAT), ("sigma_f", C.c_double),
                ("length", C.c_double * GP_MAX_FEAT), ("noise", C.c_double), ("count_noise", C.c_double)]


class AdmpcObserveParams(C.Structure):
    """The observation of a step (include/admpc_learn.h): the period between two poses, the MODEL's speed band, the RK4 sub-steps of
    the prediction, and the regressors to learn."""
    _fields_ = [("dt", C.c_double), ("blend_min", C.c_double), ("blend_max", C.c_double), ("substeps", C.c_int32), ("n_gp", C.c_int32),
                ("gp", AdmpcGpBins * GP_MAX)]


GP_SEARCH_MAX = 4096       # candidates per regressor and round of the hyperparameter search (include/admpc_hyper.h)
GP_HYPER = 16              # doubles of search state per regressor
GP_NO_OPTIMUM = -33        # info of a re-fit whose search found no finite NLL


class AdmpcGpSearchBox(C.Structure):
    """The box of one regressor's search (include/admpc_hyper.h): slots length[0 .. 2], sigma_f, noise in natural units; lo == hi
    fixes a slot."""
    _fields_ = [("lo", C.c_double * 5), ("hi", C.c_double * 5)]


class AdmpcGpSearchParams(C.Structure):
    """The zooming grid search of the hyperparameters (include/admpc_hyper.h): grid points per free slot (3, 5, 7 or 9), rounds, the
    factor the grid's step shrinks by after every round, and a box per regressor."""
    _fields_ = [("grid", C.c_int32), ("rounds", C.c_int32), ("shrink", C.c_double), ("box", AdmpcGpSearchBox * GP_MAX)]


# --- vehicle constants: src/ad_mpc/ad_3d.py:47-71 (the 3.14195 "pi" is part of the model) -----------
VEH_MASS = 1500.0
VEH_F_MASS = 900.0
VEH_R_MASS = VEH_MASS - VEH_F_MASS
VEH_L = 2.7
VEH_L_F = VEH_L * (1 - VEH_F_MASS / VEH_MASS)
VEH_L_R = VEH_L * (1 - VEH_R_MASS / VEH_MASS)
VEH_IZ = VEH_L_F * VEH_L_R * (VEH_R_MASS + VEH_F_MASS)
VEH_CF = VEH_F_MASS * 0.5 * 9.81 * 0.165 * 180 / 3.14195
VEH_CR = VEH_R_MASS * 0.5 * 9.81 * 0.165 * 180 / 3.14195
BLEND_MAX = 110.0
BLEND_MIN = 100.0
STEERING_MIN, STEERING_MAX = -0.52, 0.52
STEERING_RATE_MIN, STEERING_RATE_MAX = -3.0, 3.0
ACC_MIN, ACC_MAX = -10.0, 5.0

# --- cost weights used by the node: src/ad_mpc/create_ros_ad_mpc.py:58-59 ---------------------------
Q_DIAG_ROS = (10.0, 10.0, 100.0, 0.0, 0.0, 0.0, 0.0)
R_DIAG_ROS = (1.0, 100.0)
# optimizer-level defaults (unused by the node): src/ad_mpc/ad_3d_optimizer.py:42-45
Q_DIAG_OPT = (10.0, 10.0, 50.0, 0.0, 0.0, 0.0, 1.0)
R_DIAG_OPT = (1.0, 100.0)
TERMINAL_SCALE = 1e-6      # ocp.cost.W_e = diag(q)*1e-6, src/ad_mpc/ad_3d_optimizer.py:151
SLACK_L1 = 10.0            # ocp.cost.zl = zu = 1e1, src/ad_mpc/ad_3d_optimizer.py:171-173

# --- interior point defaults (ours; the reference delegates to HPIPM mode BALANCE, iter_max 50,
#     c_generated_code/acados_solver_sim_car.c:688-692) ---------------------------------------------
IPM_ITER_MAX = 50
IPM_MU0 = 1.0
IPM_THR0 = 0.1
IPM_WARM_THR = 0.01
IPM_WARM_RESTART = 0.1
IPM_FALLBACK_ITER = 30.0
# Stopping levels of the interior point.  Default: the reference's own -- it leaves the QP tolerances unset (acados_models/sim_car_acados_ocp.json:
# qp_solver_tol_* null) and runs HPIPM in mode BALANCE (c_generated_code/acados_solver_sim_car.c:688): every residual norm, the
# complementarity products included, <= 1e-8, and no test on the step.  TIGHT: the levels of rounds 1-2 (complementarity 1e-10, residual 1e-9,
# last input step 1e-6), which take an instance with a nearly degenerate bound pair to within 1e-8 of the exact minimiser (the reference's
# levels leave such an instance up to ~1e-4 away from it: the error of a degenerate pair is sqrt(mu)); `tight_ipm(cfg)` sets them.
IPM_TOL_COMP = 1e-8
IPM_TOL_RES = 1e-8
IPM_TOL_STEP = 1e30
IPM_TIGHT = (1e-10, 1e-9, 1e-6)


def default_config(N=20, Ts=0.05, q=Q_DIAG_ROS, r=R_DIAG_ROS, terminal_scale=TERMINAL_SCALE, sqp_iters=1, sqp_tol=0.0):
    """The reference's shipped OCP for horizon ``N`` and sampling time ``Ts``."""
    if not (2 <= N <= MAX_N):
        raise ValueError("N must be in [2, %d]" % MAX_N)
    c = AdmpcConfig()
    c.N = int(N)
    c.ipm_iter_max = IPM_ITER_MAX
    c.sqp_iters = int(sqp_iters)
    c.sqp_tol = float(sqp_tol)
    c.n_gp = 0
    c.Ts = float(Ts)
    for i in range(NX):
        c.W[i] = float(q[i])
        c.We[i] = float(q[i]) * terminal_scale
    for j in range(NU):
        c.W[NX + j] = float(r[j])
    c.lbu[0], c.lbu[1] = ACC_MIN, STEERING_RATE_MIN
    c.ubu[0], c.ubu[1] = ACC_MAX, STEERING_RATE_MAX
    c.lbx_delta, c.ubx_delta = STEERING_MIN, STEERING_MAX
    c.zl = c.zu = SLACK_L1
    c.mass, c.L_F, c.L_R, c.Iz, c.Cf, c.Cr = VEH_MASS, VEH_L_F, VEH_L_R, VEH_IZ, VEH_CF, VEH_CR
    c.ipm_mu0, c.ipm_thr0 = IPM_MU0, IPM_THR0
    c.ipm_tol_comp, c.ipm_tol_res, c.ipm_tol_step = IPM_TOL_COMP, IPM_TOL_RES, IPM_TOL_STEP
    c.ipm_try_unconstrained = 1.0
    c.ipm_warm_thr = IPM_WARM_THR
    c.ipm_warm_restart = IPM_WARM_RESTART
    c.ipm_fallback_iter = IPM_FALLBACK_ITER
    return c


def set_gp(cfg, gps):
    """Install residual GPs.  ``gps``: iterable of dicts with keys feat (an index into [x;u] or a list of up to 3), out, Z (n or
    n x d training inputs), alpha, length_scale (scalar or one per feature), sigma_f, ymean -- squared-exponential GPs with a diagonal
    length-scale matrix, src/model_fitting/gp.py:81-138,446-471."""
    gps = list(gps)
    if len(gps) > GP_MAX:
        raise ValueError("at most %d GPs" % GP_MAX)
    cfg.n_gp = len(gps)
    for g, d in enumerate(gps):
        feats = [int(f) for f in np.atleast_1d(d["feat"]).reshape(-1)]
        nf = len(feats)
        al = np.asarray(d["alpha"], dtype=np.float64).reshape(-1)
        Z = np.asarray(d["Z"], dtype=np.float64)
        Z = Z.reshape(al.size, -1) if al.size else Z.reshape(0, nf)      # no training point (the mean is ymean): nothing to infer a width from
        ell = np.broadcast_to(np.asarray(d["length_scale"], dtype=np.float64).reshape(-1), (nf,)) if np.size(d["length_scale"]) in (1, nf) else None
        if not (1 <= nf <= GP_MAX_FEAT) or Z.shape[1] != nf or ell is None or al.size > GP_MAX_POINTS:
            raise ValueError("bad GP size")
        s = cfg.gp[g]
        s.n_feat, s.out, s.n_points = nf, int(d["out"]), int(al.size)
        s.sigma_f = float(d.get("sigma_f", 1.0))
        s.ymean = float(d.get("ymean", 0.0))
        for k in range(GP_MAX_FEAT):
            s.feat[k] = feats[k] if k < nf else 0
            s.inv_l2[k] = 1.0 / float(ell[k]) ** 2 if k < nf else 0.0
            for i in range(GP_MAX_POINTS):
                s.Z[k][i] = float(Z[i, k]) if (k < nf and i < al.size) else 0.0
        for i in range(GP_MAX_POINTS):
            s.alpha[i] = float(al[i]) if i < al.size else 0.0
    return cfg


def tight_ipm(cfg):
    """The interior point's stopping levels of rounds 1-2 (in place; returns cfg): every instance to within 1e-8 of the exact minimiser."""
    cfg.ipm_tol_comp, cfg.ipm_tol_res, cfg.ipm_tol_step = IPM_TIGHT
    return cfg


def tight_config(*a, **kw):
    """default_config with the tight stopping levels (tests that compare with exact minimisers, iteration-count tables of rounds 1-2)."""
    return tight_ipm(default_config(*a, **kw))


def learn_bins(learn, feat_range=(3, 8), out_range=(3, 5), gp_max=GP_MAX):
    """The AdmpcGpBins of FleetController(learn=...): a list of dicts with the keys feat (an index into [x;u] in 3 .. 8, or a list of up
    to 3), out (3 .. 5), lo, hi, bins (one per feature; the product at most GP_MAX_POINTS), length_scale (a scalar or one per feature),
    sigma_f = 1.0, noise = 1e-6, count_noise = 0.0.  Raises ValueError on bad bins; the library refuses the same.  ``feat_range``,
    ``out_range`` and ``gp_max`` are the car's; quad_config.quad_learn_bins passes the quadrotor's."""
    learn = list(learn)
    (f_lo, f_hi), (o_lo, o_hi) = feat_range, out_range
    if not 1 <= len(learn) <= gp_max:
        raise ValueError("learn: 1 to %d regressors" % gp_max)
    out = (AdmpcGpBins * gp_max)()
    for g, d in enumerate(learn):
        feats = [int(f) for f in np.atleast_1d(d["feat"]).reshape(-1)]
        nf = len(feats)
        if not 1 <= nf <= GP_MAX_FEAT or any(not f_lo <= f <= f_hi for f in feats) or not o_lo <= int(d["out"]) <= o_hi:
            raise ValueError("learn[%d]: 1 to 3 features in %d .. %d, out in %d .. %d" % (g, f_lo, f_hi, o_lo, o_hi))
        vec = lambda k: np.asarray(d[k], dtype=np.float64).reshape(-1)
        lo, hi, nb, ell = vec("lo"), vec("hi"), np.atleast_1d(d["bins"]).reshape(-1), vec("length_scale")
        if ell.size == 1:
            ell = np.repeat(ell, nf)
        if not (lo.size == hi.size == nb.size == ell.size == nf):
            raise ValueError("learn[%d]: lo, hi, bins and length_scale need one entry per feature" % g)
        nb = [int(k) for k in nb]
        sf, noise, cn = float(d.get("sigma_f", 1.0)), float(d.get("noise", 1e-6)), float(d.get("count_noise", 0.0))
        if min(nb) < 1 or int(np.prod(nb)) > GP_MAX_POINTS or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
            raise ValueError("learn[%d]: bad bins: every count >= 1, their product <= %d, lo and hi finite with hi > lo" % (g, GP_MAX_POINTS))
        if not (np.isfinite(ell).all() and (ell > 0).all() and np.isfinite(sf) and sf > 0 and np.isfinite(noise) and noise > 0
                and np.isfinite(cn) and cn >= 0):
            raise ValueError("learn[%d]: length_scale, sigma_f and noise must be positive and finite, count_noise >= 0" % g)
        b = out[g]
        b.n_feat, b.out, b.sigma_f, b.noise, b.count_noise = nf, int(d["out"]), sf, noise, cn
        for k in range(GP_MAX_FEAT):
            used = k < nf
            b.feat[k], b.nb[k] = (feats[k], nb[k]) if used else (0, 1)
            b.lo[k], b.hi[k], b.length[k] = (lo[k], hi[k], ell[k]) if used else (0.0, 0.0, 0.0)
    return out, len(learn)


# the reference's bounds of the search (src/model_fitting/gp.py:337-338): lengths and sigma_f in [1e-5, 1e1], sigma_n in [1e-8, 1] --
# the noise searched here is sigma_n^2
SEARCH_BOUNDS = dict(length_scale=(1e-5, 1e1), sigma_f=(1e-5, 1e1), noise=(1e-16, 1.0))


def search_boxes(learn, bounds=None):
    """The AdmpcGpSearchBox of every regressor of ``learn`` (the list learn_bins takes).  ``bounds``: None for the reference's
    (SEARCH_BOUNDS), or one dict per regressor with any of length_scale (one (lo, hi) or one per feature), sigma_f, noise; lo == hi
    fixes a slot.  Raises ValueError on a bound that is not 0 < lo <= hi, finite; the library refuses the same."""
    learn = list(learn)
    if bounds is None:
        bounds = [{}] * len(learn)
    bounds = list(bounds)
    if len(bounds) != len(learn):
        raise ValueError("bounds: one dict per regressor (%d), got %d" % (len(learn), len(bounds)))
    out = (AdmpcGpSearchBox * GP_MAX)()
    for g, (d, b) in enumerate(zip(learn, bounds)):
        nf = np.atleast_1d(d["feat"]).size
        b = dict(SEARCH_BOUNDS, **(b or {}))
        ell = np.asarray(b["length_scale"], dtype=np.float64).reshape(-1, 2)
        if ell.shape[0] == 1:
            ell = np.repeat(ell, nf, axis=0)
        if ell.shape[0] != nf:
            raise ValueError("bounds[%d]: length_scale needs one (lo, hi) or one per feature" % g)
        rows = [ell[k] if k < nf else (1.0, 1.0) for k in range(GP_MAX_FEAT)] + [b["sigma_f"], b["noise"]]
        for k, (lo, hi) in enumerate(rows):
            lo, hi = float(lo), float(hi)
            if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= hi):
                raise ValueError("bounds[%d]: every bound needs 0 < lo <= hi, finite; got (%r, %r)" % (g, lo, hi))
            out[g].lo[k], out[g].hi[k] = lo, hi
    return out
