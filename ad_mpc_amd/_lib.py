"""Loader of the C-ABI shared library ``libadmpc.so`` (include/admpc.h).

There is NO fallback: if the HIP library is missing or fails to load, importing the solver
surface raises.  The CPU oracle under ``oracle/`` is test infrastructure and is never used here.
"""
import ctypes as C
import os

from .config import AdmpcConfig, AdmpcGpSearchParams, AdmpcLaneParams, AdmpcObserveParams, AdmpcPath, AdmpcPlantParams, AdmpcStepParams
from .quad_config import AdmpcQuadConfig, AdmpcQuadNoiseParams, AdmpcQuadObserveParams, AdmpcQuadPlantParams, AdmpcQuadTargetParams, AdmpcQuadTrajSpec

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libadmpc.so")

# Every prototype of include/admpc.h, include/admpc_quad.h, include/admpc_fleet.h, include/admpc_lane.h, include/admpc_plant.h, include/admpc_learn.h, include/admpc_hyper.h, include/admpc_quad_fleet.h and include/admpc_quad_learn.h: name -> (restype, argtypes).  dp: device pointer to doubles (floats on the
# _f32 entries), ip: to ints, vp: opaque (handle, stream, communicator) -- device pointers travel as integers, so all three are c_void_p.
vp = dp = ip = C.c_void_p
I, D, S = C.c_int, C.c_double, C.c_char_p
cp, qp, hp, fp = C.POINTER(AdmpcConfig), C.POINTER(AdmpcQuadConfig), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)
_CAR = {
    "admpc_default_config": (I, [cp, I, D]),
    "admpc_create": (I, [cp, I, hp]),
    "admpc_destroy": (None, [vp]),
    "admpc_reserve": (I, [vp, I]),
    "admpc_solve_batch": (I, [vp, I, dp, dp, dp, dp, dp, dp, dp, ip, ip, vp]),
    "admpc_solve_batch_ex": (I, [vp, I, dp, dp, dp, dp, dp, dp, dp, ip, ip, dp, dp, vp]),
    "admpc_nlp_residuals_batch": (I, [vp, I, dp, dp, dp, dp, dp, dp, dp, dp, dp, vp]),
    "admpc_solve_batch_f32": (I, [vp, I, dp, dp, dp, dp, dp, dp, dp, ip, ip, vp]),
    "admpc_shoot_batch": (I, [vp, I, dp, dp, dp, dp, dp, dp, vp]),
    "admpc_shoot_batch_f32": (I, [vp, I, dp, dp, dp, dp, dp, dp, vp]),
    "admpc_argmin": (I, [vp, dp, I, C.c_int64, dp, ip, vp]),
    "admpc_argmin_pairs": (I, [vp, dp, I, dp, ip, vp]),
    "admpc_argmin_pairs_host": (I, [dp, I, dp, ip]),
    "admpc_argmin_global": (I, [vp, dp, I, C.c_int64, vp, dp, ip, vp]),
    "admpc_select_cluster_batch": (I, [I, I, I, fp, dp, dp, I, dp, ip, vp]),
    "admpc_solve_batch_routed": (I, [hp, I, I, ip, dp, dp, dp, dp, dp, dp, dp, ip, ip, vp]),
    "admpc_shift_batch": (I, [vp, I, dp, dp, dp, I, vp]),
    "admpc_epilogue_batch": (I, [vp, I, dp, dp, dp, dp, ip, vp]),
    "admpc_actuation_batch": (I, [vp, I, dp, dp, dp, ip, dp, ip, I, dp, dp, ip, ip, vp]),
    "admpc_resample_vel_batch": (I, [I, I, I, I, dp, dp, D, D, dp, vp]),
    "admpc_waypoints_batch": (I, [I, I, I, D, I] + [dp] * 13 + [vp]),
    "admpc_control_step_workspace": (I, [vp, I, C.POINTER(C.c_size_t)]),
    "admpc_control_step_batch": (I, [vp, C.POINTER(AdmpcPath), C.POINTER(AdmpcStepParams), I] + [dp] * 7 + [dp] * 5 + [vp] + [dp] * 4 + [vp]),
    "admpc_last_error": (S, []),
    "admpc_version": (S, []),
}
_QUAD = {
    "admpc_quad_default_config": (None, [qp]),
    "admpc_quad_create": (I, [qp, I, hp]),
    "admpc_quad_destroy": (None, [vp]),
    "admpc_quad_solve_batch": (I, [vp, I, dp, dp, dp, dp, dp, dp, ip, ip, vp]),
    "admpc_quad_solve_batch_ex": (I, [vp, I, dp, dp, dp, dp, dp, dp, dp, ip, ip, vp]),
    "admpc_quad_select_cluster_batch": (I, [I, I, I, fp, dp, dp, I, dp, ip, vp]),
    "admpc_quad_solve_batch_routed": (I, [hp, I, I, ip, dp, dp, dp, dp, dp, dp, dp, ip, ip, vp]),
    "admpc_quad_shoot_batch": (I, [vp, I, dp, dp, dp, dp, dp, vp]),
    "admpc_quad_shoot_batch_ex": (I, [vp, I, dp, dp, dp, dp, dp, dp, vp]),
}
_FLEET = {      # include/admpc_fleet.h: a path per vehicle, the best of C candidate paths
    "admpc_path_bank_create": (I, [I, I, C.POINTER(AdmpcPath), hp]),
    "admpc_path_bank_destroy": (None, [vp]),
    "admpc_waypoints_bank_batch": (I, [vp, I, ip] + [dp] * 3 + [dp, dp, ip] + [vp]),
    "admpc_control_step_bank_batch": (I, [vp, vp, C.POINTER(AdmpcStepParams), I, ip] + [dp] * 7 + [dp] * 5 + [vp] + [dp] * 4 + [dp, vp]),
    "admpc_argmin_groups": (I, [vp, dp, I, I, dp, ip, vp]),
}
_LANE = {       # include/admpc_lane.h: the fleet step along a route, a local lane per vehicle
    "admpc_waypoints_lane_batch": (I, [vp, C.POINTER(AdmpcLaneParams), I, ip, ip] + [dp] * 5 + [I, D, D] + [dp, dp, ip] + [vp]),
    "admpc_control_step_lane_batch": (I, [vp, vp, C.POINTER(AdmpcLaneParams), C.POINTER(AdmpcStepParams), I, ip, ip] + [dp] * 7 + [dp] * 5 + [vp] +
                                      [dp] * 4 + [dp, vp]),
}
_PLANT = {      # include/admpc_plant.h: the plant step, and T closed-loop steps along a route per call
    "admpc_plant_step_batch": (I, [vp, C.POINTER(AdmpcPlantParams), I, dp, ip] + [dp] * 7 + [vp]),
    "admpc_rollout_lane_batch": (I, [vp, vp, C.POINTER(AdmpcLaneParams), C.POINTER(AdmpcStepParams), vp, C.POINTER(AdmpcPlantParams), I, I, ip, ip] +
                                 [dp] * 7 + [dp] * 5 + [vp] + [dp] * 4 + [dp] + [dp, ip, dp, vp]),
}
EXPORTS, QUAD_EXPORTS, FLEET_EXPORTS, LANE_EXPORTS = tuple(_CAR), tuple(_QUAD), tuple(_FLEET), tuple(_LANE)
PLANT_EXPORTS = tuple(_PLANT)
op = C.POINTER(AdmpcObserveParams)
_LEARN = {      # include/admpc_learn.h: observe -> bin -> fit -> install of a handle's residual GP on the device
    "admpc_observe_latch_batch": (I, [I, I] + [dp] * 7 + [dp, vp]),
    "admpc_observe_batch": (I, [vp, C.POINTER(AdmpcPlantParams), op, I, dp, ip] + [dp] * 7 + [dp, dp, dp, ip, vp]),
    "admpc_gp_fit": (I, [I, op, I, dp, vp, ip, vp]),
    "admpc_gp_install": (I, [vp, I, vp, ip, vp]),
    "admpc_rollout_observe_lane_batch": (I, _PLANT["admpc_rollout_lane_batch"][1][:-1] + [vp, op, dp, dp, dp, ip, vp]),
}
LEARN_EXPORTS = tuple(_LEARN)
_HYPER = {      # include/admpc_hyper.h: the search of a regressor's hyperparameters on the device, and the fit at the optimum
    "admpc_gp_search": (I, [I, op, C.POINTER(AdmpcGpSearchParams), I, I, dp, dp, dp, ip, vp]),
    "admpc_gp_refit": (I, [I, op, I, dp, dp, vp, ip, vp]),
}
HYPER_EXPORTS = tuple(_HYPER)
pp = C.POINTER(AdmpcQuadPlantParams)
_QUAD_FLEET = {     # include/admpc_quad_fleet.h: the quadrotor's plant step, trajectory bank, reference window and closed-loop rollout
    "admpc_quad_plant_step_batch": (I, [pp, I, I, dp, C.c_int64, dp, vp]),
    "admpc_quad_traj_bank_create": (I, [I, I, fp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), hp]),
    "admpc_quad_traj_bank_destroy": (None, [vp]),
    "admpc_quad_ref_chunk_batch": (I, [vp, I, I, I, ip, ip, dp, dp, dp, vp]),
    "admpc_quad_rollout_batch": (I, [vp, vp, pp, I, I, I, ip, ip] + [dp] * 6 + [ip, ip, dp, ip, dp, dp, vp]),
    "admpc_quad_solver_info": (I, [vp, fp, fp, fp]),
}
QUAD_FLEET_EXPORTS = tuple(_QUAD_FLEET)
qop = C.POINTER(AdmpcQuadObserveParams)
_QUAD_LEARN = {     # include/admpc_quad_learn.h: observe -> bin -> fit -> install of a quadrotor handle's body-frame residual GPs
    "admpc_quad_observe_latch_batch": (I, [I, I, dp, dp, vp]),
    "admpc_quad_observe_batch": (I, [vp, pp, qop, I, dp, C.c_int64, dp, dp, dp, dp, ip, vp]),
    "admpc_quad_gp_fit": (I, [I, qop, I, dp, vp, ip, vp]),
    "admpc_quad_gp_install": (I, [vp, I, vp, ip, vp]),
    "admpc_quad_rollout_observe_batch": (I, _QUAD_FLEET["admpc_quad_rollout_batch"][1][:-1] + [vp, qop, dp, dp, dp, ip, vp]),
}
QUAD_LEARN_EXPORTS = tuple(_QUAD_LEARN)
# header under include/ -> its table: what load() declares, and what the arity test holds against the headers' own declarations
TABLES = {"admpc.h": _CAR, "admpc_quad.h": _QUAD, "admpc_fleet.h": _FLEET, "admpc_lane.h": _LANE, "admpc_plant.h": _PLANT,
          "admpc_learn.h": _LEARN, "admpc_hyper.h": _HYPER, "admpc_quad_fleet.h": _QUAD_FLEET, "admpc_quad_learn.h": _QUAD_LEARN}
# the headers behind the nine of TABLES, declared by load() in the same way
np_ = C.POINTER(AdmpcQuadNoiseParams)
_QUAD_NOISE = {     # include/admpc_quad_noise.h: the simulator's random disturbances: the draws, the noisy plant step, the noisy rollout
    "admpc_quad_noise_draw_batch": (I, [np_, I, I, I, ip, dp, ip, vp]),
    "admpc_quad_plant_step_noise_batch": (I, [pp, np_, I, I, dp, C.c_int64, dp, ip, vp]),
    "admpc_quad_rollout_noise_batch": (I, _QUAD_LEARN["admpc_quad_rollout_observe_batch"][1][:-1] + [np_, ip, vp]),
}
QUAD_NOISE_EXPORTS = tuple(_QUAD_NOISE)
MORE_TABLES = {"admpc_quad_noise.h": _QUAD_NOISE}
# the headers of what is built on the two registers above, declared by load() in the same way
_roll = _QUAD_FLEET["admpc_quad_rollout_batch"][1][:-1]
_QUAD_ENSEMBLE = {  # include/admpc_quad_ensemble.h: a clustered GP ensemble in the quadrotor's closed loop, flown and learned on the device
    "admpc_quad_ensemble_create": (I, [hp, I, I, fp, C.POINTER(C.c_double), qop, hp]),
    "admpc_quad_ensemble_destroy": (None, [vp]),
    "admpc_quad_ensemble_route_batch": (I, [vp, I, dp, ip, vp]),
    "admpc_quad_ensemble_observe_batch": (I, [vp, vp, pp, I, dp, C.c_int64, dp, dp, dp, dp, ip, vp]),
    "admpc_quad_ensemble_fit": (I, [vp, I, dp, vp, ip, vp]),
    "admpc_quad_ensemble_install": (I, [vp, vp, ip, vp]),
    "admpc_quad_ensemble_rollout_batch": (I, _roll + [ip, ip] + [vp, dp, dp, dp, ip] + [np_, ip, vp]),
}
QUAD_ENSEMBLE_EXPORTS = tuple(_QUAD_ENSEMBLE)
ENSEMBLE_TABLES = {"admpc_quad_ensemble.h": _QUAD_ENSEMBLE}
# what finds the centroids of such an ensemble, declared by load() in the same way
_QUAD_CLUSTERS = {  # include/admpc_quad_clusters.h: the logged rollout, the Gaussian-mixture EM, the install of its means, the re-bin
    "admpc_quad_ensemble_rollout_log_batch": (I, _QUAD_ENSEMBLE["admpc_quad_ensemble_rollout_batch"][1][:-1] + [dp, vp]),
    "admpc_quad_clusters_fit": (I, [vp, I, D, D, I, C.c_int64, dp, dp, dp, dp, dp, ip, vp]),
    "admpc_quad_clusters_install": (I, [vp, dp, ip, ip, ip, vp]),
    "admpc_quad_ensemble_centroids_set": (I, [vp, dp, ip, vp]),
    "admpc_quad_ensemble_centroids_get": (I, [vp, dp, vp]),
    "admpc_quad_clusters_rebin": (I, [vp, I, I, dp, dp, ip, vp]),
}
QUAD_CLUSTERS_EXPORTS = tuple(_QUAD_CLUSTERS)
CLUSTER_TABLES = {"admpc_quad_clusters.h": _QUAD_CLUSTERS}
# the search of the quadrotor's hyperparameters, one handle or a whole ensemble, declared by load() in the same way
sp_ = C.POINTER(AdmpcGpSearchParams)
_QUAD_HYPER = {     # include/admpc_quad_hyper.h: admpc_hyper.h's search and re-fit with the quadrotor's ranges, and for all clusters of an ensemble at once
    "admpc_quad_gp_search": (I, [I, qop, sp_, I, I, dp, dp, dp, ip, vp]),
    "admpc_quad_gp_refit": (I, [I, qop, I, dp, dp, vp, ip, vp]),
    "admpc_quad_ensemble_set_search": (I, [vp, sp_]),
    "admpc_quad_ensemble_search": (I, [vp, I, I, dp, dp, dp, ip, vp]),
    "admpc_quad_ensemble_refit": (I, [vp, I, dp, dp, vp, ip, vp]),
}
QUAD_HYPER_EXPORTS = tuple(_QUAD_HYPER)
HYPER_TABLES = {"admpc_quad_hyper.h": _QUAD_HYPER}
# flying to random targets and recording, declared by load() in the same way
tp_ = C.POINTER(AdmpcQuadTargetParams)
_QUAD_TARGETS = {   # include/admpc_quad_targets.h: the draw of a target, the reset, the window with the recovery, the plant step with the reach test, the observation with a period per vehicle, the rollout
    "admpc_quad_target_draw_batch": (I, [tp_, I, I, dp, C.c_int64, ip, dp, ip, vp]),
    "admpc_quad_targets_reset_batch": (I, [tp_, I, I, dp, dp, dp, ip, ip, ip, ip, vp]),
    "admpc_quad_target_window_batch": (I, [tp_, I, I, I, dp, dp, ip, ip, ip, ip, dp, dp, dp, vp]),
    "admpc_quad_plant_target_step_batch": (I, [pp, tp_, np_, I, I, dp, C.c_int64, dp, ip, dp, dp, ip, ip, ip, ip, ip, ip, vp]),
    "admpc_quad_observe_var_batch": (I, [vp, pp, qop, I, dp, C.c_int64, dp, dp, ip, dp, dp, ip, vp]),
    "admpc_quad_rollout_targets_batch": (I, [vp, pp, tp_, I, I] + [dp] * 6 + [ip, ip] + [dp, dp, ip, ip, ip, ip, ip] + [dp, dp, ip, dp] +
                                         [vp, qop, dp, dp, dp, ip] + [np_, ip, vp]),
}
QUAD_TARGETS_EXPORTS = tuple(_QUAD_TARGETS)
TARGET_TABLES = {"admpc_quad_targets.h": _QUAD_TARGETS}
# pruning the log and the RDRv drag fit, declared by load() in the same way
_QUAD_PRUNE = {     # include/admpc_quad_prune.h: the flags of a log rewritten by the reference's prune_dataset, the linear drag fitted from what is left, its install
    "admpc_quad_records_prune": (I, [I, C.c_int64, dp, D, I, D, dp, dp, ip, ip, vp]),
    "admpc_quad_rdrv_fit": (I, [I, C.c_int64, I, dp, dp, dp, dp, ip, vp]),
    "admpc_quad_rdrv_install": (I, [vp, dp, ip, ip, vp]),
}
QUAD_PRUNE_EXPORTS = tuple(_QUAD_PRUNE)
PRUNE_TABLES = {"admpc_quad_prune.h": _QUAD_PRUNE}
# the evaluation of the learned GPs on a log, declared by load() in the same way
_QUAD_EVAL = {      # include/admpc_quad_eval.h: every regressor of an ensemble factored once (K = L L', alpha, W = L^-1), posterior mean and standard deviation per record of a log, the error statistics per cluster and regressor
    "admpc_quad_ensemble_factor": (I, [vp, I, dp, dp, dp, ip, vp]),
    "admpc_quad_ensemble_evaluate": (I, [vp, C.c_int64, dp, I, dp, dp, dp, dp, dp, ip, vp]),
}
QUAD_EVAL_EXPORTS = tuple(_QUAD_EVAL)
EVAL_TABLES = {"admpc_quad_eval.h": _QUAD_EVAL}
# the loop and lemniscate references generated on the device, declared by load() in the same way
tsp_ = C.POINTER(AdmpcQuadTrajSpec)
_QUAD_TRAJ = {      # include/admpc_quad_traj.h: the phase lengths on the host, a generated bank, what it holds, a trajectory read back, the rows of a fleet's reset
    "admpc_quad_traj_lengths": (I, [D, tsp_, fp]),
    "admpc_quad_traj_bank_generate": (I, [I, I, tsp_, pp, D, vp, hp]),
    "admpc_quad_traj_bank_info": (I, [vp, fp, C.POINTER(C.c_int64), fp]),
    "admpc_quad_traj_bank_copy": (I, [vp, I, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "admpc_quad_traj_rows_batch": (I, [vp, I, ip, ip, dp, dp, vp]),
}
QUAD_TRAJ_EXPORTS = tuple(_QUAD_TRAJ)
TRAJ_TABLES = {"admpc_quad_traj.h": _QUAD_TRAJ}
# references through keyframes generated on the device, declared by load() in the same way
hd_ = C.POINTER(C.c_double)
_QUAD_POLY_TRAJ = {  # include/admpc_quad_poly_traj.h: s and M on the host, the fit's weight matrix on the host, a bank of piecewise polynomials through keyframes
    "admpc_quad_poly_traj_lengths": (I, [D, I, hd_, D, fp, fp]),
    "admpc_quad_poly_traj_weights": (I, [I, hd_]),
    "admpc_quad_poly_traj_bank_generate": (I, [I, I, I, hd_, hd_, pp, D, vp, hp]),
}
QUAD_POLY_TRAJ_EXPORTS = tuple(_QUAD_POLY_TRAJ)
POLY_TRAJ_TABLES = {"admpc_quad_poly_traj.h": _QUAD_POLY_TRAJ}
# the training points of every regressor picked from the log, declared by load() in the same way
_QUAD_SELECT = {    # include/admpc_quad_select.h: per (cluster, regressor, bin) the median record of the reference's distance_maximizing_points_1d, into the bins the fit reads
    "admpc_quad_ensemble_select_points": (I, [vp, C.c_int64, dp, fp, ip, dp, ip, dp, ip, ip, vp]),
}
QUAD_SELECT_EXPORTS = tuple(_QUAD_SELECT)
SELECT_TABLES = {"admpc_quad_select.h": _QUAD_SELECT}

# solver_type "SQP" inside the one-wave solve kernel, declared by load() in the same way
_QUAD_SQP = {       # include/admpc_quad_sqp.h: the mode of a handle, what it holds, the solve with the QPs per instance
    "admpc_quad_set_sqp": (I, [vp, I, D]),
    "admpc_quad_get_sqp": (I, [vp, fp, C.POINTER(C.c_double)]),
    "admpc_quad_solve_batch_sqp": (I, [vp, I, dp, dp, dp, dp, dp, dp, dp, ip, ip, ip, vp]),
}
QUAD_SQP_EXPORTS = tuple(_QUAD_SQP)
SQP_TABLES = {"admpc_quad_sqp.h": _QUAD_SQP}

# the start of the Gaussian-mixture EM found on the device, declared by load() in the same way
_QUAD_KMEANS = {    # include/admpc_quad_kmeans.h: scikit-learn's k-means++ seeding and Lloyd k-means over the log, the n_init rule over two fits
    "admpc_quad_kmeans_fit": (I, [vp, C.c_uint64, C.c_uint32, I, D, C.c_int64, dp, dp, dp, ip, dp, dp, ip, dp, ip, vp]),
    "admpc_quad_clusters_keep": (I, [vp, I, dp, ip, dp, ip, ip, vp]),
    "admpc_quad_kmeans_keep": (I, [vp, I, C.c_int64, ip, dp, ip, ip, dp, ip, dp, ip, ip, dp, ip, vp]),
}
QUAD_KMEANS_EXPORTS = tuple(_QUAD_KMEANS)
KMEANS_TABLES = {"admpc_quad_kmeans.h": _QUAD_KMEANS}

_lib = None


class AdmpcError(RuntimeError):
    pass


def load():
    """dlopen libadmpc.so and declare the prototypes of the headers under include/ (no GPU needed for this)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AdmpcError("%s not found: build it with `make -C ad_mpc_amd/csrc` (or __graft_entry__.build()); "
                         "there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for table in list(TABLES.values()) + list(MORE_TABLES.values()) + list(ENSEMBLE_TABLES.values()) + list(CLUSTER_TABLES.values()) + \
            list(HYPER_TABLES.values()) + list(TARGET_TABLES.values()) + list(PRUNE_TABLES.values()) + list(EVAL_TABLES.values()) + \
            list(TRAJ_TABLES.values()) + list(POLY_TRAJ_TABLES.values()) + list(SELECT_TABLES.values()) + \
            list(SQP_TABLES.values()) + list(KMEANS_TABLES.values()):
        for name, (restype, argtypes) in table.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise AdmpcError("libadmpc error %d: %s" % (rc, load().admpc_last_error().decode()))
