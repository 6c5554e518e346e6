"""A fleet of quadrotors that flies -- and learns -- a clustered GP ensemble in closed loop on the device
(include/admpc_quad_ensemble.h): the reference keeps one solver per cluster of its GP ensemble (quad_3d_optimizer.py:207) and picks one
per solve from the first row of the reference chunk (:485-491, gp.py:738-770); here one handle per cluster solves the vehicles whose
window routes to it, in every period of a rollout, and the steps flown go to the bins of the cluster they were flown in.  The plant,
the bank, reset, the disturbances and the tally are ``QuadFleet``'s."""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .config import AdmpcGp, AdmpcGpSearchParams, GP_HYPER, GP_MAX_POINTS, GP_SEARCH_MAX, search_boxes
from .engine import QuadBatchSolver, _ptr
from .learning import decode_gps, hyper_dicts, placeholder_gps
from .quad_3d_optimizer import QuadGPEnsemble
from .quad_config import QNX, QNY, QUAD_GP_MAX, QUAD_REC, AdmpcQuadObserveParams, quad_learn_bins, select_request
from .quad_fleet import QuadFleet, fleet_quad_config, fleet_solver_type

QuadEnsembleRollout = namedtuple("QuadEnsembleRollout", ("x", "idx", "tally", "counts", "traj", "u", "routes"))
QuadClusters = namedtuple("QuadClusters", ("weights", "means", "covariances", "n_iter", "converged", "status", "perm"))
QuadEvaluation = namedtuple("QuadEvaluation", ("count", "nominal_mae", "augmented_mae", "nominal_rms", "augmented_rms", "mean_std", "within_3std",
                                               "clipped", "total"))
QuadKMeans = namedtuple("QuadKMeans", ("centers", "idx", "labels", "n_iter", "converged", "status", "n_valid", "inertia", "tol_abs", "shift",
                                       "potential", "kept"))
CLUSTERS_MAX = 8
GMM_BLOCKS_MAX, GMM_ROW, GMM_PARTIAL, GMM_ENOVALID = 256, 18, 81, -100                  # include/admpc_quad_clusters.h
KMEANS_PARTIAL, KMEANS_STATE, KMEANS_EFEW, KMEANS_N_INIT_MAX = 33, 48, -101, 64      # include/admpc_quad_kmeans.h; the last is this layer's
PRUNE_BINS_MAX, PRUNE_PARTIAL, RDRV_PARTIAL, PRUNE_ENOVALID, REC_PRUNED = 256, 9, 7, -100, 2.0        # include/admpc_quad_prune.h
EVAL_FACTOR, EVAL_STATS, EVAL_ENOVALID = 672, 8, -100                                    # include/admpc_quad_eval.h
SELECT_WORK, SELECT_ENOVALID = 201376, -100                                              # include/admpc_quad_select.h


def ensemble_layout(centroids, feats, learn=None):
    """The centroids as float64 [K, n_feat] and the features as a list, checked as admpc_quad_ensemble_create checks them, and with
    ``learn`` (K lists of quad_learn_bins dicts) the K blocks of regressors: (centroids, feats, [(AdmpcGpBins array, n_gp)] or None).
    Raises ValueError; needs no GPU."""
    feats = [int(f) for f in np.atleast_1d(feats).reshape(-1)]
    if not 1 <= len(feats) <= 3 or any(not 0 <= f < QNY for f in feats):
        raise ValueError("QuadEnsembleFleet: 1 to 3 clustering features in 0 .. 16")
    cent = np.asarray(centroids, dtype=np.float64)
    if cent.ndim == 1:
        cent = cent.reshape(-1, len(feats))
    K = cent.shape[0]
    if not 1 <= K <= CLUSTERS_MAX:
        raise ValueError("QuadEnsembleFleet: 1 to %d clusters, got %d" % (CLUSTERS_MAX, K))
    if cent.shape != (K, len(feats)):
        raise ValueError("QuadEnsembleFleet: centroids must be K x len(feats)")
    if not np.isfinite(cent).all():
        raise ValueError("QuadEnsembleFleet: a centroid is not finite")
    if learn is None:
        return np.ascontiguousarray(cent), feats, None
    learn = [[dict(d) for d in cluster] for cluster in learn]
    if len(learn) != K:
        raise ValueError("QuadEnsembleFleet: learn needs one list of regressors per cluster (%d), got %d" % (K, len(learn)))
    blocks = [quad_learn_bins(cluster) for cluster in learn]                               # ValueError on bad bins
    head = lambda cluster: [([int(f) for f in np.atleast_1d(d["feat"]).reshape(-1)], int(d["out"])) for d in cluster]
    for c in range(1, K):
        if head(learn[c]) != head(learn[0]):
            raise ValueError("QuadEnsembleFleet: the clusters of learn must agree in every regressor's feat and out (cluster %d differs); "
                             "the box, the bins and the hyperparameters may differ" % c)
    if min(feats) < 7:
        raise ValueError("QuadEnsembleFleet: a fleet that learns clusters on features in 7 .. 16 (the sample record holds no others)")
    return np.ascontiguousarray(cent), feats, blocks


def log_layout(log_steps, learns):
    """``log_steps`` of the constructor, checked: 0, or the steps the sample log holds in a fleet that learns.  Raises ValueError; needs
    no GPU."""
    steps = int(log_steps)
    if steps < 0 or steps != log_steps:
        raise ValueError("QuadEnsembleFleet: log_steps must be a whole number and not negative")
    if steps and not learns:
        raise ValueError("QuadEnsembleFleet: a sample log (log_steps) needs a fleet that learns: give centroids, feats and learn")
    return steps


def clusters_request(K, feats, steps, max_iter=100, tol=1e-3, reg_covar=1e-6, init=None):
    """The arguments of ``fit_clusters`` checked as admpc_quad_clusters_fit checks them, for K clusters on ``feats`` and a log that holds
    ``steps`` steps: (max_iter, tol, reg_covar, init as float64 [K, len(feats)] or None).  Raises ValueError; needs no GPU."""
    if min(feats) < 7:
        raise ValueError("fit_clusters: the clustering features must lie in 7 .. 16 (the sample record holds no others)")
    if int(steps) < 1:
        raise ValueError("fit_clusters: the log is empty: fly rollout(T, observe=True, log=True) first")
    if int(max_iter) != max_iter or not 1 <= int(max_iter) <= 1000:
        raise ValueError("fit_clusters: max_iter must be in 1 .. 1000")
    tol, reg_covar = float(tol), float(reg_covar)
    if not tol >= 0.0:
        raise ValueError("fit_clusters: tol must not be negative")
    if not (reg_covar >= 0.0 and np.isfinite(reg_covar)):
        raise ValueError("fit_clusters: reg_covar must be finite and not negative")
    if init is not None:
        init = centroid_block("fit_clusters: init", init, K, len(feats))
    return int(max_iter), tol, reg_covar, init


def kmeans_work(M):
    """The doubles of admpc_quad_kmeans_fit's work area for M records (ADMPC_KMEANS_WORK)."""
    return 2 * ((int(M) + 255) // 256) + GMM_BLOCKS_MAX * KMEANS_PARTIAL + KMEANS_STATE


def kmeans_request(seed, n_init=1, km_max_iter=300, km_tol=1e-4, resume=False):
    """The arguments ``fit_clusters`` takes with init="kmeans", checked as admpc_quad_kmeans_fit checks them:
    (seed, n_init, km_max_iter, km_tol).  Raises ValueError; needs no GPU."""
    if seed is None:
        raise ValueError("fit_clusters: init=\"kmeans\" needs a seed")
    if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("fit_clusters: seed must be a whole number in 0 .. 2^64 - 1")
    if isinstance(n_init, (bool, np.bool_)) or int(n_init) != n_init or not 1 <= int(n_init) <= KMEANS_N_INIT_MAX:
        raise ValueError("fit_clusters: n_init must be in 1 .. %d" % KMEANS_N_INIT_MAX)
    if int(km_max_iter) != km_max_iter or not 1 <= int(km_max_iter) <= 1000:
        raise ValueError("fit_clusters: km_max_iter must be in 1 .. 1000")
    km_tol = float(km_tol)
    if not (km_tol >= 0.0 and np.isfinite(km_tol)):
        raise ValueError("fit_clusters: km_tol must be finite and not negative")
    if resume:
        raise ValueError("fit_clusters: resume=True goes on from the last fit; init=\"kmeans\" starts a new one")
    return int(seed), int(n_init), int(km_max_iter), km_tol


def prune_request(steps, x_cap=16.0, bins=40, thresh=0.001):
    """The arguments of ``prune_log`` checked as admpc_quad_records_prune checks them, for a log that holds ``steps`` steps: (x_cap with
    None as +inf, bins, thresh).  Raises ValueError; needs no GPU."""
    if int(steps) < 1:
        raise ValueError("prune_log: the log is empty: fly rollout(T, observe=True, log=True) first")
    if int(bins) != bins or not 1 <= int(bins) <= PRUNE_BINS_MAX:
        raise ValueError("prune_log: bins must be in 1 .. %d" % PRUNE_BINS_MAX)
    thresh = float(thresh)
    if not 0.0 <= thresh <= 1.0:
        raise ValueError("prune_log: thresh must be in [0, 1]")
    x_cap = float("inf") if x_cap is None else float(x_cap)
    if not x_cap > 0.0:
        raise ValueError("prune_log: x_cap must be positive, or None for no cap")
    return x_cap, int(bins), thresh


def eval_request(log_steps, steps, has_factor, include_pruned=False, drag=False, has_rdrv=False, per_record=False):
    """The arguments of ``evaluate_log`` checked before any launch, for a fleet whose log holds ``steps`` of ``log_steps`` steps, with
    (``has_factor``) a factor from fit_gp(factor=True), search_gp(factor=True) or factor_gp(), and (``has_rdrv``) a drag from fit_rdrv:
    (take_pruned 0 or 1, drag, per_record).  Raises ValueError; needs no GPU."""
    if int(log_steps) < 1:
        raise ValueError("evaluate_log: this fleet keeps no log, create it with log_steps")
    if int(steps) < 1:
        raise ValueError("evaluate_log: the log is empty: fly rollout(T, observe=True, log=True) first")
    if not has_factor:
        raise ValueError("evaluate_log: no factor yet: call fit_gp(factor=True), search_gp(factor=True) or factor_gp() first")
    for name, v in (("include_pruned", include_pruned), ("drag", drag), ("per_record", per_record)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError("evaluate_log: %s must be True or False" % name)
    if drag and not has_rdrv:
        raise ValueError("evaluate_log: drag=True needs the drag of a fit_rdrv() first")
    return (1 if include_pruned else 0), bool(drag), bool(per_record)


def evaluation_table(stats, n, dt=None):
    """stats [K, 3, 8] of admpc_quad_ensemble_evaluate as a ``QuadEvaluation`` of [K, n] arrays, whose ``total`` is the same over all
    clusters per regressor ([n], its own total None); with ``dt`` the errors and the standard deviation are multiplied by it (the
    reference's velocity units).  A cluster without a record has count 0 and NaN elsewhere.  Needs no GPU."""
    def table(s):
        cnt = s[..., 0]
        scale = 1.0 if dt is None else float(dt)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (cnt.astype(np.int64), scale * s[..., 1] / cnt, scale * s[..., 3] / cnt, scale * np.sqrt(s[..., 2] / cnt),
                    scale * np.sqrt(s[..., 4] / cnt), scale * s[..., 5] / cnt, s[..., 6] / cnt, s[..., 7].astype(np.int64))
    s = np.asarray(stats, dtype=np.float64)[:, :n]
    return QuadEvaluation(*table(s), QuadEvaluation(*table(s.sum(axis=0)), None))


def rdrv_axes(axes):
    """``axes`` of ``fit_rdrv`` -- the reference's features, a subset of (7, 8, 9) -- as the 3-bit mask of admpc_quad_rdrv_fit.  Raises
    ValueError; needs no GPU."""
    axes = [int(a) for a in np.atleast_1d(axes).reshape(-1)]
    if not axes or any(not 7 <= a <= 9 for a in axes) or len(set(axes)) != len(axes):
        raise ValueError("fit_rdrv: axes must be a subset of (7, 8, 9) without repeats, and not empty")
    return sum(1 << (a - 7) for a in axes)


def centroid_block(who, c, K, d):
    """c as float64 [K, d], finite.  Raises ValueError; needs no GPU."""
    c = np.asarray(c, dtype=np.float64)
    if c.ndim == 1 and d == 1:
        c = c.reshape(-1, 1)
    if c.shape != (K, d):
        raise ValueError("%s must be K x len(feats) = %d x %d" % (who, K, d))
    if not np.isfinite(c).all():
        raise ValueError("%s: a centroid is not finite" % who)
    return np.ascontiguousarray(c)


class QuadEnsembleFleet(QuadFleet):
    """``QuadFleet`` with one handle per cluster.  Either ``ensemble`` (a ``QuadGPEnsemble``: the fleet flies given clusters) or
    ``centroids`` [K, n_feat], ``feats`` and ``learn`` -- K lists of ``quad_learn_bins`` dicts, one list per cluster, which agree in feat
    and out and are free in the box, the bins and the hyperparameters -- for a fleet that learns them: every cluster's handle is created
    with placeholder GPs, one nominal handle predicts for observe.

    State besides QuadFleet's: ``route`` int32 [B] (the clusters of the last period), and with ``learn`` ``bins`` [K,3,32,5],
    ``dropped`` [K,4] ([c][g]: valid records of cluster c outside regressor g's box; [0][3]: records that are not valid), ``fit_info``
    and ``installed`` [K,3].  There is ONE iterate per vehicle: a vehicle that changes cluster is warm-started from the other cluster's
    solution (the reference keeps an iterate per solver).

    With ``log_steps`` a fleet that learns also keeps the records it flies, ``log`` [log_steps,B,14] on the device with a cursor
    ``log_count`` on the host, and finds its centroids from them (include/admpc_quad_clusters.h): ``rollout(T, observe=True, log=True)``
    -> ``prune_log()`` -> ``fit_clusters()`` -> ``fit_gp()`` -> ``rollout(...)``.  ``prune_log()`` is the reference's prune_dataset over the
    log (include/admpc_quad_prune.h): it rewrites flags, which every later stage reads; ``fit_rdrv()`` learns the linear drag from the
    records that are left, in place of the GPs or under them.  Cluster c keeps the box and the hyperparameters of ``learn[c]``; ``search_gp()``
    in place of ``fit_gp()`` finds the length scales, sigma_f and the noise of every cluster from the data it holds now
    (include/admpc_quad_hyper.h), all on the same stream.  ``hyper`` [K,3,16] and ``search_info`` [K,3,2] are the state of that search.

    The chain closes with the evaluation of what was learned (include/admpc_quad_eval.h): ``fit_gp(factor=True)`` or
    ``search_gp(factor=True)`` -> ``log_reset()`` -> ``rollout(T, observe=True, log=True)`` again -> ``evaluate_log()`` -> ``evaluation()``.
    ``factor`` [K,3,672] holds every regressor factored once (alpha and W = L^-1), ``eval_stats`` [K,3,8] and ``eval_info`` [4] the sums
    and the counts of the last evaluation, ``eval_per_record`` the mean and the standard deviation of every record once asked for.

    Between the clusters and the fit, ``select_points()`` trains every GP on real records picked from the log as the reference picks
    them, in place of the bin means (include/admpc_quad_select.h): ``rollout(T, observe=True, log=True)`` -> ``prune_log()`` ->
    ``fit_clusters()`` -> ``select_points()`` -> ``search_gp(factor=True)`` -> ``evaluate_log()``.  ``sel`` [K,3,32] and ``select_info``
    [K,3,4] are its results; it overwrites ``bins``, which ``rebin()`` restores.

    ``fit_clusters(init="kmeans", seed=...)`` needs no centroids to start from: scikit-learn's k-means++ seeding and Lloyd k-means run on
    the device in front of the EM (include/admpc_quad_kmeans.h), as the reference's GaussianMixture(n_clusters).fit does by default;
    ``km_centers``, ``km_idx``, ``km_info``, ``km_stats``, ``km_labels`` and ``km_kept`` hold its results, ``learned_kmeans()`` reads them."""

    def __init__(self, B, quad=None, t_horizon=1.0, n_nodes=10, q_cost=None, r_cost=None, simulation_dt=5e-4, reference_over_sampling=5,
                 ensemble=None, centroids=None, feats=None, learn=None, rdrv_d_mat=None, device=0, observe_substeps=1, noise_seed=None,
                 log_steps=0, solver_type="SQP_RTI"):
        self._ens = None
        self._solvers = []
        fleet_solver_type("QuadEnsembleFleet", solver_type, n_nodes, None, offered=("SQP_RTI",))      # "SQP": refused, routed solves do not serve it
        self._init_plant(B, quad, t_horizon, n_nodes, simulation_dt, reference_over_sampling, noise_seed)
        # every refusal that needs no GPU, before a handle exists
        if (ensemble is None) == (learn is None):
            raise ValueError("QuadEnsembleFleet: give either ensemble=QuadGPEnsemble(...) or centroids, feats and learn")
        if ensemble is not None:
            if centroids is not None or feats is not None:
                raise ValueError("QuadEnsembleFleet: centroids and feats come with the ensemble")
            cent, feats, blocks = ensemble_layout(ensemble.centroids, ensemble.feats)
            clusters = [list(c) for c in ensemble.clusters]
            if len(clusters) != cent.shape[0]:
                raise ValueError("QuadEnsembleFleet: the ensemble needs one centroid per cluster")
        else:
            if centroids is None or feats is None:
                raise ValueError("QuadEnsembleFleet: learn needs centroids and feats")
            cent, feats, blocks = ensemble_layout(centroids, feats, learn)
            learn = [[dict(d) for d in cluster] for cluster in learn]
            if not 1 <= int(observe_substeps) <= 64:
                raise ValueError("QuadEnsembleFleet: observe_substeps must be in [1, 64]")
            clusters = [placeholder_gps(cluster) for cluster in learn]
        self.log_steps, self.log_count, self.log = log_layout(log_steps, learn is not None), 0, None
        self.K, self.feats, self.centroids = cent.shape[0], feats, cent
        self._moved = False                                                                # the device's centroids are no longer self.centroids
        self._rdrv_given = rdrv_d_mat is not None and bool(np.any(np.asarray(rdrv_d_mat, dtype=np.float64) != 0.0))
        cfgs = [fleet_quad_config(quad, t_horizon, n_nodes, q_cost, r_cost, gps, rdrv_d_mat) for gps in clusters]      # one configuration per cluster
        if learn is not None:
            self._nominal = QuadBatchSolver(fleet_quad_config(quad, t_horizon, n_nodes, q_cost, r_cost, None, rdrv_d_mat), device=device)
        self._solvers = [QuadBatchSolver(c, device=device) for c in cfgs]
        self._eng = self._solvers[0]                                                       # the stream, the device and the checks of the fleet
        self._handles = (C.c_void_p * self.K)(*[s._h for s in self._solvers])
        obs = None
        if learn is not None:
            obs = (AdmpcQuadObserveParams * self.K)()
            for c, (bins, n_gp) in enumerate(blocks):
                obs[c] = AdmpcQuadObserveParams(dt=self.control_period, substeps=int(observe_substeps), n_gp=n_gp, gp=bins)
        h = C.c_void_p(0)
        _lib.check(_lib.load().admpc_quad_ensemble_create(self._handles, self.K, len(feats), (C.c_int32 * len(feats))(*feats),
                                                          cent.ctypes.data_as(C.POINTER(C.c_double)), obs, C.byref(h)))
        self._ens = h
        self._alloc_state(self._solvers)
        self.route = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        if learn is not None:
            z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=self.device)
            self._learn, self.n_learn, self._obs, self._observer = learn, blocks[0][1], obs, self._nominal
            self._prev, self.samples = z(self.B, QNX), z(self.B, QUAD_REC)
            self.bins, self.dropped = z(self.K, QUAD_GP_MAX, GP_MAX_POINTS, 5), z(self.K, QUAD_GP_MAX + 1, dtype=torch.int32)
            self._gp_dev = z(self.K * QUAD_GP_MAX * C.sizeof(AdmpcGp), dtype=torch.uint8)
            self.fit_info, self.installed = z(self.K, QUAD_GP_MAX, dtype=torch.int32), z(self.K, QUAD_GP_MAX, dtype=torch.int32)
            # the hyperparameter search of all clusters (search_gp): its state, the scratch, the last round's picks, and the parameters
            # the object holds (set_search is synchronous, so it is called only when they change)
            self.hyper, self._nll = z(self.K, QUAD_GP_MAX, GP_HYPER), z(self.K, QUAD_GP_MAX, GP_SEARCH_MAX)
            self.search_info = z(self.K, QUAD_GP_MAX, 2, dtype=torch.int32)
            self._has_hyper = self._searched = False
            self._search_set = None
        # the centroids on their way to and from the object, and what the clustering works in
        self._cent_dev = torch.as_tensor(cent).to(self.device)
        self.centroids_installed = torch.ones(1, dtype=torch.int32, device=self.device)
        if self.log_steps:
            self.log = z(self.log_steps, self.B, QUAD_REC)
            self._packed, self._partial = z(self.log_steps * self.B, 4), z(GMM_BLOCKS_MAX, GMM_PARTIAL)
            self.gmm, self.gmm_info = z(1 + self.K, GMM_ROW), z(4, dtype=torch.int32)
            self.perm = torch.arange(self.K, dtype=torch.int32, device=self.device)
            # the prune and the drag fit (include/admpc_quad_prune.h): scratch, state and results
            self._prune_partial, self._rdrv_partial = z(GMM_BLOCKS_MAX, PRUNE_PARTIAL), z(GMM_BLOCKS_MAX, RDRV_PARTIAL)
            self.prune_edges, self.prune_counts = z(4, PRUNE_BINS_MAX + 1), z(4, PRUNE_BINS_MAX, dtype=torch.int32)
            self.prune_info = z(8, dtype=torch.int32)
            self.rdrv, self.rdrv_sums, self.rdrv_info = z(3), z(3, 2), z(2, dtype=torch.int32)
            self.rdrv_installed = z(self.K, dtype=torch.int32)
            # the evaluation of the learned GPs on the log (include/admpc_quad_eval.h): the factors, scratch, results; per_record [M,3,2]
            # is allocated when it is first asked for
            self.factor, self.factor_info = z(self.K, QUAD_GP_MAX, EVAL_FACTOR), z(self.K, QUAD_GP_MAX, dtype=torch.int32)
            self._eval_partial, self.eval_stats = z(GMM_BLOCKS_MAX, self.K * QUAD_GP_MAX * EVAL_STATS), z(self.K, QUAD_GP_MAX, EVAL_STATS)
            self.eval_info, self.eval_per_record = z(4, dtype=torch.int32), None
            self._has_factor = self._has_rdrv = self._evaluated = False
            # the training points picked from the log (include/admpc_quad_select.h): the work area, the edges, results
            self._blocks = blocks
            self._select_code, self._select_work = z(self.log_steps * self.B, dtype=torch.int32), z(SELECT_WORK, dtype=torch.int32)
            self.select_edges = z(self.K, QUAD_GP_MAX, GP_MAX_POINTS + 1)
            self.sel = torch.full((self.K, QUAD_GP_MAX, GP_MAX_POINTS), -1, dtype=torch.int32, device=self.device)
            self.select_info = z(self.K, QUAD_GP_MAX, 4, dtype=torch.int32)

    # -- lifetime ---------------------------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ens", None):
            self.lib.admpc_quad_ensemble_destroy(self._ens)
            self._ens = None
        for s in getattr(self, "_solvers", [])[1:]:
            s.close()
        super().close()                                                                    # the bank, handle 0 and the nominal handle

    def _targets_offered(self, who):
        raise ValueError("%s: clustered ensembles do not chase targets (include/admpc_quad_targets.h: not offered); QuadFleet does" % who)

    # -- routing and the routed solve, for a loop driven from the host ------------------------------------------------------------------
    def route_window(self, route=None):
        """The cluster of every vehicle from row 0 of its window ``yref`` as it stands (admpc_quad_ensemble_route_batch), into ``route``
        (default: the fleet's).  Asynchronous."""
        route = self.route if route is None else route
        self._eng._chk(route, (self.B,), torch.int32)
        _lib.check(self.lib.admpc_quad_ensemble_route_batch(self._ens, self.B, _ptr(self.yref), _ptr(route), self._stream()))
        return route

    def solve_routed(self, route=None):
        """One RTI step of every vehicle by the handle of its cluster, in place on the fleet's iterate
        (admpc_quad_solve_batch_routed under ``route``, default the fleet's).  Asynchronous."""
        route = self.route if route is None else route
        self._eng._chk(route, (self.B,), torch.int32)
        _lib.check(self.lib.admpc_quad_solve_batch_routed(self._handles, self.K, self.B, _ptr(route), _ptr(self.x), _ptr(self.yref), _ptr(self.yref_e),
                                                          None, _ptr(self.x_opt), _ptr(self.w_opt), _ptr(self.cost), _ptr(self.status),
                                                          _ptr(self.iters), self._stream()))

    # -- the closed loop --------------------------------------------------------------------------------------------------------------
    def rollout(self, T, record=False, observe=False, log=False):
        """T closed-loop steps (admpc_quad_ensemble_rollout_batch): window -> routing from the window -> routed solve -> plant, and with
        `observe` the ensemble's observation behind every plant step.  With `log` (which needs `observe`) the records of the T steps are
        appended to ``log`` (admpc_quad_ensemble_rollout_log_batch; ValueError if they do not fit).  Returns QuadEnsembleRollout(x, idx,
        tally, counts, traj, u, routes): QuadRollout's fields, and with record routes int32 [T,B], the cluster that solved every vehicle
        in every step."""
        self._need_bank("rollout")
        if observe:
            self._learns("rollout")
        if log:
            if not observe:
                raise ValueError("rollout: log=True needs observe=True (logging implies observing)")
            if int(T) > self.log_steps - self.log_count:
                raise ValueError("rollout: %d steps do not fit into the log (log_steps = %d, %d of them taken); log_reset() empties it"
                                 % (int(T), self.log_steps, self.log_count))
        T, traj, u = self._records("rollout", T, record)
        routes = torch.empty((T, self.B), dtype=torch.int32, device=self.device) if record else None
        watch = (self._observer._h, _ptr(self._prev), _ptr(self.samples), _ptr(self.bins), _ptr(self.dropped)) if observe else (None,) * 5
        noise = (C.byref(self._noise), _ptr(self.noise_step)) if self._noise is not None else (None, None)
        if log and T > 0:
            at = C.c_void_p(self.log.data_ptr() + self.log_count * self.B * QUAD_REC * 8)
            _lib.check(self.lib.admpc_quad_ensemble_rollout_log_batch(*self._rollout_args(self._ens, T, traj, u), _ptr(self.route), _ptr(routes),
                                                                      *watch, *noise, at, self._stream()))
            self.log_count += T
        else:
            _lib.check(self.lib.admpc_quad_ensemble_rollout_batch(*self._rollout_args(self._ens, T, traj, u), _ptr(self.route), _ptr(routes),
                                                                  *watch, *noise, self._stream()))
        return QuadEnsembleRollout(self.x, self.idx, self.tally, self.counts, traj, u, routes)

    # -- the centroids: given, or found from the log -----------------------------------------------------------------------------------------
    def log_reset(self):
        """Empties the sample log (the cursor; the tensor is not touched)."""
        self.log_count = 0

    def set_centroids(self, c):
        """c [K, n_feat] into the ensemble's device centroids, on the stream (admpc_quad_ensemble_centroids_set): routing and the bin
        kernel use them from the next launch on, a captured rollout at its next replay.  Asynchronous; returns the device tensor
        ``centroids_installed`` int32 [1].  Bins filled under the old centroids are the caller's to zero (or ``rebin``)."""
        self._cent_dev.copy_(torch.as_tensor(centroid_block("set_centroids: c", c, self.K, len(self.feats))))
        _lib.check(self.lib.admpc_quad_ensemble_centroids_set(self._ens, _ptr(self._cent_dev), _ptr(self.centroids_installed), self._stream()))
        self._moved = True
        return self.centroids_installed

    def _device_centroids(self):
        """self.centroids refreshed from the device once an install or set_centroids has moved them (synchronises)."""
        if self._moved:
            _lib.check(self.lib.admpc_quad_ensemble_centroids_get(self._ens, _ptr(self._cent_dev), self._stream()))
            torch.cuda.current_stream(self.device).synchronize()
            self.centroids = self._cent_dev.cpu().numpy().copy()
        return self.centroids

    def rebin(self):
        """bins and dropped zeroed, then the logged steps binned under the present centroids (admpc_quad_clusters_rebin).  Asynchronous."""
        self._learns("rebin")
        self.bins.zero_()
        self.dropped.zero_()
        if self.log_count:
            _lib.check(self.lib.admpc_quad_clusters_rebin(self._ens, self.log_count, self.B, _ptr(self.log), _ptr(self.bins), _ptr(self.dropped),
                                                          self._stream()))

    def prune_log(self, x_cap=16.0, bins=40, thresh=0.001, rebin=True):
        """The reference's prune_dataset over the logged steps (admpc_quad_records_prune; the defaults are its ModelFitConfig, x_cap=None
        is no cap): a record behind the velocity cap or in a sparse bin of one of the four error histograms leaves with flag 2.0, every
        other valid one with 1.0, so that ``fit_clusters``, ``rebin``, ``fit_gp`` and ``search_gp`` see what is left; then (`rebin`) the
        log binned again.  The result depends on the data alone: a second call with other parameters prunes afresh.  Asynchronous;
        returns the device tensor info int32 [8]: status, n_valid, n_kept, pruned by the cap, by axis 0, 1, 2, by the norm."""
        self._learns("prune_log")
        if not self.log_steps:
            raise ValueError("prune_log: this fleet keeps no log, create it with log_steps")
        x_cap, bins, thresh = prune_request(self.log_count, x_cap, bins, thresh)
        _lib.check(self.lib.admpc_quad_records_prune(self.device_index, self.log_count * self.B, _ptr(self.log), x_cap, bins, thresh,
                                                     _ptr(self._prune_partial), _ptr(self.prune_edges), _ptr(self.prune_counts),
                                                     _ptr(self.prune_info), self._stream()))
        if rebin:
            self.rebin()
        return self.prune_info

    def select_points(self, n_points=None):
        """The training points of every regressor of every cluster picked from the logged records, as the reference's
        distance_maximizing_points_1d picks them (admpc_quad_ensemble_select_points; include/admpc_quad_select.h has the rule): a
        histogram of ``n_points`` bins over the feature values of the cluster's records with flag 1.0, and the median record of every
        bin that is not empty.  ``n_points``: a scalar, one value per regressor, or None for each regressor's nbins; at most
        min(32, nbins).  Every regressor must have ONE feature.  ``bins`` is OVERWRITTEN: a row per selected record, with count 1, so
        ``fit_gp()``, ``search_gp()``, ``factor_gp()`` and ``evaluate_log()`` follow unchanged with min_count=1.  ``rebin()``,
        ``prune_log(rebin=True)`` and ``fit_clusters(rebin=True)`` go back to the bin means.  An observed flight after a selection adds
        its sums to rows that hold single records: re-bin or select again before the next fit.  One chain of 22 launches on the stream,
        asynchronous; returns the device tensors (sel int32 [K, n, 32]: the record index t * B + b per bin, -1 for an empty bin or one
        past n_points; info int32 [K, n, 4]: the points, the cluster's records that took part, the empty bins, the status)."""
        self._learns("select_points")
        if not self.log_steps:
            raise ValueError("select_points: this fleet keeps no log, create it with log_steps")
        want = select_request(self._blocks, n_points)
        if self.log_count < 1:
            raise ValueError("select_points: the log is empty: fly rollout(T, observe=True, log=True) first")
        _lib.check(self.lib.admpc_quad_ensemble_select_points(self._ens, self.log_count * self.B, _ptr(self.log), (C.c_int32 * QUAD_GP_MAX)(*want),
                                                              _ptr(self._select_code), _ptr(self.select_edges), _ptr(self._select_work),
                                                              _ptr(self.bins), _ptr(self.sel), _ptr(self.select_info), self._stream()))
        self._selected = True
        return self.sel[:, :self.n_learn], self.select_info[:, :self.n_learn]

    def selected_points(self):
        """The last ``select_points`` as numpy (synchronises): K lists of one dict per regressor with ``index`` (the record indices in
        ascending bin order), ``z`` and ``y`` (the records' feature and target), ``bins`` (the bin of every point), ``took_part``,
        ``empty`` and ``status``."""
        self._learns("selected_points")
        if not getattr(self, "_selected", False):
            raise ValueError("selected_points: nothing selected yet: call select_points() first")
        torch.cuda.current_stream(self.device).synchronize()
        sel, info = self.sel.cpu().numpy(), self.select_info.cpu().numpy()
        log = self.log.reshape(-1, QUAD_REC).cpu().numpy()
        out = []
        for c in range(self.K):
            row = []
            for g in range(self.n_learn):
                gp = self._blocks[c][0][g]
                at = np.flatnonzero(sel[c, g] >= 0)
                idx = sel[c, g, at].astype(np.int64)
                row.append({"index": idx, "z": log[idx, int(gp.feat[0]) - 7].copy(), "y": log[idx, 10 + int(gp.out) - 7].copy(), "bins": at,
                            "took_part": int(info[c, g, 1]), "empty": int(info[c, g, 2]), "status": int(info[c, g, 3])})
            out.append(row)
        return out

    def fit_rdrv(self, axes=(7, 8, 9), install=True):
        """Faessler's diagonal linear drag from the logged records with flag 1.0 (admpc_quad_rdrv_fit: D_i = sum v_b,i y_i / sum v_b,i^2
        for the features in ``axes``, 0 elsewhere), and (`install`) into rdrv of all K cluster handles on the device
        (admpc_quad_rdrv_install); the nominal handle, which predicts for observe, keeps none.  The values are set, not added, so a
        fleet created with a non-zero ``rdrv_d_mat`` is refused: its residual was observed against a model that had drag already.
        Asynchronous; returns the device tensors (d float64 [3], info int32 [2]: n_used and status, installed int32 [K] or None)."""
        self._learns("fit_rdrv")
        if not self.log_steps:
            raise ValueError("fit_rdrv: this fleet keeps no log, create it with log_steps")
        if self._rdrv_given:
            raise ValueError("fit_rdrv: the fleet was created with a non-zero rdrv_d_mat; the fit sets the drag, it does not add to it")
        mask = rdrv_axes(axes)
        if self.log_count < 1:
            raise ValueError("fit_rdrv: the log is empty: fly rollout(T, observe=True, log=True) first")
        s = self._stream()
        self._has_rdrv = True
        _lib.check(self.lib.admpc_quad_rdrv_fit(self.device_index, self.log_count * self.B, mask, _ptr(self.log), _ptr(self._rdrv_partial),
                                                _ptr(self.rdrv), _ptr(self.rdrv_sums), _ptr(self.rdrv_info), s))
        if not install:
            return self.rdrv, self.rdrv_info, None
        for c, solver in enumerate(self._solvers):
            _lib.check(self.lib.admpc_quad_rdrv_install(solver._h, _ptr(self.rdrv), _ptr(self.rdrv_info),
                                                        C.c_void_p(self.rdrv_installed.data_ptr() + 4 * c), s))
        return self.rdrv, self.rdrv_info, self.rdrv_installed

    def learned_rdrv(self):
        """The drag of the last fit_rdrv as a 3 x 3 diagonal numpy matrix, what ``rdrv_d_mat`` takes (synchronises)."""
        self._learns("learned_rdrv")
        if not self.log_steps:
            raise ValueError("learned_rdrv: this fleet keeps no log, create it with log_steps")
        torch.cuda.current_stream(self.device).synchronize()
        return np.diag(self.rdrv.cpu().numpy())

    def fit_clusters(self, max_iter=100, tol=1e-3, reg_covar=1e-6, init=None, install=True, rebin=True, resume=False, seed=None, n_init=1,
                     km_max_iter=300, km_tol=1e-4):
        """The centroids from the log: sklearn's Gaussian-mixture EM (full covariances; max_iter, tol and reg_covar are its defaults) from
        the means ``init`` [K, n_feat] (default: the present centroids; a float64 tensor on the fleet's device is taken as it is, which
        keeps the call free of copies for a graph) over the logged records (admpc_quad_clusters_fit), then
        (`install`) its means, sorted along the first feature, as the ensemble's centroids, and (`rebin`) the log binned again under
        them.  One chain of launches on the stream, asynchronous; returns the device tensors (info int32 [4]: iterations, converged,
        status, n_valid; perm int32 [K]; installed int32 [1]), the last two None without `install`.

        ``init="kmeans"`` is what the reference's GaussianMixture(n_clusters).fit does with nothing given: scikit-learn's k-means++
        seeding and Lloyd k-means under ``seed`` (required; ``km_max_iter`` and ``km_tol`` are KMeans' defaults) find the means the EM
        starts from (admpc_quad_kmeans_fit; include/admpc_quad_kmeans.h), and with ``n_init`` > 1 the chain runs under draw = 0 ..
        n_init - 1 and the fit with the largest lower bound is kept (admpc_quad_clusters_keep), installed and returned; ``km_kept``
        int32 [1] is its draw.  A k-means that fails hands the EM the present centroids.  ``km_centers``, ``km_idx``, ``km_info``,
        ``km_stats`` and ``km_labels`` are allocated at the first such call (call once before capturing a graph, with the n_init that
        will be captured) and hold the k-means of the fit that was kept (admpc_quad_kmeans_keep); ``learned_kmeans()`` returns them."""
        self._learns("fit_clusters")
        if isinstance(init, str):
            if init != "kmeans":
                raise ValueError("fit_clusters: init must be None, K x len(feats) means or \"kmeans\"")
            return self._fit_clusters_kmeans(max_iter, tol, reg_covar, install, rebin, resume, seed, n_init, km_max_iter, km_tol)
        if seed is not None or n_init != 1:
            raise ValueError("fit_clusters: seed and n_init go with init=\"kmeans\"")
        start = None
        if torch.is_tensor(init):
            self._eng._chk(init, (self.K, len(self.feats)))
            start, init = init, None
        max_iter, tol, reg_covar, init = clusters_request(self.K, self.feats, self.log_count, max_iter, tol, reg_covar, init)
        s = self._stream()
        if init is not None:
            start = torch.as_tensor(init).to(self.device)
        _lib.check(self.lib.admpc_quad_clusters_fit(self._ens, max_iter, tol, reg_covar, 1 if resume else 0, self.log_count * self.B, _ptr(self.log),
                                                    _ptr(start), _ptr(self._packed), _ptr(self._partial), _ptr(self.gmm), _ptr(self.gmm_info), s))
        if install:
            _lib.check(self.lib.admpc_quad_clusters_install(self._ens, _ptr(self.gmm), _ptr(self.gmm_info), _ptr(self.perm),
                                                            _ptr(self.centroids_installed), s))
            self._moved = True
        if rebin:
            self.rebin()
        return (self.gmm_info, self.perm, self.centroids_installed) if install else (self.gmm_info, None, None)

    def _fit_clusters_kmeans(self, max_iter, tol, reg_covar, install, rebin, resume, seed, n_init, km_max_iter, km_tol):
        max_iter, tol, reg_covar, _ = clusters_request(self.K, self.feats, self.log_count, max_iter, tol, reg_covar, None)
        seed, n_init, km_max_iter, km_tol = kmeans_request(seed, n_init, km_max_iter, km_tol, resume)
        if getattr(self, "km_centers", None) is None:
            z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=self.device)
            cap = self.log_steps * self.B
            self.km_centers, self.km_idx = z(self.K, len(self.feats)), z(self.K, dtype=torch.int64)
            self.km_info, self.km_stats, self.km_labels = z(4, dtype=torch.int32), z(4), z(cap, dtype=torch.int32)
            self.km_kept = z(1, dtype=torch.int32)
            self._km_dist, self._km_work = z(cap), z(kmeans_work(cap))
            self._gmm_try, self._gmm_info_try = z(1 + self.K, GMM_ROW), z(4, dtype=torch.int32)
            self._km_try = None                                                                # the k-means results of a try, at the first n_init > 1
        s, M = self._stream(), self.log_count * self.B
        many = n_init > 1
        gmm, info = (self._gmm_try, self._gmm_info_try) if many else (self.gmm, self.gmm_info)
        best = (self.km_centers, self.km_idx, self.km_labels, self.km_stats, self.km_info)
        if many and self._km_try is None:
            self._km_try = tuple(torch.zeros_like(t) for t in best)
        centers, idx, labels, stats, kinfo = self._km_try if many else best
        for draw in range(n_init):
            _lib.check(self.lib.admpc_quad_kmeans_fit(self._ens, seed, draw, km_max_iter, km_tol, M, _ptr(self.log), _ptr(self._packed),
                                                      _ptr(self._km_dist), _ptr(labels), _ptr(self._km_work), _ptr(centers), _ptr(idx), _ptr(stats),
                                                      _ptr(kinfo), s))
            _lib.check(self.lib.admpc_quad_clusters_fit(self._ens, max_iter, tol, reg_covar, 0, M, _ptr(self.log), _ptr(centers),
                                                        _ptr(self._packed), _ptr(self._partial), _ptr(gmm), _ptr(info), s))
            if many:
                _lib.check(self.lib.admpc_quad_clusters_keep(self._ens, draw, _ptr(gmm), _ptr(info), _ptr(self.gmm), _ptr(self.gmm_info),
                                                             _ptr(self.km_kept), s))
                _lib.check(self.lib.admpc_quad_kmeans_keep(self._ens, draw, M, _ptr(self.km_kept), _ptr(centers), _ptr(idx), _ptr(labels), _ptr(stats),
                                                           _ptr(kinfo), *[_ptr(t) for t in best], s))
        self._km_many = many
        if install:
            _lib.check(self.lib.admpc_quad_clusters_install(self._ens, _ptr(self.gmm), _ptr(self.gmm_info), _ptr(self.perm),
                                                            _ptr(self.centroids_installed), s))
            self._moved = True
        if rebin:
            self.rebin()
        return (self.gmm_info, self.perm, self.centroids_installed) if install else (self.gmm_info, None, None)

    def learned_kmeans(self):
        """The k-means of the last fit_clusters(init="kmeans") as numpy (synchronises): QuadKMeans(centers [K,n_feat], idx int64 [K] the
        seeded records t * B + b, labels int32 [records logged] with -1 where a record does not count, n_iter, converged (0; 1 by
        tolerance; 2 because no label changed), status, n_valid, inertia, tol_abs, shift, potential, kept: the draw whose fit was kept
        with n_init > 1, else 0; everything else is that draw's k-means)."""
        self._learns("learned_kmeans")
        if getattr(self, "km_centers", None) is None:
            raise ValueError("learned_kmeans: no k-means yet: call fit_clusters(init=\"kmeans\", seed=...) first")
        torch.cuda.current_stream(self.device).synchronize()
        info, stats = self.km_info.cpu().numpy(), self.km_stats.cpu().numpy()
        return QuadKMeans(self.km_centers.cpu().numpy().copy(), self.km_idx.cpu().numpy().copy(),
                          self.km_labels[:self.log_count * self.B].cpu().numpy().copy(), int(info[0]), int(info[1]), int(info[2]), int(info[3]),
                          float(stats[0]), float(stats[1]), float(stats[2]), float(stats[3]), int(self.km_kept.cpu()[0]) if self._km_many else 0)

    def learned_clusters(self):
        """The mixture of the last fit_clusters as numpy (synchronises): QuadClusters(weights [K], means [K,n_feat], covariances
        [K,n_feat,n_feat], n_iter, converged, status, perm [K]), the components in the order of the fit -- cluster c is component
        perm[c].  ``self.centroids`` is refreshed from the device."""
        self._learns("learned_clusters")
        if not self.log_steps:
            raise ValueError("learned_clusters: this fleet keeps no log, create it with log_steps")
        self._device_centroids()
        torch.cuda.current_stream(self.device).synchronize()
        g, info, d = self.gmm.cpu().numpy(), self.gmm_info.cpu().numpy(), len(self.feats)
        tri = np.array([[4, 5, 6], [5, 7, 8], [6, 8, 9]])
        return QuadClusters(g[1:, 0].copy(), g[1:, 1:1 + d].copy(), g[1:][:, tri][:, :d, :d].copy(), int(info[0]), bool(info[1]), int(info[2]),
                            self.perm.cpu().numpy().copy())

    # -- learning, per cluster ----------------------------------------------------------------------------------------------------------
    def set_observer(self, learned=False, cluster=0):
        """Which handle predicts in observe: the nominal one (default) or, with `learned`, the handle of ``cluster`` with whatever GPs
        are installed in it."""
        self._learns("set_observer")
        if learned and not 0 <= int(cluster) < self.K:
            raise ValueError("set_observer: cluster must be in 0 .. %d" % (self.K - 1))
        self._observer = self._solvers[int(cluster)] if learned else self._nominal

    def observe(self, u=None):
        """QuadFleet.observe with every record going to the bins of ITS cluster, the centroid nearest to the record's own features
        (admpc_quad_ensemble_observe_batch).  Asynchronous."""
        self._learns("observe")
        u = self.w_opt[:, 0, :] if u is None else u
        stride = self._u_stride("observe", u, self.B)
        _lib.check(self.lib.admpc_quad_ensemble_observe_batch(self._ens, self._observer._h, C.byref(self._plant), self.B, C.c_void_p(u.data_ptr()),
                                                              stride, _ptr(self.x), _ptr(self._prev), _ptr(self.samples), _ptr(self.bins),
                                                              _ptr(self.dropped), self._stream()))

    def fit_gp(self, min_count=1, install=True, factor=False):
        """Fits every regressor of every cluster to the means of its bins with at least `min_count` samples, at that cluster's
        hyperparameters, and (`install`) overwrites the GPs of the K handles on the device.  With `factor` the factors of the evaluation
        (``factor_gp``) follow the fit in the same chain, from the same bins.  Asynchronous; returns the device tensors
        (info int32 [K,n], installed int32 [K,n] or None) as QuadFleet.fit_gp explains them."""
        self._learns("fit_gp")
        if factor:
            self._keeps_log("fit_gp: factor=True")
        n, s = self.n_learn, self._stream()
        _lib.check(self.lib.admpc_quad_ensemble_fit(self._ens, int(min_count), _ptr(self.bins), _ptr(self._gp_dev), _ptr(self.fit_info), s))
        self._searched = False                                                             # the records hold the given hyperparameters again
        if factor:
            self.factor_gp(min_count)
        if not install:
            return self.fit_info[:, :n], None
        _lib.check(self.lib.admpc_quad_ensemble_install(self._ens, _ptr(self._gp_dev), _ptr(self.installed), s))
        return self.fit_info[:, :n], self.installed[:, :n]

    def search_gp(self, min_count=1, grid=5, rounds=10, shrink=0.5, bounds=None, resume=False, install=True, factor=False):
        """QuadFleet.search_gp for every regressor of every cluster in one chain of launches (include/admpc_quad_hyper.h:
        admpc_quad_ensemble_search -> admpc_quad_ensemble_refit -> admpc_quad_ensemble_install): 2 * rounds + 1 + K launches on the
        fleet's stream, one more where the search starts.  ``bounds``: None (the reference's box everywhere), one list of
        config.search_boxes dicts per regressor (every cluster searches that box), or K such lists.  grid, rounds and shrink serve all
        clusters.  The parameters go to the object by admpc_quad_ensemble_set_search, which synchronises, only when they differ from the
        last call's: a second call with the same ones has no host synchronisation and no allocation.  After ``fit_clusters()`` call
        with resume=False: the clusters hold other data.  With `factor` the factors of the evaluation (``factor_gp``) follow the re-fit in
        the same chain, from the same bins and the same ``hyper``.  Returns the device tensors (info int32 [K,n], installed int32 [K,n] or None,
        hyper float64 [K,n,16])."""
        self._learns("search_gp")
        if factor:
            self._keeps_log("search_gp: factor=True")
        n = self.n_learn
        sp = (AdmpcGpSearchParams * self.K)()
        for c, b in enumerate(self._cluster_bounds(bounds)):
            sp[c] = AdmpcGpSearchParams(grid=int(grid), rounds=int(rounds), shrink=float(shrink), box=search_boxes(self._learn[c], b))
        key = bytes(sp)
        if key != self._search_set:
            _lib.check(self.lib.admpc_quad_ensemble_set_search(self._ens, sp))
            self._search_set = key
        s = self._stream()
        _lib.check(self.lib.admpc_quad_ensemble_search(self._ens, int(min_count), 1 if resume else 0, _ptr(self.bins), _ptr(self.hyper),
                                                       _ptr(self._nll), _ptr(self.search_info), s))
        _lib.check(self.lib.admpc_quad_ensemble_refit(self._ens, int(min_count), _ptr(self.bins), _ptr(self.hyper), _ptr(self._gp_dev),
                                                      _ptr(self.fit_info), s))
        self._has_hyper = self._searched = True
        if factor:
            self.factor_gp(min_count)
        if not install:
            return self.fit_info[:, :n], None, self.hyper[:, :n]
        _lib.check(self.lib.admpc_quad_ensemble_install(self._ens, _ptr(self._gp_dev), _ptr(self.installed), s))
        return self.fit_info[:, :n], self.installed[:, :n], self.hyper[:, :n]

    # -- the evaluation of the learned GPs on the log (include/admpc_quad_eval.h) -----------------------------------------------------------
    def _keeps_log(self, who):
        if not self.log_steps:
            raise ValueError("%s: this fleet keeps no log, create it with log_steps" % who)

    def factor_gp(self, min_count=1):
        """Every regressor of every cluster factored once from the present bins (admpc_quad_ensemble_factor: the fit's K, its Cholesky
        factor, alpha, and W = L^-1), at the hyperparameters of the last ``fit_gp`` / ``search_gp``: each cluster's given ones, or what the
        search left in ``hyper``.  One launch, asynchronous; returns the device tensor factor_info int32 [K,n]: the points, or the fit's
        failure code.  What a later flight adds to the bins does not reach the factor."""
        self._learns("factor_gp")
        self._keeps_log("factor_gp")
        _lib.check(self.lib.admpc_quad_ensemble_factor(self._ens, int(min_count), _ptr(self.bins), _ptr(self.hyper) if self._searched else None,
                                                       _ptr(self.factor), _ptr(self.factor_info), self._stream()))
        self._has_factor = True
        return self.factor_info[:, :self.n_learn]

    def evaluate_log(self, include_pruned=False, drag=False, per_record=False):
        """The learned GPs, as the last factor holds them, evaluated over the ``log_count * B`` logged records
        (admpc_quad_ensemble_evaluate: the reference's gp_evaluate_test_set): per record the posterior mean and standard deviation of
        every regressor of its cluster, per cluster and regressor the error sums.  `include_pruned` also takes the records a prune took
        out (the reference's pruned=False); `drag` scores the linear drag of the last ``fit_rdrv`` under the GPs; `per_record` asks for
        the [log_count * B, 3, 2] tensor of mean and standard deviation (allocated at the first call that asks, so make that call
        outside a capture).  Asynchronous; returns the device tensors (stats float64 [K,3,8], info int32 [4]: status, took part, skipped
        by flag, skipped as not finite; per_record or None).  ``evaluation()`` reads them."""
        self._learns("evaluate_log")
        take, drag, per_record = eval_request(self.log_steps, self.log_count, getattr(self, "_has_factor", False), include_pruned, drag,
                                              getattr(self, "_has_rdrv", False), per_record)
        out = None
        if per_record:
            if self.eval_per_record is None:
                self.eval_per_record = torch.zeros((self.log_steps * self.B, QUAD_GP_MAX, 2), dtype=torch.float64, device=self.device)
            out = self.eval_per_record[:self.log_count * self.B]
        _lib.check(self.lib.admpc_quad_ensemble_evaluate(self._ens, self.log_count * self.B, _ptr(self.log), take, _ptr(self.factor),
                                                         _ptr(self.rdrv) if drag else None, _ptr(out), _ptr(self._eval_partial),
                                                         _ptr(self.eval_stats), _ptr(self.eval_info), self._stream()))
        self._evaluated = True
        return self.eval_stats, self.eval_info, out

    def evaluation(self, units="rate"):
        """The last ``evaluate_log`` as a ``QuadEvaluation`` (synchronises): per [K, n] count, nominal_mae and augmented_mae (what the
        reference prints as "RMSE" is a mean absolute error), nominal_rms, augmented_rms, mean_std, within_3std (the share of the records
        with |r| <= 3 std) and clipped (variances below 0, taken as 0), and in ``total`` the same over all clusters per regressor.
        units="rate" leaves the residual as it is recorded, per second; units="velocity" multiplies by the observe dt, the reference's
        ``* dt_test``."""
        self._learns("evaluation")
        if units not in ("rate", "velocity"):
            raise ValueError("evaluation: units must be 'rate' or 'velocity'")
        if not getattr(self, "_evaluated", False):
            raise ValueError("evaluation: nothing evaluated yet: call evaluate_log() first")
        torch.cuda.current_stream(self.device).synchronize()
        return evaluation_table(self.eval_stats.cpu().numpy(), self.n_learn, self.control_period if units == "velocity" else None)

    def _cluster_bounds(self, bounds):
        """``bounds`` of search_gp as K entries for config.search_boxes: None, one list per regressor for every cluster, or K lists."""
        if bounds is None:
            return [None] * self.K
        bounds = list(bounds)
        if bounds and all(b is None or isinstance(b, dict) for b in bounds):
            return [bounds] * self.K
        if len(bounds) != self.K or any(isinstance(b, dict) or not isinstance(b, (list, tuple, type(None))) for b in bounds):
            raise ValueError("bounds: None, one list of dicts per regressor, or one such list per cluster (%d)" % self.K)
        return bounds

    def learned_hyper(self):
        """QuadFleet.learned_hyper per cluster (synchronises): K lists of dicts."""
        self._learns("learned_hyper")
        torch.cuda.current_stream(self.device).synchronize()
        hy = self.hyper.cpu().numpy()
        return [hyper_dicts(hy[c], self._obs[c].gp, self.n_learn, self._has_hyper) for c in range(self.K)]

    def learned_gps(self):
        """The GPs of the last fit_gp or search_gp as a ``QuadGPEnsemble`` with the centroids the device holds and the fleet's features
        (synchronises): what ``QuadEnsembleFleet(ensemble=...)`` takes.  Every cluster is decoded as QuadFleet.learned_gps decodes its one:
        after a search_gp with the length scales and sigma_f it found for that cluster."""
        self._learns("learned_gps")
        torch.cuda.current_stream(self.device).synchronize()
        raw = self._gp_dev.cpu().numpy().tobytes()
        per = QUAD_GP_MAX * C.sizeof(AdmpcGp)
        heads = [list(cluster) for cluster in self._learn]
        if self._searched:
            hy = self.hyper.cpu().numpy()
            heads = [[dict(d, length_scale=hy[c, g, 10:10 + int(self._obs[c].gp[g].n_feat)].tolist(), sigma_f=float(hy[c, g, 13]))
                      for g, d in enumerate(cluster)] for c, cluster in enumerate(heads)]
        return QuadGPEnsemble([decode_gps(raw[c * per:(c + 1) * per], heads[c], self._EMPTY) for c in range(self.K)], self._device_centroids(),
                              self.feats)
