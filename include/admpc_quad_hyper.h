/*
 * admpc_quad_hyper.h -- searching the hyperparameters of the quadrotor's body-frame residual GPs on the device: the length scales, sigma_f
 * and the noise of every regressor of admpc_quad_learn.h, and of every regressor of every cluster of admpc_quad_ensemble.h, by the zooming
 * grid search of admpc_hyper.h, and the fit at the optimum (libadmpc.so; csrc/admpc_quad_hyper.hip).  An addition to admpc_hyper.h,
 * admpc_quad_learn.h and admpc_quad_ensemble.h, whose conventions hold here: device pointers owned by the caller, `stream` a hipStream_t
 * passed as void*, 0 or a negative ADMPC_E* code returned, admpc_last_error() for the message, the caller's HIP device restored, every
 * refusal in front of the first device call, in the order it is listed; no host synchronisation and no allocation in the stream entries
 * (all but admpc_quad_ensemble_set_search), which can be captured into a graph.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/...)                               replaced by
 *   -------------------------------------------------------------------------------------  ------------------------------------
 *   model_fitting/gp.py:278-316          nll: K, its Cholesky, the three terms               admpc_quad_gp_search, admpc_quad_ensemble_search:
 *                                                                                          the NLL kernel
 *   model_fitting/gp.py:318-323, 337-352 minimize(L-BFGS-B) from one start, bounds           the same: the rounds (grid, pick, zoom)
 *   model_fitting/gp.py:354-363          the optimum taken over, K^-1 y at it                admpc_quad_gp_refit, admpc_quad_ensemble_refit
 *   model_fitting/gp_fitting.py          GPR.fit of every axis of every cluster              admpc_quad_ensemble_search and _refit: all
 *                                                                                          K * n_gp regressors in one chain of launches
 *
 * The reference never fits a quadrotor GP at given hyperparameters: every GP of every cluster goes through GPR.fit, which minimises the
 * NLL first.  After admpc_quad_clusters.h has moved the centroids every cluster holds other data than its block was written for; a search
 * with resume = 0 on the new statistics replaces the given length scales by found ones.
 *
 * NOT offered:
 *   - the evaluation of what a search found on held-out records, and any predictive variance, by THESE entries: admpc_quad_eval.h
 *     factors every regressor at the hyperparameters the search left in `hyper` and scores them on a log, on the same stream;
 *   - gradients, L-BFGS-B or random restarts: the search is the zooming grid of admpc_hyper.h;
 *   - a warm start of the search across new statistics (call with resume = 0 after a re-bin);
 *   - a K chosen by the search; handles in SQP mode.  admpc_quad_sqp.h has the SQP loop that one-handle rollouts fly;
 *   - per-cluster grid, rounds or shrink in an ensemble (one chain of launches serves all clusters; the boxes are free per cluster).
 *
 * WHY THE ENSEMBLE HAS KERNELS OF ITS OWN.  The kernels behind admpc_gp_search take their regressors and search descriptors by value:
 * 136 + 184 bytes per regressor.  The 24 regressors of K = 8 come to 7.7 KB, past the 4 KB of kernel arguments.  The ensemble's kernels
 * run the same bodies (csrc/gp_search_dev.h, csrc/gp_fit_dev.h) and read the regressors from the object's device copy and the descriptors
 * from a second device copy, which admpc_quad_ensemble_set_search writes: both by pointer.
 *
 * Measured on one MI355X at B = 4096 with three 32-bin regressors per cluster (32 points each), grid 5, 10 rounds, 125 candidates per
 * regressor and round, captured graphs replayed, the forms alternating in one session, medians of three (scripts/quad_hyper_time.py;
 * DESIGN section 7), microseconds at K = 1 / 4 / 8: a round (NLL launch + pick launch) of admpc_quad_ensemble_search 45.8 / 44.6 / 49.1
 * against 47.4 / 189.7 / 379.5 for K calls of admpc_quad_gp_search; ten rounds from resume = 0 468 / 456 / 501 against 484 / 1913 / 3817;
 * search -> re-fit -> install whole 517 / 525 / 595 (admpc_quad_ensemble_fit with install at given values: 55 / 207 / 405, K launches of
 * the fit and K of the install); the route it replaces -- bins to the host, scipy L-BFGS-B per regressor from the centre of the same box,
 * K new handles -- 5.1 / 19.2 / 38.4 ms on the host clock.  One chain costs at K = 8 what it costs at K = 1: 24 regressors of 125
 * candidates are 384 blocks a round, and a round's time is the latency of its two launches and of one 32-step Cholesky.
 */
#ifndef ADMPC_QUAD_HYPER_H
#define ADMPC_QUAD_HYPER_H

#include <stdint.h>
#include "admpc_hyper.h"
#include "admpc_quad_learn.h"
#include "admpc_quad_ensemble.h"

#ifdef __cplusplus
extern "C" {
#endif

/* admpc_gp_search of admpc_hyper.h in every respect -- the state hyper [n_gp][ADMPC_GP_HYPER], the decoding of a candidate, the pick
 * rule, resume, nll [n_gp][ADMPC_GP_SEARCH_MAX] as scratch, search_info [n_gp][2] -- with the quadrotor's ranges: feat in 7 .. 16, out
 * in 7 .. 9, n_gp <= ADMPC_QUAD_GP_MAX.  Of sp->box the first n_gp entries are read.  The feature indices and the output rows never
 * enter an NLL, and the kernels are the car's own (one host side behind both entries, csrc/admpc_hyper.hip): on equal statistics,
 * n_feat, nb and boxes this entry returns admpc_gp_search's hyper, nll and search_info bit for bit.
 * ADMPC_EINVAL, in this order: obs as admpc_quad_learn.h refuses it; sp null, grid, rounds, shrink; per regressor a bad used slot, then a
 * candidate count above ADMPC_GP_SEARCH_MAX; min_count < 1; resume not 0 or 1; a null array. */
int admpc_quad_gp_search(int device, const AdmpcQuadObserveParams* obs, const AdmpcGpSearchParams* sp, int min_count, int resume,
                         const double* bins, double* hyper, double* nll, int32_t* search_info, void* stream);

/* admpc_gp_refit of admpc_hyper.h in every respect, ADMPC_GP_NO_OPTIMUM included, with the quadrotor's ranges: admpc_quad_gp_fit at the
 * natural values hyper[g][10 .. 14].  The install is admpc_quad_gp_install.
 * ADMPC_EINVAL, in this order: obs as admpc_quad_learn.h refuses it; min_count < 1; a null array. */
int admpc_quad_gp_refit(int device, const AdmpcQuadObserveParams* obs, int min_count, const double* bins, const double* hyper,
                        AdmpcGp* gp_out, int32_t* info, void* stream);

/* The search parameters of an ensemble that learns: sp [K] (host), one block per cluster, of each the first n_gp boxes.  The blocks
 * agree in grid, rounds and shrink; the boxes are free per cluster.  SYNCHRONOUS, like create: it waits for the device, forms on the
 * host, in double, what admpc_gp_search forms (log lo, log hi, the free slots, the candidate count C, the centre and the step of a
 * start) and copies it into a device allocation that the object owns -- made at the first call, reused by every later one, freed by
 * admpc_quad_ensemble_destroy.  The kernels take the descriptors by pointer: a graph captured earlier reads the new boxes, grid and shrink
 * at its next replay; the number of rounds and the launch geometry (the largest C over all regressors) are those of the capture.
 * ADMPC_EINVAL, in this order: a null ensemble; an ensemble created without observe parameters; a null sp; then per cluster, in the
 * order of the clusters, admpc_gp_search's refusals of grid, rounds, shrink, the box slots and the candidate count; then blocks that
 * differ in grid, rounds or shrink.  A refused call leaves the object's search as it was. */
int admpc_quad_ensemble_set_search(AdmpcQuadEnsemble* e, const AdmpcGpSearchParams* sp);

/* The search of all K * n_gp regressors: init when resume == 0, then `rounds` times (the NLL kernel, the pick kernel), every launch over
 * all regressors: grid (ceil(max C / 8), K * n_gp) for the NLL, K * n_gp waves for the init and the pick.
 *   bins [K][3][32][5] (read only), hyper [K][3][ADMPC_GP_HYPER] in/out, nll [K][3][ADMPC_GP_SEARCH_MAX] scratch, search_info [K][3][2]
 * Cluster c, regressor g is admpc_quad_gp_search on bins[c] under block c of the ensemble's observe parameters and block c of the
 * search parameters, BIT FOR BIT in hyper, in nll up to C_{c,g} and in search_info: one body of the kernels serves both.  The entries of
 * a regressor past n_gp, and of nll past C_{c,g}, are not written.
 * ADMPC_EINVAL, in this order: a null ensemble; an ensemble created without observe parameters; no admpc_quad_ensemble_set_search yet;
 * min_count < 1; resume not 0 or 1; a null array. */
int admpc_quad_ensemble_search(const AdmpcQuadEnsemble* e, int min_count, int resume, const double* bins, double* hyper, double* nll,
                               int32_t* search_info, void* stream);

/* gp_out [K][3] AdmpcGp records and info [K][3] int32 from bins and hyper as above: cluster c is admpc_quad_gp_refit of bins[c] and
 * hyper[c] under block c, byte for byte, in ONE launch of K * n_gp waves (admpc_quad_ensemble_fit takes K launches).  The entries of a
 * regressor past n_gp are not written.  The install stays admpc_quad_ensemble_install.
 * ADMPC_EINVAL, in this order: a null ensemble; an ensemble created without observe parameters; min_count < 1; a null array. */
int admpc_quad_ensemble_refit(const AdmpcQuadEnsemble* e, int min_count, const double* bins, const double* hyper, AdmpcGp* gp_out,
                              int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_HYPER_H */
