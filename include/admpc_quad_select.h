/*
 * admpc_quad_select.h -- the stage of the reference's training pipeline that picks the training points of every GP, on the device
 * (libadmpc.so; csrc/admpc_quad_select.hip).  The reference trains every regressor of every cluster on at most n_train_points REAL
 * records of the cluster, which it picks so that they spread over the feature's range; the other entries of this library fit to the MEANS
 * of a fixed grid of bins over a box the caller supplies.  With this entry record -> prune -> cluster -> select -> search / fit -> install
 * -> evaluate is one chain of launches on one stream, and the models are trained on the records the reference would train on.  An addition to
 * admpc_quad_prune.h and admpc_quad_eval.h, whose conventions hold here: device pointers owned by the caller, dense; `stream` a hipStream_t
 * passed as void*; 0 or a negative ADMPC_E* code returned, admpc_last_error() of admpc.h for the message; the caller's HIP device restored;
 * no host synchronisation and no allocation, the entry can be captured into a graph; every refusal in front of the first device call, in
 * the order it is listed; an empty log (M == 0) is a no-op.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/...)                                  replaced by
 *   ----------------------------------------------------------------------------------------  ------------------------------------
 *   model_fitting/gp_fitting.py:230-249  TRAINING POINT SELECTION: per cluster the indices of    admpc_quad_ensemble_select_points: all
 *                                     the records the GP of every output is trained on            clusters and regressors in one chain
 *   utils/utils.py:621-626            distance_maximizing_points: the route by the number of      the one-feature route; more features
 *                                     features                                                    are refused
 *   utils/utils.py:536-581            distance_maximizing_points_1d: a histogram of n_train_points the same entry: range, edges, count,
 *                                     bins over the cluster's feature values, the median record    eight digit passes, lowest, gather
 *                                     of every bin
 *   model_fitting/gp_fitting.py:251-300  the GP of every cluster and output fitted to x[indices],  admpc_quad_ensemble_fit / _search /
 *                                     y[indices]                                                  _refit / _factor as they stand, with
 *                                                                                               min_count = 1: a selected record is a
 *                                                                                               bin with count 1
 *
 * NOT offered:
 *   - the random draw for an empty bin (utils.py: a bin of the histogram without a member gets a random record of the cluster): an empty
 *     bin gives no point.  This is the one deliberate difference on the route that is offered;
 *   - n_train_points above ADMPC_GP_MAX_POINTS = 32 (the reference's default is 50, its command line's 20);
 *   - the dense-GP branch (dense_gp is not None) and sample_random_points, which the 1-D route never reaches;
 *   - the route for two or more features, a randomly started k-means with random picks, which cannot be pinned; the dead PCA branch;
 *   - the reference's y_mean = the mean of ALL targets of the cluster (gp_fitting.py:242, 296): the fit keeps the mean of the selected
 *     targets (gp_ymean);
 *   - soft top-2 cluster membership (gp_common.py:253-262); handles in SQP mode.  admpc_quad_sqp.h has the SQP loop that one-handle
 *     rollouts fly;
 *   - a selection for QuadFleet, which keeps no log.
 *
 * THE RULE, quirks included.  For cluster c and regressor g with ONE feature f and output o, the POINTS are the records of the log, in log
 * order (record index i), that meet all of: the flag (entry 13) is exactly 1.0; the clustering features lie nearest to centroid c (the
 * routing predicate of the bin kernel, at the centroids on the device); z = rec[f - 7] and y = rec[10 + o - 7] are both finite.  With
 * n = n_points[g]:
 *   range    lo, hi the min and max of z over the points; lo - 0.5, hi + 0.5 if they are equal.
 *   edges    np.linspace's: e_j = lo + j * ((hi - lo) / n) for j < n, e_n = hi exactly; every operation rounded on its own.
 *   bin      np.digitize(z, e) - 1 = (the number of edges <= z) - 1, by comparison against the edges and not by a formula.  A point
 *            with z == hi has index n and is in NO bin: the quirk is kept.
 *   pick     a bin with m members: m == 0 gives no point.  For an even m the member with the highest record index is set aside.  The
 *            median is the element of rank (m' - 1) / 2 by value of the m' (odd) members that are left.  The selected record is the one
 *            with the LOWEST record index among ALL the bin's members whose z compares equal to the median (-0.0 == 0.0), which may be
 *            the member that was set aside.
 *   output   the selected records in ascending bin order.
 *
 * WHAT IS WRITTEN.  bins [K][3][32][5] is overwritten for every regressor of every cluster: row r of regressor g of cluster c is
 * {1.0, z, 0, 0, y} of the record of the r-th bin that is NOT EMPTY (the rows are compacted here; gp_points would skip a row of count 0
 * just as well), z and y the record's own bits; every other row, and every row of a regressor the object does not hold, is zero.  To every
 * kernel that reads bins such a row is a bin with one sample, so admpc_quad_ensemble_fit, _search, _refit and _factor work on it with
 * min_count = 1; they read only the rows below a regressor's nbins, which is why n_points may not exceed it.  sel [K][3][32] int32: the
 * record index per BIN (not compacted), -1 where the bin is empty or past n_points.  info [K][3][4] int32: the number of points; the
 * number of records of the cluster that took part (those with z == hi included); the number of empty bins below n_points; the status, 0 or
 * ADMPC_SELECT_ENOVALID where no record takes part (then the regressor's rows are all zero).
 * An observation that follows (admpc_quad_ensemble_observe_batch, an observed rollout) ADDS its sums to rows that now hold single records:
 * re-bin (admpc_quad_clusters_rebin on zeroed bins) or select again before the next fit.
 *
 * THE WORK AREA.  code [M] int32: per record its cluster (bits 0 .. 2) and its bin under each regressor (6 bits each, 63: none).
 * edges [K][3][33]: e_0 .. e_n of every (cluster, regressor); the rest of a row, and the row of a pair without a record, is not written.
 * work [ADMPC_SELECT_WORK] int32, 8-byte aligned: per bin the members, the highest and the lowest index, the rank that is left and the
 * 64-bit prefix of the median's key, per (cluster, regressor) the records that took part and the 64-bit minimum and maximum key, and
 * 256 counters per bin.  All of it is initialised by the entry; nothing needs to be kept between calls.
 *
 * THE CHAIN: 4 + 2 * ADMPC_SELECT_PASSES + 2 = 22 launches, whatever the data.  The grid of every kernel over the records is
 * min(ceil(M / 256), ADMPC_GMM_BLOCKS_MAX) blocks of 256 threads.  The order statistic is a radix select on a 64-bit key of z that orders
 * as z does (-0.0 folded onto +0.0): eight passes of 8 bits, each a histogram of the next digit of the keys that still match the prefix
 * found so far, followed by one wave per bin that picks the digit holding the wanted rank.
 *
 * DETERMINISM.  Integer atomics only: counts by atomicAdd, record indices and keys by atomicMin / atomicMax, in LDS first and one per block
 * and destination to memory where a block can reduce first.  Two runs on the same input give the same bits.
 *
 * Compiled for gfx950 (VGPRs / bytes of LDS, no scratch): init 17 / 0, range 40 / 384, edges 20 / 0, count 44 / 12 576, digit 30 / 15 360,
 * pick 18 / 0, lowest 24 / 9 216, gather 16 / 0.
 *
 * Measured on one MI355X at B = 4096, 60 logged steps (M = 245 760 records), three one-feature regressors, captured graphs replayed, the
 * forms alternating in one session, medians of three (scripts/quad_select_time.py), microseconds at K = 1 / 4 / 8:
 * the selection at n_points 20 421.3 / 297.3 / 298.6, at 32 386.7 / 273.5 / 270.0; the re-bin of the same log (the bins zeroed, 60 bin
 * launches) 3679 / 5391 / 7294.  The route it replaces -- the log to the host, the numpy restatement of the rule, the rows uploaded --
 * 751 713 / 1 282 506 / 1 957 519: 1784 / 4314 / 6556 times the selection, with the same sel and the same rows.  By kernel trace at K = 4,
 * per selection: the eight digit passes 215.7 (7.0 ... 134.8 each), the eight picks 38.3, count 14.3, range 9.5, lowest 6.3, edges 4.6,
 * init 4.4, gather 4.2.  The digit passes of one selection in order: 19.6, 105.2, 30.0, 8.2, 7.8, 8.0, 7.5, 7.6.  The first is not bound
 * by atomics (sign and exponent are one value per bin, and a block counts the first digit it meets in a bin in LDS); the second, whose
 * digits are spread over a bin's members, is: most (record, regressor) pairs issue a global atomic of their own.
 */
#ifndef ADMPC_QUAD_SELECT_H
#define ADMPC_QUAD_SELECT_H

#include <stdint.h>
#include "admpc_quad_ensemble.h"
#include "admpc_quad_clusters.h"    /* ADMPC_GMM_BLOCKS_MAX */

#ifdef __cplusplus
extern "C" {
#endif

#define ADMPC_SELECT_PASSES 8           /* digit passes of 8 bits over the 64-bit key */
#define ADMPC_SELECT_WORK 201376        /* int32 words of `work` */
#define ADMPC_SELECT_ENOVALID (-100)

/* log [M][14] -> bins, sel, info (WHAT IS WRITTEN above) for all K * n_gp regressors of the ensemble; n_points [3] on the HOST, one value
 * per regressor (those past n_gp are not read).  The regressors' feature and output and the centroids are read from the object's device
 * copies by pointer: a captured chain follows the centroids that admpc_quad_clusters_install or admpc_quad_ensemble_centroids_set wrote.
 * ADMPC_EINVAL, in this order: a null ensemble; an ensemble created without observe parameters; M < 0 or M > INT32_MAX; a regressor with
 * more than one feature; a null n_points; an n_points[g] outside 1 .. min(32, nbins of regressor g in every cluster); a clustering
 * feature outside 7 .. 16; then (M > 0) a null log, code, edges, work, bins, sel or info. */
int admpc_quad_ensemble_select_points(const AdmpcQuadEnsemble* e, int64_t M, const double* log, const int32_t* n_points, int32_t* code,
                                      double* edges, int32_t* work, double* bins, int32_t* sel, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_SELECT_H */
