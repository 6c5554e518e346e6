/*
 * admpc_quad_eval.h -- the stage that closes the reference's training pipeline, on the device (libadmpc.so; csrc/admpc_quad_eval.hip):
 * the learned GPs of a clustered ensemble evaluated on a log of sample records.  Every regressor is factored ONCE -- the fit's K, its
 * Cholesky factor L, alpha, and W = L^-1, which the fit throws away -- and one pass over the records then gives, per record, the
 * cluster, the posterior mean and the posterior standard deviation of every regressor, and per cluster and regressor the error
 * statistics the reference prints with the coverage of the 3-std band it plots.  The log does not leave the device.  With it
 * record -> prune -> cluster -> search -> evaluate is one chain of launches on one stream: a model can be accepted or rejected, before
 * an install for instance, without a host round trip.  An addition to admpc_quad_ensemble.h, admpc_quad_hyper.h, admpc_quad_clusters.h
 * and admpc_quad_prune.h, whose conventions hold here: device pointers owned by the caller, dense, fp64; `stream` a hipStream_t passed as
 * void*; 0 or a negative ADMPC_E* code returned, admpc_last_error() of admpc.h for the message; the caller's HIP device restored; no host
 * synchronisation and no allocation in any entry, each of which can be captured into a graph; every refusal in front of the first device
 * call, in the order it is listed, under the entry's own name; an empty array (M == 0) is a no-op.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/...)                                  replaced by
 *   ----------------------------------------------------------------------------------------  ------------------------------------
 *   model_fitting/gp_fitting.py:304-311, 314-348  gp_evaluate_test_set: the data set loaded,      admpc_quad_ensemble_factor once, then
 *                                     the ensemble's predict over it, the errors printed         admpc_quad_ensemble_evaluate over the log
 *   model_fitting/gp_visualization.py:74-93  GPEnsemble.predict(x, u, return_std=True) over      the same entry: per_record [M][3][2]
 *                                     every record; nominal against augmented mean absolute      and stats [K][3][8]
 *                                     error (printed as "RMSE"), the 3-std band
 *   model_fitting/gp.py:632-736       GPEnsemble.predict: the GP of every record's cluster       the evaluate kernel: route, mean, std
 *   model_fitting/gp.py:738-770       select_gp: the nearest centroid per record                 quad_route_dev.h's body, as the bin kernel routes
 *   model_fitting/gp.py:403-444       CustomGPRegression.predict: mu = k' K^-1 y + ymean,        mu = ymean + k' alpha; var = k_ss - |W k|^2 with
 *                                     var = k_ss - k' K^-1 k, k_ss = sigma_f + 1e-8 (:427)        W = L^-1, L L' = K: the same quadratic form
 *   model_fitting/gp.py:361-363       fit: K_inv = inv(K), K_inv_y, y_mean kept                  admpc_quad_ensemble_factor: W, alpha, ymean kept
 *
 * NOT offered:
 *   - a NaN standard deviation.  The reference takes sqrt of a variance that rounding has made negative and returns NaN
 *     (gp.py:436-441).  Here the variance is CLIPPED at 0, std = sqrt(max(var, 0)), and every clip is counted (stats entry 7);
 *   - covariance propagation through the horizon (the reference raises NotImplementedError there with a GP, quad_3d_opt_utils.py:123);
 *   - sample_y, the plots and the dense-GP resampling of gp_visualization.py;
 *   - training-point selection (distance_maximizing_points) by THESE entries: they factor whatever the bins hold, the means of a grid or
 *     the records that admpc_quad_select.h picks from the log;
 *   - a log for QuadFleet and for flights to targets: the entries work on ANY array of records, the fleet that keeps one is the
 *     clustered ensemble's;
 *   - the car.
 *
 * THE FACTOR.  factor [K][3][ADMPC_EVAL_FACTOR] doubles, one self-contained block per (cluster, regressor); integers are stored as
 * doubles:
 *   [0] n   [1] n_feat   [2 .. 4] feat   [5] out   [6] sigma_f   [7 .. 9] inv_l2   [10] ymean   [11 .. 15] 0
 *   [16 .. 111] Z [3][32]   [112 .. 143] alpha [32]   [144 .. 671] W = L^-1, lower triangular, packed by rows: W_ij at 144 + i (i + 1) / 2 + j
 * n, Z, alpha and ymean are the bits admpc_quad_ensemble_fit / _refit write into an AdmpcGp from the same bins and hyperparameters (the
 * kernels share the text of the points, K, the Cholesky factor and the two solves, gp_fit_dev.h).  Rows of Z, alpha and W past n are 0.
 * THE EMPTY FACTOR -- no bin with min_count samples, a failed pivot, a search without an optimum -- has n = 0, ymean = 0 and the
 * hyperparameters it was asked for: its mean is 0 and its variance the prior's, sigma_f + 1e-8.
 *
 * WHICH RECORDS TAKE PART in an evaluation.  records [M][14] in admpc_quad_learn.h's layout.  A record takes part if its flag (entry 13)
 * is exactly 1.0, or ADMPC_QUAD_REC_PRUNED (2.0) when take_pruned is 1 (the reference's pruned=False: the whole data set), and its
 * entries 0 .. 12 are finite.  Every other record is counted in info and otherwise absent.
 *
 * PER RECORD that takes part: the cluster c is the centroid of the ensemble's DEVICE copy nearest to the record's own clustering
 * features (quad_route_dev.h; ties to the lower index), exactly as the ensemble's bin kernel routes.  For regressor g < n_gp of
 * cluster c, with z_d = record[feat_d - 7]:
 *   k_i = sigma_f exp(-1/2 sum_d (z_d - Z_d,i)^2 inv_l2_d)     mu = ymean + sum_i k_i alpha_i     v = W k
 *   var = (sigma_f + 1e-8) - sum_i v_i^2                          std = sqrt(max(var, 0))
 *   y = record[10 + out - 7]                                      r = y - mu
 * With drag (device [3], what admpc_quad_rdrv_fit writes) r = y - mu - D_a v_b,a for a = out - 7, v_b = record[0 .. 2]: a learned
 * linear drag, alone (empty factors) or under the GPs, is scored on the same log.  per_record, NULL or [M][3][2]: mu (the drag term
 * included) and std of regressor g < n_gp; NaN in both for a record that does not take part; regressors past n_gp are not written.
 *
 * THE STATISTICS.  stats [K][3][ADMPC_EVAL_STATS], per (cluster, regressor) over the records routed to the cluster:
 *   [0] n   [1] sum |y|   [2] sum y^2   [3] sum |r|   [4] sum r^2   [5] sum std   [6] records with |r| <= 3 std   [7] clipped variances
 * sum |y| / n is the reference's nominal error, sum |r| / n its augmented one (gp_visualization.py:92-93, per second: times dt for its
 * velocity units).  The rows of regressors past n_gp are 0.  info [4] int32: the status, 0 or ADMPC_EVAL_ENOVALID if no record takes
 * part (stats is then all 0); the records that took part; those skipped by their flag; those skipped as not finite.
 *
 * DETERMINISM.  No floating-point atomics.  The grid of the evaluate kernel is min(ceil(M / 256), ADMPC_GMM_BLOCKS_MAX) blocks of 256
 * threads, a function of M alone; a wave adds its lanes by a shuffle tree, a block its four waves in their order, every block writes one
 * row of partial [ADMPC_GMM_BLOCKS_MAX][K * 3 * 8], and a one-wave finish launch adds the rows in a fixed order (lane l rows l, l + 64, ..., then the shuffle tree).  The two skip counts are
 * added by INTEGER atomics, one per block and count.  Two runs on the same input give the same bits.  The order inside the sums is not
 * part of the contract.
 *
 * THE KERNEL.  One lane per record.  A block walks the clusters; a cluster that none of its 256 records routes to is skipped (a barrier
 * with a vote), and so is a wave none of whose lanes does (a ballot).  The three packed factors of the cluster in turn are staged in
 * LDS (header, Z, alpha and the n (n + 1) / 2 doubles of W in use), where every read is a broadcast: the active lanes share the cluster.
 * A lane keeps its n kernel values in registers (the loops over the 32 points are unrolled under uniform guards) and forms v row by
 * row, up to 528 multiply-adds.  The alternative mapping -- tiles of 16 records of one cluster against W' on v_mfma_f64_16x16x4_f64 --
 * has not been built; profiles/HISTORY.md has the note.  Resources on gfx950 (make resources): evaluate 161 VGPRs, 22 560 bytes
 * of LDS; factor 51 VGPRs, 18 176 bytes of LDS; finish 48 VGPRs; scratch 0 in all.
 *
 * Measured on one MI355X at B = 4096, 60 logged steps of the noisy simulator (M = 245 760 records), N = 10, three 32-point regressors per
 * cluster, clusters on v_x at the quantiles of the log, captured graphs replayed, both routes in one session, medians of three
 * (scripts/quad_eval_time.py), microseconds at K = 1 / 4 / 8: the factor launch 77.3 / 78.4 / 79.4; the evaluation (zero,
 * evaluate, finish) 169.3 / 597.0 / 1195.7, with per_record 168.7 / 604.5 / 1210.5; by kernel trace the evaluate kernel 609.6 (148.9 ... 1171.2: K = 1 ... 8), the finish 38.5 (8.8 ... 72.1), the factor kernel 71.9 (67.5 ... 76.2), the zero kernel 4.2.
 * The route they replace -- the log to the host, the numpy spec's predict over all records, the statistics -- 380287 / 282892 / 268830:
 * 2246 / 474 / 225 times the evaluation.  The evaluate kernel's time grows with K because a wave runs the whole loop once for every
 * cluster among its 64 records: the records are not sorted by cluster.  The first finish kernel (a lane per column, 256 dependent loads)
 * took 57.7 to 176.3; a lane per row and the shuffle tree take 8.8 to 72.1 (K = 1 to 8).
 */
#ifndef ADMPC_QUAD_EVAL_H
#define ADMPC_QUAD_EVAL_H

#include <stdint.h>
#include "admpc_quad_ensemble.h"
#include "admpc_quad_clusters.h"    /* ADMPC_GMM_BLOCKS_MAX */
#include "admpc_quad_prune.h"       /* ADMPC_QUAD_REC_PRUNED */

#ifdef __cplusplus
extern "C" {
#endif

#define ADMPC_EVAL_FACTOR 672           /* doubles per (cluster, regressor) of `factor` */
#define ADMPC_EVAL_STATS 8              /* doubles per (cluster, regressor) of `stats` and of a row of `partial` */
#define ADMPC_EVAL_ENOVALID (-100)

/* bins [K][3][32][5] (and hyper, NULL or [K][3][16]) -> factor, info [K][3] int32 (THE FACTOR above).  One wave per (cluster,
 * regressor), all in one launch; the regressors are read from the object's device copies by pointer, as admpc_quad_ensemble_refit reads
 * them.  hyper == NULL: each block's given hyperparameters, as admpc_quad_ensemble_fit; otherwise the natural values a search left in
 * hyper, read exactly as admpc_quad_ensemble_refit reads them -- a search without an optimum gives the empty factor and info
 * ADMPC_GP_NO_OPTIMUM.  The diagonal of K is noise + count_noise / count_i, as in the fit.  info is n, or -(k + 1) for pivot k that is not
 * positive and finite, as the fit reports it.  Entries of regressors past n_gp are not written.
 * ADMPC_EINVAL, in this order: a null ensemble; an ensemble created without observe parameters; min_count < 1; a null bins, factor or
 * info. */
int admpc_quad_ensemble_factor(const AdmpcQuadEnsemble* e, int min_count, const double* bins, const double* hyper, double* factor,
                               int32_t* info, void* stream);

/* records [M][14], factor -> per_record (NULL or [M][3][2]), stats [K][3][8], info [4] int32, through partial
 * [ADMPC_GMM_BLOCKS_MAX][K * 3 * 8] (WHICH RECORDS TAKE PART, PER RECORD, THE STATISTICS above).  drag: NULL or device [3].  Three
 * launches: info zeroed (one wave), the evaluate kernel, the one-wave finish.  The factor, the drag and the centroids are read by pointer: a captured
 * evaluation picks up a new factor at its next replay.
 * ADMPC_EINVAL, in this order: a null ensemble; a clustering feature outside 7 .. 16 (the record holds no others); M < 0 or
 * M > INT32_MAX; take_pruned other than 0 and 1; then (M > 0) a null records, factor, partial, stats or info. */
int admpc_quad_ensemble_evaluate(const AdmpcQuadEnsemble* e, int64_t M, const double* records, int take_pruned, const double* factor,
                                 const double* drag, double* per_record, double* partial, double* stats, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_EVAL_H */
