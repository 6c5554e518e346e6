/*
 * admpc_quad_prune.h -- the two stages of the reference's training pipeline that stand between the recorded flight and the models, on
 * the device (libadmpc.so; csrc/admpc_quad_prune.hip): the pruning of the data set, which rewrites the flags of a log of sample records,
 * and the RDRv model, Faessler's diagonal linear drag matrix fitted from the records that are left and installed into a handle.  With it
 * record -> prune -> cluster -> fit -> install is one chain of launches on one stream.  An addition to admpc_quad_learn.h and
 * admpc_quad_clusters.h, whose conventions hold here: device pointers owned by the caller, dense, fp64; `stream` a hipStream_t passed as
 * void*; 0 or a negative ADMPC_E* code returned, admpc_last_error() of admpc.h for the message; the caller's HIP device restored; no host
 * synchronisation and no allocation in any entry, each of which can be captured into a graph; every refusal in front of the first device
 * call, in the order it is listed; an empty array (M == 0) is a no-op.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/...)                                  replaced by
 *   ----------------------------------------------------------------------------------------  ------------------------------------
 *   model_fitting/gp_common.py:64-66, 101-112  GPDataset.__init__ -> prune(): the indices that   admpc_quad_records_prune: the flag of every
 *                                     every later x, y of the data set is taken at              record, 1.0 kept, 2.0 pruned
 *   utils/utils.py:458-533            prune_dataset: the velocity cap, the four error            the same entry: range, edges, count, mark
 *                                     histograms (one per body axis, one of the norm)
 *   model_fitting/gp_common.py:224-271  GaussianMixture(n_clusters).fit(x_pruned); the GP fits    admpc_quad_clusters_fit, admpc_quad_clusters_rebin,
 *                                     on the pruned set                                          admpc_quad_ensemble_fit / _search as they stand:
 *                                                                                              they take a record only if its flag is 1.0
 *   model_fitting/rdrv_fitting.py:27-33  linear_rdrv_fitting: LinearRegression(fit_intercept=    admpc_quad_rdrv_fit
 *                                     False) per axis on the pruned set
 *   experiments/comparative_experiment.py  the RDRv model loaded into the MPC (rdrv_d_mat)       admpc_quad_rdrv_install (no host in between)
 *
 * NOT offered:
 *   - the evaluation of the fitted drag or of the GPs on a data set by THESE entries: admpc_quad_eval.h scores either, or the drag under
 *     the GPs, on a log of records, pruned ones included or not;
 *   - the reference's plotting of the histograms (utils.py:476-485, 508-510, 519-530);
 *   - the second normalisation of the NORM's ratios (utils.py:507, 513: h / sum(h), then h[j] / sum(h) again): all four columns compare
 *     count / n_valid with thresh.  The two differ only where a ratio lies within rounding of thresh;
 *   - np.linspace's other formula for a step that underflows to 0 (a range below 2^-1022 * n_bins);
 *   - pruning that feeds anything but flags: no compaction of the log, no index list;
 *   - a log for QuadFleet and for flights to targets (admpc_quad_targets.h): the entries work on ANY array of records, the fleet that
 *     keeps one is the clustered ensemble's;
 *   - RDRv in covariance mode, a full (non-diagonal) drag matrix, an intercept; handles in SQP mode.  admpc_quad_sqp.h has the SQP loop that
 *     one-handle rollouts fly.
 *
 * THE RECORDS are admpc_quad_learn.h's [14]: entries 0 .. 2 the body-frame velocity v_b, 10 .. 12 the residual y, entry 13 the flag.
 * ADMPC_QUAD_REC_PRUNED (2.0) is a third value of the flag next to 0.0 (not valid) and 1.0 (valid, kept): the pack kernel of the EM and the
 * bin body take a record only if its flag is exactly 1.0, so a pruned record is in no fit, and no kernel of theirs changes.
 *
 * WHICH RECORDS TAKE PART in a prune: flag 1.0 or 2.0, and entries 0 .. 2 and 10 .. 12 finite.  Every other record is left as it is and
 * counted nowhere.  One that takes part leaves with flag 1.0 or 2.0; only entry 13 of any record is ever written.  The result is a
 * function of the data, not of earlier prunes: pruning twice gives the bits of pruning once, and x_cap = +inf with thresh = 0 restores
 * every flag to 1.0.
 *
 * WHAT IS PRUNED: the reference's rule, quirks included.  The columns are c_0 .. c_2 = y_0 .. y_2 and c_3 = sqrt((y_0^2 + y_1^2) + y_2^2),
 * every operation rounded on its own (no contraction), the square root correctly rounded as numpy's.
 *   cap         |v_b,i| > x_cap for some i.
 *   histograms  per column over ALL records that take part, capped ones included: lo / hi the column's min / max, lo - 0.5 / hi + 0.5 if
 *               they are equal (np.histogram); the edges np.linspace(lo, hi, n_bins + 1): e_j = lo + j * ((hi - lo) / n_bins), e_n = hi;
 *               the bin of v by np.histogram's uniform-bin rule: idx = trunc(((v - lo) / (hi - lo)) * n_bins), n_bins becomes
 *               n_bins - 1, one less if v < e[idx], one more if v >= e[idx + 1] and idx is not the last bin (then held into
 *               0 .. n_bins - 1, which changes nothing for a finite range).  Bin j is SPARSE if (double)count_j / (double)n_valid <
 *               thresh.  A record is pruned if its bin is sparse, and also if it lies exactly on e[idx], idx > 0, and bin idx - 1 is
 *               sparse: the reference tests bins[j + 1] >= y >= bins[j], closed on both sides.
 * A quirk that follows and is kept: a CONSTANT column has lo = v - 0.5, hi = v + 0.5, so for an even n_bins every record lies on the
 * edge e[n_bins / 2], the bin below it is empty, and with thresh > 0 everything is pruned.
 *
 * THE STATE of a prune.  partial [ADMPC_GMM_BLOCKS_MAX][ADMPC_PRUNE_PARTIAL]: per block min and max of c_0 .. c_3 (min_0, max_0, min_1,
 * ...) and the number of records that take part.  edges [4][ADMPC_PRUNE_BINS_MAX + 1]: e_0 .. e_n of every column, so lo = edges[c][0],
 * hi = edges[c][n_bins]; the rest of a row is not written.  counts [4][ADMPC_PRUNE_BINS_MAX] int32: the histograms, the bins past
 * n_bins at 0.  info [8] int32:
 *   [0]       status: 0, or ADMPC_PRUNE_ENOVALID if no record takes part; then no record and no edge is written, counts and
 *             info[1 .. 7] are 0
 *   [1]       n_valid, the records that take part
 *   [2]       n_kept
 *   [3]       pruned by the cap
 *   [4 .. 6]  pruned by the histogram of axis 0, 1, 2
 *   [7]       pruned by the histogram of the norm
 * The causes overlap: n_valid - n_kept is at most their sum.
 *
 * THE STATE of an RDRv fit.  partial [ADMPC_GMM_BLOCKS_MAX][ADMPC_RDRV_PARTIAL]: per block sum v_b,i y_i and sum v_b,i^2 for i = 0, 1, 2
 * (xy_0, xx_0, xy_1, ...) and the number of records.  d_out [3]: D_i = S_xy / S_xx, 0 for an axis that is not asked.  sums [3][2]: S_xy,
 * S_xx, 0 for an axis that is not asked.  info [2] int32: n_used; status: 0, or -(i + 1) for the lowest asked axis whose S_xx is not
 * positive and finite or whose D_i is not finite.
 *
 * DETERMINISM.  No floating-point atomics.  The grid of every kernel over the records is min(ceil(M / 256), ADMPC_GMM_BLOCKS_MAX) blocks
 * of 256 threads, a function of M alone; minima, maxima and integer counts do not depend on an order, the histograms and the tallies are
 * added by INTEGER atomics, and the sums of the drag fit go through one row of partial per block, which one wave adds in a fixed order.
 * Two runs on the same input give the same bits.  The order inside the sums of the drag fit is not part of the contract.
 *
 * Measured on one MI355X at B = 4096, 60 logged steps of the noisy simulator (M = 245 760 records), K = 1, N = 10, captured graphs replayed,
 * both routes in one session, medians of three (scripts/quad_prune_time.py), microseconds: the prune 39.8 (by kernel
 * trace range 6.8, edges 4.7, count 11.4, mark 11.6); the drag fit with one install 18.0 (sums 5.6, finish 5.3, install 3.9); a fleet's
 * prune_log() with the re-bin of the 60 steps 3699.  The route they replace -- the log to the host 4489, the numpy restatement of
 * prune_dataset 30 672, LinearRegression per axis 15 833, the flags uploaded 785 -- 51 778: 896 times the prune and the fit.  99.4 % of
 * the records were kept; the flags equal the host route's, the drag differs from LinearRegression's by 2.2e-16.  The chain is four
 * launches that depend on each other, the shortest of which (edges, one wave) takes 4.7.  With one atomic per WAVE and tally the mark
 * kernel took 27.6 and the chain 55.5; with one per block and tally, 11.6 and 39.8.
 */
#ifndef ADMPC_QUAD_PRUNE_H
#define ADMPC_QUAD_PRUNE_H

#include <stdint.h>
#include "admpc_quad_clusters.h"    /* ADMPC_GMM_BLOCKS_MAX */

#ifdef __cplusplus
extern "C" {
#endif

#define ADMPC_QUAD_REC_PRUNED 2.0       /* entry 13 of a record that a prune took out */
#define ADMPC_PRUNE_BINS_MAX 256
#define ADMPC_PRUNE_PARTIAL 9           /* doubles per row of a prune's `partial`: min / max of four columns, the count */
#define ADMPC_RDRV_PARTIAL 7            /* doubles per row of a drag fit's `partial`: S_xy, S_xx of three axes, the count */
#define ADMPC_PRUNE_ENOVALID (-100)

/* records [M][14], in/out: utils.prune_dataset(v_b, y, x_cap, n_bins, thresh) over the records that take part, the result in their
 * flags (WHAT IS PRUNED above).  Four launches, whatever the data:
 *   range   every block reduces min / max of the four columns and the count over its records: one row of partial.
 *   edges   one wave: reduces the rows, writes edges, zeroes counts and info[2 .. 7], sets info[0] and info[1].
 *   count   the edges and four integer histograms in LDS; every block adds its histograms to counts by integer atomics.
 *   mark    the edges and the sparse flags (from counts and n_valid) in LDS; a thread strides over its records, writes entry 13 of
 *           each that takes part where it changes, and the block adds its tallies to info[2 .. 7] by integer atomics, one per tally.
 * count and mark read the status and return at once if it is set.  x_cap = +inf is "no cap" (the reference's x_cap=None).
 * ADMPC_EINVAL, in this order: M < 0 or M > INT32_MAX; n_bins outside 1 .. ADMPC_PRUNE_BINS_MAX; a thresh outside [0, 1] or NaN; an x_cap
 * that is not > 0; then (M > 0) a null records, partial, edges, counts or info. */
int admpc_quad_records_prune(int device, int64_t M, double* records, double x_cap, int n_bins, double thresh, double* partial,
                             double* edges, int32_t* counts, int32_t* info, void* stream);

/* records [M][14] -> d_out, sums, info (THE STATE of an RDRv fit above): rdrv_fitting.linear_rdrv_fitting over the records whose flag is
 * exactly 1.0, for the axes of the 3-bit mask `axes` (bit i: body axis i, the reference's feature 7 + i).  Two launches: every block
 * writes one row of partial; one wave adds the rows in a fixed order and divides.  A record with flag 1.0 and a value that is not finite
 * is not skipped: it shows in the status.
 * ADMPC_EINVAL, in this order: M < 0 or M > INT32_MAX; axes outside 1 .. 7; then (M > 0) a null records, partial, d_out, sums or info. */
int admpc_quad_rdrv_fit(int device, int64_t M, int axes, const double* records, double* partial, double* d_out, double* sums,
                        int32_t* info, void* stream);

/* One wave.  If the status info[1] of the fit is 0 and d_dev [3] is finite: d_dev into rdrv of the handle's DEVICE configuration and
 * installed [1] int32 = 1.  Otherwise nothing moves and installed = 0.  The values are SET, not added: the residual they were fitted to
 * must have been observed against a model without RDRv.  The host copy of the handle's configuration is not changed.  The solve kernels
 * take the configuration by pointer: a captured rollout flies the new drag at its next replay.  The caller orders the install against
 * the solves of the handle (the same stream does).
 * ADMPC_EINVAL, in this order: a null handle; a null array. */
int admpc_quad_rdrv_install(AdmpcQuadSolver* s, const double* d_dev, const int32_t* info, int32_t* installed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_PRUNE_H */
