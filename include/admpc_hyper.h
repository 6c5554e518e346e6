/*
 * admpc_hyper.h -- searching the hyperparameters of a handle's residual GP on the device: the length scales, sigma_f and the noise of
 * every regressor of admpc_learn.h, by a zooming grid search of the negative log marginal likelihood (NLL) of its points, and the fit at
 * the optimum (libadmpc.so; csrc/admpc_hyper.hip).  An addition to admpc_learn.h, whose conventions hold here: device pointers owned by
 * the caller, `stream` a hipStream_t passed as void*, 0 or a negative ADMPC_E* code returned, admpc_last_error() for the message, the
 * caller's HIP device restored, no host synchronisation and no allocation, every refusal in front of the first device call.  Both
 * functions can be captured into a graph.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/...)                                replaced by
 *   ----------------------------------------------------------------------------------  ------------------------------------
 *   src/model_fitting/gp.py:278-316          nll: K, its Cholesky, the three terms         admpc_gp_search: the NLL kernel
 *   src/model_fitting/gp.py:318-323, 337-352 minimize(L-BFGS-B) from one start, bounds     admpc_gp_search: the rounds (grid, pick, zoom)
 *   src/model_fitting/gp.py:354-363          the optimum taken over, K^-1 y at it          admpc_gp_refit
 *
 * The reference descends from ONE start; the search here evaluates up to ADMPC_GP_SEARCH_MAX candidates per regressor and round, a
 * regular grid in the logarithms of the free slots around the best candidate so far, and shrinks the grid's step after every round.
 * Not part of it: random restarts, gradients, a warm start when the statistics change (call with resume = 0 on new statistics).
 */
#ifndef ADMPC_HYPER_H
#define ADMPC_HYPER_H

#include <stdint.h>
#include "admpc_learn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADMPC_GP_SEARCH_MAX 4096      /* candidates per regressor and round */
#define ADMPC_GP_HYPER      16        /* doubles of search state per regressor */
#define ADMPC_GP_NO_OPTIMUM (-33)     /* info of a re-fit whose search found no finite NLL (pivot failures use -1 .. -32) */

typedef struct AdmpcGpSearchBox {     /* 80 bytes. Slots: length[0..2], sigma_f, noise, in NATURAL units */
    double lo[5], hi[5];              /* used slots: 0 < lo <= hi, finite; lo == hi fixes the slot; slots of unused features are not read */
} AdmpcGpSearchBox;

typedef struct AdmpcGpSearchParams {  /* 336 bytes */
    int32_t grid, rounds;             /* grid in {3,5,7,9}; rounds in [1, 64] */
    double  shrink;                   /* in (0, 1), finite */
    AdmpcGpSearchBox box[ADMPC_GP_MAX];
} AdmpcGpSearchParams;

/* The search.  The length, sigma_f and noise of obs->gp[g] are NOT read (they pass the check of obs); count_noise is kept as given.
 *
 * State, in/out: hyper [n_gp][ADMPC_GP_HYPER] doubles per regressor --
 *   0 .. 4    centre theta, the natural logarithm of the five slots            5 .. 9   step per slot in log units, 0 for a fixed slot
 *   10 .. 14  natural values v = exp(theta) of the centre, as the device's exp gave them          15   best NLL so far, +inf when none
 * (slots of unused features: theta 0, step 0, v 1).  search_info [n_gp][2] int32, out: of the last round, the index of the candidate
 * that was picked (-1 if none improved) and the number of candidates with a finite NLL.  nll [n_gp][ADMPC_GP_SEARCH_MAX]: scratch.
 *
 * resume == 0 starts: centre_d = 0.5 * (log lo_d + log hi_d), step_d = (log hi_d - log lo_d) / (grid - 1), both formed on the host in
 * double; v = exp(centre) on the device; best = +inf.  resume == 1 continues from hyper as it stands, on the same statistics: nothing
 * is initialised, so R calls of one round equal one call of R rounds bit for bit.  Then `rounds` times two launches:
 *   a. the NLL kernel, one candidate per half wave.  Candidate c < C_g = grid^(free slots of g) has one digit per free slot, slots in
 *      ascending order, the last free slot the fastest digit: theta_d = min(max(centre_d + (digit_d - (grid - 1) / 2) * step_d, log lo_d),
 *      log hi_d), every operation rounded on its own; a fixed slot keeps centre_d; v_d = exp(theta_d).  The points (Z, t, counts, ymean)
 *      are those of admpc_gp_fit from bins and min_count.  K_ij = v_3 * exp(-0.5 * sum_d (Z_i,d - Z_j,d)^2 * il_d) + delta_ij * (v_4 +
 *      count_noise / count_i), il_d = 1 / (v_d * v_d), exp as in the fit; the Cholesky of the fit, L w = t - ymean;
 *      NLL = sum_k log L_kk + 0.5 * sum_k w_k^2 + 0.5 * n * log(2 pi)    (gp.py:311-313 with noise = sigma_n^2 searched directly).
 *      A pivot that is not positive and finite, or a t_k that is not finite, gives +inf; n == 0 gives 0.  The order of the sums inside
 *      one NLL is not part of the contract.
 *   b. the pick kernel, one wave per regressor: i* = the lowest index attaining the minimum over c < C_g, where NaN and +-inf count
 *      as +inf.  If nll[i*] < best: centre <- theta(i*), v <- v(i*) (bit for bit what the NLL kernel used), best <- nll[i*], picked
 *      <- i*; otherwise picked <- -1.  step <- step * shrink, always.  From the second round on the centre candidate is the incumbent.
 *
 * ADMPC_EINVAL, in this order: obs as admpc_learn.h refuses it; sp null, grid, rounds, shrink; per regressor a bad used slot (lo not
 * > 0, hi < lo, either not finite), then a candidate count above ADMPC_GP_SEARCH_MAX (5^5 and 7^4 pass, 7^5 does not); min_count < 1;
 * resume not 0 or 1; a null array. */
int admpc_gp_search(int device, const AdmpcObserveParams* obs, const AdmpcGpSearchParams* sp, int min_count, int resume,
                    const double* bins, double* hyper, double* nll, int32_t* search_info, void* stream);

/* admpc_gp_fit with sigma_f = v_3, noise = v_4 and inv_l2_d = 1 / (v_d * v_d) taken from hyper[g][10 .. 14] (device memory): the
 * inv_l2 is formed on the device, each operation rounded on its own, and written into gp_out.  Bit for bit admpc_gp_fit where the
 * natural values equal the given ones.  Where hyper[g][15] is not finite: the empty GP and info[g] = ADMPC_GP_NO_OPTIMUM.
 * ADMPC_EINVAL, in this order: obs as admpc_learn.h refuses it; min_count < 1; a null array. */
int admpc_gp_refit(int device, const AdmpcObserveParams* obs, int min_count, const double* bins, const double* hyper,
                   AdmpcGp* gp_out, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_HYPER_H */
