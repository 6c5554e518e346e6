// admpc_hyper.hip -- searching the hyperparameters of a handle's residual GP on the device (include/admpc_hyper.h): a zooming grid
// search of the negative log marginal likelihood (NLL) of a regressor's points, and the fit at the optimum.  The kernels are thin callers
// of the bodies in gp_search_dev.h, which the kernels of a clustered ensemble (admpc_quad_hyper.hip) share; here the regressors and the
// search descriptors travel in the kernel arguments, by value.
//
//   init   admpc_gp_search_init_kernel  a block per regressor: centre and step as the host formed them, v = exp(centre), best = +inf
//   nll    admpc_gp_nll_kernel          a candidate per HALF wave, 8 candidates per block of 4 waves; 35 KB of LDS a block, four blocks a CU
//   pick   admpc_gp_pick_kernel         a wave per regressor: the lowest index of the minimum, the new centre, the step shrunk
//   refit  admpc_gp_refit_kernel        the fit's body (gp_fit_dev.h) at the natural values the search left in `hyper`
//
// The host side behind the check of the observe parameters serves both vehicles (admpc_hyper_search, admpc_hyper_refit: the quadrotor's
// entries of admpc_quad_hyper.hip call them with their ranges' unused feature), as admpc_learn_fit does for the fit.
#include <stdio.h>
#include <math.h>
#include "admpc_host.h"
#include "../../include/admpc_hyper.h"

#define NX ADMPC_NX
#define NU ADMPC_NU
#define NY ADMPC_NY
#include "gp_search_dev.h"

struct SearchArgs {
    int grid, half;                          // half = (grid - 1) / 2
    double shrink;
    SearchGp s[ADMPC_GP_MAX];
    double* hyper;                           // [n_gp][HYP]
    double* nll;                             // [n_gp][ADMPC_GP_SEARCH_MAX]
    int32_t* info;                           // [n_gp][2]
};

namespace {

#include "model_dev.h"

}  // namespace

// grid n_gp, one wave each; lane 0 writes the 16 doubles of the regressor
__global__ __launch_bounds__(WAVE) void admpc_gp_search_init_kernel(const SearchArgs q)
{
    const int g = (int)blockIdx.x;
    gp_search_init_body(q.s[g], q.hyper + (long)g * HYP);
}

// grid (ceil(max C_g / 8), n_gp), 4 waves each: candidate 8 * blockIdx.x + 2 * wave + half of regressor blockIdx.y.
__global__ __launch_bounds__(NLL_WAVES * WAVE) void admpc_gp_nll_kernel(const LearnArgs a, const SearchArgs q)
{
    const int g = (int)blockIdx.y;
    gp_nll_body(a, g, q.s[g], q.grid, q.half, q.hyper + (long)g * HYP, q.nll + (long)g * ADMPC_GP_SEARCH_MAX);
}

// grid n_gp, one wave each
__global__ __launch_bounds__(WAVE) void admpc_gp_pick_kernel(const SearchArgs q)
{
    const int g = (int)blockIdx.x;
    gp_pick_body(q.s[g], q.grid, q.half, q.shrink, q.hyper + (long)g * HYP, q.nll + (long)g * ADMPC_GP_SEARCH_MAX, q.info + 2 * g);
}

// grid n_gp, one wave each: the fit at the natural values of the search's centre
__global__ __launch_bounds__(WAVE) void admpc_gp_refit_kernel(const LearnArgs a, const double* __restrict__ hyper)
{
    const int g = (int)blockIdx.x;
    gp_refit_body(a, g, hyper + (long)g * HYP);
}

// The refusals of a search block and the descriptors of its first n_gp boxes (gp_search_dev.h).
extern "C" int admpc_hyper_form(const char* who, int n_gp, const AdmpcGpBins* gp, const AdmpcGpSearchParams* sp, SearchGp* s, int* cmax)
{
    if (!sp) return admpc_learn_refuse(who, "the search parameters are not set");
    if (sp->grid != 3 && sp->grid != 5 && sp->grid != 7 && sp->grid != 9) return admpc_learn_refuse(who, "grid must be 3, 5, 7 or 9");
    if (sp->rounds < 1 || sp->rounds > 64) return admpc_learn_refuse(who, "rounds must be in [1, 64]");
    if (!(sp->shrink > 0.0 && sp->shrink < 1.0)) return admpc_learn_refuse(who, "shrink must be in (0, 1)");
    *cmax = 1;
    for (int g = 0; g < n_gp; ++g) {
        const AdmpcGpSearchBox& b = sp->box[g];
        SearchGp& S = s[g];
        S = SearchGp();
        char what[120];
        for (int d = 0; d < NSLOT; ++d) {
            if (d < 3 && d >= gp[g].n_feat) continue;                  // the slot of an unused feature is not read: theta 0, step 0, v 1
            if (!(b.lo[d] > 0.0) || !(b.hi[d] >= b.lo[d]) || !isfinite(b.lo[d]) || !isfinite(b.hi[d])) {
                snprintf(what, sizeof what, "regressor %d: slot %d of the box needs 0 < lo <= hi, finite", g, d);
                return admpc_learn_refuse(who, what);
            }
            S.free_[d] = b.hi[d] != b.lo[d];
            S.loglo[d] = log(b.lo[d]); S.loghi[d] = log(b.hi[d]);
            S.centre0[d] = 0.5 * (S.loglo[d] + S.loghi[d]);
            S.step0[d] = S.free_[d] ? (S.loghi[d] - S.loglo[d]) / (double)(sp->grid - 1) : 0.0;
        }
    }
    for (int g = 0; g < n_gp; ++g) {
        SearchGp& S = s[g];
        char what[120];
        long C = 1;
        for (int d = 0; d < NSLOT; ++d) if (S.free_[d]) C *= sp->grid;
        if (C > ADMPC_GP_SEARCH_MAX) {
            snprintf(what, sizeof what, "regressor %d: %ld candidates per round, at most %d (fix a slot or take a smaller grid)", g, C, ADMPC_GP_SEARCH_MAX);
            return admpc_learn_refuse(who, what);
        }
        S.C = (int)C;
        if (S.C > *cmax) *cmax = S.C;
    }
    return ADMPC_OK;
}

// admpc_gp_search behind the check of the observe parameters, for either vehicle
extern "C" int admpc_hyper_search(const char* who, int device, int n_gp, const AdmpcGpBins* gp, int unused_feat, const AdmpcGpSearchParams* sp,
                                  int min_count, int resume, const double* bins, double* hyper, double* nll, int32_t* search_info, void* stream)
{
    SearchArgs q = SearchArgs();
    int cmax = 1;
    const int rc = admpc_hyper_form(who, n_gp, gp, sp, q.s, &cmax);
    if (rc) return rc;
    q.grid = sp->grid; q.half = (sp->grid - 1) / 2; q.shrink = sp->shrink;
    if (min_count < 1) return admpc_learn_refuse(who, "min_count must be at least 1");
    if (resume != 0 && resume != 1) return admpc_learn_refuse(who, "resume must be 0 or 1");
    if (!bins || !hyper || !nll || !search_info) return admpc_learn_refuse(who, "null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    LearnArgs l = LearnArgs();
    admpc_learn_fill(l, n_gp, gp, unused_feat);
    l.min_count = (double)min_count; l.bins = const_cast<double*>(bins);
    q.hyper = hyper; q.nll = nll; q.info = search_info;
    const dim3 one((unsigned)n_gp), cand((unsigned)((cmax + NLL_CAND - 1) / NLL_CAND), (unsigned)n_gp);
    if (!resume) {
        hipLaunchKernelGGL(admpc_gp_search_init_kernel, one, dim3(WAVE), 0, (hipStream_t)stream, q);
        if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_gp_search_init_kernel: launch failed");
    }
    for (int it = 0; it < sp->rounds; ++it) {
        hipLaunchKernelGGL(admpc_gp_nll_kernel, cand, dim3(NLL_WAVES * WAVE), 0, (hipStream_t)stream, l, q);
        if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_gp_nll_kernel: launch failed");
        hipLaunchKernelGGL(admpc_gp_pick_kernel, one, dim3(WAVE), 0, (hipStream_t)stream, q);
        if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_gp_pick_kernel: launch failed");
    }
    return ADMPC_OK;
}

// admpc_gp_refit behind the check of the observe parameters, for either vehicle
extern "C" int admpc_hyper_refit(const char* who, int device, int n_gp, const AdmpcGpBins* gp, int unused_feat, int min_count, const double* bins,
                                 const double* hyper, AdmpcGp* gp_out, int32_t* info, void* stream)
{
    if (min_count < 1) return admpc_learn_refuse(who, "min_count must be at least 1");
    if (!bins || !hyper || !gp_out || !info) return admpc_learn_refuse(who, "null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    LearnArgs l = LearnArgs();
    admpc_learn_fill(l, n_gp, gp, unused_feat);
    l.min_count = (double)min_count; l.bins = const_cast<double*>(bins); l.out = gp_out; l.info = info;
    hipLaunchKernelGGL(admpc_gp_refit_kernel, dim3((unsigned)n_gp), dim3(WAVE), 0, (hipStream_t)stream, l, hyper);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_gp_refit_kernel: launch failed");
    return ADMPC_OK;
}

extern "C" {

int admpc_gp_search(int device, const AdmpcObserveParams* obs, const AdmpcGpSearchParams* sp, int min_count, int resume,
                    const double* bins, double* hyper, double* nll, int32_t* search_info, void* stream)
{
    const int rc = admpc_observe_params_check("admpc_gp_search", obs);
    return rc ? rc : admpc_hyper_search("admpc_gp_search", device, obs->n_gp, obs->gp, CAR_LEARN.feat_lo, sp, min_count, resume, bins, hyper, nll,
                                        search_info, stream);
}

int admpc_gp_refit(int device, const AdmpcObserveParams* obs, int min_count, const double* bins, const double* hyper,
                   AdmpcGp* gp_out, int32_t* info, void* stream)
{
    const int rc = admpc_observe_params_check("admpc_gp_refit", obs);
    return rc ? rc : admpc_hyper_refit("admpc_gp_refit", device, obs->n_gp, obs->gp, CAR_LEARN.feat_lo, min_count, bins, hyper, gp_out, info, stream);
}

}  // extern "C"
