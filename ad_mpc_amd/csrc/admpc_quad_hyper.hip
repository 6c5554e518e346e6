// admpc_quad_hyper.hip -- searching the hyperparameters of the quadrotor's residual GPs on the device (include/admpc_quad_hyper.h).
//
// One handle: admpc_quad_gp_search and admpc_quad_gp_refit are the car's entries behind the quadrotor's check of its observe parameters
// (admpc_hyper.hip: admpc_hyper_search, admpc_hyper_refit, which launch that unit's kernels); nothing of a vehicle enters an NLL.
//
// A clustered ensemble: all K * n_gp regressors in ONE chain of launches.  The kernels of admpc_hyper.hip take their regressors and
// search descriptors by value, 136 + 184 bytes per regressor; 24 regressors come to 7.7 KB, past the 4 KB of kernel arguments.  The
// kernels here run the same bodies (gp_search_dev.h, gp_fit_dev.h) and take the regressors -- the object's device copy [K][3] -- and the
// descriptors -- a second device copy, written by admpc_quad_ensemble_set_search -- by pointer.  A block copies the one regressor and the
// one descriptor it works on into locals and hands the bodies a LearnArgs of that ONE regressor at the constant index 0 (a variable index
// into a local block would live in scratch), as admpc_quad_ensemble_bin_kernel does.
//
//   init   admpc_quad_ensemble_search_init_kernel  grid K * n_gp, one wave each
//   nll    admpc_quad_ensemble_nll_kernel          grid (ceil(max C / 8), K * n_gp), 4 waves each; a block whose first candidate is past
//                                                  the C of ITS regressor returns in front of every barrier (the boxes are free per
//                                                  cluster, so C differs across blockIdx.y)
//   pick   admpc_quad_ensemble_pick_kernel         grid K * n_gp, one wave each
//   refit  admpc_quad_ensemble_refit_kernel        grid K * n_gp, one wave each
//
// No atomics, no grid that depends on data.  Regressor (c, g) lives at the flat index c * 3 + g of every array; the entries of a regressor
// past n_gp are not touched.
#include <math.h>
#include "admpc_host.h"
#include "../../include/admpc_quad_hyper.h"

#define NX ADMPC_NX           // model_dev.h (exp_nonpos, which the bodies of gp_fit_dev.h and gp_search_dev.h name) wants the car's dimensions defined
#define NU ADMPC_NU
#define NY ADMPC_NY
#include "gp_search_dev.h"    // WAVE, NPT, ACC, NLL_WAVES, NLL_CAND, HYP; LearnGp, LearnArgs, SearchGp; the bodies; admpc_hyper_*
#define KMAX ADMPC_QUAD_CLUSTERS_MAX
#define GMAX ADMPC_QUAD_GP_MAX

// the device copy of an ensemble's search: what the K blocks agree in, and a descriptor per (cluster, regressor)
struct EnsembleSearchDev {
    int grid, half;                           // half = (grid - 1) / 2
    double shrink;
    SearchGp s[KMAX * GMAX];
};

// what one launch of the kernels below works on (passed by value: 80 bytes whatever K is)
struct EnsembleSearchArgs {
    int n_gp;
    double min_count;
    const LearnGp* gp;                        // [K][GMAX], the object's
    const EnsembleSearchDev* sd;              // the object's
    const double* bins;                       // [K][GMAX][NPT][ACC]
    double* hyper;                            // [K][GMAX][HYP]
    double* nll;                              // [K][GMAX][ADMPC_GP_SEARCH_MAX]
    int32_t* search_info;                     // [K][GMAX][2]
    AdmpcGp* out;                             // [K][GMAX]
    int32_t* info;                            // [K][GMAX]
};

namespace {

#include "model_dev.h"

// block y of a launch over K * n_gp regressors -> the flat index of regressor (c, g)
__device__ __forceinline__ int flat_index(const int y, const int n_gp) { return (y / n_gp) * GMAX + y % n_gp; }

// the LearnArgs of regressor i alone, at index 0: its bins, its output record and its info are at the front of what the bodies are given
__device__ __forceinline__ void one_regressor(LearnArgs& l, const EnsembleSearchArgs& a, const int i)
{
    l.B = 0; l.n_gp = 1;
    l.min_count = a.min_count;
    l.gp[0] = a.gp[i];
    l.samples = nullptr; l.dropped = nullptr;
    l.bins = const_cast<double*>(a.bins) + (long)i * NPT * ACC;       // the bodies used here read them only
    l.out = a.out + i;
    l.info = a.info + i;
}

}  // namespace

__global__ __launch_bounds__(WAVE) void admpc_quad_ensemble_search_init_kernel(const EnsembleSearchArgs a)
{
    const int i = flat_index((int)blockIdx.x, a.n_gp);
    const SearchGp S = a.sd->s[i];
    gp_search_init_body(S, a.hyper + (long)i * HYP);
}

__global__ __launch_bounds__(NLL_WAVES * WAVE) void admpc_quad_ensemble_nll_kernel(const EnsembleSearchArgs a)
{
    const int i = flat_index((int)blockIdx.y, a.n_gp);
    const SearchGp S = a.sd->s[i];
    LearnArgs l;
    one_regressor(l, a, i);
    gp_nll_body(l, 0, S, a.sd->grid, a.sd->half, a.hyper + (long)i * HYP, a.nll + (long)i * ADMPC_GP_SEARCH_MAX);
}

__global__ __launch_bounds__(WAVE) void admpc_quad_ensemble_pick_kernel(const EnsembleSearchArgs a)
{
    const int i = flat_index((int)blockIdx.x, a.n_gp);
    const SearchGp S = a.sd->s[i];
    gp_pick_body(S, a.sd->grid, a.sd->half, a.sd->shrink, a.hyper + (long)i * HYP, a.nll + (long)i * ADMPC_GP_SEARCH_MAX, a.search_info + 2 * i);
}

__global__ __launch_bounds__(WAVE) void admpc_quad_ensemble_refit_kernel(const EnsembleSearchArgs a)
{
    const int i = flat_index((int)blockIdx.x, a.n_gp);
    LearnArgs l;
    one_regressor(l, a, i);
    gp_refit_body(l, 0, a.hyper + (long)i * HYP);
}

namespace {

// the first refusals of the three ensemble entries, and the view of a checked ensemble
int ensemble_check(const char* who, const AdmpcQuadEnsemble* e, QuadEnsembleView& v)
{
    if (!e) return admpc_refuse(who, "null ensemble");
    admpc_quad_ensemble_view(e, &v);
    if (!v.learns) return admpc_refuse(who, "the ensemble was created without observe parameters");
    return ADMPC_OK;
}

}  // namespace

extern "C" {

int admpc_quad_gp_search(int device, const AdmpcQuadObserveParams* obs, const AdmpcGpSearchParams* sp, int min_count, int resume,
                         const double* bins, double* hyper, double* nll, int32_t* search_info, void* stream)
{
    const int rc = admpc_quad_observe_params_check("admpc_quad_gp_search", obs);
    return rc ? rc : admpc_hyper_search("admpc_quad_gp_search", device, obs->n_gp, obs->gp, QUAD_LEARN.feat_lo, sp, min_count, resume, bins, hyper,
                                        nll, search_info, stream);
}

int admpc_quad_gp_refit(int device, const AdmpcQuadObserveParams* obs, int min_count, const double* bins, const double* hyper,
                        AdmpcGp* gp_out, int32_t* info, void* stream)
{
    const int rc = admpc_quad_observe_params_check("admpc_quad_gp_refit", obs);
    return rc ? rc : admpc_hyper_refit("admpc_quad_gp_refit", device, obs->n_gp, obs->gp, QUAD_LEARN.feat_lo, min_count, bins, hyper, gp_out, info,
                                       stream);
}

int admpc_quad_ensemble_set_search(AdmpcQuadEnsemble* e, const AdmpcGpSearchParams* sp)
{
    const char* who = "admpc_quad_ensemble_set_search";
    QuadEnsembleView v;
    int rc = ensemble_check(who, e, v);
    if (rc) return rc;
    if (!sp) return admpc_refuse(who, "the search parameters are not set");
    EnsembleSearchDev host = EnsembleSearchDev();
    int cmax = 1;
    for (int c = 0; c < v.K; ++c) {
        int cm = 1;
        rc = admpc_hyper_form(who, v.n_gp, v.obs[c].gp, sp + c, host.s + c * GMAX, &cm);
        if (rc) return rc;
        if (cm > cmax) cmax = cm;
    }
    for (int c = 1; c < v.K; ++c)
        if (sp[c].grid != sp[0].grid || sp[c].rounds != sp[0].rounds || sp[c].shrink != sp[0].shrink)
            return admpc_refuse(who, "the search parameters of the clusters must share grid, rounds and shrink (the boxes are free per cluster)");
    host.grid = sp[0].grid; host.half = (sp[0].grid - 1) / 2; host.shrink = sp[0].shrink;
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    QuadEnsembleSearch* q = v.search;
    if (!q->d_desc && hipMalloc(&q->d_desc, sizeof(EnsembleSearchDev)) != hipSuccess) {
        q->d_desc = nullptr;
        return admpc_set_error(ADMPC_EHIP, "admpc_quad_ensemble_set_search: device allocation failed");
    }
    // a search in flight on any stream reads the descriptors: wait for it, then write them
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(q->d_desc, &host, sizeof host, hipMemcpyHostToDevice) != hipSuccess)
        return admpc_set_error(ADMPC_EHIP, "admpc_quad_ensemble_set_search: device copy failed");
    q->set = 1; q->grid = host.grid; q->rounds = sp[0].rounds; q->cmax = cmax; q->shrink = host.shrink;
    return ADMPC_OK;
}

int admpc_quad_ensemble_search(const AdmpcQuadEnsemble* e, int min_count, int resume, const double* bins, double* hyper, double* nll,
                               int32_t* search_info, void* stream)
{
    const char* who = "admpc_quad_ensemble_search";
    QuadEnsembleView v;
    const int rc = ensemble_check(who, e, v);
    if (rc) return rc;
    if (!v.search->set) return admpc_refuse(who, "no search parameters yet: call admpc_quad_ensemble_set_search first");
    if (min_count < 1) return admpc_refuse(who, "min_count must be at least 1");
    if (resume != 0 && resume != 1) return admpc_refuse(who, "resume must be 0 or 1");
    if (!bins || !hyper || !nll || !search_info) return admpc_refuse(who, "null array argument");
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    EnsembleSearchArgs a = EnsembleSearchArgs();
    a.n_gp = v.n_gp; a.min_count = (double)min_count; a.gp = v.gp; a.sd = (const EnsembleSearchDev*)v.search->d_desc;
    a.bins = bins; a.hyper = hyper; a.nll = nll; a.search_info = search_info;
    const unsigned regs = (unsigned)(v.K * v.n_gp);
    const dim3 one(regs), cand((unsigned)((v.search->cmax + NLL_CAND - 1) / NLL_CAND), regs);
    if (!resume) {
        hipLaunchKernelGGL(admpc_quad_ensemble_search_init_kernel, one, dim3(WAVE), 0, (hipStream_t)stream, a);
        if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_ensemble_search_init_kernel: launch failed");
    }
    for (int it = 0; it < v.search->rounds; ++it) {
        hipLaunchKernelGGL(admpc_quad_ensemble_nll_kernel, cand, dim3(NLL_WAVES * WAVE), 0, (hipStream_t)stream, a);
        if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_ensemble_nll_kernel: launch failed");
        hipLaunchKernelGGL(admpc_quad_ensemble_pick_kernel, one, dim3(WAVE), 0, (hipStream_t)stream, a);
        if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_ensemble_pick_kernel: launch failed");
    }
    return ADMPC_OK;
}

int admpc_quad_ensemble_refit(const AdmpcQuadEnsemble* e, int min_count, const double* bins, const double* hyper, AdmpcGp* gp_out,
                              int32_t* info, void* stream)
{
    const char* who = "admpc_quad_ensemble_refit";
    QuadEnsembleView v;
    const int rc = ensemble_check(who, e, v);
    if (rc) return rc;
    if (min_count < 1) return admpc_refuse(who, "min_count must be at least 1");
    if (!bins || !hyper || !gp_out || !info) return admpc_refuse(who, "null array argument");
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    EnsembleSearchArgs a = EnsembleSearchArgs();
    a.n_gp = v.n_gp; a.min_count = (double)min_count; a.gp = v.gp;
    a.bins = bins; a.hyper = const_cast<double*>(hyper); a.out = gp_out; a.info = info;
    hipLaunchKernelGGL(admpc_quad_ensemble_refit_kernel, dim3((unsigned)(v.K * v.n_gp)), dim3(WAVE), 0, (hipStream_t)stream, a);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_ensemble_refit_kernel: launch failed");
    return ADMPC_OK;
}

}  // extern "C"
