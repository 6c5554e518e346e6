// admpc_quad_ensemble.hip -- a clustered GP ensemble in the quadrotor's closed loop (include/admpc_quad_ensemble.h): the object that holds
// one handle per cluster, and two kernels.
//
//   route  admpc_quad_ensemble_route_kernel  the cluster of every vehicle from row 0 of its reference window: the body of
//                                            admpc_quad_select_cluster_kernel (quad_route_dev.h) read through the window's row stride,
//                                            one thread per vehicle
//   bin    admpc_quad_ensemble_bin_kernel    one wave per (cluster, regressor, bin), all clusters in one launch: the body of the bin kernels
//                                            (gp_fit_dev.h) with a predicate that takes the records of the wave's cluster, under that
//                                            cluster's box, which the wave reads from the object's device copy
//
// The period of the routed rollout (window -> route -> routed solve -> plant) is admpc_quad_fleet.hip's, the observed run
// admpc_quad_learn.hip's: their argument block carries the ensemble, and they call the two launches below.  The observe kernel, the fit and
// the install are those units' own, per cluster.  The search of the hyperparameters of all clusters is admpc_quad_hyper.hip's, which
// reaches the object through admpc_quad_ensemble_view and keeps its search descriptors in the object's `search` slot.
#include <math.h>
#include <new>
#include "admpc_host.h"
#include "../../include/admpc_quad_ensemble.h"

#define NX ADMPC_NX           // model_dev.h (exp_nonpos, which the fit body of gp_fit_dev.h names) wants the car's dimensions defined
#define NU ADMPC_NU
#define NY ADMPC_NY
#include "gp_fit_dev.h"       // WAVE, NPT, ACC; LearnGp, LearnArgs, QUAD_LEARN; gp_bin_body; admpc_learn_*
#define QREC 14               // doubles per sample record, as admpc_quad_learn.hip lays it out
#define KMAX ADMPC_QUAD_CLUSTERS_MAX
#define GMAX ADMPC_QUAD_GP_MAX

struct AdmpcQuadEnsemble {
    int device, K, N, n_feat, feat[3];
    int learns, n_gp;                         // created with observe parameters; their common n_gp
    AdmpcQuadSolver* solvers[KMAX];
    AdmpcQuadObserveParams obs[KMAX];         // the host copies (learns)
    void* d_mem;                              // the one allocation: centroids [K][n_feat], then LearnGp [K][GMAX]
    double* d_cent;                           // written by admpc_quad_clusters.hip's install and set kernels
    const LearnGp* d_gp;
    QuadEnsembleSearch search;                // admpc_quad_hyper.hip's: the search descriptors of admpc_quad_ensemble_set_search
};

// what one launch of the bin kernel works on (passed by value; the regressors and the centroids by pointer into the object's device copy)
struct EnsembleBinArgs {
    int B, K, n_gp, n_feat, feat[3];
    const double* cent;                       // [K][n_feat]
    const LearnGp* gp;                        // [K][GMAX]
    const double* samples;                    // [B][QREC]
    double* bins;                             // [K][GMAX][NPT][ACC]
    int32_t* dropped;                         // [K][GMAX + 1]
};

namespace {

#include "model_dev.h"

constexpr int QX = ADMPC_QUAD_NX, QU = ADMPC_QUAD_NU, QY = ADMPC_QUAD_NY;
typedef AdmpcQuadConfig Cfg;

#include "quad_model_dev.h"
#include "quad_route_dev.h"

// gp_bin_body's predicate: the records whose own features lie nearest to centroid c; regressor 0 of cluster 0 tallies the records that
// are not valid
struct TakesCluster {
    int c, g, K, d, f[3];
    const double* cent;
    __device__ __forceinline__ bool operator()(const double* __restrict__ r) const
    {
        double z[3] = { 0, 0, 0 };
        for (int j = 0; j < d; ++j) z[j] = r[f[j] - QUAD_LEARN.feat_lo];
        return quad_nearest(z, d, K, cent) == c;
    }
    __device__ __forceinline__ bool tallies_invalid() const { return c == 0 && g == 0; }
};

}  // namespace

__global__ void admpc_quad_ensemble_route_kernel(int B, int d, int f0, int f1, int f2, const double* __restrict__ yref, long long stride, int K,
                                                 const double* __restrict__ cent, int32_t* __restrict__ route, int32_t* __restrict__ route_out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* row = yref + (size_t)b * stride;
    const int r = quad_route_row(row, row + QX, d, f0, f1, f2, K, cent);
    route[b] = r;
    if (route_out) route_out[b] = r;
}

// grid K * n_gp * NPT: block (c, g, bin)
__global__ __launch_bounds__(WAVE) void admpc_quad_ensemble_bin_kernel(const EnsembleBinArgs a)
{
    const int blk = (int)blockIdx.x, c = blk / (a.n_gp * NPT), g = (blk / NPT) % a.n_gp, bin = blk % NPT;
    // the body sees ONE regressor, at a constant index (a variable one would put the block into scratch): its bins and its dropped count
    // are at the front of what it is given, and the count of the invalid records, GMAX entries on, is touched by regressor 0 alone
    LearnArgs l;
    l.B = a.B; l.n_gp = 1;
    l.gp[0] = a.gp[c * GMAX + g];
    l.samples = a.samples;
    l.bins = a.bins + (long)(c * GMAX + g) * NPT * ACC;
    l.dropped = a.dropped + c * (GMAX + 1) + g;
    const TakesCluster takes = { c, g, a.K, a.n_feat, { a.feat[0], a.feat[1], a.feat[2] }, a.cent };
    gp_bin_body<QREC, 7, 10, GMAX>(l, 0, bin, takes);
}

namespace {

bool same_structure(const AdmpcQuadObserveParams& a, const AdmpcQuadObserveParams& b)
{
    if (a.dt != b.dt || a.substeps != b.substeps || a.n_gp != b.n_gp) return false;
    for (int g = 0; g < a.n_gp; ++g) {
        if (a.gp[g].n_feat != b.gp[g].n_feat || a.gp[g].out != b.gp[g].out) return false;
        for (int d = 0; d < a.gp[g].n_feat; ++d) if (a.gp[g].feat[d] != b.gp[g].feat[d]) return false;
    }
    return true;
}

}  // namespace

// for admpc_quad_fleet.hip's period: the handles of an ensemble (returns K)
extern "C" int admpc_quad_ensemble_handles(const AdmpcQuadEnsemble* e, AdmpcQuadSolver* const** solvers)
{
    *solvers = e->solvers;
    return e->K;
}

// for admpc_quad_clusters.hip and admpc_quad_hyper.hip: the device centroids, the features, the blocks, the device regressors and the
// search slot of an ensemble (the slot is the object's own state, which a set_search writes whoever holds the object)
extern "C" void admpc_quad_ensemble_view(const AdmpcQuadEnsemble* e, QuadEnsembleView* v)
{
    v->device = e->device; v->K = e->K; v->n_feat = e->n_feat; v->learns = e->learns; v->n_gp = e->n_gp;
    for (int j = 0; j < 3; ++j) v->feat[j] = e->feat[j];
    v->cent = e->d_cent; v->obs = e->obs; v->gp = e->d_gp;
    v->search = const_cast<QuadEnsembleSearch*>(&e->search);
}

// one launch of the route kernel for a checked ensemble, B > 0, on its device (the caller holds it); route_out: null or [B]
extern "C" int admpc_quad_ensemble_route_launch(const AdmpcQuadEnsemble* e, int B, const double* yref, int32_t* route, int32_t* route_out, void* stream)
{
    hipLaunchKernelGGL(admpc_quad_ensemble_route_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, e->n_feat, e->feat[0], e->feat[1],
                       e->feat[2], yref, (long long)e->N * QY, e->K, e->d_cent, route, route_out);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_ensemble_route_kernel: launch failed");
    return ADMPC_OK;
}

// one launch of the bin kernel for an ensemble that learns, B > 0, on its device (the caller holds it)
extern "C" int admpc_quad_ensemble_bin_launch(const AdmpcQuadEnsemble* e, int B, const double* samples, double* bins, int32_t* dropped, void* stream)
{
    EnsembleBinArgs a;
    a.B = B; a.K = e->K; a.n_gp = e->n_gp; a.n_feat = e->n_feat;
    for (int j = 0; j < 3; ++j) a.feat[j] = e->feat[j];
    a.cent = e->d_cent; a.gp = e->d_gp; a.samples = samples; a.bins = bins; a.dropped = dropped;
    hipLaunchKernelGGL(admpc_quad_ensemble_bin_kernel, dim3((unsigned)(e->K * e->n_gp * NPT)), dim3(WAVE), 0, (hipStream_t)stream, a);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_ensemble_bin_kernel: launch failed");
    return ADMPC_OK;
}

extern "C" {

int admpc_quad_ensemble_create(AdmpcQuadSolver* const* solvers, int K, int n_feat, const int32_t* feats, const double* centroids,
                               const AdmpcQuadObserveParams* obs, AdmpcQuadEnsemble** out)
{
    const char* who = "admpc_quad_ensemble_create";
    if (!solvers || !feats || !centroids || !out) return admpc_refuse(who, "null argument");
    if (K < 1 || K > KMAX) return admpc_refuse(who, "K must be in [1, 8]");
    for (int c = 0; c < K; ++c) if (!solvers[c]) return admpc_refuse(who, "null solver");
    int device = 0, N = 0;
    (void)admpc_quad_solver_info(solvers[0], &device, &N, nullptr);
    for (int c = 1; c < K; ++c) {
        int dv = 0, n = 0;
        (void)admpc_quad_solver_info(solvers[c], &dv, &n, nullptr);
        if (dv != device || n != N) return admpc_refuse(who, "the cluster solvers must share device and horizon");
    }
    for (int c = 0; c < K; ++c) {
        int sqp = 0;
        (void)admpc_quad_solver_info(solvers[c], nullptr, nullptr, &sqp);
        if (sqp > 1) return admpc_refuse(who, "a solver in SQP mode (sqp_iters > 1) is not served: the rollout is the RTI loop");
    }
    if (n_feat < 1 || n_feat > ADMPC_GP_MAX_FEAT) return admpc_refuse(who, "n_feat must be in [1, 3]");
    for (int j = 0; j < n_feat; ++j) if (feats[j] < 0 || feats[j] >= QY) return admpc_refuse(who, "feature index outside z = [x; u]");
    for (int i = 0; i < K * n_feat; ++i) if (!isfinite(centroids[i])) return admpc_refuse(who, "a centroid is not finite");
    if (obs) {
        for (int c = 0; c < K; ++c) {
            const int rc = admpc_quad_observe_params_check(who, obs + c);
            if (rc) return rc;
        }
        for (int c = 1; c < K; ++c)
            if (!same_structure(obs[0], obs[c])) return admpc_refuse(who, "the observe parameters of the clusters must share dt, substeps, n_gp and every regressor's n_feat, feat and out");
        for (int j = 0; j < n_feat; ++j)
            if (feats[j] < QUAD_LEARN.feat_lo) return admpc_refuse(who, "an ensemble that learns clusters on features in [7, 16]: the sample record holds no others");
        for (int c = 0; c < K; ++c) {
            int have = 0;
            (void)admpc_quad_solver_config_device(solvers[c], &have);
            if (have != obs[0].n_gp) return admpc_refuse(who, "a handle's n_gp is not the observe parameters' n_gp (create it with placeholder GPs of n_points = 0)");
        }
    }
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    AdmpcQuadEnsemble* e = new (std::nothrow) AdmpcQuadEnsemble();
    if (!e) return admpc_set_error(ADMPC_ENOMEM, "out of host memory");
    e->device = device; e->K = K; e->N = N; e->n_feat = n_feat;
    for (int j = 0; j < 3; ++j) e->feat[j] = j < n_feat ? feats[j] : 0;
    e->learns = obs ? 1 : 0; e->n_gp = obs ? obs[0].n_gp : 0;
    LearnGp host_gp[KMAX * GMAX];
    for (int i = 0; i < KMAX * GMAX; ++i) host_gp[i] = LearnGp();
    for (int c = 0; c < K; ++c) {
        e->solvers[c] = solvers[c];
        if (!obs) continue;
        e->obs[c] = obs[c];
        LearnArgs l = LearnArgs();
        admpc_learn_fill(l, obs[c].n_gp, obs[c].gp, QUAD_LEARN.feat_lo);
        for (int g = 0; g < GMAX; ++g) host_gp[c * GMAX + g] = l.gp[g];
    }
    const size_t nc = (size_t)K * n_feat * sizeof(double), ng = (size_t)K * GMAX * sizeof(LearnGp);
    e->d_mem = nullptr;
    if (hipMalloc(&e->d_mem, nc + ng) != hipSuccess || hipMemcpy(e->d_mem, centroids, nc, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((char*)e->d_mem + nc, host_gp, ng, hipMemcpyHostToDevice) != hipSuccess) {
        if (e->d_mem) (void)hipFree(e->d_mem);
        delete e;
        return admpc_set_error(ADMPC_EHIP, "admpc_quad_ensemble_create: device allocation or copy failed");
    }
    e->d_cent = (double*)e->d_mem; e->d_gp = (const LearnGp*)((char*)e->d_mem + nc);
    *out = e;
    return ADMPC_OK;
}

void admpc_quad_ensemble_destroy(AdmpcQuadEnsemble* e)
{
    if (!e) return;
    DeviceGuard guard(e->device);
    if (e->d_mem) (void)hipFree(e->d_mem);
    if (e->search.d_desc) (void)hipFree(e->search.d_desc);
    delete e;
}

int admpc_quad_ensemble_route_batch(const AdmpcQuadEnsemble* e, int B, const double* yref, int32_t* route, void* stream)
{
    const char* who = "admpc_quad_ensemble_route_batch";
    if (!e) return admpc_refuse(who, "null ensemble");
    if (B < 0) return admpc_refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!yref || !route) return admpc_refuse(who, "null array argument");
    DeviceGuard guard(e->device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    return admpc_quad_ensemble_route_launch(e, B, yref, route, nullptr, stream);
}

int admpc_quad_ensemble_observe_batch(const AdmpcQuadEnsemble* e, const AdmpcQuadSolver* model, const AdmpcQuadPlantParams* plant, int B,
                                      const double* u, int64_t u_stride, const double* x, double* prev, double* samples, double* bins,
                                      int32_t* dropped, void* stream)
{
    const char* who = "admpc_quad_ensemble_observe_batch";
    if (!e) return admpc_refuse(who, "null ensemble");
    if (!e->learns) return admpc_refuse(who, "the ensemble was created without observe parameters");
    const int rc = admpc_quad_plant_params_check(who, plant);
    if (rc) return rc;
    if (!model) return admpc_refuse(who, "null model");
    if (B < 0) return admpc_refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!u || !x || !prev || !samples || !bins || !dropped) return admpc_refuse(who, "null array argument");
    if (u_stride < QU) return admpc_refuse(who, "u_stride must be at least 4");
    DeviceGuard guard(e->device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    return admpc_quad_observe_launch(model, plant, &e->obs[0], e, B, u, (long long)u_stride, x, prev, nullptr, samples, bins, dropped, stream);
}

int admpc_quad_ensemble_fit(const AdmpcQuadEnsemble* e, int min_count, const double* bins, AdmpcGp* gp_out, int32_t* info, void* stream)
{
    const char* who = "admpc_quad_ensemble_fit";
    if (!e) return admpc_refuse(who, "null ensemble");
    if (!e->learns) return admpc_refuse(who, "the ensemble was created without observe parameters");
    if (min_count < 1) return admpc_refuse(who, "min_count must be at least 1");
    if (!bins || !gp_out || !info) return admpc_refuse(who, "null array argument");
    for (int c = 0; c < e->K; ++c) {
        const int rc = admpc_learn_fit(who, e->device, e->n_gp, e->obs[c].gp, QUAD_LEARN.feat_lo, min_count, bins + (size_t)c * GMAX * NPT * ACC,
                                       gp_out + (size_t)c * GMAX, info + (size_t)c * GMAX, stream);
        if (rc) return rc;
    }
    return ADMPC_OK;
}

int admpc_quad_ensemble_install(AdmpcQuadEnsemble* e, const AdmpcGp* gp_dev, int32_t* installed, void* stream)
{
    const char* who = "admpc_quad_ensemble_install";
    if (!e) return admpc_refuse(who, "null ensemble");
    int have[KMAX];
    for (int c = 0; c < e->K; ++c) {
        (void)admpc_quad_solver_config_device(e->solvers[c], &have[c]);
        if (have[c] < 1) return admpc_refuse(who, "a handle was created without GPs (create it with placeholder GPs of n_points = 0)");
    }
    if (!gp_dev || !installed) return admpc_refuse(who, "null array argument");
    for (int c = 0; c < e->K; ++c) {
        const int rc = admpc_quad_gp_install(e->solvers[c], have[c], gp_dev + (size_t)c * GMAX, installed + (size_t)c * GMAX, stream);
        if (rc) return rc;
    }
    return ADMPC_OK;
}

int admpc_quad_ensemble_rollout_batch(AdmpcQuadEnsemble* e, const AdmpcQuadTrajBank* bank, const AdmpcQuadPlantParams* plant, int over,
                                      int B, int T, const int32_t* traj_of, int32_t* idx, double* x, double* xbar, double* ubar,
                                      double* yref, double* yref_e, double* cost, int32_t* status, int32_t* iters,
                                      double* tally, int32_t* counts, double* traj_out, double* u_out,
                                      int32_t* route, int32_t* route_out,
                                      const AdmpcQuadSolver* model, double* prev, double* samples, double* bins, int32_t* dropped,
                                      const AdmpcQuadNoiseParams* noise, uint64_t* noise_step, void* stream)
{
    const char* who = "admpc_quad_ensemble_rollout_batch";
    if (!e) return admpc_refuse(who, "null ensemble");
    if (model && !e->learns) return admpc_refuse(who, "the ensemble was created without observe parameters");
    if (noise) {
        int rc = admpc_quad_plant_params_check("admpc_quad_rollout_noise_batch", plant);
        if (!rc) rc = admpc_quad_noise_params_check("admpc_quad_rollout_noise_batch", noise, plant);
        if (rc) return rc;
    }
    // the chain of the plain, observed and noisy rollouts: handle 0 stands for the device, the horizon and the RTI mode of all
    const QuadRolloutArgs a = { e->solvers[0], bank, plant, over, B, traj_of, idx, x, xbar, ubar, yref, yref_e, cost, status, iters, tally, counts,
                                noise, noise ? noise_step : nullptr, e, route, route_out };
    return model ? admpc_quad_rollout_observe_run(a, T, traj_out, u_out, model, &e->obs[0], prev, samples, 0, bins, dropped, stream)
                 : admpc_quad_rollout_run(a, T, traj_out, u_out, stream);
}

}  // extern "C"
