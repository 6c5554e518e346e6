// admpc_quad_learn.hip -- fitting a quadrotor handle's body-frame residual GPs on the device from the steps a fleet has flown
// (include/admpc_quad_learn.h):
//
//   observe  admpc_quad_observe_kernel     the model's own prediction of the period that has just passed, from the latched state and the
//                                          activations the plant applied; what the plant did beyond it to the body-frame velocity, per
//                                          second, is the sample.  One lane per vehicle, as the plant kernel (admpc_quad_plant.hip); the
//                                          model is quad_f_tan of quad_model_dev.h, the text the solve kernels integrate, called with zero
//                                          tangents: the doubled arithmetic is nothing next to a solve.  <VAR>: the period is the
//                                          vehicle's own, the sub-steps it flew towards its target (include/admpc_quad_targets.h)
//   bin      admpc_quad_bin_kernel         one wave per (regressor, bin): the body of the car's bin kernel (gp_fit_dev.h) on this record
//   fit      admpc_gp_fit_kernel           the car's kernel, launched by admpc_learn.hip (admpc_learn_fit): it reads nothing of a vehicle
//   install  admpc_quad_gp_install_kernel  one wave: checks each record and copies it into the handle's device configuration; the body
//                                          of the car's (gp_fit_dev.h) with the quadrotor's ranges
//
// To this unit's fit the hyperparameters are given (admpc_quad_learn.h: what is not offered); admpc_quad_hyper.hip searches them.  The refusals of the regressors, their form for the kernels
// and the fit entry are admpc_learn.hip's (declared in gp_fit_dev.h).  The rollout with observation is at the end of the file.
#include <stdio.h>
#include <math.h>
#include "admpc_host.h"

#define NX ADMPC_NX           // model_dev.h (exp_nonpos, which the fit body of gp_fit_dev.h names) wants the car's dimensions defined
#define NU ADMPC_NU
#define NY ADMPC_NY
#include "gp_fit_dev.h"       // WAVE, NPT, ACC; LearnGp, LearnArgs, LearnRanges; the bodies of the bin and install kernels; admpc_learn_*
#define QREC 14               // doubles per sample record: v_b (3), body rates (3), activations (4), y (3), the flag
#define QO_GRID 4096          // blocks of the observe kernel at most, as the plant kernel's; more vehicles go round the stride loop

static_assert(sizeof(AdmpcQuadObserveParams) == 16 + ADMPC_QUAD_GP_MAX * sizeof(AdmpcGpBins) && sizeof(AdmpcGpBins) == 128, "the layout the Python side mirrors");

// what one launch of the observe kernel works on (passed by value); h = dt / M is formed on the host, as it always was
struct QuadObserveArgs {
    double h, dt, plant_dt, u_min, u_max;
    int M, B, plant_substeps;
    const double* u; long long u_stride;      // row b at u + b * u_stride
    const double* x;                          // [B][13] the states now
    double* prev;                             // [B][13] the states one period ago, in/out
    const int32_t* nsub;                      // [B] the sub-steps a vehicle flew (VAR), or null
    double* samples;                          // [B][QREC]
};

namespace {

#include "model_dev.h"

constexpr int QX = ADMPC_QUAD_NX, QU = ADMPC_QUAD_NU;
typedef AdmpcQuadConfig Cfg;

#include "quad_model_dev.h"
#include "quad_observe_dev.h"  // quad_rk4_state, body_velocity

}  // namespace

__global__ void admpc_quad_latch_kernel(long long n, const double* __restrict__ x, double* __restrict__ prev)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) prev[i] = x[i];
}

// VAR: vehicle b flew nsub[b] sub-steps of the plant; a full period is dt itself, so that it is observed as without VAR, bit for bit
template <bool VAR>
__global__ __launch_bounds__(WAVE) void admpc_quad_observe_kernel(const AdmpcQuadConfig* __restrict__ cfg, const QuadObserveArgs a)
{
    for (long long b = (long long)blockIdx.x * WAVE + threadIdx.x; b < a.B; b += (long long)gridDim.x * WAVE) {
        double xh[QX], now[QX], act[QU];
        double* pb = a.prev + b * QX;
        const double* xb = a.x + b * QX;
        const double* ub = a.u + b * a.u_stride;
        int ns = 1;
        double dt = a.dt, h = a.h;
        if (VAR) {
            ns = a.nsub[b];
            dt = ns == a.plant_substeps ? a.dt : (double)ns * a.plant_dt;                     // the period this vehicle flew
            h = dt / (double)a.M;
        }
#pragma unroll
        for (int i = 0; i < QX; ++i) { xh[i] = pb[i]; now[i] = xb[i]; }
#pragma unroll
        for (int m = 0; m < QU; ++m) {
            const double raw = ub[m];
            double v = raw < a.u_max ? raw : a.u_max;            // max(min(u, u_max), u_min), as the plant kernel
            v = v > a.u_min ? v : a.u_min;
            if (!isfinite(raw)) v = a.u_min;
            act[m] = v;
        }
        double* r = a.samples + b * QREC;
        double vp[3], vn[3], vh[3];
        body_velocity(xh, vp);
        bool fin = ns >= 1;
#pragma unroll
        for (int i = 0; i < 3; ++i) { r[i] = vp[i]; r[3 + i] = xh[10 + i]; fin = fin && isfinite(vp[i]) && isfinite(xh[10 + i]); }
#pragma unroll
        for (int m = 0; m < QU; ++m) { r[6 + m] = act[m]; fin = fin && isfinite(act[m]); }
        for (int m = 0; m < a.M; ++m) quad_rk4_state(cfg, xh, act, h);
        body_velocity(now, vn);
        body_velocity(xh, vh);
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double y = (vn[j] - vh[j]) / dt;
                r[10 + j] = y;
                fin = fin && isfinite(y);
            }
        }
        r[13] = fin ? 1.0 : 0.0;
#pragma unroll
        for (int i = 0; i < QX; ++i) pb[i] = now[i];
    }
}

// grid n_gp * NPT: block (g, bin)
__global__ __launch_bounds__(WAVE) void admpc_quad_bin_kernel(const LearnArgs a)
{
    gp_bin_body<QREC, 7, 10, ADMPC_QUAD_GP_MAX>(a, (int)blockIdx.x / NPT, (int)blockIdx.x % NPT);
}

// one wave.  src [n_gp] -> cfg->gp[0 .. n_gp); a record that fails the check is replaced by the empty GP (gp_fit_dev.h has the body).
__global__ __launch_bounds__(WAVE) void admpc_quad_gp_install_kernel(AdmpcQuadConfig* cfg, int n_gp, const AdmpcGp* src, int32_t* installed)
{
    gp_install_body<QUAD_LEARN.feat_lo, QUAD_LEARN.feat_hi, QUAD_LEARN.out_lo, QUAD_LEARN.out_hi>(cfg->gp, n_gp, src, installed);
}

// hidden (admpc_host.h), for admpc_quad_ensemble.hip and admpc_quad_targets.hip too
extern "C" {

// The refusals of the observe parameters, for the entry points that take them (`who` leads the message): the quadrotor's head, which
// has no speed band, in front of the regressors' refusals of admpc_learn.hip.
int admpc_quad_observe_params_check(const char* who, const AdmpcQuadObserveParams* obs)
{
    if (!obs) return admpc_learn_refuse(who, "the observe parameters are not set");
    if (!(obs->dt > 0) || !isfinite(obs->dt)) return admpc_learn_refuse(who, "dt must be positive and finite");
    if (obs->substeps < 1 || obs->substeps > 64) return admpc_learn_refuse(who, "substeps must be in [1, 64]");
    return admpc_learn_regressors_check(who, obs->n_gp, obs->gp, QUAD_LEARN);
}

// the bin launch of an observation alone, for checked arguments, B > 0, on the current device
int admpc_quad_bin_launch(const AdmpcQuadObserveParams* obs, int B, const double* samples, double* bins, int32_t* dropped, void* stream)
{
    LearnArgs l = LearnArgs();
    admpc_learn_fill(l, obs->n_gp, obs->gp, QUAD_LEARN.feat_lo);
    l.B = B; l.samples = samples; l.bins = bins; l.dropped = dropped;
    hipLaunchKernelGGL(admpc_quad_bin_kernel, dim3((unsigned)(obs->n_gp * NPT)), dim3(WAVE), 0, (hipStream_t)stream, l);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_bin_kernel: launch failed");
    return ADMPC_OK;
}

// the latch, likewise
int admpc_quad_latch_launch(int B, const double* x, double* prev, void* stream)
{
    const long long n = (long long)B * QX, nblk = (n + 255) / 256;
    hipLaunchKernelGGL(admpc_quad_latch_kernel, dim3((unsigned)(nblk < 4096 ? nblk : 4096)), dim3(256), 0, (hipStream_t)stream, n, x, prev);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_latch_kernel: launch failed");
    return ADMPC_OK;
}

// The two launches of an observation for checked arguments, B > 0, on the model's device (the caller holds it).  nsub: null, or the
// sub-steps every vehicle flew.  With ens the records go to the bins of their clusters: the ensemble's bin launch
// (admpc_quad_ensemble.hip), all clusters at once, under its own boxes.
int admpc_quad_observe_launch(const AdmpcQuadSolver* model, const AdmpcQuadPlantParams* plant, const AdmpcQuadObserveParams* obs,
                              const AdmpcQuadEnsemble* ens, int B, const double* u, long long u_stride, const double* x, double* prev,
                              const int32_t* nsub, double* samples, double* bins, int32_t* dropped, void* stream)
{
    QuadObserveArgs a;
    a.h = obs->dt / obs->substeps; a.dt = obs->dt; a.plant_dt = plant->dt; a.u_min = plant->u_min; a.u_max = plant->u_max;
    a.M = obs->substeps; a.B = B; a.plant_substeps = plant->substeps;
    a.u = u; a.u_stride = u_stride; a.x = x; a.prev = prev; a.nsub = nsub; a.samples = samples;
    const int nblk = (B + WAVE - 1) / WAVE;
    hipLaunchKernelGGL(nsub ? admpc_quad_observe_kernel<true> : admpc_quad_observe_kernel<false>, dim3((unsigned)(nblk < QO_GRID ? nblk : QO_GRID)),
                       dim3(WAVE), 0, (hipStream_t)stream, admpc_quad_solver_config_device(model, nullptr), a);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_observe_kernel: launch failed");
    if (ens) return admpc_quad_ensemble_bin_launch(ens, B, samples, bins, dropped, stream);
    return admpc_quad_bin_launch(obs, B, samples, bins, dropped, stream);
}

}  // extern "C"

namespace {

// admpc_quad_observe_batch and, with var, admpc_quad_observe_var_batch behind their names: the same refusals in the same order, nsub
// among the arrays where it is read
int quad_observe_entry(const char* who, bool var, const AdmpcQuadSolver* model, const AdmpcQuadPlantParams* plant, const AdmpcQuadObserveParams* obs,
                       int B, const double* u, int64_t u_stride, const double* x, double* prev, const int32_t* nsub, double* samples, double* bins,
                       int32_t* dropped, void* stream)
{
    int rc = admpc_quad_observe_params_check(who, obs);
    if (rc) return rc;
    rc = admpc_quad_plant_params_check(who, plant);
    if (rc) return rc;
    if (!model) return admpc_refuse(who, "null model");
    if (B < 0) return admpc_refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!u || !x || !prev || (var && !nsub) || !samples || !bins || !dropped) return admpc_refuse(who, "null array argument");
    if (u_stride < QU) return admpc_refuse(who, "u_stride must be at least 4");
    int device = 0;
    (void)admpc_quad_solver_info(model, &device, nullptr, nullptr);
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    return admpc_quad_observe_launch(model, plant, obs, nullptr, B, u, (long long)u_stride, x, prev, var ? nsub : nullptr, samples, bins, dropped, stream);
}

}  // namespace

extern "C" {

int admpc_quad_observe_latch_batch(int device, int B, const double* x, double* prev, void* stream)
{
    if (B < 0) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_observe_latch_batch: negative batch");
    if (B == 0) return ADMPC_OK;
    if (!x || !prev) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_observe_latch_batch: null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    return admpc_quad_latch_launch(B, x, prev, stream);
}

int admpc_quad_observe_batch(const AdmpcQuadSolver* model, const AdmpcQuadPlantParams* plant, const AdmpcQuadObserveParams* obs, int B,
                             const double* u, int64_t u_stride, const double* x, double* prev, double* samples, double* bins,
                             int32_t* dropped, void* stream)
{
    return quad_observe_entry("admpc_quad_observe_batch", false, model, plant, obs, B, u, u_stride, x, prev, nullptr, samples, bins, dropped, stream);
}

// include/admpc_quad_targets.h: the observation over the flown time
int admpc_quad_observe_var_batch(const AdmpcQuadSolver* model, const AdmpcQuadPlantParams* plant, const AdmpcQuadObserveParams* obs, int B,
                                 const double* u, int64_t u_stride, const double* x, double* prev, const int32_t* nsub, double* samples,
                                 double* bins, int32_t* dropped, void* stream)
{
    return quad_observe_entry("admpc_quad_observe_var_batch", true, model, plant, obs, B, u, u_stride, x, prev, nsub, samples, bins, dropped, stream);
}

int admpc_quad_gp_fit(int device, const AdmpcQuadObserveParams* obs, int min_count, const double* bins, AdmpcGp* gp_out, int32_t* info,
                      void* stream)
{
    const int rc = admpc_quad_observe_params_check("admpc_quad_gp_fit", obs);
    return rc ? rc : admpc_learn_fit("admpc_quad_gp_fit", device, obs->n_gp, obs->gp, QUAD_LEARN.feat_lo, min_count, bins, gp_out, info, stream);
}

int admpc_quad_gp_install(AdmpcQuadSolver* s, int n_gp, const AdmpcGp* gp_dev, int32_t* installed, void* stream)
{
    if (!s) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_gp_install: null solver");
    int device = 0, have = 0;
    (void)admpc_quad_solver_info(s, &device, nullptr, nullptr);
    AdmpcQuadConfig* d_cfg = admpc_quad_solver_config_device(s, &have);
    if (have < 1 || n_gp != have) {
        char msg[180];
        snprintf(msg, sizeof msg, "admpc_quad_gp_install: n_gp = %d, but the handle was created with %d GPs (create it with placeholder GPs of n_points = 0)", n_gp, have);
        return admpc_set_error(ADMPC_EINVAL, msg);
    }
    if (!gp_dev || !installed) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_gp_install: null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_quad_gp_install_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, d_cfg, n_gp, gp_dev, installed);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_gp_install_kernel: launch failed");
    return ADMPC_OK;
}

// The refusals of admpc_quad_rollout_observe_batch behind its arguments' block, in its order; 0 also where B == 0 or T == 0, whose arrays are
// not looked at.  The logged rollout of admpc_quad_clusters.hip has one refusal more behind these.
int admpc_quad_rollout_observe_check(const QuadRolloutArgs& a, int T, const AdmpcQuadSolver* model, const AdmpcQuadObserveParams* obs,
                                     const double* prev, const double* samples, const double* bins, const int32_t* dropped)
{
    int rc = admpc_quad_observe_params_check("admpc_quad_rollout_observe_batch", obs);
    if (rc) return rc;
    if (!model) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_observe_batch: null model");
    // the rollout's own refusals but those of its arrays, which are among the ones below
    rc = admpc_quad_rollout_check(a, T);
    if (rc) return rc;
    int device = 0, model_device = 0;
    (void)admpc_quad_solver_info(a.s, &device, nullptr, nullptr);
    (void)admpc_quad_solver_info(model, &model_device, nullptr, nullptr);
    if (model_device != device) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_observe_batch: the model lives on another device than the solver");
    if (a.B == 0 || T == 0) return ADMPC_OK;
    if (!a.traj_of || !a.idx || !a.x || !a.xbar || !a.ubar || !a.yref || !a.yref_e || !a.status || !a.tally || !a.counts || !prev || !samples || !bins || !dropped ||
        (a.ens && !a.route))
        return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_observe_batch: null array argument");
    if (a.noise && !a.noise_step) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_noise_batch: null noise_step");
    return ADMPC_OK;
}

// admpc_quad_rollout_observe_batch behind its arguments' block: the refusals, the no-ops, the latch and the T observed periods; with
// a.noise the plant of every period is the noisy one (admpc_quad_plant.hip), whose counter array is refused last; with a.ens the solve of
// every period is the ensemble's routed one and the bin launch the ensemble's (admpc_quad_ensemble.hip), obs being the block its clusters
// share.  Period t writes and bins the records at samples + t * samples_step: 0 for one [B][14] that every period overwrites.
int admpc_quad_rollout_observe_run(const QuadRolloutArgs& a, int T, double* traj_out, double* u_out, const AdmpcQuadSolver* model,
                                   const AdmpcQuadObserveParams* obs, double* prev, double* samples, long long samples_step, double* bins,
                                   int32_t* dropped, void* stream)
{
    const int B = a.B;
    int rc = admpc_quad_rollout_observe_check(a, T, model, obs, prev, samples, bins, dropped);
    if (rc || B == 0 || T == 0) return rc;
    int device = 0, N = 0;
    (void)admpc_quad_solver_info(a.s, &device, &N, nullptr);
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    rc = admpc_quad_latch_launch(B, a.x, prev, stream);
    for (int t = 0; t < T && !rc; ++t) {
        const QuadRecordSlots rec = admpc_quad_record_slots(traj_out, u_out, B, t);
        rc = admpc_quad_rollout_enqueue(a, rec.traj_pre, rec.traj_post, rec.u_out, a.route_out ? a.route_out + (size_t)t * B : nullptr, stream);
        if (!rc) rc = admpc_quad_observe_launch(model, a.plant, obs, a.ens, B, a.ubar, (long long)N * QU, a.x, prev, nullptr, samples + (long long)t * samples_step, bins, dropped, stream);
    }
    return rc;
}

int admpc_quad_rollout_observe_batch(AdmpcQuadSolver* s, const AdmpcQuadTrajBank* bank, const AdmpcQuadPlantParams* plant, int over, int B,
                                     int T, const int32_t* traj_of, int32_t* idx, double* x, double* xbar, double* ubar,
                                     double* yref, double* yref_e, double* cost, int32_t* status, int32_t* iters,
                                     double* tally, int32_t* counts, double* traj_out, double* u_out,
                                     const AdmpcQuadSolver* model, const AdmpcQuadObserveParams* obs,
                                     double* prev, double* samples, double* bins, int32_t* dropped, void* stream)
{
    const QuadRolloutArgs a = { s, bank, plant, over, B, traj_of, idx, x, xbar, ubar, yref, yref_e, cost, status, iters, tally, counts, nullptr, nullptr };
    return admpc_quad_rollout_observe_run(a, T, traj_out, u_out, model, obs, prev, samples, 0, bins, dropped, stream);
}

}  // extern "C"
