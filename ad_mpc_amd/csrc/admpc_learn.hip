// admpc_learn.hip -- fitting a handle's residual GP on the device from the steps a fleet has taken (include/admpc_learn.h):
//
//   observe  admpc_observe_kernel  the model's own prediction of the period that has just passed, from the latched poses and the record
//                                  the step issued; what the plant did beyond it, per second, is the sample (three lanes per vehicle,
//                                  the plant kernel's map: gp_eval shares its sums among a triple)
//   bin      admpc_bin_kernel      one wave per (regressor, bin): count, feature sums and target sum of the samples of that bin, in a
//                                  stated order, so that numpy reproduces them bit for bit
//   fit      admpc_gp_fit_kernel   one wave per regressor: the bin means are the points; K by exp_nonpos; Cholesky with one row per
//                                  lane, the matrix in LDS (33 doubles a row), pivots passed by lane reads.  The same with the row in
//                                  registers and every loop unrolled took 256 VGPRs, 256 AGPRs and 728 bytes of scratch per lane.
//   install  admpc_gp_install_kernel   one wave: checks each record and copies it into the handle's device configuration
//
// The hyperparameters are given (admpc_learn.h: scope); the body of the fit is in gp_fit_dev.h, which admpc_hyper.hip shares for the fit at
// searched hyperparameters.  The rollout with observation is at the end of the file.
#include <stdio.h>
#include <math.h>
#include "admpc_host.h"

#define NX ADMPC_NX
#define NU ADMPC_NU
#define NY ADMPC_NY
#include "gp_fit_dev.h"   // WAVE, NPT, ACC; LearnGp, LearnArgs; the body of the fit
#define LIN_TASKS 63     // tasks per block (multiple of 3), as in admpc_kernels.hip
#define REC 10           // doubles per sample record

// what one launch of the observe kernel works on (passed by value)
struct ObserveArgs {
    double h, dt, blend_min, blend_max, brake;
    int M, B;
    const float* ack;            // [B][4]
    const int32_t* mode;         // [B]
    const double* st[NX];        // px, py, yaw, vx, vy, yaw_rate, steer: [B] each, the poses now
    double* prev;                // [7][B] the poses one period ago, in/out
    double* samples;             // [B][REC]
};

namespace {

#include "model_dev.h"
#include "plant_dev.h"

// the record of one vehicle and the latch; every operation rounded on its own, so that numpy reproduces the flag bit for bit
__device__ __forceinline__ void observe_record(const ObserveArgs& a, long b, const double* z, const double* u, const double* now, const double* xh)
{
#pragma clang fp contract(off)
    double* r = a.samples + b * REC;
    bool fin = isfinite(u[0]) && isfinite(u[1]);
#pragma unroll
    for (int i = 0; i < 4; ++i) { r[i] = z[i]; fin = fin && isfinite(z[i]); }
    r[4] = u[0]; r[5] = u[1];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double y = (now[3 + j] - xh[3 + j]) / a.dt;
        r[6 + j] = y;
        fin = fin && isfinite(y);
    }
    r[9] = fin ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) a.prev[(long)i * a.B + b] = now[i];
}

}  // namespace

__global__ void admpc_latch_kernel(int B, const double* p0, const double* p1, const double* p2, const double* p3, const double* p4,
                                   const double* p5, const double* p6, double* __restrict__ prev)
{
    const double* st[NX] = { p0, p1, p2, p3, p4, p5, p6 };
    for (long b = (long)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += (long)gridDim.x * blockDim.x) {
#pragma unroll
        for (int i = 0; i < NX; ++i) prev[(long)i * B + b] = st[i][b];
    }
}

__global__ __launch_bounds__(WAVE) void admpc_observe_kernel(const AdmpcConfig* __restrict__ cfg, const ObserveArgs a)
{
    const long total = (long)a.B * 3;
    if (threadIdx.x >= LIN_TASKS) return;                // the task -> lane map of the shooting kernels (gp_eval relies on it)
    const double lbu0 = cfg->lbu[0], ubu0 = cfg->ubu[0], lbu1 = cfg->lbu[1], ubu1 = cfg->ubu[1];
    for (long tsk = (long)blockIdx.x * LIN_TASKS + threadIdx.x; tsk < total; tsk += (long)gridDim.x * LIN_TASKS) {
        const long b = tsk / 3; const int g = (int)(tsk % 3);
        double x[NX], now[NX], z[4], u[NU];
#pragma unroll
        for (int i = 0; i < NX; ++i) { x[i] = a.prev[(long)i * a.B + b]; now[i] = a.st[i][b]; }
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = x[3 + i];
        const double p = plant_blend(x[3], a.blend_min, a.blend_max);
        const double acc = (double)a.ack[b * 4 + 3], rate = (double)a.ack[b * 4 + 1];
        const bool mpc = a.mode[b] == 1 && isfinite(acc) && isfinite(rate);
        u[0] = mpc ? fmin(fmax(acc, lbu0), ubu0) : a.brake;
        u[1] = mpc ? fmin(fmax(rate, lbu1), ubu1) : 0.0;
        for (int m = 0; m < a.M; ++m) {                  // uniform over the wave: the shuffles of gp_eval see every lane of a triple
            double phi[NX];
            rk4_state(cfg, x, u, p, a.h, phi);
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] = phi[i];
        }
        // the latch is behind the integration: every lane of the triple has consumed its loads of prev before lane 0 of it stores
        if (g == 0) observe_record(a, b, z, u, now, x);
    }
}

// grid n_gp * NPT: block (g, bin).  Bin 0 of a regressor also counts what fell outside its box, block 0 also what was not valid.
__global__ __launch_bounds__(WAVE) void admpc_bin_kernel(const LearnArgs a)
{
    gp_bin_body<REC, 3, 6, ADMPC_GP_MAX>(a, (int)blockIdx.x / NPT, (int)blockIdx.x % NPT);      // gp_fit_dev.h: shared with the quadrotor's
}

// grid n_gp, one wave each: the fit at the hyperparameters given to the regressor (gp_fit_dev.h has the body, which admpc_hyper.hip shares).
__global__ __launch_bounds__(WAVE) void admpc_gp_fit_kernel(const LearnArgs a)
{
    const int g = (int)blockIdx.x;
    const LearnGp& G = a.gp[g];
    const GpHyper h = { G.sigma_f, { G.inv_l2[0], G.inv_l2[1], G.inv_l2[2] }, G.noise, 0 };
    gp_fit_body(a, g, h);
}

// one wave.  src [n_gp] -> cfg->gp[0 .. n_gp); a record that fails the check is replaced by the empty GP (gp_fit_dev.h has the body).
__global__ __launch_bounds__(WAVE) void admpc_gp_install_kernel(AdmpcConfig* cfg, int n_gp, const AdmpcGp* src, int32_t* installed)
{
    gp_install_body<CAR_LEARN.feat_lo, CAR_LEARN.feat_hi, CAR_LEARN.out_lo, CAR_LEARN.out_hi>(cfg->gp, n_gp, src, installed);
}

// ---- the host side both vehicles share (gp_fit_dev.h declares it; admpc_quad_learn.hip and admpc_hyper.hip call it) ----

extern "C" int admpc_learn_refuse(const char* who, const char* what)
{
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return admpc_set_error(ADMPC_EINVAL, msg);
}

// The refusals of the regressors of a parameter block, behind those of its head, which is the vehicle's own.
extern "C" int admpc_learn_regressors_check(const char* who, int n_gp, const AdmpcGpBins* gp, const LearnRanges& r)
{
    char what[120], range[40];
    what[0] = 0;
    if (n_gp < 1 || n_gp > r.n_gp_max) snprintf(what, sizeof what, "n_gp must be in [1, %d]", r.n_gp_max);
    for (int g = 0; !what[0] && g < n_gp; ++g) {
        const AdmpcGpBins& b = gp[g];
        const int nf = b.n_feat;
        const char* bad = nullptr;
        if (nf < 1 || nf > ADMPC_GP_MAX_FEAT) bad = "n_feat must be in [1, 3]";
        for (int d = 0; !bad && d < nf; ++d)
            if (b.feat[d] < r.feat_lo || b.feat[d] > r.feat_hi) { snprintf(range, sizeof range, "feat must be in [%d, %d]", r.feat_lo, r.feat_hi); bad = range; }
        if (!bad && (b.out < r.out_lo || b.out > r.out_hi)) { snprintf(range, sizeof range, "out must be in [%d, %d]", r.out_lo, r.out_hi); bad = range; }
        long prod = 1;
        for (int d = 0; !bad && d < 3; ++d) {
            if (b.nb[d] < 1 || (d >= nf && b.nb[d] != 1)) bad = "nb must be >= 1, and 1 for an unused feature";
            else if ((prod *= b.nb[d]) > NPT) bad = "the product of nb must not exceed 32";
        }
        for (int d = 0; !bad && d < nf; ++d) if (!isfinite(b.lo[d]) || !isfinite(b.hi[d]) || !(b.hi[d] > b.lo[d])) bad = "lo and hi must be finite, hi > lo";
        if (!bad && (!(b.sigma_f > 0) || !isfinite(b.sigma_f))) bad = "sigma_f must be positive and finite";
        for (int d = 0; !bad && d < nf; ++d) if (!(b.length[d] > 0) || !isfinite(b.length[d])) bad = "length must be positive and finite";
        if (!bad && (!(b.noise > 0) || !isfinite(b.noise))) bad = "noise must be positive and finite";
        if (!bad && (!(b.count_noise >= 0) || !isfinite(b.count_noise))) bad = "count_noise must not be negative";
        if (bad) snprintf(what, sizeof what, "regressor %d: %s", g, bad);
    }
    return what[0] ? admpc_learn_refuse(who, what) : ADMPC_OK;
}

// The regressors as the bin kernels and the fit read them; an unused feature slot names feature `unused_feat`, which nothing reads.
extern "C" void admpc_learn_fill(LearnArgs& a, int n_gp, const AdmpcGpBins* gp, int unused_feat)
{
    a.n_gp = n_gp;
    for (int g = 0; g < ADMPC_GP_MAX; ++g) {
        LearnGp& G = a.gp[g];
        G = LearnGp();
        if (g >= n_gp) continue;
        const AdmpcGpBins& b = gp[g];
        G.n_feat = b.n_feat; G.out = b.out; G.nbins = 1;
        for (int d = 0; d < 3; ++d) {
            const bool used = d < b.n_feat;
            G.feat[d] = used ? b.feat[d] : unused_feat; G.nb[d] = used ? b.nb[d] : 1; G.nbins *= G.nb[d];
            G.lo[d] = used ? b.lo[d] : 0.0;
            G.scale[d] = used ? (double)b.nb[d] / (b.hi[d] - b.lo[d]) : 0.0;
            G.inv_l2[d] = used ? 1.0 / (b.length[d] * b.length[d]) : 0.0;
        }
        G.sigma_f = b.sigma_f; G.noise = b.noise; G.count_noise = b.count_noise;
    }
}

// admpc_gp_fit and admpc_quad_gp_fit behind the check of their parameter block: a __global__ function is launched from its own unit.
extern "C" int admpc_learn_fit(const char* who, int device, int n_gp, const AdmpcGpBins* gp, int unused_feat, int min_count, const double* bins,
                               AdmpcGp* gp_out, int32_t* info, void* stream)
{
    if (min_count < 1) return admpc_learn_refuse(who, "min_count must be at least 1");
    if (!bins || !gp_out || !info) return admpc_learn_refuse(who, "null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    LearnArgs l = LearnArgs();
    admpc_learn_fill(l, n_gp, gp, unused_feat);
    l.min_count = (double)min_count; l.bins = const_cast<double*>(bins); l.out = gp_out; l.info = info;
    hipLaunchKernelGGL(admpc_gp_fit_kernel, dim3((unsigned)n_gp), dim3(WAVE), 0, (hipStream_t)stream, l);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_gp_fit_kernel: launch failed");
    return ADMPC_OK;
}

// The refusals of the observe parameters, for the entry points that take them (`who` leads the message); admpc_hyper.hip's too.
extern "C" int admpc_observe_params_check(const char* who, const AdmpcObserveParams* obs)
{
    if (!obs) return admpc_learn_refuse(who, "the observe parameters are not set");
    if (!(obs->dt > 0) || !isfinite(obs->dt)) return admpc_learn_refuse(who, "dt must be positive and finite");
    if (!(obs->blend_max > obs->blend_min)) return admpc_learn_refuse(who, "blend_max must exceed blend_min");
    if (obs->substeps < 1 || obs->substeps > 64) return admpc_learn_refuse(who, "substeps must be in [1, 64]");
    return admpc_learn_regressors_check(who, obs->n_gp, obs->gp, CAR_LEARN);
}

namespace {

// The two launches of an observation for checked arguments, B > 0, on the model's device (the caller holds it).
int observe_launch(const AdmpcSolver* model, const AdmpcPlantParams* plant, const AdmpcObserveParams* obs, int B, const float* ack,
                   const int32_t* mode, const double* const* st, double* prev, double* samples, double* bins, int32_t* dropped, void* stream)
{
    const AdmpcConfig* cfg = admpc_solver_config(model, nullptr);
    ObserveArgs a;
    a.h = obs->dt / obs->substeps; a.dt = obs->dt;
    a.blend_min = obs->blend_min; a.blend_max = obs->blend_max;
    a.brake = plant->brake_acc > cfg->lbu[0] ? plant->brake_acc : cfg->lbu[0];
    a.M = obs->substeps; a.B = B;
    a.ack = ack; a.mode = mode;
    for (int i = 0; i < NX; ++i) a.st[i] = st[i];
    a.prev = prev; a.samples = samples;
    const int nblk = (int)(((long)B * 3 + LIN_TASKS - 1) / LIN_TASKS);
    const int grid = nblk < 4096 ? nblk : 4096;
    hipLaunchKernelGGL(admpc_observe_kernel, dim3((unsigned)grid), dim3(WAVE), 0, (hipStream_t)stream, admpc_solver_config_device(model), a);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_observe_kernel: launch failed");
    LearnArgs l = LearnArgs();
    admpc_learn_fill(l, obs->n_gp, obs->gp, CAR_LEARN.feat_lo);
    l.B = B; l.samples = samples; l.bins = bins; l.dropped = dropped;
    hipLaunchKernelGGL(admpc_bin_kernel, dim3((unsigned)(obs->n_gp * NPT)), dim3(WAVE), 0, (hipStream_t)stream, l);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_bin_kernel: launch failed");
    return ADMPC_OK;
}

int latch_launch(int B, const double* const* st, double* prev, void* stream)
{
    const int nblk = (B + 255) / 256;
    hipLaunchKernelGGL(admpc_latch_kernel, dim3((unsigned)(nblk < 4096 ? nblk : 4096)), dim3(256), 0, (hipStream_t)stream, B, st[0], st[1], st[2],
                       st[3], st[4], st[5], st[6], prev);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_latch_kernel: launch failed");
    return ADMPC_OK;
}

}  // namespace

extern "C" {

int admpc_observe_latch_batch(int device, int B, const double* px, const double* py, const double* yaw, const double* vx, const double* vy,
                              const double* yaw_rate, const double* steer, double* prev, void* stream)
{
    if (B < 0) return admpc_set_error(ADMPC_EINVAL, "admpc_observe_latch_batch: negative batch");
    if (B == 0) return ADMPC_OK;
    if (!px || !py || !yaw || !vx || !vy || !yaw_rate || !steer || !prev)
        return admpc_set_error(ADMPC_EINVAL, "admpc_observe_latch_batch: null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    const double* st[NX] = { px, py, yaw, vx, vy, yaw_rate, steer };
    return latch_launch(B, st, prev, stream);
}

int admpc_observe_batch(const AdmpcSolver* model, const AdmpcPlantParams* plant, const AdmpcObserveParams* obs, int B,
                        const float* ack, const int32_t* mode,
                        const double* px, const double* py, const double* yaw, const double* vx, const double* vy,
                        const double* yaw_rate, const double* steer,
                        double* prev, double* samples, double* bins, int32_t* dropped, void* stream)
{
    int rc = admpc_observe_params_check("admpc_observe_batch", obs);
    if (rc) return rc;
    rc = admpc_plant_params_check("admpc_observe_batch", plant);
    if (rc) return rc;
    if (!model || B < 0) return admpc_set_error(ADMPC_EINVAL, "admpc_observe_batch: null model or negative batch");
    if (B == 0) return ADMPC_OK;
    if (!ack || !mode || !px || !py || !yaw || !vx || !vy || !yaw_rate || !steer || !prev || !samples || !bins || !dropped)
        return admpc_set_error(ADMPC_EINVAL, "admpc_observe_batch: null array argument");
    int device = 0;
    (void)admpc_solver_config(model, &device);
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    const double* st[NX] = { px, py, yaw, vx, vy, yaw_rate, steer };
    return observe_launch(model, plant, obs, B, ack, mode, st, prev, samples, bins, dropped, stream);
}

int admpc_gp_fit(int device, const AdmpcObserveParams* obs, int min_count, const double* bins, AdmpcGp* gp_out, int32_t* info, void* stream)
{
    const int rc = admpc_observe_params_check("admpc_gp_fit", obs);
    return rc ? rc : admpc_learn_fit("admpc_gp_fit", device, obs->n_gp, obs->gp, CAR_LEARN.feat_lo, min_count, bins, gp_out, info, stream);
}

int admpc_gp_install(AdmpcSolver* s, int n_gp, const AdmpcGp* gp_dev, int32_t* installed, void* stream)
{
    if (!s) return admpc_set_error(ADMPC_EINVAL, "admpc_gp_install: null solver");
    int device = 0;
    const int have = admpc_solver_config(s, &device)->n_gp;
    if (have < 1 || n_gp != have) {
        char msg[160];
        snprintf(msg, sizeof msg, "admpc_gp_install: n_gp = %d, but the handle was created with %d GPs (create it with placeholder GPs of n_points = 0)", n_gp, have);
        return admpc_set_error(ADMPC_EINVAL, msg);
    }
    if (!gp_dev || !installed) return admpc_set_error(ADMPC_EINVAL, "admpc_gp_install: null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_gp_install_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, admpc_solver_config_device_rw(s), n_gp, gp_dev, installed);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_gp_install_kernel: launch failed");
    return ADMPC_OK;
}

int admpc_rollout_observe_lane_batch(AdmpcSolver* s, const AdmpcPathBank* bank, const AdmpcLaneParams* lane, const AdmpcStepParams* prm,
                                     const AdmpcSolver* plant_model, const AdmpcPlantParams* plant, int B, int T,
                                     const int32_t* path_of, int32_t* lane_idx,
                                     double* px, double* py, double* yaw, double* vx, double* vy, double* yaw_rate, double* steer,
                                     double* xbar, double* ubar, int32_t* safe_count, double* prev_u, int32_t* has_valid, void* work,
                                     float* ack, int32_t* mode, int32_t* valid, int32_t* status, double* cost,
                                     double* tally, int32_t* counts, double* traj,
                                     const AdmpcSolver* model, const AdmpcObserveParams* obs,
                                     double* prev, double* samples, double* bins, int32_t* dropped, void* stream)
{
    const RolloutArgs a = { s, bank, lane, prm, plant_model, plant, B, path_of, lane_idx, { px, py, yaw, vx, vy, yaw_rate, steer },
                            { xbar, ubar, safe_count, prev_u, has_valid, work, ack, mode, valid, status, cost }, tally, counts };
    int rc = admpc_observe_params_check("admpc_rollout_observe_lane_batch", obs);
    if (rc) return rc;
    if (!model) return admpc_set_error(ADMPC_EINVAL, "admpc_rollout_observe_lane_batch: null model");
    // the rollout's own refusals but those of its arrays, which are among the ones below
    rc = admpc_rollout_check_step(a);
    if (!rc) rc = admpc_rollout_check_run(a, T);
    if (rc) return rc;
    int device = 0, model_device = 0;
    (void)admpc_solver_config(s, &device);
    (void)admpc_solver_config(model, &model_device);
    if (model_device != device) return admpc_set_error(ADMPC_EINVAL, "admpc_rollout_observe_lane_batch: the model lives on another device than the solver");
    if (B == 0 || T == 0) return ADMPC_OK;
    if (!path_of || !px || !py || !yaw || !vx || !vy || !yaw_rate || !steer || !xbar || !ubar || !safe_count || !prev_u || !has_valid || !work ||
        !ack || !mode || !valid || !status || !tally || !counts || !prev || !samples || !bins || !dropped)
        return admpc_set_error(ADMPC_EINVAL, "admpc_rollout_observe_lane_batch: null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    rc = latch_launch(B, a.st, prev, stream);
    const size_t slot = (size_t)NX * B;
    // slot 0 is written by the first launch; every launch writes the state it leaves into the next slot
    for (int t = 0; t < T && !rc; ++t) {
        rc = admpc_rollout_enqueue(a, (traj && t == 0) ? traj : nullptr, traj ? traj + (t + 1) * slot : nullptr, stream);
        if (!rc) rc = observe_launch(model, plant, obs, B, ack, mode, a.st, prev, samples, bins, dropped, stream);
    }
    return rc;
}

}  // extern "C"
