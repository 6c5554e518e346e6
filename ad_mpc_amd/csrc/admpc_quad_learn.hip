// admpc_quad_learn.hip -- fitting a quadrotor handle's body-frame residual GPs on the device from the steps a fleet has flown
// (include/admpc_quad_learn.h):
//
//   observe  admpc_quad_observe_kernel     the model's own prediction of the period that has just passed, from the latched state and the
//                                          activations the plant applied; what the plant did beyond it to the body-frame velocity, per
//                                          second, is the sample.  One lane per vehicle, as the plant kernel (admpc_quad_fleet.hip); the
//                                          model is quad_f_tan of quad_model_dev.h, the text the solve kernels integrate, called with zero
//                                          tangents: the doubled arithmetic is nothing next to a solve
//   bin      admpc_quad_bin_kernel         one wave per (regressor, bin): the body of the car's bin kernel (gp_fit_dev.h) on this record
//   fit      admpc_quad_gp_fit_kernel      one wave per regressor: gp_fit_body of gp_fit_dev.h, unchanged
//   install  admpc_quad_gp_install_kernel  one wave: checks each record and copies it into the handle's device configuration
//
// The hyperparameters are given (admpc_quad_learn.h: what is not offered).  The rollout with observation is at the end of the file.
#include <stdio.h>
#include <math.h>
#include "admpc_host.h"

#define NX ADMPC_NX           // model_dev.h (exp_nonpos, which the fit evaluates the kernel with) wants the car's dimensions defined
#define NU ADMPC_NU
#define NY ADMPC_NY
#include "gp_fit_dev.h"       // WAVE, NPT, ACC; LearnGp, LearnArgs; the bodies of the bin kernel and of the fit
#define QREC 14               // doubles per sample record: v_b (3), body rates (3), activations (4), y (3), the flag
#define QO_GRID 4096          // blocks of the observe kernel at most, as the plant kernel's; more vehicles go round the stride loop
#define GP_WORDS (sizeof(AdmpcGp) / 8)

static_assert(sizeof(AdmpcGp) % 8 == 0 && offsetof(AdmpcQuadConfig, gp) % 8 == 0, "AdmpcGp is copied in 8-byte words");
static_assert(ADMPC_QUAD_GP_MAX <= ADMPC_GP_MAX, "LearnArgs holds the regressors of either vehicle");
static_assert(sizeof(AdmpcQuadObserveParams) == 16 + ADMPC_QUAD_GP_MAX * sizeof(AdmpcGpBins) && sizeof(AdmpcGpBins) == 128, "the layout the Python side mirrors");

// what one launch of the observe kernel works on (passed by value)
struct QuadObserveArgs {
    double h, dt, u_min, u_max;
    int M, B;
    const double* u; long long u_stride;      // row b at u + b * u_stride
    const double* x;                          // [B][13] the states now
    double* prev;                             // [B][13] the states one period ago, in/out
    double* samples;                          // [B][QREC]
};

namespace {

#include "model_dev.h"

constexpr int QX = ADMPC_QUAD_NX, QU = ADMPC_QUAD_NU;
typedef AdmpcQuadConfig Cfg;

#include "quad_model_dev.h"

// one classic RK4 step of length h of the model's state alone: quad_f_tan with zero tangents, the GP features from the integrated state
__device__ __forceinline__ void quad_rk4_state(const Cfg* __restrict__ c, double (&x)[QX], const double (&u)[QU], const double h)
{
    const double sx[QX] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 }, su[QU] = { 0, 0, 0, 0 };
    double kx[QX], ax[QX];
#pragma unroll
    for (int i = 0; i < QX; ++i) { kx[i] = 0; ax[i] = 0; }
    // ONE copy of the model in the kernel: with the four stages unrolled the constants of all four copies were held in scalar registers
    // at once (4 SGPR spills, 256 VGPRs); the stage's node and weight are selects, not table reads, which would live in scratch
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {
        const double cs = s == 0 ? 0.0 : (s == 3 ? 1.0 : 0.5), ws = (s == 0 || s == 3) ? 1.0 / 6 : 2.0 / 6;
        double X[QX], f[QX], df[QX];
#pragma unroll
        for (int i = 0; i < QX; ++i) X[i] = x[i] + cs * h * kx[i];
        quad_f_tan(c, X, u, sx, su, false, X, f, df);
#pragma unroll
        for (int i = 0; i < QX; ++i) { kx[i] = f[i]; ax[i] += ws * f[i]; }
    }
#pragma unroll
    for (int i = 0; i < QX; ++i) x[i] = x[i] + h * ax[i];
}

// The velocity of state s in the body frame of s's own attitude: the expressions of quad_rot, every operation rounded on its own, so
// that numpy reproduces the features bit for bit (quad_rot itself is compiled with contraction, as the solve wants it).
__device__ __forceinline__ void body_velocity(const double (&s)[QX], double (&vb)[3])
{
#pragma clang fp contract(off)
    const double qw = s[3], qx = s[4], qy = s[5], qz = s[6];
    double R[3][3];
    R[0][0] = 1 - 2 * (qy * qy + qz * qz); R[0][1] = 2 * (qx * qy - qw * qz); R[0][2] = 2 * (qx * qz + qw * qy);
    R[1][0] = 2 * (qx * qy + qw * qz); R[1][1] = 1 - 2 * (qx * qx + qz * qz); R[1][2] = 2 * (qy * qz - qw * qx);
    R[2][0] = 2 * (qx * qz - qw * qy); R[2][1] = 2 * (qy * qz + qw * qx); R[2][2] = 1 - 2 * (qx * qx + qy * qy);
#pragma unroll
    for (int i = 0; i < 3; ++i) vb[i] = (R[0][i] * s[7] + R[1][i] * s[8]) + R[2][i] * s[9];
}

__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

}  // namespace

__global__ void admpc_quad_latch_kernel(long long n, const double* __restrict__ x, double* __restrict__ prev)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) prev[i] = x[i];
}

__global__ __launch_bounds__(WAVE) void admpc_quad_observe_kernel(const AdmpcQuadConfig* __restrict__ cfg, const QuadObserveArgs a)
{
    for (long long b = (long long)blockIdx.x * WAVE + threadIdx.x; b < a.B; b += (long long)gridDim.x * WAVE) {
        double xh[QX], now[QX], act[QU];
        double* pb = a.prev + b * QX;
        const double* xb = a.x + b * QX;
        const double* ub = a.u + b * a.u_stride;
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
        bool fin = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) { r[i] = vp[i]; r[3 + i] = xh[10 + i]; fin = fin && isfinite(vp[i]) && isfinite(xh[10 + i]); }
#pragma unroll
        for (int m = 0; m < QU; ++m) { r[6 + m] = act[m]; fin = fin && isfinite(act[m]); }
        for (int m = 0; m < a.M; ++m) quad_rk4_state(cfg, xh, act, a.h);
        body_velocity(now, vn);
        body_velocity(xh, vh);
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double y = (vn[j] - vh[j]) / a.dt;
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

// grid n_gp, one wave each: the fit at the hyperparameters given to the regressor
__global__ __launch_bounds__(WAVE) void admpc_quad_gp_fit_kernel(const LearnArgs a)
{
    const int g = (int)blockIdx.x;
    const LearnGp& G = a.gp[g];
    const GpHyper h = { G.sigma_f, { G.inv_l2[0], G.inv_l2[1], G.inv_l2[2] }, G.noise, 0 };
    gp_fit_body(a, g, h);
}

// one wave.  src [n_gp] -> cfg->gp[0 .. n_gp); a record that fails the check is replaced by the empty GP.
__global__ __launch_bounds__(WAVE) void admpc_quad_gp_install_kernel(AdmpcQuadConfig* cfg, int n_gp, const AdmpcGp* src, int32_t* installed)
{
    const int lane = lane_id();
    for (int g = 0; g < n_gp; ++g) {
        const AdmpcGp* s = src + g;
        const int nf = s->n_feat, n = s->n_points, out = s->out;
        bool head = nf >= 1 && nf <= ADMPC_GP_MAX_FEAT && out >= 7 && out <= 9 && n >= 0 && n <= NPT;
        head = head && isfinite(s->sigma_f) && isfinite(s->ymean);
#pragma unroll
        for (int d = 0; d < ADMPC_GP_MAX_FEAT; ++d)
            if (d < nf) head = head && s->feat[d] >= 7 && s->feat[d] < ADMPC_QUAD_NY && isfinite(s->inv_l2[d]);
        bool bad = false;
        if (head && lane < n) {
            bad = !isfinite(s->alpha[lane]);
#pragma unroll
            for (int d = 0; d < ADMPC_GP_MAX_FEAT; ++d)
                if (d < nf) bad = bad || !isfinite(s->Z[d][lane]);
        }
        const bool take = head && __ballot(bad) == 0ull;
        const uint64_t* sw = (const uint64_t*)s;
        uint64_t* dw = (uint64_t*)&cfg->gp[g];
        for (int w = lane; w < (int)GP_WORDS; w += WAVE) {
            // the empty GP: n_feat 1, feat 7 0 0, out 7, n_points 0, every double zero (the six int32 of the head are words 0 .. 2)
            const uint64_t empty = w == 0 ? (1ull | (7ull << 32)) : (w == 2 ? 7ull : 0ull);
            dw[w] = take ? sw[w] : empty;
        }
        if (lane == 0) installed[g] = take ? 1 : 0;
    }
}

namespace {

// The refusals of the observe parameters, for the entry points that take them (`who` leads the message): admpc_learn.hip's, with the
// quadrotor's ranges and without the speed band.
int quad_observe_params_check(const char* who, const AdmpcQuadObserveParams* obs)
{
    char msg[200], what[120];
    what[0] = 0;
    if (!obs) snprintf(what, sizeof what, "the observe parameters are not set");
    else if (!(obs->dt > 0) || !isfinite(obs->dt)) snprintf(what, sizeof what, "dt must be positive and finite");
    else if (obs->substeps < 1 || obs->substeps > 64) snprintf(what, sizeof what, "substeps must be in [1, 64]");
    else if (obs->n_gp < 1 || obs->n_gp > ADMPC_QUAD_GP_MAX) snprintf(what, sizeof what, "n_gp must be in [1, %d]", ADMPC_QUAD_GP_MAX);
    for (int g = 0; !what[0] && g < obs->n_gp; ++g) {
        const AdmpcGpBins& b = obs->gp[g];
        const int nf = b.n_feat;
        const char* bad = nullptr;
        if (nf < 1 || nf > ADMPC_GP_MAX_FEAT) bad = "n_feat must be in [1, 3]";
        for (int d = 0; !bad && d < nf; ++d) if (b.feat[d] < 7 || b.feat[d] >= ADMPC_QUAD_NY) bad = "feat must be in [7, 16]";
        if (!bad && (b.out < 7 || b.out > 9)) bad = "out must be in [7, 9]";
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
    if (!what[0]) return ADMPC_OK;
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return admpc_set_error(ADMPC_EINVAL, msg);
}

// a regressor as the bin kernel and the fit read it (admpc_learn.hip: fill_learn, on the quadrotor's parameter block)
void quad_fill_learn(LearnArgs& a, const AdmpcQuadObserveParams* obs)
{
    a.n_gp = obs->n_gp;
    for (int g = 0; g < ADMPC_GP_MAX; ++g) {
        LearnGp& G = a.gp[g];
        G = LearnGp();
        if (g >= obs->n_gp) continue;
        const AdmpcGpBins& b = obs->gp[g];
        G.n_feat = b.n_feat; G.out = b.out; G.nbins = 1;
        for (int d = 0; d < 3; ++d) {
            const bool used = d < b.n_feat;
            G.feat[d] = used ? b.feat[d] : 7; G.nb[d] = used ? b.nb[d] : 1; G.nbins *= G.nb[d];
            G.lo[d] = used ? b.lo[d] : 0.0;
            G.scale[d] = used ? (double)b.nb[d] / (b.hi[d] - b.lo[d]) : 0.0;
            G.inv_l2[d] = used ? 1.0 / (b.length[d] * b.length[d]) : 0.0;
        }
        G.sigma_f = b.sigma_f; G.noise = b.noise; G.count_noise = b.count_noise;
    }
}

// The two launches of an observation for checked arguments, B > 0, on the model's device (the caller holds it).
int quad_observe_launch(const AdmpcQuadSolver* model, const AdmpcQuadPlantParams* plant, const AdmpcQuadObserveParams* obs, int B,
                        const double* u, long long u_stride, const double* x, double* prev, double* samples, double* bins, int32_t* dropped,
                        void* stream)
{
    QuadObserveArgs a;
    a.h = obs->dt / obs->substeps; a.dt = obs->dt; a.u_min = plant->u_min; a.u_max = plant->u_max;
    a.M = obs->substeps; a.B = B;
    a.u = u; a.u_stride = u_stride; a.x = x; a.prev = prev; a.samples = samples;
    const int nblk = (B + WAVE - 1) / WAVE;
    hipLaunchKernelGGL(admpc_quad_observe_kernel, dim3((unsigned)(nblk < QO_GRID ? nblk : QO_GRID)), dim3(WAVE), 0, (hipStream_t)stream,
                       admpc_quad_solver_config_device(model, nullptr), a);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_observe_kernel: launch failed");
    LearnArgs l = LearnArgs();
    quad_fill_learn(l, obs);
    l.B = B; l.samples = samples; l.bins = bins; l.dropped = dropped;
    hipLaunchKernelGGL(admpc_quad_bin_kernel, dim3((unsigned)(obs->n_gp * NPT)), dim3(WAVE), 0, (hipStream_t)stream, l);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_bin_kernel: launch failed");
    return ADMPC_OK;
}

int quad_latch_launch(int B, const double* x, double* prev, void* stream)
{
    const long long n = (long long)B * QX, nblk = (n + 255) / 256;
    hipLaunchKernelGGL(admpc_quad_latch_kernel, dim3((unsigned)(nblk < 4096 ? nblk : 4096)), dim3(256), 0, (hipStream_t)stream, n, x, prev);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_latch_kernel: launch failed");
    return ADMPC_OK;
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
    return quad_latch_launch(B, x, prev, stream);
}

int admpc_quad_observe_batch(const AdmpcQuadSolver* model, const AdmpcQuadPlantParams* plant, const AdmpcQuadObserveParams* obs, int B,
                             const double* u, int64_t u_stride, const double* x, double* prev, double* samples, double* bins,
                             int32_t* dropped, void* stream)
{
    int rc = quad_observe_params_check("admpc_quad_observe_batch", obs);
    if (rc) return rc;
    rc = admpc_quad_plant_params_check("admpc_quad_observe_batch", plant);
    if (rc) return rc;
    if (!model) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_observe_batch: null model");
    if (B < 0) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_observe_batch: negative batch");
    if (B == 0) return ADMPC_OK;
    if (!u || !x || !prev || !samples || !bins || !dropped) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_observe_batch: null array argument");
    if (u_stride < QU) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_observe_batch: u_stride must be at least 4");
    int device = 0;
    (void)admpc_quad_solver_info(model, &device, nullptr, nullptr);
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    return quad_observe_launch(model, plant, obs, B, u, (long long)u_stride, x, prev, samples, bins, dropped, stream);
}

int admpc_quad_gp_fit(int device, const AdmpcQuadObserveParams* obs, int min_count, const double* bins, AdmpcGp* gp_out, int32_t* info,
                      void* stream)
{
    const int rc = quad_observe_params_check("admpc_quad_gp_fit", obs);
    if (rc) return rc;
    if (min_count < 1) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_gp_fit: min_count must be at least 1");
    if (!bins || !gp_out || !info) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_gp_fit: null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    LearnArgs l = LearnArgs();
    quad_fill_learn(l, obs);
    l.min_count = (double)min_count; l.bins = const_cast<double*>(bins); l.out = gp_out; l.info = info;
    hipLaunchKernelGGL(admpc_quad_gp_fit_kernel, dim3((unsigned)obs->n_gp), dim3(WAVE), 0, (hipStream_t)stream, l);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_gp_fit_kernel: launch failed");
    return ADMPC_OK;
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

int admpc_quad_rollout_observe_batch(AdmpcQuadSolver* s, const AdmpcQuadTrajBank* bank, const AdmpcQuadPlantParams* plant, int over, int B,
                                     int T, const int32_t* traj_of, int32_t* idx, double* x, double* xbar, double* ubar,
                                     double* yref, double* yref_e, double* cost, int32_t* status, int32_t* iters,
                                     double* tally, int32_t* counts, double* traj_out, double* u_out,
                                     const AdmpcQuadSolver* model, const AdmpcQuadObserveParams* obs,
                                     double* prev, double* samples, double* bins, int32_t* dropped, void* stream)
{
    int rc = quad_observe_params_check("admpc_quad_rollout_observe_batch", obs);
    if (rc) return rc;
    if (!model) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_observe_batch: null model");
    // the rollout's own refusals but those of its arrays, which are among the ones below: an empty batch reaches them and launches nothing
    rc = admpc_quad_rollout_batch(s, bank, plant, over, B < 0 ? B : 0, T, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
    if (rc) return rc;
    int device = 0, model_device = 0, N = 0;
    (void)admpc_quad_solver_info(s, &device, &N, nullptr);
    (void)admpc_quad_solver_info(model, &model_device, nullptr, nullptr);
    if (model_device != device) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_observe_batch: the model lives on another device than the solver");
    if (B == 0 || T == 0) return ADMPC_OK;
    if (!traj_of || !idx || !x || !xbar || !ubar || !yref || !yref_e || !status || !tally || !counts || !prev || !samples || !bins || !dropped)
        return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_observe_batch: null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    rc = quad_latch_launch(B, x, prev, stream);
    const size_t slot = (size_t)B * QX;
    // slot t of traj_out is written by step t (slot 0 by the first), slot t + 1 too: every step writes the state it leaves
    for (int t = 0; t < T && !rc; ++t) {
        rc = admpc_quad_rollout_batch(s, bank, plant, over, B, 1, traj_of, idx, x, xbar, ubar, yref, yref_e, cost, status, iters, tally, counts,
                                      traj_out ? traj_out + (size_t)t * slot : nullptr, u_out ? u_out + (size_t)t * B * QU : nullptr, stream);
        if (!rc) rc = quad_observe_launch(model, plant, obs, B, ubar, (long long)N * QU, x, prev, samples, bins, dropped, stream);
    }
    return rc;
}

}  // extern "C"
