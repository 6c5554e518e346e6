// admpc_quad_targets.hip -- flying to random target points and recording, on the device (include/admpc_quad_targets.h): three kernels and
// their host side.
//
//   admpc_quad_target_window_kernel  the recovery of a vehicle that has run away and the point reference of every vehicle, one lane per
//                                    vehicle as the plant kernel maps it, the same grid cap and stride loop
//   admpc_quad_target_draw_kernel    the target a number gives a vehicle, for the host, through the device function the plant uses
//   admpc_quad_targets_reset_kernel  the counters zeroed, `fast` from the state, target number 0
//
// The plant step towards the targets is admpc_quad_plant.hip's (admpc_quad_plant_period_kernel<NOISY, L, true>, behind
// admpc_quad_plant_launch), the observation over the flown time admpc_quad_learn.hip's (admpc_quad_observe_kernel<true>, behind
// admpc_quad_observe_launch); the targets' device text, which the plant kernel shares, is quad_target_dev.h.
#include <math.h>
#include "admpc_host.h"
#include "quad_sim_dev.h"     // QuadPlantArgs

#define WAVE 64
#define QT_GRID 4096           // blocks at most, as the plant kernels'; more vehicles go round the stride loop

static_assert(sizeof(AdmpcQuadTargetParams) == 48, "the layout the Python side mirrors");

constexpr int QX = ADMPC_QUAD_NX, QU = ADMPC_QUAD_NU, QY = ADMPC_QUAD_NY;

namespace {

#include "quad_noise_dev.h"   // philox4x32_10: the generator the uniforms of a target call

}  // namespace

#include "quad_target_dev.h"  // QuadTargetArgs, target_sample, too_fast

__global__ __launch_bounds__(WAVE) void admpc_quad_target_window_kernel(const AdmpcQuadTargetParams t, int B, int N, double* __restrict__ x,
                                                                        const double* __restrict__ target, const uint64_t* __restrict__ target_no,
                                                                        int32_t* __restrict__ n_iter, const int32_t* __restrict__ fast,
                                                                        int32_t* __restrict__ tcounts, double* __restrict__ prev,
                                                                        double* __restrict__ yref, double* __restrict__ yref_e)
{
    for (long long b = (long long)blockIdx.x * WAVE + threadIdx.x; b < B; b += (long long)gridDim.x * WAVE) {
        double row[QX];
#pragma unroll
        for (int i = 0; i < QX; ++i) row[i] = i == 3 ? 1.0 : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) row[i] = target[b * 3 + i];
        const bool done = t.mode == 0 && target_no[b] >= (uint64_t)t.n_preset;
        if (!done && (fast[b] != 0 || n_iter[b] > t.max_iters)) {
#pragma unroll
            for (int i = 0; i < QX; ++i) x[b * QX + i] = row[i];
            if (prev) {
#pragma unroll
                for (int i = 0; i < QX; ++i) prev[b * QX + i] = row[i];
            }
            n_iter[b] = 0;
            tcounts[b * 5 + 1] = tcounts[b * 5 + 1] + 1;
        }
        double* yb = yref + b * (long long)N * QY;
        for (int j = 0; j < N; ++j) {
#pragma unroll
            for (int i = 0; i < QY; ++i) yb[j * QY + i] = i < QX ? row[i] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < QX; ++i) yref_e[b * QX + i] = row[i];
    }
}

// vehicle b: target_out[b] and, if asked, raw[b][0 .. 3]
__global__ __launch_bounds__(WAVE) void admpc_quad_target_draw_kernel(const AdmpcQuadTargetParams t, int B, const double* __restrict__ x, long long x_stride,
                                                                      const uint64_t* __restrict__ target_no, double* __restrict__ target_out,
                                                                      uint64_t* __restrict__ raw)
{
    for (long long b = (long long)blockIdx.x * WAVE + threadIdx.x; b < B; b += (long long)gridDim.x * WAVE) {
        const double pos[3] = { x[b * x_stride], x[b * x_stride + 1], x[b * x_stride + 2] };
        double tg[3];
        uint64_t w[4];
        target_sample(t, (uint32_t)b, target_no[b], pos, tg, w);
#pragma unroll
        for (int i = 0; i < 3; ++i) target_out[b * 3 + i] = tg[i];
        if (raw) {
#pragma unroll
            for (int i = 0; i < 4; ++i) raw[b * 4 + i] = w[i];
        }
    }
}

// counters zeroed, fast from x, target number 0
__global__ __launch_bounds__(WAVE) void admpc_quad_targets_reset_kernel(const AdmpcQuadTargetParams t, int B, const double* __restrict__ x,
                                                                        const double* __restrict__ presets, double* __restrict__ target,
                                                                        uint64_t* __restrict__ target_no, int32_t* __restrict__ n_iter,
                                                                        int32_t* __restrict__ fast, int32_t* __restrict__ tcounts)
{
    for (long long b = (long long)blockIdx.x * WAVE + threadIdx.x; b < B; b += (long long)gridDim.x * WAVE) {
        const double* xb = x + b * QX;
        target_no[b] = 0; n_iter[b] = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) tcounts[b * 5 + i] = 0;
        fast[b] = too_fast(xb[7], xb[8], xb[9], t.v_max);
        double tg[3];
        if (t.mode == 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) tg[i] = presets[b * (long long)t.n_preset * 3 + i];
        }
        else {
            const double pos[3] = { xb[0], xb[1], xb[2] };
            uint64_t w[4];
            target_sample(t, (uint32_t)b, 0, pos, tg, w);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) target[b * 3 + i] = tg[i];
    }
}

// the refusals of the target parameters, in the header's order; for admpc_quad_plant.hip too
extern "C" int admpc_quad_target_params_check(const char* who, const AdmpcQuadTargetParams* t)
{
    if (!t) return admpc_refuse(who, "the target parameters are not set");
    if (t->mode < 0 || t->mode > 2) return admpc_refuse(who, "mode must be 0 (presets), 1 (aggressive) or 2 (uniform)");
    if (!(t->world_radius > 0) || !isfinite(t->world_radius)) return admpc_refuse(who, "world_radius must be positive and finite");
    if (!(t->thresh > 0) || !isfinite(t->thresh)) return admpc_refuse(who, "thresh must be positive and finite");
    if (t->v_max != t->v_max) return admpc_refuse(who, "v_max must not be NaN");
    if (t->max_iters < 0) return admpc_refuse(who, "max_iters must not be negative");
    if (t->mode == 0 && t->n_preset < 1) return admpc_refuse(who, "mode 0 needs n_preset >= 1");
    return ADMPC_OK;
}

namespace {

int grid_of(int B)
{
    const int nblk = (B + WAVE - 1) / WAVE;
    return nblk < QT_GRID ? nblk : QT_GRID;
}

int window_launch(const AdmpcQuadTargetParams* tp, int B, int N, double* x, const double* target, const uint64_t* target_no, int32_t* n_iter,
                  const int32_t* fast, int32_t* tcounts, double* prev, double* yref, double* yref_e, void* stream)
{
    hipLaunchKernelGGL(admpc_quad_target_window_kernel, dim3((unsigned)grid_of(B)), dim3(WAVE), 0, (hipStream_t)stream, *tp, B, N, x, target, target_no,
                       n_iter, fast, tcounts, prev, yref, yref_e);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_target_window_kernel: launch failed");
    return ADMPC_OK;
}

}  // namespace

extern "C" {

int admpc_quad_target_draw_batch(const AdmpcQuadTargetParams* tp, int device, int B, const double* x, int64_t x_stride,
                                 const uint64_t* target_no, double* target_out, uint64_t* raw, void* stream)
{
    const char* who = "admpc_quad_target_draw_batch";
    const int rc = admpc_quad_target_params_check(who, tp);
    if (rc) return rc;
    if (tp->mode == 0) return admpc_refuse(who, "mode 0: the presets are not drawn");
    if (B < 0) return admpc_refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!x || !target_no || !target_out) return admpc_refuse(who, "null array argument");
    if (x_stride < 3) return admpc_refuse(who, "x_stride must be at least 3");
    if (admpc_device_check(device)) return ADMPC_ENODEV;
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_quad_target_draw_kernel, dim3((unsigned)grid_of(B)), dim3(WAVE), 0, (hipStream_t)stream, *tp, B, x, (long long)x_stride,
                       target_no, target_out, raw);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_target_draw_kernel: launch failed");
    return ADMPC_OK;
}

int admpc_quad_targets_reset_batch(const AdmpcQuadTargetParams* tp, int device, int B, const double* x, const double* presets,
                                   double* target, uint64_t* target_no, int32_t* n_iter, int32_t* fast, int32_t* tcounts, void* stream)
{
    const char* who = "admpc_quad_targets_reset_batch";
    const int rc = admpc_quad_target_params_check(who, tp);
    if (rc) return rc;
    if (B < 0) return admpc_refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!x || !target || !target_no || !n_iter || !fast || !tcounts) return admpc_refuse(who, "null array argument");
    if (tp->mode == 0 && !presets) return admpc_refuse(who, "mode 0 needs the presets");
    if (admpc_device_check(device)) return ADMPC_ENODEV;
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_quad_targets_reset_kernel, dim3((unsigned)grid_of(B)), dim3(WAVE), 0, (hipStream_t)stream, *tp, B, x, presets, target,
                       target_no, n_iter, fast, tcounts);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_targets_reset_kernel: launch failed");
    return ADMPC_OK;
}

int admpc_quad_target_window_batch(const AdmpcQuadTargetParams* tp, int device, int B, int N, double* x, const double* target,
                                   const uint64_t* target_no, int32_t* n_iter, const int32_t* fast, int32_t* tcounts, double* prev,
                                   double* yref, double* yref_e, void* stream)
{
    const char* who = "admpc_quad_target_window_batch";
    const int rc = admpc_quad_target_params_check(who, tp);
    if (rc) return rc;
    if (B < 0) return admpc_refuse(who, "negative batch");
    if (N < 2 || N > ADMPC_QUAD_MAX_N) return admpc_refuse(who, "N must be in [2, 24]");
    if (B == 0) return ADMPC_OK;
    if (!x || !target || !n_iter || !fast || !tcounts || !yref || !yref_e) return admpc_refuse(who, "null array argument");
    if (tp->mode == 0 && !target_no) return admpc_refuse(who, "mode 0 needs target_no");
    if (admpc_device_check(device)) return ADMPC_ENODEV;
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    return window_launch(tp, B, N, x, target, target_no, n_iter, fast, tcounts, prev, yref, yref_e, stream);
}

int admpc_quad_rollout_targets_batch(AdmpcQuadSolver* s, const AdmpcQuadPlantParams* plant, const AdmpcQuadTargetParams* tp, int B, int T,
                                     double* x, double* xbar, double* ubar, double* yref, double* yref_e, double* cost, int32_t* status,
                                     int32_t* iters, const double* presets, double* target, uint64_t* target_no, int32_t* n_iter,
                                     int32_t* fast, int32_t* tcounts, int32_t* nsub, double* traj_out, double* u_out, int32_t* nsub_out,
                                     double* target_out, const AdmpcQuadSolver* model, const AdmpcQuadObserveParams* obs, double* prev,
                                     double* samples, double* bins, int32_t* dropped, const AdmpcQuadNoiseParams* noise,
                                     uint64_t* noise_step, void* stream)
{
    const char* who = "admpc_quad_rollout_targets_batch";
    int rc = admpc_quad_plant_params_check(who, plant);
    if (!rc) rc = admpc_quad_target_params_check(who, tp);
    if (!rc && noise) rc = admpc_quad_noise_params_check(who, noise, plant);
    if (!rc && model) rc = admpc_quad_observe_params_check(who, obs);
    if (rc) return rc;
    if (!s) return admpc_refuse(who, "null solver");
    int device = 0, N = 0, sqp = 0;
    (void)admpc_quad_solver_info(s, &device, &N, &sqp);
    if (sqp > 1) return admpc_refuse(who, "a solver in SQP mode (sqp_iters > 1) is not served: the rollout is the RTI loop");
    if (B < 0) return admpc_refuse(who, "negative batch");
    if (T < 0 || T > 4096) return admpc_refuse(who, "T must be in [0, 4096]");
    if (model) {
        int model_device = 0;
        (void)admpc_quad_solver_info(model, &model_device, nullptr, nullptr);
        if (model_device != device) return admpc_refuse(who, "the model lives on another device than the solver");
    }
    if (B == 0 || T == 0) return ADMPC_OK;
    if (!x || !xbar || !ubar || !yref || !yref_e || !status || !target || !target_no || !n_iter || !fast || !tcounts || !nsub ||
        (model && (!prev || !samples || !bins || !dropped)))
        return admpc_refuse(who, "null array argument");
    if (tp->mode == 0 && !presets) return admpc_refuse(who, "mode 0 needs the presets");
    if (noise && !noise_step) return admpc_refuse(who, "null noise_step");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    if (model) rc = admpc_quad_latch_launch(B, x, prev, stream);
    for (int t = 0; t < T && !rc; ++t) {
        rc = window_launch(tp, B, N, x, target, target_no, n_iter, fast, tcounts, model ? prev : nullptr, yref, yref_e, stream);
        if (!rc) rc = admpc_quad_solve_batch_ex(s, B, x, yref, yref_e, nullptr, xbar, ubar, cost, status, iters, stream);
        if (rc) break;
        const QuadRecordSlots rec = admpc_quad_record_slots(traj_out, u_out, B, t);
        QuadPlantArgs a;
        admpc_quad_plant_fill(a, plant, B, ubar, (long long)N * QU, x);
        a.status = status; a.traj_pre = rec.traj_pre; a.traj_post = rec.traj_post; a.u_out = rec.u_out;
        const QuadTargetArgs g = { *tp, presets, target, target_no, n_iter, fast, tcounts, nsub, nsub_out ? nsub_out + (size_t)t * B : nullptr,
                                   target_out ? target_out + (size_t)t * B * 3 : nullptr };
        rc = admpc_quad_plant_launch(a, noise, noise_step, &g, stream);
        if (!rc && model) rc = admpc_quad_observe_launch(model, plant, obs, nullptr, B, ubar, (long long)N * QU, x, prev, nsub, samples, bins, dropped, stream);
    }
    return rc;
}

}  // extern "C"
