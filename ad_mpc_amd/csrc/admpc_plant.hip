// admpc_plant.hip -- the plant step of a fleet (include/admpc_plant.h: admpc_plant_step_batch) and the launch behind every step of a
// rollout (admpc_rollout_lane_batch, at the end of admpc_step.hip): one kernel, admpc_plant_kernel.
//
//   inputs   an MPC record (mode == 1, finite fields) drives the model with its acceleration and steering-angle velocity, clipped to the
//            model's input bounds (create_ros_ad_mpc.py:96,98); every other record is the auxiliary controller's brake record
//            (gp_ad_mpc_node.py:455-476): steering held, the plant's braking acceleration
//   model    M classic RK4 steps of model_dev.h's f(x, u, p), GP residual included -- the state part of rk4_group, the same model_eval;
//            after each the steering is clipped to its bounds and v_x raised to v_min
//   yaw      bound_angle_within_pi once, at the end (ref_traj.py:28)
//   tally    (rollout only) the step's tracking errors summed, the records counted, the trajectory slot written
//
// Three lanes per vehicle and 63 tasks per 64-thread block, the lane map of admpc_shoot_kernel / admpc_shift_kernel: gp_eval shares its
// kernel sums among the three lanes of a task.  All three carry the same state through the sub-steps; lane 0 of the triple stores.
#include <stdio.h>
#include <math.h>
#include "admpc_host.h"

#define NX ADMPC_NX
#define NU ADMPC_NU
#define NY ADMPC_NY
#define WAVE 64
#define LIN_TASKS 63     // tasks per block (multiple of 3), as in admpc_kernels.hip

// what one launch works on (passed by value); the rollout's pointers are null for a plant-only step
struct PlantArgs {
    double h, blend_min, blend_max, brake, v_min;
    int M, B;
    const float* ack;            // [B][4]
    const int32_t* mode;         // [B]
    double* st[NX];              // px, py, yaw, vx, vy, yaw_rate, steer: [B] each, in/out
    const double* err;           // [B][3] out_err of the step's generator, or null
    const int32_t* status;       // [B]
    const int32_t* valid;        // [B]
    double* tally;               // [B][3]
    int32_t* counts;             // [B][3]
    double* traj_pre;            // [7][B] the state before the period, or null
    double* traj_post;           // [7][B] the state after it, or null
};

namespace {

#include "model_dev.h"
#include "plant_dev.h"       // rk4_state, plant_blend: shared with the observation of a step (admpc_learn.hip)

// bound_angle_within_pi (ref_traj.py:28) with Python's floor modulo
__device__ __forceinline__ double wrap_pi(double a)
{
#pragma clang fp contract(off)
    double m = fmod(a + M_PI, 2.0 * M_PI);
    if (m < 0.0) m = m + 2.0 * M_PI;
    return m - M_PI;
}

// the sums of a rollout for one vehicle: every operation rounded on its own, so that numpy reproduces them bit for bit
__device__ __forceinline__ void plant_tally(const PlantArgs& a, long b)
{
#pragma clang fp contract(off)
    const double ey = a.err[b * 3 + 1], epsi = a.err[b * 3 + 2];
    double* t = a.tally + b * 3;
    if (isfinite(ey) && isfinite(epsi)) {
        t[0] = t[0] + ey * ey;
        t[1] = t[1] + epsi * epsi;
        const double ay = fabs(ey);
        if (ay > t[2]) t[2] = ay;
    }
    int32_t* n = a.counts + b * 3;
    n[0] = n[0] + 1;
    if (a.mode[b] == 1) n[1] = n[1] + 1;
    if (a.status[b] != 0 || a.valid[b] == 0) n[2] = n[2] + 1;
}

}  // namespace

__global__ __launch_bounds__(WAVE) void admpc_plant_kernel(const AdmpcConfig* __restrict__ cfg, const PlantArgs a)
{
    const long total = (long)a.B * 3;
    if (threadIdx.x >= LIN_TASKS) return;                // the task -> lane map of the shooting kernels (gp_eval relies on it)
    const double lbu0 = cfg->lbu[0], ubu0 = cfg->ubu[0], lbu1 = cfg->lbu[1], ubu1 = cfg->ubu[1];
    const double dl_min = cfg->lbx_delta, dl_max = cfg->ubx_delta;
    for (long tsk = (long)blockIdx.x * LIN_TASKS + threadIdx.x; tsk < total; tsk += (long)gridDim.x * LIN_TASKS) {
        const long b = tsk / 3; const int g = (int)(tsk % 3);
        double x[NX], u[NU];
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = a.st[i][b];
        if (g == 0 && a.traj_pre) {
#pragma unroll
            for (int i = 0; i < NX; ++i) a.traj_pre[(long)i * a.B + b] = x[i];
        }
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
            if (x[6] < dl_min) x[6] = dl_min;
            if (x[6] > dl_max) x[6] = dl_max;
            if (x[3] < a.v_min) x[3] = a.v_min;
        }
        x[2] = wrap_pi(x[2]);
        if (g == 0) {
#pragma unroll
            for (int i = 0; i < NX; ++i) a.st[i][b] = x[i];
            if (a.traj_post) {
#pragma unroll
                for (int i = 0; i < NX; ++i) a.traj_post[(long)i * a.B + b] = x[i];
            }
            if (a.tally) plant_tally(a, b);
        }
    }
}

extern "C" {

// The refusals of the plant parameters, for the entry points that take them (`who` leads the message).
int admpc_plant_params_check(const char* who, const AdmpcPlantParams* plant)
{
    char msg[160];
    const char* what = nullptr;
    if (!plant) what = "the plant parameters are not set";
    else if (!(plant->dt > 0) || !isfinite(plant->dt)) what = "dt must be positive and finite";
    else if (!(plant->blend_max > plant->blend_min)) what = "blend_max must exceed blend_min";
    else if (!(plant->brake_acc <= 0)) what = "brake_acc must not be positive";
    else if (!(plant->v_min >= 0)) what = "v_min must not be negative";
    else if (plant->substeps < 1 || plant->substeps > 64) what = "substeps must be in [1, 64]";
    if (!what) return ADMPC_OK;
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return admpc_set_error(ADMPC_EINVAL, msg);
}

// One launch of admpc_plant_kernel for checked arguments, B > 0, on the model's device (the caller holds it).  st: the seven pose
// arrays; err .. counts null for a plant-only step; traj_pre / traj_post null or [7][B].
int admpc_plant_launch(const AdmpcSolver* model, const AdmpcPlantParams* plant, int B, const float* ack, const int32_t* mode,
                       double* const* st, const double* err, const int32_t* status, const int32_t* valid, double* tally,
                       int32_t* counts, double* traj_pre, double* traj_post, void* stream)
{
    const AdmpcConfig* cfg = admpc_solver_config(model, nullptr);
    PlantArgs a;
    a.h = plant->dt / plant->substeps;
    a.blend_min = plant->blend_min; a.blend_max = plant->blend_max;
    a.brake = plant->brake_acc > cfg->lbu[0] ? plant->brake_acc : cfg->lbu[0];
    a.v_min = plant->v_min;
    a.M = plant->substeps; a.B = B;
    a.ack = ack; a.mode = mode;
    for (int i = 0; i < NX; ++i) a.st[i] = st[i];
    a.err = err; a.status = status; a.valid = valid; a.tally = tally; a.counts = counts;
    a.traj_pre = traj_pre; a.traj_post = traj_post;
    const int nblk = (int)(((long)B * 3 + LIN_TASKS - 1) / LIN_TASKS);
    int grid = nblk < 4096 ? nblk : 4096;
    hipLaunchKernelGGL(admpc_plant_kernel, dim3((unsigned)grid), dim3(WAVE), 0, (hipStream_t)stream, admpc_solver_config_device(model), a);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_plant_kernel: launch failed");
    return ADMPC_OK;
}

int admpc_plant_step_batch(const AdmpcSolver* model, const AdmpcPlantParams* plant, int B,
                           const float* ack, const int32_t* mode,
                           double* px, double* py, double* yaw, double* vx, double* vy, double* yaw_rate, double* steer,
                           void* stream)
{
    const int rc = admpc_plant_params_check("admpc_plant_step_batch", plant);
    if (rc) return rc;
    if (!model || B < 0) return admpc_set_error(ADMPC_EINVAL, "admpc_plant_step_batch: null model or negative batch");
    if (B == 0) return ADMPC_OK;
    if (!ack || !mode || !px || !py || !yaw || !vx || !vy || !yaw_rate || !steer)
        return admpc_set_error(ADMPC_EINVAL, "admpc_plant_step_batch: null array argument");
    int device = 0;
    (void)admpc_solver_config(model, &device);
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    double* st[NX] = { px, py, yaw, vx, vy, yaw_rate, steer };
    return admpc_plant_launch(model, plant, B, ack, mode, st, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

}  // extern "C"
