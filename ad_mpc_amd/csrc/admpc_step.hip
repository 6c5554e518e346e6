// admpc_step.hip -- the batched control step of a fleet (include/admpc.h: admpc_control_step_batch): what the reference node does
// for one pose message (nodes/gp_ad_mpc_node.py:389-438 -> run_mpc :160-230), for B vehicles on one global path, as one chain of
// launches on one stream:
//
//   admpc_waypoints_batch      RefTrajectory.get_waypoints                         ref_traj.py:89-171
//   admpc_resample_vel_batch   the speed clamp, on each vehicle's local window     gp_ad_mpc_node.py:344-349 (see below)
//   P  admpc_step_assemble_kernel  x0, padded references, yaw fix, blend p      gp_ad_mpc_node.py:180-187,410; ad_3d_optimizer.py:347-349,
//                                                                                :423-443
//   admpc_solve_batch          one SQP-RTI step (kernel F at N = 20, kernel S at N = 40 / 60, kernel R otherwise)
//   Q  admpc_step_command_kernel   validity, fallback, previous valid inputs,   ad_3d_optimizer.py:385-394,:466-476;
//                                  Ackermann fields, the node's gate            create_ros_ad_mpc.py:92-98; gp_ad_mpc_node.py:199-235,:455-476
//
// The one deliberate deviation: the node clamps the speed of the GLOBAL path once per waypoint message, at the speed the vehicle had
// then (:351-368).  Vehicles at different speeds cannot share that, so the clamp runs on each vehicle's local window of N speeds at its
// current speed (what admpc_resample_vel_batch documents); AdmpcStepParams.resample = 0 turns it off.  The step along a route
// (admpc_control_step_lane_batch, at the end of this file) has a lane to clamp and clamps that, as the node does.
//
// The assembly computes bit for bit what the host functions of ad_mpc_amd/host.py compute (same operations, same order, no
// contraction); the command kernel's distance tests sum in the order of a wave reduction (numpy's own sum is pairwise).
#include <stdio.h>
#include <math.h>
#include "admpc_host.h"

#define NX ADMPC_NX
#define NU ADMPC_NU
#define NY ADMPC_NY
#define WAVE 64
#define STEP_MAX_H WAVE     // admpc_waypoints_batch, and the command kernel: one lane per slot of the horizon

namespace {

// P: one thread per (vehicle, row j = 0..N).  ref [B][6][N] (x, y, psi, v, cdist, curv of the waypoint kernel, H = N).
//   j < N : yref[b][j] = [x_j, y_j, yaw_fix(psi_j), v_j, 0, 0, 0 | 0, 0]   (the node's rows :180-187, its zero input references)
//   j = N : yref_e[b] = row N-1 again (pad_reference repeats the last row) with the yaw fixed; x0[b] (:410); p[b] = vel_switch(v_x)
__global__ void admpc_step_assemble_kernel(int N, int B, const double* __restrict__ ref,
                                           const double* __restrict__ px, const double* __restrict__ py, const double* __restrict__ yaw,
                                           const double* __restrict__ vx, const double* __restrict__ vy, const double* __restrict__ yaw_rate,
                                           const double* __restrict__ steer, double blend_min, double blend_max,
                                           double* __restrict__ x0, double* __restrict__ yref, double* __restrict__ yref_e, double* __restrict__ p)
{
#pragma clang fp contract(off)      // every operation rounded on its own, as the host's numpy arithmetic does
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)B * (N + 1)) return;
    const int b = (int)(t / (N + 1)), j = (int)(t - (long)b * (N + 1));
    const double* r = ref + (size_t)b * 6 * N;
    const int k = j < N ? j : N - 1;
    // host.yaw_fix (ad_3d_optimizer.py:423-437): relative to the sign of the initial yaw x0[2]
    const double psi0 = yaw[b];
    double psi = r[2 * N + k];
    if (psi0 < 0.0 && psi0 + M_PI < psi) psi = psi - 2.0 * M_PI;
    else if (psi0 > 0.0 && psi0 - M_PI > psi) psi = psi + 2.0 * M_PI;
    double* o = j < N ? yref + ((size_t)b * N + j) * NY : yref_e + (size_t)b * NX;
    o[0] = r[k]; o[1] = r[N + k]; o[2] = psi; o[3] = r[3 * N + k]; o[4] = 0.0; o[5] = 0.0; o[6] = 0.0;
    if (j < N) { o[7] = 0.0; o[8] = 0.0; return; }
    double* x = x0 + (size_t)b * NX;
    x[0] = px[b]; x[1] = py[b]; x[2] = psi0; x[3] = vx[b]; x[4] = vy[b]; x[5] = yaw_rate[b]; x[6] = steer[b];
    // host.vel_switch (ad_3d_optimizer.py:443): clip((v_x - blend_min) / (blend_max - blend_min), 0, 1), NaN kept as numpy keeps it
    double q = (vx[b] - blend_min) / (blend_max - blend_min);
    if (q < 0.0) q = 0.0;
    if (q > 1.0) q = 1.0;
    p[b] = q;
}

// Wave reductions over the 64 lanes (every lane receives the result).
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, WAVE));
    return v;
}

// The distance test of ad_3d_optimizer.py:385-394 / gp_ad_mpc_node.py:248-257 over n slots, the last one 0: lane i holds the XY
// distance d of slot i (i < n - 1); mean < 3, unbiased variance < 2, max < 4.  n <= WAVE + 1: a slot beyond the last lane is the
// trailing zero and enters the variance as (0 - mean)^2.
__device__ int path_close(double d, int lane, int n)
{
#pragma clang fp contract(off)
    const double di = lane < n - 1 ? d : 0.0;
    const double mean = wave_sum(di) / n;
    const double dv = lane < n ? di - mean : 0.0;
    double var = wave_sum(dv * dv);
    if (n > WAVE) var += mean * mean;
    var /= (n - 1);
    const double mx = wave_max(di);
    return (mean < 3.0 && var < 2.0 && mx < 4.0) ? 1 : 0;
}

// Q: one wave per vehicle (lane i <-> slot i of the horizon), behind the solve.  In the order of the reference:
//   valid      is_valid_command(x_opt, target) against the padded target, N + 1 slots (ad_3d_optimizer.py:466)
//   fallback   not valid and a previous valid solution exists: w[0:2] = prev[2:4] (host.fallback_command; only those two reach the
//              message, :474-476)
//   prev       valid: prev_u = this step's inputs, has_valid = 1 (:467-468)
//   message    steering_angle = x_opt[0,6], steering_angle_velocity = w[1], speed = x_opt[0,3], acceleration = w[0]
//              (create_ros_ad_mpc.py:95-98, float32 fields)
//   gate       check_pred_trj(x_opt, ref) against the node's N-row window, N slots (:203); status > 0 resets safe_count, else +1;
//              an MPC command needs safe_count >= threshold and a healthy prediction, with the steering command
//              clip(clip(rate) * 0.1 + measured steering) (:206-223); otherwise the auxiliary controller's brake record (:455-476)
//   cost       (the step against a bank of paths only; nullptr otherwise) +inf where the solve failed or the prediction is not valid
// Vehicle b, called by every lane of the block's single wave.
__device__ __forceinline__ void step_command_one(int N, int b, const double* __restrict__ ref, const double* __restrict__ xbar,
                                          const double* __restrict__ ubar, const int32_t* __restrict__ status, const double* __restrict__ steer,
                                          int32_t* __restrict__ safe_count, double* __restrict__ prev_u, int32_t* __restrict__ has_valid,
                                          int threshold, double rate_min, double rate_max, double steer_min, double steer_max,
                                          float* __restrict__ ack, int32_t* __restrict__ mode, int32_t* __restrict__ valid, double* __restrict__ cost)
{
#pragma clang fp contract(off)      // the steering command is two separately rounded operations in the reference (:223)
    const int lane = threadIdx.x;
    const double* x = xbar + (size_t)b * (N + 1) * NX;
    const double* rx = ref + (size_t)b * 6 * N;
    const double* ry = rx + N;
    const double* u = ubar + (size_t)b * N * NU;
    double* pu = prev_u + (size_t)b * N * NU;
    double d = 0.0;
    if (lane < N) {
        const double dxv = rx[lane] - x[lane * NX], dyv = ry[lane] - x[lane * NX + 1];
        d = __dsqrt_rn(dxv * dxv + dyv * dyv);
    }
    const int ok_pred = path_close(d, lane, N + 1);
    const int healthy = path_close(d, lane, N);
    const int had = has_valid[b];
    double w0 = u[0], w1 = u[1];
    if (!ok_pred && had) { w0 = pu[2]; w1 = pu[3]; }
    __syncthreads();                                              // every lane has read prev_u before it is overwritten
    if (ok_pred)
        for (int i = lane; i < N * NU; i += WAVE) pu[i] = u[i];
    if (lane == 0) {
        if (ok_pred) has_valid[b] = 1;
        const int cnt = status[b] > 0 ? 0 : safe_count[b] + 1;
        safe_count[b] = cnt;
        const int ok = (cnt >= threshold && healthy) ? 1 : 0;
        const double sth = steer[b];
        if (ok) {
            const double rate_msg = (double)(float)w1;                   // the value travels through a float32 message field
            const double sv = fmax(fmin(rate_max, rate_msg), rate_min);
            const double scaled = sv * 0.1;
            const double ang = fmax(fmin(steer_max, scaled + sth), steer_min);
            ack[b * 4 + 0] = (float)ang; ack[b * 4 + 1] = (float)w1; ack[b * 4 + 2] = (float)x[3]; ack[b * 4 + 3] = (float)w0;
        } else {
            ack[b * 4 + 0] = (float)sth; ack[b * 4 + 1] = 0.0f; ack[b * 4 + 2] = 0.0f; ack[b * 4 + 3] = (float)(-1e5);
        }
        mode[b] = ok;
        valid[b] = ok_pred;
        if (cost && (status[b] != 0 || !ok_pred)) cost[b] = INFINITY;
    }
}

// cost [B]: null, or (the steps against a bank) the objective of each solve, masked in place
__global__ __launch_bounds__(WAVE) void admpc_step_command_kernel(int N, int B, const double* __restrict__ ref, const double* __restrict__ xbar,
                                          const double* __restrict__ ubar, const int32_t* __restrict__ status, const double* __restrict__ steer,
                                          int32_t* __restrict__ safe_count, double* __restrict__ prev_u, int32_t* __restrict__ has_valid,
                                          int threshold, double rate_min, double rate_max, double steer_min, double steer_max,
                                          float* __restrict__ ack, int32_t* __restrict__ mode, int32_t* __restrict__ valid,
                                          double* __restrict__ cost)
{
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        step_command_one(N, b, ref, xbar, ubar, status, steer, safe_count, prev_u, has_valid, threshold, rate_min, rate_max, steer_min, steer_max,
                         ack, mode, valid, cost);
    }
}

// workspace layout: every region on a 256-byte boundary
inline size_t align32(size_t n) { return (n + 31) / 32 * 32; }
struct StepWork {
    double *ref, *err, *x0, *yref, *yref_e, *p;
    int32_t* stop;
    size_t bytes;
    StepWork(void* base, int N, int B) {
        double* w = (double*)base;
        size_t o = 0;
        ref = w + o; o += align32((size_t)B * 6 * N);
        err = w + o; o += align32((size_t)B * 3);
        x0 = w + o; o += align32((size_t)B * NX);
        yref = w + o; o += align32((size_t)B * N * NY);
        yref_e = w + o; o += align32((size_t)B * NX);
        p = w + o; o += align32((size_t)B);
        stop = (int32_t*)(w + o); o += align32(((size_t)B + 1) / 2);
        bytes = o * sizeof(double);
    }
};

const char STEP[] = "admpc_control_step_batch", BANK[] = "admpc_control_step_bank_batch", LANE[] = "admpc_control_step_lane_batch",
           ROLLOUT[] = "admpc_rollout_lane_batch";

int refuse(const char* who, const char* what)
{
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return admpc_set_error(ADMPC_EINVAL, msg);
}

// The refusals the three steps share, in the order every one of them makes them: check_solver, then those of the step's own reference
// source, then check_params; an empty batch returns there, and the others need arrays_set.
int check_solver(const char* who, const AdmpcSolver* s, const AdmpcStepParams* prm, int B, const AdmpcConfig** cfg, int* device)
{
    if (!s || !prm || B < 0) return refuse(who, "null solver / params or negative batch");
    *cfg = admpc_solver_config(s, device);
    if ((*cfg)->N < 3 || (*cfg)->N > STEP_MAX_H) return refuse(who, "the solver's N must be in [3, 64] (the waypoint kernel's horizon)");
    return ADMPC_OK;
}

int check_params(const char* who, const AdmpcStepParams* prm)
{
    if (prm->threshold < 0 || !(prm->blend_max > prm->blend_min)) return refuse(who, "bad step parameters");
    return ADMPC_OK;
}

// all of them for a step whose reference source is a bank
int check_bank_step(const char* who, const AdmpcSolver* s, const AdmpcPathBank* bank, const AdmpcStepParams* prm, int B, const AdmpcConfig** cfg,
                    int* device)
{
    int bank_device = 0;
    const int rc = check_solver(who, s, prm, B, cfg, device);
    if (rc) return rc;
    if (!bank) return refuse(who, "the bank is not set");
    if (admpc_path_bank_horizon(bank, &bank_device) != (*cfg)->N) return refuse(who, "the bank's horizon H must equal the solver's N");
    if (bank_device != *device) return refuse(who, "the bank lives on another device than the solver");
    return check_params(who, prm);
}

// st: the seven pose arrays, px .. steer
bool arrays_set(const double* const* st, const StepOut& o)
{
    for (int i = 0; i < NX; ++i) if (!st[i]) return false;
    return o.xbar && o.ubar && o.safe_count && o.prev_u && o.has_valid && o.work && o.ack && o.mode && o.valid && o.status;
}

// The chain behind the reference generator, which has left ref [B][6][N] in the workspace: assembly, solve, command.  For checked
// arguments and B > 0, on the solver's device (the caller holds it).
int step_tail(AdmpcSolver* s, const AdmpcConfig* cfg, const AdmpcStepParams* prm, int B, const StepWork& w, const double* const* st,
              const StepOut& o, void* stream)
{
    const int N = cfg->N;
    const double* steer = st[6];
    const long nP = (long)B * (N + 1);
    hipLaunchKernelGGL(admpc_step_assemble_kernel, dim3((unsigned)((nP + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, B, (const double*)w.ref,
                       st[0], st[1], st[2], st[3], st[4], st[5], steer, prm->blend_min, prm->blend_max, w.x0, w.yref, w.yref_e, w.p);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_step_assemble_kernel: launch failed");
    const int rc = admpc_solve_batch(s, B, w.x0, w.yref, w.yref_e, w.p, o.xbar, o.ubar, o.cost, o.status, nullptr, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(admpc_step_command_kernel, dim3(B < 65536 ? B : 65536), dim3(WAVE), 0, (hipStream_t)stream, N, B, (const double*)w.ref,
                       (const double*)o.xbar, (const double*)o.ubar, (const int32_t*)o.status, steer, o.safe_count, o.prev_u, o.has_valid,
                       prm->threshold, cfg->lbu[1], cfg->ubu[1], cfg->lbx_delta, cfg->ubx_delta, o.ack, o.mode, o.valid, o.cost);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_step_command_kernel: launch failed");
    return ADMPC_OK;
}

// the speed clamp on each vehicle's window, behind the waypoint call of the steps that have no lane to clamp
int clamp_window(const AdmpcStepParams* prm, int device, int N, int B, const double* const* st, const StepWork& w, void* stream)
{
    if (!prm->resample) return ADMPC_OK;
    return admpc_resample_vel_batch(device, B, N, 6 * N, st[3], st[4], prm->acc_max, prm->resample_dt, w.ref + 3 * N, stream);
}

}  // namespace

extern "C" {

int admpc_control_step_workspace(const AdmpcSolver* s, int B, size_t* bytes)
{
    if (!s || B < 0 || !bytes) return admpc_set_error(ADMPC_EINVAL, "admpc_control_step_workspace: bad argument");
    *bytes = StepWork(nullptr, admpc_solver_config(s, nullptr)->N, B).bytes;
    return ADMPC_OK;
}

int admpc_control_step_batch(AdmpcSolver* s, const AdmpcPath* path, const AdmpcStepParams* prm, int B,
                             const double* px, const double* py, const double* yaw, const double* vx, const double* vy,
                             const double* yaw_rate, const double* steer,
                             double* xbar, double* ubar, int32_t* safe_count, double* prev_u, int32_t* has_valid,
                             void* work, float* ack, int32_t* mode, int32_t* valid, int32_t* status, void* stream)
{
    const double* st[NX] = { px, py, yaw, vx, vy, yaw_rate, steer };
    const StepOut o = { xbar, ubar, safe_count, prev_u, has_valid, work, ack, mode, valid, status, nullptr };
    const AdmpcConfig* cfg = nullptr;
    int device = 0;
    int rc = check_solver(STEP, s, prm, B, &cfg, &device);
    if (rc) return rc;
    const int N = cfg->N;
    if (!path || path->M < 2 || !path->vel || !path->x || !path->y || !path->psi || !path->psi_unwrapped || !path->cdist || !path->curv)
        return refuse(STEP, "the path is not set");
    if (path->H != N) return refuse(STEP, "the path horizon H must equal the solver's N");
    if (!(path->dt > 0)) return refuse(STEP, "the path needs dt > 0");
    rc = check_params(STEP, prm);
    if (rc || B == 0) return rc;
    if (!arrays_set(st, o)) return refuse(STEP, "null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    const StepWork w(work, N, B);
    rc = admpc_waypoints_batch(device, path->M, N, path->dt, B, path->vel, path->x, path->y, path->psi, path->psi_unwrapped,
                               path->cdist, path->curv, px, py, yaw, w.ref, w.err, w.stop, stream);
    if (!rc) rc = clamp_window(prm, device, N, B, st, w, stream);
    return rc ? rc : step_tail(s, cfg, prm, B, w, st, o, stream);
}

// admpc_control_step_batch with a path per vehicle and the objective of each solve (include/admpc_fleet.h): the differences are the
// waypoint call and `cost`, which the solve fills and the command kernel masks.
int admpc_control_step_bank_batch(AdmpcSolver* s, const AdmpcPathBank* bank, const AdmpcStepParams* prm, int B, const int32_t* path_of,
                                  const double* px, const double* py, const double* yaw, const double* vx, const double* vy,
                                  const double* yaw_rate, const double* steer,
                                  double* xbar, double* ubar, int32_t* safe_count, double* prev_u, int32_t* has_valid,
                                  void* work, float* ack, int32_t* mode, int32_t* valid, int32_t* status, double* cost, void* stream)
{
    const double* st[NX] = { px, py, yaw, vx, vy, yaw_rate, steer };
    const StepOut o = { xbar, ubar, safe_count, prev_u, has_valid, work, ack, mode, valid, status, cost };
    const AdmpcConfig* cfg = nullptr;
    int device = 0;
    int rc = check_bank_step(BANK, s, bank, prm, B, &cfg, &device);
    if (rc || B == 0) return rc;
    if (!path_of || !arrays_set(st, o)) return refuse(BANK, "null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    const StepWork w(work, cfg->N, B);
    rc = admpc_waypoints_bank_batch(bank, B, path_of, px, py, yaw, w.ref, w.err, w.stop, stream);
    if (!rc) rc = clamp_window(prm, device, cfg->N, B, st, w, stream);
    return rc ? rc : step_tail(s, cfg, prm, B, w, st, o, stream);
}

// admpc_control_step_bank_batch along a route (include/admpc_lane.h): the lane generator of admpc_lane.hip cuts, clamps and tabulates a
// local lane per vehicle and lays the window on it, in place of the waypoint call and of the clamp on the window behind it.
int admpc_control_step_lane_batch(AdmpcSolver* s, const AdmpcPathBank* bank, const AdmpcLaneParams* lane, const AdmpcStepParams* prm, int B,
                                  const int32_t* path_of, int32_t* lane_idx,
                                  const double* px, const double* py, const double* yaw, const double* vx, const double* vy,
                                  const double* yaw_rate, const double* steer,
                                  double* xbar, double* ubar, int32_t* safe_count, double* prev_u, int32_t* has_valid,
                                  void* work, float* ack, int32_t* mode, int32_t* valid, int32_t* status, double* cost, void* stream)
{
    const double* st[NX] = { px, py, yaw, vx, vy, yaw_rate, steer };
    const StepOut o = { xbar, ubar, safe_count, prev_u, has_valid, work, ack, mode, valid, status, cost };
    const AdmpcConfig* cfg = nullptr;
    int device = 0;
    int rc = admpc_lane_params_check(LANE, lane, lane_idx);
    if (!rc) rc = check_bank_step(LANE, s, bank, prm, B, &cfg, &device);
    if (rc || B == 0) return rc;
    if (!path_of || !arrays_set(st, o)) return refuse(LANE, "null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    const StepWork w(work, cfg->N, B);
    rc = admpc_waypoints_lane_batch(bank, lane, B, path_of, lane_idx, px, py, yaw, vx, vy, prm->resample, prm->acc_max, prm->resample_dt,
                                    w.ref, w.err, w.stop, stream);
    return rc ? rc : step_tail(s, cfg, prm, B, w, st, o, stream);
}

// The refusals of a rollout before those of its arrays: its own of the lane and plant parameters, then the lane step's, under that step's name.
int admpc_rollout_check_step(const RolloutArgs& a)
{
    const AdmpcConfig* cfg = nullptr;
    int device = 0;
    int rc = admpc_lane_params_check(ROLLOUT, a.lane, a.lane_idx);
    if (!rc) rc = admpc_plant_params_check(ROLLOUT, a.plant);
    return rc ? rc : check_bank_step(LANE, a.s, a.bank, a.prm, a.B, &cfg, &device);
}

// Those behind its arrays, for arguments that have passed admpc_rollout_check_step.
int admpc_rollout_check_run(const RolloutArgs& a, int T)
{
    if (T < 0 || T > 4096) return refuse(ROLLOUT, "T must be in [0, 4096]");
    int device = 0, plant_device = 0;
    (void)admpc_solver_config(a.s, &device);
    (void)admpc_solver_config(a.plant_model ? a.plant_model : a.s, &plant_device);
    if (plant_device != device) return refuse(ROLLOUT, "the plant model lives on another device than the solver");
    return ADMPC_OK;
}

// One closed-loop period for checked arguments, B > 0, on the solver's device (the caller holds it): the lane step's chain, and behind
// it one launch of admpc_plant_kernel (admpc_plant.hip) that moves the vehicles under the record just issued and tallies the tracking
// errors the step's generator left in the workspace.  traj_pre / traj_post: null or [7][B], the states before and after the period.
int admpc_rollout_enqueue(const RolloutArgs& a, double* traj_pre, double* traj_post, void* stream)
{
    const AdmpcConfig* cfg = admpc_solver_config(a.s, nullptr);
    const StepWork w(a.out.work, cfg->N, a.B);
    int rc = admpc_waypoints_lane_batch(a.bank, a.lane, a.B, a.path_of, a.lane_idx, a.st[0], a.st[1], a.st[2], a.st[3], a.st[4], a.prm->resample,
                                        a.prm->acc_max, a.prm->resample_dt, w.ref, w.err, w.stop, stream);
    if (!rc) rc = step_tail(a.s, cfg, a.prm, a.B, w, a.st, a.out, stream);
    if (rc) return rc;
    return admpc_plant_launch(a.plant_model ? a.plant_model : a.s, a.plant, a.B, a.out.ack, a.out.mode, a.st, w.err, a.out.status, a.out.valid,
                              a.tally, a.counts, traj_pre, traj_post, stream);
}

// T closed-loop steps along a route (include/admpc_plant.h).  Everything is enqueued on `stream`; nothing waits for the device.
int admpc_rollout_lane_batch(AdmpcSolver* s, const AdmpcPathBank* bank, const AdmpcLaneParams* lane, const AdmpcStepParams* prm,
                             const AdmpcSolver* plant_model, const AdmpcPlantParams* plant, int B, int T,
                             const int32_t* path_of, int32_t* lane_idx,
                             double* px, double* py, double* yaw, double* vx, double* vy, double* yaw_rate, double* steer,
                             double* xbar, double* ubar, int32_t* safe_count, double* prev_u, int32_t* has_valid, void* work,
                             float* ack, int32_t* mode, int32_t* valid, int32_t* status, double* cost,
                             double* tally, int32_t* counts, double* traj, void* stream)
{
    const RolloutArgs a = { s, bank, lane, prm, plant_model, plant, B, path_of, lane_idx, { px, py, yaw, vx, vy, yaw_rate, steer },
                            { xbar, ubar, safe_count, prev_u, has_valid, work, ack, mode, valid, status, cost }, tally, counts };
    int rc = admpc_rollout_check_step(a);
    if (rc) return rc;
    if (B > 0 && (!path_of || !arrays_set(a.st, a.out))) return refuse(ROLLOUT, "null array argument");
    rc = admpc_rollout_check_run(a, T);
    if (rc || B == 0 || T == 0) return rc;
    if (!tally || !counts) return refuse(ROLLOUT, "null tally or counts");
    int device = 0;
    (void)admpc_solver_config(s, &device);
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    const size_t slot = (size_t)NX * B;
    // slot 0 is written by the first launch; every launch writes the state it leaves into the next slot
    for (int t = 0; t < T && !rc; ++t)
        rc = admpc_rollout_enqueue(a, (traj && t == 0) ? traj : nullptr, traj ? traj + (t + 1) * slot : nullptr, stream);
    return rc;
}

}  // extern "C"
