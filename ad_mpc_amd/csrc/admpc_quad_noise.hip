// admpc_quad_noise.hip -- the simulator's random disturbances on the device (include/admpc_quad_noise.h): two kernels and their host side.
//
//   admpc_quad_plant_noise_kernel  admpc_quad_plant_kernel (admpc_quad_fleet.hip) with the draws of quad_3d.py:187-202 in every
//                                  sub-step, the stride loop and the grid cap of the plant kernel, the same side outputs of a rollout's
//                                  step.  The draws do not depend on the state, and at B = 4096 the device is mostly empty: a vehicle
//                                  gets QN_LANES lanes, which share out the generator's calls of a chunk of sub-steps and leave the
//                                  normals in LDS; lane 0 then integrates the chunk.  A fleet beyond QN_WIDE_MAX runs the same text
//                                  with one lane per vehicle
//   admpc_quad_noise_draw_kernel   the ten normals of every (vehicle, sub-step) of one period for the host, one thread each, through
//                                  the device function the plant uses
//
// The simulator's device text is quad_sim_dev.h, shared with admpc_quad_fleet.hip.  The noisy rollout is that unit's and
// admpc_quad_learn.hip's (admpc_quad_rollout_run, admpc_quad_rollout_observe_run) with the disturbances in the arguments' block.
#include <stdio.h>
#include <math.h>
#include "admpc_host.h"
#include "quad_sim_dev.h"

#define QX ADMPC_QUAD_NX
#define QU ADMPC_QUAD_NU
#define WAVE 64
#define QP_GRID 4096           // blocks of the noisy plant kernel at most, as admpc_quad_plant_kernel's; more vehicles go round the stride loop
#define QD_THREADS 256
#define QD_GRID 4096           // blocks of the draw kernel at most
#define NZ 10                  // normals per (vehicle, sub-step)
#define QN_LANES 4             // lanes per vehicle of the noisy plant kernel for a fleet of up to QN_WIDE_MAX vehicles: 147 us at B = 4096 and 40 sub-steps,
                               // against 177 with 8, 310 with 16 and 209 .. 213 with one lane per vehicle and no LDS (profiles/HISTORY.md)
#define QN_WIDE_MAX 8192       // beyond, one lane per vehicle: at 8192 four lanes still win (169 against 214 us); 1024 blocks of any width lost
#define QN_LDS_DOUBLES 1600    // the normals of a chunk in LDS, 12.5 KiB a block: 10 sub-steps of 16 vehicles, 2 sub-steps of 64

static_assert(sizeof(AdmpcQuadNoiseParams) == 56, "the layout the Python side mirrors");

namespace {

#include "quad_noise_dev.h"   // philox4x32_10, noise_pair: the generator, which admpc_quad_targets.hip draws from too

}  // namespace

// L lanes of a wave per vehicle, V = 64 / L vehicles per block.  The draws of a chunk of C sub-steps are independent of the state and of
// each other: the L lanes of a vehicle share out its (sub-step, call) pairs and leave the normals in LDS, laid out [sub-step][normal][vehicle]
// so that the leaders read neighbouring words; then lane 0 of the vehicle integrates the chunk.  The body around the sub-steps is
// admpc_quad_plant_kernel's, repeated here and not shared as device functions: routed through such functions the deterministic kernel's
// address arithmetic compiled differently, and its instruction stream is held unchanged.
template <int L>
__global__ __launch_bounds__(WAVE) void admpc_quad_plant_noise_kernel(const QuadPlantArgs a, const AdmpcQuadNoiseParams n, uint64_t* __restrict__ noise_step)
{
    constexpr int V = WAVE / L, C = QN_LDS_DOUBLES / (V * NZ);
    static_assert(WAVE % L == 0 && C >= 1, "whole vehicles per wave, at least one sub-step per chunk");
    __shared__ double zs[C * NZ * V];
    const SimConst c = sim_const(a.p);
    const double fstd = vreg(n.force_std), tstd = vreg(n.torque_std), mbias = vreg(n.motor_bias), mref = vreg(n.motor_ref), mstd = vreg(n.motor_std);
    const int v = (int)threadIdx.x / L, l = (int)threadIdx.x % L;
    const int j_lo = n.motor_noise ? 0 : 2, nj = (n.noisy ? 5 : 2) - j_lo;       // the calls a sub-step needs: 0, 1 the rotors, 2 .. 4 f_d and t_d
    // every test of the loops below is uniform over the block, so the barriers are met by all lanes
    for (long long base = (long long)blockIdx.x * V; base < a.B; base += (long long)gridDim.x * V) {
        const long long b = base + v;
        const bool active = b < a.B, leader = active && l == 0;
        const uint64_t p = active ? noise_step[b] : 0;
        double x[QX], act[QU], f[QU], mean[QU], scale[QU];
        double* xb = a.x + b * QX;
        Thrust th0;
        if (leader) {
#pragma unroll
            for (int i = 0; i < QX; ++i) x[i] = xb[i];
            const double* ub = a.u + b * a.u_stride;
            bool replaced = false;
#pragma unroll
            for (int m = 0; m < QU; ++m) {
                const double raw = ub[m];
                if (a.u_out) a.u_out[b * QU + m] = raw;
                double w = raw < c.u_max ? raw : c.u_max;        // max(min(u, u_max), u_min)
                w = w > c.u_min ? w : c.u_min;
                if (!isfinite(raw)) { w = c.u_min; replaced = true; }
                act[m] = w;
            }
            if (a.tally) quad_tally(a, b, x, replaced);          // the error at the START of the step
            if (a.traj_pre) {
#pragma unroll
                for (int i = 0; i < QX; ++i) a.traj_pre[b * QX + i] = x[i];
            }
            // what does not change over the period: the deterministic thrusts, and the mean and the scale of a rotor's error (:190-191)
#pragma unroll
            for (int i = 0; i < QU; ++i) {
                f[i] = act[i] * c.max_thrust;
                const double q = act[i] / mref;
                mean[i] = mbias * (q * q);
                scale[i] = mstd * sqrt(act[i]);
            }
            th0 = quad_thrust(c, f);
        }
        for (int m0 = 0; m0 < a.p.substeps; m0 += C) {
            const int cnt = a.p.substeps - m0 < C ? a.p.substeps - m0 : C;
            if (active) {
                for (int i = l; i < cnt * nj; i += L) {
                    const int m = i / nj, j = j_lo + (i - m * nj);
                    uint64_t w0, w1;
                    double z0, z1;
                    noise_pair(n.seed, (uint32_t)b, p, m0 + m, j, w0, w1, z0, z1);
                    zs[(m * NZ + 2 * j) * V + v] = z0; zs[(m * NZ + 2 * j + 1) * V + v] = z1;
                }
            }
            __syncthreads();
            if (leader) {
                for (int m = 0; m < cnt; ++m) {
                    const double* z = zs + m * NZ * V + v;       // normal k at z[k * V]
                    Thrust th = th0;
                    if (n.motor_noise) {
#pragma unroll
                        for (int i = 0; i < QU; ++i) {
                            double w = act[i] - (mean[i] + scale[i] * z[i * V]);
                            w = w < c.u_max ? w : c.u_max;
                            w = w > c.u_min ? w : c.u_min;
                            f[i] = w * c.max_thrust;
                        }
                        th = quad_thrust(c, f);
                    }
                    if (n.noisy) {
                        th.fx = fstd * z[4 * V] / c.mass; th.fy = fstd * z[5 * V] / c.mass; th.az = th.az + fstd * z[6 * V] / c.mass;
                        th.ty = th.ty + tstd * z[7 * V]; th.tx = th.tx - tstd * z[8 * V]; th.tz = th.tz + tstd * z[9 * V];
                    }
                    quad_sim_update<true>(c, th, x);
                }
            }
            __syncthreads();
        }
        if (leader) {
#pragma unroll
            for (int i = 0; i < QX; ++i) xb[i] = x[i];
            noise_step[b] = p + 1;
            if (a.traj_post) {
#pragma unroll
                for (int i = 0; i < QX; ++i) a.traj_post[b * QX + i] = x[i];
            }
            if (a.idx) {                                          // idx <- min(idx + 1, M - 1) where the vehicle has a window
                const int k = a.traj_of[b];
                if (k >= 0 && k < a.K) {
                    const int M = a.desc[k].M, i = a.idx[b];
                    if (i >= 0 && i < M) a.idx[b] = i + 1 < M ? i + 1 : M - 1;
                }
            }
        }
    }
}

// thread t = b * substeps + m writes z[t][0 .. 9] and, if asked, raw[t][0 .. 9]
__global__ __launch_bounds__(QD_THREADS) void admpc_quad_noise_draw_kernel(uint64_t seed, int B, int substeps, const uint64_t* __restrict__ noise_step,
                                                                           double* __restrict__ z, uint64_t* __restrict__ raw)
{
    const long long total = (long long)B * substeps;
    for (long long t = (long long)blockIdx.x * QD_THREADS + threadIdx.x; t < total; t += (long long)gridDim.x * QD_THREADS) {
        const long long b = t / substeps;
        const int m = (int)(t - b * substeps);
        const uint64_t p = noise_step[b];
#pragma unroll
        for (int j = 0; j < NZ / 2; ++j) {
            uint64_t w0, w1;
            double z0, z1;
            noise_pair(seed, (uint32_t)b, p, m, j, w0, w1, z0, z1);
            z[t * NZ + 2 * j] = z0; z[t * NZ + 2 * j + 1] = z1;
            if (raw) { raw[t * NZ + 2 * j] = w0; raw[t * NZ + 2 * j + 1] = w1; }
        }
    }
}

namespace {

int refuse(const char* who, const char* what)
{
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return admpc_set_error(ADMPC_EINVAL, msg);
}

// refusals 2 .. 6 of include/admpc_quad_noise.h, and 7 where there is a plant
int noise_params_check(const char* who, const AdmpcQuadNoiseParams* n, const AdmpcQuadPlantParams* plant)
{
    if (!n) return refuse(who, "the noise parameters are not set");
    if ((n->noisy != 0 && n->noisy != 1) || (n->motor_noise != 0 && n->motor_noise != 1)) return refuse(who, "noisy and motor_noise must be 0 or 1");
    if (!n->noisy && !n->motor_noise) return refuse(who, "noisy and motor_noise are both 0: call admpc_quad_plant_step_batch");
    if (!(n->force_std >= 0) || !isfinite(n->force_std) || !(n->torque_std >= 0) || !isfinite(n->torque_std) || !(n->motor_std >= 0) || !isfinite(n->motor_std))
        return refuse(who, "force_std, torque_std and motor_std must be non-negative and finite");
    if (!(n->motor_ref > 0) || !isfinite(n->motor_ref) || !isfinite(n->motor_bias)) return refuse(who, "motor_ref must be positive and finite, motor_bias finite");
    if (plant && n->motor_noise && plant->u_min < 0) return refuse(who, "motor_noise needs u_min >= 0 (the reference takes sqrt(u_i))");
    return ADMPC_OK;
}

}  // namespace

// for admpc_quad_ensemble.hip: the refusals of the disturbances
extern "C" int admpc_quad_noise_params_check(const char* who, const AdmpcQuadNoiseParams* noise, const AdmpcQuadPlantParams* plant) { return noise_params_check(who, noise, plant); }

// for admpc_quad_fleet.hip's period: one launch of the noisy plant kernel
extern "C" int admpc_quad_plant_noise_launch(const QuadPlantArgs& a, const AdmpcQuadNoiseParams* noise, uint64_t* noise_step, void* stream)
{
    // a fleet that does not fill the device by itself gets QN_LANES lanes a vehicle, for the draws; a larger one a lane a vehicle
    static_assert(QN_WIDE_MAX / (WAVE / QN_LANES) <= QP_GRID, "the wide mapping stays within the grid cap");
    if (a.B <= QN_WIDE_MAX) {
        const int per = WAVE / QN_LANES, nblk = (a.B + per - 1) / per;
        hipLaunchKernelGGL(admpc_quad_plant_noise_kernel<QN_LANES>, dim3((unsigned)(nblk < QP_GRID ? nblk : QP_GRID)), dim3(WAVE), 0, (hipStream_t)stream, a, *noise, noise_step);
    }
    else {
        const int nblk = (a.B + WAVE - 1) / WAVE;
        hipLaunchKernelGGL(admpc_quad_plant_noise_kernel<1>, dim3((unsigned)(nblk < QP_GRID ? nblk : QP_GRID)), dim3(WAVE), 0, (hipStream_t)stream, a, *noise, noise_step);
    }
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_plant_noise_kernel: launch failed");
    return ADMPC_OK;
}

extern "C" {

int admpc_quad_noise_draw_batch(const AdmpcQuadNoiseParams* noise, int device, int B, int substeps, const uint64_t* noise_step,
                                double* z, uint64_t* raw, void* stream)
{
    const char* who = "admpc_quad_noise_draw_batch";
    const int rc = noise_params_check(who, noise, nullptr);
    if (rc) return rc;
    if (B < 0) return refuse(who, "negative batch");
    if (substeps < 1 || substeps > 1024) return refuse(who, "substeps must be in [1, 1024]");
    if (B == 0) return ADMPC_OK;
    if (!noise_step || !z) return refuse(who, "null array argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return admpc_set_error(ADMPC_ENODEV, "no such device");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    const long long total = (long long)B * substeps, nblk = (total + QD_THREADS - 1) / QD_THREADS;
    hipLaunchKernelGGL(admpc_quad_noise_draw_kernel, dim3((unsigned)(nblk < QD_GRID ? nblk : QD_GRID)), dim3(QD_THREADS), 0, (hipStream_t)stream,
                       noise->seed, B, substeps, noise_step, z, raw);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_noise_draw_kernel: launch failed");
    return ADMPC_OK;
}

int admpc_quad_plant_step_noise_batch(const AdmpcQuadPlantParams* plant, const AdmpcQuadNoiseParams* noise, int device, int B,
                                      const double* u, int64_t u_stride, double* x, uint64_t* noise_step, void* stream)
{
    const char* who = "admpc_quad_plant_step_noise_batch";
    int rc = admpc_quad_plant_params_check(who, plant);
    if (!rc) rc = noise_params_check(who, noise, plant);
    if (rc) return rc;
    if (B < 0) return refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!u || !x) return refuse(who, "null array argument");
    if (u_stride < QU) return refuse(who, "u_stride must be at least 4");
    if (!noise_step) return refuse(who, "null noise_step");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return admpc_set_error(ADMPC_ENODEV, "no such device");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    QuadPlantArgs a;
    a.p = *plant; a.B = B; a.K = 0;
    a.u = u; a.u_stride = (long long)u_stride; a.x = x;
    a.yref = nullptr; a.yref_stride = 0; a.status = nullptr; a.tally = nullptr; a.counts = nullptr;
    a.traj_of = nullptr; a.idx = nullptr; a.desc = nullptr; a.traj_pre = a.traj_post = nullptr; a.u_out = nullptr;
    return admpc_quad_plant_noise_launch(a, noise, noise_step, stream);
}

int admpc_quad_rollout_noise_batch(AdmpcQuadSolver* s, const AdmpcQuadTrajBank* bank, const AdmpcQuadPlantParams* plant, int over, int B,
                                   int T, const int32_t* traj_of, int32_t* idx, double* x, double* xbar, double* ubar,
                                   double* yref, double* yref_e, double* cost, int32_t* status, int32_t* iters,
                                   double* tally, int32_t* counts, double* traj_out, double* u_out,
                                   const AdmpcQuadSolver* model, const AdmpcQuadObserveParams* obs,
                                   double* prev, double* samples, double* bins, int32_t* dropped,
                                   const AdmpcQuadNoiseParams* noise, uint64_t* noise_step, void* stream)
{
    const char* who = "admpc_quad_rollout_noise_batch";
    int rc = admpc_quad_plant_params_check(who, plant);
    if (!rc) rc = noise_params_check(who, noise, plant);
    if (rc) return rc;
    const QuadRolloutArgs a = { s, bank, plant, over, B, traj_of, idx, x, xbar, ubar, yref, yref_e, cost, status, iters, tally, counts, noise, noise_step };
    return model ? admpc_quad_rollout_observe_run(a, T, traj_out, u_out, model, obs, prev, samples, 0, bins, dropped, stream)
                 : admpc_quad_rollout_run(a, T, traj_out, u_out, stream);
}

}  // extern "C"
