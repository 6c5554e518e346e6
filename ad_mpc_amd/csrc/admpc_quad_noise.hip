// admpc_quad_noise.hip -- the simulator's random disturbances on the device (include/admpc_quad_noise.h): their refusals, the draws for
// the host and the noisy rollout's entry.
//
//   admpc_quad_noise_draw_kernel   the ten normals of every (vehicle, sub-step) of one period for the host, one thread each, through
//                                  the device function the plant uses
//
// The noisy plant kernel and its entry are admpc_quad_plant.hip's.  The noisy rollout is admpc_quad_fleet.hip's and
// admpc_quad_learn.hip's (admpc_quad_rollout_run, admpc_quad_rollout_observe_run) with the disturbances in the arguments' block.
#include <math.h>
#include "admpc_host.h"

#define QD_THREADS 256
#define QD_GRID 4096           // blocks of the draw kernel at most
#define NZ 10                  // normals per (vehicle, sub-step)

static_assert(sizeof(AdmpcQuadNoiseParams) == 56, "the layout the Python side mirrors");

namespace {

#include "quad_noise_dev.h"   // philox4x32_10, noise_pair: the generator, which admpc_quad_plant.hip and admpc_quad_targets.hip draw from too

}  // namespace

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

// for this unit, admpc_quad_plant.hip, admpc_quad_targets.hip and admpc_quad_ensemble.hip: refusals 2 .. 6 of
// include/admpc_quad_noise.h, and 7 where there is a plant
extern "C" int admpc_quad_noise_params_check(const char* who, const AdmpcQuadNoiseParams* n, const AdmpcQuadPlantParams* plant)
{
    if (!n) return admpc_refuse(who, "the noise parameters are not set");
    if ((n->noisy != 0 && n->noisy != 1) || (n->motor_noise != 0 && n->motor_noise != 1)) return admpc_refuse(who, "noisy and motor_noise must be 0 or 1");
    if (!n->noisy && !n->motor_noise) return admpc_refuse(who, "noisy and motor_noise are both 0: call admpc_quad_plant_step_batch");
    if (!(n->force_std >= 0) || !isfinite(n->force_std) || !(n->torque_std >= 0) || !isfinite(n->torque_std) || !(n->motor_std >= 0) || !isfinite(n->motor_std))
        return admpc_refuse(who, "force_std, torque_std and motor_std must be non-negative and finite");
    if (!(n->motor_ref > 0) || !isfinite(n->motor_ref) || !isfinite(n->motor_bias)) return admpc_refuse(who, "motor_ref must be positive and finite, motor_bias finite");
    if (plant && n->motor_noise && plant->u_min < 0) return admpc_refuse(who, "motor_noise needs u_min >= 0 (the reference takes sqrt(u_i))");
    return ADMPC_OK;
}

extern "C" {

int admpc_quad_noise_draw_batch(const AdmpcQuadNoiseParams* noise, int device, int B, int substeps, const uint64_t* noise_step,
                                double* z, uint64_t* raw, void* stream)
{
    const char* who = "admpc_quad_noise_draw_batch";
    const int rc = admpc_quad_noise_params_check(who, noise, nullptr);
    if (rc) return rc;
    if (B < 0) return admpc_refuse(who, "negative batch");
    if (substeps < 1 || substeps > 1024) return admpc_refuse(who, "substeps must be in [1, 1024]");
    if (B == 0) return ADMPC_OK;
    if (!noise_step || !z) return admpc_refuse(who, "null array argument");
    if (admpc_device_check(device)) return ADMPC_ENODEV;
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    const long long total = (long long)B * substeps, nblk = (total + QD_THREADS - 1) / QD_THREADS;
    hipLaunchKernelGGL(admpc_quad_noise_draw_kernel, dim3((unsigned)(nblk < QD_GRID ? nblk : QD_GRID)), dim3(QD_THREADS), 0, (hipStream_t)stream,
                       noise->seed, B, substeps, noise_step, z, raw);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_noise_draw_kernel: launch failed");
    return ADMPC_OK;
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
    if (!rc) rc = admpc_quad_noise_params_check(who, noise, plant);
    if (rc) return rc;
    const QuadRolloutArgs a = { s, bank, plant, over, B, traj_of, idx, x, xbar, ubar, yref, yref_e, cost, status, iters, tally, counts, noise, noise_step };
    return model ? admpc_quad_rollout_observe_run(a, T, traj_out, u_out, model, obs, prev, samples, 0, bins, dropped, stream)
                 : admpc_quad_rollout_run(a, T, traj_out, u_out, stream);
}

}  // extern "C"
