// admpc_quad_plant.hip -- the quadrotor's plant step (include/admpc_quad_fleet.h, admpc_quad_noise.h, admpc_quad_targets.h): two kernel
// texts, the one launch behind every period of a rollout, and the three plant-step entries.
//
//   admpc_quad_plant_kernel         Quadrotor3D.update `substeps` times under one input (quad_3d.py:175-287): substeps x 4 evaluations of
//                                   the simulator's model in a serial chain, ONE lane per vehicle (QP_LANES), everything in registers;
//                                   behind a step of the rollout the same launch does the tally, the counts, the records and the index
//                                   update
//   admpc_quad_plant_period_kernel  <NOISY, L, TARGET>: every other plant step.  NOISY: the draws of quad_3d.py:187-202 in every sub-step.
//                                   The draws do not depend on the state, and at B = 4096 the device is mostly empty: a vehicle gets
//                                   L = QN_LANES lanes, which share out the generator's calls of a chunk of sub-steps and leave the
//                                   normals in LDS; lane 0 then integrates the chunk.  A fleet beyond QN_WIDE_MAX runs the same text with
//                                   one lane per vehicle.  TARGET: the reach test behind every sub-step, and in the same launch the next
//                                   target, the counters and `fast` in place of the rollout's tally and index update; a vehicle that has
//                                   reached keeps meeting the barriers and only skips the integration.  Instantiated as <true, 4, false>
//                                   and <true, 1, false> (the noisy plant), <true, 4, true>, <true, 1, true> and <false, 1, true> (the
//                                   plant towards targets, under the disturbances and without)
//
// The deterministic plant without targets keeps a text of its own: as <false, 1, false> of the shared text it compiled to 1302
// instructions and 232 VGPRs against 1243 and 230, with another register assignment throughout, and routed through shared device
// functions its address arithmetic compiled differently too.  Its instruction stream is held unchanged.  The simulator's device text is
// quad_sim_dev.h, the generator's quad_noise_dev.h, the targets' quad_target_dev.h.
#include <math.h>
#include "admpc_host.h"
#include "quad_sim_dev.h"     // QuadTrajDesc, QuadPlantArgs, the simulator's device text

#define QX ADMPC_QUAD_NX
#define QU ADMPC_QUAD_NU
#define WAVE 64
#define QP_LANES 1             // lanes per vehicle of the plant kernel; four (a lane per state group) measured 1.40 times slower: profiles/HISTORY.md
#define QP_GRID 4096           // blocks of a plant kernel at most (the cap of admpc_plant_kernel); more vehicles go round the stride loop
#define NZ 10                  // normals per (vehicle, sub-step)
// The mapping of the noisy forms, measured twice at B = 4096 (profiles/HISTORY.md has both).  The noisy plant of the circle flight at 40
// sub-steps, the plant launch timed alone: 147 us with QN_LANES = 4 lanes a vehicle, against 177 with 8, 310 with 16 and 209 .. 213 with
// one lane per vehicle and no LDS; at 8192 vehicles four lanes still win (169 against 214 us), and 1024 blocks of any width lost, hence
// QN_WIDE_MAX.  The noisy plant towards targets by kernel trace, the average over the periods of N = 10 and N = 20: 120.3 us with four
// lanes a vehicle against 186.1 us with one (-DQN_WIDE_MAX=0).
#define QN_LANES 4             // lanes per vehicle of a noisy plant kernel for a fleet of up to QN_WIDE_MAX vehicles
#ifndef QN_WIDE_MAX
#define QN_WIDE_MAX 8192       // beyond, one lane per vehicle
#endif
#define QN_LDS_DOUBLES 1600    // the normals of a chunk in LDS, 12.5 KiB a block: 10 sub-steps of 16 vehicles, 2 sub-steps of 64
static_assert(QP_LANES == 1, "admpc_quad_plant_kernel maps one lane to one vehicle");
static_assert(QN_WIDE_MAX / (WAVE / QN_LANES) <= QP_GRID, "the wide mapping stays within the grid cap");

namespace {

#include "quad_noise_dev.h"   // philox4x32_10, noise_pair: the generator

}  // namespace

#include "quad_target_dev.h"  // QuadTargetArgs, target_sample, too_fast, target_reached

__global__ __launch_bounds__(WAVE) void admpc_quad_plant_kernel(const QuadPlantArgs a)
{
    const SimConst c = sim_const(a.p);
    for (long long b = (long long)blockIdx.x * WAVE + threadIdx.x; b < a.B; b += (long long)gridDim.x * WAVE) {
        double x[QX];
        double* xb = a.x + b * QX;
#pragma unroll
        for (int i = 0; i < QX; ++i) x[i] = xb[i];
        const double* ub = a.u + b * a.u_stride;
        double f[QU];
        bool replaced = false;
#pragma unroll
        for (int m = 0; m < QU; ++m) {
            const double raw = ub[m];
            if (a.u_out) a.u_out[b * QU + m] = raw;
            double v = raw < c.u_max ? raw : c.u_max;        // max(min(u, u_max), u_min)
            v = v > c.u_min ? v : c.u_min;
            if (!isfinite(raw)) { v = c.u_min; replaced = true; }
            f[m] = v * c.max_thrust;
        }
        if (a.tally) quad_tally(a, b, x, replaced);          // the error at the START of the step
        if (a.traj_pre) {
#pragma unroll
            for (int i = 0; i < QX; ++i) a.traj_pre[b * QX + i] = x[i];
        }
        const Thrust th = quad_thrust(c, f);
        for (int m = 0; m < a.p.substeps; ++m) quad_sim_update<false>(c, th, x);
#pragma unroll
        for (int i = 0; i < QX; ++i) xb[i] = x[i];
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

// L lanes of a wave per vehicle, V = 64 / L vehicles per block.  The draws of a chunk of C sub-steps are independent of the state and of
// each other: the L lanes of a vehicle share out its (sub-step, call) pairs and leave the normals in LDS, laid out [sub-step][normal][vehicle]
// so that the leaders read neighbouring words; then lane 0 of the vehicle integrates the chunk.  NOISY == false: L == 1, no LDS, no
// barrier, one chunk.  TARGET == false: g is not read, and the tally and the index update are the rollout's.  The two sides store in
// the order they always did (the period counter before the record without targets, behind nsub with them).
template <bool NOISY, int L, bool TARGET>
__global__ __launch_bounds__(WAVE) void admpc_quad_plant_period_kernel(const QuadPlantArgs a, const QuadTargetArgs g, const AdmpcQuadNoiseParams n,
                                                                       uint64_t* __restrict__ noise_step)
{
    constexpr int V = WAVE / L, C = NOISY ? QN_LDS_DOUBLES / (V * NZ) : 1024;
    static_assert(WAVE % L == 0 && C >= 1 && (NOISY || L == 1), "whole vehicles per wave, at least one sub-step per chunk");
    static_assert(NOISY || TARGET, "the deterministic plant without targets is admpc_quad_plant_kernel");
    __shared__ double zs[NOISY ? C * NZ * V : 1];
    const SimConst c = sim_const(a.p);
    double fstd = 0, tstd = 0, mbias = 0, mref = 1, mstd = 0, thresh = 0;
    if (NOISY) { fstd = vreg(n.force_std); tstd = vreg(n.torque_std); mbias = vreg(n.motor_bias); mref = vreg(n.motor_ref); mstd = vreg(n.motor_std); }
    if (TARGET) thresh = vreg(g.t.thresh);
    const int v = (int)threadIdx.x / L, l = (int)threadIdx.x % L;
    const int j_lo = n.motor_noise ? 0 : 2, nj = (n.noisy ? 5 : 2) - j_lo;       // the calls a sub-step needs: 0, 1 the rotors, 2 .. 4 f_d and t_d
    // every test of the chunk loop is uniform over the block, so the barriers are met by all lanes
    for (long long base = (long long)blockIdx.x * V; base < a.B; base += (long long)gridDim.x * V) {
        const long long b = base + v;
        const bool active = b < a.B, leader = active && l == 0;
        uint64_t p = 0;
        if (NOISY) p = active ? noise_step[b] : 0;
        double x[QX], act[QU], f[QU], mean[QU], scale[QU], tg[3];
        double* xb = a.x + b * QX;
        Thrust th0;
        bool replaced = false, done = false, reached = false;
        int nsub = a.p.substeps;
        if (leader) {
#pragma unroll
            for (int i = 0; i < QX; ++i) x[i] = xb[i];
            if (TARGET) {
                g.fast[b] = too_fast(x[7], x[8], x[9], g.t.v_max);
#pragma unroll
                for (int i = 0; i < 3; ++i) tg[i] = g.target[b * 3 + i];
                done = g.t.mode == 0 && g.target_no[b] >= (uint64_t)g.t.n_preset;
            }
            const double* ub = a.u + b * a.u_stride;
#pragma unroll
            for (int m = 0; m < QU; ++m) {
                const double raw = ub[m];
                if (a.u_out) a.u_out[b * QU + m] = raw;
                double w = raw < c.u_max ? raw : c.u_max;        // max(min(u, u_max), u_min)
                w = w > c.u_min ? w : c.u_min;
                if (!isfinite(raw)) { w = c.u_min; replaced = true; }
                act[m] = w;
            }
            if (!TARGET && a.tally) quad_tally(a, b, x, replaced);   // the error at the START of the step
            if (a.traj_pre) {
#pragma unroll
                for (int i = 0; i < QX; ++i) a.traj_pre[b * QX + i] = x[i];
            }
            if (TARGET && g.target_out) {
#pragma unroll
                for (int i = 0; i < 3; ++i) g.target_out[b * 3 + i] = tg[i];
            }
            // what does not change over the period: the deterministic thrusts, and the mean and the scale of a rotor's error (:190-191)
#pragma unroll
            for (int i = 0; i < QU; ++i) {
                f[i] = act[i] * c.max_thrust;
                if (NOISY) {
                    const double q = act[i] / mref;
                    mean[i] = mbias * (q * q);
                    scale[i] = mstd * sqrt(act[i]);
                }
            }
            th0 = quad_thrust(c, f);
        }
        for (int m0 = 0; m0 < a.p.substeps; m0 += C) {
            const int cnt = a.p.substeps - m0 < C ? a.p.substeps - m0 : C;
            if (NOISY) {
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
            }
            if (leader && !reached) {
                for (int m = 0; m < cnt; ++m) {
                    if (NOISY) {
                        const double* z = zs + m * NZ * V + v;   // normal k at z[k * V]
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
                    else quad_sim_update<false>(c, th0, x);
                    if (TARGET && !done && target_reached(tg, x, thresh)) { reached = true; nsub = m0 + m + 1; break; }
                }
            }
            if (NOISY) __syncthreads();
        }
        if (leader) {
#pragma unroll
            for (int i = 0; i < QX; ++i) xb[i] = x[i];
            if (!TARGET) noise_step[b] = p + 1;
            if (a.traj_post) {
#pragma unroll
                for (int i = 0; i < QX; ++i) a.traj_post[b * QX + i] = x[i];
            }
            if (!TARGET) {
                if (a.idx) {                                      // idx <- min(idx + 1, M - 1) where the vehicle has a window
                    const int k = a.traj_of[b];
                    if (k >= 0 && k < a.K) {
                        const int M = a.desc[k].M, i = a.idx[b];
                        if (i >= 0 && i < M) a.idx[b] = i + 1 < M ? i + 1 : M - 1;
                    }
                }
            }
            else {
                g.nsub[b] = nsub;
                if (g.nsub_out) g.nsub_out[b] = nsub;
                if (NOISY) noise_step[b] = p + 1;
                if (!done) {
                    int32_t* tc = g.tcounts + b * 5;
                    tc[2] = tc[2] + 1;
                    if (a.status && a.status[b] != 0) tc[3] = tc[3] + 1;
                    if (replaced) tc[4] = tc[4] + 1;
                    const int it = g.n_iter[b];
                    g.n_iter[b] = (reached ? 0 : it) + 1;
                    if (reached) {
                        tc[0] = tc[0] + 1;
                        const uint64_t no = g.target_no[b] + 1;
                        g.target_no[b] = no;
                        if (g.t.mode == 0) {
                            if (no < (uint64_t)g.t.n_preset) {
                                const double* pr = g.presets + (b * g.t.n_preset + (long long)no) * 3;
#pragma unroll
                                for (int i = 0; i < 3; ++i) g.target[b * 3 + i] = pr[i];
                            }
                        }
                        else {
                            const double pos[3] = { x[0], x[1], x[2] };
                            double nt[3];
                            uint64_t w[4];
                            target_sample(g.t, (uint32_t)b, no, pos, nt, w);
#pragma unroll
                            for (int i = 0; i < 3; ++i) g.target[b * 3 + i] = nt[i];
                        }
                    }
                }
            }
        }
    }
}

namespace {

template <bool NOISY, int L, bool TARGET>
void period_launch(const QuadPlantArgs& a, const QuadTargetArgs& g, const AdmpcQuadNoiseParams& n, uint64_t* noise_step, hipStream_t st)
{
    const int per = WAVE / L, nblk = (a.B + per - 1) / per;
    hipLaunchKernelGGL((admpc_quad_plant_period_kernel<NOISY, L, TARGET>), dim3((unsigned)(nblk < QP_GRID ? nblk : QP_GRID)), dim3(WAVE), 0, st, a, g, n, noise_step);
}

}  // namespace

extern "C" {

// The refusals of the plant parameters, for the entry points that take them (`who` leads the message).
int admpc_quad_plant_params_check(const char* who, const AdmpcQuadPlantParams* p)
{
    if (!p) return admpc_refuse(who, "the plant parameters are not set");
    if (!(p->dt > 0) || !isfinite(p->dt)) return admpc_refuse(who, "dt must be positive and finite");
    if (p->substeps < 1 || p->substeps > 1024) return admpc_refuse(who, "substeps must be in [1, 1024]");
    if (!(p->mass > 0) || !(p->J[0] > 0 && p->J[1] > 0 && p->J[2] > 0)) return admpc_refuse(who, "mass and J must be positive");
    if (!(p->u_min <= p->u_max) || !isfinite(p->u_min) || !isfinite(p->u_max)) return admpc_refuse(who, "u_min <= u_max, both finite, required");
    if (p->drag != 0 && p->drag != 1) return admpc_refuse(who, "drag must be 0 or 1");
    return ADMPC_OK;
}

// The arguments of a plant-only step; a period of a rollout sets its own pointers behind this.
void admpc_quad_plant_fill(QuadPlantArgs& a, const AdmpcQuadPlantParams* plant, int B, const double* u, long long u_stride, double* x)
{
    a.p = *plant; a.B = B; a.K = 0;
    a.u = u; a.u_stride = u_stride; a.x = x;
    a.yref = nullptr; a.yref_stride = 0; a.status = nullptr; a.tally = nullptr; a.counts = nullptr;
    a.traj_of = nullptr; a.idx = nullptr; a.desc = nullptr; a.traj_pre = a.traj_post = nullptr; a.u_out = nullptr;
}

// One launch of a plant kernel for filled arguments, B > 0, on the current device.  noise: null, or checked disturbances with the
// vehicles' period counters; g: null, or the target state.  A noisy fleet that does not fill the device by itself gets QN_LANES lanes a
// vehicle, for the draws; a larger one a lane a vehicle.
int admpc_quad_plant_launch(const QuadPlantArgs& a, const AdmpcQuadNoiseParams* noise, uint64_t* noise_step, const QuadTargetArgs* g, void* stream)
{
    const hipStream_t st = (hipStream_t)stream;
    const bool wide = a.B <= QN_WIDE_MAX;
    if (!noise && !g) {
        const int nblk = (a.B + WAVE - 1) / WAVE;
        hipLaunchKernelGGL(admpc_quad_plant_kernel, dim3((unsigned)(nblk < QP_GRID ? nblk : QP_GRID)), dim3(WAVE), 0, st, a);
    }
    else if (!noise) period_launch<false, 1, true>(a, *g, AdmpcQuadNoiseParams(), nullptr, st);
    else if (g) wide ? period_launch<true, QN_LANES, true>(a, *g, *noise, noise_step, st) : period_launch<true, 1, true>(a, *g, *noise, noise_step, st);
    else wide ? period_launch<true, QN_LANES, false>(a, QuadTargetArgs(), *noise, noise_step, st) : period_launch<true, 1, false>(a, QuadTargetArgs(), *noise, noise_step, st);
    if (hipGetLastError() != hipSuccess)
        return admpc_set_error(ADMPC_EHIP, noise || g ? "admpc_quad_plant_period_kernel: launch failed" : "admpc_quad_plant_kernel: launch failed");
    return ADMPC_OK;
}

int admpc_quad_plant_step_batch(const AdmpcQuadPlantParams* plant, int device, int B, const double* u, int64_t u_stride, double* x,
                                void* stream)
{
    const char* who = "admpc_quad_plant_step_batch";
    const int rc = admpc_quad_plant_params_check(who, plant);
    if (rc) return rc;
    if (B < 0) return admpc_refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!u || !x) return admpc_refuse(who, "null array argument");
    if (u_stride < QU) return admpc_refuse(who, "u_stride must be at least 4");
    if (admpc_device_check(device)) return ADMPC_ENODEV;
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    QuadPlantArgs a;
    admpc_quad_plant_fill(a, plant, B, u, (long long)u_stride, x);
    return admpc_quad_plant_launch(a, nullptr, nullptr, nullptr, stream);
}

int admpc_quad_plant_step_noise_batch(const AdmpcQuadPlantParams* plant, const AdmpcQuadNoiseParams* noise, int device, int B,
                                      const double* u, int64_t u_stride, double* x, uint64_t* noise_step, void* stream)
{
    const char* who = "admpc_quad_plant_step_noise_batch";
    int rc = admpc_quad_plant_params_check(who, plant);
    if (!rc) rc = admpc_quad_noise_params_check(who, noise, plant);
    if (rc) return rc;
    if (B < 0) return admpc_refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!u || !x) return admpc_refuse(who, "null array argument");
    if (u_stride < QU) return admpc_refuse(who, "u_stride must be at least 4");
    if (!noise_step) return admpc_refuse(who, "null noise_step");
    if (admpc_device_check(device)) return ADMPC_ENODEV;
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    QuadPlantArgs a;
    admpc_quad_plant_fill(a, plant, B, u, (long long)u_stride, x);
    return admpc_quad_plant_launch(a, noise, noise_step, nullptr, stream);
}

int admpc_quad_plant_target_step_batch(const AdmpcQuadPlantParams* plant, const AdmpcQuadTargetParams* tp, const AdmpcQuadNoiseParams* noise,
                                       int device, int B, const double* u, int64_t u_stride, double* x, const int32_t* status,
                                       const double* presets, double* target, uint64_t* target_no, int32_t* n_iter, int32_t* fast,
                                       int32_t* tcounts, int32_t* nsub, uint64_t* noise_step, void* stream)
{
    const char* who = "admpc_quad_plant_target_step_batch";
    int rc = admpc_quad_plant_params_check(who, plant);
    if (!rc) rc = admpc_quad_target_params_check(who, tp);
    if (!rc && noise) rc = admpc_quad_noise_params_check(who, noise, plant);
    if (rc) return rc;
    if (B < 0) return admpc_refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!u || !x || !target || !target_no || !n_iter || !fast || !tcounts || !nsub) return admpc_refuse(who, "null array argument");
    if (u_stride < QU) return admpc_refuse(who, "u_stride must be at least 4");
    if (tp->mode == 0 && !presets) return admpc_refuse(who, "mode 0 needs the presets");
    if (noise && !noise_step) return admpc_refuse(who, "null noise_step");
    if (admpc_device_check(device)) return ADMPC_ENODEV;
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    QuadPlantArgs a;
    admpc_quad_plant_fill(a, plant, B, u, (long long)u_stride, x);
    a.status = status;
    const QuadTargetArgs g = { *tp, presets, target, target_no, n_iter, fast, tcounts, nsub, nullptr, nullptr };
    return admpc_quad_plant_launch(a, noise, noise_step, &g, stream);
}

}  // extern "C"
