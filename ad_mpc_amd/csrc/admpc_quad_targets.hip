// admpc_quad_targets.hip -- flying to random target points and recording, on the device (include/admpc_quad_targets.h): four kernels and
// their host side.
//
//   admpc_quad_target_window_kernel  the recovery of a vehicle that has run away and the point reference of every vehicle, one lane per
//                                    vehicle as the plant kernel maps it, the same grid cap and stride loop
//   admpc_quad_plant_target_kernel   admpc_quad_plant_kernel (NOISY: admpc_quad_plant_noise_kernel) with the reach test behind every
//                                    sub-step, and in the same launch the next target, the counters and `fast`.  The deterministic form
//                                    is one lane per vehicle without LDS; the noisy form has the noisy plant kernel's mapping (L lanes a
//                                    vehicle share out the draws of a chunk through LDS, lane 0 integrates), and a vehicle that has
//                                    reached keeps meeting the barriers and only skips the integration
//   admpc_quad_observe_var_kernel    admpc_quad_observe_kernel (admpc_quad_learn.hip) with a period per vehicle
//   admpc_quad_target_draw_kernel    the target a number gives a vehicle, for the host, through the device function the plant uses
//
// The simulator's device text is quad_sim_dev.h, the generator's quad_noise_dev.h, the prediction's quad_observe_dev.h.  The bodies
// around the sub-steps are repeated from the two plant kernels and not shared with them: their instruction streams are held unchanged
// (admpc_quad_noise.hip says why).
#include <stdio.h>
#include <math.h>
#include "admpc_host.h"
#include "../../include/admpc_quad_targets.h"
#include "quad_sim_dev.h"

#define NX ADMPC_NX           // model_dev.h wants the car's dimensions defined
#define NU ADMPC_NU
#define NY ADMPC_NY
#define WAVE 64
#define QP_GRID 4096           // blocks at most, as admpc_quad_plant_kernel's; more vehicles go round the stride loop
#define NZ 10                  // normals per (vehicle, sub-step)
#define QN_LANES 4             // admpc_quad_noise.hip's mapping, threshold and LDS budget: by kernel trace at B = 4096, over the periods of N = 10 and
#ifndef QN_WIDE_MAX            // N = 20, the noisy kernel takes 120.3 us with four lanes a vehicle and 186.1 us with one (-DQN_WIDE_MAX=0; profiles/HISTORY.md)
#define QN_WIDE_MAX 8192
#endif
#define QN_LDS_DOUBLES 1600
#define QREC 14                // doubles per sample record (admpc_quad_learn.hip)

static_assert(sizeof(AdmpcQuadTargetParams) == 48, "the layout the Python side mirrors");

// the target state of a launch and the records of a rollout's period (null outside one)
struct QuadTargetArgs {
    AdmpcQuadTargetParams t;
    const double* presets;                    // [B][n_preset][3], mode 0
    double* target;                           // [B][3]
    uint64_t* target_no;                      // [B]
    int32_t *n_iter, *fast, *tcounts, *nsub;  // [B], [B], [B][5], [B]
    int32_t* nsub_out;                        // [B] slot, or null
    double* target_out;                       // [B][3] slot, or null
};

// what one launch of the observe kernel with a period per vehicle works on
struct QuadObserveVarArgs {
    double dt, plant_dt, u_min, u_max;
    int M, B, plant_substeps;
    const double* u; long long u_stride;
    const double* x;
    double* prev;
    const int32_t* nsub;
    double* samples;
};

namespace {

#include "model_dev.h"

constexpr int QX = ADMPC_QUAD_NX, QU = ADMPC_QUAD_NU, QY = ADMPC_QUAD_NY;
typedef AdmpcQuadConfig Cfg;

#include "quad_model_dev.h"
#include "quad_observe_dev.h"
#include "quad_noise_dev.h"

// the words of calls 0 and 1 of (vehicle b, target number t) and the three uniforms of include/admpc_quad_targets.h
__device__ __forceinline__ void target_uniforms(uint64_t seed, uint32_t b, uint64_t t, uint64_t (&w)[4], double (&u)[3])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        uint32_t o[4];
        philox4x32_10(b, (uint32_t)t, (uint32_t)(t >> 32), 0xffffffffu - (uint32_t)j, (uint32_t)seed, (uint32_t)(seed >> 32), o);
        w[2 * j] = (uint64_t)o[0] | (uint64_t)o[1] << 32;
        w[2 * j + 1] = (uint64_t)o[2] | (uint64_t)o[3] << 32;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = ((double)(w[k] >> 11) + 0.5) * 0x1p-53;
}

// target number t of vehicle b at position p, modes 1 and 2: every operation rounded on its own
__device__ __forceinline__ void target_sample(const AdmpcQuadTargetParams& t, uint32_t b, uint64_t no, const double (&p)[3], double (&tg)[3], uint64_t (&w)[4])
{
#pragma clang fp contract(off)
    double u[3];
    target_uniforms(t.seed, b, no, w, u);
    const double R = t.world_radius;
    if (t.mode == 1) {
        const double th = 6.283185307179586 * u[0], ps = 6.283185307179586 * u[1];
        const double r = R + (u[2] - 0.5) * R;
        const double rs = r * sin(th);
        tg[0] = p[0] + rs * cos(ps); tg[1] = p[1] + rs * sin(ps); tg[2] = p[2] + r * cos(th);
    }
    else {
        const double R2 = 2.0 * R;
#pragma unroll
        for (int k = 0; k < 3; ++k) tg[k] = -R + R2 * u[k];
    }
}

// 1 iff a velocity component of x is above v_max: signed, and a NaN compares false
__device__ __forceinline__ int too_fast(const double v0, const double v1, const double v2, const double v_max)
{
    return (v0 > v_max || v1 > v_max || v2 > v_max) ? 1 : 0;
}

// whether the target t is reached from x
__device__ __forceinline__ bool target_reached(const double (&t)[3], const double (&x)[QX], const double thresh)
{
#pragma clang fp contract(off)
    const double e0 = t[0] - x[0], e1 = t[1] - x[1], e2 = t[2] - x[2];
    const double d = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    return d < thresh;
}

}  // namespace

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

// L lanes of a wave per vehicle, V = 64 / L vehicles per block; NOISY == false: L == 1, no LDS, no barrier, one chunk.
template <bool NOISY, int L>
__global__ __launch_bounds__(WAVE) void admpc_quad_plant_target_kernel(const QuadPlantArgs a, const QuadTargetArgs g, const AdmpcQuadNoiseParams n,
                                                                       uint64_t* __restrict__ noise_step)
{
    constexpr int V = WAVE / L, C = NOISY ? QN_LDS_DOUBLES / (V * NZ) : 1024;
    static_assert(WAVE % L == 0 && C >= 1 && (NOISY || L == 1), "whole vehicles per wave, at least one sub-step per chunk");
    __shared__ double zs[NOISY ? C * NZ * V : 1];
    const SimConst c = sim_const(a.p);
    double fstd = 0, tstd = 0, mbias = 0, mref = 1, mstd = 0;
    if (NOISY) { fstd = vreg(n.force_std); tstd = vreg(n.torque_std); mbias = vreg(n.motor_bias); mref = vreg(n.motor_ref); mstd = vreg(n.motor_std); }
    const double thresh = vreg(g.t.thresh);
    const int v = (int)threadIdx.x / L, l = (int)threadIdx.x % L;
    const int j_lo = n.motor_noise ? 0 : 2, nj = (n.noisy ? 5 : 2) - j_lo;
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
            g.fast[b] = too_fast(x[7], x[8], x[9], g.t.v_max);
#pragma unroll
            for (int i = 0; i < 3; ++i) tg[i] = g.target[b * 3 + i];
            done = g.t.mode == 0 && g.target_no[b] >= (uint64_t)g.t.n_preset;
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
            if (a.traj_pre) {
#pragma unroll
                for (int i = 0; i < QX; ++i) a.traj_pre[b * QX + i] = x[i];
            }
            if (g.target_out) {
#pragma unroll
                for (int i = 0; i < 3; ++i) g.target_out[b * 3 + i] = tg[i];
            }
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
                    if (!done && target_reached(tg, x, thresh)) { reached = true; nsub = m0 + m + 1; break; }
                }
            }
            if (NOISY) __syncthreads();
        }
        if (leader) {
#pragma unroll
            for (int i = 0; i < QX; ++i) xb[i] = x[i];
            if (a.traj_post) {
#pragma unroll
                for (int i = 0; i < QX; ++i) a.traj_post[b * QX + i] = x[i];
            }
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

__global__ __launch_bounds__(WAVE) void admpc_quad_observe_var_kernel(const AdmpcQuadConfig* __restrict__ cfg, const QuadObserveVarArgs a)
{
    for (long long b = (long long)blockIdx.x * WAVE + threadIdx.x; b < a.B; b += (long long)gridDim.x * WAVE) {
        double xh[QX], now[QX], act[QU];
        double* pb = a.prev + b * QX;
        const double* xb = a.x + b * QX;
        const double* ub = a.u + b * a.u_stride;
        const int ns = a.nsub[b];
        const double dt = ns == a.plant_substeps ? a.dt : (double)ns * a.plant_dt;      // the period this vehicle flew
        const double h = dt / (double)a.M;
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

namespace {

int refuse(const char* who, const char* what)
{
    char msg[220];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return admpc_set_error(ADMPC_EINVAL, msg);
}

// the refusals of the target parameters, in the header's order
int target_params_check(const char* who, const AdmpcQuadTargetParams* t)
{
    if (!t) return refuse(who, "the target parameters are not set");
    if (t->mode < 0 || t->mode > 2) return refuse(who, "mode must be 0 (presets), 1 (aggressive) or 2 (uniform)");
    if (!(t->world_radius > 0) || !isfinite(t->world_radius)) return refuse(who, "world_radius must be positive and finite");
    if (!(t->thresh > 0) || !isfinite(t->thresh)) return refuse(who, "thresh must be positive and finite");
    if (t->v_max != t->v_max) return refuse(who, "v_max must not be NaN");
    if (t->max_iters < 0) return refuse(who, "max_iters must not be negative");
    if (t->mode == 0 && t->n_preset < 1) return refuse(who, "mode 0 needs n_preset >= 1");
    return ADMPC_OK;
}

int grid_of(int B)
{
    const int nblk = (B + WAVE - 1) / WAVE;
    return nblk < QP_GRID ? nblk : QP_GRID;
}

int device_check(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return admpc_set_error(ADMPC_ENODEV, "no such device");
    return ADMPC_OK;
}

int window_launch(const AdmpcQuadTargetParams* tp, int B, int N, double* x, const double* target, const uint64_t* target_no, int32_t* n_iter,
                  const int32_t* fast, int32_t* tcounts, double* prev, double* yref, double* yref_e, void* stream)
{
    hipLaunchKernelGGL(admpc_quad_target_window_kernel, dim3((unsigned)grid_of(B)), dim3(WAVE), 0, (hipStream_t)stream, *tp, B, N, x, target, target_no,
                       n_iter, fast, tcounts, prev, yref, yref_e);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_target_window_kernel: launch failed");
    return ADMPC_OK;
}

// one launch of the plant-target kernel for filled arguments, B > 0; noise: null (deterministic) or checked disturbances
int plant_target_launch(const QuadPlantArgs& a, const QuadTargetArgs& g, const AdmpcQuadNoiseParams* noise, uint64_t* noise_step, void* stream)
{
    static_assert(QN_WIDE_MAX / (WAVE / QN_LANES) <= QP_GRID, "the wide mapping stays within the grid cap");
    const hipStream_t st = (hipStream_t)stream;
    if (!noise) {
        const AdmpcQuadNoiseParams none = AdmpcQuadNoiseParams();
        hipLaunchKernelGGL((admpc_quad_plant_target_kernel<false, 1>), dim3((unsigned)grid_of(a.B)), dim3(WAVE), 0, st, a, g, none, nullptr);
    }
    else if (a.B <= QN_WIDE_MAX) {
        const int per = WAVE / QN_LANES, nblk = (a.B + per - 1) / per;
        hipLaunchKernelGGL((admpc_quad_plant_target_kernel<true, QN_LANES>), dim3((unsigned)(nblk < QP_GRID ? nblk : QP_GRID)), dim3(WAVE), 0, st, a, g, *noise, noise_step);
    }
    else hipLaunchKernelGGL((admpc_quad_plant_target_kernel<true, 1>), dim3((unsigned)grid_of(a.B)), dim3(WAVE), 0, st, a, g, *noise, noise_step);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_plant_target_kernel: launch failed");
    return ADMPC_OK;
}

QuadPlantArgs plant_args(const AdmpcQuadPlantParams* plant, int B, const double* u, long long u_stride, double* x, const int32_t* status)
{
    QuadPlantArgs a;
    a.p = *plant; a.B = B; a.K = 0;
    a.u = u; a.u_stride = u_stride; a.x = x;
    a.yref = nullptr; a.yref_stride = 0; a.status = status; a.tally = nullptr; a.counts = nullptr;
    a.traj_of = nullptr; a.idx = nullptr; a.desc = nullptr; a.traj_pre = a.traj_post = nullptr; a.u_out = nullptr;
    return a;
}

int observe_var_launch(const AdmpcQuadSolver* model, const AdmpcQuadPlantParams* plant, const AdmpcQuadObserveParams* obs, int B, const double* u,
                       long long u_stride, const double* x, double* prev, const int32_t* nsub, double* samples, double* bins, int32_t* dropped,
                       void* stream)
{
    QuadObserveVarArgs a;
    a.dt = obs->dt; a.plant_dt = plant->dt; a.u_min = plant->u_min; a.u_max = plant->u_max;
    a.M = obs->substeps; a.B = B; a.plant_substeps = plant->substeps;
    a.u = u; a.u_stride = u_stride; a.x = x; a.prev = prev; a.nsub = nsub; a.samples = samples;
    hipLaunchKernelGGL(admpc_quad_observe_var_kernel, dim3((unsigned)grid_of(B)), dim3(WAVE), 0, (hipStream_t)stream,
                       admpc_quad_solver_config_device(model, nullptr), a);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_observe_var_kernel: launch failed");
    return admpc_quad_bin_launch(obs, B, samples, bins, dropped, stream);
}

}  // namespace

extern "C" {

int admpc_quad_target_draw_batch(const AdmpcQuadTargetParams* tp, int device, int B, const double* x, int64_t x_stride,
                                 const uint64_t* target_no, double* target_out, uint64_t* raw, void* stream)
{
    const char* who = "admpc_quad_target_draw_batch";
    const int rc = target_params_check(who, tp);
    if (rc) return rc;
    if (tp->mode == 0) return refuse(who, "mode 0: the presets are not drawn");
    if (B < 0) return refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!x || !target_no || !target_out) return refuse(who, "null array argument");
    if (x_stride < 3) return refuse(who, "x_stride must be at least 3");
    if (device_check(device)) return ADMPC_ENODEV;
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
    const int rc = target_params_check(who, tp);
    if (rc) return rc;
    if (B < 0) return refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!x || !target || !target_no || !n_iter || !fast || !tcounts) return refuse(who, "null array argument");
    if (tp->mode == 0 && !presets) return refuse(who, "mode 0 needs the presets");
    if (device_check(device)) return ADMPC_ENODEV;
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
    const int rc = target_params_check(who, tp);
    if (rc) return rc;
    if (B < 0) return refuse(who, "negative batch");
    if (N < 2 || N > ADMPC_QUAD_MAX_N) return refuse(who, "N must be in [2, 24]");
    if (B == 0) return ADMPC_OK;
    if (!x || !target || !n_iter || !fast || !tcounts || !yref || !yref_e) return refuse(who, "null array argument");
    if (tp->mode == 0 && !target_no) return refuse(who, "mode 0 needs target_no");
    if (device_check(device)) return ADMPC_ENODEV;
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    return window_launch(tp, B, N, x, target, target_no, n_iter, fast, tcounts, prev, yref, yref_e, stream);
}

int admpc_quad_plant_target_step_batch(const AdmpcQuadPlantParams* plant, const AdmpcQuadTargetParams* tp, const AdmpcQuadNoiseParams* noise,
                                       int device, int B, const double* u, int64_t u_stride, double* x, const int32_t* status,
                                       const double* presets, double* target, uint64_t* target_no, int32_t* n_iter, int32_t* fast,
                                       int32_t* tcounts, int32_t* nsub, uint64_t* noise_step, void* stream)
{
    const char* who = "admpc_quad_plant_target_step_batch";
    int rc = admpc_quad_plant_params_check(who, plant);
    if (!rc) rc = target_params_check(who, tp);
    if (!rc && noise) rc = admpc_quad_noise_params_check(who, noise, plant);
    if (rc) return rc;
    if (B < 0) return refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!u || !x || !target || !target_no || !n_iter || !fast || !tcounts || !nsub) return refuse(who, "null array argument");
    if (u_stride < QU) return refuse(who, "u_stride must be at least 4");
    if (tp->mode == 0 && !presets) return refuse(who, "mode 0 needs the presets");
    if (noise && !noise_step) return refuse(who, "null noise_step");
    if (device_check(device)) return ADMPC_ENODEV;
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    const QuadTargetArgs g = { *tp, presets, target, target_no, n_iter, fast, tcounts, nsub, nullptr, nullptr };
    return plant_target_launch(plant_args(plant, B, u, (long long)u_stride, x, status), g, noise, noise_step, stream);
}

int admpc_quad_observe_var_batch(const AdmpcQuadSolver* model, const AdmpcQuadPlantParams* plant, const AdmpcQuadObserveParams* obs, int B,
                                 const double* u, int64_t u_stride, const double* x, double* prev, const int32_t* nsub, double* samples,
                                 double* bins, int32_t* dropped, void* stream)
{
    const char* who = "admpc_quad_observe_var_batch";
    int rc = admpc_quad_observe_params_check(who, obs);
    if (rc) return rc;
    rc = admpc_quad_plant_params_check(who, plant);
    if (rc) return rc;
    if (!model) return refuse(who, "null model");
    if (B < 0) return refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!u || !x || !prev || !nsub || !samples || !bins || !dropped) return refuse(who, "null array argument");
    if (u_stride < QU) return refuse(who, "u_stride must be at least 4");
    int device = 0;
    (void)admpc_quad_solver_info(model, &device, nullptr, nullptr);
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    return observe_var_launch(model, plant, obs, B, u, (long long)u_stride, x, prev, nsub, samples, bins, dropped, stream);
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
    if (!rc) rc = target_params_check(who, tp);
    if (!rc && noise) rc = admpc_quad_noise_params_check(who, noise, plant);
    if (!rc && model) rc = admpc_quad_observe_params_check(who, obs);
    if (rc) return rc;
    if (!s) return refuse(who, "null solver");
    int device = 0, N = 0, sqp = 0;
    (void)admpc_quad_solver_info(s, &device, &N, &sqp);
    if (sqp > 1) return refuse(who, "a solver in SQP mode (sqp_iters > 1) is not served: the rollout is the RTI loop");
    if (B < 0) return refuse(who, "negative batch");
    if (T < 0 || T > 4096) return refuse(who, "T must be in [0, 4096]");
    if (model) {
        int model_device = 0;
        (void)admpc_quad_solver_info(model, &model_device, nullptr, nullptr);
        if (model_device != device) return refuse(who, "the model lives on another device than the solver");
    }
    if (B == 0 || T == 0) return ADMPC_OK;
    if (!x || !xbar || !ubar || !yref || !yref_e || !status || !target || !target_no || !n_iter || !fast || !tcounts || !nsub ||
        (model && (!prev || !samples || !bins || !dropped)))
        return refuse(who, "null array argument");
    if (tp->mode == 0 && !presets) return refuse(who, "mode 0 needs the presets");
    if (noise && !noise_step) return refuse(who, "null noise_step");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    if (model) rc = admpc_quad_latch_launch(B, x, prev, stream);
    const size_t slot = (size_t)B * QX;
    for (int t = 0; t < T && !rc; ++t) {
        rc = window_launch(tp, B, N, x, target, target_no, n_iter, fast, tcounts, model ? prev : nullptr, yref, yref_e, stream);
        if (!rc) rc = admpc_quad_solve_batch_ex(s, B, x, yref, yref_e, nullptr, xbar, ubar, cost, status, iters, stream);
        if (rc) break;
        QuadPlantArgs a = plant_args(plant, B, ubar, (long long)N * QU, x, status);
        a.traj_pre = t == 0 ? traj_out : nullptr;
        a.traj_post = traj_out ? traj_out + (size_t)(t + 1) * slot : nullptr;
        a.u_out = u_out ? u_out + (size_t)t * B * QU : nullptr;
        const QuadTargetArgs g = { *tp, presets, target, target_no, n_iter, fast, tcounts, nsub, nsub_out ? nsub_out + (size_t)t * B : nullptr,
                                   target_out ? target_out + (size_t)t * B * 3 : nullptr };
        rc = plant_target_launch(a, g, noise, noise_step, stream);
        if (!rc && model) rc = observe_var_launch(model, plant, obs, B, ubar, (long long)N * QU, x, prev, nsub, samples, bins, dropped, stream);
    }
    return rc;
}

}  // extern "C"
