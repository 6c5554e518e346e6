// quad_target_dev.h -- the targets of include/admpc_quad_targets.h as device text, for admpc_quad_plant.hip (the reach test behind every
// sub-step and the next target, in the plant kernel's launch) and admpc_quad_targets.hip (the window, the draw for the host, the reset):
// the target state of a launch, the uniforms and the sample of a target, the speed test and the reach test.  Include behind
// quad_noise_dev.h, whose generator the uniforms call at the far end of the fourth counter word; every function is static and
// __forceinline__, so each unit has its own copy.
#pragma once
#include <stdint.h>
#include "../../include/admpc_quad_targets.h"

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

// the words of calls 0 and 1 of (vehicle b, target number t) and the three uniforms of include/admpc_quad_targets.h
static __device__ __forceinline__ void target_uniforms(uint64_t seed, uint32_t b, uint64_t t, uint64_t (&w)[4], double (&u)[3])
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
static __device__ __forceinline__ void target_sample(const AdmpcQuadTargetParams& t, uint32_t b, uint64_t no, const double (&p)[3], double (&tg)[3], uint64_t (&w)[4])
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
static __device__ __forceinline__ int too_fast(const double v0, const double v1, const double v2, const double v_max)
{
    return (v0 > v_max || v1 > v_max || v2 > v_max) ? 1 : 0;
}

// whether the target t is reached from x
static __device__ __forceinline__ bool target_reached(const double (&t)[3], const double (&x)[ADMPC_QUAD_NX], const double thresh)
{
#pragma clang fp contract(off)
    const double e0 = t[0] - x[0], e1 = t[1] - x[1], e2 = t[2] - x[2];
    const double d = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    return d < thresh;
}
