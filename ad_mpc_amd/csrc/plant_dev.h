// plant_dev.h -- device code shared by the plant step (admpc_plant.hip) and the observation of a step (admpc_learn.hip): the state part
// of one RK4 step of the model, and the blend parameter of a speed band.  Both kernels must integrate the same way: the residual the
// observation forms is zero, to rounding, where the plant is the model.
// Include INSIDE the translation unit's anonymous namespace, after model_dev.h; every function is __forceinline__.
#pragma once

// The state part of rk4_group: the same stages, weights and model_eval, without the sensitivity columns the plant would throw away.
__device__ __forceinline__ void rk4_state(const AdmpcConfig* __restrict__ c, const double* x, const double* u, double p, double h, double* phi)
{
    double kx[NX], accx[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) { kx[i] = 0.0; accx[i] = 0.0; }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const double cs = (s == 0) ? 0.0 : (s == 3 ? 1.0 : 0.5);
        const double ws = (s == 0 || s == 3) ? (1.0 / 6.0) : (2.0 / 6.0);
        double X[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) X[i] = x[i] + cs * h * kx[i];
        ModelEvalT<double> e;
        model_eval<double>(c, X, u, p, e);
#pragma unroll
        for (int i = 0; i < NX; ++i) { kx[i] = e.f[i]; accx[i] += ws * e.f[i]; }
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) phi[i] = x[i] + h * accx[i];
}

// host.vel_switch (ad_3d_optimizer.py:443) on the plant's band, NaN kept as numpy keeps it
__device__ __forceinline__ double plant_blend(double vx, double blend_min, double blend_max)
{
#pragma clang fp contract(off)
    double q = (vx - blend_min) / (blend_max - blend_min);
    if (q < 0.0) q = 0.0;
    if (q > 1.0) q = 1.0;
    return q;
}
