// quad_observe_dev.h -- what the observe kernel of admpc_quad_learn.hip is made of: the model's prediction of a flown period and the
// body-frame map.  Include INSIDE the translation unit's
// anonymous namespace, behind quad_model_dev.h; every function is __forceinline__.
#pragma once

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
