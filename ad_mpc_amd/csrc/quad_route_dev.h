// quad_route_dev.h -- the cluster of a quadrotor instance, shared by admpc_quad_select_cluster_kernel (admpc_quad.hip) and the kernels of
// the clustered ensemble in the closed loop (admpc_quad_ensemble.hip): nearest centroid in the selected features of
// z = [x with the velocity in the BODY frame; u], Euclidean distance, ties to the lower index, a feature that is not finite -> cluster 0
// (numpy.argmin over distances that are then NaN or all infinite; gp.py:738-770 select_gp).  Include INSIDE the translation unit's
// anonymous namespace behind quad_model_dev.h (quad_rot); every function is __forceinline__.
#pragma once

// the centroid (cent [K][d]) nearest to the d features z
__device__ __forceinline__ int quad_nearest(const double (&z)[3], const int d, const int K, const double* __restrict__ cent)
{
    double best = INFINITY; int bi = 0;
    for (int c = 0; c < K; ++c) {
        double acc = 0.0;
        for (int j = 0; j < d; ++j) { const double e = z[j] - cent[c * d + j]; acc = acc + e * e; }
        const double dist = __dsqrt_rn(acc);
        if (dist < best) { best = dist; bi = c; }
    }
    return bi;
}

// the cluster of the state x [13] (world-frame velocity: the rotation by x's own quaternion happens here) and the input u [4]; the two
// may be the halves of one row of a reference window
__device__ __forceinline__ int quad_route_row(const double* __restrict__ x, const double* __restrict__ u, const int d, const int f0, const int f1,
                                              const int f2, const int K, const double* __restrict__ cent)
{
    double R[3][3];
    quad_rot(x[3], x[4], x[5], x[6], R);
    double zz[ADMPC_QUAD_NY];
#pragma unroll
    for (int i = 0; i < ADMPC_QUAD_NX; ++i) zz[i] = x[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) zz[7 + i] = R[0][i] * x[7] + R[1][i] * x[8] + R[2][i] * x[9];        // v_b = R' v
#pragma unroll
    for (int m = 0; m < ADMPC_QUAD_NU; ++m) zz[ADMPC_QUAD_NX + m] = u[m];
    const int f[3] = { f0, f1, f2 };
    double z[3] = { 0, 0, 0 };
    for (int j = 0; j < d; ++j) {
        double v = 0;
#pragma unroll
        for (int i = 0; i < ADMPC_QUAD_NY; ++i) v = f[j] == i ? zz[i] : v;
        z[j] = v;
    }
    return quad_nearest(z, d, K, cent);
}
