// quad_traj_tail_dev.h -- what the two trajectory generators share on the device (admpc_quad_traj.hip: loop and lemniscate;
// admpc_quad_poly_traj.hip: piecewise polynomials through keyframes): the vehicle's block of arguments, the quaternion helpers, the scan of
// a tile, and ONE text of steps 5 .. 9 of the rule of include/admpc_quad_traj.h, the passes B, C and D of its MAPPING.  A kernel runs its
// own pass A (the rows (pos, q, vel, 0) and (0, 0, 0, f_t) of a trajectory written, a barrier behind the last tile) and then calls
// quad_traj_tail with every lane of the group.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/admpc_quad.h"

#define QX ADMPC_QUAD_NX
#define QU ADMPC_QUAD_NU
#define QT_THREADS 256
#define QT_WAVES (QT_THREADS / 64)
#define QT_GRID 512            // work-groups of a generator at most: trajectories past it are served by the stride loop
#define QT_ROW (QX + QU)       // doubles a row stages in LDS
#define QT_GRAVITY 9.81        // trajectories.py:154, not the plant's g

// what a generator reads of the vehicle, by pointer (a copy in the bank's allocation: by value it costs scalar-register spills); ainv is the inverse of [y_f; -x_f; z_l_tau; 1 1 1 1], row-major
struct QuadTrajGenArgs {
    double dt, mass, J[3], max_thrust, ainv[16];
};

namespace {

// q_dot_q of utils.py:341: q rotated by r
__device__ inline void qmul(const double q[4], const double r[4], double t[4])
{
    t[0] = r[0] * q[0] - r[1] * q[1] - r[2] * q[2] - r[3] * q[3];
    t[1] = r[0] * q[1] + r[1] * q[0] - r[2] * q[3] + r[3] * q[2];
    t[2] = r[0] * q[2] + r[1] * q[3] + r[2] * q[0] - r[3] * q[1];
    t[3] = r[0] * q[3] - r[1] * q[2] + r[2] * q[1] + r[3] * q[0];
}

// 2 * (conj(q) (x) ((hi - lo) / div / dt))[1:4]: the body rate of q from a difference of its neighbours (div 2: central, 1: one-sided)
__device__ inline void body_rate(const double q[4], const double lo[4], const double hi[4], double div, double dt, double w[3])
{
    const double qi[4] = { q[0], -q[1], -q[2], -q[3] };
    double d[4], t[4];
    for (int c = 0; c < 4; ++c) d[c] = (hi[c] - lo[c]) / div / dt;
    qmul(qi, d, t);
    w[0] = 2.0 * t[1]; w[1] = 2.0 * t[2]; w[2] = 2.0 * t[3];
}

// the inclusive scan of one tile with its carry (include/admpc_quad_traj.h, THE SCAN): every lane of the group calls it
__device__ inline double tile_scan(double v, double* s_tot, double* s_carry)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double carry = *s_carry;
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(v, d);
        if (lane >= d) v = o + v;
    }
    if (lane == 63) s_tot[wave] = v;
    __syncthreads();                              // the waves' totals are in LDS; every lane has read the carry
    double r = v;
    if (wave > 0) {
        double before = s_tot[0];
        for (int m = 1; m < wave; ++m) before += s_tot[m];
        r = before + v;
    }
    const double out = carry + r;
    if (threadIdx.x == QT_THREADS - 1) *s_carry = out;
    __syncthreads();                              // the carry of the next tile is in LDS; s_tot may be written again
    return out;
}

// qn of row i from its q and its yaw (step 6)
__device__ inline void corrected(int i, const double q[4], double yaw, double qn[4])
{
    if (i == 0) { for (int c = 0; c < 4; ++c) qn[c] = q[c]; return; }
    const double r[4] = { cos(yaw / 2.0), 0.0, 0.0, sin(yaw / 2.0) };
    qmul(q, r, qn);
}

__device__ inline void load4(const double* p, double v[4]) { v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3]; }

// Passes B, C and D over the M rows of one trajectory at Xk / Uk, whose pass A is complete: q in X[.][3:7], f_t in U[.][3], and a barrier
// behind the last write.  s_row [QT_THREADS * QT_ROW], s_tot [QT_WAVES] and s_carry [1 at least] are the group's LDS.  It ends with the
// barrier behind the last tile's rows: LDS may be written again.
__device__ __forceinline__ void quad_traj_tail(int M, double dt, const QuadTrajGenArgs* gp, double* Xk, double* Uk, double* s_row, double* s_tot,
                                               double* s_carry)
{
    const int tid = threadIdx.x;
    const int tiles = (M + QT_THREADS - 1) / QT_THREADS;

    // ---- pass B: the first body rates, the yaw correction accumulated -----------------------------------------------------------
    if (tid == 0) s_carry[0] = 0.0;
    __syncthreads();
    for (int tile = 0; tile < tiles; ++tile) {
        const int i = tile * QT_THREADS + tid;
        double term = 0.0;
        if (i > 0 && i < M) {
            double q[4], lo[4], hi[4], w0[3];
            load4(Xk + (size_t)i * QX + 3, q);
            load4(Xk + (size_t)(i - 1) * QX + 3, lo);
            if (i < M - 1) load4(Xk + (size_t)(i + 1) * QX + 3, hi); else load4(Xk + (size_t)i * QX + 3, hi);
            body_rate(q, lo, hi, i < M - 1 ? 2.0 : 1.0, dt, w0);
            term = -w0[2] * dt;
        }
        const double yaw = tile_scan(term, s_tot, &s_carry[0]);
        if (i < M) Uk[(size_t)i * QU] = yaw;
    }
    __syncthreads();                              // yaw of every row is visible

    // ---- pass C: the body rates of the corrected attitude ------------------------------------------------------------------------
    for (int tile = 0; tile < tiles; ++tile) {
        const int i = tile * QT_THREADS + tid;
        if (i < M) {
            double q[4], lo[4], hi[4], qn[4], w[3];
            load4(Xk + (size_t)i * QX + 3, q);
            if (i == 0) {                         // the first pass' rate of row 0, from the uncorrected q[0] and q[1]
                load4(Xk + (size_t)QX + 3, hi);
                body_rate(q, q, hi, 1.0, dt, w);
            }
            else {
                double t[4];
                corrected(i, q, Uk[(size_t)i * QU], qn);
                load4(Xk + (size_t)(i - 1) * QX + 3, t);
                corrected(i - 1, t, Uk[(size_t)(i - 1) * QU], lo);
                if (i < M - 1) { load4(Xk + (size_t)(i + 1) * QX + 3, t); corrected(i + 1, t, Uk[(size_t)(i + 1) * QU], hi); }
                else for (int c = 0; c < 4; ++c) hi[c] = qn[c];
                body_rate(qn, lo, hi, i < M - 1 ? 2.0 : 1.0, dt, w);
            }
            Xk[(size_t)i * QX + 10] = w[0]; Xk[(size_t)i * QX + 11] = w[1]; Xk[(size_t)i * QX + 12] = w[2];
        }
    }
    __syncthreads();                              // the rate of every row is visible

    // ---- pass D: the inputs, the final rows -------------------------------------------------------------------------------------
    const double px0 = Xk[0], py0 = Xk[1];        // read by every lane in front of the barrier that precedes the first write
    for (int tile = 0; tile < tiles; ++tile) {
        const int i = tile * QT_THREADS + tid;
        double* row = s_row + tid * QT_ROW;
        if (i < M) {
            const double* xi = Xk + (size_t)i * QX;
            const int il = i > 0 ? i - 1 : i, ih = i < M - 1 ? i + 1 : i;
            const double div = (i > 0 && i < M - 1) ? 2.0 : 1.0;
            double r[3], rd[3], q[4], qn[4];
            for (int c = 0; c < 3; ++c) {
                r[c] = xi[10 + c];
                rd[c] = (Xk[(size_t)ih * QX + 10 + c] - Xk[(size_t)il * QX + 10 + c]) / div / dt;
            }
            const QuadTrajGenArgs g = *gp;
            const double b[4] = { rd[0] * g.J[0] + (g.J[2] - g.J[1]) * r[2] * r[1], rd[1] * g.J[1] + (g.J[0] - g.J[2]) * r[0] * r[2],
                                  rd[2] * g.J[2] + (g.J[1] - g.J[0]) * r[1] * r[0], Uk[(size_t)i * QU + 3] };
            load4(xi + 3, q);
            corrected(i, q, Uk[(size_t)i * QU], qn);
            row[0] = xi[0] - px0; row[1] = xi[1] - py0; row[2] = xi[2];
            for (int c = 0; c < 4; ++c) row[3 + c] = qn[c];
            row[7] = xi[7]; row[8] = xi[8]; row[9] = xi[9];
            for (int c = 0; c < 3; ++c) row[10 + c] = r[c];
            for (int m = 0; m < 4; ++m)
                row[QX + m] = (g.ainv[m * 4] * b[0] + g.ainv[m * 4 + 1] * b[1] + g.ainv[m * 4 + 2] * b[2] + g.ainv[m * 4 + 3] * b[3]) / g.max_thrust;
        }
        __syncthreads();                          // the tile's rows are in LDS, and every read of this tile's rows is done
        const int r0 = tile * QT_THREADS, cnt = M - r0 < QT_THREADS ? M - r0 : QT_THREADS;
        for (int e = tid; e < cnt * QX; e += QT_THREADS) Xk[(size_t)r0 * QX + e] = s_row[(e / QX) * QT_ROW + e % QX];
        for (int e = tid; e < cnt * QU; e += QT_THREADS) Uk[(size_t)r0 * QU + e] = s_row[(e / QU) * QT_ROW + QX + e % QU];
        __syncthreads();                          // LDS may be written again
    }
}

}  // namespace
