// quad_sim_dev.h -- the device text of the quadrotor's simplified simulator (Quadrotor3D.update, quad_3d.py:175-287) that the two plant
// kernels of admpc_quad_plant.hip share, and whose argument block the rollouts of admpc_quad_fleet.hip and admpc_quad_targets.hip fill: the
// argument block of a plant launch, the vehicle's constants in vector registers, the derivative, one RK4 update, and the rollout's tally.  Everything is static and inlined: each unit
// has its own copy, and the deterministic instantiation (DIST = false) carries no term of the disturbances.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/admpc_quad_fleet.h"

#define QSIM_NX ADMPC_QUAD_NX
#define QSIM_NU ADMPC_QUAD_NU

// one trajectory of a bank: its first row in the bank's row space and its length
struct QuadTrajDesc { long long off; int32_t M; int32_t pad; };

// what one launch of a plant kernel works on (by value); the rollout's pointers are null for a plant-only step
struct QuadPlantArgs {
    AdmpcQuadPlantParams p;
    int B, K;
    const double* u; long long u_stride;      // row b at u + b * u_stride
    double* x;                                // [B][13] in/out
    const double* yref; long long yref_stride;    // the window: yref[b * yref_stride + 0 .. 2] is the position reference
    const int32_t* status;                    // [B]
    double* tally;                            // [B][3]
    int32_t* counts;                          // [B][3]
    const int32_t* traj_of;                   // [B]
    int32_t* idx;                             // [B]
    const QuadTrajDesc* desc;                 // [K]
    double *traj_pre, *traj_post;             // [B][13] slots of traj_out, or null
    double* u_out;                            // [B][4] slot of u_out, or null
};

// the thrusts' constants of a sub-step: what f_vel and f_rate take from u (quad_3d.py:253, 284-286).  With a disturbance (DIST) the
// torque t_d is folded into ty, tx, tz and f_d[2] / mass into az -- the sums the reference forms first, so nothing is rounded
// differently -- and fx, fy are f_d[0 .. 1] / mass; without one, fx and fy are not read.
struct Thrust { double az, ty, tx, tz, fx, fy; };

// The vehicle constants a period reads, held in VECTOR registers: a gfx9 VALU instruction reads one scalar operand at most, and with the
// whole parameter block and the rollout's pointers live across the stride loop the scalar file ran over (14 SGPR spills in the first
// build; none now, 230 VGPRs, two waves per SIMD).  vreg() is an empty asm statement that pins its operand to a VGPR.
struct SimConst { double dt, half, mass, aero, rd[3], gz, iJ[3], dJ[3], xf[4], yf[4], zt[4], u_min, u_max, max_thrust; int drag; };
static __device__ __forceinline__ double vreg(double v) { asm volatile("" : "+v"(v)); return v; }
static __device__ __forceinline__ SimConst sim_const(const AdmpcQuadPlantParams& p)
{
    SimConst c;
    c.dt = vreg(p.dt); c.half = vreg(p.dt / 2.0); c.mass = vreg(p.mass); c.aero = vreg(p.aero_drag);
    for (int i = 0; i < 3; ++i) { c.rd[i] = vreg(p.rotor_drag[i]); c.iJ[i] = vreg(1.0 / p.J[i]); }
    c.gz = vreg(-p.g + -p.payload_mass * p.g / p.mass);                      // -g + a_payload
    c.dJ[0] = vreg(p.J[1] - p.J[2]); c.dJ[1] = vreg(p.J[2] - p.J[0]); c.dJ[2] = vreg(p.J[0] - p.J[1]);
    for (int i = 0; i < 4; ++i) { c.xf[i] = vreg(p.x_f[i]); c.yf[i] = vreg(p.y_f[i]); c.zt[i] = vreg(p.z_l_tau[i]); }
    c.u_min = vreg(p.u_min); c.u_max = vreg(p.u_max); c.max_thrust = vreg(p.max_thrust);
    c.drag = p.drag;
    return c;
}

// the thrusts' constants from the four thrusts in N
static __device__ __forceinline__ Thrust quad_thrust(const SimConst& c, const double (&f)[QSIM_NU])
{
    Thrust th;
    th.az = (((f[0] + f[1]) + f[2]) + f[3]) / c.mass;
    th.ty = f[0] * c.yf[0] + f[1] * c.yf[1] + f[2] * c.yf[2] + f[3] * c.yf[3];
    th.tx = f[0] * c.xf[0] + f[1] * c.xf[1] + f[2] * c.xf[2] + f[3] * c.xf[3];
    th.tz = f[0] * c.zt[0] + f[1] * c.zt[1] + f[2] * c.zt[2] + f[3] * c.zt[3];
    th.fx = 0.0; th.fy = 0.0;
    return th;
}

// d/dt of [p, q, v, w] (quad_3d.py:222-287) at state s; DIST: a disturbance force acts (f_d of :198, through v_dot_q of :271)
template <bool DIST>
static __device__ __forceinline__ void quad_sim_f(const SimConst& c, const Thrust& th, const double (&s)[QSIM_NX], double (&k)[QSIM_NX])
{
    const double qw = s[3], qx = s[4], qy = s[5], qz = s[6];
    const double vx = s[7], vy = s[8], vz = s[9];
    const double w0 = s[10], w1 = s[11], w2 = s[12];
    k[0] = vx; k[1] = vy; k[2] = vz;                                                         // f_pos
    k[3] = 0.5 * (-w0 * qx - w1 * qy - w2 * qz);                                             // f_att: 1/2 skew_symmetric(w) q
    k[4] = 0.5 * (w0 * qw + w2 * qy - w1 * qz);
    k[5] = 0.5 * (w1 * qw - w2 * qx + w0 * qz);
    k[6] = 0.5 * (w2 * qw + w1 * qx - w0 * qy);
    // q_to_rot_mat(q) (utils.py:323-338); q_to_rot_mat(quaternion_inverse(q)) is its transpose, entry for entry
    const double r00 = 1.0 - 2.0 * (qy * qy + qz * qz), r01 = 2.0 * (qx * qy - qw * qz), r02 = 2.0 * (qx * qz + qw * qy);
    const double r10 = 2.0 * (qx * qy + qw * qz), r11 = 1.0 - 2.0 * (qx * qx + qz * qz), r12 = 2.0 * (qy * qz - qw * qx);
    const double r20 = 2.0 * (qx * qz - qw * qy), r21 = 2.0 * (qy * qz + qw * qx), r22 = 1.0 - 2.0 * (qx * qx + qy * qy);
    double dx = 0.0, dy = 0.0, dz = 0.0;
    if (c.drag) {                                                                            // uniform over the launch
        const double b0 = r00 * vx + r10 * vy + r20 * vz, b1 = r01 * vx + r11 * vy + r21 * vz, b2 = r02 * vx + r12 * vy + r22 * vz;
        const double s0 = (double)((b0 > 0.0) - (b0 < 0.0)), s1 = (double)((b1 > 0.0) - (b1 < 0.0)), s2 = (double)((b2 > 0.0) - (b2 < 0.0));
        const double a0 = -c.aero * (b0 * b0) * s0 / c.mass - c.rd[0] * b0 / c.mass;
        const double a1 = -c.aero * (b1 * b1) * s1 / c.mass - c.rd[1] * b1 / c.mass;
        const double a2 = -c.aero * (b2 * b2) * s2 / c.mass - c.rd[2] * b2 / c.mass;
        dx = r00 * a0 + r01 * a1 + r02 * a2; dy = r10 * a0 + r11 * a1 + r12 * a2; dz = r20 * a0 + r21 * a1 + r22 * a2;
    }
    if (DIST) {                                                                              // f_vel with R(q) (a_thrust + f_d / mass)
        k[7] = dx + ((r00 * th.fx + r01 * th.fy) + r02 * th.az);
        k[8] = dy + ((r10 * th.fx + r11 * th.fy) + r12 * th.az);
        k[9] = (c.gz + dz) + ((r20 * th.fx + r21 * th.fy) + r22 * th.az);
    }
    else {
        k[7] = dx + r02 * th.az;                                                             // f_vel
        k[8] = dy + r12 * th.az;
        k[9] = (c.gz + dz) + r22 * th.az;
    }
    k[10] = c.iJ[0] * (th.ty + c.dJ[0] * w1 * w2);                                           // f_rate
    k[11] = c.iJ[1] * (-th.tx + c.dJ[1] * w2 * w0);
    k[12] = c.iJ[2] * (th.tz + c.dJ[2] * w0 * w1);
}

// one Quadrotor3D.update: classic RK4 with step dt, then unit_quat
template <bool DIST>
static __device__ __forceinline__ void quad_sim_update(const SimConst& c, const Thrust& th, double (&x)[QSIM_NX])
{
    const double dt = c.dt, half = c.half;
    double k[QSIM_NX], acc[QSIM_NX], s[QSIM_NX];
    quad_sim_f<DIST>(c, th, x, k);
#pragma unroll
    for (int i = 0; i < QSIM_NX; ++i) { acc[i] = 1.0 / 6.0 * k[i]; s[i] = x[i] + half * k[i]; }
    quad_sim_f<DIST>(c, th, s, k);
#pragma unroll
    for (int i = 0; i < QSIM_NX; ++i) { acc[i] += 2.0 / 6.0 * k[i]; s[i] = x[i] + half * k[i]; }
    quad_sim_f<DIST>(c, th, s, k);
#pragma unroll
    for (int i = 0; i < QSIM_NX; ++i) { acc[i] += 2.0 / 6.0 * k[i]; s[i] = x[i] + dt * k[i]; }
    quad_sim_f<DIST>(c, th, s, k);
#pragma unroll
    for (int i = 0; i < QSIM_NX; ++i) x[i] = x[i] + dt * (acc[i] + 1.0 / 6.0 * k[i]);
    const double inv = 1.0 / sqrt(((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]) + x[6] * x[6]);
    x[3] *= inv; x[4] *= inv; x[5] *= inv; x[6] *= inv;
}

// the sums of a rollout for one vehicle: every operation rounded on its own, so that numpy reproduces them bit for bit
static __device__ __forceinline__ void quad_tally(const QuadPlantArgs& a, long long b, const double (&x)[QSIM_NX], bool replaced)
{
#pragma clang fp contract(off)
    const double* r = a.yref + b * a.yref_stride;
    const double ex = r[0] - x[0], ey = r[1] - x[1], ez = r[2] - x[2];
    const double n2 = (ex * ex + ey * ey) + ez * ez;
    double* t = a.tally + b * 3;
    if (isfinite(n2)) {
        const double n = sqrt(n2);
        t[0] = t[0] + n;
        t[1] = t[1] + n2;
        if (n > t[2]) t[2] = n;
    }
    int32_t* c = a.counts + b * 3;
    c[0] = c[0] + 1;
    if (a.status[b] != 0) c[1] = c[1] + 1;
    if (replaced) c[2] = c[2] + 1;
}
