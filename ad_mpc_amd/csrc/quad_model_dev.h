// quad_model_dev.h -- device code of the quadrotor model shared by the solve kernels (admpc_quad.hip) and the observe kernel
// (admpc_quad_learn.hip; with a period per vehicle: admpc_quad_targets.hip): the rotation matrix of a quaternion, its directional derivative, and f(x, u) with its forward-mode tangent,
// the GP residual and the linear rotor drag included.  Include INSIDE the translation unit's anonymous namespace, after QX, QU and
// Cfg (AdmpcQuadConfig) are defined; every function is __forceinline__.
#pragma once

// f(x, u) and df = Jx sx + Ju su   (oracle/quad_oracle.c:quad_f_tan, same expressions)
// rotation matrix of a quaternion and its directional derivative along sq (utils.py:323-338)
__device__ __forceinline__ void quad_rot(double qw, double qx, double qy, double qz, double (&R)[3][3]) {
    R[0][0] = 1 - 2 * (qy * qy + qz * qz); R[0][1] = 2 * (qx * qy - qw * qz); R[0][2] = 2 * (qx * qz + qw * qy);
    R[1][0] = 2 * (qx * qy + qw * qz); R[1][1] = 1 - 2 * (qx * qx + qz * qz); R[1][2] = 2 * (qy * qz - qw * qx);
    R[2][0] = 2 * (qx * qz - qw * qy); R[2][1] = 2 * (qy * qz + qw * qx); R[2][2] = 1 - 2 * (qx * qx + qy * qy);
}
__device__ __forceinline__ void quad_drot(double qw, double qx, double qy, double qz, double sw, double sxx, double sy, double sz, double (&D)[3][3]) {
    D[0][0] = -4 * (qy * sy + qz * sz); D[0][1] = 2 * (sxx * qy + qx * sy - sw * qz - qw * sz); D[0][2] = 2 * (sxx * qz + qx * sz + sw * qy + qw * sy);
    D[1][0] = 2 * (sxx * qy + qx * sy + sw * qz + qw * sz); D[1][1] = -4 * (qx * sxx + qz * sz); D[1][2] = 2 * (sy * qz + qy * sz - sw * qx - qw * sxx);
    D[2][0] = 2 * (sxx * qz + qx * sz - sw * qy - qw * sy); D[2][1] = 2 * (sy * qz + qy * sz + sw * qx + qw * sxx); D[2][2] = -4 * (qx * sxx + qy * sy);
}

// trig / gq: the first node's GP-state parameter (quad_3d_optimizer.py:291-297, :546-552; oracle: gpx).  On lanes with trig set the GP
// features and the rotation of the means come from the constant state gq[13] (zero tangent along sx), elsewhere from x.  gq must be
// readable on every lane when c->n_gp > 0.
__device__ __forceinline__ void quad_f_tan(const Cfg* __restrict__ c, const double* x, const double* u, const double* sx, const double* su,
                                           bool trig, const double* __restrict__ gq, double* f, double* df)
{
    const double qw = x[3], qx = x[4], qy = x[5], qz = x[6], r0 = x[10], r1 = x[11], r2 = x[12];
    const double sw = sx[3], sxx = sx[4], sy = sx[5], sz = sx[6], t0 = sx[10], t1 = sx[11], t2 = sx[12];
    double ga[3] = { 0, 0, 0 }, dga[3] = { 0, 0, 0 };        // GP residual and drag term of the acceleration, evaluated first (shorter live ranges)
    if (c->n_gp > 0) {                       // wave-uniform.  GP residual: v' += R(q) mu(z), z = [x with v in the body frame; u]
        // the state the features and the rotation come from: entries 3..12 (attitude, velocity, body rates) of x or of the parameter
        double xe[10], se[10];
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            double gv = gq[3 + i];
            asm volatile("" : "+v"(gv));      // a value, not an address: otherwise the select becomes `load (trig ? gq : &x)` with x spilled to scratch for it
            xe[i] = trig ? gv : x[3 + i]; se[i] = trig ? 0.0 : sx[3 + i];
        }
        const double ew = xe[0], ex = xe[1], ey = xe[2], ez = xe[3], fw = se[0], fx = se[1], fy = se[2], fz = se[3];
        const double R[3][3] = { { 1 - 2 * (ey * ey + ez * ez), 2 * (ex * ey - ew * ez), 2 * (ex * ez + ew * ey) },
                                 { 2 * (ex * ey + ew * ez), 1 - 2 * (ex * ex + ez * ez), 2 * (ey * ez - ew * ex) },
                                 { 2 * (ex * ez - ew * ey), 2 * (ey * ez + ew * ex), 1 - 2 * (ex * ex + ey * ey) } };
        // dR = directional derivative of R, formed where it is used (twice) instead of kept live across the GP loop
        auto dRm = [&](double (&D)[3][3]) {
            D[0][0] = -4 * (ey * fy + ez * fz); D[0][1] = 2 * (fx * ey + ex * fy - fw * ez - ew * fz); D[0][2] = 2 * (fx * ez + ex * fz + fw * ey + ew * fy);
            D[1][0] = 2 * (fx * ey + ex * fy + fw * ez + ew * fz); D[1][1] = -4 * (ex * fx + ez * fz); D[1][2] = 2 * (fy * ez + ey * fz - fw * ex - ew * fx);
            D[2][0] = 2 * (fx * ez + ex * fz - fw * ey - ew * fy); D[2][1] = 2 * (fy * ez + ey * fz + fw * ex + ew * fx); D[2][2] = -4 * (ex * fx + ey * fy);
        };
        // candidate features: entries 7..16 of z (body-frame velocity, body rates, inputs); position and attitude are not offered
        double z[10], dz[10];
        { double dR[3][3]; dRm(dR);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double a2 = 0, d2 = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { a2 += R[k][i] * xe[4 + k]; d2 += dR[k][i] * xe[4 + k] + R[k][i] * se[4 + k]; }
            z[i] = a2; dz[i] = d2;
            z[3 + i] = xe[7 + i]; dz[3 + i] = se[7 + i];
        } }
#pragma unroll
        for (int m = 0; m < QU; ++m) { z[6 + m] = u[m]; dz[6 + m] = su[m]; }
        double mb[3] = { 0, 0, 0 }, dmb[3] = { 0, 0, 0 };
        for (int g = 0; g < c->n_gp; ++g) {
            const AdmpcGp& gp = c->gp[g];
            // features by compare-select chains (a runtime-indexed private array would live in scratch memory)
            double zf[ADMPC_GP_MAX_FEAT], dzf[ADMPC_GP_MAX_FEAT], il[ADMPC_GP_MAX_FEAT];
#pragma unroll
            for (int k = 0; k < ADMPC_GP_MAX_FEAT; ++k) {
                const int fk = k < gp.n_feat ? gp.feat[k] - 7 : -1;
                double zv = 0, dzv = 0;
#pragma unroll
                for (int i = 0; i < 10; ++i) { zv = fk == i ? z[i] : zv; dzv = fk == i ? dz[i] : dzv; }
                zf[k] = zv; dzf[k] = dzv; il[k] = k < gp.n_feat ? gp.inv_l2[k] : 0.0;
            }
            double m = 0, dm = 0;
            for (int i = 0; i < gp.n_points; ++i) {
                double e = 0, de = 0;
#pragma unroll
                for (int k = 0; k < ADMPC_GP_MAX_FEAT; ++k) {      // unused feature: difference 0, whatever the caller left in Z[k]
                    const double dzk = k < gp.n_feat ? zf[k] - gp.Z[k][i] : 0.0; e += dzk * dzk * il[k]; de += dzk * il[k] * dzf[k];
                }
                const double ka = gp.sigma_f * exp(-0.5 * e) * gp.alpha[i];
                m += ka; dm -= ka * de;
            }
            const int o = gp.out - 7;
#pragma unroll
            for (int i = 0; i < 3; ++i) { mb[i] += o == i ? m + gp.ymean : 0.0; dmb[i] += o == i ? dm : 0.0; }
        }
        double dR[3][3]; dRm(dR);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double a2 = 0, d2 = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { a2 += R[i][k] * mb[k]; d2 += dR[i][k] * mb[k] + R[i][k] * dmb[k]; }
            ga[i] = a2; dga[i] = d2;
        }
    }
    if (c->rdrv[0] != 0.0 || c->rdrv[1] != 0.0 || c->rdrv[2] != 0.0) {      // wave-uniform.  Linear rotor drag (:364-381): v' += R(q) D R(q)' v
        const double R[3][3] = { { 1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy) },
                                 { 2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx) },
                                 { 2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy) } };
        const double dR[3][3] = { { -4 * (qy * sy + qz * sz), 2 * (sxx * qy + qx * sy - sw * qz - qw * sz), 2 * (sxx * qz + qx * sz + sw * qy + qw * sy) },
                                  { 2 * (sxx * qy + qx * sy + sw * qz + qw * sz), -4 * (qx * sxx + qz * sz), 2 * (sy * qz + qy * sz - sw * qx - qw * sxx) },
                                  { 2 * (sxx * qz + qx * sz - sw * qy - qw * sy), 2 * (sy * qz + qy * sz + sw * qx + qw * sxx), -4 * (qx * sxx + qy * sy) } };
        double wb[3], dwb[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double a2 = 0, d2 = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { a2 += R[k][i] * x[7 + k]; d2 += dR[k][i] * x[7 + k] + R[k][i] * sx[7 + k]; }
            wb[i] = c->rdrv[i] * a2; dwb[i] = c->rdrv[i] * d2;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double a2 = 0, d2 = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { a2 += R[i][k] * wb[k]; d2 += dR[i][k] * wb[k] + R[i][k] * dwb[k]; }
            ga[i] += a2; dga[i] += d2;
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) { f[i] = x[7 + i]; df[i] = sx[7 + i]; }
    f[3] = 0.5 * (-r0 * qx - r1 * qy - r2 * qz);
    f[4] = 0.5 * ( r0 * qw + r2 * qy - r1 * qz);
    f[5] = 0.5 * ( r1 * qw - r2 * qx + r0 * qz);
    f[6] = 0.5 * ( r2 * qw + r1 * qx - r0 * qy);
    df[3] = 0.5 * (-t0 * qx - r0 * sxx - t1 * qy - r1 * sy - t2 * qz - r2 * sz);
    df[4] = 0.5 * ( t0 * qw + r0 * sw + t2 * qy + r2 * sy - t1 * qz - r1 * sz);
    df[5] = 0.5 * ( t1 * qw + r1 * sw - t2 * qx - r2 * sxx + t0 * qz + r0 * sz);
    df[6] = 0.5 * ( t2 * qw + r2 * sw + t1 * qx + r1 * sxx - t0 * qy - r0 * sy);
    const double a = c->max_thrust * (u[0] + u[1] + u[2] + u[3]) / c->mass;
    const double da = c->max_thrust * (su[0] + su[1] + su[2] + su[3]) / c->mass;
    const double c0 = 2 * (qx * qz + qw * qy), c1 = 2 * (qy * qz - qw * qx), c2 = 1 - 2 * (qx * qx + qy * qy);
    const double d0 = 2 * (sxx * qz + qx * sz + sw * qy + qw * sy), d1 = 2 * (sy * qz + qy * sz - sw * qx - qw * sxx),
                 d2 = -4 * (qx * sxx + qy * sy);
    f[7] = c0 * a; f[8] = c1 * a; f[9] = c2 * a - c->g;
    df[7] = d0 * a + c0 * da; df[8] = d1 * a + c1 * da; df[9] = d2 * a + c2 * da;
    double tx = 0, ty = 0, tz = 0, dtx = 0, dty = 0, dtz = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        tx += c->max_thrust * u[i] * c->y_f[i]; ty -= c->max_thrust * u[i] * c->x_f[i]; tz += c->max_thrust * u[i] * c->z_l_tau[i];
        dtx += c->max_thrust * su[i] * c->y_f[i]; dty -= c->max_thrust * su[i] * c->x_f[i]; dtz += c->max_thrust * su[i] * c->z_l_tau[i];
    }
    f[10] = (tx + (c->J[1] - c->J[2]) * r1 * r2) / c->J[0];
    f[11] = (ty + (c->J[2] - c->J[0]) * r2 * r0) / c->J[1];
    f[12] = (tz + (c->J[0] - c->J[1]) * r0 * r1) / c->J[2];
    df[10] = (dtx + (c->J[1] - c->J[2]) * (t1 * r2 + r1 * t2)) / c->J[0];
    df[11] = (dty + (c->J[2] - c->J[0]) * (t2 * r0 + r2 * t0)) / c->J[1];
    df[12] = (dtz + (c->J[0] - c->J[1]) * (t0 * r1 + r0 * t1)) / c->J[2];
    f[7] += ga[0]; f[8] += ga[1]; f[9] += ga[2]; df[7] += dga[0]; df[8] += dga[1]; df[9] += dga[2];
}
