/*
 * quad_oracle.c -- CPU restatement (plain C, fp64) of one acados SQP-RTI step of the reference's quadrotor MPC.
 * TEST INFRASTRUCTURE ONLY: loaded by tests/ (and nothing else); the product path is ad_mpc_amd/csrc/admpc_quad.hip.
 *
 * What it follows (data_driven_mpc/ros_gp_mpc):
 *   model        src/quad_mpc/quad_3d_optimizer.py:341-393 (p, q, v, w dynamics; the linear drag term :364-381 is an option of the class
 *                that the shipped generated code does not contain: cfg.rdrv), :289-327 GP residual with the first node's GP state,
 *                src/utils/utils.py:323-338 (q_to_rot_mat), :392-410 (skew_symmetric), src/quad_mpc/quad_3d.py:40-74 (vehicle)
 *   formulation  src/quad_mpc/quad_3d_optimizer.py:150-207 + acados_models/my_quad_acados_ocp.json (LINEAR_LS, W scaled by Ts,
 *                hard input box, x0 fixed, ERK4 with one step per interval, Gauss-Newton, full condensing, RTI)
 *   QP           the condensed QP is strictly convex in du (R > 0): any method reaching its minimiser is equivalent; here a Mehrotra
 *                predictor-corrector on the box-constrained dense QP (HPIPM's own algorithm is not in the reference tree).
 * Pins: the model against the reference's compiled CasADi code (oracle/_ref/libquad_ref.so, tests/golden/quad_shooting.json);
 * the QP solution against an independent bounded solve of the condensed QP built from the reference's VDE (tests/test_quad_oracle.py).
 */
#include "../include/admpc_quad.h"
#include <math.h>
#include <string.h>

#define NX ADMPC_QUAD_NX
#define NU ADMPC_QUAD_NU
#define NMAX (ADMPC_QUAD_MAX_N * ADMPC_QUAD_NU)
#ifdef ORACLE_LONG_DOUBLE                 /* libquad_oracle_ld.so: every real in the x87 80-bit format, the rounding-error yardstick */
typedef long double real;
#define R_EXP expl
#define R_SQRT sqrtl
#define R_FABS fabsl
#define R_FMAX fmaxl
#define R_FMIN fminl
#else
typedef double real;
#define R_EXP exp
#define R_SQRT sqrt
#define R_FABS fabs
#define R_FMAX fmax
#define R_FMIN fmin
#endif
typedef AdmpcQuadConfig Cfg;

/* f(x, u) and its directional derivative df = Jx sx + Ju su (forward mode, by hand).
 * gpx (may be NULL): the "GP state" parameter of the first optimisation node (quad_3d_optimizer.py:291-297, :546-552: p = [gp_x, 1] at node
 * 0, zeros elsewhere -- `gp_x * trigger_var + x * (1 - trigger_var)`): with it the GP features AND the rotation of the GP means back to the
 * world frame are taken from that constant state instead of the integrated one, so the residual does not depend on x there (zero tangent
 * along sx; the input features still carry su). */
static void quad_f_tan(const Cfg* c, const real* x, const real* u, const real* sx, const real* su, const real* gpx, real* f, real* df)
{
    const real qw = x[3], qx = x[4], qy = x[5], qz = x[6], r0 = x[10], r1 = x[11], r2 = x[12];
    const real sw = sx[3], sxx = sx[4], sy = sx[5], sz = sx[6], t0 = sx[10], t1 = sx[11], t2 = sx[12];
    for (int i = 0; i < 3; ++i) { f[i] = x[7 + i]; df[i] = sx[7 + i]; }                       /* :361 p' = v */
    f[3] = 0.5 * (-r0 * qx - r1 * qy - r2 * qz);                                               /* :364 q' = 1/2 S(r) q, utils.py:401-404 */
    f[4] = 0.5 * ( r0 * qw + r2 * qy - r1 * qz);
    f[5] = 0.5 * ( r1 * qw - r2 * qx + r0 * qz);
    f[6] = 0.5 * ( r2 * qw + r1 * qx - r0 * qy);
    df[3] = 0.5 * (-t0 * qx - r0 * sxx - t1 * qy - r1 * sy - t2 * qz - r2 * sz);
    df[4] = 0.5 * ( t0 * qw + r0 * sw + t2 * qy + r2 * sy - t1 * qz - r1 * sz);
    df[5] = 0.5 * ( t1 * qw + r1 * sw - t2 * qx - r2 * sxx + t0 * qz + r0 * sz);
    df[6] = 0.5 * ( t2 * qw + r2 * sw + t1 * qx + r1 * sxx - t0 * qy - r0 * sy);
    const real a = c->max_thrust * (u[0] + u[1] + u[2] + u[3]) / c->mass;                     /* :372-374 */
    const real da = c->max_thrust * (su[0] + su[1] + su[2] + su[3]) / c->mass;
    const real c0 = 2 * (qx * qz + qw * qy), c1 = 2 * (qy * qz - qw * qx), c2 = 1 - 2 * (qx * qx + qy * qy);   /* third column of R(q) */
    const real d0 = 2 * (sxx * qz + qx * sz + sw * qy + qw * sy), d1 = 2 * (sy * qz + qy * sz - sw * qx - qw * sxx),
               d2 = -4 * (qx * sxx + qy * sy);
    f[7] = c0 * a; f[8] = c1 * a; f[9] = c2 * a - c->g;                                        /* :376 v' = R(q) a_thrust - g */
    df[7] = d0 * a + c0 * da; df[8] = d1 * a + c1 * da; df[9] = d2 * a + c2 * da;
    real tx = 0, ty = 0, tz = 0, dtx = 0, dty = 0, dtz = 0;                                     /* :386-393 */
    for (int i = 0; i < 4; ++i) {
        tx += c->max_thrust * u[i] * c->y_f[i]; ty -= c->max_thrust * u[i] * c->x_f[i]; tz += c->max_thrust * u[i] * c->z_l_tau[i];
        dtx += c->max_thrust * su[i] * c->y_f[i]; dty -= c->max_thrust * su[i] * c->x_f[i]; dtz += c->max_thrust * su[i] * c->z_l_tau[i];
    }
    f[10] = (tx + ((real)c->J[1] - c->J[2]) * r1 * r2) / c->J[0];
    f[11] = (ty + ((real)c->J[2] - c->J[0]) * r2 * r0) / c->J[1];
    f[12] = (tz + ((real)c->J[0] - c->J[1]) * r0 * r1) / c->J[2];
    df[10] = (dtx + ((real)c->J[1] - c->J[2]) * (t1 * r2 + r1 * t2)) / c->J[0];
    df[11] = (dty + ((real)c->J[2] - c->J[0]) * (t2 * r0 + r2 * t0)) / c->J[1];
    df[12] = (dtz + ((real)c->J[0] - c->J[1]) * (t0 * r1 + r0 * t1)) / c->J[2];
    const int drag = c->rdrv[0] != 0 || c->rdrv[1] != 0 || c->rdrv[2] != 0;
    if (drag) {
        /* linear rotor-drag compensation (quad_3d_optimizer.py:364-381, Faessler et al.): v' += R(q) D R(q)' v, D = diag(rdrv) */
        const real R[3][3] = { { 1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy) },
                               { 2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx) },
                               { 2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy) } };
        const real dR[3][3] = { { -4 * (qy * sy + qz * sz), 2 * (sxx * qy + qx * sy - sw * qz - qw * sz), 2 * (sxx * qz + qx * sz + sw * qy + qw * sy) },
                                { 2 * (sxx * qy + qx * sy + sw * qz + qw * sz), -4 * (qx * sxx + qz * sz), 2 * (sy * qz + qy * sz - sw * qx - qw * sxx) },
                                { 2 * (sxx * qz + qx * sz - sw * qy - qw * sy), 2 * (sy * qz + qy * sz + sw * qx + qw * sxx), -4 * (qx * sxx + qy * sy) } };
        real wb[3], dwb[3];
        for (int i = 0; i < 3; ++i) {                                  /* D v_b, v_b = R' v */
            real a2 = 0, d2 = 0;
            for (int k = 0; k < 3; ++k) { a2 += R[k][i] * x[7 + k]; d2 += dR[k][i] * x[7 + k] + R[k][i] * sx[7 + k]; }
            wb[i] = c->rdrv[i] * a2; dwb[i] = c->rdrv[i] * d2;
        }
        for (int i = 0; i < 3; ++i) {
            real a2 = 0, d2 = 0;
            for (int k = 0; k < 3; ++k) { a2 += R[i][k] * wb[k]; d2 += dR[i][k] * wb[k] + R[i][k] * dwb[k]; }
            f[7 + i] += a2; df[7 + i] += d2;
        }
    }
    if (c->n_gp > 0) {
        /* GP residual (quad_3d_optimizer.py:289-327): features from z = [x with v in the body frame; u], means of the body-frame
         * acceleration components rotated back to the world frame:  v' += R(q) mu(z);  utils.py:323-338 for R.
         * The state the features and the rotation come from: the integrated one, or the node's GP-state parameter (zero tangent). */
        real xe[NX], se[NX];
        for (int i = 0; i < NX; ++i) { xe[i] = gpx ? gpx[i] : x[i]; se[i] = gpx ? 0 : sx[i]; }
        const real ew = xe[3], ex = xe[4], ey = xe[5], ez = xe[6], fw = se[3], fx = se[4], fy = se[5], fz = se[6];
        real R[3][3] = { { 1 - 2 * (ey * ey + ez * ez), 2 * (ex * ey - ew * ez), 2 * (ex * ez + ew * ey) },
                         { 2 * (ex * ey + ew * ez), 1 - 2 * (ex * ex + ez * ez), 2 * (ey * ez - ew * ex) },
                         { 2 * (ex * ez - ew * ey), 2 * (ey * ez + ew * ex), 1 - 2 * (ex * ex + ey * ey) } };
        real dR[3][3] = { { -4 * (ey * fy + ez * fz), 2 * (fx * ey + ex * fy - fw * ez - ew * fz), 2 * (fx * ez + ex * fz + fw * ey + ew * fy) },
                          { 2 * (fx * ey + ex * fy + fw * ez + ew * fz), -4 * (ex * fx + ez * fz), 2 * (fy * ez + ey * fz - fw * ex - ew * fx) },
                          { 2 * (fx * ez + ex * fz - fw * ey - ew * fy), 2 * (fy * ez + ey * fz + fw * ex + ew * fx), -4 * (ex * fx + ey * fy) } };
        real z[17], dz[17];
        for (int i = 0; i < NX; ++i) { z[i] = xe[i]; dz[i] = se[i]; }
        for (int i = 0; i < 3; ++i) {                                  /* v_b = R' v  (v_dot_q(v, q^-1)) */
            real a2 = 0, d2 = 0;
            for (int k = 0; k < 3; ++k) { a2 += R[k][i] * xe[7 + k]; d2 += dR[k][i] * xe[7 + k] + R[k][i] * se[7 + k]; }
            z[7 + i] = a2; dz[7 + i] = d2;
        }
        for (int m = 0; m < NU; ++m) { z[NX + m] = u[m]; dz[NX + m] = su[m]; }
        real mb[3] = {0, 0, 0}, dmb[3] = {0, 0, 0};
        for (int g = 0; g < c->n_gp; ++g) {
            const AdmpcGp* gp = &c->gp[g];
            real m = 0, dm = 0;
            for (int i = 0; i < gp->n_points; ++i) {
                real e = 0, de = 0;
                for (int k = 0; k < gp->n_feat; ++k) { const real dzk = z[gp->feat[k]] - gp->Z[k][i]; e += dzk * dzk * gp->inv_l2[k]; de += dzk * gp->inv_l2[k] * dz[gp->feat[k]]; }
                const real ka = gp->sigma_f * R_EXP(-0.5 * e) * gp->alpha[i];
                m += ka; dm -= ka * de;
            }
            mb[gp->out - 7] += m + gp->ymean; dmb[gp->out - 7] += dm;
        }
        for (int i = 0; i < 3; ++i) {
            real a2 = 0, d2 = 0;
            for (int k = 0; k < 3; ++k) { a2 += R[i][k] * mb[k]; d2 += dR[i][k] * mb[k] + R[i][k] * dmb[k]; }
            f[7 + i] += a2; df[7 + i] += d2;
        }
    }
}

/* classic RK4 (one step of length h) of the state and ONE sensitivity column: col < 13 -> d/dx_col, col >= 13 -> d/du_(col-13) */
static void rk4_col(const Cfg* c, const real* x, const real* u, const real* gpx, real h, int col, real* phi, real* scol)
{
    static const real cs[4] = { 0, 0.5, 0.5, 1.0 }, ws[4] = { (real)1 / 6, (real)2 / 6, (real)2 / 6, (real)1 / 6 };
    real kx[NX] = {0}, ks[NX] = {0}, ax[NX] = {0}, as[NX] = {0}, su[NU] = {0};
    if (col >= NX) su[col - NX] = 1;
    for (int s = 0; s < 4; ++s) {
        real X[NX], S[NX], f[NX], df[NX];
        for (int i = 0; i < NX; ++i) { X[i] = x[i] + cs[s] * h * kx[i]; S[i] = (col == i ? 1.0 : 0.0) + cs[s] * h * ks[i]; }
        quad_f_tan(c, X, u, S, su, gpx, f, df);
        for (int i = 0; i < NX; ++i) { kx[i] = f[i]; ks[i] = df[i]; ax[i] += ws[s] * f[i]; as[i] += ws[s] * df[i]; }
    }
    for (int i = 0; i < NX; ++i) { phi[i] = x[i] + h * ax[i]; scol[i] = (col == i ? 1.0 : 0.0) + h * as[i]; }
}

/* phi [13], A [13][13], B [13][4] (row-major) */
static void rk4_sens(const Cfg* c, const real* x, const real* u, const real* gpx, real h, real* phi, real* A, real* B)
{
    real col[NX];
    for (int cc = 0; cc < NX + NU; ++cc) {
        rk4_col(c, x, u, gpx, h, cc, phi, col);
        for (int i = 0; i < NX; ++i) { if (cc < NX) A[i * NX + cc] = col[i]; else B[i * NU + (cc - NX)] = col[i]; }
    }
}

/* the exported entry points take double: inputs are copied into real buffers (NULL stays NULL), outputs rounded back to double */
static const real* to_real(real* dst, const double* src, int n)
{
    if (!src) return 0;
    for (int i = 0; i < n; ++i) dst[i] = src[i];
    return dst;
}
static void to_double(double* dst, const real* src, int n)
{
    for (int i = 0; i < n; ++i) dst[i] = (double)src[i];
}

/* gpx: NULL, or the GP-state parameter of a first node (see quad_f_tan) */
void quad_oracle_f(const Cfg* c, const double* x, const double* u, const double* gpx, double* f)
{
    real xr[NX], ur[NU], gr[NX], z13[NX] = {0}, z4[NU] = {0}, fr[NX], df[NX];
    quad_f_tan(c, to_real(xr, x, NX), to_real(ur, u, NU), z13, z4, to_real(gr, gpx, NX), fr, df);
    to_double(f, fr, NX);
}

void quad_oracle_rk4_sens(const Cfg* c, const double* x, const double* u, const double* gpx, double h, double* phi, double* A, double* B)
{
    real xr[NX], ur[NU], gr[NX], ph[NX], a[NX * NX], b[NX * NU];
    rk4_sens(c, to_real(xr, x, NX), to_real(ur, u, NU), to_real(gr, gpx, NX), h, ph, a, b);
    to_double(phi, ph, NX); to_double(A, a, NX * NX); to_double(B, b, NX * NU);
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* one RTI step of one instance                                                                                        */
/* ------------------------------------------------------------------------------------------------------------------ */
typedef struct { real A[ADMPC_QUAD_MAX_N][NX][NX], B[ADMPC_QUAD_MAX_N][NX][NU], b[ADMPC_QUAD_MAX_N][NX]; real H[NMAX][NMAX], g[NMAX]; } Work;

static void condense(const Cfg* c, const real* x0, const real* yref, const real* yref_e, const real* xbar, const real* ubar, Work* w)
{
    const int N = c->N, n = N * NU;
    real G[NX][NMAX], xh[NX];                     /* Gamma_k (13 x n), free response */
    memset(G, 0, sizeof G); memset(w->H, 0, sizeof w->H);
    for (int i = 0; i < NX; ++i) xh[i] = x0[i] - xbar[i];
    for (int i = 0; i < n; ++i) w->g[i] = (real)c->Ts * c->W[NX + i % NU] * (ubar[i] - yref[(i / NU) * ADMPC_QUAD_NY + NX + i % NU]);
    for (int k = 0; k < N; ++k) {
        real Gn[NX][NMAX], xn[NX];
        for (int r = 0; r < NX; ++r) {
            real a = w->b[k][r];
            for (int cc = 0; cc < NX; ++cc) a += w->A[k][r][cc] * xh[cc];
            xn[r] = a;
            for (int i = 0; i < n; ++i) {
                real s = 0;
                if (i / NU == k) s = w->B[k][r][i % NU];
                else if (i / NU < k) for (int cc = 0; cc < NX; ++cc) s += w->A[k][r][cc] * G[cc][i];
                Gn[r][i] = s;
            }
        }
        memcpy(G, Gn, sizeof G); memcpy(xh, xn, sizeof xh);
        /* cost of stage k + 1: weight Ts W (stages < N) or W_e (terminal) on  xbar + xhat + Gamma du - ref */
        const real* ref = k + 1 < N ? yref + (k + 1) * ADMPC_QUAD_NY : yref_e;
        for (int cc = 0; cc < NX; ++cc) {
            const real wq = k + 1 < N ? (real)c->Ts * c->W[cc] : c->We[cc];
            if (wq == 0) continue;
            const real e = xbar[(k + 1) * NX + cc] + xh[cc] - ref[cc];
            for (int i = 0; i < (k + 1) * NU; ++i) {
                w->g[i] += G[cc][i] * wq * e;
                for (int j = 0; j <= i; ++j) w->H[i][j] += G[cc][i] * wq * G[cc][j];
            }
        }
    }
    for (int i = 0; i < n; ++i) { w->H[i][i] += (real)c->Ts * c->W[NX + i % NU]; for (int j = 0; j < i; ++j) w->H[j][i] = w->H[i][j]; }
}

/* in-place Cholesky M = L L' (strictly lower part of L in M, reciprocals of its diagonal in invd) and solve M x = rhs;
 * returns 0 on a non-positive pivot.  Divisions are one reciprocal per column (as the device does) */
static int chol(int n, real M[NMAX][NMAX], real* invd)
{
    for (int j = 0; j < n; ++j) {
        real d = M[j][j];
        for (int k = 0; k < j; ++k) d -= M[j][k] * M[j][k];
        if (!(d > 0)) return 0;
        invd[j] = 1.0 / R_SQRT(d);
        for (int i = j + 1; i < n; ++i) {
            real s = M[i][j];
            for (int k = 0; k < j; ++k) s -= M[i][k] * M[j][k];
            M[i][j] = s * invd[j];
        }
    }
    return 1;
}
static void chol_solve(int n, real L[NMAX][NMAX], const real* invd, real* x)
{
    for (int i = 0; i < n; ++i) { real s = x[i]; for (int k = 0; k < i; ++k) s -= L[i][k] * x[k]; x[i] = s * invd[i]; }
    for (int i = n - 1; i >= 0; --i) { real s = x[i]; for (int k = i + 1; k < n; ++k) s -= L[k][i] * x[k]; x[i] = s * invd[i]; }
}

/* Mehrotra predictor-corrector on  min 1/2 du'H du + g'du,  lo <= du <= hi.  Returns 0 ok, 4 failure. */
static int box_qp(const Cfg* c, int n, real H[NMAX][NMAX], const real* g, const real* lo, const real* hi, real* du, int* iters)
{
    real tl[NMAX], tu[NMAX], ll[NMAX], lu[NMAX];
    for (int i = 0; i < n; ++i) {
        du[i] = 0;
        tl[i] = R_FMAX(du[i] - lo[i], c->ipm_thr0); tu[i] = R_FMAX(hi[i] - du[i], c->ipm_thr0);
        ll[i] = c->ipm_mu0 / tl[i]; lu[i] = c->ipm_mu0 / tu[i];
    }
    real alpha_prev = 1;
    int it = 0, cons = 0;                 /* cons: fallback mode (admpc_quad.h), no second-order term */
    for (;; ++it) {
        real rs[NMAX], rl[NMAX], ru[NMAX], mu, cmax, rmax;
    residuals:
        mu = 0; cmax = 0; rmax = 0;
        for (int i = 0; i < n; ++i) {
            real s = g[i] - ll[i] + lu[i];
            for (int j = 0; j < n; ++j) s += H[i][j] * du[j];
            rs[i] = s; rl[i] = du[i] - lo[i] - tl[i]; ru[i] = hi[i] - du[i] - tu[i];
            mu += tl[i] * ll[i] + tu[i] * lu[i];
            cmax = R_FMAX(cmax, R_FMAX(tl[i] * ll[i], tu[i] * lu[i]));
            rmax = R_FMAX(rmax, R_FMAX(R_FABS(rs[i]), R_FMAX(R_FABS(rl[i]), R_FABS(ru[i]))));
        }
        mu /= 2 * n;
        if (!(mu == mu) || !(rmax == rmax)) { *iters = it; return 4; }
        if ((cmax <= c->ipm_tol_comp && rmax <= c->ipm_tol_res) || it >= c->ipm_iter_max + (cons ? ADMPC_QUAD_IPM_FALLBACK_ITER : 0)) break;
        if (!cons && it >= ADMPC_QUAD_IPM_FALLBACK_ITER) {
            cons = 1;
            for (int i = 0; i < n; ++i) {
                du[i] = 0;
                tl[i] = R_FMAX(du[i] - lo[i], c->ipm_thr0); tu[i] = R_FMAX(hi[i] - du[i], c->ipm_thr0);
                ll[i] = c->ipm_mu0 / tl[i]; lu[i] = c->ipm_mu0 / tu[i];
            }
            alpha_prev = 1;
            goto residuals;
        }
        real M[NMAX][NMAX], invd[NMAX];
        real Dl[NMAX], Du[NMAX], da[NMAX], dtl[NMAX], dtu[NMAX], dll[NMAX], dlu[NMAX];
        for (int i = 0; i < n; ++i) {
            Dl[i] = ll[i] / tl[i]; Du[i] = lu[i] / tu[i];
            for (int j = 0; j <= i; ++j) M[i][j] = H[i][j];
            M[i][i] += Dl[i] + Du[i];
        }
        if (!chol(n, M, invd)) { *iters = it; return 4; }
        /* predictor (sigma = 0) */
        for (int i = 0; i < n; ++i) da[i] = -rs[i] + (-ll[i] - Dl[i] * rl[i]) - (-lu[i] - Du[i] * ru[i]);
        chol_solve(n, M, invd, da);
        real amax = 1, muaff = 0;
        for (int i = 0; i < n; ++i) {
            dtl[i] = da[i] + rl[i]; dtu[i] = -da[i] + ru[i];
            dll[i] = -ll[i] - Dl[i] * dtl[i]; dlu[i] = -lu[i] - Du[i] * dtu[i];
            if (dtl[i] < 0) amax = R_FMIN(amax, -tl[i] / dtl[i]);
            if (dtu[i] < 0) amax = R_FMIN(amax, -tu[i] / dtu[i]);
            if (dll[i] < 0) amax = R_FMIN(amax, -ll[i] / dll[i]);
            if (dlu[i] < 0) amax = R_FMIN(amax, -lu[i] / dlu[i]);
        }
        for (int i = 0; i < n; ++i) muaff += (tl[i] + amax * dtl[i]) * (ll[i] + amax * dll[i]) + (tu[i] + amax * dtu[i]) * (lu[i] + amax * dlu[i]);
        muaff /= 2 * n;
        real sigma = muaff / mu; sigma = sigma * sigma * sigma;
        if (alpha_prev < ADMPC_QUAD_IPM_BLOCKED_STEP) sigma = 1;              /* blocked step: centre (admpc_quad.h) */
        const real smu = sigma * mu;
        /* corrector: complementarity target  sigma mu - dt_aff dlam_aff */
        real d[NMAX], cl[NMAX], cu[NMAX];
        for (int i = 0; i < n; ++i) {
            cl[i] = (smu - (cons ? 0 : dtl[i] * dll[i])) / tl[i]; cu[i] = (smu - (cons ? 0 : dtu[i] * dlu[i])) / tu[i];
            d[i] = -rs[i] + (cl[i] - ll[i] - Dl[i] * rl[i]) - (cu[i] - lu[i] - Du[i] * ru[i]);
        }
        chol_solve(n, M, invd, d);
        amax = 1;
        for (int i = 0; i < n; ++i) {
            dtl[i] = d[i] + rl[i]; dtu[i] = -d[i] + ru[i];
            dll[i] = cl[i] - ll[i] - Dl[i] * dtl[i]; dlu[i] = cu[i] - lu[i] - Du[i] * dtu[i];
            if (dtl[i] < 0) amax = R_FMIN(amax, -tl[i] / dtl[i]);
            if (dtu[i] < 0) amax = R_FMIN(amax, -tu[i] / dtu[i]);
            if (dll[i] < 0) amax = R_FMIN(amax, -ll[i] / dll[i]);
            if (dlu[i] < 0) amax = R_FMIN(amax, -lu[i] / dlu[i]);
        }
        real tau = 1 - muaff; tau = R_FMAX(tau, 0.995); tau = R_FMIN(tau, 0.999999);
        const real alpha = R_FMIN(tau * amax, 1.0);
        for (int i = 0; i < n; ++i) {
            du[i] += alpha * d[i];
            tl[i] = R_FMAX(tl[i] + alpha * dtl[i], 1e-40); tu[i] = R_FMAX(tu[i] + alpha * dtu[i], 1e-40);
            ll[i] = R_FMAX(ll[i] + alpha * dll[i], 1e-40); lu[i] = R_FMAX(lu[i] + alpha * dlu[i], 1e-40);
        }
        alpha_prev = alpha;
    }
    *iters = it;
    return 0;
}

/* gp_state: the GP state of the first node (run_optimization's gp_regression_state, :546-552; NULL: the initial state x0, its default) */
/* pi_out [N][13], m_out [N][4] (may be NULL): the multipliers of the QP just solved, as acados holds them for the next stopping test.
 * With full condensing the QP solver returns none for the dynamics: they follow from the adjoint recursion of the QP's stationarity in the
 * states, and the net multiplier of an input's box pair (lower minus upper) from its stationarity in the inputs:
 *   pi_{N-1} = We (x+_N - xref_N),   pi_{k-1} = Ts Q (x+_k - xref_k) + A_k' pi_k,   m_k = Ts R (u+_k - uref_k) + B_k' pi_k
 * (A_k, B_k of the linearisation the QP was built on; x+, u+ the iterate after the full step). */
static int rti_step(const Cfg* c, const real* x0, const real* yref, const real* yref_e, const real* gp_state, real* xbar, real* ubar, real* cost, int* iters,
                    double* H_out, double* g_out, real* pi_out, real* m_out)
{
    Work w;
    const int N = c->N, n = N * NU;
    for (int k = 0; k < N; ++k) {
        real phi[NX];
        rk4_sens(c, xbar + k * NX, ubar + k * NU, (k == 0 && c->n_gp > 0) ? (gp_state ? gp_state : x0) : 0, c->Ts, phi, &w.A[k][0][0], &w.B[k][0][0]);
        for (int i = 0; i < NX; ++i) w.b[k][i] = phi[i] - xbar[(k + 1) * NX + i];
    }
    condense(c, x0, yref, yref_e, xbar, ubar, &w);
    if (H_out) for (int i = 0; i < n; ++i) { for (int j = 0; j < n; ++j) H_out[i * n + j] = w.H[i][j]; g_out[i] = w.g[i]; }
    real lo[NMAX], hi[NMAX], du[NMAX];
    for (int i = 0; i < n; ++i) { lo[i] = c->lbu[i % NU] - ubar[i]; hi[i] = c->ubu[i % NU] - ubar[i]; }
    int st = box_qp(c, n, w.H, w.g, lo, hi, du, iters);
    /* expand + full step */
    real xn[(ADMPC_QUAD_MAX_N + 1) * NX], un[NMAX], dx[NX];
    for (int i = 0; i < NX; ++i) { dx[i] = x0[i] - xbar[i]; xn[i] = xbar[i] + dx[i]; }
    int bad = st != 0;
    real J = 0;
    for (int k = 0; k < N && !bad; ++k) {
        real dn[NX];
        for (int r = 0; r < NX; ++r) {
            real a = w.b[k][r];
            for (int cc = 0; cc < NX; ++cc) a += w.A[k][r][cc] * dx[cc];
            for (int m = 0; m < NU; ++m) a += w.B[k][r][m] * du[k * NU + m];
            dn[r] = a;
        }
        for (int m = 0; m < NU; ++m) { un[k * NU + m] = ubar[k * NU + m] + du[k * NU + m]; if (!(R_FABS(un[k * NU + m]) <= 1e300)) bad = 1; }
        for (int r = 0; r < NX; ++r) { dx[r] = dn[r]; xn[(k + 1) * NX + r] = xbar[(k + 1) * NX + r] + dn[r]; if (!(R_FABS(xn[(k + 1) * NX + r]) <= 1e300)) bad = 1; }
    }
    if (bad) { *cost = INFINITY; return 4; }
    for (int k = 0; k < N; ++k) {
        for (int cc = 0; cc < NX; ++cc) { const real e = xn[k * NX + cc] - yref[k * ADMPC_QUAD_NY + cc]; J += 0.5 * (real)c->Ts * c->W[cc] * e * e; }
        for (int m = 0; m < NU; ++m) { const real e = un[k * NU + m] - yref[k * ADMPC_QUAD_NY + NX + m]; J += 0.5 * (real)c->Ts * c->W[NX + m] * e * e; }
    }
    for (int cc = 0; cc < NX; ++cc) { const real e = xn[N * NX + cc] - yref_e[cc]; J += 0.5 * c->We[cc] * e * e; }
    memcpy(xbar, xn, sizeof(real) * (N + 1) * NX); memcpy(ubar, un, sizeof(real) * n);
    *cost = J;
    if (pi_out) {
        real pk[NX];
        for (int i = 0; i < NX; ++i) pk[i] = c->We[i] * (xn[N * NX + i] - yref_e[i]);
        for (int k = N - 1; k >= 0; --k) {
            for (int i = 0; i < NX; ++i) pi_out[k * NX + i] = pk[i];
            for (int m = 0; m < NU; ++m) {
                real a = (real)c->Ts * c->W[NX + m] * (un[k * NU + m] - yref[k * ADMPC_QUAD_NY + NX + m]);
                for (int i = 0; i < NX; ++i) a += w.B[k][i][m] * pk[i];
                m_out[k * NU + m] = a;
            }
            if (k >= 1) {
                real pn[NX];
                for (int j = 0; j < NX; ++j) {
                    real a = (real)c->Ts * c->W[j] * (xn[k * NX + j] - yref[k * ADMPC_QUAD_NY + j]);
                    for (int i = 0; i < NX; ++i) a += w.A[k][i][j] * pk[i];
                    pn[j] = a;
                }
                memcpy(pk, pn, sizeof pk);
            }
        }
    }
    return 0;
}

/* acados' SQP stopping test (ocp_nlp_sqp.c / ocp_nlp_res_compute at the pinned commit 91a01d4c, requirements.txt:1; restated from the
 * published algorithm): inf-norms of the NLP's KKT residuals at the iterate (xbar, ubar) with the multipliers (pi, m) of the last QP --
 * res[0] stationarity, res[1] shooting defects (and x_0 - x0), res[2] violation of the input box, res[3] complementarity. */
static void quad_nlp_residuals(const Cfg* c, const real* x0, const real* yref, const real* yref_e, const real* gp_state,
                               const real* xbar, const real* ubar, const real* pi, const real* mm, real res[4])
{
    const int N = c->N;
    real rs = 0, re = 0, ri = 0, rc = 0;
#define UPN(acc, v) do { real a_ = R_FABS(v); if (a_ > acc || !(a_ == a_)) acc = a_; } while (0)
    for (int i = 0; i < NX; ++i) UPN(re, xbar[i] - x0[i]);
    for (int k = 0; k < N; ++k) {
        real phi[NX], A[NX][NX], Bm[NX][NU];
        rk4_sens(c, xbar + k * NX, ubar + k * NU, (k == 0 && c->n_gp > 0) ? (gp_state ? gp_state : x0) : 0, c->Ts, phi, &A[0][0], &Bm[0][0]);
        for (int i = 0; i < NX; ++i) UPN(re, phi[i] - xbar[(k + 1) * NX + i]);
        for (int m = 0; m < NU; ++m) {
            const real u = ubar[k * NU + m];
            real a = (real)c->Ts * c->W[NX + m] * (u - yref[k * ADMPC_QUAD_NY + NX + m]) - mm[k * NU + m];
            for (int i = 0; i < NX; ++i) a += Bm[i][m] * pi[k * NX + i];
            UPN(rs, a);
            const real vl = c->lbu[m] - u, vu = u - c->ubu[m];
            UPN(ri, vl > 0 ? vl : 0); UPN(ri, vu > 0 ? vu : 0);
            const real ml = mm[k * NU + m] > 0 ? mm[k * NU + m] : 0, mu_ = mm[k * NU + m] < 0 ? -mm[k * NU + m] : 0;
            UPN(rc, ml * (u - c->lbu[m])); UPN(rc, mu_ * (c->ubu[m] - u));
        }
        if (k >= 1)
            for (int j = 0; j < NX; ++j) {
                real a = (real)c->Ts * c->W[j] * (xbar[k * NX + j] - yref[k * ADMPC_QUAD_NY + j]) - pi[(k - 1) * NX + j];
                for (int i = 0; i < NX; ++i) a += A[i][j] * pi[k * NX + i];
                UPN(rs, a);
            }
    }
    for (int j = 0; j < NX; ++j) UPN(rs, c->We[j] * (xbar[N * NX + j] - yref_e[j]) - pi[(N - 1) * NX + j]);
#undef UPN
    res[0] = rs; res[1] = re; res[2] = ri; res[3] = rc;
}

/* one instance's arguments in real (see to_real) */
typedef struct { real x0[NX], yref[ADMPC_QUAD_MAX_N * ADMPC_QUAD_NY], yref_e[NX], gs[NX], xbar[(ADMPC_QUAD_MAX_N + 1) * NX], ubar[NMAX]; const real* gp; } Inst;

static void load_inst(const Cfg* c, Inst* r, const double* x0, const double* yref, const double* yref_e, const double* gp_state, const double* xbar, const double* ubar)
{
    const int N = c->N;
    to_real(r->x0, x0, NX); to_real(r->yref, yref, N * ADMPC_QUAD_NY); to_real(r->yref_e, yref_e, NX);
    r->gp = to_real(r->gs, gp_state, NX);
    to_real(r->xbar, xbar, (N + 1) * NX); to_real(r->ubar, ubar, N * NU);
}

/* tests: the four residuals of an iterate with given multipliers */
int quad_oracle_nlp_residuals(const Cfg* c, const double* x0, const double* yref, const double* yref_e, const double* gp_state,
                              const double* xbar, const double* ubar, const double* pi, const double* mm, double* res)
{
    Inst r; real pr[ADMPC_QUAD_MAX_N * NX], mr[NMAX], rr[4];
    load_inst(c, &r, x0, yref, yref_e, gp_state, xbar, ubar);
    quad_nlp_residuals(c, r.x0, r.yref, r.yref_e, r.gp, r.xbar, r.ubar, to_real(pr, pi, c->N * NX), to_real(mr, mm, c->N * NU), rr);
    to_double(res, rr, 4);
    return 0;
}

/* x, u in place; returns the number of instances with a non-zero status */
int quad_oracle_solve_batch(const Cfg* c, int B, const double* x0, const double* yref, const double* yref_e, const double* gp_state,
                            double* xbar, double* ubar, double* cost, int32_t* status, int32_t* iters, int nthreads)
{
    const int N = c->N;
    int nbad = 0;
    (void)nthreads;
#ifdef _OPENMP
#pragma omp parallel for num_threads(nthreads > 0 ? nthreads : 1) reduction(+ : nbad) schedule(dynamic, 8)
#endif
    for (int b = 0; b < B; ++b) {
        int it = 0; real J = 0;
        /* cfg.sqp_iters > 1: that many SQP steps (solver_type "SQP", create_ros_gp_mpc.py:63-68); with cfg.sqp_tol > 0 acados' stopping test
         * in front of every QP but the first (a cold solver holds no multipliers: the first QP is always solved): converged -> status 0,
         * the limit reached -> status 2 (ACADOS_MAXITER, iterate valid), a non-finite QP -> status 4 at once */
        const int nsqp = c->sqp_iters > 1 ? c->sqp_iters : 1;
        const int tol_on = nsqp > 1 && c->sqp_tol > 0;
        real pi[ADMPC_QUAD_MAX_N * NX], mm[NMAX];
        Inst r;
        double* xb = xbar + (size_t)b * (N + 1) * NX; double* ub = ubar + (size_t)b * N * NU;
        load_inst(c, &r, x0 + (size_t)b * NX, yref + (size_t)b * N * ADMPC_QUAD_NY, yref_e + (size_t)b * NX, gp_state ? gp_state + (size_t)b * NX : 0, xb, ub);
        int st = 0;
        for (int sq = 0; sq < nsqp; ++sq) {
            if (tol_on && sq > 0) {
                real res[4];
                quad_nlp_residuals(c, r.x0, r.yref, r.yref_e, r.gp, r.xbar, r.ubar, pi, mm, res);
                if (res[0] <= c->sqp_tol && res[1] <= c->sqp_tol && res[2] <= c->sqp_tol && res[3] <= c->sqp_tol) { st = -1; break; }
            }
            st = rti_step(c, r.x0, r.yref, r.yref_e, r.gp, r.xbar, r.ubar, &J, &it, 0, 0, pi, mm);
            if (st != 0) break;
        }
        to_double(xb, r.xbar, (N + 1) * NX); to_double(ub, r.ubar, N * NU);
        if (tol_on) st = st == -1 ? 0 : (st == 0 ? 2 : st);
        if (cost) cost[b] = (double)J;
        if (status) status[b] = st;
        if (iters) iters[b] = it;
        nbad += st != 0;
    }
    return nbad;
}

/* the condensed QP of one instance (tests): H [n][n], g [n]; xbar / ubar receive the step as in quad_oracle_solve_batch */
int quad_oracle_qp_debug(const Cfg* c, const double* x0, const double* yref, const double* yref_e, double* xbar, double* ubar,
                         double* H, double* g, int32_t* iters)
{
    int it = 0; real J; Inst r;
    load_inst(c, &r, x0, yref, yref_e, 0, xbar, ubar);
    const int st = rti_step(c, r.x0, r.yref, r.yref_e, 0, r.xbar, r.ubar, &J, &it, H, g, 0, 0);
    to_double(xbar, r.xbar, (c->N + 1) * NX); to_double(ubar, r.ubar, c->N * NU);
    *iters = it;
    return st;
}
