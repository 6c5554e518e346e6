// admpc_quad_poly_traj.hip -- reference trajectories through keyframes generated on the device (include/admpc_quad_poly_traj.h, which
// has the rule, the mapping and the refusals): the reference's random_trajectory and straight_trajectory behind their keyframes.
//
//   admpc_quad_poly_traj_gen_kernel   one work-group per trajectory: the coefficients c = W p into LDS, pass A' over tiles of 256 rows
//                                     (the segment's polynomial and its two derivatives by Horner, the attitude from the thrust), then
//                                     the passes B, C, D of quad_traj_tail_dev.h, the text the loop generator runs
// The host side computes the lengths and W (Gauss-Jordan in long double) and returns an AdmpcQuadTrajBank like admpc_quad_traj.hip's.
#include <math.h>
#include <new>
#include "admpc_host.h"
#include "../../include/admpc_quad_poly_traj.h"
#include "quad_sim_dev.h"     // QuadTrajDesc
#include "quad_traj_tail_dev.h"   // QuadTrajGenArgs, the passes B, C and D

#define QP_MIN_KEYS ADMPC_QUAD_POLY_TRAJ_MIN_KEYS
#define QP_MAX_KEYS ADMPC_QUAD_POLY_TRAJ_MAX_KEYS
#define QP_MAX_SEG (QP_MAX_KEYS - 1)
#define QP_MAX_UNK (8 * QP_MAX_SEG)      // unknowns of the fit per axis at most

namespace {

// t1 and compress of row j of segment seg (step 2), every operation rounded by itself as numpy rounds it
__device__ inline double poly_t1(int seg, int j, double T, double dt, double* compress)
{
#pragma clang fp contract(off)
    const double t0 = seg * T, tn = (seg + 1) * T;
    const double tau = t0 + j * dt;
    *compress = 2.0 / (tn - t0);
    return (tau - t0) / (tn - t0) * 2.0 - 1.0;
}

// position, velocity and acceleration of one axis at t1 (step 3); c: the segment's 8 coefficients of that axis, ascending powers, stride 3
__device__ inline void poly_eval(const double* c, double t1, double compress, double* p, double* v, double* a)
{
#pragma clang fp contract(off)
    double y0 = c[7 * 3], y1 = c[7 * 3] * 7.0, y2 = (c[7 * 3] * 7.0) * 6.0;
    for (int pw = 6; pw >= 0; --pw) {                // pw: the power of the coefficient that joins position's Horner
        const double cc = c[pw * 3];
        y0 = y0 * t1 + cc;
        if (pw >= 1) y1 = y1 * t1 + cc * (double)pw;
        if (pw >= 2) y2 = y2 * t1 + (cc * (double)pw) * (double)(pw - 1);
    }
    *p = y0;
    *v = y1 * compress;
    *a = y2 * (compress * compress);
}

}  // namespace

__global__ __launch_bounds__(QT_THREADS) void admpc_quad_poly_traj_gen_kernel(const QuadTrajDesc* desc, const double* W, const double* keys,
                                                                               const int32_t* seg_rows, int n_key, int K,
                                                                               const QuadTrajGenArgs* gp, double* X, double* U)
{
    __shared__ double s_row[QT_THREADS * QT_ROW];
    __shared__ double s_c[QP_MAX_UNK * 3];
    __shared__ double s_tot[QT_WAVES];
    __shared__ double s_carry[1];
    const int tid = threadIdx.x;
    const double dt = gp->dt;
    const int n_seg = n_key - 1;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const int M = desc[k].M, s = seg_rows[k];
        double* Xk = X + desc[k].off * QX;
        double* Uk = U + desc[k].off * QU;
        const double* pk = keys + (size_t)k * n_key * 3;
        const int tiles = (M + QT_THREADS - 1) / QT_THREADS;
        const double T = s * dt;

        // ---- the coefficients: c[8 seg + a][axis] = sum over the keyframes, in index order ----------------------------------------------
        __syncthreads();                              // the previous trajectory's last reads of LDS are done
        for (int e = tid; e < 8 * n_seg * 3; e += QT_THREADS) {
            const int r = e / 3, ax = e - r * 3;
            const double* w = W + (size_t)r * n_key;
            double acc = w[0] * pk[ax];
            for (int m = 1; m < n_key; ++m) acc += w[m] * pk[m * 3 + ax];
            s_c[e] = acc;
        }
        __syncthreads();                              // the coefficients are in LDS

        // ---- pass A': the polynomial and its derivatives, the attitude before the correction ---------------------------------------------
        for (int tile = 0; tile < tiles; ++tile) {
            const int i = tile * QT_THREADS + tid;
            double* row = s_row + tid * QT_ROW;
            if (i < M) {
                int seg = i / s;
                if (seg > n_seg - 1) seg = n_seg - 1;   // the last row: j = s of the last segment
                const int j = i - seg * s;
                double compress, pos[3], vel[3], acc[3];
                const double t1 = poly_t1(seg, j, T, dt, &compress);
                for (int ax = 0; ax < 3; ++ax) poly_eval(s_c + seg * 24 + ax, t1, compress, &pos[ax], &vel[ax], &acc[ax]);
                const double ax = acc[0], ay = acc[1], az = acc[2] + QT_GRAVITY;
                const double nt = sqrt(ax * ax + ay * ay + az * az);
                const double zx = ax / nt, zy = ay / nt, zz = az / nt;
                const double ft = gp->mass * (zx * ax + zy * ay + zz * az);
                const double q0 = 0.5 * (1.0 + zz), q1 = 0.5 * -zy, q2 = 0.5 * zx, q3 = 0.0;
                const double nq = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
                row[0] = pos[0]; row[1] = pos[1]; row[2] = pos[2];
                row[3] = q0 / nq; row[4] = q1 / nq; row[5] = q2 / nq; row[6] = q3 / nq;
                row[7] = vel[0]; row[8] = vel[1]; row[9] = vel[2];
                row[10] = row[11] = row[12] = 0.0;
                row[13] = row[14] = row[15] = 0.0; row[16] = ft;
            }
            __syncthreads();                          // the tile's rows are in LDS
            const int r0 = tile * QT_THREADS, cnt = M - r0 < QT_THREADS ? M - r0 : QT_THREADS;
            for (int e = tid; e < cnt * QX; e += QT_THREADS) Xk[(size_t)r0 * QX + e] = s_row[(e / QX) * QT_ROW + e % QX];
            for (int e = tid; e < cnt * QU; e += QT_THREADS) Uk[(size_t)r0 * QU + e] = s_row[(e / QU) * QT_ROW + QX + e % QU];
            __syncthreads();                          // LDS may be written again; behind the last tile: q and f_t of every row are visible
        }

        // ---- passes B, C, D: the body rates under the yaw correction, the inputs, the final rows (quad_traj_tail_dev.h) -------------
        quad_traj_tail(M, dt, gp, Xk, Uk, s_row, s_tot, s_carry);
    }
}

namespace {

const char* const GEN = "admpc_quad_poly_traj_bank_generate";

bool positive(double v) { return v > 0.0 && isfinite(v); }

// the refusals one by one, so that a batch can raise each over all K trajectories before the next
int keys_count_check(const char* who, int n_key)
{
    return (n_key < QP_MIN_KEYS || n_key > QP_MAX_KEYS) ? admpc_refuse(who, "n_key must be in [3, 32]") : ADMPC_OK;
}
int keys_finite_check(const char* who, int n_key, const double* keys)
{
    for (int e = 0; e < n_key * 3; ++e) if (!isfinite(keys[e])) return admpc_refuse(who, "a keyframe coordinate is not finite");
    return ADMPC_OK;
}
int speed_check(const char* who, double speed) { return positive(speed) ? ADMPC_OK : admpc_refuse(who, "speed must be positive and finite"); }
int dt_check(const char* who, double dt)
{
    if (!positive(dt)) return admpc_refuse(who, "dt must be positive and finite");
    return dt < ADMPC_QUAD_POLY_TRAJ_MIN_DT ? admpc_refuse(who, "dt must be at least 1e-3") : ADMPC_OK;
}

// np.add.reduce of n doubles (n < 128): numpy's pairwise sum, eight running sums over blocks of eight, the rest added serially
double numpy_sum(const double* a, int n)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r[8];
    for (int c = 0; c < 8; ++c) r[c] = a[c];
    int i = 8;
    for (; i < n - n % 8; i += 8) for (int c = 0; c < 8; ++c) r[c] += a[i + c];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

// s of checked keyframes, speed and dt as a double (it may be 0 or huge): round-half-even(mean distance / speed / dt)
double seg_rows_of(double dt, int n_key, const double* keys, double speed)
{
    double d[QP_MAX_SEG];
    for (int m = 0; m + 1 < n_key; ++m) {
        const double dx = keys[(m + 1) * 3] - keys[m * 3], dy = keys[(m + 1) * 3 + 1] - keys[m * 3 + 1], dz = keys[(m + 1) * 3 + 2] - keys[m * 3 + 2];
        d[m] = sqrt((dx * dx + dy * dy) + dz * dz);
    }
    const double av_dist = numpy_sum(d, n_key - 1) / (double)(n_key - 1);
    const double av_dt = av_dist / speed;
    return nearbyint(av_dt / dt);                     // the default rounding mode: to nearest, ties to even
}
int seg_rows_check(const char* who, double s) { return !(s >= 1.0) ? admpc_refuse(who, "s < 1: less than one row per segment (speed * dt above the mean keyframe distance)") : ADMPC_OK; }
// M of s >= 1; past the cap: something above it
long long rows_of(int n_key, double s)
{
    if (s > (double)ADMPC_QUAD_TRAJ_MAX_M) return (long long)ADMPC_QUAD_TRAJ_MAX_M + 1;
    return (long long)(n_key - 1) * (long long)s + 1;
}
int cap_check(const char* who, long long M)
{
    return M > ADMPC_QUAD_TRAJ_MAX_M ? admpc_refuse(who, "more rows than ADMPC_QUAD_TRAJ_MAX_M") : ADMPC_OK;
}

// row `d` of matrix_generation(ts), ts = +1 or -1: the d-th derivative of the monomials 1, t, .., t^7 at ts
void monomial_row(int d, double ts, long double row[8])
{
    for (int a = 0; a < 8; ++a) {
        if (a < d) { row[a] = 0.0L; continue; }
        long double f = 1.0L;
        for (int m = 0; m < d; ++m) f *= (long double)(a - m);
        row[a] = f * (((a - d) & 1) ? (long double)ts : 1.0L);
    }
}

// W = multiple_waypoints(n_seg)^-1 S, S the scatter of rhs_generation, by Gauss-Jordan elimination with partial pivoting in long double on
// [M_fit | S]; false: out of memory or a pivot that is zero or not finite (it does not happen for n_key in [3, 32]: cond(M_fit) < 3e4)
bool fit_weights(int n_key, double* W)
{
    const int n = n_key - 1, N = 8 * n, C = N + n_key;
    long double* a = new (std::nothrow) long double[(size_t)N * C];
    if (!a) return false;
    for (size_t e = 0; e < (size_t)N * C; ++e) a[e] = 0.0L;
    long double row[8];
    auto put = [&](int r, int seg, int d, double ts, long double sign) {
        monomial_row(d, ts, row);
        for (int c = 0; c < 8; ++c) a[(size_t)r * C + 8 * seg + c] = sign * row[c];
    };
    for (int d = 0; d < 4; ++d) put(d, 0, d, -1.0, 1.0L);                          // the start: position and three derivatives at -1
    for (int i = 0; i < n - 1; ++i) {
        for (int d = 0; d < 7; ++d) put(8 * i + 4 + d, i, d, 1.0, 1.0L);           // segment i at +1: position, derivatives 1 .. 6
        for (int d = 1; d < 7; ++d) put(8 * i + 4 + d, i + 1, d, -1.0, -1.0L);     // minus the derivatives of segment i + 1 at -1
        put(8 * i + 11, i + 1, 0, -1.0, 1.0L);                                     // segment i + 1 starts at the keyframe
    }
    for (int d = 0; d < 4; ++d) put(8 * (n - 1) + 4 + d, n - 1, d, 1.0, 1.0L);     // the end: position and three derivatives at +1
    a[(size_t)0 * C + N + 0] = 1.0L;
    a[(size_t)(N - 4) * C + N + n] = 1.0L;
    for (int i = 1; i < n; ++i) { a[(size_t)(8 * (i - 1) + 4) * C + N + i] = 1.0L; a[(size_t)(8 * (i - 1) + 11) * C + N + i] = 1.0L; }
    bool ok = true;
    for (int col = 0; col < N && ok; ++col) {
        int piv = col;
        for (int r = col + 1; r < N; ++r) if (fabsl(a[(size_t)r * C + col]) > fabsl(a[(size_t)piv * C + col])) piv = r;
        const long double d = a[(size_t)piv * C + col];
        if (!(fabsl(d) > 0.0L) || !isfinite((double)d)) { ok = false; break; }
        if (piv != col) for (int c = 0; c < C; ++c) { const long double t = a[(size_t)col * C + c]; a[(size_t)col * C + c] = a[(size_t)piv * C + c]; a[(size_t)piv * C + c] = t; }
        for (int c = 0; c < C; ++c) a[(size_t)col * C + c] /= d;
        for (int r = 0; r < N; ++r) {
            if (r == col) continue;
            const long double f = a[(size_t)r * C + col];
            if (f == 0.0L) continue;
            for (int c = 0; c < C; ++c) a[(size_t)r * C + c] -= f * a[(size_t)col * C + c];
        }
    }
    for (int r = 0; r < N && ok; ++r) for (int m = 0; m < n_key; ++m) {
        W[(size_t)r * n_key + m] = (double)a[(size_t)r * C + N + m];
        if (!isfinite(W[(size_t)r * n_key + m])) ok = false;
    }
    delete[] a;
    return ok;
}

}  // namespace

extern "C" {

int admpc_quad_poly_traj_lengths(double dt, int n_key, const double* keys, double speed, int32_t* s, int32_t* M)
{
    const char* who = "admpc_quad_poly_traj_lengths";
    if (!keys || !s || !M) return admpc_refuse(who, "null argument");
    int rc = keys_count_check(who, n_key);
    if (!rc) rc = keys_finite_check(who, n_key, keys);
    if (!rc) rc = speed_check(who, speed);
    if (!rc) rc = dt_check(who, dt);
    if (rc) return rc;
    const double sd = seg_rows_of(dt, n_key, keys, speed);
    rc = seg_rows_check(who, sd);
    if (rc) return rc;
    const long long rows = rows_of(n_key, sd);
    rc = cap_check(who, rows);
    if (rc) return rc;
    *s = (int32_t)sd; *M = (int32_t)rows;
    return ADMPC_OK;
}

int admpc_quad_poly_traj_weights(int n_key, double* W)
{
    const char* who = "admpc_quad_poly_traj_weights";
    if (!W) return admpc_refuse(who, "null argument");
    const int rc = keys_count_check(who, n_key);
    if (rc) return rc;
    return fit_weights(n_key, W) ? ADMPC_OK : admpc_set_error(ADMPC_ENOMEM, "admpc_quad_poly_traj_weights: the elimination failed");
}

int admpc_quad_poly_traj_bank_generate(int device, int K, int n_key, const double* keys_host, const double* speed_host,
                                       const AdmpcQuadPlantParams* plant, double dt, void* stream, AdmpcQuadTrajBank** bank)
{
    if (!keys_host || !speed_host || !plant || !bank) return admpc_refuse(GEN, "null argument");
    if (K < 1) return admpc_refuse(GEN, "K must be at least 1");
    int rc = keys_count_check(GEN, n_key);
    for (int k = 0; k < K && !rc; ++k) rc = keys_finite_check(GEN, n_key, keys_host + (size_t)k * n_key * 3);
    for (int k = 0; k < K && !rc; ++k) rc = speed_check(GEN, speed_host[k]);
    if (!rc) rc = dt_check(GEN, dt);
    if (rc) return rc;
    const size_t nW = (size_t)8 * (n_key - 1) * n_key;
    int32_t* seg = new (std::nothrow) int32_t[K];
    int32_t* hM = new (std::nothrow) int32_t[K];
    QuadTrajDesc* desc = new (std::nothrow) QuadTrajDesc[K];
    double* W = new (std::nothrow) double[nW];
    AdmpcQuadTrajBank* b = new (std::nothrow) AdmpcQuadTrajBank();
    struct Hold {                                      // the host arrays of this call; the bank owns hM once it is returned
        int32_t *seg, *hM; QuadTrajDesc* desc; double* W; AdmpcQuadTrajBank* b;
        ~Hold() { delete[] seg; delete[] hM; delete[] desc; delete[] W; if (b) { if (b->d_mem) (void)hipFree(b->d_mem); delete b; } }
    } hold = { seg, hM, desc, W, b };
    if (!seg || !hM || !desc || !W || !b) return admpc_set_error(ADMPC_ENOMEM, "out of host memory");
    for (int k = 0; k < K && !rc; ++k) {
        const double sd = seg_rows_of(dt, n_key, keys_host + (size_t)k * n_key * 3, speed_host[k]);
        rc = seg_rows_check(GEN, sd);
        seg[k] = sd > (double)ADMPC_QUAD_TRAJ_MAX_M ? ADMPC_QUAD_TRAJ_MAX_M + 1 : (int32_t)sd;
    }
    long long rows = 0;
    for (int k = 0; k < K && !rc; ++k) {
        const long long M = rows_of(n_key, (double)seg[k]);
        rc = cap_check(GEN, M);
        desc[k].off = rows; desc[k].M = (int32_t)M; desc[k].pad = 0; hM[k] = (int32_t)M;
        rows += M;
    }
    if (rc) return rc;
    QuadTrajGenArgs g;
    rc = admpc_quad_traj_gen_args(GEN, plant, dt, &g);
    if (rc) return rc;
    if (!fit_weights(n_key, W)) return admpc_set_error(ADMPC_ENOMEM, "admpc_quad_poly_traj_bank_generate: the elimination failed");
    rc = admpc_device_check(device);
    if (rc) return rc;
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    const size_t nd = (size_t)K * sizeof(QuadTrajDesc), nx = (size_t)rows * QX * sizeof(double), nu = (size_t)rows * QU * sizeof(double);
    const size_t ng = sizeof(QuadTrajGenArgs), nw = nW * sizeof(double), nk = (size_t)K * n_key * 3 * sizeof(double), ns = (size_t)K * sizeof(int32_t);
    b->device = device; b->K = K; b->rows = rows; b->d_mem = nullptr; b->h_M = nullptr;
    if (hipMalloc(&b->d_mem, nd + nx + nu + ng + nw + nk + ns) != hipSuccess) { b->d_mem = nullptr; return admpc_set_error(ADMPC_EHIP, "admpc_quad_poly_traj_bank_generate: device allocation failed"); }
    char* base = (char*)b->d_mem;
    b->d_desc = (const QuadTrajDesc*)base; b->d_X = (const double*)(base + nd); b->d_U = (const double*)(base + nd + nx);
    const QuadTrajGenArgs* d_g = (const QuadTrajGenArgs*)(base + nd + nx + nu);
    const double* d_W = (const double*)(base + nd + nx + nu + ng);
    const double* d_keys = (const double*)(base + nd + nx + nu + ng + nw);
    const int32_t* d_seg = (const int32_t*)(base + nd + nx + nu + ng + nw + nk);
    if (hipMemcpy(base, desc, nd, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy((void*)d_g, &g, ng, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((void*)d_W, W, nw, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy((void*)d_keys, keys_host, nk, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((void*)d_seg, seg, ns, hipMemcpyHostToDevice) != hipSuccess)
        return admpc_set_error(ADMPC_EHIP, "admpc_quad_poly_traj_bank_generate: upload failed");
    const int grid = K < QT_GRID ? K : QT_GRID;
    hipLaunchKernelGGL(admpc_quad_poly_traj_gen_kernel, dim3((unsigned)grid), dim3(QT_THREADS), 0, (hipStream_t)stream, b->d_desc, d_W, d_keys, d_seg,
                       n_key, K, d_g, (double*)b->d_X, (double*)b->d_U);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_poly_traj_gen_kernel: launch failed");
    b->h_M = hM;
    hold.hM = nullptr; hold.b = nullptr;
    *bank = b;
    return ADMPC_OK;
}

}  // extern "C"
