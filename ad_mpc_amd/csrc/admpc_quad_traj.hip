// admpc_quad_traj.hip -- the loop and lemniscate references of the quadrotor's experiments generated on the device
// (include/admpc_quad_traj.h, which has the rule, the mapping and the scan's structure): two kernels and their host side.
//
//   admpc_quad_traj_gen_kernel    one work-group per trajectory, four passes over tiles of 256 rows; the intermediates live in the
//                                 output rows between the passes, the final rows leave through LDS in contiguous lanes
//   admpc_quad_traj_rows_kernel   the state (and input) row of every vehicle at its index: a gather, one thread per double written
#include <math.h>
#include <new>
#include "admpc_host.h"
#include "../../include/admpc_quad_traj.h"
#include "quad_sim_dev.h"     // QuadTrajDesc
#include "quad_traj_tail_dev.h"   // QuadTrajGenArgs, the scan of a tile, the passes B, C and D

namespace {

// alpha of row i (step 1); n: the five phase lengths
__device__ inline double alpha_of(int i, const int32_t* n, double a, double dt, int clockwise)
{
    const double q4 = 3.14159265358979323846 / 4.0;
    int p = 0, j = i;
    while (p < 4 && j >= n[p]) { j -= n[p]; ++p; }
    const double t = j * dt;
    double al;
    if (p == 0 || p == 4) { const double s = sin(q4 * t); al = a * (s * s); if (p == 4) al = al - a; }
    else if (p == 1) al = a;
    else if (p == 2) al = a * cos(q4 * t);
    else al = -a;
    return clockwise ? al : -al;
}

}  // namespace

__global__ __launch_bounds__(QT_THREADS) void admpc_quad_traj_gen_kernel(const QuadTrajDesc* desc, const AdmpcQuadTrajSpec* specs,
                                                                          const int32_t* lengths, int K, const QuadTrajGenArgs* gp, double* X, double* U)
{
    __shared__ double s_row[QT_THREADS * QT_ROW];
    __shared__ double s_tot[QT_WAVES];
    __shared__ double s_carry[2];
    const int tid = threadIdx.x;
    const double dt = gp->dt;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const AdmpcQuadTrajSpec sp = specs[k];
        const int32_t* n = lengths + (size_t)k * 5;
        const int M = desc[k].M;
        double* Xk = X + desc[k].off * QX;
        double* Uk = U + desc[k].off * QU;
        const int tiles = (M + QT_THREADS - 1) / QT_THREADS;
        const double a = sp.lin_acc / sp.radius, R = sp.radius;

        // ---- pass A: alpha, w, angle, the flat outputs, the attitude before the correction -----------------------------------------
        __syncthreads();                              // the previous trajectory's last reads of LDS are done
        if (tid < 2) s_carry[tid] = 0.0;
        __syncthreads();
        for (int tile = 0; tile < tiles; ++tile) {
            const int i = tile * QT_THREADS + tid;
            const bool live = i < M;
            const double al = live ? alpha_of(i, n, a, dt, sp.clockwise) : 0.0;
            const double w = tile_scan(al, s_tot, &s_carry[0]) * dt;
            const double ang = tile_scan(live ? w : 0.0, s_tot, &s_carry[1]) * dt;
            double* row = s_row + tid * QT_ROW;
            if (live) {
                const double s = sin(ang), c = cos(ang);
                double ax, ay;
                if (sp.kind == 0) {
                    row[0] = R * s; row[1] = R * c;
                    row[7] = R * w * c; row[8] = -(R * w * s);
                    ax = R * (al * c - w * w * s);
                    ay = -R * (al * s + w * w * c);
                }
                else {
                    row[0] = R * c; row[1] = R * (s * c);
                    row[7] = -R * (w * s); row[8] = R * (w * (c * c) - w * (s * s));
                    ax = -R * (al * s + w * w * c);
                    ay = R * (al * (c * c) - 2.0 * (w * w) * c * s - al * (s * s) - 2.0 * (w * w) * s * c);
                }
                row[2] = sp.z; row[9] = 0.0;
                const double az = QT_GRAVITY;
                const double nt = sqrt(ax * ax + ay * ay + az * az);
                const double zx = ax / nt, zy = ay / nt, zz = az / nt;
                const double ft = gp->mass * (zx * ax + zy * ay + zz * az);
                const double q0 = 0.5 * (1.0 + zz), q1 = 0.5 * -zy, q2 = 0.5 * zx, q3 = 0.0;
                const double nq = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
                row[3] = q0 / nq; row[4] = q1 / nq; row[5] = q2 / nq; row[6] = q3 / nq;
                row[10] = row[11] = row[12] = 0.0;
                row[13] = row[14] = row[15] = 0.0; row[16] = ft;
            }
            __syncthreads();                          // the tile's rows are in LDS
            const int r0 = tile * QT_THREADS, cnt = M - r0 < QT_THREADS ? M - r0 : QT_THREADS;
            for (int e = tid; e < cnt * QX; e += QT_THREADS) Xk[(size_t)r0 * QX + e] = s_row[(e / QX) * QT_ROW + e % QX];
            for (int e = tid; e < cnt * QU; e += QT_THREADS) Uk[(size_t)r0 * QU + e] = s_row[(e / QU) * QT_ROW + QX + e % QU];
            __syncthreads();                          // LDS may be written again; behind the last tile: q and f_t of every row are visible
        }

        // ---- passes B, C, D: the body rates under the yaw correction, the inputs, the final rows (quad_traj_tail_dev.h) ---------
        quad_traj_tail(M, dt, gp, Xk, Uk, s_row, s_tot, s_carry);
    }
}

__global__ __launch_bounds__(QT_THREADS) void admpc_quad_traj_rows_kernel(const QuadTrajDesc* __restrict__ desc, const double* __restrict__ X,
                                                                           const double* __restrict__ U, int K, int B,
                                                                           const int32_t* __restrict__ traj_of, const int32_t* __restrict__ idx,
                                                                           double* __restrict__ x, double* __restrict__ u)
{
    const int W = u ? QX + QU : QX;
    const long long total = (long long)B * W;
    for (long long t = (long long)blockIdx.x * QT_THREADS + threadIdx.x; t < total; t += (long long)gridDim.x * QT_THREADS) {
        const long long b = t / W;
        const int r = (int)(t - b * W);
        const int k = traj_of[b], i = idx[b];
        double val = __builtin_nan("");
        if (k >= 0 && k < K && i >= 0 && i < desc[k].M) {
            const long long row = desc[k].off + i;
            val = r < QX ? X[row * QX + r] : U[row * QU + (r - QX)];
        }
        if (r < QX) x[b * QX + r] = val; else u[b * QU + (r - QX)] = val;
    }
}

namespace {

const char* const GEN = "admpc_quad_traj_bank_generate";

bool positive(double v) { return v > 0.0 && isfinite(v); }

// the refusals of a spec and of dt one by one, so that a batch can raise them in the listed order
int spec_kind_check(const char* who, const AdmpcQuadTrajSpec& s)
{
    return (s.kind != 0 && s.kind != 1) ? admpc_refuse(who, "kind must be 0 (loop) or 1 (lemniscate)") : ADMPC_OK;
}
int spec_values_check(const char* who, const AdmpcQuadTrajSpec& s)
{
    if (s.clockwise != 0 && s.clockwise != 1) return admpc_refuse(who, "clockwise must be 0 or 1");
    if (!positive(s.radius) || !positive(s.z) || !positive(s.lin_acc) || !positive(s.v_max))
        return admpc_refuse(who, "radius, z, lin_acc and v_max must be positive and finite");
    return ADMPC_OK;
}
int dt_check(const char* who, double dt) { return positive(dt) ? ADMPC_OK : admpc_refuse(who, "dt must be positive and finite"); }

// numpy's arange rule for arange(0, stop, dt), in double; more rows than the cap are reported as the cap + 1
long long arange_len(double stop, double dt)
{
    const double len = ceil(stop / dt);
    if (!(len > 0.0)) return 0;
    return len > (double)ADMPC_QUAD_TRAJ_MAX_M ? (long long)ADMPC_QUAD_TRAJ_MAX_M + 1 : (long long)len;
}

// the five lengths of a checked spec; returns M (past the cap: something above it)
long long phase_lengths(double dt, const AdmpcQuadTrajSpec& s, int32_t n[5])
{
    const double t_total = 2.0 * s.v_max / s.lin_acc + 4.0;
    const double coasting = (t_total - 8.0) / 2.0;
    const double stop[5] = { 2.0, coasting, 4.0, coasting, 2.0 };
    long long M = 0;
    for (int p = 0; p < 5; ++p) { const long long l = arange_len(stop[p], dt); n[p] = (int32_t)l; M += l; }
    return M;
}
int coasting_check(const char* who, const int32_t n[5])
{
    return n[1] < 1 ? admpc_refuse(who, "the coasting phase is empty (v_max / lin_acc must be above 2)") : ADMPC_OK;
}
int cap_check(const char* who, long long M)
{
    return M > ADMPC_QUAD_TRAJ_MAX_M ? admpc_refuse(who, "more rows than ADMPC_QUAD_TRAJ_MAX_M") : ADMPC_OK;
}

// the inverse of [y_f; -x_f; z_l_tau; 1 1 1 1] by Gauss-Jordan elimination with partial pivoting; false: singular
bool arm_inverse(const AdmpcQuadPlantParams* p, double inv[16])
{
    double a[4][8];
    for (int c = 0; c < 4; ++c) { a[0][c] = p->y_f[c]; a[1][c] = -p->x_f[c]; a[2][c] = p->z_l_tau[c]; a[3][c] = 1.0; }
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) a[r][4 + c] = r == c ? 1.0 : 0.0;
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int r = col + 1; r < 4; ++r) if (fabs(a[r][col]) > fabs(a[piv][col])) piv = r;
        if (!(fabs(a[piv][col]) > 0.0) || !isfinite(a[piv][col])) return false;
        for (int c = 0; c < 8; ++c) { const double t = a[col][c]; a[col][c] = a[piv][c]; a[piv][c] = t; }
        const double d = a[col][col];
        for (int c = 0; c < 8; ++c) a[col][c] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double f = a[r][col];
            for (int c = 0; c < 8; ++c) a[r][c] -= f * a[col][c];
        }
    }
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { inv[r * 4 + c] = a[r][4 + c]; if (!isfinite(a[r][4 + c])) return false; }
    return true;
}

}  // namespace

// the refusals of the vehicle (mass, J, max_thrust, the arm matrix), in that order, and what a generator reads of it: admpc_quad_poly_traj.hip's too
int admpc_quad_traj_gen_args(const char* who, const AdmpcQuadPlantParams* plant, double dt, QuadTrajGenArgs* g)
{
    if (!positive(plant->mass) || !positive(plant->J[0]) || !positive(plant->J[1]) || !positive(plant->J[2]) || !positive(plant->max_thrust))
        return admpc_refuse(who, "the plant's mass, J and max_thrust must be positive and finite");
    g->dt = dt; g->mass = plant->mass; g->max_thrust = plant->max_thrust;
    for (int c = 0; c < 3; ++c) g->J[c] = plant->J[c];
    if (!arm_inverse(plant, g->ainv)) return admpc_refuse(who, "the arm matrix [y_f; -x_f; z_l_tau; 1] is singular");
    return ADMPC_OK;
}

extern "C" {

int admpc_quad_traj_lengths(double dt, const AdmpcQuadTrajSpec* spec, int32_t n[5])
{
    const char* who = "admpc_quad_traj_lengths";
    if (!spec || !n) return admpc_refuse(who, "null argument");
    int rc = spec_kind_check(who, *spec);
    if (!rc) rc = spec_values_check(who, *spec);
    if (!rc) rc = dt_check(who, dt);
    if (rc) return rc;
    int32_t l[5];
    const long long M = phase_lengths(dt, *spec, l);
    rc = coasting_check(who, l);
    if (!rc) rc = cap_check(who, M);
    if (rc) return rc;
    for (int p = 0; p < 5; ++p) n[p] = l[p];
    return ADMPC_OK;
}

int admpc_quad_traj_bank_generate(int device, int K, const AdmpcQuadTrajSpec* specs, const AdmpcQuadPlantParams* plant, double dt,
                                  void* stream, AdmpcQuadTrajBank** bank)
{
    if (!specs || !plant || !bank) return admpc_refuse(GEN, "null argument");
    if (K < 1) return admpc_refuse(GEN, "K must be at least 1");
    int rc = ADMPC_OK;
    for (int k = 0; k < K && !rc; ++k) rc = spec_kind_check(GEN, specs[k]);
    for (int k = 0; k < K && !rc; ++k) rc = spec_values_check(GEN, specs[k]);
    if (!rc) rc = dt_check(GEN, dt);
    if (rc) return rc;
    int32_t* len = new (std::nothrow) int32_t[(size_t)K * 5];
    int32_t* hM = new (std::nothrow) int32_t[K];
    QuadTrajDesc* desc = new (std::nothrow) QuadTrajDesc[K];
    AdmpcQuadTrajBank* b = new (std::nothrow) AdmpcQuadTrajBank();
    struct Hold {                                      // the host arrays of this call; the bank owns hM once it is returned
        int32_t *len, *hM; QuadTrajDesc* desc; AdmpcQuadTrajBank* b;
        ~Hold() { delete[] len; delete[] hM; delete[] desc; if (b) { if (b->d_mem) (void)hipFree(b->d_mem); delete b; } }
    } hold = { len, hM, desc, b };
    if (!len || !hM || !desc || !b) return admpc_set_error(ADMPC_ENOMEM, "out of host memory");
    long long rows = 0;
    for (int k = 0; k < K && !rc; ++k) {
        (void)phase_lengths(dt, specs[k], len + (size_t)k * 5);
        rc = coasting_check(GEN, len + (size_t)k * 5);
    }
    for (int k = 0; k < K && !rc; ++k) {
        long long M = 0;
        for (int p = 0; p < 5; ++p) M += len[(size_t)k * 5 + p];
        rc = cap_check(GEN, M);
        desc[k].off = rows; desc[k].M = (int32_t)M; desc[k].pad = 0; hM[k] = (int32_t)M;
        rows += M;
    }
    if (rc) return rc;
    QuadTrajGenArgs g;
    rc = admpc_quad_traj_gen_args(GEN, plant, dt, &g);
    if (rc) return rc;
    rc = admpc_device_check(device);
    if (rc) return rc;
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    const size_t nd = (size_t)K * sizeof(QuadTrajDesc), nx = (size_t)rows * QX * sizeof(double), nu = (size_t)rows * QU * sizeof(double);
    const size_t ng = sizeof(QuadTrajGenArgs), ns = (size_t)K * sizeof(AdmpcQuadTrajSpec), nl = (size_t)K * 5 * sizeof(int32_t);
    b->device = device; b->K = K; b->rows = rows; b->d_mem = nullptr; b->h_M = nullptr;
    if (hipMalloc(&b->d_mem, nd + nx + nu + ng + ns + nl) != hipSuccess) { b->d_mem = nullptr; return admpc_set_error(ADMPC_EHIP, "admpc_quad_traj_bank_generate: device allocation failed"); }
    char* base = (char*)b->d_mem;
    b->d_desc = (const QuadTrajDesc*)base; b->d_X = (const double*)(base + nd); b->d_U = (const double*)(base + nd + nx);
    const QuadTrajGenArgs* d_g = (const QuadTrajGenArgs*)(base + nd + nx + nu);
    const AdmpcQuadTrajSpec* d_specs = (const AdmpcQuadTrajSpec*)(base + nd + nx + nu + ng);
    const int32_t* d_len = (const int32_t*)(base + nd + nx + nu + ng + ns);
    if (hipMemcpy(base, desc, nd, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy((void*)d_g, &g, ng, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy((void*)d_specs, specs, ns, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((void*)d_len, len, nl, hipMemcpyHostToDevice) != hipSuccess)
        return admpc_set_error(ADMPC_EHIP, "admpc_quad_traj_bank_generate: upload failed");
    const int grid = K < QT_GRID ? K : QT_GRID;
    hipLaunchKernelGGL(admpc_quad_traj_gen_kernel, dim3((unsigned)grid), dim3(QT_THREADS), 0, (hipStream_t)stream, b->d_desc, d_specs, d_len, K, d_g,
                       (double*)b->d_X, (double*)b->d_U);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_traj_gen_kernel: launch failed");
    b->h_M = hM;
    hold.hM = nullptr; hold.b = nullptr;
    *bank = b;
    return ADMPC_OK;
}

int admpc_quad_traj_bank_info(const AdmpcQuadTrajBank* bank, int* K, int64_t* rows, int32_t* M)
{
    if (!bank) return admpc_refuse("admpc_quad_traj_bank_info", "null bank");
    if (K) *K = bank->K;
    if (rows) *rows = bank->rows;
    if (M) for (int k = 0; k < bank->K; ++k) M[k] = bank->h_M[k];
    return ADMPC_OK;
}

int admpc_quad_traj_bank_copy(const AdmpcQuadTrajBank* bank, int k, double* traj_host, double* u_host)
{
    if (!bank) return admpc_refuse("admpc_quad_traj_bank_copy", "null bank");
    if (k < 0 || k >= bank->K) return admpc_refuse("admpc_quad_traj_bank_copy", "k must be in [0, K)");
    DeviceGuard guard(bank->device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    long long off = 0;
    for (int m = 0; m < k; ++m) off += bank->h_M[m];
    const size_t M = (size_t)bank->h_M[k];
    bool ok = hipDeviceSynchronize() == hipSuccess;
    if (ok && traj_host) ok = hipMemcpy(traj_host, bank->d_X + (size_t)off * QX, M * QX * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    if (ok && u_host) ok = hipMemcpy(u_host, bank->d_U + (size_t)off * QU, M * QU * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    return ok ? ADMPC_OK : admpc_set_error(ADMPC_EHIP, "admpc_quad_traj_bank_copy: synchronise or copy failed");
}

int admpc_quad_traj_rows_batch(const AdmpcQuadTrajBank* bank, int B, const int32_t* traj_of, const int32_t* idx, double* x, double* u,
                               void* stream)
{
    const char* who = "admpc_quad_traj_rows_batch";
    if (!bank) return admpc_refuse(who, "null bank");
    if (B < 0) return admpc_refuse(who, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!traj_of || !idx || !x) return admpc_refuse(who, "null array argument");
    DeviceGuard guard(bank->device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    const long long total = (long long)B * (u ? QX + QU : QX);
    const long long nblk = (total + QT_THREADS - 1) / QT_THREADS;
    const int grid = (int)(nblk < 4096 ? nblk : 4096);
    hipLaunchKernelGGL(admpc_quad_traj_rows_kernel, dim3((unsigned)grid), dim3(QT_THREADS), 0, (hipStream_t)stream, bank->d_desc, bank->d_X, bank->d_U,
                       bank->K, B, traj_of, idx, x, u);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_traj_rows_kernel: launch failed");
    return ADMPC_OK;
}

}  // extern "C"
