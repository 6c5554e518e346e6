// admpc_quad_fleet.hip -- the quadrotor's closed loop on the device (include/admpc_quad_fleet.h): two kernels and their host side.
//
//   admpc_quad_chunk_kernel   the reference window of every vehicle (get_reference_chunk + set_reference_trajectory's padding): a
//                             gather, one thread per double written, so the 17 doubles of a node row leave contiguous lanes
//   admpc_quad_plant_kernel   Quadrotor3D.update `substeps` times under one input (quad_3d.py:175-287): substeps x 4 evaluations of the
//                             simulator's model in a serial chain, ONE lane per vehicle (QP_LANES), everything in registers; behind a step
//                             of the rollout the same launch does the tally, the counts, the records and the index update
//
// The rollout (admpc_quad_rollout_batch) is T times chunk -> admpc_quad_solve_batch_ex -> plant on one stream.
#include <stdio.h>
#include <math.h>
#include <new>
#include "admpc_host.h"
#include "../../include/admpc_quad_fleet.h"

#define QX ADMPC_QUAD_NX
#define QU ADMPC_QUAD_NU
#define QY ADMPC_QUAD_NY
#define WAVE 64
#define QP_LANES 1             // lanes per vehicle of the plant kernel; four (a lane per state group) measured 1.40 times slower: profiles/HISTORY.md
#define QP_GRID 4096           // blocks of the plant kernel at most (the cap of admpc_plant_kernel); more vehicles go round the stride loop
#define QC_THREADS 256
#define QC_GRID 4096           // blocks of the chunk kernel at most
static_assert(QP_LANES == 1, "admpc_quad_plant_kernel maps one lane to one vehicle");

// one trajectory of a bank: its first row in the bank's row space and its length
struct QuadTrajDesc { long long off; int32_t M; int32_t pad; };

struct AdmpcQuadTrajBank {
    int device, K;
    long long rows;              // sum of M
    void* d_mem;                 // the one allocation: desc [K], X [rows][13], U [rows][4]
    const QuadTrajDesc* d_desc;
    const double *d_X, *d_U;
};

// what one launch of the plant kernel works on (by value); the rollout's pointers are null for a plant-only step
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

namespace {

// the thrusts' constants of a period: what f_vel and f_rate take from u (quad_3d.py:253, 284-286)
struct Thrust { double az, ty, tx, tz; };

// The vehicle constants a period reads, held in VECTOR registers: a gfx9 VALU instruction reads one scalar operand at most, and with the
// whole parameter block and the rollout's pointers live across the stride loop the scalar file ran over (14 SGPR spills in the first
// build; none now, 230 VGPRs, two waves per SIMD).  vreg() is an empty asm statement that pins its operand to a VGPR.
struct SimConst { double dt, half, mass, aero, rd[3], gz, iJ[3], dJ[3], xf[4], yf[4], zt[4], u_min, u_max, max_thrust; int drag; };
__device__ __forceinline__ double vreg(double v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ SimConst sim_const(const AdmpcQuadPlantParams& p)
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

// d/dt of [p, q, v, w] (quad_3d.py:222-287) at state s
__device__ __forceinline__ void quad_sim_f(const SimConst& c, const Thrust& th, const double (&s)[QX], double (&k)[QX])
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
    k[7] = dx + r02 * th.az;                                                                 // f_vel
    k[8] = dy + r12 * th.az;
    k[9] = (c.gz + dz) + r22 * th.az;
    k[10] = c.iJ[0] * (th.ty + c.dJ[0] * w1 * w2);                                           // f_rate
    k[11] = c.iJ[1] * (-th.tx + c.dJ[1] * w2 * w0);
    k[12] = c.iJ[2] * (th.tz + c.dJ[2] * w0 * w1);
}

// one Quadrotor3D.update: classic RK4 with step dt, then unit_quat
__device__ __forceinline__ void quad_sim_update(const SimConst& c, const Thrust& th, double (&x)[QX])
{
    const double dt = c.dt, half = c.half;
    double k[QX], acc[QX], s[QX];
    quad_sim_f(c, th, x, k);
#pragma unroll
    for (int i = 0; i < QX; ++i) { acc[i] = 1.0 / 6.0 * k[i]; s[i] = x[i] + half * k[i]; }
    quad_sim_f(c, th, s, k);
#pragma unroll
    for (int i = 0; i < QX; ++i) { acc[i] += 2.0 / 6.0 * k[i]; s[i] = x[i] + half * k[i]; }
    quad_sim_f(c, th, s, k);
#pragma unroll
    for (int i = 0; i < QX; ++i) { acc[i] += 2.0 / 6.0 * k[i]; s[i] = x[i] + dt * k[i]; }
    quad_sim_f(c, th, s, k);
#pragma unroll
    for (int i = 0; i < QX; ++i) x[i] = x[i] + dt * (acc[i] + 1.0 / 6.0 * k[i]);
    const double inv = 1.0 / sqrt(((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]) + x[6] * x[6]);
    x[3] *= inv; x[4] *= inv; x[5] *= inv; x[6] *= inv;
}

// the sums of a rollout for one vehicle: every operation rounded on its own, so that numpy reproduces them bit for bit
__device__ __forceinline__ void quad_tally(const QuadPlantArgs& a, long long b, const double (&x)[QX], bool replaced)
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

}  // namespace

__global__ __launch_bounds__(WAVE) void admpc_quad_plant_kernel(const QuadPlantArgs a)
{
    const SimConst c = sim_const(a.p);
    for (long long b = (long long)blockIdx.x * WAVE + threadIdx.x; b < a.B; b += (long long)gridDim.x * WAVE) {
        double x[QX];
        double* xb = a.x + b * QX;
#pragma unroll
        for (int i = 0; i < QX; ++i) x[i] = xb[i];
        const double* ub = a.u + b * a.u_stride;
        double f[QU];
        bool replaced = false;
#pragma unroll
        for (int m = 0; m < QU; ++m) {
            const double raw = ub[m];
            if (a.u_out) a.u_out[b * QU + m] = raw;
            double v = raw < c.u_max ? raw : c.u_max;        // max(min(u, u_max), u_min)
            v = v > c.u_min ? v : c.u_min;
            if (!isfinite(raw)) { v = c.u_min; replaced = true; }
            f[m] = v * c.max_thrust;
        }
        if (a.tally) quad_tally(a, b, x, replaced);          // the error at the START of the step
        if (a.traj_pre) {
#pragma unroll
            for (int i = 0; i < QX; ++i) a.traj_pre[b * QX + i] = x[i];
        }
        Thrust th;
        th.az = (((f[0] + f[1]) + f[2]) + f[3]) / c.mass;
        th.ty = f[0] * c.yf[0] + f[1] * c.yf[1] + f[2] * c.yf[2] + f[3] * c.yf[3];
        th.tx = f[0] * c.xf[0] + f[1] * c.xf[1] + f[2] * c.xf[2] + f[3] * c.xf[3];
        th.tz = f[0] * c.zt[0] + f[1] * c.zt[1] + f[2] * c.zt[2] + f[3] * c.zt[3];
        for (int m = 0; m < a.p.substeps; ++m) quad_sim_update(c, th, x);
#pragma unroll
        for (int i = 0; i < QX; ++i) xb[i] = x[i];
        if (a.traj_post) {
#pragma unroll
            for (int i = 0; i < QX; ++i) a.traj_post[b * QX + i] = x[i];
        }
        if (a.idx) {                                          // idx <- min(idx + 1, M - 1) where the vehicle has a window
            const int k = a.traj_of[b];
            if (k >= 0 && k < a.K) {
                const int M = a.desc[k].M, i = a.idx[b];
                if (i >= 0 && i < M) a.idx[b] = i + 1 < M ? i + 1 : M - 1;
            }
        }
    }
}

__global__ __launch_bounds__(QC_THREADS) void admpc_quad_chunk_kernel(const QuadTrajDesc* __restrict__ desc, const double* __restrict__ X,
                                                                       const double* __restrict__ U, int K, int B, int N, int over,
                                                                       const int32_t* __restrict__ traj_of, const int32_t* __restrict__ idx,
                                                                       double* __restrict__ yref, double* __restrict__ yref_e,
                                                                       double* __restrict__ pos_ref)
{
    const int nyr = N * QY, W = nyr + QX + 3;                // doubles per vehicle: the window, the terminal row, the position
    const long long total = (long long)B * W;
    for (long long t = (long long)blockIdx.x * QC_THREADS + threadIdx.x; t < total; t += (long long)gridDim.x * QC_THREADS) {
        const long long b = t / W;
        const int r = (int)(t - b * W);
        const int k = traj_of[b], i = idx[b];
        bool ok = k >= 0 && k < K;
        long long off = 0, L = 1;
        if (ok) {
            const int M = desc[k].M;
            off = desc[k].off;
            ok = i >= 0 && i < M;
            if (ok) {
                L = ((long long)M - i + over - 1) / over;     // rows of the down-sampled window, at least 1
                if (L > N + 1) L = N + 1;
            }
        }
        double val = __builtin_nan("");
        if (r < nyr) {
            const int j = r / QY, col = r - j * QY;
            if (ok) {
                if (col < QX) { const long long jj = j < L - 1 ? j : L - 1; val = X[(off + i + jj * over) * QX + col]; }
                else { const long long last = L - 2 > 0 ? L - 2 : 0, jj = j < last ? j : last; val = U[(off + i + jj * over) * QU + (col - QX)]; }
            }
            yref[b * nyr + r] = val;
        }
        else if (r < nyr + QX) {
            const int col = r - nyr;
            if (ok) { const long long jj = N < L - 1 ? N : L - 1; val = X[(off + i + jj * over) * QX + col]; }
            yref_e[b * QX + col] = val;
        }
        else if (pos_ref) {
            const int col = r - nyr - QX;
            if (ok) val = X[(off + i) * QX + col];
            pos_ref[b * 3 + col] = val;
        }
    }
}

namespace {

int plant_params_check(const char* who, const AdmpcQuadPlantParams* p)
{
    char msg[160];
    const char* what = nullptr;
    if (!p) what = "the plant parameters are not set";
    else if (!(p->dt > 0) || !isfinite(p->dt)) what = "dt must be positive and finite";
    else if (p->substeps < 1 || p->substeps > 1024) what = "substeps must be in [1, 1024]";
    else if (!(p->mass > 0) || !(p->J[0] > 0 && p->J[1] > 0 && p->J[2] > 0)) what = "mass and J must be positive";
    else if (!(p->u_min <= p->u_max) || !isfinite(p->u_min) || !isfinite(p->u_max)) what = "u_min <= u_max, both finite, required";
    else if (p->drag != 0 && p->drag != 1) what = "drag must be 0 or 1";
    if (!what) return ADMPC_OK;
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return admpc_set_error(ADMPC_EINVAL, msg);
}

// one launch of the chunk kernel for checked arguments, B > 0, on the bank's device (the caller holds it)
int chunk_launch(const AdmpcQuadTrajBank* bank, int B, int N, int over, const int32_t* traj_of, const int32_t* idx, double* yref,
                 double* yref_e, double* pos_ref, hipStream_t st)
{
    const long long total = (long long)B * (N * QY + QX + 3);
    const long long nblk = (total + QC_THREADS - 1) / QC_THREADS;
    const int grid = (int)(nblk < QC_GRID ? nblk : QC_GRID);
    hipLaunchKernelGGL(admpc_quad_chunk_kernel, dim3((unsigned)grid), dim3(QC_THREADS), 0, st, bank->d_desc, bank->d_X, bank->d_U, bank->K, B, N, over,
                       traj_of, idx, yref, yref_e, pos_ref);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_chunk_kernel: launch failed");
    return ADMPC_OK;
}

// one launch of the plant kernel for filled arguments, B > 0
int plant_launch(const QuadPlantArgs& a, hipStream_t st)
{
    const int nblk = (a.B + WAVE - 1) / WAVE;
    const int grid = nblk < QP_GRID ? nblk : QP_GRID;
    hipLaunchKernelGGL(admpc_quad_plant_kernel, dim3((unsigned)grid), dim3(WAVE), 0, st, a);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_quad_plant_kernel: launch failed");
    return ADMPC_OK;
}

QuadPlantArgs plant_only(const AdmpcQuadPlantParams* plant, int B, const double* u, long long u_stride, double* x)
{
    QuadPlantArgs a;
    a.p = *plant; a.B = B; a.K = 0;
    a.u = u; a.u_stride = u_stride; a.x = x;
    a.yref = nullptr; a.yref_stride = 0; a.status = nullptr; a.tally = nullptr; a.counts = nullptr;
    a.traj_of = nullptr; a.idx = nullptr; a.desc = nullptr; a.traj_pre = a.traj_post = nullptr; a.u_out = nullptr;
    return a;
}

}  // namespace

// for admpc_quad_learn.hip: the refusals of the plant parameters
extern "C" int admpc_quad_plant_params_check(const char* who, const AdmpcQuadPlantParams* plant) { return plant_params_check(who, plant); }

extern "C" {

int admpc_quad_plant_step_batch(const AdmpcQuadPlantParams* plant, int device, int B, const double* u, int64_t u_stride, double* x,
                                void* stream)
{
    const int rc = plant_params_check("admpc_quad_plant_step_batch", plant);
    if (rc) return rc;
    if (B < 0) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_plant_step_batch: negative batch");
    if (B == 0) return ADMPC_OK;
    if (!u || !x) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_plant_step_batch: null array argument");
    if (u_stride < QU) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_plant_step_batch: u_stride must be at least 4");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return admpc_set_error(ADMPC_ENODEV, "no such device");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    return plant_launch(plant_only(plant, B, u, (long long)u_stride, x), (hipStream_t)stream);
}

int admpc_quad_traj_bank_create(int device, int K, const int32_t* M, const double* const* traj, const double* const* u,
                                AdmpcQuadTrajBank** bank)
{
    if (!M || !traj || !u || !bank) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_traj_bank_create: null argument");
    if (K < 1) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_traj_bank_create: K must be at least 1");
    long long rows = 0;
    for (int k = 0; k < K; ++k) {
        if (M[k] < 1) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_traj_bank_create: every trajectory needs M >= 1 rows");
        if (!traj[k] || !u[k]) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_traj_bank_create: null trajectory");
        rows += M[k];
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return admpc_set_error(ADMPC_ENODEV, "no HIP device");
    if (device < 0 || device >= ndev) return admpc_set_error(ADMPC_ENODEV, "no such device");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    AdmpcQuadTrajBank* b = new (std::nothrow) AdmpcQuadTrajBank();
    QuadTrajDesc* desc = new (std::nothrow) QuadTrajDesc[K];
    if (!b || !desc) { delete b; delete[] desc; return admpc_set_error(ADMPC_ENOMEM, "out of host memory"); }
    const size_t nd = (size_t)K * sizeof(QuadTrajDesc), nx = (size_t)rows * QX * sizeof(double), nu = (size_t)rows * QU * sizeof(double);
    b->device = device; b->K = K; b->rows = rows; b->d_mem = nullptr;
    bool ok = hipMalloc(&b->d_mem, nd + nx + nu) == hipSuccess;
    if (ok) {
        char* base = (char*)b->d_mem;
        b->d_desc = (const QuadTrajDesc*)base; b->d_X = (const double*)(base + nd); b->d_U = (const double*)(base + nd + nx);
        long long off = 0;
        for (int k = 0; k < K && ok; ++k) {
            desc[k].off = off; desc[k].M = M[k]; desc[k].pad = 0;
            ok = hipMemcpy(base + nd + (size_t)off * QX * sizeof(double), traj[k], (size_t)M[k] * QX * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(base + nd + nx + (size_t)off * QU * sizeof(double), u[k], (size_t)M[k] * QU * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
            off += M[k];
        }
        ok = ok && hipMemcpy(base, desc, nd, hipMemcpyHostToDevice) == hipSuccess;
    }
    delete[] desc;
    if (!ok) {
        if (b->d_mem) (void)hipFree(b->d_mem);
        delete b;
        return admpc_set_error(ADMPC_EHIP, "admpc_quad_traj_bank_create: device allocation or copy failed");
    }
    *bank = b;
    return ADMPC_OK;
}

void admpc_quad_traj_bank_destroy(AdmpcQuadTrajBank* bank)
{
    if (!bank) return;
    DeviceGuard guard(bank->device);
    if (bank->d_mem) (void)hipFree(bank->d_mem);
    delete bank;
}

int admpc_quad_ref_chunk_batch(const AdmpcQuadTrajBank* bank, int B, int N, int over, const int32_t* traj_of, const int32_t* idx,
                               double* yref, double* yref_e, double* pos_ref, void* stream)
{
    if (!bank) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_ref_chunk_batch: null bank");
    if (B < 0) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_ref_chunk_batch: negative batch");
    if (N < 2 || N > ADMPC_QUAD_MAX_N) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_ref_chunk_batch: N must be in [2, 24]");
    if (over < 1) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_ref_chunk_batch: over must be at least 1");
    if (B == 0) return ADMPC_OK;
    if (!traj_of || !idx || !yref || !yref_e) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_ref_chunk_batch: null array argument");
    DeviceGuard guard(bank->device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    return chunk_launch(bank, B, N, over, traj_of, idx, yref, yref_e, pos_ref, (hipStream_t)stream);
}

// The refusals of a rollout up to those of its arrays.
int admpc_quad_rollout_check(const QuadRolloutArgs& a, int T)
{
    int device = 0, sqp = 0;
    if (!a.s) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: null solver");
    (void)admpc_quad_solver_info(a.s, &device, nullptr, &sqp);
    if (sqp > 1) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: a solver in SQP mode (sqp_iters > 1) is not served: the rollout is the RTI loop");
    if (!a.bank) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: null bank");
    if (a.bank->device != device) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: the bank is on another device than the solver");
    const int rc = plant_params_check("admpc_quad_rollout_batch", a.plant);
    if (rc) return rc;
    if (a.over < 1) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: over must be at least 1");
    if (a.B < 0) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: negative batch");
    if (T < 0 || T > 4096) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: T must be in [0, 4096]");
    return ADMPC_OK;
}

// One closed-loop period for checked arguments, B > 0, on the solver's device (the caller holds it): window -> RTI step -> plant.
// traj_pre / traj_post: null or [B][13], the states before and after the period; u_out: null or [B][4], the input applied in it.
int admpc_quad_rollout_enqueue(const QuadRolloutArgs& r, double* traj_pre, double* traj_post, double* u_out, void* stream)
{
    int N = 0;
    (void)admpc_quad_solver_info(r.s, nullptr, &N, nullptr);
    int rc = chunk_launch(r.bank, r.B, N, r.over, r.traj_of, r.idx, r.yref, r.yref_e, nullptr, (hipStream_t)stream);
    if (!rc) rc = admpc_quad_solve_batch_ex(r.s, r.B, r.x, r.yref, r.yref_e, nullptr, r.xbar, r.ubar, r.cost, r.status, r.iters, stream);
    if (rc) return rc;
    QuadPlantArgs a = plant_only(r.plant, r.B, r.ubar, (long long)N * QU, r.x);
    a.K = r.bank->K; a.desc = r.bank->d_desc;
    a.yref = r.yref; a.yref_stride = (long long)N * QY; a.status = r.status; a.tally = r.tally; a.counts = r.counts;
    a.traj_of = r.traj_of; a.idx = r.idx;
    a.traj_pre = traj_pre; a.traj_post = traj_post; a.u_out = u_out;
    return plant_launch(a, (hipStream_t)stream);
}

int admpc_quad_rollout_batch(AdmpcQuadSolver* s, const AdmpcQuadTrajBank* bank, const AdmpcQuadPlantParams* plant, int over, int B, int T,
                             const int32_t* traj_of, int32_t* idx, double* x, double* xbar, double* ubar,
                             double* yref, double* yref_e, double* cost, int32_t* status, int32_t* iters,
                             double* tally, int32_t* counts, double* traj_out, double* u_out, void* stream)
{
    const QuadRolloutArgs a = { s, bank, plant, over, B, traj_of, idx, x, xbar, ubar, yref, yref_e, cost, status, iters, tally, counts };
    int rc = admpc_quad_rollout_check(a, T);
    if (rc || B == 0 || T == 0) return rc;
    if (!traj_of || !idx || !x || !xbar || !ubar || !yref || !yref_e || !status)
        return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: null array argument");
    if (!tally || !counts) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: null tally or counts");
    int device = 0;
    (void)admpc_quad_solver_info(s, &device, nullptr, nullptr);
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    // slot 0 of traj_out is written by the first period; every period writes the state it leaves into the next slot
    for (int t = 0; t < T && !rc; ++t)
        rc = admpc_quad_rollout_enqueue(a, t == 0 ? traj_out : nullptr, traj_out ? traj_out + (size_t)(t + 1) * B * QX : nullptr,
                                        u_out ? u_out + (size_t)t * B * QU : nullptr, stream);
    return rc;
}

}  // extern "C"
