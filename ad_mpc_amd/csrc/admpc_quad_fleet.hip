// admpc_quad_fleet.hip -- the quadrotor's closed loop on the device (include/admpc_quad_fleet.h): the bank of trajectories, one kernel
// and the rollout.
//
//   admpc_quad_chunk_kernel   the reference window of every vehicle (get_reference_chunk + set_reference_trajectory's padding): a
//                             gather, one thread per double written, so the 17 doubles of a node row leave contiguous lanes
//
// The rollout (admpc_quad_rollout_batch) is T times chunk -> admpc_quad_solve_batch_ex -> plant on one stream; with a clustered ensemble in
// its argument block (admpc_quad_ensemble.hip) the solve is route -> admpc_quad_solve_batch_routed.  The plant kernels and their launch
// are admpc_quad_plant.hip's: a rollout whose argument block carries disturbances gets the noisy kernel in every period.
#include <math.h>
#include <new>
#include "admpc_host.h"
#include "../../include/admpc_quad_fleet.h"
#include "quad_sim_dev.h"     // QuadTrajDesc, QuadPlantArgs

#define QX ADMPC_QUAD_NX
#define QU ADMPC_QUAD_NU
#define QY ADMPC_QUAD_NY
#define QC_THREADS 256
#define QC_GRID 4096           // blocks of the chunk kernel at most

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

}  // namespace

extern "C" {

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
    int32_t* hM = new (std::nothrow) int32_t[K];
    if (!b || !desc || !hM) { delete b; delete[] desc; delete[] hM; return admpc_set_error(ADMPC_ENOMEM, "out of host memory"); }
    for (int k = 0; k < K; ++k) hM[k] = M[k];
    b->h_M = hM;
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
        delete[] b->h_M;
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
    delete[] bank->h_M;
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
    const int rc = admpc_quad_plant_params_check("admpc_quad_rollout_batch", a.plant);
    if (rc) return rc;
    if (a.over < 1) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: over must be at least 1");
    if (a.B < 0) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: negative batch");
    if (T < 0 || T > 4096) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: T must be in [0, 4096]");
    return ADMPC_OK;
}

// One closed-loop period for checked arguments, B > 0, on the solver's device (the caller holds it): window -> RTI step -> plant.
// traj_pre / traj_post: null or [B][13], the states before and after the period; u_out: null or [B][4], the input applied in it.
// With r.ens the RTI step is the ensemble's: the cluster of every vehicle from row 0 of its window (route_out: null or [B], the record of
// it), then admpc_quad_solve_batch_routed over the ensemble's handles on the ONE iterate xbar / ubar.
int admpc_quad_rollout_enqueue(const QuadRolloutArgs& r, double* traj_pre, double* traj_post, double* u_out, int32_t* route_out, void* stream)
{
    int N = 0;
    (void)admpc_quad_solver_info(r.s, nullptr, &N, nullptr);
    int rc = chunk_launch(r.bank, r.B, N, r.over, r.traj_of, r.idx, r.yref, r.yref_e, nullptr, (hipStream_t)stream);
    if (!rc && r.ens) {
        AdmpcQuadSolver* const* handles = nullptr;
        const int K = admpc_quad_ensemble_handles(r.ens, &handles);
        rc = admpc_quad_ensemble_route_launch(r.ens, r.B, r.yref, r.route, route_out, stream);
        if (!rc) rc = admpc_quad_solve_batch_routed(handles, K, r.B, r.route, r.x, r.yref, r.yref_e, nullptr, r.xbar, r.ubar, r.cost, r.status, r.iters, stream);
    }
    else if (!rc) rc = admpc_quad_solve_batch_ex(r.s, r.B, r.x, r.yref, r.yref_e, nullptr, r.xbar, r.ubar, r.cost, r.status, r.iters, stream);
    if (rc) return rc;
    QuadPlantArgs a;
    admpc_quad_plant_fill(a, r.plant, r.B, r.ubar, (long long)N * QU, r.x);
    a.K = r.bank->K; a.desc = r.bank->d_desc;
    a.yref = r.yref; a.yref_stride = (long long)N * QY; a.status = r.status; a.tally = r.tally; a.counts = r.counts;
    a.traj_of = r.traj_of; a.idx = r.idx;
    a.traj_pre = traj_pre; a.traj_post = traj_post; a.u_out = u_out;
    return admpc_quad_plant_launch(a, r.noise, r.noise_step, nullptr, stream);
}

// admpc_quad_rollout_batch behind its arguments' block: the refusals, the no-ops and the T periods; with a.noise the plant of every
// period is the noisy one, whose counter array is refused last
int admpc_quad_rollout_run(const QuadRolloutArgs& a, int T, double* traj_out, double* u_out, void* stream)
{
    int rc = admpc_quad_rollout_check(a, T);
    if (rc || a.B == 0 || T == 0) return rc;
    if (!a.traj_of || !a.idx || !a.x || !a.xbar || !a.ubar || !a.yref || !a.yref_e || !a.status || (a.ens && !a.route))
        return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: null array argument");
    if (!a.tally || !a.counts) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_batch: null tally or counts");
    if (a.noise && !a.noise_step) return admpc_set_error(ADMPC_EINVAL, "admpc_quad_rollout_noise_batch: null noise_step");
    int device = 0;
    (void)admpc_quad_solver_info(a.s, &device, nullptr, nullptr);
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    for (int t = 0; t < T && !rc; ++t) {
        const QuadRecordSlots rec = admpc_quad_record_slots(traj_out, u_out, a.B, t);
        rc = admpc_quad_rollout_enqueue(a, rec.traj_pre, rec.traj_post, rec.u_out, a.route_out ? a.route_out + (size_t)t * a.B : nullptr, stream);
    }
    return rc;
}

int admpc_quad_rollout_batch(AdmpcQuadSolver* s, const AdmpcQuadTrajBank* bank, const AdmpcQuadPlantParams* plant, int over, int B, int T,
                             const int32_t* traj_of, int32_t* idx, double* x, double* xbar, double* ubar,
                             double* yref, double* yref_e, double* cost, int32_t* status, int32_t* iters,
                             double* tally, int32_t* counts, double* traj_out, double* u_out, void* stream)
{
    const QuadRolloutArgs a = { s, bank, plant, over, B, traj_of, idx, x, xbar, ubar, yref, yref_e, cost, status, iters, tally, counts, nullptr, nullptr };
    return admpc_quad_rollout_run(a, T, traj_out, u_out, stream);
}

}  // extern "C"
