// admpc_kernels.hip -- gfx950 (MI355X / CDNA4) kernels of the batched AD-MPC solve engine, main translation unit.
//
// One SQP step:
//   A  admpc_linearize_kernel  one thread per (instance, stage, sensitivity-column group): ERK4 + forward
//                              sensitivities, writes the packed stage linearisation (42+7 values per stage)
//   then the QP of the step (H2-H6), one of
//   R  admpc_rowqp_kernel      (admpc_rowqp.hip) stage-wise Riccati interior point, one instance per 16-lane DPP row:
//                              every horizon, fp64 and fp32
//   F  admpc_fused20_kernel    (admpc_fused20.hip) N = 20 fp64, condensed (the reference's own QP strategy): shooting,
//                              condensing, dense LDL' interior point and expansion in one persistent kernel, no kernel A
//   S  admpc_seg_kernel        (admpc_seg.hip) N = 40 / 60 / 80 fp64, segmented condensed interior point, no kernel A
//
// Hot path restated (reference = data_driven_mpc/ros_gp_mpc/src/ad_mpc/...):
//   H0/H1  model + ERK4 with forward sensitivities   ad_3d_optimizer.py:280-310, acados ERK
//                                                     (acados_solver_sim_car.c:655-665)
//   H2/H3  Gauss-Newton LS cost, soft/hard bounds     ad_3d_optimizer.py:146-199
//   H4/H5  QP solve: Mehrotra predictor-corrector primal-dual IPM (reference: full condensing + HPIPM,
//          acados_solver_sim_car.c:145,688-692; same unique minimiser)
//   H6     full step update of the iterate            acados_solver_sim_car.c:647-648,677
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>
#include <math.h>
#include "admpc_host.h"
#include "argmin_rule.h"

#define NX ADMPC_NX
#define NU ADMPC_NU
#define NY ADMPC_NY
#define WAVE 64
#define IPM_FLOOR 1e-40

namespace {

#include "model_dev.h"

// ---------------------------------------------------------------------------------------------
// kernel A: shooting + linearisation, one thread per (instance, stage, column group), T = double or float
// (storage and arithmetic).  Output, instance-major and packed as the QP kernels read it:
//   GTg [B][N][7][6]  stored columns c=0..6 <-> (A[:,2..6], B[:,0..1]), rows 0..5 of each column.
//                     Not stored because they are structural for this model (delta' = u1, positions
//                     do not feed back): A[:,0]=e0, A[:,1]=e1, row 6 of [A B] = [e6, 0, h].
//   blg [B][N][7]     defect b_k = phi(xbar_k,ubar_k) - xbar_{k+1}
// ---------------------------------------------------------------------------------------------
#define GTS 42           // values per stage of the packed linearisation
#define LIN_BLOCK 64     // threads per block of the linearisation kernel: single waves balance best over the CUs (256 registers each)
#define LIN_TASKS 63     // tasks per block (multiple of 3)
// ticket header of kernel R (int array): [0] ticket counter, zeroed by the linearisation kernel
#define SCHED_HDR 128

template <class T>
__global__ __launch_bounds__(LIN_BLOCK) void admpc_linearize_kernel(const AdmpcConfig* __restrict__ cfg, int B,
                                                              const T* __restrict__ xbarg, const T* __restrict__ ubarg,
                                                              const T* __restrict__ pg, const int32_t* __restrict__ skip,
                                                              T* __restrict__ GTg, T* __restrict__ blg, int* __restrict__ sched)
{
    const int N = cfg->N;
    const long total = (long)B * N * 3;
    if (sched && blockIdx.x == 0) for (int i = threadIdx.x; i < SCHED_HDR; i += blockDim.x) sched[i] = 0;     // ticket counter of this step
    // 63 tasks per 64-lane block: the three threads of a stage sit in adjacent lanes of one wave (gp_eval shares work among them)
    if (threadIdx.x >= LIN_TASKS) return;
    for (long tsk = (long)blockIdx.x * LIN_TASKS + threadIdx.x; tsk < total; tsk += (long)gridDim.x * LIN_TASKS) {
        const long sk = tsk / 3; const int g = (int)(tsk % 3);
        const long inst = sk / N; const int k = (int)(sk % N);
        if (skip && skip[inst] != 0) continue;
        T x[NX], u[NU], phi[NX], col[3][NX];
        const T* xs = xbarg + (inst * (N + 1) + k) * NX;
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = xs[i];
        u[0] = ubarg[(inst * N + k) * NU]; u[1] = ubarg[(inst * N + k) * NU + 1];
        rk4_group<T>(cfg, x, u, pg[inst], (T)cfg->Ts, g, phi, col);
        T* GT = GTg + sk * GTS;
        const int c0 = g == 0 ? 0 : (g == 1 ? 3 : 5);
        const int nc = g == 0 ? 3 : 2;
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
            if (cc < nc)
#pragma unroll
                for (int i = 0; i < 6; ++i) GT[(c0 + cc) * 6 + i] = col[cc][i];
        if (g == 0) {
#pragma unroll
            for (int i = 0; i < NX; ++i) blg[sk * NX + i] = phi[i] - xs[NX + i];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// wave-level primitives
// ---------------------------------------------------------------------------------------------
#include "dense40.h"      // wave_reduce

// ---------------------------------------------------------------------------------------------
// local reference generator: bound_pi, interp_np, waypoints_one and PathDesc, one wavefront per vehicle pose
// ---------------------------------------------------------------------------------------------
#include "waypoints_dev.h"

__global__ __launch_bounds__(WAVE) void admpc_waypoints_kernel(int M, int H, double dt, int B,
        const double* __restrict__ vel, const double* __restrict__ tx, const double* __restrict__ ty,
        const double* __restrict__ tpsi, const double* __restrict__ tpsi_unw, const double* __restrict__ cdist, const double* __restrict__ curv,
        const double* __restrict__ Xi, const double* __restrict__ Yi, const double* __restrict__ Pi,
        double* __restrict__ out_ref, double* __restrict__ out_err, int32_t* __restrict__ out_stop)
{
    __shared__ double sh[WAVE];
    for (int b = blockIdx.x; b < B; b += gridDim.x)
        waypoints_one(M, H, dt, b, vel, tx, ty, tpsi, tpsi_unw, cdist, curv, Xi, Yi, Pi, out_ref, out_err, out_stop, sh);
}

// The generator with a path per vehicle: vehicle b reads the columns that descriptor path_of[b] names.  An index outside [0, K) reads no
// path: NaN rows, stop 0 (the solve then fails that vehicle alone).  path_of[b] is uniform over the block, so are the barriers.
__global__ __launch_bounds__(WAVE) void admpc_waypoints_bank_kernel(int K, int H, double dt, int B,
        const PathDesc* __restrict__ desc, const double* __restrict__ cols, const int32_t* __restrict__ path_of,
        const double* __restrict__ Xi, const double* __restrict__ Yi, const double* __restrict__ Pi,
        double* __restrict__ out_ref, double* __restrict__ out_err, int32_t* __restrict__ out_stop)
{
    __shared__ double sh[WAVE];
    const int lane = threadIdx.x;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const int k = path_of[b];
        if (k < 0 || k >= K) {
            double* o = out_ref + (size_t)b * 6 * H;
            if (lane < H)
                for (int r = 0; r < 6; ++r) o[r * H + lane] = NAN;
            if (lane < 3) out_err[b * 3 + lane] = NAN;
            if (lane == 0) out_stop[b] = 0;
            continue;
        }
        const PathDesc d = desc[k];
        waypoints_one((int)d.M, H, dt, b, cols + d.off[0], cols + d.off[1], cols + d.off[2], cols + d.off[3], cols + d.off[4], cols + d.off[5],
                      cols + d.off[6], Xi, Yi, Pi, out_ref, out_err, out_stop, sh);
    }
}

// shooting only: phi, A, B to global memory (parity tests of H0/H1), T = double or float
template <class T>
__global__ __launch_bounds__(WAVE) void admpc_shoot_kernel(const AdmpcConfig* __restrict__ cfg, int B,
                                                           const T* __restrict__ xbarg, const T* __restrict__ ubarg,
                                                           const T* __restrict__ pg,
                                                           T* __restrict__ phig, T* __restrict__ Ag, T* __restrict__ Bg)
{
    const int N = cfg->N;
    const long total = (long)B * N * 3;
    if (threadIdx.x >= LIN_TASKS) return;                // same task -> lane map as the linearisation kernel (gp_eval relies on it)
    for (long tsk = (long)blockIdx.x * LIN_TASKS + threadIdx.x; tsk < total; tsk += (long)gridDim.x * LIN_TASKS) {
        const long sk = tsk / 3; const int g = (int)(tsk % 3);
        const long inst = sk / N; const int k = (int)(sk % N);
        T x[NX], u[NU], phi[NX], col[3][NX];
        for (int i = 0; i < NX; ++i) x[i] = xbarg[(inst * (N + 1) + k) * NX + i];
        u[0] = ubarg[(inst * N + k) * NU]; u[1] = ubarg[(inst * N + k) * NU + 1];
        rk4_group<T>(cfg, x, u, pg[inst], (T)cfg->Ts, g, phi, col);
        T* A = Ag + sk * NX * NX; T* Bm = Bg + sk * NX * NU;
        if (g == 0) {
            for (int i = 0; i < NX; ++i) {
                phig[sk * NX + i] = phi[i];
                A[i * 7 + 0] = i == 0 ? (T)1 : (T)0; A[i * 7 + 1] = i == 1 ? (T)1 : (T)0;
                A[i * 7 + 2] = col[0][i]; A[i * 7 + 3] = col[1][i]; A[i * 7 + 4] = col[2][i];
            }
        } else if (g == 1) {
            for (int i = 0; i < NX; ++i) { A[i * 7 + 5] = col[0][i]; A[i * 7 + 6] = col[1][i]; }
        } else {
            for (int i = 0; i < NX; ++i) { Bm[i * 2] = col[0][i]; Bm[i * 2 + 1] = col[1][i]; }
        }
    }
}

// receding-horizon shift of the iterate: stage k takes the values of stage k+1, the last input is kept and the new
// terminal state is either a copy (rollout = 0) or one model step from the old terminal state under the last input.
// Three lanes per instance as in the linearisation kernel (gp_eval shares its sums among them); lane 0 moves x, lane 1 moves u.
__global__ __launch_bounds__(WAVE) void admpc_shift_kernel(const AdmpcConfig* __restrict__ cfg, int B, double* __restrict__ xbarg,
                                                           double* __restrict__ ubarg, const double* __restrict__ pg, int rollout)
{
    const int N = cfg->N;
    const long total = (long)B * 3;
    if (threadIdx.x >= LIN_TASKS) return;
    for (long tsk = (long)blockIdx.x * LIN_TASKS + threadIdx.x; tsk < total; tsk += (long)gridDim.x * LIN_TASKS) {
        const long inst = tsk / 3; const int g = (int)(tsk % 3);
        double* xb = xbarg + inst * (N + 1) * NX;
        double* ub = ubarg + inst * N * NU;
        double x[NX], u[NU], phi[NX], col[3][NX];
        for (int i = 0; i < NX; ++i) { x[i] = xb[N * NX + i]; phi[i] = x[i]; }
        u[0] = ub[(N - 1) * NU]; u[1] = ub[(N - 1) * NU + 1];
        if (rollout) rk4_group<double>(cfg, x, u, pg[inst], cfg->Ts, g, phi, col);
        if (g == 0) {
            for (int i = 0; i < N * NX; ++i) xb[i] = xb[i + NX];
            for (int i = 0; i < NX; ++i) xb[N * NX + i] = phi[i];
        } else if (g == 1) {
            for (int i = 0; i < (N - 1) * NU; ++i) ub[i] = ub[i + NU];
        }
    }
}

// arg-min over cost[0..B): one block; the ordering rules (ties -> lowest index; NaN read as +inf) live in argmin_rule.h
__global__ __launch_bounds__(256) void admpc_argmin_kernel(const double* __restrict__ cost, int B, int64_t offset,
                                                           double* __restrict__ val, int64_t* __restrict__ idx)
{
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    ArgminBest b = argmin_identity();
    for (int i = threadIdx.x; i < B; i += blockDim.x) argmin_fold(b, argmin_cost(cost[i]), (int64_t)i);
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(b.v, o, WAVE);
        const int64_t oi = __shfl_xor((long long)b.i, o, WAVE);
        argmin_fold(b, ov, oi);
    }
    const int w = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) { sv[w] = b.v; si[w] = b.i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) argmin_fold(b, sv[i], si[i]);
        *val = b.v;
        *idx = argmin_final_index(b) + offset;
    }
}

// second level of the arg-min: W gathered (cost, global index) pairs, 16 bytes each, as the per-GPU admpc_argmin wrote them
// and an all-gather laid them out; one wave; same rules (argmin_rule.h)
__global__ __launch_bounds__(WAVE) void admpc_argmin_pairs_kernel(const double* __restrict__ pairs, int W,
                                                                  double* __restrict__ val, int64_t* __restrict__ idx)
{
    ArgminBest b = argmin_identity();
    for (int i = threadIdx.x; i < W; i += WAVE)
        argmin_fold(b, argmin_cost(pairs[2 * i]), (int64_t)__double_as_longlong(pairs[2 * i + 1]));
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(b.v, o, WAVE);
        const int64_t oi = __shfl_xor((long long)b.i, o, WAVE);
        argmin_fold(b, ov, oi);
    }
    if (threadIdx.x == 0) { *val = b.v; *idx = argmin_final_index(b); }
}

// arg-min per group of `group` consecutive costs (admpc_argmin_groups): one wave per group, lane l folds costs l, l + 64, ...; groups of
// up to 16 costs sit four to a wave, one per 16-lane row, and the butterfly then stays inside the row.  Indices are those of the batch.
// Same rules as above (argmin_rule.h); a group is never empty, so argmin_final_index returns the index it is given.
#define ARGMIN_GROUPS_WAVES 4          // waves per block
#define ARGMIN_GROUPS_GRID 256         // blocks at the most: a stride loop past it
__global__ __launch_bounds__(ARGMIN_GROUPS_WAVES * WAVE) void admpc_argmin_groups_kernel(const double* __restrict__ cost, int G, int group,
                                                                                       double* __restrict__ val, int64_t* __restrict__ idx)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = blockIdx.x * ARGMIN_GROUPS_WAVES + threadIdx.x / WAVE, nwaves = gridDim.x * ARGMIN_GROUPS_WAVES;
    const bool packed = group <= 16;
    const int per_wave = packed ? 4 : 1;
    const int width = packed ? 16 : WAVE;                 // lanes that share a group
    const int l = lane & (width - 1);
    for (long g0 = (long)wave * per_wave; g0 < G; g0 += (long)nwaves * per_wave) {
        const long g = g0 + (packed ? lane >> 4 : 0);
        const int64_t base = (int64_t)g * group;
        ArgminBest b = argmin_identity();
        if (g < G)
            for (int i = l; i < group; i += width) argmin_fold(b, argmin_cost(cost[base + i]), base + i);
        for (int o = width >> 1; o > 0; o >>= 1) {
            const double ov = __shfl_xor(b.v, o, WAVE);
            const int64_t oi = __shfl_xor((long long)b.i, o, WAVE);
            argmin_fold(b, ov, oi);
        }
        if (l == 0 && g < G) { val[g] = b.v; idx[g] = argmin_final_index(b); }
    }
}

// post-solve epilogue: validity test ad_3d_optimizer.py:385-394 + Ackermann mapping
// create_ros_ad_mpc.py:95-98; one thread per instance
__global__ void admpc_epilogue_kernel(int N, int B, const double* __restrict__ xopt, const double* __restrict__ uopt,
                                      const double* __restrict__ xref_xy, float* __restrict__ ack, int32_t* __restrict__ valid)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* x = xopt + (size_t)b * (N + 1) * NX;
    const double* r = xref_xy + (size_t)b * (N + 1) * 2;
    const int n = N + 1;
    double s = 0.0, mx = 0.0;
    for (int i = 0; i < n - 1; ++i) {
        const double dxv = r[i * 2] - x[i * 7], dyv = r[i * 2 + 1] - x[i * 7 + 1];
        const double d = sqrt(dxv * dxv + dyv * dyv);
        s += d; mx = fmax(mx, d);
    }
    const double mean = s / n;
    double var = 0.0;
    for (int i = 0; i < n; ++i) {
        double d = 0.0;
        if (i < n - 1) { const double dxv = r[i * 2] - x[i * 7], dyv = r[i * 2 + 1] - x[i * 7 + 1]; d = sqrt(dxv * dxv + dyv * dyv); }
        var += (d - mean) * (d - mean);
    }
    var /= (n - 1);
    valid[b] = (mean < 3.0 && var < 2.0 && mx < 4.0) ? 1 : 0;
    const double* u = uopt + (size_t)b * N * NU;
    ack[b * 4 + 0] = (float)x[6]; ack[b * 4 + 1] = (float)u[1]; ack[b * 4 + 2] = (float)x[3]; ack[b * 4 + 3] = (float)u[0];
}

// SQP solve with a tolerance (cfg.sqp_iters > 1, cfg.sqp_tol > 0: reference solver_type "SQP", create_ros_ad_mpc.py:47-51; the tolerances
// are acados' defaults nlp_solver_tol_{stat,eq,ineq,comp} = 1e-6, acados_models/sim_car_acados_ocp.json:870-873): acados' stopping test
// (ocp_nlp_sqp.c: linearise -> residuals of the NLP's KKT system with the iterate's multipliers -> all four inf-norms within tolerance:
// ACADOS_SUCCESS, else solve the QP and step; ACADOS_MAXITER after nlp_solver_max_iter QPs).  Runs between the linearisation and kernel R
// in every pass of a solve but the first (the C ABI takes no multipliers in: a cold solver), on the NEW linearisation GT / bl with the
// multipliers kernel R left for the previous QP (pi: adjoint recursion, as HPIPM's expansion of the condensed solution; ineq: slacks t and
// multipliers lam in the record order of admpc.h):
//   res_stat  rows of grad L:  u: R (u - uref) + B' pi_k - lam_lo + lam_up;  slacks: rho - lam - lam_s;
//                              x_k: Q (x_k - xref_k) + A_k' pi_k - pi_{k-1} (- lam_d,lo + lam_d,up on delta);  x_N: Q_e (x_N - xref_e) - pi_{N-1};
//                              x_0: against pi_N, the multiplier of the initial-state equality
//   res_eq    shooting defects b_k, x0 - x_0
//   res_ineq  constraint value minus its slack t (slack variables read from the slacks of their own bounds)
//   res_comp  lam .* t
// One wave per instance, lane <-> stage.  A converged instance gets status -1 and is skipped by the rest of the solve.
// fp32 (kernel R's float instantiation stops its QPs at residual 1e-2 / complementarity 1e-3, rowqp_core.h): the tolerances are floored
// at those levels (and the defects at 1e-4: the float shooting), since no NLP residual can be driven below the QP's own.
template <class T>
__global__ __launch_bounds__(WAVE) void admpc_nlp_res_kernel(const AdmpcConfig* __restrict__ cfg, int B, const T* __restrict__ x0g,
                                                             const T* __restrict__ yrefg, const T* __restrict__ yrefeg,
                                                             const T* __restrict__ xbarg, const T* __restrict__ ubarg,
                                                             const T* __restrict__ GTg, const T* __restrict__ blg,
                                                             const T* __restrict__ pig, const T* __restrict__ ineqg,
                                                             int32_t* __restrict__ statusg, T* __restrict__ resg)
{
    constexpr bool f32 = sizeof(T) == 4;
    const int N = cfg->N, lane = threadIdx.x;
    const T h = (T)cfg->Ts;
    const T rho_l = (T)(cfg->Ts * cfg->zl), rho_u = (T)(cfg->Ts * cfg->zu);
    const double tol = cfg->sqp_tol;
    const double tol_stat = f32 && tol < 1e-2 ? 1e-2 : tol, tol_eq = f32 && tol < 1e-4 ? 1e-4 : tol;
    const double tol_ineq = tol_stat, tol_comp = f32 && tol < 1e-3 ? 1e-3 : tol;
    for (int inst = blockIdx.x; inst < B; inst += gridDim.x) {
        if (statusg[inst] != 0) continue;                                   // failed or converged in an earlier pass
        const T* xb = xbarg + (size_t)inst * (N + 1) * NX;
        const T* ub = ubarg + (size_t)inst * N * NU;
        const T* yr = yrefg + (size_t)inst * N * NY;
        const T* pi = pig + (size_t)inst * (N + 1) * NX;
        T rs = 0, re = 0, ri = 0, rc = 0;
        auto upd = [](T& acc, T v) __attribute__((always_inline)) { const T a = v < 0 ? -v : v; if (a > acc || a != a) acc = a; };
        for (int k = lane; k <= N; k += WAVE) {
            T x[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] = xb[k * NX + i];
            if (k == N) {
#pragma unroll
                for (int i = 0; i < NX; ++i) upd(rs, (T)cfg->We[i] * (x[i] - yrefeg[(size_t)inst * NX + i]) - pi[(N - 1) * NX + i]);
                continue;
            }
            const T* G = GTg + ((size_t)inst * N + k) * GTS;
            const T* pk = pi + k * NX;
            const T* pp = pi + (k >= 1 ? k - 1 : N) * NX;
            const T* iq = ineqg + ((size_t)inst * N + k) * 20;
            T pv[NX], t[10], lm[10];
#pragma unroll
            for (int i = 0; i < NX; ++i) pv[i] = pk[i];
#pragma unroll
            for (int i = 0; i < 10; ++i) { t[i] = iq[i]; lm[i] = iq[10 + i]; }
            // stationarity in x_k: columns 0, 1 of A_k are unit vectors, row 6 of [A B] is [e6, 0, h] (not stored)
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                T a = (T)(cfg->Ts * cfg->W[i]) * (x[i] - yr[k * NY + i]) - pp[i];
                if (i < 2) a += pv[i];
                else {
#pragma unroll
                    for (int r = 0; r < 6; ++r) a += G[(i - 2) * 6 + r] * pv[r];
                    if (i == 6) { a += pv[6]; if (k >= 1) a += lm[5] - lm[4]; }
                }
                upd(rs, a);
            }
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const T u = ub[k * NU + j];
                T a = (T)(cfg->Ts * cfg->W[NX + j]) * (u - yr[k * NY + NX + j]) - lm[2 * j] + lm[2 * j + 1];
#pragma unroll
                for (int r = 0; r < 6; ++r) a += G[(5 + j) * 6 + r] * pv[r];
                if (j == 1) a += h * pv[6];
                upd(rs, a);
                upd(rs, rho_l - lm[2 * j] - lm[6 + 2 * j]); upd(rs, rho_u - lm[2 * j + 1] - lm[7 + 2 * j]);
                upd(ri, u + t[6 + 2 * j] - (T)cfg->lbu[j] - t[2 * j]); upd(ri, (T)cfg->ubu[j] - u + t[7 + 2 * j] - t[2 * j + 1]);
                upd(rc, lm[2 * j] * t[2 * j]); upd(rc, lm[2 * j + 1] * t[2 * j + 1]);
                upd(rc, lm[6 + 2 * j] * t[6 + 2 * j]); upd(rc, lm[7 + 2 * j] * t[7 + 2 * j]);
            }
#pragma unroll
            for (int i = 0; i < NX; ++i) upd(re, blg[((size_t)inst * N + k) * NX + i]);
            if (k >= 1) {
                upd(ri, x[6] - (T)cfg->lbx_delta - t[4]); upd(ri, (T)cfg->ubx_delta - x[6] - t[5]);
                upd(rc, lm[4] * t[4]); upd(rc, lm[5] * t[5]);
            } else {
#pragma unroll
                for (int i = 0; i < NX; ++i) upd(re, x0g[(size_t)inst * NX + i] - x[i]);
            }
        }
        const double ws = wave_reduce<OpMaxNan>((double)rs), we = wave_reduce<OpMaxNan>((double)re);
        const double wi = wave_reduce<OpMaxNan>((double)ri), wc = wave_reduce<OpMaxNan>((double)rc);
        if (lane == 0) {
            if (ws <= tol_stat && we <= tol_eq && wi <= tol_ineq && wc <= tol_comp) statusg[inst] = -1;
            if (resg) { resg[(size_t)inst * 4 + 0] = (T)ws; resg[(size_t)inst * 4 + 1] = (T)we; resg[(size_t)inst * 4 + 2] = (T)wi; resg[(size_t)inst * 4 + 3] = (T)wc; }
        }
    }
}

// end of an SQP solve with a tolerance: -1 (converged in some step) -> 0, still 0 after the last step -> ADMPC_STATUS_MAXITER
__global__ void admpc_sqp_finalize_kernel(int B, int32_t* __restrict__ status)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int st = status[b];
    status[b] = st == -1 ? ADMPC_STATUS_SUCCESS : (st == 0 ? ADMPC_STATUS_MAXITER : st);
}

// Speed-reference clamp in front of the solve: gp_ad_mpc_node.py:344-349 resample_vel -- the reference speed of
// slot i may not exceed |v| + i * (acc_max * dt * 0.8), the bound growing by repeated addition as in the reference (same rounding).
// One thread per vehicle; vel_ref [B] rows of H values, `ld` values apart (e.g. row 3 of admpc_waypoints_batch's out_ref: ld = 6 H).
__global__ void admpc_resample_vel_kernel(int B, int H, int ld, const double* __restrict__ vx, const double* __restrict__ vy,
                                          double acc_max, double dt, double* __restrict__ vel_ref)
{
#pragma clang fp contract(off)      // every product and sum rounded on its own, as the host's Python arithmetic does (hipcc contracts by default)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    // plain operators under the pragma above (the __dmul_rn / __dadd_rn wrappers of the HIP headers are inlined WITH the translation
    // unit's contraction flag and would be fused into an FMA)
    const double sx = vx[b] * vx[b], sy = vy[b] * vy[b];
    double bound = __dsqrt_rn(sx + sy);
    const double inc = (acc_max * dt) * 0.8;
    double* v = vel_ref + (size_t)b * ld;
    for (int i = 0; i < H; ++i) {
        if (v[i] > bound) v[i] = bound;
        bound = bound + inc;
    }
}

// Post-solve safety and actuation, one thread per vehicle slot / candidate:
//   check_pred_trj                          gp_ad_mpc_node.py:248-257 (same formula as is_valid_command, ad_3d_optimizer.py:385-394)
//   consecutive-success gate                :206-213  (status > 0 resets the counter; fewer than `threshold` successes: no MPC command)
//   steering command                        :222-223  clip(clip(rate) * 0.1 + measured steering)
//   fallback (auxiliary controller)         :455-476  steering held at the measured value, acceleration -1e5 (hard brake)
//   Ackermann record                        create_ros_ad_mpc.py:95-98 (float32 message fields)
// cost_io (may be null): +inf for every candidate that does not produce an MPC command, so that an arg-min over it picks
// a valid candidate only.
__global__ void admpc_actuation_kernel(int N, int B, const double* __restrict__ xopt, const double* __restrict__ uopt,
                                       const double* __restrict__ xref_xy, const int32_t* __restrict__ status,
                                       const double* __restrict__ steer_meas, int32_t* __restrict__ safe_count, int threshold,
                                       double rate_min, double rate_max, double steer_min, double steer_max,
                                       double* __restrict__ cost_io, float* __restrict__ ack, int32_t* __restrict__ mode, int32_t* __restrict__ valid)
{
#pragma clang fp contract(off)      // the steering command is two separately rounded operations in the reference (:223)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* x = xopt + (size_t)b * (N + 1) * NX;
    const double* r = xref_xy + (size_t)b * (N + 1) * 2;
    const int n = N + 1;
    double sm = 0.0, mx = 0.0;
    for (int i = 0; i < n - 1; ++i) {
        const double dxv = r[i * 2] - x[i * 7], dyv = r[i * 2 + 1] - x[i * 7 + 1];
        const double d = sqrt(dxv * dxv + dyv * dyv);
        sm += d; mx = fmax(mx, d);
    }
    const double mean = sm / n;
    double var = 0.0;
    for (int i = 0; i < n; ++i) {
        double d = 0.0;
        if (i < n - 1) { const double dxv = r[i * 2] - x[i * 7], dyv = r[i * 2 + 1] - x[i * 7 + 1]; d = sqrt(dxv * dxv + dyv * dyv); }
        var += (d - mean) * (d - mean);
    }
    var /= (n - 1);
    const int healthy = (mean < 3.0 && var < 2.0 && mx < 4.0) ? 1 : 0;
    const int cnt = status[b] > 0 ? 0 : safe_count[b] + 1;
    safe_count[b] = cnt;
    const int ok = (cnt >= threshold && healthy) ? 1 : 0;
    const double* u = uopt + (size_t)b * N * NU;
    const double sth = steer_meas[b];
    if (ok) {
        const double rate_msg = (double)(float)u[1];                 // the value travels through a float32 message field
        const double sv = fmax(fmin(rate_max, rate_msg), rate_min);
        const double scaled = sv * 0.1;
        const double ang = fmax(fmin(steer_max, scaled + sth), steer_min);
        ack[b * 4 + 0] = (float)ang; ack[b * 4 + 1] = (float)u[1]; ack[b * 4 + 2] = (float)x[3]; ack[b * 4 + 3] = (float)u[0];
    } else {
        ack[b * 4 + 0] = (float)sth; ack[b * 4 + 1] = 0.0f; ack[b * 4 + 2] = 0.0f; ack[b * 4 + 3] = (float)(-1e5);
    }
    mode[b] = ok;
    valid[b] = healthy;
    if (cost_io && !ok) cost_io[b] = INFINITY;
}

}  // namespace

// =============================================================================================
// C ABI (include/admpc.h)
// =============================================================================================
#include <string>
#include <dlfcn.h>
#include <mutex>
#include <cstdio>
#include <cstring>
#include <cstdlib>

struct AdmpcSolver {
    AdmpcConfig cfg;
    AdmpcConfig* d_cfg;
    int device;
    int num_cu;
    int use_dense;           // N = 20 fp64 steps run the fused condensed kernel (admpc_fused20.hip) unless ADMPC_QP=riccati
    int use_seg;             // N = 40 / 60 / 80 fp64 steps without GP models run the segmented condensed kernel (admpc_seg.hip; with GP models on ADMPC_QP=seg); ADMPC_QP=riccati: kernel R
    int* d_tick;             // 2 x [128 + 64 cap_fused] tickets, exit counter and work-order bins of the persistent kernels: two states used alternately (work_order.h)
    int tick_flip;           // which of the two the last launch used
    int cap_fused;
    double* d_slot;          // per-wave slot buffers of the fused / segmented kernel (H while its factor holds the LDS buffer), allocated at the first launch
    // Workspaces, each grown on demand by the path that needs it (admpc_reserve sizes the handle's default path up front):
    int cap;                 // instances: d_status
    int32_t* d_status;       // [cap] used when the caller passes status == NULL
    int cap_lin;             // kernel A's output: every path but the fused one
    double* d_GT;            // [cap_lin][N][42]
    double* d_bl;            // [cap_lin][N][7]
    int* d_sched;            // [SCHED_HDR] ticket counter of kernel R
    int qmask;               // 7 when only x, y, psi carry tracking weights (specialised condensing kernel), else 127
    int cap_row;             // kernel R: every fp32 solve, fp64 for N != 20, every solve that asks for multipliers
    int row_elem;            // element width (8 / 4) the row workspace was sized for
    double* d_ws;            // [cap_row][N+1][38] workspace of the row kernel (sweep-private state, L2-resident)
    int32_t* d_split;        // [2 cap_row + 1] keys, order and count of the row kernel's second phase (split batches)
    double* d_dump;          // [cap_row][16 + 31 N] LDS regions of the deferred instances between the two phases
    double* d_mult;          // [cap_mult][(N+1) 7 + 20 N] multipliers between the passes of an SQP solve with a tolerance, when the caller keeps none
    int cap_mult, mult_elem;
    int row_chunk;           // > 0: cap of the chunk size of kernel-R solves (ADMPC_ROWQP_CHUNK; tests)
    int split_mode;          // -1: split batches of more than one round of waves (default), 0: never, 1: always (ADMPC_ROWQP_SPLIT)
    double* d_pairs;         // [1 + 256] 16-byte (cost, index) records: this rank's, then the all-gathered ones (admpc_argmin_global)
};

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(ADMPC_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

// kernel R (admpc_rowqp.hip)
extern "C" int admpc_rowqp_plan(int N, int elem, int B, int num_cu, int* rows, int* inst_stride, int* lds_bytes, int* grid);
extern "C" void admpc_rowqp_prepare(void);
extern "C" void admpc_rowqp_launch_f64(int grid, int lds_bytes, hipStream_t st, const AdmpcConfig* d_cfg, int B, int rows, int inst_stride,
        const double* x0, const double* yref, const double* yref_e, const double* GT, const double* bl,
        double* xbar, double* ubar, double* cost, int32_t* stat, int32_t* iters, double* pi, double* ineq, double* ws, int first, int* ticket, int32_t* split, double* dump);
extern "C" void admpc_rowqp_launch_f32(int grid, int lds_bytes, hipStream_t st, const AdmpcConfig* d_cfg, int B, int rows, int inst_stride,
        const float* x0, const float* yref, const float* yref_e, const float* GT, const float* bl,
        float* xbar, float* ubar, float* cost, int32_t* stat, int32_t* iters, float* pi, float* ineq, float* ws, int first, int* ticket, int32_t* split, float* dump);

// fused N = 20 step (admpc_fused20.hip)
extern "C" void admpc_fused20_launch(int num_cu, hipStream_t st, const AdmpcConfig* d_cfg, int B, int qmask,
        const double* x0, const double* yref, const double* yref_e, const double* p, double* xbar, double* ubar,
        double* cost, int32_t* stat, int32_t* iters, int first, int* sched2, int cap, int flip, double* slotbuf);
extern "C" size_t admpc_fused20_slot_doubles(int num_cu);
extern "C" size_t admpc_fused20_sched_ints(int cap);
// segmented condensed step, N = 40 / 60 / 80 fp64 (admpc_seg.hip)
extern "C" int admpc_seg_supports(int N);
extern "C" void admpc_seg_launch(int N, int num_cu, hipStream_t st, const AdmpcConfig* d_cfg, int B, int qmask,
        const double* x0, const double* yref, const double* yref_e, const double* p, double* xbar, double* ubar,
        double* cost, int32_t* stat, int32_t* iters, int first, int* sched2, int cap, int flip, double* hslot);
extern "C" size_t admpc_seg_slot_doubles(int num_cu);

extern "C" {

const char* admpc_last_error(void) { return g_err.c_str(); }
// for the other translation units of the library (admpc_quad.hip)
int admpc_set_error(int code, const char* msg) { return fail(code, msg ? msg : ""); }
// a refusal of the entry point `who`
int admpc_refuse(const char* who, const char* what)
{
    char msg[220];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return fail(ADMPC_EINVAL, msg);
}
// for the entry points that take a device and no handle
int admpc_device_check(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(ADMPC_ENODEV, "no such device");
    return ADMPC_OK;
}
const char* admpc_version(void) { return "admpc-mi355x 0.1 (gfx950)"; }
// for the control step (admpc_step.hip): the problem a handle solves and the device it lives on
const AdmpcConfig* admpc_solver_config(const AdmpcSolver* s, int* device)
{
    if (device) *device = s->device;
    return &s->cfg;
}
// for the plant step (admpc_plant.hip): the device copy of that problem, as the kernels read it
const AdmpcConfig* admpc_solver_config_device(const AdmpcSolver* s) { return s->d_cfg; }
// for the install of a fitted GP (admpc_learn.hip): the same copy, to be written
AdmpcConfig* admpc_solver_config_device_rw(AdmpcSolver* s) { return s->d_cfg; }

int admpc_default_config(AdmpcConfig* c, int N, double Ts)
{
    if (!c || N < 2 || N > ADMPC_MAX_N || !(Ts > 0)) return fail(ADMPC_EINVAL, "admpc_default_config: bad N/Ts");
    memset(c, 0, sizeof *c);
    c->N = N; c->ipm_iter_max = 50; c->sqp_iters = 1; c->n_gp = 0; c->Ts = Ts;
    const double q[NX] = {10, 10, 100, 0, 0, 0, 0}, r[NU] = {1, 100};          // create_ros_ad_mpc.py:58-59
    for (int i = 0; i < NX; ++i) { c->W[i] = q[i]; c->We[i] = q[i] * 1e-6; }   // ad_3d_optimizer.py:149-151
    for (int j = 0; j < NU; ++j) c->W[NX + j] = r[j];
    c->lbu[0] = -10; c->lbu[1] = -3; c->ubu[0] = 5; c->ubu[1] = 3;             // ad_3d.py:66-71
    c->lbx_delta = -0.52; c->ubx_delta = 0.52;
    c->zl = c->zu = 10;                                                        // ad_3d_optimizer.py:171-173
    const double mass = 1500, f_mass = 900, r_mass = mass - f_mass, Lw = 2.7;  // ad_3d.py:47-60
    c->mass = mass; c->L_F = Lw * (1 - f_mass / mass); c->L_R = Lw * (1 - r_mass / mass);
    c->Iz = c->L_F * c->L_R * (r_mass + f_mass);
    c->Cf = f_mass * 0.5 * 9.81 * 0.165 * 180 / 3.14195; c->Cr = r_mass * 0.5 * 9.81 * 0.165 * 180 / 3.14195;
    c->ipm_mu0 = 1.0; c->ipm_thr0 = 0.1; c->ipm_tol_comp = 1e-8; c->ipm_tol_res = 1e-8; c->ipm_tol_step = 1e30;      // HPIPM BALANCE's levels (the reference's setting), no step test; admpc.h
    c->ipm_try_unconstrained = 1.0; c->ipm_warm_thr = 0.01; c->ipm_warm_restart = 0.1; c->ipm_fallback_iter = 30.0;
    return ADMPC_OK;
}

static int validate(const AdmpcConfig* c)
{
    if (c->N < 2 || c->N > ADMPC_MAX_N) return fail(ADMPC_EINVAL, "N out of range [2,128]");
    if (!(c->Ts > 0)) return fail(ADMPC_EINVAL, "Ts must be positive");
    if (c->n_gp < 0 || c->n_gp > ADMPC_GP_MAX) return fail(ADMPC_EINVAL, "n_gp out of range");
    for (int g = 0; g < c->n_gp; ++g) {
        const AdmpcGp& gp = c->gp[g];
        bool okf = gp.n_feat >= 1 && gp.n_feat <= ADMPC_GP_MAX_FEAT;
        for (int d = 0; okf && d < gp.n_feat; ++d) okf = gp.feat[d] >= 3 && gp.feat[d] <= 8;
        if (gp.out < 3 || gp.out > 5 || !okf || gp.n_points < 0 || gp.n_points > ADMPC_GP_MAX_POINTS)
            return fail(ADMPC_EINVAL, "GP: out must be in {3,4,5}, 1..3 features in {3..8}, n_points <= 32");
    }
    if (!(c->W[NX] > 0 && c->W[NX + 1] > 0)) return fail(ADMPC_EINVAL, "input weights must be positive (strict convexity)");
    if (c->ipm_iter_max < 1) return fail(ADMPC_EINVAL, "ipm_iter_max < 1");
    if (!(c->sqp_tol >= 0)) return fail(ADMPC_EINVAL, "sqp_tol must be >= 0");
    if (!(c->ipm_mu0 > 0) || !(c->ipm_thr0 > 0) || !(c->ipm_warm_thr >= 0) || !(c->ipm_warm_restart >= 0 && c->ipm_warm_restart < 1) || !(c->ipm_fallback_iter >= 0 && c->ipm_fallback_iter <= 1e6)) return fail(ADMPC_EINVAL, "ipm_mu0, ipm_thr0 must be > 0, ipm_warm_thr >= 0, ipm_warm_restart in [0, 1), ipm_fallback_iter in [0, 1e6]");
    return ADMPC_OK;
}

int admpc_create(const AdmpcConfig* cfg, int device, AdmpcSolver** out)
{
    if (!cfg || !out) return fail(ADMPC_EINVAL, "admpc_create: null argument");
    int rc = validate(cfg); if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(ADMPC_ENODEV, "no HIP device");
    if (device < 0 || device >= ndev) return fail(ADMPC_ENODEV, "device index out of range");
    DeviceGuard guard(device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    AdmpcSolver* s = new (std::nothrow) AdmpcSolver();
    if (!s) return fail(ADMPC_ENOMEM, "out of host memory");
    s->cfg = *cfg; s->device = device; s->num_cu = prop.multiProcessorCount;
    {   // the row kernel must fit at least one instance per wave into the 160 KB of LDS
        int r_, st_, lb_, g_;
        if (admpc_rowqp_plan(cfg->N, 8, 1, s->num_cu, &r_, &st_, &lb_, &g_) != 0) { delete s; return fail(ADMPC_EINVAL, "horizon too long for the LDS-resident kernel"); }
    }
    s->cap = s->cap_lin = s->cap_row = 0; s->row_elem = 8; s->d_tick = nullptr; s->tick_flip = 0; s->d_slot = nullptr; s->cap_fused = 0;
    s->d_GT = nullptr; s->d_bl = nullptr; s->d_status = nullptr; s->d_ws = nullptr; s->d_pairs = nullptr; s->d_split = nullptr; s->d_dump = nullptr; s->d_mult = nullptr; s->cap_mult = 0; s->mult_elem = 0;
    {   // ADMPC_ROWQP_SPLIT=0 / 1: never / always run the row kernel in two phases (A/B tests); default: by batch size
        const char* e = getenv("ADMPC_ROWQP_SPLIT");
        s->split_mode = e && e[0] == '0' ? 0 : (e && e[0] == '1' ? 1 : -1);
        const char* c = getenv("ADMPC_ROWQP_CHUNK");
        s->row_chunk = c ? atoi(c) : 0;
    }
    {   // ADMPC_QP=riccati forces the stage-wise Riccati kernel (A/B tests); default: condensed kernel where instantiated
        const char* e = getenv("ADMPC_QP");
        s->use_dense = (cfg->N == 20) && !(e && strcmp(e, "riccati") == 0);
        // default at N = 40 (the reference's shipped horizon: 6.2 M solves/s against kernel R's 3.4 M at B = 4096), 60 and 80 (2.7 / 2.0 M against
        // 1.7 / 1.2 M; scripts/cmp_seg_rowqp.sh); ADMPC_QP=riccati selects kernel R there
        // (nominal model only: with GP residuals in the dynamics the linearisation can have strongly unstable modes -- random regressors are
        // arbitrary dynamics -- and eliminating 20 stages at a time loses what the stage-wise Riccati recursion keeps: the N = 40 + GP census
        // family came out 3e-6 off in the inputs on the segmented kernel, 1e-8 on kernel R; with GPs the default stays kernel R, ADMPC_QP=seg selects kernel S)
        s->use_seg = admpc_seg_supports(cfg->N) && (cfg->n_gp == 0 ? !(e && strcmp(e, "riccati") == 0) : (e && strcmp(e, "seg") == 0));
    }
    hipError_t e = hipMalloc((void**)&s->d_cfg, sizeof(AdmpcConfig));
    if (e != hipSuccess) { delete s; return fail(ADMPC_EHIP, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    e = hipMemcpy(s->d_cfg, cfg, sizeof(AdmpcConfig), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(s->d_cfg); delete s; return fail(ADMPC_EHIP, std::string("hipMemcpy: ") + hipGetErrorString(e)); }
    s->d_sched = nullptr;
    s->qmask = 7;
    for (int c = 3; c < NX; ++c) if (cfg->W[c] != 0.0 || cfg->We[c] != 0.0) s->qmask = 127;
    // opt in to > 64 KB of dynamic LDS
    admpc_rowqp_prepare();
    *out = s;
    return ADMPC_OK;
}

void admpc_destroy(AdmpcSolver* s)
{
    if (!s) return;
    DeviceGuard guard(s->device);
    (void)hipFree(s->d_cfg);
    if (s->d_tick) (void)hipFree(s->d_tick);
    if (s->d_slot) (void)hipFree(s->d_slot);
    if (s->d_sched) (void)hipFree(s->d_sched);
    if (s->d_GT) (void)hipFree(s->d_GT);
    if (s->d_bl) (void)hipFree(s->d_bl);
    if (s->d_status) (void)hipFree(s->d_status);
    if (s->d_ws) (void)hipFree(s->d_ws);
    if (s->d_split) (void)hipFree(s->d_split);
    if (s->d_mult) (void)hipFree(s->d_mult);
    if (s->d_dump) (void)hipFree(s->d_dump);
    if (s->d_pairs) (void)hipFree(s->d_pairs);
    delete s;
}

// Kernel R addresses its arrays with 32-bit byte offsets from the (64-bit) array bases: a batch whose largest array would pass 4 GB
// is solved in consecutive chunks on the caller's stream (same results: instances are independent; the workspace is sized for one
// chunk).  ADMPC_ROWQP_CHUNK=n caps the chunk (tests).
static int rowqp_chunk(const AdmpcSolver* s, int N, int elem)
{
    const unsigned long long per = (unsigned long long)(N + 1) * 42ull * (unsigned long long)elem;
    unsigned long long m = ((1ull << 32) - 1ull) / per;
    if (m > 0x7fffffffull) m = 0x7fffffffull;
    if (s->row_chunk > 0 && (unsigned long long)s->row_chunk < m) m = (unsigned long long)s->row_chunk;
    return (int)m;
}

// ---- workspaces: grown on demand, each by the path that uses it.  Growing synchronises the device (nothing may still be using
//      the old block) and allocates; admpc_reserve does it up front for the handle's default path.
#define GROW(ptr, type, count) do { if (ptr) (void)hipFree(ptr); ptr = nullptr; HIPCHK(hipMalloc((void**)&(ptr), (size_t)(count) * sizeof(type))); } while (0)
static int ensure_status(AdmpcSolver* s, int B)
{
    if (B <= s->cap) return ADMPC_OK;
    HIPCHK(hipDeviceSynchronize());
    s->cap = 0;
    GROW(s->d_status, int32_t, B);
    s->cap = B;
    return ADMPC_OK;
}
static int ensure_sched(AdmpcSolver* s)                         // kernel R's ticket counter
{
    if (s->d_sched) return ADMPC_OK;
    HIPCHK(hipDeviceSynchronize());
    GROW(s->d_sched, int, SCHED_HDR);
    return ADMPC_OK;
}
static int ensure_lin(AdmpcSolver* s, int B)                    // kernel A's output
{
    int rc = ensure_sched(s); if (rc) return rc;
    if (B <= s->cap_lin) return ADMPC_OK;
    HIPCHK(hipDeviceSynchronize());
    const size_t N = (size_t)s->cfg.N;
    s->cap_lin = 0;
    GROW(s->d_GT, double, (size_t)B * N * GTS);
    GROW(s->d_bl, double, (size_t)B * N * NX);
    s->cap_lin = B;
    return ADMPC_OK;
}
static int ensure_fused(AdmpcSolver* s, int B)                  // fused N = 20 step and segmented kernel: one slot buffer per resident
{                                                                // wave, the work-order lists
    // one packed Hessian per resident wave (its LDS buffer doubles as the factor's): fused kernel and segmented kernel alike
    if (!s->d_slot && !s->use_seg) HIPCHK(hipMalloc((void**)&s->d_slot, admpc_fused20_slot_doubles(s->num_cu) * sizeof(double)));
    if (!s->d_slot && s->use_seg) HIPCHK(hipMalloc((void**)&s->d_slot, admpc_seg_slot_doubles(s->num_cu) * sizeof(double)));
    if (B <= s->cap_fused) return ADMPC_OK;
    HIPCHK(hipDeviceSynchronize());
    s->cap_fused = 0;
    GROW(s->d_tick, int, admpc_fused20_sched_ints(B));
    HIPCHK(hipMemset(s->d_tick, 0, admpc_fused20_sched_ints(B) * sizeof(int)));
    HIPCHK(hipDeviceSynchronize());                 // the memset runs on the null stream: the caller's (non-blocking) stream must not overtake it
    s->cap_fused = B;
    return ADMPC_OK;
}
static int ensure_row(AdmpcSolver* s, int B, int elem)          // kernel R; sized by the element width of the solve
{
    int rc = ensure_lin(s, B); if (rc) return rc;
    if (B <= s->cap_row && elem <= s->row_elem) return ADMPC_OK;
    HIPCHK(hipDeviceSynchronize());
    const size_t N = (size_t)s->cfg.N;
    const int nb = B > s->cap_row ? B : s->cap_row;
    const int ne = (s->cap_row > 0 && s->row_elem > elem) ? s->row_elem : elem;
    s->cap_row = 0;
    if (s->d_ws) (void)hipFree(s->d_ws); s->d_ws = nullptr;
    if (s->d_dump) (void)hipFree(s->d_dump); s->d_dump = nullptr;
    HIPCHK(hipMalloc((void**)&s->d_ws, (size_t)nb * (N + 1) * 38 * (size_t)ne));          // RQ_RW = 38 values per record
    HIPCHK(hipMalloc((void**)&s->d_dump, (size_t)nb * (16 + 31 * N) * (size_t)ne));
    GROW(s->d_split, int32_t, (size_t)2 * nb + 1);
    s->cap_row = nb; s->row_elem = ne;
    return ADMPC_OK;
}

static int ensure_mult(AdmpcSolver* s, int B, int elem)         // SQP solves with a tolerance whose caller passes no multiplier arrays
{
    if (B <= s->cap_mult && elem <= s->mult_elem) return ADMPC_OK;
    HIPCHK(hipDeviceSynchronize());
    const size_t N = (size_t)s->cfg.N;
    const int nb = B > s->cap_mult ? B : s->cap_mult;
    const int ne = elem > s->mult_elem ? elem : s->mult_elem;
    s->cap_mult = 0;
    if (s->d_mult) (void)hipFree(s->d_mult); s->d_mult = nullptr;
    HIPCHK(hipMalloc((void**)&s->d_mult, (size_t)nb * ((N + 1) * NX + 20 * N) * (size_t)ne));
    s->cap_mult = nb; s->mult_elem = ne;
    return ADMPC_OK;
}

int admpc_reserve(AdmpcSolver* s, int B)
{
    if (!s || B < 0) return fail(ADMPC_EINVAL, "admpc_reserve: bad argument");
    DeviceGuard guard(s->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    int rc = ensure_status(s, B); if (rc) return rc;
    const bool tol_on = s->cfg.sqp_iters > 1 && s->cfg.sqp_tol > 0.0;  // such solves run on the row kernel at every horizon (solve_impl)
    if ((s->use_dense || s->use_seg) && !tol_on) return ensure_fused(s, B);      // no per-instance workspace
    const int chunk = rowqp_chunk(s, s->cfg.N, 8);
    rc = ensure_row(s, B < chunk ? B : chunk, 8); if (rc) return rc;
    return tol_on ? ensure_mult(s, B < chunk ? B : chunk, 8) : ADMPC_OK;
}

// Two phases for the row kernel (admpc_rowqp.hip)?  Only with the unconstrained trial on; by default when the batch is more than one
// round of waves (up to one round every instance starts at t = 0 anyway: -4 .. +4 % measured; at 1.2 rounds the split already wins 18 %).
static int32_t* rowqp_split(const AdmpcSolver* s, int B, int rows, int grid)
{
    if (s->cfg.ipm_try_unconstrained == 0.0 || s->split_mode == 0) return nullptr;
    const int nquads = (B + rows - 1) / rows;
    return (s->split_mode == 1 || nquads > grid) ? s->d_split : nullptr;
}

}  // extern "C"

// linearisation (kernel A) + row-mapped Riccati interior point (kernel R) for a batch of any size, T = double or float
template <class T>
static int solve_rows(AdmpcSolver* s, int B, const T* x0, const T* yref, const T* yref_e, const T* p, T* xbar, T* ubar,
                      T* cost, int32_t* stat, int32_t* iters, T* pi, T* ineq, hipStream_t st, int routed = 0)
{
    const int N = s->cfg.N, elem = (int)sizeof(T);
    const int chunk = rowqp_chunk(s, N, elem);
    const int nsqp = s->cfg.sqp_iters > 0 ? s->cfg.sqp_iters : 1;
    const bool tol_on = nsqp > 1 && s->cfg.sqp_tol > 0.0;      // acados' residual test in front of every QP but the first (admpc_nlp_res_kernel)
    { int rc = ensure_row(s, B < chunk ? B : chunk, elem); if (rc) return rc; }
    if (tol_on && !pi) { int rc = ensure_mult(s, B < chunk ? B : chunk, elem); if (rc) return rc; }
    for (long off = 0; off < (long)B; off += chunk) {
        const int nb = (long)B - off < (long)chunk ? (int)((long)B - off) : chunk;
        int rows, stride, ldsb, gridR;
        if (admpc_rowqp_plan(N, elem, nb, s->num_cu, &rows, &stride, &ldsb, &gridR) != 0) return fail(ADMPC_EINVAL, "horizon too long for the LDS-resident kernel");
        const long totalA = (long)nb * N * 3;
        int gridA = (int)((totalA + LIN_TASKS - 1) / LIN_TASKS);
        if (gridA > s->num_cu * 64) gridA = s->num_cu * 64;
        const T* cx0 = x0 + off * NX; const T* cyr = yref + off * N * NY; const T* cye = yref_e + off * NX; const T* cp = p + off;
        T* cxb = xbar + off * (N + 1) * NX; T* cub = ubar + off * N * NU;
        T* cco = cost ? cost + off : nullptr; int32_t* cst = stat + off; int32_t* cit = iters ? iters + off : nullptr;
        T* cpi = pi ? pi + off * (N + 1) * NX : nullptr; T* ciq = ineq ? ineq + off * N * 20 : nullptr;
        if (tol_on && !pi) { cpi = (T*)s->d_mult; ciq = cpi + (size_t)nb * (N + 1) * NX; }      // the chunk's multipliers live between its passes only
        for (int sq = 0; sq < nsqp; ++sq) {
            const int first = (sq == 0 && !routed) ? 1 : 0;      // routed: the status array says which instances are this handle's (0) from the start
            hipLaunchKernelGGL(admpc_linearize_kernel<T>, dim3(gridA), dim3(LIN_BLOCK), 0, st, s->d_cfg, nb, (const T*)cxb, (const T*)cub, cp,
                               first ? (const int32_t*)nullptr : (const int32_t*)cst, (T*)s->d_GT, (T*)s->d_bl, s->d_sched);
            if (tol_on && sq > 0)
                hipLaunchKernelGGL(admpc_nlp_res_kernel<T>, dim3(nb < s->num_cu * 32 ? nb : s->num_cu * 32), dim3(WAVE), 0, st, s->d_cfg, nb, cx0, cyr, cye,
                                   (const T*)cxb, (const T*)cub, (const T*)s->d_GT, (const T*)s->d_bl, (const T*)cpi, (const T*)ciq, cst, (T*)nullptr);
            if constexpr (sizeof(T) == 8)
                admpc_rowqp_launch_f64(gridR, ldsb, st, s->d_cfg, nb, rows, stride, cx0, cyr, cye, (const double*)s->d_GT, (const double*)s->d_bl,
                                       cxb, cub, cco, cst, cit, cpi, ciq, s->d_ws, first, s->d_sched, rowqp_split(s, nb, rows, gridR), s->d_dump);
            else
                admpc_rowqp_launch_f32(gridR, ldsb, st, s->d_cfg, nb, rows, stride, cx0, cyr, cye, (const float*)s->d_GT, (const float*)s->d_bl,
                                       cxb, cub, cco, cst, cit, cpi, ciq, (float*)s->d_ws, first, s->d_sched, rowqp_split(s, nb, rows, gridR), (float*)s->d_dump);
        }
    }
    return ADMPC_OK;
}

extern "C" {

int admpc_solve_batch_ex(AdmpcSolver* s, int B, const double* x0, const double* yref, const double* yref_e, const double* p,
                         double* xbar, double* ubar, double* cost, int32_t* status, int32_t* iters, double* pi, double* ineq, void* stream);

int admpc_solve_batch(AdmpcSolver* s, int B, const double* x0, const double* yref, const double* yref_e, const double* p,
                      double* xbar, double* ubar, double* cost, int32_t* status, int32_t* iters, void* stream)
{
    return admpc_solve_batch_ex(s, B, x0, yref, yref_e, p, xbar, ubar, cost, status, iters, nullptr, nullptr, stream);
}

/* admpc_solve_batch plus the multipliers of the returned iterate (acados store_iterate contents).  With pi / ineq given the step
 * runs on the row kernel at every horizon (the condensed N = 20 pipeline eliminates the states and carries no multipliers of the
 * dynamics).  routed (admpc_solve_batch_routed): `status` arrives filled -- 0 for the instances this handle is to solve, non-zero for
 * the others, which every kernel then leaves alone (the mechanism that skips failed / converged instances in later SQP passes). */
static int solve_impl(AdmpcSolver* s, int B, const double* x0, const double* yref, const double* yref_e, const double* p,
                      double* xbar, double* ubar, double* cost, int32_t* status, int32_t* iters,
                      double* pi, double* ineq, void* stream, int routed)
{
    const bool snap = pi != nullptr || ineq != nullptr;
    if (snap && !(pi && ineq)) return fail(ADMPC_EINVAL, "pi and ineq must be given together");
    if (!s) return fail(ADMPC_EINVAL, "null solver");
    if (B < 0) return fail(ADMPC_EINVAL, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!x0 || !yref || !yref_e || !p || !xbar || !ubar) return fail(ADMPC_EINVAL, "null array argument");
    DeviceGuard guard(s->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    const int N = s->cfg.N;
    const int nsqp = s->cfg.sqp_iters > 0 ? s->cfg.sqp_iters : 1;
    // the condensed N = 20 kernels carry no multipliers: solves that return them, and SQP solves with a tolerance (whose stopping test
    // needs them between the passes), run on the row kernel at every horizon
    const bool dense = s->use_dense && !snap && !(nsqp > 1 && s->cfg.sqp_tol > 0.0);
    {   // workspaces of the path this call takes (no-ops once sized: admpc_reserve up front keeps the default path allocation-free)
        int rc = ensure_status(s, B); if (rc) return rc;
        if (dense) { rc = ensure_fused(s, B); if (rc) return rc; }
    }
    hipStream_t st = (hipStream_t)stream;
    int32_t* stat = status ? status : s->d_status;
    if (s->use_seg && !snap && !(nsqp > 1 && s->cfg.sqp_tol > 0.0)) {
        // N = 40 / 60 / 80: S cooperating waves per instance, each condensing 20 stages; no workspace, no kernel boundary (admpc_seg.hip)
        int rc = ensure_fused(s, B); if (rc) return rc;
        for (int sq = 0; sq < nsqp; ++sq)
            admpc_seg_launch(N, s->num_cu, st, s->d_cfg, B, s->qmask, x0, yref, yref_e, p, xbar, ubar, cost, stat, iters, (sq == 0 && !routed) ? 1 : 0, s->d_tick, s->cap_fused, (s->tick_flip ^= 1), s->d_slot);
        HIPCHK(hipGetLastError());
        return ADMPC_OK;
    }
    if (!dense) {      // every horizon but N = 20, and every solve that asks for multipliers: kernel A + kernel R, in chunks if need be
        int rc = solve_rows<double>(s, B, x0, yref, yref_e, p, xbar, ubar, cost, stat, iters, pi, ineq, st, routed); if (rc) return rc;
        if (nsqp > 1 && s->cfg.sqp_tol > 0.0)
            hipLaunchKernelGGL(admpc_sqp_finalize_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, stat);
        HIPCHK(hipGetLastError());
        return ADMPC_OK;
    }
    // shooting, condensing, interior point and expansion of an instance in one persistent kernel: no workspace, no kernel boundary
    for (int sq = 0; sq < nsqp; ++sq)
        admpc_fused20_launch(s->num_cu, st, s->d_cfg, B, s->qmask, x0, yref, yref_e, p, xbar, ubar, cost, stat, iters, (sq == 0 && !routed) ? 1 : 0, s->d_tick, s->cap_fused, (s->tick_flip ^= 1), s->d_slot);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

int admpc_solve_batch_ex(AdmpcSolver* s, int B, const double* x0, const double* yref, const double* yref_e, const double* p,
                         double* xbar, double* ubar, double* cost, int32_t* status, int32_t* iters,
                         double* pi, double* ineq, void* stream)
{
    return solve_impl(s, B, x0, yref, yref_e, p, xbar, ubar, cost, status, iters, pi, ineq, stream, 0);
}

// ---- clustered GP ensembles (reference: one solver per cluster, chosen per solve by GPEnsemble.select_gp)
namespace {
#pragma clang fp contract(off)
// nearest centroid of z = [x; u][feats] (Euclidean distance as numpy / the reference computes it, ties -> lowest index): gp.py:738-770
__global__ void admpc_select_cluster_kernel(int B, int d, int f0, int f1, int f2, const double* __restrict__ xs, const double* __restrict__ us,
                                            int K, const double* __restrict__ cent, int32_t* __restrict__ route)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int f[3] = { f0, f1, f2 };
    double z[3];
    for (int j = 0; j < d; ++j) z[j] = f[j] < NX ? xs[(size_t)b * NX + f[j]] : us[(size_t)b * NU + f[j] - NX];
    double best = INFINITY; int bi = 0;
    for (int c = 0; c < K; ++c) {
        double acc = 0.0;
        for (int j = 0; j < d; ++j) { const double e = z[j] - cent[c * d + j]; acc = acc + e * e; }
        const double dist = __dsqrt_rn(acc);
        if (dist < best) { best = dist; bi = c; }
    }
    route[b] = bi;
}
// status array of one cluster's solve: 0 = this handle's instance, ADMPC_STATUS_SKIP = somebody else's
#define ADMPC_STATUS_SKIP (-2)
__global__ void admpc_route_fill_kernel(int B, const int32_t* __restrict__ route, int c, int32_t* __restrict__ tmp)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) tmp[b] = route[b] == c ? 0 : ADMPC_STATUS_SKIP;
}
__global__ void admpc_route_merge_kernel(int B, const int32_t* __restrict__ route, int c, const int32_t* __restrict__ tmp, int32_t* __restrict__ status)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && route[b] == c) status[b] = tmp[b];
}
// an instance routed to no cluster at all is reported as failed instead of being passed over in silence
__global__ void admpc_route_invalid_kernel(int B, const int32_t* __restrict__ route, int K, int32_t* __restrict__ status, double* __restrict__ cost, int32_t* __restrict__ iters)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && (route[b] < 0 || route[b] >= K)) { if (status) status[b] = ADMPC_STATUS_QP_FAILURE; if (cost) cost[b] = INFINITY; if (iters) iters[b] = 0; }
}
}

int admpc_select_cluster_batch(int device, int B, int n_feat, const int32_t* feats, const double* x_sel, const double* u_sel,
                               int K, const double* centroids, int32_t* route, void* stream)
{
    if (B < 0 || n_feat < 1 || n_feat > 3 || !feats || K < 1) return fail(ADMPC_EINVAL, "bad argument");
    if (B == 0) return ADMPC_OK;
    if (!x_sel || !u_sel || !centroids || !route) return fail(ADMPC_EINVAL, "null array argument");
    for (int j = 0; j < n_feat; ++j) if (feats[j] < 0 || feats[j] >= NX + NU) return fail(ADMPC_EINVAL, "feature index outside [x; u]");
    DeviceGuard guard(device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_select_cluster_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, n_feat, feats[0], n_feat > 1 ? feats[1] : 0,
                       n_feat > 2 ? feats[2] : 0, x_sel, u_sel, K, centroids, route);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

int admpc_solve_batch_routed(AdmpcSolver* const* solvers, int K, int B, const int32_t* route,
                             const double* x0, const double* yref, const double* yref_e, const double* p,
                             double* xbar, double* ubar, double* cost, int32_t* status, int32_t* iters, void* stream)
{
    if (!solvers || K < 1) return fail(ADMPC_EINVAL, "bad argument");
    if (B < 0) return fail(ADMPC_EINVAL, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!route || !x0 || !yref || !yref_e || !p || !xbar || !ubar) return fail(ADMPC_EINVAL, "null array argument");
    for (int c = 0; c < K; ++c) {
        if (!solvers[c]) return fail(ADMPC_EINVAL, "null solver");
        if (solvers[c]->device != solvers[0]->device || solvers[c]->cfg.N != solvers[0]->cfg.N) return fail(ADMPC_EINVAL, "the cluster solvers must share device and horizon");
    }
    DeviceGuard guard(solvers[0]->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    const dim3 g((B + 255) / 256), blk(256);
    hipLaunchKernelGGL(admpc_route_invalid_kernel, g, blk, 0, st, B, route, K, status, cost, iters);
    for (int c = 0; c < K; ++c) {
        AdmpcSolver* s = solvers[c];
        int rc = ensure_status(s, B); if (rc) return rc;
        hipLaunchKernelGGL(admpc_route_fill_kernel, g, blk, 0, st, B, route, c, s->d_status);
        rc = solve_impl(s, B, x0, yref, yref_e, p, xbar, ubar, cost, s->d_status, iters, nullptr, nullptr, stream, 1); if (rc) return rc;
        if (status) hipLaunchKernelGGL(admpc_route_merge_kernel, g, blk, 0, st, B, route, c, (const int32_t*)s->d_status, status);
    }
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

/* fp32 storage and arithmetic (BASELINE configs[4]): same arguments as admpc_solve_batch with float arrays. */
int admpc_solve_batch_f32(AdmpcSolver* s, int B, const float* x0, const float* yref, const float* yref_e, const float* p,
                          float* xbar, float* ubar, float* cost, int32_t* status, int32_t* iters, void* stream)
{
    if (!s) return fail(ADMPC_EINVAL, "null solver");
    if (B < 0) return fail(ADMPC_EINVAL, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!x0 || !yref || !yref_e || !p || !xbar || !ubar) return fail(ADMPC_EINVAL, "null array argument");
    // beyond this horizon the float recursion on GP-augmented dynamics returns status 0 on iterates without a correct digit (admpc.h)
    if (s->cfg.n_gp > 0 && s->cfg.N > ADMPC_F32_GP_MAX_N)
        return fail(ADMPC_EINVAL, "fp32 solve of a model with GP residuals: horizon beyond ADMPC_F32_GP_MAX_N (28), use the fp64 entry");
    DeviceGuard guard(s->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    { int rc = ensure_status(s, B); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    int32_t* stat = status ? status : s->d_status;
    const int nsqp = s->cfg.sqp_iters > 0 ? s->cfg.sqp_iters : 1;
    { int rc = solve_rows<float>(s, B, x0, yref, yref_e, p, xbar, ubar, cost, stat, iters, (float*)nullptr, (float*)nullptr, st); if (rc) return rc; }
    if (nsqp > 1 && s->cfg.sqp_tol > 0.0)
        hipLaunchKernelGGL(admpc_sqp_finalize_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, stat);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

int admpc_nlp_residuals_batch(AdmpcSolver* s, int B, const double* x0, const double* yref, const double* yref_e, const double* p,
                              const double* xbar, const double* ubar, const double* pi, const double* ineq, double* res, void* stream)
{
    if (!s) return fail(ADMPC_EINVAL, "null solver");
    if (B < 0) return fail(ADMPC_EINVAL, "negative batch");
    if (B == 0) return ADMPC_OK;
    if (!x0 || !yref || !yref_e || !p || !xbar || !ubar || !pi || !ineq || !res) return fail(ADMPC_EINVAL, "null array argument");
    const int N = s->cfg.N;
    if ((double)B * N * GTS * 8.0 > 4.0e9) return fail(ADMPC_EINVAL, "batch too large for one linearisation: split it");
    DeviceGuard guard(s->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    { int rc = ensure_status(s, B); if (rc) return rc; rc = ensure_lin(s, B); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    const long totalA = (long)B * N * 3;
    int gridA = (int)((totalA + LIN_TASKS - 1) / LIN_TASKS);
    if (gridA > s->num_cu * 64) gridA = s->num_cu * 64;
    HIPCHK(hipMemsetAsync(s->d_status, 0, (size_t)B * sizeof(int32_t), st));
    hipLaunchKernelGGL(admpc_linearize_kernel<double>, dim3(gridA), dim3(LIN_BLOCK), 0, st, s->d_cfg, B, xbar, ubar, p,
                       (const int32_t*)nullptr, s->d_GT, s->d_bl, s->d_sched);
    hipLaunchKernelGGL(admpc_nlp_res_kernel<double>, dim3(B < s->num_cu * 32 ? B : s->num_cu * 32), dim3(WAVE), 0, st, s->d_cfg, B, x0, yref, yref_e,
                       xbar, ubar, (const double*)s->d_GT, (const double*)s->d_bl, pi, ineq, s->d_status, res);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

}  // extern "C"

template <class T>
static int shoot_impl(AdmpcSolver* s, int B, const T* xbar, const T* ubar, const T* p, T* phi, T* A, T* Bm, void* stream)
{
    if (!s || B < 0) return fail(ADMPC_EINVAL, "bad argument");
    if (B == 0) return ADMPC_OK;
    if (!xbar || !ubar || !p || !phi || !A || !Bm) return fail(ADMPC_EINVAL, "null array argument");
    DeviceGuard guard(s->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    long total = (long)B * s->cfg.N * 3;
    int grid = (int)((total + LIN_TASKS - 1) / LIN_TASKS); if (grid > s->num_cu * 32) grid = s->num_cu * 32;
    hipLaunchKernelGGL(admpc_shoot_kernel<T>, dim3(grid), dim3(WAVE), 0, (hipStream_t)stream, s->d_cfg, B, xbar, ubar, p, phi, A, Bm);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

extern "C" {

int admpc_shoot_batch(AdmpcSolver* s, int B, const double* xbar, const double* ubar, const double* p,
                      double* phi, double* A, double* Bm, void* stream)
{
    return shoot_impl<double>(s, B, xbar, ubar, p, phi, A, Bm, stream);
}

int admpc_shoot_batch_f32(AdmpcSolver* s, int B, const float* xbar, const float* ubar, const float* p,
                          float* phi, float* A, float* Bm, void* stream)
{
    return shoot_impl<float>(s, B, xbar, ubar, p, phi, A, Bm, stream);
}

int admpc_argmin(AdmpcSolver* s, const double* cost, int B, int64_t index_offset, double* val, int64_t* idx, void* stream)
{
    if (!s || !cost || !val || !idx || B <= 0) return fail(ADMPC_EINVAL, "bad argument");
    DeviceGuard guard(s->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_argmin_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, cost, B, index_offset, val, idx);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

int admpc_argmin_pairs(AdmpcSolver* s, const double* pairs, int W, double* val, int64_t* idx, void* stream)
{
    if (!s || W <= 0) return fail(ADMPC_EINVAL, "bad argument");
    if (!pairs || !val || !idx) return fail(ADMPC_EINVAL, "null array argument");
    DeviceGuard guard(s->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_argmin_pairs_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, pairs, W, val, idx);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

/* Host-side twin of admpc_argmin_pairs for records that were gathered into HOST memory (gloo / MPI hosts; the CPU tests of the
 * N > 1 path): same rules, same code (argmin_rule.h).  No device, no solver handle. */
int admpc_argmin_pairs_host(const double* pairs, int W, double* val, int64_t* idx)
{
    if (W <= 0) return fail(ADMPC_EINVAL, "bad argument");
    if (!pairs || !val || !idx) return fail(ADMPC_EINVAL, "null array argument");
    ArgminBest b = argmin_identity();
    for (int i = 0; i < W; ++i) {
        int64_t ix; memcpy(&ix, pairs + 2 * i + 1, sizeof ix);
        argmin_fold(b, argmin_cost(pairs[2 * i]), ix);
    }
    *val = b.v; *idx = argmin_final_index(b);
    return ADMPC_OK;
}

// RCCL is resolved at the first call (dlopen): the library loads and every other entry point works on a host without it.
namespace {
typedef int (*nccl_allgather_t)(const void*, void*, size_t, int, void*, hipStream_t);
typedef int (*nccl_count_t)(void*, int*);
struct RcclApi { nccl_allgather_t all_gather; nccl_count_t comm_count; };
RcclApi g_rccl = { nullptr, nullptr };
std::once_flag g_rccl_once;
// The caller's ncclComm_t belongs to the RCCL copy that created it -- in a torch process that is the librccl torch bundles
// (SONAME librccl.so.1), not necessarily the one under /opt/rocm.  Look the symbols up in what the process has ALREADY loaded
// first (global scope, then the two sonames without loading anything); map a fresh copy only when none is there.
void rccl_lookup() {
    void* ag = dlsym(RTLD_DEFAULT, "ncclAllGather");
    void* cc = dlsym(RTLD_DEFAULT, "ncclCommCount");
    if (!(ag && cc)) {
        static const char* names[2] = { "librccl.so.1", "librccl.so" };
        for (int pass = 0; pass < 2 && !(ag && cc); ++pass)           // pass 0: RTLD_NOLOAD (already mapped copies only)
            for (int k = 0; k < 2 && !(ag && cc); ++k) {
                void* h = dlopen(names[k], RTLD_NOW | RTLD_GLOBAL | (pass == 0 ? RTLD_NOLOAD : 0));
                if (!h) continue;
                ag = dlsym(h, "ncclAllGather"); cc = dlsym(h, "ncclCommCount");
            }
    }
    if (ag && cc) { g_rccl.all_gather = (nccl_allgather_t)ag; g_rccl.comm_count = (nccl_count_t)cc; }
}
}

int admpc_argmin_global(AdmpcSolver* s, const double* cost, int B, int64_t index_offset, void* nccl_comm,
                        double* val, int64_t* idx, void* stream)
{
    if (!s || !cost || !val || !idx || B <= 0 || !nccl_comm) return fail(ADMPC_EINVAL, "bad argument");
    std::call_once(g_rccl_once, rccl_lookup);
    if (!g_rccl.all_gather || !g_rccl.comm_count) return fail(ADMPC_ENODEV, "librccl.so (ncclAllGather, ncclCommCount) not available");
    DeviceGuard guard(s->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    int nranks = 0;
    if (g_rccl.comm_count(nccl_comm, &nranks) != 0 || nranks < 1 || nranks > 256) return fail(ADMPC_EINVAL, "ncclCommCount failed or more than 256 ranks");
    if (!s->d_pairs) HIPCHK(hipMalloc((void**)&s->d_pairs, (size_t)(1 + 256) * 2 * sizeof(double)));
    hipStream_t st = (hipStream_t)stream;
    double* mine = s->d_pairs;                       // (cost, index bits)
    double* all = s->d_pairs + 2;
    hipLaunchKernelGGL(admpc_argmin_kernel, dim3(1), dim3(256), 0, st, cost, B, index_offset, mine, (int64_t*)(mine + 1));
    if (g_rccl.all_gather(mine, all, 2, 8 /* ncclFloat64 */, nccl_comm, st) != 0) return fail(ADMPC_EHIP, "ncclAllGather failed");
    hipLaunchKernelGGL(admpc_argmin_pairs_kernel, dim3(1), dim3(WAVE), 0, st, (const double*)all, nranks, val, idx);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

int admpc_shift_batch(AdmpcSolver* s, int B, double* xbar, double* ubar, const double* p, int rollout, void* stream)
{
    if (!s || B < 0) return fail(ADMPC_EINVAL, "bad argument");
    if (B == 0) return ADMPC_OK;
    if (!xbar || !ubar || (rollout && !p)) return fail(ADMPC_EINVAL, "null array argument");
    DeviceGuard guard(s->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    const long total = (long)B * 3;
    long grid = (total + LIN_TASKS - 1) / LIN_TASKS;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(admpc_shift_kernel, dim3((unsigned)grid), dim3(WAVE), 0, (hipStream_t)stream, s->d_cfg, B, xbar, ubar, p, rollout ? 1 : 0);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

int admpc_epilogue_batch(AdmpcSolver* s, int B, const double* xopt, const double* uopt, const double* xref_xy,
                         float* ack, int32_t* valid, void* stream)
{
    if (!s || B < 0) return fail(ADMPC_EINVAL, "bad argument");
    if (B == 0) return ADMPC_OK;
    if (!xopt || !uopt || !xref_xy || !ack || !valid) return fail(ADMPC_EINVAL, "null array argument");
    DeviceGuard guard(s->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_epilogue_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->cfg.N, B, xopt, uopt, xref_xy, ack, valid);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

int admpc_actuation_batch(AdmpcSolver* s, int B, const double* xopt, const double* uopt, const double* xref_xy, const int32_t* status,
                          const double* steer_meas, int32_t* safe_count, int threshold, double* cost_io,
                          float* ack, int32_t* mode, int32_t* valid, void* stream)
{
    if (!s || B < 0 || threshold < 0) return fail(ADMPC_EINVAL, "bad argument");
    if (B == 0) return ADMPC_OK;
    if (!xopt || !uopt || !xref_xy || !status || !steer_meas || !safe_count || !ack || !mode || !valid) return fail(ADMPC_EINVAL, "null array argument");
    DeviceGuard guard(s->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_actuation_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->cfg.N, B, xopt, uopt, xref_xy, status,
                       steer_meas, safe_count, threshold, s->cfg.lbu[1], s->cfg.ubu[1], s->cfg.lbx_delta, s->cfg.ubx_delta, cost_io, ack, mode, valid);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

int admpc_resample_vel_batch(int device, int B, int H, int ld, const double* vx, const double* vy, double acc_max, double dt,
                             double* vel_ref, void* stream)
{
    if (B < 0 || H < 1 || ld < H) return fail(ADMPC_EINVAL, "admpc_resample_vel_batch: need H >= 1, ld >= H");
    if (B == 0) return ADMPC_OK;
    if (!vx || !vy || !vel_ref) return fail(ADMPC_EINVAL, "null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_resample_vel_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, H, ld, vx, vy, acc_max, dt, vel_ref);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

int admpc_waypoints_batch(int device, int M, int H, double dt, int B,
                          const double* vel, const double* x, const double* y, const double* psi, const double* psi_unwrapped,
                          const double* cdist, const double* curv,
                          const double* X_init, const double* Y_init, const double* psi_init,
                          double* out_ref, double* out_err, int32_t* out_stop, void* stream)
{
    if (M < 2 || H < 3 || H > WAVE || B < 0 || !(dt > 0)) return fail(ADMPC_EINVAL, "admpc_waypoints_batch: need M >= 2, 3 <= H <= 64, dt > 0");
    if (B == 0) return ADMPC_OK;
    if (!vel || !x || !y || !psi || !psi_unwrapped || !cdist || !curv || !X_init || !Y_init || !psi_init || !out_ref || !out_err || !out_stop)
        return fail(ADMPC_EINVAL, "null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    int grid = B < 4096 ? B : 4096;
    hipLaunchKernelGGL(admpc_waypoints_kernel, dim3(grid), dim3(WAVE), 0, (hipStream_t)stream, M, H, dt, B, vel, x, y, psi, psi_unwrapped, cdist, curv,
                       X_init, Y_init, psi_init, out_ref, out_err, out_stop);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

}  // extern "C"

// =============================================================================================
// include/admpc_fleet.h: a bank of paths, the generator against it, the arg-min per group
// =============================================================================================
struct AdmpcPathBank {
    int device, K, H;
    double dt;
    double* d_block;         // the ONE allocation: K descriptors (64 bytes each), then the columns of every path
    const PathDesc* d_desc;  // = d_block
    const double* d_cols;    // = d_block + 8 K
};

extern "C" {

// for the control step (admpc_step.hip): the horizon every path of the bank was laid out for, and the device it lives on
int admpc_path_bank_horizon(const AdmpcPathBank* bank, int* device)
{
    if (device) *device = bank->device;
    return bank->H;
}

// for the lane generator (admpc_lane.hip): the bank's table of K descriptors and its block of columns, its dt and its device; returns H
int admpc_path_bank_table(const AdmpcPathBank* bank, int* device, int* K, double* dt, const void** desc, const double** cols)
{
    *device = bank->device; *K = bank->K; *dt = bank->dt; *desc = bank->d_desc; *cols = bank->d_cols;
    return bank->H;
}

int admpc_path_bank_create(int device, int K, const AdmpcPath* paths, AdmpcPathBank** out)
{
    if (!out || !paths) return fail(ADMPC_EINVAL, "admpc_path_bank_create: null argument");
    if (K < 1) return fail(ADMPC_EINVAL, "admpc_path_bank_create: need K >= 1");
    size_t total = 0;
    for (int k = 0; k < K; ++k) {
        const AdmpcPath& p = paths[k];
        if (p.M < 2 || !p.vel || !p.x || !p.y || !p.psi || !p.psi_unwrapped || !p.cdist || !p.curv)
            return fail(ADMPC_EINVAL, "admpc_path_bank_create: path " + std::to_string(k) + " needs M >= 2 and seven columns");
        if (p.H != paths[0].H || p.dt != paths[0].dt)
            return fail(ADMPC_EINVAL, "admpc_path_bank_create: path " + std::to_string(k) + " differs from path 0 in H or dt");
        total += (size_t)7 * (size_t)p.M;
    }
    if (paths[0].H < 3 || paths[0].H > WAVE) return fail(ADMPC_EINVAL, "admpc_path_bank_create: H must be in [3, 64] (the waypoint kernel's horizon)");
    if (!(paths[0].dt > 0)) return fail(ADMPC_EINVAL, "admpc_path_bank_create: the paths need dt > 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(ADMPC_ENODEV, "no HIP device");
    if (device < 0 || device >= ndev) return fail(ADMPC_ENODEV, "device index out of range");
    DeviceGuard guard(device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    static_assert(sizeof(PathDesc) == 8 * sizeof(double), "a descriptor takes eight doubles of the block");
    AdmpcPathBank* b = new (std::nothrow) AdmpcPathBank();
    PathDesc* host = new (std::nothrow) PathDesc[K];
    if (!b || !host) { delete b; delete[] host; return fail(ADMPC_ENOMEM, "out of host memory"); }
    b->device = device; b->K = K; b->H = paths[0].H; b->dt = paths[0].dt; b->d_block = nullptr;
    const size_t head = (size_t)8 * K;
    hipError_t e = hipMalloc((void**)&b->d_block, (head + total) * sizeof(double));
    size_t at = 0;
    for (int k = 0; e == hipSuccess && k < K; ++k) {
        const AdmpcPath& p = paths[k];
        const double* col[7] = { p.vel, p.x, p.y, p.psi, p.psi_unwrapped, p.cdist, p.curv };
        host[k].M = p.M;
        for (int c = 0; e == hipSuccess && c < 7; ++c, at += (size_t)p.M) {
            host[k].off[c] = (int64_t)at;
            e = hipMemcpy(b->d_block + head + at, col[c], (size_t)p.M * sizeof(double), hipMemcpyDeviceToDevice);
        }
    }
    if (e == hipSuccess) e = hipMemcpy(b->d_block, host, (size_t)K * sizeof(PathDesc), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();               // the caller may free its columns as soon as this returns
    delete[] host;
    if (e != hipSuccess) {
        if (b->d_block) (void)hipFree(b->d_block);
        delete b;
        return fail(ADMPC_EHIP, std::string("admpc_path_bank_create: ") + hipGetErrorString(e));
    }
    b->d_desc = (const PathDesc*)b->d_block; b->d_cols = b->d_block + head;
    *out = b;
    return ADMPC_OK;
}

void admpc_path_bank_destroy(AdmpcPathBank* bank)
{
    if (!bank) return;
    DeviceGuard guard(bank->device);
    (void)hipFree(bank->d_block);
    delete bank;
}

int admpc_waypoints_bank_batch(const AdmpcPathBank* bank, int B, const int32_t* path_of,
                               const double* X_init, const double* Y_init, const double* psi_init,
                               double* out_ref, double* out_err, int32_t* out_stop, void* stream)
{
    if (!bank || B < 0) return fail(ADMPC_EINVAL, "admpc_waypoints_bank_batch: null bank or negative batch");
    if (B == 0) return ADMPC_OK;
    if (!path_of || !X_init || !Y_init || !psi_init || !out_ref || !out_err || !out_stop) return fail(ADMPC_EINVAL, "null array argument");
    DeviceGuard guard(bank->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    int grid = B < 4096 ? B : 4096;                                // as admpc_waypoints_batch
    hipLaunchKernelGGL(admpc_waypoints_bank_kernel, dim3(grid), dim3(WAVE), 0, (hipStream_t)stream, bank->K, bank->H, bank->dt, B, bank->d_desc,
                       bank->d_cols, path_of, X_init, Y_init, psi_init, out_ref, out_err, out_stop);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

int admpc_argmin_groups(AdmpcSolver* s, const double* cost, int G, int group, double* val, int64_t* idx, void* stream)
{
    if (!s || G < 0 || group < 1) return fail(ADMPC_EINVAL, "admpc_argmin_groups: need a solver, G >= 0, group >= 1");
    if ((long long)G * group > 0x7fffffffLL) return fail(ADMPC_EINVAL, "admpc_argmin_groups: G * group beyond INT32_MAX");
    if (!val || !idx) return fail(ADMPC_EINVAL, "admpc_argmin_groups: null output array");
    if (G == 0) return ADMPC_OK;
    if (!cost) return fail(ADMPC_EINVAL, "admpc_argmin_groups: null cost array");
    DeviceGuard guard(s->device);
    if (!guard.ok()) return fail(ADMPC_EHIP, "hipSetDevice failed");
    const int per_block = ARGMIN_GROUPS_WAVES * (group <= 16 ? 4 : 1);          // groups a block takes per round
    int grid = (G + per_block - 1) / per_block;
    if (grid > ARGMIN_GROUPS_GRID) grid = ARGMIN_GROUPS_GRID;
    hipLaunchKernelGGL(admpc_argmin_groups_kernel, dim3(grid), dim3(ARGMIN_GROUPS_WAVES * WAVE), 0, (hipStream_t)stream, cost, G, group, val, idx);
    HIPCHK(hipGetLastError());
    return ADMPC_OK;
}

}  // extern "C"
