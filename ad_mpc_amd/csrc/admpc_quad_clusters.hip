// admpc_quad_clusters.hip -- the centroids of a clustered GP ensemble found on the device (include/admpc_quad_clusters.h): the logged
// rollout, a Gaussian-mixture EM over the logged sample records, the install of its means as the ensemble's centroids, and the re-bin of
// the log under them.
//
//   pack     admpc_quad_gmm_pack_kernel        one thread per record [14] -> (z_0, z_1, z_2, flag): what an EM iteration reads
//   E        admpc_quad_gmm_e_kernel<K, START> 256-thread blocks striding over the packed records; the K component blocks staged in LDS once
//                                              per block; 10 K + 1 fp64 sums per thread in registers (K is a template argument: every index
//                                              into them is a constant after unrolling; a variable one would put them into scratch), reduced
//                                              by wave shuffles, then across the four waves through LDS: one row of partial per block.
//                                              START: hard responsibilities from the nearest initial mean (quad_route_dev.h) instead
//   M        admpc_quad_gmm_m_kernel           one wave: lane e adds column e of the partial rows in a fixed order, lanes 0 .. K - 1 each finish
//                                              one component (shifted moments, 3 x 3 Cholesky, precision factor), lane 0 the bound and the flags
//   install  admpc_quad_clusters_install_kernel, admpc_quad_centroids_set_kernel   one wave each: the means (sorted by the first feature) or
//                                              given centroids into the ensemble's device centroids, unless one is not finite
//
// No floating-point atomics and no ticket: two launches per iteration, each of which reads the converged / status flags and returns at
// once when one is set, so that the number of launches is fixed and a call can be captured.  The bin kernel and the observed run are
// admpc_quad_ensemble.hip's and admpc_quad_learn.hip's.
#include <stdio.h>
#include <math.h>
#include "admpc_host.h"
#include "../../include/admpc_quad_clusters.h"

#define QREC 14               // doubles per sample record, as admpc_quad_learn.hip lays it out
#define FEAT_LO 7             // clustering feature f reads entry f - FEAT_LO of a record
#define KMAX ADMPC_QUAD_CLUSTERS_MAX
#define GROW ADMPC_GMM_ROW
#define GPART ADMPC_GMM_PARTIAL
#define GSUMS 10              // per component: sum r, sum r D [3], sum r D D' [6]
#define GTHREADS 256

namespace {

#define NX ADMPC_NX           // model_dev.h wants the car's dimensions defined
#define NU ADMPC_NU
#define NY ADMPC_NY
#include "model_dev.h"

[[maybe_unused]] constexpr int QX = ADMPC_QUAD_NX, QU = ADMPC_QUAD_NU, QY = ADMPC_QUAD_NY;      // quad_model_dev.h speaks of them
typedef AdmpcQuadConfig Cfg;

#include "quad_model_dev.h"
#include "quad_route_dev.h"

static_assert(GPART == GSUMS * KMAX + 1, "a row of partial holds the sums of eight components and the log-likelihood");

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace

__global__ __launch_bounds__(GTHREADS) void admpc_quad_gmm_pack_kernel(long long M, int d, int f0, int f1, int f2, const double* __restrict__ rec,
                                                                       double* __restrict__ packed)
{
    for (long long i = (long long)blockIdx.x * GTHREADS + threadIdx.x; i < M; i += (long long)gridDim.x * GTHREADS) {
        const double* r = rec + i * QREC;
        const double z0 = r[f0 - FEAT_LO], z1 = d > 1 ? r[f1 - FEAT_LO] : 0.0, z2 = d > 2 ? r[f2 - FEAT_LO] : 0.0;
        const bool ok = r[QREC - 1] == 1.0 && isfinite(z0) && isfinite(z1) && isfinite(z2);
        double* p = packed + i * 4;
        p[0] = ok ? z0 : 0.0; p[1] = ok ? z1 : 0.0; p[2] = ok ? z2 : 0.0; p[3] = ok ? 1.0 : 0.0;
    }
}

// grid: a function of M alone (gmm_blocks below).  START: init [K][d] are the means, the responsibilities are hard; else gmm is read.
template <int K, bool START>
__global__ __launch_bounds__(GTHREADS) void admpc_quad_gmm_e_kernel(long long M, int d, const double* __restrict__ packed, const double* __restrict__ init,
                                                                    const double* __restrict__ gmm, const int32_t* __restrict__ info,
                                                                    double* __restrict__ partial)
{
    __shared__ double par[K][10];                 // mean [3], P [6], log w + sum log P_jj - d/2 log 2 pi
    __shared__ double red[GTHREADS / 64][GSUMS * K + 1];
    const int tid = (int)threadIdx.x;
    // the thread's first record is asked for in front of the flags and the component blocks, and every next one in front of the
    // arithmetic of the one before it: the latencies overlap
    const long long stride = (long long)gridDim.x * GTHREADS;
    long long i = (long long)blockIdx.x * GTHREADS + tid;
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, n3 = 0.0;
    if (i < M) { const double* p = packed + i * 4; n0 = p[0]; n1 = p[1]; n2 = p[2]; n3 = p[3]; }
    if (!START && (info[1] | info[2])) return;
    if (tid < K) {
        if (START) {
            for (int j = 0; j < 3; ++j) par[tid][j] = j < d ? init[tid * d + j] : 0.0;
            for (int j = 3; j < 10; ++j) par[tid][j] = 0.0;
        }
        else {
            const double* g = gmm + (1 + tid) * GROW;
            for (int j = 0; j < 3; ++j) par[tid][j] = g[1 + j];
            for (int j = 0; j < 6; ++j) par[tid][3 + j] = g[10 + j];
            par[tid][9] = log(g[0]) + g[16] - 0.5 * d * 1.8378770664093453;        // log 2 pi
        }
    }
    __syncthreads();
    double acc[K][GSUMS], lse = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int i = 0; i < GSUMS; ++i) acc[k][i] = 0.0;
    for (; i < M; i += stride) {
        const double x0 = n0, x1 = n1, x2 = n2, flag = n3;
        if (i + stride < M) { const double* p = packed + (i + stride) * 4; n0 = p[0]; n1 = p[1]; n2 = p[2]; n3 = p[3]; }
        if (flag == 0.0) continue;
        double r[K];
        if (START) {
            const double z[3] = { x0, x1, x2 };
            const int c = quad_nearest(z, d, K, init);
#pragma unroll
            for (int k = 0; k < K; ++k) r[k] = c == k ? 1.0 : 0.0;
        }
        else {
            double mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double D0 = x0 - par[k][0], D1 = x1 - par[k][1], D2 = x2 - par[k][2];
                const double y0 = D0 * par[k][3], y1 = D0 * par[k][4] + D1 * par[k][6], y2 = D0 * par[k][5] + D1 * par[k][7] + D2 * par[k][8];
                r[k] = par[k][9] - 0.5 * (y0 * y0 + y1 * y1 + y2 * y2);
                mx = r[k] > mx ? r[k] : mx;
            }
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) s += exp(r[k] - mx);
            const double l = mx + log(s);
            lse += l;
#pragma unroll
            for (int k = 0; k < K; ++k) r[k] = exp(r[k] - l);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double D0 = x0 - par[k][0], D1 = x1 - par[k][1], D2 = x2 - par[k][2];
            const double r0 = r[k] * D0, r1 = r[k] * D1, r2 = r[k] * D2;
            acc[k][0] += r[k];
            acc[k][1] += r0; acc[k][2] += r1; acc[k][3] += r2;
            acc[k][4] += r0 * D0; acc[k][5] += r0 * D1; acc[k][6] += r0 * D2;
            acc[k][7] += r1 * D1; acc[k][8] += r1 * D2; acc[k][9] += r2 * D2;
        }
    }
    const int wave = tid / 64, lane = tid % 64;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int i = 0; i < GSUMS; ++i) {
            const double v = wave_sum(acc[k][i]);
            if (lane == 0) red[wave][k * GSUMS + i] = v;
        }
    lse = wave_sum(lse);
    if (lane == 0) red[wave][GSUMS * K] = lse;
    __syncthreads();
    if (tid < GSUMS * K + 1) partial[(size_t)blockIdx.x * GPART + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// one wave.  start: the means the sums were taken about are init's, and the bound is not formed
__global__ __launch_bounds__(64) void admpc_quad_gmm_m_kernel(int nblk, int K, int d, int start, double tol, double reg, const double* __restrict__ init,
                                                              const double* __restrict__ partial, double* __restrict__ gmm, int32_t* __restrict__ info)
{
    if (!start && (info[1] | info[2])) return;
    __shared__ double sum[GPART];
    const int lane = (int)threadIdx.x, ne = GSUMS * K + 1;
    for (int e = lane; e < ne; e += 64) {
        // sixteen rows in flight: the wave waits for memory once per sixteen rows, not once per row
        double a[8] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        int r = 0;
        for (; r + 15 < nblk; r += 16) {
            double v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) v[q] = partial[(size_t)(r + q) * GPART + e];
#pragma unroll
            for (int q = 0; q < 16; ++q) a[q & 7] += v[q];
        }
        for (; r < nblk; ++r) a[0] += partial[(size_t)r * GPART + e];
        sum[e] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    __syncthreads();
    double n_valid;
    if (start) {                                  // hard responsibilities: the sums of r_k are whole numbers, and so is their sum
        n_valid = 0.0;
        for (int k = 0; k < K; ++k) n_valid += sum[k * GSUMS];
    }
    else n_valid = gmm[2];
    if (!(n_valid > 0.0)) {
        if (lane == 0) { info[0] = 0; info[1] = 0; info[2] = ADMPC_GMM_ENOVALID; info[3] = 0; }
        return;
    }
    const int k = lane < K ? lane : 0;
    const double* S = sum + k * GSUMS;
    const double N = S[0] + 10.0 * 2.220446049250313e-16, w = N / n_valid;
    const double s0 = S[1] / N, s1 = S[2] / N, s2 = S[3] / N;
    double m0, m1, m2;
    if (start) { m0 = init[k * d]; m1 = d > 1 ? init[k * d + 1] : 0.0; m2 = d > 2 ? init[k * d + 2] : 0.0; }
    else { const double* g = gmm + (1 + k) * GROW; m0 = g[1]; m1 = g[2]; m2 = g[3]; }
    m0 += s0; m1 += s1; m2 += s2;
    double c00 = S[4] / N - s0 * s0 + reg, c01 = S[5] / N - s0 * s1, c02 = S[6] / N - s0 * s2;
    double c11 = S[7] / N - s1 * s1 + reg, c12 = S[8] / N - s1 * s2, c22 = S[9] / N - s2 * s2 + reg;
    if (d < 2) { m1 = 0.0; c01 = 0.0; c11 = 1.0; c12 = 0.0; }       // a feature that is not there: the identity's row
    if (d < 3) { m2 = 0.0; c02 = 0.0; c12 = 0.0; c22 = 1.0; }
    // Sigma = L L', P = L^-T
    const double p0 = c00, l00 = sqrt(p0), l10 = c01 / l00, l20 = c02 / l00;
    const double p1 = c11 - l10 * l10, l11 = sqrt(p1), l21 = (c12 - l20 * l10) / l11;
    const double p2 = c22 - l20 * l20 - l21 * l21, l22 = sqrt(p2);
    const bool good = p0 > 0.0 && p1 > 0.0 && p2 > 0.0 && isfinite(p0) && isfinite(p1) && isfinite(p2);
    const double P00 = 1.0 / l00, P11 = 1.0 / l11, P22 = 1.0 / l22;
    const double P01 = -(l10 * P00) / l11, P12 = -(l21 * P11) / l22, P02 = -(l20 * P00 + l21 * P01) / l22;
    const unsigned long long failed = __ballot(lane < K && !good);
    if (failed) {                                 // the state stays as the iteration before left it
        if (lane == 0) {
            info[2] = -(__ffsll((long long)failed));
            if (start) { info[0] = 0; info[1] = 0; info[3] = (int32_t)n_valid; }
        }
        return;
    }
    double lb = -INFINITY, change = INFINITY;
    if (!start) { lb = sum[GSUMS * K] / n_valid; change = lb - gmm[0]; }
    if (lane < K) {
        double* g = gmm + (1 + k) * GROW;
        g[0] = w; g[1] = m0; g[2] = m1; g[3] = m2;
        g[4] = c00; g[5] = c01; g[6] = c02; g[7] = c11; g[8] = c12; g[9] = c22;
        g[10] = P00; g[11] = P01; g[12] = P02; g[13] = P11; g[14] = P12; g[15] = P22;
        g[16] = log(P00) + log(P11) + log(P22);
        g[17] = N;
    }
    if (lane == 0) {
        gmm[0] = lb; gmm[1] = change; gmm[2] = n_valid;
        for (int j = 3; j < GROW; ++j) gmm[j] = 0.0;
        info[0] = start ? 0 : info[0] + 1;
        info[1] = !start && fabs(change) < tol ? 1 : 0;
        info[2] = 0;
        info[3] = (int32_t)n_valid;
    }
}

__global__ __launch_bounds__(64) void admpc_quad_clusters_install_kernel(int K, int d, const double* __restrict__ gmm, const int32_t* __restrict__ info,
                                                                         double* __restrict__ cent, int32_t* __restrict__ perm, int32_t* __restrict__ installed)
{
    const int lane = (int)threadIdx.x, k = lane < K ? lane : 0;
    const double* g = gmm + (1 + k) * GROW + 1;
    const double m0 = g[0], m1 = d > 1 ? g[1] : 0.0, m2 = d > 2 ? g[2] : 0.0;
    const bool bad = !(isfinite(m0) && isfinite(m1) && isfinite(m2));
    if (info[2] != 0 || __ballot(lane < K && bad)) {
        if (lane < K) perm[lane] = lane;
        if (lane == 0) installed[0] = 0;
        return;
    }
    int rank = 0;
    for (int j = 0; j < K; ++j) {
        const double o = gmm[(1 + j) * GROW + 1];
        rank += (o < m0 || (o == m0 && j < k)) ? 1 : 0;
    }
    if (lane < K) {
        cent[rank * d] = m0;
        if (d > 1) cent[rank * d + 1] = m1;
        if (d > 2) cent[rank * d + 2] = m2;
        perm[rank] = lane;
    }
    if (lane == 0) installed[0] = 1;
}

__global__ __launch_bounds__(64) void admpc_quad_centroids_set_kernel(int n, const double* __restrict__ src, double* __restrict__ cent, int32_t* __restrict__ installed)
{
    const int lane = (int)threadIdx.x;
    const double v = lane < n ? src[lane] : 0.0;
    const bool any_bad = __ballot(!isfinite(v)) != 0;
    if (!any_bad && lane < n) cent[lane] = v;
    if (lane == 0) installed[0] = any_bad ? 0 : 1;
}

namespace {

int launched(const char* kernel)
{
    if (hipGetLastError() == hipSuccess) return ADMPC_OK;
    char msg[120];
    snprintf(msg, sizeof msg, "%s: launch failed", kernel);
    return admpc_set_error(ADMPC_EHIP, msg);
}

// the grid of the E kernel: a function of M alone
int gmm_blocks(long long M)
{
    const long long n = (M + GTHREADS - 1) / GTHREADS;
    return (int)(n < ADMPC_GMM_BLOCKS_MAX ? n : ADMPC_GMM_BLOCKS_MAX);
}

template <bool START>
void e_launch(int K, int nblk, long long M, int d, const double* packed, const double* init, const double* gmm, const int32_t* info, double* partial, hipStream_t st)
{
#define E_CASE(k) case k: hipLaunchKernelGGL((admpc_quad_gmm_e_kernel<k, START>), dim3(nblk), dim3(GTHREADS), 0, st, M, d, packed, init, gmm, info, partial); break;
    switch (K) { E_CASE(1) E_CASE(2) E_CASE(3) E_CASE(4) E_CASE(5) E_CASE(6) E_CASE(7) E_CASE(8) }
#undef E_CASE
}

}  // namespace

extern "C" {

int admpc_quad_ensemble_rollout_log_batch(AdmpcQuadEnsemble* e, const AdmpcQuadTrajBank* bank, const AdmpcQuadPlantParams* plant, int over,
                                          int B, int T, const int32_t* traj_of, int32_t* idx, double* x, double* xbar, double* ubar,
                                          double* yref, double* yref_e, double* cost, int32_t* status, int32_t* iters,
                                          double* tally, int32_t* counts, double* traj_out, double* u_out,
                                          int32_t* route, int32_t* route_out,
                                          const AdmpcQuadSolver* model, double* prev, double* samples, double* bins, int32_t* dropped,
                                          const AdmpcQuadNoiseParams* noise, uint64_t* noise_step, double* log, void* stream)
{
    const char* who = "admpc_quad_ensemble_rollout_batch";                  // the refusals it shares are under that entry's name
    (void)samples;
    if (!e) return admpc_refuse(who, "null ensemble");
    QuadEnsembleView v;
    admpc_quad_ensemble_view(e, &v);
    if (model && !v.learns) return admpc_refuse(who, "the ensemble was created without observe parameters");
    if (noise) {
        int rc = admpc_quad_plant_params_check("admpc_quad_rollout_noise_batch", plant);
        if (!rc) rc = admpc_quad_noise_params_check("admpc_quad_rollout_noise_batch", noise, plant);
        if (rc) return rc;
    }
    AdmpcQuadSolver* const* handles = nullptr;
    (void)admpc_quad_ensemble_handles(e, &handles);
    const QuadRolloutArgs a = { handles[0], bank, plant, over, B, traj_of, idx, x, xbar, ubar, yref, yref_e, cost, status, iters, tally, counts,
                                noise, noise ? noise_step : nullptr, e, route, route_out };
    if (!model) {
        const int rc = admpc_quad_rollout_check(a, T);
        return rc ? rc : admpc_refuse("admpc_quad_ensemble_rollout_log_batch", "null model: logging implies observing");
    }
    // the observed run's refusals with prev standing in for a log that is not there, which is refused behind them
    const int rc = admpc_quad_rollout_observe_check(a, T, model, v.obs, prev, log ? log : prev, bins, dropped);
    if (rc || B == 0 || T == 0) return rc;
    if (!log) return admpc_refuse("admpc_quad_ensemble_rollout_log_batch", "null log");
    return admpc_quad_rollout_observe_run(a, T, traj_out, u_out, model, v.obs, prev, log, (long long)B * QREC, bins, dropped, stream);
}

int admpc_quad_clusters_fit(const AdmpcQuadEnsemble* e, int max_iter, double tol, double reg_covar, int resume, int64_t M,
                            const double* records, const double* init, double* packed, double* partial, double* gmm, int32_t* info,
                            void* stream)
{
    const char* who = "admpc_quad_clusters_fit";
    if (!e) return admpc_refuse(who, "null ensemble");
    QuadEnsembleView v;
    admpc_quad_ensemble_view(e, &v);
    for (int j = 0; j < v.n_feat; ++j)
        if (v.feat[j] < FEAT_LO) return admpc_refuse(who, "the clustering features must lie in [7, 16]: the sample record holds no others");
    if (max_iter < 1 || max_iter > 1000) return admpc_refuse(who, "max_iter must be in [1, 1000]");
    if (!(tol >= 0.0)) return admpc_refuse(who, "tol must not be negative");
    if (!(reg_covar >= 0.0) || !isfinite(reg_covar)) return admpc_refuse(who, "reg_covar must be finite and not negative");
    if (resume != 0 && resume != 1) return admpc_refuse(who, "resume must be 0 or 1");
    if (M < 0) return admpc_refuse(who, "negative number of records");
    if (M == 0) return ADMPC_OK;
    if (!records || !packed || !partial || !gmm || !info) return admpc_refuse(who, "null array argument");
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    const int K = v.K, d = v.n_feat, nblk = gmm_blocks(M);
    const long long pblk = (M + GTHREADS - 1) / GTHREADS;
    hipLaunchKernelGGL(admpc_quad_gmm_pack_kernel, dim3((unsigned)(pblk < 65536 ? pblk : 65536)), dim3(GTHREADS), 0, st, (long long)M, d, v.feat[0], v.feat[1],
                       v.feat[2], records, packed);
    int rc = launched("admpc_quad_gmm_pack_kernel");
    if (!rc && !resume) {
        const double* from = init ? init : v.cent;
        e_launch<true>(K, nblk, M, d, packed, from, gmm, info, partial, st);
        rc = launched("admpc_quad_gmm_e_kernel");
        if (!rc) {
            hipLaunchKernelGGL(admpc_quad_gmm_m_kernel, dim3(1), dim3(64), 0, st, nblk, K, d, 1, tol, reg_covar, from, partial, gmm, info);
            rc = launched("admpc_quad_gmm_m_kernel");
        }
    }
    for (int it = 0; it < max_iter && !rc; ++it) {
        e_launch<false>(K, nblk, M, d, packed, nullptr, gmm, info, partial, st);
        rc = launched("admpc_quad_gmm_e_kernel");
        if (rc) break;
        hipLaunchKernelGGL(admpc_quad_gmm_m_kernel, dim3(1), dim3(64), 0, st, nblk, K, d, 0, tol, reg_covar, (const double*)nullptr, partial, gmm, info);
        rc = launched("admpc_quad_gmm_m_kernel");
    }
    return rc;
}

int admpc_quad_clusters_install(AdmpcQuadEnsemble* e, const double* gmm, const int32_t* info, int32_t* perm, int32_t* installed, void* stream)
{
    const char* who = "admpc_quad_clusters_install";
    if (!e) return admpc_refuse(who, "null ensemble");
    if (!gmm || !info || !perm || !installed) return admpc_refuse(who, "null array argument");
    QuadEnsembleView v;
    admpc_quad_ensemble_view(e, &v);
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_quad_clusters_install_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, v.K, v.n_feat, gmm, info, v.cent, perm, installed);
    return launched("admpc_quad_clusters_install_kernel");
}

int admpc_quad_ensemble_centroids_set(AdmpcQuadEnsemble* e, const double* centroids, int32_t* installed, void* stream)
{
    const char* who = "admpc_quad_ensemble_centroids_set";
    if (!e) return admpc_refuse(who, "null ensemble");
    if (!centroids || !installed) return admpc_refuse(who, "null array argument");
    QuadEnsembleView v;
    admpc_quad_ensemble_view(e, &v);
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_quad_centroids_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, v.K * v.n_feat, centroids, v.cent, installed);
    return launched("admpc_quad_centroids_set_kernel");
}

int admpc_quad_ensemble_centroids_get(const AdmpcQuadEnsemble* e, double* centroids, void* stream)
{
    const char* who = "admpc_quad_ensemble_centroids_get";
    if (!e) return admpc_refuse(who, "null ensemble");
    if (!centroids) return admpc_refuse(who, "null array argument");
    QuadEnsembleView v;
    admpc_quad_ensemble_view(e, &v);
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    if (hipMemcpyAsync(centroids, v.cent, (size_t)v.K * v.n_feat * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
        return admpc_set_error(ADMPC_EHIP, "admpc_quad_ensemble_centroids_get: the copy failed");
    return ADMPC_OK;
}

int admpc_quad_clusters_rebin(const AdmpcQuadEnsemble* e, int steps, int B, const double* log, double* bins, int32_t* dropped, void* stream)
{
    const char* who = "admpc_quad_clusters_rebin";
    if (!e) return admpc_refuse(who, "null ensemble");
    QuadEnsembleView v;
    admpc_quad_ensemble_view(e, &v);
    if (!v.learns) return admpc_refuse(who, "the ensemble was created without observe parameters");
    if (steps < 0 || B < 0) return admpc_refuse(who, "negative steps or batch");
    if (steps == 0 || B == 0) return ADMPC_OK;
    if (!log || !bins || !dropped) return admpc_refuse(who, "null array argument");
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    int rc = ADMPC_OK;
    for (int t = 0; t < steps && !rc; ++t) rc = admpc_quad_ensemble_bin_launch(e, B, log + (size_t)t * B * QREC, bins, dropped, stream);
    return rc;
}

}  // extern "C"
