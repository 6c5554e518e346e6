// admpc_quad_eval.hip -- the learned GPs of a clustered ensemble evaluated on a log of sample records (include/admpc_quad_eval.h).
//
//   factor    admpc_quad_eval_factor_kernel  grid K * n_gp, one wave each: the points, K, its Cholesky factor and alpha by the fit's own
//                                            text (gp_fit_dev.h: gp_points, gp_ymean, gp_chol, gp_alpha), then W = L^-1 by forward
//                                            substitution on the identity, lane j column j, and the packed block of the regressor
//   evaluate  admpc_quad_eval_kernel         256-thread blocks striding over the records, one lane per record: the route, then per
//                                            cluster that a record of the block routes to its three packed factors staged in LDS, the
//                                            kernel values of a record in registers, v = W k row by row from broadcast reads; eight sums
//                                            per (cluster, regressor) by wave shuffles into the wave's row in LDS; one row of partial per
//                                            block
//   zero      admpc_quad_eval_zero_kernel    one wave: info zeroed
//   finish    admpc_quad_eval_finish_kernel  one wave: lane l adds rows l, l + 64, ..., the wave the lanes by the shuffle tree; the status
//
// No floating-point atomics; the two skip counts are integer atomics, one per block and count.  The regressors, the centroids and the
// search's hyper are read by pointer from the object's device copies, as admpc_quad_hyper.hip's kernels read them.
#include <stdio.h>
#include <math.h>
#include "admpc_host.h"
#include "../../include/admpc_quad_eval.h"

#define NX ADMPC_NX           // model_dev.h (exp_nonpos, which the bodies of gp_fit_dev.h name) wants the car's dimensions defined
#define NU ADMPC_NU
#define NY ADMPC_NY
#include "gp_search_dev.h"    // WAVE, NPT, ACC, HYP; LearnGp, LearnArgs, GpHyper; gp_points, gp_ymean, gp_chol, gp_alpha, gp_hyper_natural
#define QREC 14               // doubles per sample record, as admpc_quad_learn.hip lays it out
#define KMAX ADMPC_QUAD_CLUSTERS_MAX
#define GMAX ADMPC_QUAD_GP_MAX
#define FACT ADMPC_EVAL_FACTOR
#define NST ADMPC_EVAL_STATS
#define ETHREADS 256
#define EWAVES (ETHREADS / WAVE)
#define F_Z 16                // the offsets of a factor block (include/admpc_quad_eval.h: THE FACTOR)
#define F_ALPHA (F_Z + 3 * NPT)
#define F_W (F_ALPHA + NPT)

static_assert(F_W + NPT * (NPT + 1) / 2 == FACT, "header, Z, alpha and the packed W fill a factor block");
static_assert(GMAX == 3 && NST == 8, "include/admpc_quad_eval.h lays stats out as [K][3][8]");

struct EvalFactorArgs {
    int n_gp;
    double min_count;
    const LearnGp* gp;                        // [K][GMAX], the object's
    const double* bins;                       // [K][GMAX][NPT][ACC]
    const double* hyper;                      // null, or [K][GMAX][HYP]
    double* factor;                           // [K][GMAX][FACT]
    int32_t* info;                            // [K][GMAX]
};

struct EvalArgs {
    long long M;
    int K, n_gp, d, f[3], take_pruned;
    const double* cent;                       // [K][d], the object's
    const double* rec;                        // [M][QREC]
    const double* factor;                     // [K][GMAX][FACT]
    const double* drag;                       // null, or [3]
    double* per_record;                       // null, or [M][GMAX][2]
    double* partial;                          // [ADMPC_GMM_BLOCKS_MAX][K * GMAX * NST]
    int32_t* info;                            // [4]
};

namespace {

#include "model_dev.h"

constexpr int QU = ADMPC_QUAD_NU, QY = ADMPC_QUAD_NY;
typedef AdmpcQuadConfig Cfg;

#include "quad_model_dev.h"
#include "quad_route_dev.h"

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int wave_sum_int(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int held(const double v, const int lo, const int hi)
{
    const int i = (int)v;
    return i < lo ? lo : (i > hi ? hi : i);
}

}  // namespace

// grid K * n_gp: block y is regressor (y / n_gp, y % n_gp), at the flat index c * 3 + g of every array
__global__ __launch_bounds__(WAVE) void admpc_quad_eval_factor_kernel(const EvalFactorArgs a)
{
    __shared__ double Zs[3][NPT], ts[NPT], cs[NPT], As[NPT][NPT + 1], Ws[NPT][NPT + 1];
    const int i = ((int)blockIdx.x / a.n_gp) * GMAX + (int)blockIdx.x % a.n_gp;
    // the bodies see ONE regressor at the constant index 0, as admpc_quad_hyper.hip hands it to them
    LearnArgs l;
    l.B = 0; l.n_gp = 1;
    l.min_count = a.min_count;
    l.gp[0] = a.gp[i];
    l.samples = nullptr; l.dropped = nullptr; l.out = nullptr; l.info = nullptr;
    l.bins = const_cast<double*>(a.bins) + (long)i * NPT * ACC;       // read only
    const LearnGp& G = l.gp[0];
    const int nf = G.n_feat;
    GpHyper h = { G.sigma_f, { G.inv_l2[0], G.inv_l2[1], G.inv_l2[2] }, G.noise, 0 };
    if (a.hyper) h = gp_hyper_natural(nf, a.hyper + (long)i * HYP);
    const int lane = gp_lane_id(), r = lane & (NPT - 1);
    const bool act = lane < NPT;
    const int n = gp_points(l, 0, lane, Zs, ts, cs);
    __syncthreads();
    const double ymean = gp_ymean(ts, n);
    const int fail = gp_chol(G, h, n, lane, Zs, ts, cs, As);
    const double bb = gp_alpha(fail, n, lane, ts, ymean, As);
    const int np = fail ? 0 : n;
    // W = L^-1: L W = I by forward substitution, a row per step; lane j owns column j and reads back only what it wrote
#pragma unroll 1
    for (int row = 0; row < np; ++row) {
        if (act && r <= row) {
            double s = r == row ? 1.0 : 0.0;
#pragma unroll 1
            for (int k = r; k < row; ++k) s = s - As[row][k] * Ws[k][r];
            Ws[row][r] = s / As[row][row];
        }
    }
    __syncthreads();
    double* f = a.factor + (long)i * FACT;
    if (lane == 0) {
        f[0] = (double)np; f[1] = (double)nf;
#pragma unroll
        for (int d = 0; d < 3; ++d) { f[2 + d] = d < nf ? (double)G.feat[d] : 0.0; f[7 + d] = d < nf ? h.inv_l2[d] : 0.0; }
        f[5] = (double)G.out; f[6] = h.sigma_f;
        f[10] = fail ? 0.0 : ymean;
#pragma unroll
        for (int d = 11; d < F_Z; ++d) f[d] = 0.0;
    }
    if (act) {
#pragma unroll
        for (int d = 0; d < 3; ++d) f[F_Z + d * NPT + r] = (r < np && d < nf) ? Zs[d][r] : 0.0;
        f[F_ALPHA + r] = r < np ? bb : 0.0;
#pragma unroll 1
        for (int row = r; row < NPT; ++row) f[F_W + row * (row + 1) / 2 + r] = row < np ? Ws[row][r] : 0.0;
    }
    if (lane == 0) a.info[i] = fail ? -fail : n;
}

// one wave: info zeroed in front of the integer atomics of the evaluate kernel (a kernel, not a memset node: the same in a captured graph)
__global__ __launch_bounds__(WAVE) void admpc_quad_eval_zero_kernel(int32_t* __restrict__ info)
{
    if (threadIdx.x < 4) info[threadIdx.x] = 0;
}

// grid: a function of M alone (eval_blocks below)
__global__ __launch_bounds__(ETHREADS) void admpc_quad_eval_kernel(const EvalArgs a)
{
    __shared__ double fac[GMAX][FACT];
    __shared__ double acc[EWAVES][KMAX * GMAX * NST];
    __shared__ int skip[EWAVES][2];
    const int tid = (int)threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const int width = a.K * GMAX * NST;
    for (int k = tid; k < EWAVES * KMAX * GMAX * NST; k += ETHREADS) (&acc[0][0])[k] = 0.0;
    int by_flag = 0, not_finite = 0;
    const double nan = __builtin_nan("");
    for (long long base = (long long)blockIdx.x * ETHREADS; base < a.M; base += (long long)gridDim.x * ETHREADS) {
        const long long i = base + tid;
        const double* __restrict__ r = a.rec + (i < a.M ? i : 0) * QREC;
        int mine = -1;
        if (i < a.M) {
            const double flag = r[QREC - 1];
            if (!(flag == 1.0 || (a.take_pruned && flag == ADMPC_QUAD_REC_PRUNED))) by_flag += 1;
            else {
                bool fin = true;
#pragma unroll
                for (int j = 0; j < QREC - 1; ++j) fin = fin && isfinite(r[j]);
                if (!fin) not_finite += 1;
                else {
                    const double z[3] = { r[a.f[0] - 7], a.d > 1 ? r[a.f[1] - 7] : 0.0, a.d > 2 ? r[a.f[2] - 7] : 0.0 };
                    mine = quad_nearest(z, a.d, a.K, a.cent);
                }
            }
            if (mine < 0 && a.per_record)
                for (int g = 0; g < a.n_gp; ++g) { a.per_record[(i * GMAX + g) * 2] = nan; a.per_record[(i * GMAX + g) * 2 + 1] = nan; }
        }
#pragma unroll 1
        for (int c = 0; c < a.K; ++c) {
            // the barrier also closes the reads of the factors staged before; uniform over the block
            if (!__syncthreads_or(mine == c)) continue;
            for (int g = 0; g < a.n_gp; ++g) {
                const double* __restrict__ src = a.factor + (long)(c * GMAX + g) * FACT;
                const int n = held(src[0], 0, NPT), cnt = F_W + n * (n + 1) / 2;
                for (int k = tid; k < cnt; k += ETHREADS) fac[g][k] = src[k];
            }
            __syncthreads();
            const bool on = mine == c;
            if (__ballot(on) == 0ull) continue;                    // uniform over the wave; no barrier below
#pragma unroll 1
            for (int g = 0; g < a.n_gp; ++g) {
                const double* F = fac[g];
                double st[NST] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
                if (on) {
                    const int n = held(F[0], 0, NPT), nf = held(F[1], 0, 3), out = held(F[5], 7, 9) - 7;
                    const double sigma_f = F[6], il0 = nf > 0 ? F[7] : 0.0, il1 = nf > 1 ? F[8] : 0.0, il2 = nf > 2 ? F[9] : 0.0;
                    const double z0 = nf > 0 ? r[held(F[2], 7, 16) - 7] : 0.0, z1 = nf > 1 ? r[held(F[3], 7, 16) - 7] : 0.0,
                                 z2 = nf > 2 ? r[held(F[4], 7, 16) - 7] : 0.0;
                    double k[NPT], mu = F[10];
#pragma unroll
                    for (int p = 0; p < NPT; ++p) {
                        k[p] = 0.0;
                        if (p < n) {                                  // uniform: n is the cluster's
                            const double e0 = z0 - F[F_Z + p], e1 = z1 - F[F_Z + NPT + p], e2 = z2 - F[F_Z + 2 * NPT + p];
                            k[p] = sigma_f * exp_nonpos(-0.5 * (e0 * e0 * il0 + e1 * e1 * il1 + e2 * e2 * il2));
                            mu += k[p] * F[F_ALPHA + p];
                        }
                    }
                    double q = 0.0;
#pragma unroll
                    for (int p = 0; p < NPT; ++p) {
                        if (p < n) {
                            const double* w = F + F_W + p * (p + 1) / 2;
                            double v = 0.0;
#pragma unroll
                            for (int j = 0; j <= p; ++j) v += w[j] * k[j];
                            q += v * v;
                        }
                    }
                    const double var = (sigma_f + 1e-8) - q;
                    const double sd = var > 0.0 ? sqrt(var) : 0.0;
                    const double y = r[10 + out];
                    const double dterm = a.drag ? a.drag[out] * r[out] : 0.0;
                    const double m = mu + dterm, res = y - m;
                    if (a.per_record) { a.per_record[(i * GMAX + g) * 2] = m; a.per_record[(i * GMAX + g) * 2 + 1] = sd; }
                    st[0] = 1.0; st[1] = fabs(y); st[2] = y * y; st[3] = fabs(res); st[4] = res * res; st[5] = sd;
                    st[6] = fabs(res) <= 3.0 * sd ? 1.0 : 0.0;
                    st[7] = var < 0.0 ? 1.0 : 0.0;
                }
                double* o = acc[wave] + (c * GMAX + g) * NST;
#pragma unroll
                for (int s = 0; s < NST; ++s) {
                    const double v = wave_sum(st[s]);
                    if (lane == 0) o[s] = o[s] + v;
                }
            }
        }
    }
    by_flag = wave_sum_int(by_flag); not_finite = wave_sum_int(not_finite);
    if (lane == 0) { skip[wave][0] = by_flag; skip[wave][1] = not_finite; }
    __syncthreads();
    for (int k = tid; k < width; k += ETHREADS) a.partial[(size_t)blockIdx.x * width + k] = ((acc[0][k] + acc[1][k]) + acc[2][k]) + acc[3][k];
    if (tid < 2) {
        const int v = (skip[0][tid] + skip[1][tid]) + (skip[2][tid] + skip[3][tid]);
        if (v) atomicAdd(&a.info[2 + tid], v);
    }
}

// one wave: per (cluster, regressor) lane l adds rows l, l + 64, ... in order, the wave the lanes by the shuffle tree: a fixed order; the
// records that took part are the n of regressor 0.  (A lane per column that walked all rows took 58 to 176 us: 256 dependent loads.)
__global__ __launch_bounds__(WAVE) void admpc_quad_eval_finish_kernel(int nblk, int K, const double* __restrict__ partial, double* __restrict__ stats,
                                                                      int32_t* __restrict__ info)
{
    const int lane = (int)threadIdx.x, width = K * GMAX * NST;
    double took = 0.0;
#pragma unroll 1
    for (int grp = 0; grp < K * GMAX; ++grp) {
        double a[NST] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        for (int r = lane; r < nblk; r += WAVE) {
            const double* __restrict__ p = partial + (size_t)r * width + grp * NST;
#pragma unroll
            for (int s = 0; s < NST; ++s) a[s] += p[s];
        }
#pragma unroll
        for (int s = 0; s < NST; ++s) {
            const double v = wave_sum(a[s]);
            if (lane == 0) stats[grp * NST + s] = v;
            if (s == 0 && grp % GMAX == 0) took += v;     // whole numbers below 2^31: exact
        }
    }
    if (lane == 0) { info[0] = took > 0.0 ? 0 : ADMPC_EVAL_ENOVALID; info[1] = (int32_t)took; }
}

namespace {

int launched(const char* kernel)
{
    if (hipGetLastError() == hipSuccess) return ADMPC_OK;
    char msg[120];
    snprintf(msg, sizeof msg, "%s: launch failed", kernel);
    return admpc_set_error(ADMPC_EHIP, msg);
}

// the grid of the kernel over the records: a function of M alone, as admpc_quad_prune.hip's
int eval_blocks(long long M)
{
    const long long n = (M + ETHREADS - 1) / ETHREADS;
    return (int)(n < ADMPC_GMM_BLOCKS_MAX ? n : ADMPC_GMM_BLOCKS_MAX);
}

}  // namespace

extern "C" {

int admpc_quad_ensemble_factor(const AdmpcQuadEnsemble* e, int min_count, const double* bins, const double* hyper, double* factor,
                               int32_t* info, void* stream)
{
    const char* who = "admpc_quad_ensemble_factor";
    if (!e) return admpc_refuse(who, "null ensemble");
    QuadEnsembleView v;
    admpc_quad_ensemble_view(e, &v);
    if (!v.learns) return admpc_refuse(who, "the ensemble was created without observe parameters");
    if (min_count < 1) return admpc_refuse(who, "min_count must be at least 1");
    if (!bins || !factor || !info) return admpc_refuse(who, "null array argument");
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    EvalFactorArgs a = EvalFactorArgs();
    a.n_gp = v.n_gp; a.min_count = (double)min_count; a.gp = v.gp; a.bins = bins; a.hyper = hyper; a.factor = factor; a.info = info;
    hipLaunchKernelGGL(admpc_quad_eval_factor_kernel, dim3((unsigned)(v.K * v.n_gp)), dim3(WAVE), 0, (hipStream_t)stream, a);
    return launched("admpc_quad_eval_factor_kernel");
}

int admpc_quad_ensemble_evaluate(const AdmpcQuadEnsemble* e, int64_t M, const double* records, int take_pruned, const double* factor,
                                 const double* drag, double* per_record, double* partial, double* stats, int32_t* info, void* stream)
{
    const char* who = "admpc_quad_ensemble_evaluate";
    if (!e) return admpc_refuse(who, "null ensemble");
    QuadEnsembleView v;
    admpc_quad_ensemble_view(e, &v);
    for (int j = 0; j < v.n_feat; ++j)
        if (v.feat[j] < 7 || v.feat[j] >= QY) return admpc_refuse(who, "the clustering features must lie in [7, 16]: the sample record holds no others");
    if (M < 0 || M > INT32_MAX) return admpc_refuse(who, "the number of records must be in [0, INT32_MAX]");
    if (take_pruned != 0 && take_pruned != 1) return admpc_refuse(who, "take_pruned must be 0 or 1");
    if (M == 0) return ADMPC_OK;
    if (!records || !factor || !partial || !stats || !info) return admpc_refuse(who, "null array argument");
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    EvalArgs a = EvalArgs();
    a.M = (long long)M; a.K = v.K; a.n_gp = v.learns ? v.n_gp : 0; a.d = v.n_feat; a.take_pruned = take_pruned;
    for (int j = 0; j < 3; ++j) a.f[j] = j < v.n_feat ? v.feat[j] : 7;
    a.cent = v.cent; a.rec = records; a.factor = factor; a.drag = drag; a.per_record = per_record; a.partial = partial; a.info = info;
    hipLaunchKernelGGL(admpc_quad_eval_zero_kernel, dim3(1), dim3(WAVE), 0, st, info);
    int rc = launched("admpc_quad_eval_zero_kernel");
    if (rc) return rc;
    const int nblk = eval_blocks(M);
    hipLaunchKernelGGL(admpc_quad_eval_kernel, dim3(nblk), dim3(ETHREADS), 0, st, a);
    rc = launched("admpc_quad_eval_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(admpc_quad_eval_finish_kernel, dim3(1), dim3(WAVE), 0, st, nblk, v.K, (const double*)partial, stats, info);
    return launched("admpc_quad_eval_finish_kernel");
}

}  // extern "C"
