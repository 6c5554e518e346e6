// admpc_quad_prune.hip -- the pruning of a log of sample records and the RDRv drag fit on the device (include/admpc_quad_prune.h).
//
//   range    admpc_quad_prune_range_kernel   256-thread blocks striding over the records: min / max of the four columns and the count of
//                                            the records that take part, by wave shuffles and across the four waves through LDS: one row
//                                            of partial per block
//   edges    admpc_quad_prune_edges_kernel   one wave: lane l reduces rows l, l + 64, ..., the wave the lanes; np.linspace's edges, lane l
//                                            edge l, l + 64, ...; counts and the tallies zeroed, the status and n_valid set
//   count    admpc_quad_prune_count_kernel   edges and four int histograms in LDS, LDS integer atomics per record, then one global integer
//                                            atomic per bin that is not empty
//   mark     admpc_quad_prune_mark_kernel    edges and sparse flags in LDS; entry 13 of every record that takes part, written where it
//                                            changes; six tallies per thread in registers, reduced by wave shuffles and across the four
//                                            waves through LDS, one global integer atomic per block and tally
//   fit      admpc_quad_rdrv_sums_kernel, admpc_quad_rdrv_finish_kernel   the six sums and the count per block; one wave adds the rows
//   install  admpc_quad_rdrv_install_kernel  one wave: three doubles into rdrv of a handle's device configuration, unless one is not finite
//
// Everything the rule rounds (the norm, the edges, the bin index) is written without contraction: it has to give numpy's bits.  No
// floating-point atomics.  range / count / mark share prune_take and prune_bin, so that the three agree on who takes part and where.
#include <stdio.h>
#include <math.h>
#include "admpc_host.h"
#include "../../include/admpc_quad_prune.h"

#define QREC 14               // doubles per sample record, as admpc_quad_learn.hip lays it out
#define PBINS ADMPC_PRUNE_BINS_MAX
#define PPART ADMPC_PRUNE_PARTIAL
#define RPART ADMPC_RDRV_PARTIAL
#define PTHREADS 256

namespace {

// Does the record take part, and with which columns?  c [4]: y_0 .. y_2 and the norm; capped: |v_b,i| > x_cap for some i.
__device__ __forceinline__ bool prune_take(const double* __restrict__ r, double x_cap, double c[4], bool& capped)
{
#pragma clang fp contract(off)
    const double flag = r[QREC - 1];
    const double v0 = r[0], v1 = r[1], v2 = r[2], y0 = r[10], y1 = r[11], y2 = r[12];
    const bool ok = (flag == 1.0 || flag == ADMPC_QUAD_REC_PRUNED) && isfinite(v0) && isfinite(v1) && isfinite(v2) && isfinite(y0) && isfinite(y1) &&
                    isfinite(y2);
    c[0] = y0; c[1] = y1; c[2] = y2;
    const double s01 = y0 * y0 + y1 * y1;
    c[3] = __dsqrt_rn(s01 + y2 * y2);
    capped = fabs(v0) > x_cap || fabs(v1) > x_cap || fabs(v2) > x_cap;
    return ok;
}

// np.histogram's uniform-bin index of v among e_0 .. e_n (e in LDS), held into 0 .. n - 1
__device__ __forceinline__ int prune_bin(double v, const double* e, int n)
{
#pragma clang fp contract(off)
    const double lo = e[0], hi = e[n];
    const double f = ((v - lo) / (hi - lo)) * (double)n;
    int idx = f >= 0.0 ? (f >= (double)n ? n : (int)f) : 0;
    if (idx == n) idx = n - 1;
    if (v < e[idx]) idx -= 1;
    idx = idx < 0 ? 0 : idx;
    if (v >= e[idx + 1] && idx != n - 1) idx += 1;
    return idx;
}

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

}  // namespace

// grid: a function of M alone (prune_blocks below)
__global__ __launch_bounds__(PTHREADS) void admpc_quad_prune_range_kernel(long long M, const double* __restrict__ rec, double* __restrict__ partial)
{
    __shared__ double red[PTHREADS / 64][PPART];
    const int tid = (int)threadIdx.x, wave = tid / 64, lane = tid % 64;
    double mn[4] = { INFINITY, INFINITY, INFINITY, INFINITY }, mx[4] = { -INFINITY, -INFINITY, -INFINITY, -INFINITY };
    int n = 0;
    for (long long i = (long long)blockIdx.x * PTHREADS + tid; i < M; i += (long long)gridDim.x * PTHREADS) {
        double c[4];
        bool capped;
        if (!prune_take(rec + i * QREC, INFINITY, c, capped)) continue;
        n += 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) { mn[j] = c[j] < mn[j] ? c[j] : mn[j]; mx[j] = c[j] > mx[j] ? c[j] : mx[j]; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double a = __shfl_xor(mn[j], o), b = __shfl_xor(mx[j], o);
            mn[j] = a < mn[j] ? a : mn[j]; mx[j] = b > mx[j] ? b : mx[j];
        }
        if (lane == 0) { red[wave][2 * j] = mn[j]; red[wave][2 * j + 1] = mx[j]; }
    }
    n = wave_sum_int(n);
    if (lane == 0) red[wave][8] = (double)n;
    __syncthreads();
    if (tid < PPART) {
        double v = red[0][tid];
        for (int w = 1; w < PTHREADS / 64; ++w) {
            const double o = red[w][tid];
            v = tid == 8 ? v + o : (tid & 1) ? (o > v ? o : v) : (o < v ? o : v);          // counts below 2^31: exact
        }
        partial[(size_t)blockIdx.x * PPART + tid] = v;
    }
}

// one wave
__global__ __launch_bounds__(64) void admpc_quad_prune_edges_kernel(int nblk, int n_bins, const double* __restrict__ partial, double* __restrict__ edges,
                                                                    int32_t* __restrict__ counts, int32_t* __restrict__ info)
{
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x;
    double mn[4] = { INFINITY, INFINITY, INFINITY, INFINITY }, mx[4] = { -INFINITY, -INFINITY, -INFINITY, -INFINITY }, n = 0.0;
    for (int r = lane; r < nblk; r += 64) {
        const double* p = partial + (size_t)r * PPART;
#pragma unroll
        for (int j = 0; j < 4; ++j) { mn[j] = p[2 * j] < mn[j] ? p[2 * j] : mn[j]; mx[j] = p[2 * j + 1] > mx[j] ? p[2 * j + 1] : mx[j]; }
        n += p[8];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double a = __shfl_xor(mn[j], o), b = __shfl_xor(mx[j], o);
            mn[j] = a < mn[j] ? a : mn[j]; mx[j] = b > mx[j] ? b : mx[j];
        }
    n = wave_sum(n);                                  // whole numbers below 2^31: exact in any order
    for (int i = lane; i < 4 * PBINS; i += 64) counts[i] = 0;
    if (lane >= 2 && lane < 8) info[lane] = 0;
    if (lane == 0) { info[0] = n > 0.0 ? 0 : ADMPC_PRUNE_ENOVALID; info[1] = (int32_t)n; }
    if (!(n > 0.0)) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double lo = mn[j], hi = mx[j];
        if (lo == hi) { lo = lo - 0.5; hi = hi + 0.5; }
        const double step = (hi - lo) / (double)n_bins;
        double* e = edges + j * (PBINS + 1);
        for (int k = lane; k < n_bins; k += 64) {
            const double ks = (double)k * step;
            e[k] = ks + lo;
        }
        if (lane == 0) e[n_bins] = hi;
    }
}

// grid: a function of M alone
__global__ __launch_bounds__(PTHREADS) void admpc_quad_prune_count_kernel(long long M, int n_bins, const double* __restrict__ rec, const double* __restrict__ edges,
                                                                          const int32_t* __restrict__ info, int32_t* __restrict__ counts)
{
    __shared__ double e[4][PBINS + 1];
    __shared__ int hist[4][PBINS];
    if (info[0] != 0) return;
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < 4 * (n_bins + 1); i += PTHREADS) { const int j = i / (n_bins + 1), k = i % (n_bins + 1); e[j][k] = edges[j * (PBINS + 1) + k]; }
    for (int i = tid; i < 4 * PBINS; i += PTHREADS) hist[i / PBINS][i % PBINS] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * PTHREADS + tid; i < M; i += (long long)gridDim.x * PTHREADS) {
        double c[4];
        bool capped;
        if (!prune_take(rec + i * QREC, INFINITY, c, capped)) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(&hist[j][prune_bin(c[j], e[j], n_bins)], 1);
    }
    __syncthreads();
    for (int i = tid; i < 4 * n_bins; i += PTHREADS) {
        const int j = i / n_bins, k = i % n_bins, h = hist[j][k];
        if (h) atomicAdd(&counts[j * PBINS + k], h);
    }
}

// grid: a function of M alone
__global__ __launch_bounds__(PTHREADS) void admpc_quad_prune_mark_kernel(long long M, int n_bins, double x_cap, double thresh, double* __restrict__ rec,
                                                                         const double* __restrict__ edges, const int32_t* __restrict__ counts,
                                                                         int32_t* __restrict__ info)
{
    __shared__ double e[4][PBINS + 1];
    __shared__ int sparse[4][PBINS];
    __shared__ int tally[PTHREADS / 64][6];
    if (info[0] != 0) return;
    const int tid = (int)threadIdx.x;
    const double n_valid = (double)info[1];
    for (int i = tid; i < 4 * (n_bins + 1); i += PTHREADS) { const int j = i / (n_bins + 1), k = i % (n_bins + 1); e[j][k] = edges[j * (PBINS + 1) + k]; }
    for (int i = tid; i < 4 * n_bins; i += PTHREADS) {
        const int j = i / n_bins, k = i % n_bins;
        sparse[j][k] = (double)counts[j * PBINS + k] / n_valid < thresh ? 1 : 0;
    }
    __syncthreads();
    int t[6] = { 0, 0, 0, 0, 0, 0 };                    // kept, cap, axis 0 .. 2, norm
    for (long long i = (long long)blockIdx.x * PTHREADS + tid; i < M; i += (long long)gridDim.x * PTHREADS) {
        double c[4];
        bool capped;
        double* r = rec + i * QREC;
        if (!prune_take(r, x_cap, c, capped)) continue;
        bool out = capped;
        t[1] += capped ? 1 : 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = prune_bin(c[j], e[j], n_bins);
            const bool hit = sparse[j][idx] || (idx > 0 && c[j] == e[j][idx] && sparse[j][idx - 1]);
            t[2 + j] += hit ? 1 : 0;
            out = out || hit;
        }
        t[0] += out ? 0 : 1;
        const double flag = out ? ADMPC_QUAD_REC_PRUNED : 1.0;
        if (r[QREC - 1] != flag) r[QREC - 1] = flag;            // most records keep the flag they came with: 1.5 us of 55 at M = 245 760
    }
    // one atomic per block and tally: one per WAVE and tally, 6144 on six neighbouring words, cost 14 us of 55 at M = 245 760
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int v = wave_sum_int(t[j]);
        if (tid % 64 == 0) tally[tid / 64][j] = v;
    }
    __syncthreads();
    if (tid < 6) {
        const int v = (tally[0][tid] + tally[1][tid]) + (tally[2][tid] + tally[3][tid]);
        if (v) atomicAdd(&info[2 + tid], v);
    }
}

// grid: a function of M alone.  A row of partial: S_xy and S_xx of the three axes, the count
__global__ __launch_bounds__(PTHREADS) void admpc_quad_rdrv_sums_kernel(long long M, const double* __restrict__ rec, double* __restrict__ partial)
{
    __shared__ double red[PTHREADS / 64][RPART];
    const int tid = (int)threadIdx.x, wave = tid / 64, lane = tid % 64;
    double s[RPART] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (long long i = (long long)blockIdx.x * PTHREADS + tid; i < M; i += (long long)gridDim.x * PTHREADS) {
        const double* r = rec + i * QREC;
        if (r[QREC - 1] != 1.0) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j) { const double v = r[j], y = r[10 + j]; s[2 * j] += v * y; s[2 * j + 1] += v * v; }
        s[6] += 1.0;
    }
#pragma unroll
    for (int j = 0; j < RPART; ++j) {
        const double v = wave_sum(s[j]);
        if (lane == 0) red[wave][j] = v;
    }
    __syncthreads();
    if (tid < RPART) partial[(size_t)blockIdx.x * RPART + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// one wave: lane l adds rows l, l + 64, ... in order, the wave the lanes by the shuffle tree: a fixed order
__global__ __launch_bounds__(64) void admpc_quad_rdrv_finish_kernel(int nblk, int axes, const double* __restrict__ partial, double* __restrict__ d_out,
                                                                    double* __restrict__ sums, int32_t* __restrict__ info)
{
    const int lane = (int)threadIdx.x;
    double s[RPART];
#pragma unroll
    for (int j = 0; j < RPART; ++j) {
        double a = 0.0;
        for (int r = lane; r < nblk; r += 64) a += partial[(size_t)r * RPART + j];
        s[j] = wave_sum(a);
    }
    if (lane != 0) return;
    int status = 0;
    for (int i = 2; i >= 0; --i) {
        const bool asked = (axes >> i) & 1;
        const double xy = asked ? s[2 * i] : 0.0, xx = asked ? s[2 * i + 1] : 0.0;
        const double d = asked ? xy / xx : 0.0;
        if (asked && !(xx > 0.0 && isfinite(xx) && isfinite(d))) status = -(i + 1);
        d_out[i] = d; sums[2 * i] = xy; sums[2 * i + 1] = xx;
    }
    info[0] = (int32_t)s[6]; info[1] = status;
}

__global__ __launch_bounds__(64) void admpc_quad_rdrv_install_kernel(AdmpcQuadConfig* cfg, const double* __restrict__ d, const int32_t* __restrict__ info,
                                                                     int32_t* __restrict__ installed)
{
    const int lane = (int)threadIdx.x;
    const double v = lane < 3 ? d[lane] : 0.0;
    const bool declined = info[1] != 0 || __ballot(!isfinite(v)) != 0;
    if (!declined && lane < 3) cfg->rdrv[lane] = v;
    if (lane == 0) installed[0] = declined ? 0 : 1;
}

namespace {

int launched(const char* kernel)
{
    if (hipGetLastError() == hipSuccess) return ADMPC_OK;
    char msg[120];
    snprintf(msg, sizeof msg, "%s: launch failed", kernel);
    return admpc_set_error(ADMPC_EHIP, msg);
}

// the grid of every kernel over the records: a function of M alone, the E kernel's of admpc_quad_clusters.hip
int prune_blocks(long long M)
{
    const long long n = (M + PTHREADS - 1) / PTHREADS;
    return (int)(n < ADMPC_GMM_BLOCKS_MAX ? n : ADMPC_GMM_BLOCKS_MAX);
}

}  // namespace

extern "C" {

int admpc_quad_records_prune(int device, int64_t M, double* records, double x_cap, int n_bins, double thresh, double* partial,
                             double* edges, int32_t* counts, int32_t* info, void* stream)
{
    const char* who = "admpc_quad_records_prune";
    if (M < 0 || M > INT32_MAX) return admpc_refuse(who, "the number of records must be in [0, INT32_MAX]");
    if (n_bins < 1 || n_bins > PBINS) return admpc_refuse(who, "n_bins must be in [1, 256]");
    if (!(thresh >= 0.0 && thresh <= 1.0)) return admpc_refuse(who, "thresh must be in [0, 1]");
    if (!(x_cap > 0.0)) return admpc_refuse(who, "x_cap must be positive (+inf: no cap)");
    if (M == 0) return ADMPC_OK;
    if (!records || !partial || !edges || !counts || !info) return admpc_refuse(who, "null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = prune_blocks(M);
    hipLaunchKernelGGL(admpc_quad_prune_range_kernel, dim3(nblk), dim3(PTHREADS), 0, st, (long long)M, (const double*)records, partial);
    int rc = launched("admpc_quad_prune_range_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(admpc_quad_prune_edges_kernel, dim3(1), dim3(64), 0, st, nblk, n_bins, (const double*)partial, edges, counts, info);
    rc = launched("admpc_quad_prune_edges_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(admpc_quad_prune_count_kernel, dim3(nblk), dim3(PTHREADS), 0, st, (long long)M, n_bins, (const double*)records, (const double*)edges,
                       (const int32_t*)info, counts);
    rc = launched("admpc_quad_prune_count_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(admpc_quad_prune_mark_kernel, dim3(nblk), dim3(PTHREADS), 0, st, (long long)M, n_bins, x_cap, thresh, records, (const double*)edges,
                       (const int32_t*)counts, info);
    return launched("admpc_quad_prune_mark_kernel");
}

int admpc_quad_rdrv_fit(int device, int64_t M, int axes, const double* records, double* partial, double* d_out, double* sums,
                        int32_t* info, void* stream)
{
    const char* who = "admpc_quad_rdrv_fit";
    if (M < 0 || M > INT32_MAX) return admpc_refuse(who, "the number of records must be in [0, INT32_MAX]");
    if (axes < 1 || axes > 7) return admpc_refuse(who, "axes must be a mask in [1, 7]");
    if (M == 0) return ADMPC_OK;
    if (!records || !partial || !d_out || !sums || !info) return admpc_refuse(who, "null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = prune_blocks(M);
    hipLaunchKernelGGL(admpc_quad_rdrv_sums_kernel, dim3(nblk), dim3(PTHREADS), 0, st, (long long)M, records, partial);
    int rc = launched("admpc_quad_rdrv_sums_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(admpc_quad_rdrv_finish_kernel, dim3(1), dim3(64), 0, st, nblk, axes, (const double*)partial, d_out, sums, info);
    return launched("admpc_quad_rdrv_finish_kernel");
}

int admpc_quad_rdrv_install(AdmpcQuadSolver* s, const double* d_dev, const int32_t* info, int32_t* installed, void* stream)
{
    const char* who = "admpc_quad_rdrv_install";
    if (!s) return admpc_refuse(who, "null solver");
    if (!d_dev || !info || !installed) return admpc_refuse(who, "null array argument");
    int device = 0;
    (void)admpc_quad_solver_info(s, &device, nullptr, nullptr);
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_quad_rdrv_install_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, admpc_quad_solver_config_device(s, nullptr), d_dev, info, installed);
    return launched("admpc_quad_rdrv_install_kernel");
}

}  // extern "C"
