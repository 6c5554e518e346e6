// admpc_quad_select.hip -- the training points of every regressor of a clustered ensemble picked from a log of sample records on the
// device (include/admpc_quad_select.h): per (cluster, regressor, bin) the median record of the reference's distance_maximizing_points_1d,
// by a radix select on an order-preserving 64-bit key of the feature value.
//
//   init     admpc_quad_select_init_kernel    the work area: histograms, counts and ranks zeroed, the minima and maxima at their identities
//   range    admpc_quad_select_range_kernel   256-thread blocks striding over the records: who takes part and in which cluster (the code of
//                                             a record), min / max of the key per (cluster, regressor) by 64-bit INTEGER atomics in LDS, one
//                                             global one per block and destination
//   edges    admpc_quad_select_edges_kernel   one wave, lane (c, g): np.linspace's edges from the two keys
//   count    admpc_quad_select_count_kernel   the bin of every record by comparison against the edges (into its code), the members and the
//                                             highest record index of every bin in LDS, one global atomic per block and bin that is not empty
//   digit    admpc_quad_select_digit_kernel   once per digit, eight times: the histogram of the next 8 bits of the keys that still match the
//                                             prefix, without the member set aside; per block and bin the FIRST digit seen is counted in LDS
//                                             and leaves as one atomic, any other digit goes to memory at once
//   pick     admpc_quad_select_pick_kernel    behind every digit pass, one wave per bin: the digit that holds the wanted rank, by a wave scan
//                                             over the 256 counters, which it zeroes for the next pass
//   lowest   admpc_quad_select_lowest_kernel  the lowest record index whose key equals the median's, the member set aside included
//   gather   admpc_quad_select_gather_kernel  one wave per (cluster, regressor): the records into bins, sel and info
//
// Integer atomics only: every sum, minimum and maximum is of integers, so two runs give the same bits.  Every grid is a function of M and
// of constants.  The regressors' feature and output and the centroids are read by pointer from the object's device copies.  Everything the
// rule rounds (the edges) is written without contraction.
#include <stdio.h>
#include <math.h>
#include <limits.h>
#include "admpc_host.h"
#include "../../include/admpc_quad_select.h"

#define NX ADMPC_NX           // model_dev.h (exp_nonpos, which the bodies of gp_fit_dev.h name) wants the car's dimensions defined
#define NU ADMPC_NU
#define NY ADMPC_NY
#include "gp_fit_dev.h"       // WAVE, NPT, ACC; LearnGp
#define QREC 14               // doubles per sample record, as admpc_quad_learn.hip lays it out
#define KMAX ADMPC_QUAD_CLUSTERS_MAX
#define GMAX ADMPC_QUAD_GP_MAX
#define STHREADS 256
#define NCG (KMAX * GMAX)                 // (cluster, regressor) pairs of the work area, whatever K is
#define NSLOT (NCG * NPT)                 // bins of the work area
#define RADIX 256
#define PASSES ADMPC_SELECT_PASSES
#define NONE 63                           // the 6-bit bin of a record's code that is in no bin of a regressor
#define EROW (NPT + 1)                    // doubles per row of edges

// the work area, in int32 words (include/admpc_quad_select.h: THE WORK AREA); the 64-bit arrays at even offsets
#define W_CNT 0
#define W_MAXI (W_CNT + NSLOT)
#define W_MINI (W_MAXI + NSLOT)
#define W_RANK (W_MINI + NSLOT)
#define W_TOOK (W_RANK + NSLOT)
#define W_KMIN (W_TOOK + 32)
#define W_KMAX (W_KMIN + 2 * 32)
#define W_PRE (W_KMAX + 2 * 32)
#define W_HIST (W_PRE + 2 * NSLOT)
#define W_END (W_HIST + NSLOT * RADIX)

static_assert(W_END == ADMPC_SELECT_WORK, "include/admpc_quad_select.h states the size of the work area");
static_assert(NPT == 32 && GMAX == 3 && KMAX == 8 && NCG <= 32, "a code holds a 3-bit cluster and three 6-bit bins; a (c, g) pair per lane");
static_assert(PASSES * 8 == 64, "the digits cover the key");

typedef unsigned long long u64;

struct SelectArgs {
    long long M;
    int K, n_gp, d, f[3], n[3], pass;
    const double* cent;                       // [K][d], the object's
    const LearnGp* gp;                        // [K][GMAX], the object's
    const double* rec;                        // [M][QREC]
    int32_t* code;                            // [M]
    double* edges;                            // [K][GMAX][EROW]
    int32_t* work;                            // [ADMPC_SELECT_WORK]
    double* bins;                             // [K][GMAX][NPT][ACC]
    int32_t* sel;                             // [K][GMAX][NPT]
    int32_t* info;                            // [K][GMAX][4]
};

namespace {

#include "model_dev.h"

constexpr int QU = ADMPC_QUAD_NU, QY = ADMPC_QUAD_NY;
typedef AdmpcQuadConfig Cfg;

#include "quad_model_dev.h"
#include "quad_route_dev.h"

// the order of the finite doubles as the order of unsigned integers, -0.0 folded onto +0.0; no finite value has the key 0
__device__ __forceinline__ u64 sel_key(double z)
{
    z = z == 0.0 ? 0.0 : z;
    const u64 b = (u64)__double_as_longlong(z);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double sel_unkey(u64 k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// where regressor g reads its feature and its target in a record (held into the record, whatever the device copy says)
__device__ __forceinline__ int sel_zi(const LearnGp* __restrict__ gp, int g) { const int i = gp[g].feat[0] - 7; return i < 0 ? 0 : (i > 9 ? 9 : i); }
__device__ __forceinline__ int sel_yi(const LearnGp* __restrict__ gp, int g) { const int i = gp[g].out - 7; return 10 + (i < 0 ? 0 : (i > 2 ? 2 : i)); }

__device__ __forceinline__ int code_bin(int code, int g) { return (code >> (3 + 6 * g)) & 63; }

}  // namespace

// grid: a function of M alone (select_blocks below)
__global__ __launch_bounds__(STHREADS) void admpc_quad_select_init_kernel(int32_t* __restrict__ work)
{
    for (int i = (int)(blockIdx.x * STHREADS + threadIdx.x); i < W_END; i += (int)gridDim.x * STHREADS) {
        int v = 0;
        if (i >= W_MAXI && i < W_MINI) v = -1;
        else if (i >= W_MINI && i < W_RANK) v = INT_MAX;
        else if (i >= W_KMIN && i < W_KMAX) v = -1;             // all ones: the identity of the unsigned minimum
        work[i] = v;
    }
}

// grid: a function of M alone
__global__ __launch_bounds__(STHREADS) void admpc_quad_select_range_kernel(const SelectArgs a)
{
    __shared__ u64 mn[NCG], mx[NCG];
    const int tid = (int)threadIdx.x;
    if (tid < NCG) { mn[tid] = ~0ull; mx[tid] = 0ull; }
    __syncthreads();
    const int zi[3] = { sel_zi(a.gp, 0), a.n_gp > 1 ? sel_zi(a.gp, 1) : 0, a.n_gp > 2 ? sel_zi(a.gp, 2) : 0 };
    const int yi[3] = { sel_yi(a.gp, 0), a.n_gp > 1 ? sel_yi(a.gp, 1) : 10, a.n_gp > 2 ? sel_yi(a.gp, 2) : 10 };
    for (long long i = (long long)blockIdx.x * STHREADS + tid; i < a.M; i += (long long)gridDim.x * STHREADS) {
        const double* __restrict__ r = a.rec + i * QREC;
        int code = (NONE << 3) | (NONE << 9) | (NONE << 15);
        if (r[QREC - 1] == 1.0) {
            const double zc[3] = { r[a.f[0] - 7], a.d > 1 ? r[a.f[1] - 7] : 0.0, a.d > 2 ? r[a.f[2] - 7] : 0.0 };
            const int c = quad_nearest(zc, a.d, a.K, a.cent);
            code |= c;
#pragma unroll
            for (int g = 0; g < GMAX; ++g) {
                if (g < a.n_gp) {
                    const double z = r[zi[g]], y = r[yi[g]];
                    if (isfinite(z) && isfinite(y)) {
                        const u64 k = sel_key(z);
                        atomicMin(&mn[c * GMAX + g], k);
                        atomicMax(&mx[c * GMAX + g], k);
                        code &= ~(NONE << (3 + 6 * g));          // takes part: bin 0 until the count pass says which
                    }
                }
            }
        }
        a.code[i] = code;
    }
    __syncthreads();
    if (tid < NCG && mx[tid] != 0ull) {
        atomicMin((u64*)(a.work + W_KMIN) + tid, mn[tid]);
        atomicMax((u64*)(a.work + W_KMAX) + tid, mx[tid]);
    }
}

// one wave: lane c * 3 + g writes the edges of its regressor, e_j = lo + j * ((hi - lo) / n) and e_n = hi
__global__ __launch_bounds__(WAVE) void admpc_quad_select_edges_kernel(const SelectArgs a)
{
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x, c = lane / GMAX, g = lane % GMAX;
    if (lane >= NCG || c >= a.K || g >= a.n_gp) return;
    const u64 kmin = ((const u64*)(a.work + W_KMIN))[lane], kmax = ((const u64*)(a.work + W_KMAX))[lane];
    if (kmax == 0ull) return;                                    // no record takes part: nothing reads the edges
    const int n = a.n[g];
    double lo = sel_unkey(kmin), hi = sel_unkey(kmax);
    if (lo == hi) { lo = lo - 0.5; hi = hi + 0.5; }
    const double step = (hi - lo) / (double)n;
    double* e = a.edges + (size_t)lane * EROW;
    for (int j = 0; j < n; ++j) {
        const double js = (double)j * step;
        e[j] = lo + js;
    }
    e[n] = hi;
}

// grid: a function of M alone
__global__ __launch_bounds__(STHREADS) void admpc_quad_select_count_kernel(const SelectArgs a)
{
    __shared__ double e[NCG][EROW];
    __shared__ int cnt[NSLOT], mxi[NSLOT], took[NCG];
    const int tid = (int)threadIdx.x;
    for (int k = tid; k < a.K * GMAX * EROW; k += STHREADS) (&e[0][0])[k] = a.edges[k];
    for (int k = tid; k < NSLOT; k += STHREADS) { cnt[k] = 0; mxi[k] = -1; }
    if (tid < NCG) took[tid] = 0;
    __syncthreads();
    const int zi[3] = { sel_zi(a.gp, 0), a.n_gp > 1 ? sel_zi(a.gp, 1) : 0, a.n_gp > 2 ? sel_zi(a.gp, 2) : 0 };
    for (long long i = (long long)blockIdx.x * STHREADS + tid; i < a.M; i += (long long)gridDim.x * STHREADS) {
        int code = a.code[i];
        const int c = code & 7;
        bool mine = false;
#pragma unroll
        for (int g = 0; g < GMAX; ++g) {
            if (code_bin(code, g) == NONE) continue;
            mine = true;
            const int cg = c * GMAX + g, n = a.n[g];
            const double z = a.rec[i * QREC + zi[g]];
            atomicAdd(&took[cg], 1);
            // np.digitize(z, e) - 1: the edges that are <= z, less one; z == hi has index n and is in no bin
            int le = 0;
            for (int j = 0; j <= n; ++j) le += e[cg][j] <= z ? 1 : 0;
            const int bin = le - 1;
            const bool in = bin >= 0 && bin < n;
            if (in) {
                atomicAdd(&cnt[cg * NPT + bin], 1);
                atomicMax(&mxi[cg * NPT + bin], (int)i);
            }
            code = (code & ~(NONE << (3 + 6 * g))) | ((in ? bin : NONE) << (3 + 6 * g));
        }
        if (mine) a.code[i] = code;
    }
    __syncthreads();
    for (int k = tid; k < a.K * GMAX * NPT; k += STHREADS) {
        if (cnt[k]) { atomicAdd(a.work + W_CNT + k, cnt[k]); atomicMax(a.work + W_MAXI + k, mxi[k]); }
    }
    if (tid < NCG && took[tid]) atomicAdd(a.work + W_TOOK + tid, took[tid]);
}

// grid: a function of M alone.  a.pass: 0 .. PASSES - 1, the most significant digit first
__global__ __launch_bounds__(STHREADS) void admpc_quad_select_digit_kernel(const SelectArgs a)
{
    __shared__ u64 pre[NSLOT];
    __shared__ int excl[NSLOT], cdig[NSLOT], ccnt[NSLOT];
    const int tid = (int)threadIdx.x, p = a.pass;
    for (int k = tid; k < a.K * GMAX * NPT; k += STHREADS) {
        const int m = a.work[W_CNT + k];
        excl[k] = (m > 0 && (m & 1) == 0) ? a.work[W_MAXI + k] : -1;        // an even bin sets its highest record index aside
        pre[k] = ((const u64*)(a.work + W_PRE))[k];
        cdig[k] = -1; ccnt[k] = 0;
    }
    __syncthreads();
    const int zi[3] = { sel_zi(a.gp, 0), a.n_gp > 1 ? sel_zi(a.gp, 1) : 0, a.n_gp > 2 ? sel_zi(a.gp, 2) : 0 };
    int32_t* __restrict__ hist = a.work + W_HIST;
    for (long long i = (long long)blockIdx.x * STHREADS + tid; i < a.M; i += (long long)gridDim.x * STHREADS) {
        const int code = a.code[i], c = code & 7;
#pragma unroll
        for (int g = 0; g < GMAX; ++g) {
            const int bin = code_bin(code, g);
            if (bin == NONE) continue;
            const int slot = (c * GMAX + g) * NPT + bin;
            if ((int)i == excl[slot]) continue;
            const u64 k = sel_key(a.rec[i * QREC + zi[g]]);
            if (p > 0 && (k >> (64 - 8 * p)) != pre[slot]) continue;
            const int dig = (int)((k >> (56 - 8 * p)) & (RADIX - 1));
            // the first digit a block sees in a bin is counted in LDS (the leading digits of a bin's members are nearly always one value)
            const int old = atomicCAS(&cdig[slot], -1, dig);
            if (old == -1 || old == dig) atomicAdd(&ccnt[slot], 1);
            else atomicAdd(hist + slot * RADIX + dig, 1);
        }
    }
    __syncthreads();
    for (int k = tid; k < a.K * GMAX * NPT; k += STHREADS)
        if (ccnt[k]) atomicAdd(hist + k * RADIX + cdig[k], ccnt[k]);
}

// grid K * GMAX * NPT, one wave per bin: the digit whose counter holds the rank that is left, into the prefix; the counters zeroed
__global__ __launch_bounds__(WAVE) void admpc_quad_select_pick_kernel(const SelectArgs a)
{
    const int slot = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int m = a.work[W_CNT + slot];
    if (m == 0) return;
    const int odd = (m & 1) ? m : m - 1;
    const int rank = a.pass == 0 ? (odd - 1) / 2 : a.work[W_RANK + slot];
    int32_t* __restrict__ h = a.work + W_HIST + slot * RADIX + 4 * lane;
    const int h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3];
    h[0] = 0; h[1] = 0; h[2] = 0; h[3] = 0;
    const int own = (h0 + h1) + (h2 + h3);
    int incl = own;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    const int before = incl - own;
    if (rank >= before && rank < incl) {                         // one lane: the counters are not negative and sum to more than rank
        int left = rank - before, dig = 0;
        if (left >= h0) { left -= h0; dig = 1; if (left >= h1) { left -= h1; dig = 2; if (left >= h2) { left -= h2; dig = 3; } } }
        u64* pre = (u64*)(a.work + W_PRE) + slot;
        *pre = (a.pass == 0 ? 0ull : (*pre << 8)) | (u64)(4 * lane + dig);
        a.work[W_RANK + slot] = left;
    }
}

// grid: a function of M alone
__global__ __launch_bounds__(STHREADS) void admpc_quad_select_lowest_kernel(const SelectArgs a)
{
    __shared__ u64 pre[NSLOT];
    __shared__ int mni[NSLOT];
    const int tid = (int)threadIdx.x;
    for (int k = tid; k < a.K * GMAX * NPT; k += STHREADS) { pre[k] = ((const u64*)(a.work + W_PRE))[k]; mni[k] = INT_MAX; }
    __syncthreads();
    const int zi[3] = { sel_zi(a.gp, 0), a.n_gp > 1 ? sel_zi(a.gp, 1) : 0, a.n_gp > 2 ? sel_zi(a.gp, 2) : 0 };
    for (long long i = (long long)blockIdx.x * STHREADS + tid; i < a.M; i += (long long)gridDim.x * STHREADS) {
        const int code = a.code[i], c = code & 7;
#pragma unroll
        for (int g = 0; g < GMAX; ++g) {
            const int bin = code_bin(code, g);
            if (bin == NONE) continue;
            const int slot = (c * GMAX + g) * NPT + bin;
            if (sel_key(a.rec[i * QREC + zi[g]]) == pre[slot]) atomicMin(&mni[slot], (int)i);
        }
    }
    __syncthreads();
    for (int k = tid; k < a.K * GMAX * NPT; k += STHREADS)
        if (mni[k] != INT_MAX) atomicMin(a.work + W_MINI + k, mni[k]);
}

// grid K * GMAX, one wave per (cluster, regressor), lane j < 32 bin j: row r of bins is the record of the r-th bin that is not empty
__global__ __launch_bounds__(WAVE) void admpc_quad_select_gather_kernel(const SelectArgs a)
{
    const int cg = (int)blockIdx.x, g = cg % GMAX, lane = (int)threadIdx.x;
    const bool asked = g < a.n_gp;
    const int n = asked ? a.n[g] : 0;
    const int took = asked ? a.work[W_TOOK + cg] : 0;
    int idx = -1;
    if (lane < n && a.work[W_CNT + cg * NPT + lane] > 0) idx = a.work[W_MINI + cg * NPT + lane];
    const bool has = idx >= 0 && idx != INT_MAX && (long long)idx < a.M;
    const u64 mask = __ballot(has);
    const int npts = __popcll(mask), pos = __popcll(mask & ((1ull << lane) - 1ull));
    double* rows = a.bins + (size_t)cg * NPT * ACC;
    if (has) {
        const double* __restrict__ r = a.rec + (long long)idx * QREC;
        double* o = rows + pos * ACC;
        o[0] = 1.0; o[1] = r[sel_zi(a.gp, g)]; o[2] = 0.0; o[3] = 0.0; o[4] = r[sel_yi(a.gp, g)];
    }
    if (lane < NPT) {
        a.sel[cg * NPT + lane] = has ? idx : -1;
        if (lane >= npts) {
            double* o = rows + lane * ACC;
#pragma unroll
            for (int k = 0; k < ACC; ++k) o[k] = 0.0;
        }
    }
    if (lane == 0) {
        int32_t* o = a.info + cg * 4;
        o[0] = npts; o[1] = took; o[2] = n - npts; o[3] = (asked && took == 0) ? ADMPC_SELECT_ENOVALID : 0;
    }
}

namespace {

int launched(const char* kernel)
{
    if (hipGetLastError() == hipSuccess) return ADMPC_OK;
    char msg[120];
    snprintf(msg, sizeof msg, "%s: launch failed", kernel);
    return admpc_set_error(ADMPC_EHIP, msg);
}

// the grid of every kernel over the records: a function of M alone, as admpc_quad_prune.hip's
int select_blocks(long long M)
{
    const long long n = (M + STHREADS - 1) / STHREADS;
    return (int)(n < ADMPC_GMM_BLOCKS_MAX ? n : ADMPC_GMM_BLOCKS_MAX);
}

}  // namespace

extern "C" int admpc_quad_ensemble_select_points(const AdmpcQuadEnsemble* e, int64_t M, const double* log, const int32_t* n_points, int32_t* code,
                                                 double* edges, int32_t* work, double* bins, int32_t* sel, int32_t* info, void* stream)
{
    const char* who = "admpc_quad_ensemble_select_points";
    if (!e) return admpc_refuse(who, "null ensemble");
    QuadEnsembleView v;
    admpc_quad_ensemble_view(e, &v);
    if (!v.learns) return admpc_refuse(who, "the ensemble was created without observe parameters");
    if (M < 0 || M > INT32_MAX) return admpc_refuse(who, "the number of records must be in [0, INT32_MAX]");
    for (int c = 0; c < v.K; ++c)
        for (int g = 0; g < v.n_gp; ++g)
            if (v.obs[c].gp[g].n_feat != 1) return admpc_refuse(who, "a regressor with more than one feature: the selection is offered for one-feature regressors");
    if (!n_points) return admpc_refuse(who, "null n_points");
    for (int g = 0; g < v.n_gp; ++g) {
        int most = NPT;
        for (int c = 0; c < v.K; ++c) {
            const AdmpcGpBins& b = v.obs[c].gp[g];
            const int nbins = b.nb[0] * b.nb[1] * b.nb[2];
            most = nbins < most ? nbins : most;
        }
        if (n_points[g] < 1 || n_points[g] > most) return admpc_refuse(who, "n_points must be in [1, min(32, nbins)] of every regressor");
    }
    for (int j = 0; j < v.n_feat; ++j)
        if (v.feat[j] < 7 || v.feat[j] >= QY) return admpc_refuse(who, "the clustering features must lie in [7, 16]: the sample record holds no others");
    if (M == 0) return ADMPC_OK;
    if (!log || !code || !edges || !work || !bins || !sel || !info) return admpc_refuse(who, "null array argument");
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    SelectArgs a = SelectArgs();
    a.M = (long long)M; a.K = v.K; a.n_gp = v.n_gp; a.d = v.n_feat;
    for (int j = 0; j < 3; ++j) { a.f[j] = j < v.n_feat ? v.feat[j] : 7; a.n[j] = j < v.n_gp ? n_points[j] : 0; }
    a.cent = v.cent; a.gp = v.gp; a.rec = log; a.code = code; a.edges = edges; a.work = work; a.bins = bins; a.sel = sel; a.info = info;
    const int nblk = select_blocks(M);
    hipLaunchKernelGGL(admpc_quad_select_init_kernel, dim3(nblk), dim3(STHREADS), 0, st, work);
    int rc = launched("admpc_quad_select_init_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(admpc_quad_select_range_kernel, dim3(nblk), dim3(STHREADS), 0, st, a);
    rc = launched("admpc_quad_select_range_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(admpc_quad_select_edges_kernel, dim3(1), dim3(WAVE), 0, st, a);
    rc = launched("admpc_quad_select_edges_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(admpc_quad_select_count_kernel, dim3(nblk), dim3(STHREADS), 0, st, a);
    rc = launched("admpc_quad_select_count_kernel");
    if (rc) return rc;
    for (int p = 0; p < PASSES; ++p) {
        a.pass = p;
        hipLaunchKernelGGL(admpc_quad_select_digit_kernel, dim3(nblk), dim3(STHREADS), 0, st, a);
        rc = launched("admpc_quad_select_digit_kernel");
        if (rc) return rc;
        hipLaunchKernelGGL(admpc_quad_select_pick_kernel, dim3((unsigned)(v.K * GMAX * NPT)), dim3(WAVE), 0, st, a);
        rc = launched("admpc_quad_select_pick_kernel");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(admpc_quad_select_lowest_kernel, dim3(nblk), dim3(STHREADS), 0, st, a);
    rc = launched("admpc_quad_select_lowest_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(admpc_quad_select_gather_kernel, dim3((unsigned)(v.K * GMAX)), dim3(WAVE), 0, st, a);
    return launched("admpc_quad_select_gather_kernel");
}
