// admpc_quad_kmeans.hip -- the start of the Gaussian-mixture EM found on the device (include/admpc_quad_kmeans.h): scikit-learn's greedy
// k-means++ seeding and its Lloyd k-means over the logged sample records, and the n_init rule that keeps the best of several fits.
//
//   pack     admpc_quad_gmm_pack_kernel         admpc_quad_clusters.hip's, launched from here as it is: record [14] -> (z_0, z_1, z_2, flag)
//   prep     admpc_quad_kmeans_prep_kernel      tiles of 256 records: the count of every tile, labels = -1, and one row of partial per block
//                                               with the count and the first two moments about record 0 (the variance behind tol_abs)
//   seed0    admpc_quad_kmeans_seed0_kernel     one wave: n_valid, tol_abs, the refusals of the data, the scan of the tile counts and the walk
//                                               to the r-th counting record
//   cand     admpc_quad_kmeans_cand_kernel      per trial the sum of min(D2, d2(x, x_cand)): one row of partial per block
//   finish   admpc_quad_kmeans_finish_kernel    one wave: adds the rows, the smallest potential wins, its record becomes centre c
//   update   admpc_quad_kmeans_update_kernel    D2 <- min(D2, d2(x, centre c)) and the sum of every tile
//   pick     admpc_quad_kmeans_pick_kernel      one wave: the thresholds of a round, the scan of the tile sums, the walk inside one tile (its
//                                               last counting record if rounding hides the crossing there)
//   assign   admpc_quad_kmeans_assign_kernel<K, FINAL>  labels by quad_nearest, changed labels counted, count and first moment about the
//                                               current centre per cluster, and the inertia: one row of partial per block
//   move     admpc_quad_kmeans_move_kernel      one wave: adds the rows, moves the centres, the shift and the two stops
//   end      admpc_quad_kmeans_end_kernel       one wave: the inertia, the centres, stats
//   keep     admpc_quad_clusters_keep_kernel    one wave: the n_init rule over two mixture states
//            admpc_quad_kmeans_keep_kernel      the k-means results of the try that rule has just kept, copied beside it
//
// No floating-point atomics: every sum goes through rows of partial that one wave adds in a fixed order; the one atomic counts changed
// labels, in integers.  Every kernel behind seed0 reads the status (the Lloyd kernels the converged flag too) and returns at once when it
// is set, so that the number of launches is a function of K and max_iter alone and a call can be captured.
#include <stdio.h>
#include <math.h>
#include "admpc_host.h"
#include "../../include/admpc_quad_clusters.h"
#include "../../include/admpc_quad_kmeans.h"

#define QREC 14
#define FEAT_LO 7
#define KMAX ADMPC_QUAD_CLUSTERS_MAX
#define KT 256                                  // records per tile, threads per block
#define KPART ADMPC_KMEANS_PARTIAL
#define KSTATE ADMPC_KMEANS_STATE
#define KTRIALS 4                               // 2 + int(ln 8)
// the state at the end of work, in doubles: the potential, tol_abs, the last shift, then the current centres [K][d] from ST_CUR; from
// ST_INT on 64-bit integers: the candidates of a round [4] and the last counting record; at ST_CHANGED an int32 counter
#define ST_POT 0
#define ST_TOL 1
#define ST_SHIFT 2
#define ST_CUR 8
#define ST_INT 32
#define ST_LAST 4
#define ST_CHANGED 40

// admpc_quad_clusters.hip defines it; the pack of the EM is the pack of the k-means
__global__ void admpc_quad_gmm_pack_kernel(long long M, int d, int f0, int f1, int f2, const double* __restrict__ rec, double* __restrict__ packed);

namespace {

#define NX ADMPC_NX           // model_dev.h wants the car's dimensions defined
#define NU ADMPC_NU
#define NY ADMPC_NY
#include "model_dev.h"

[[maybe_unused]] constexpr int QX = ADMPC_QUAD_NX, QU = ADMPC_QUAD_NU, QY = ADMPC_QUAD_NY;      // quad_model_dev.h speaks of them
typedef AdmpcQuadConfig Cfg;

#include "quad_model_dev.h"
#include "quad_route_dev.h"
#include "quad_noise_dev.h"

static_assert(KPART == 4 * KMAX + 1, "a row of partial holds count and first moment of eight clusters and the inertia");
static_assert(ST_CUR + 3 * KMAX <= ST_INT && ST_CHANGED < KSTATE, "the state fits");

struct Work {
    double* tsum; long long* tcnt; double* partial; double* st; long long* sti; int* changed;
};

__host__ __device__ __forceinline__ Work work_of(double* work, long long M)
{
    const long long nt = (M + KT - 1) / KT;
    Work w;
    w.tsum = work; w.tcnt = (long long*)(work + nt); w.partial = work + 2 * nt; w.st = w.partial + (size_t)ADMPC_GMM_BLOCKS_MAX * KPART;
    w.sti = (long long*)(w.st + ST_INT); w.changed = (int*)(w.st + ST_CHANGED);
    return w;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double wave_scan(double v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const double t = __shfl_up(v, o); if (lane >= o) v += t; }
    return v;
}

__device__ __forceinline__ long long wave_scan(long long v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long t = __shfl_up(v, o); if (lane >= o) v += t; }
    return v;
}

// the header's D2: every operation rounded on its own
__device__ __forceinline__ double dsq(double x0, double x1, double x2, double c0, double c1, double c2)
{
#pragma clang fp contract(off)
    const double e0 = x0 - c0, e1 = x1 - c1, e2 = x2 - c2;
    return (e0 * e0 + e1 * e1) + e2 * e2;
}

// the sum of one value per thread over the block, the same in every thread; red [4] is LDS
__device__ __forceinline__ double block_sum(double v, double* red, int tid)
{
    v = wave_sum(v);
    __syncthreads();
    if (tid % 64 == 0) red[tid / 64] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave adds column e (< ne <= 64) of the nblk rows of partial in a fixed order into sum [ne] (LDS)
__device__ __forceinline__ void add_rows(const double* __restrict__ partial, int nblk, int ne, int lane, double* sum)
{
    if (lane < ne) {
        double a[4] = { 0.0, 0.0, 0.0, 0.0 };
        int r = 0;
        for (; r + 3 < nblk; r += 4) {
            double v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = partial[(size_t)(r + q) * KPART + lane];
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] += v[q];
        }
        for (; r < nblk; ++r) a[0] += partial[(size_t)r * KPART + lane];
        sum[lane] = (a[0] + a[1]) + (a[2] + a[3]);
    }
    __syncthreads();
}

// a failure: the status, and the ensemble's present centroids into centers
__device__ __forceinline__ void fail(int status, int n, const double* __restrict__ cent, double* __restrict__ centers, int32_t* __restrict__ info, int lane)
{
    if (lane < n) centers[lane] = cent[lane];
    if (lane == 0) info[2] = status;
}

// the `want`-th (0-based) counting record of tile `tile`, or the last one of it (last != 0); -1 if the tile has no such record.  One wave,
// four consecutive records per lane.
__device__ __forceinline__ long long tile_nth(const double* __restrict__ packed, long long M, long long tile, long long want, int last, int lane)
{
    const long long i0 = tile * KT + 4 * lane;
    int f[4], n = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { f[q] = i0 + q < M && packed[(i0 + q) * 4 + 3] == 1.0; n += f[q]; }
    const long long incl = wave_scan((long long)n, lane), excl = incl - n;
    int hit = -1;
    if (last) {
#pragma unroll
        for (int q = 0; q < 4; ++q) if (f[q]) hit = q;
        const unsigned long long who = __ballot(hit >= 0);
        if (!who) return -1;
        const int L = 63 - __clzll((long long)who);
        return __shfl((long long)(i0 + hit), L);
    }
    long long seen = excl;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (f[q]) { if (seen == want && hit < 0) hit = q; ++seen; }
    }
    const unsigned long long who = __ballot(hit >= 0);
    if (!who) return -1;
    const int L = __ffsll((long long)who) - 1;
    return __shfl((long long)(i0 + hit), L);
}

}  // namespace

__global__ __launch_bounds__(KT) void admpc_quad_kmeans_prep_kernel(long long M, const double* __restrict__ packed, int32_t* __restrict__ labels,
                                                                    double* __restrict__ work)
{
    __shared__ int wc[4];
    __shared__ double red[4];
    const Work w = work_of(work, M);
    const int tid = (int)threadIdx.x;
    const long long nt = (M + KT - 1) / KT;
    const double p0 = packed[0], p1 = packed[1], p2 = packed[2];         // the pivot of the moments: record 0 (zeros if it does not count)
    double acc[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (long long tile = blockIdx.x; tile < nt; tile += gridDim.x) {
        const long long i = tile * KT + tid;
        bool ok = false;
        if (i < M) {
            const double* p = packed + i * 4;
            labels[i] = -1;
            ok = p[3] == 1.0;
            if (ok) {
                const double e0 = p[0] - p0, e1 = p[1] - p1, e2 = p[2] - p2;
                acc[0] += 1.0; acc[1] += e0; acc[2] += e1; acc[3] += e2; acc[4] += e0 * e0; acc[5] += e1 * e1; acc[6] += e2 * e2;
            }
        }
        const int n = __popcll(__ballot(ok));
        __syncthreads();
        if (tid % 64 == 0) wc[tid / 64] = n;
        __syncthreads();
        if (tid == 0) w.tcnt[tile] = (wc[0] + wc[1]) + (wc[2] + wc[3]);
    }
    for (int e = 0; e < 7; ++e) {
        const double v = block_sum(acc[e], red, tid);
        if (tid == 0) w.partial[(size_t)blockIdx.x * KPART + e] = v;
    }
}

__global__ __launch_bounds__(64) void admpc_quad_kmeans_seed0_kernel(long long M, int nblk, int K, int d, uint64_t seed, uint32_t draw, double tol,
                                                                     const double* __restrict__ packed, const double* __restrict__ cent, double* __restrict__ work,
                                                                     double* __restrict__ centers, double* __restrict__ stats, int32_t* __restrict__ info)
{
    __shared__ double sum[64];
    const Work w = work_of(work, M);
    const int lane = (int)threadIdx.x;
    const long long nt = (M + KT - 1) / KT;
    add_rows(w.partial, nblk, 7, lane, sum);
    const double n = sum[0];
    if (lane == 0) {
        info[0] = 0; info[1] = 0; info[2] = 0; info[3] = (int32_t)n;
        w.changed[0] = 0;
        w.st[ST_POT] = 0.0; w.st[ST_SHIFT] = 0.0; w.st[ST_TOL] = 0.0;
    }
    if (lane < 4) stats[lane] = 0.0;
    if (!(n > 0.0)) { fail(ADMPC_GMM_ENOVALID, K * d, cent, centers, info, lane); return; }
    if (n < (double)K) { fail(ADMPC_KMEANS_EFEW, K * d, cent, centers, info, lane); return; }
    if (lane == 0) {
        double var = 0.0;
        for (int j = 0; j < d; ++j) { const double s = sum[1 + j] / n; var += sum[4 + j] / n - s * s; }
        w.st[ST_TOL] = tol * (var / d);
    }
    uint32_t o[4];
    philox4x32_10(0u, draw, 0u, ADMPC_KMEANS_PHILOX_WORD, (uint32_t)seed, (uint32_t)(seed >> 32), o);
    const uint64_t w0 = (uint64_t)o[0] | (uint64_t)o[1] << 32;
    const double u = ((double)(w0 >> 11) + 0.5) * 0x1p-53;
    long long r = (long long)floor(u * n);
    const long long nv = (long long)n;
    r = r < nv - 1 ? r : nv - 1;
    // the scan of the tile counts: lane l has the tiles [l per, (l + 1) per)
    const long long per = (nt + 63) / 64, lo = lane * per, hi = lo + per < nt ? lo + per : nt;
    long long mine = 0;
    for (long long t = lo; t < hi; ++t) mine += w.tcnt[t];
    const long long incl = wave_scan(mine, lane);
    long long tile = 0, base = 0, ltile = 0;
    {
        const int L = __ffsll((long long)__ballot(incl > r)) - 1;          // n_valid > r: there is one
        long long seen = incl - mine, tt = lo;
        if (lane == L)
            for (long long t = lo; t < hi; ++t) { const long long c = w.tcnt[t]; if (seen + c > r) { tt = t; break; } seen += c; }
        tile = __shfl(tt, L); base = __shfl(seen, L);
        const int LL = 63 - __clzll((long long)__ballot(mine > 0));
        long long lt = lo;
        if (lane == LL)
            for (long long t = lo; t < hi; ++t) if (w.tcnt[t] > 0) lt = t;
        ltile = __shfl(lt, LL);
    }
    const long long first = tile_nth(packed, M, tile, r - base, 0, lane), last = tile_nth(packed, M, ltile, 0, 1, lane);
    if (lane == 0) { w.sti[0] = first; w.sti[ST_LAST] = last; }
}

// per trial t < T the block's sum of min(D2_i, d2(x_i, x_cand t)) (first: of d2 alone) into row blockIdx.x of partial
__global__ __launch_bounds__(KT) void admpc_quad_kmeans_cand_kernel(long long M, int T, int first, const double* __restrict__ packed,
                                                                    const double* __restrict__ dist, double* __restrict__ work, const int32_t* __restrict__ info)
{
    __shared__ double red[4];
    if (info[2]) return;
    const Work w = work_of(work, M);
    const int tid = (int)threadIdx.x;
    double xc[KTRIALS][3], acc[KTRIALS];
#pragma unroll
    for (int t = 0; t < KTRIALS; ++t) {
        long long c = t < T ? w.sti[t] : w.sti[0];
        c = c >= 0 && c < M ? c : 0;
        xc[t][0] = packed[c * 4]; xc[t][1] = packed[c * 4 + 1]; xc[t][2] = packed[c * 4 + 2];
        acc[t] = 0.0;
    }
    for (long long i = (long long)blockIdx.x * KT + tid; i < M; i += (long long)gridDim.x * KT) {
        const double* p = packed + i * 4;
        if (p[3] != 1.0) continue;
        const double x0 = p[0], x1 = p[1], x2 = p[2], D = first ? INFINITY : dist[i];
#pragma unroll
        for (int t = 0; t < KTRIALS; ++t) {
            if (t < T) {
                const double e = dsq(x0, x1, x2, xc[t][0], xc[t][1], xc[t][2]);
                acc[t] += e < D ? e : D;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < KTRIALS; ++t) {
        if (t < T) {                                  // T is the launch's: every thread of the block takes the same way
            const double v = block_sum(acc[t], red, tid);
            if (tid == 0) w.partial[(size_t)blockIdx.x * KPART + t] = v;
        }
    }
}

// one wave: the trial with the smallest potential wins, ties to the lower trial; its record is centre c
__global__ __launch_bounds__(64) void admpc_quad_kmeans_finish_kernel(long long M, int nblk, int K, int d, int c, int T, const double* __restrict__ packed,
                                                                      const double* __restrict__ cent, double* __restrict__ work, double* __restrict__ centers,
                                                                      int64_t* __restrict__ idx, int32_t* __restrict__ info)
{
    __shared__ double sum[64];
    if (info[2]) return;
    const Work w = work_of(work, M);
    const int lane = (int)threadIdx.x;
    add_rows(w.partial, nblk, T, lane, sum);
    int best = 0;
    for (int t = 1; t < T; ++t) best = sum[t] < sum[best] ? t : best;
    const double pot = sum[best];
    long long rec = w.sti[best];
    rec = rec >= 0 && rec < M ? rec : 0;
    if (c + 1 < K && !(pot > 0.0)) { fail(ADMPC_KMEANS_EFEW, K * d, cent, centers, info, lane); return; }
    if (lane < d) w.st[ST_CUR + c * d + lane] = packed[rec * 4 + lane];
    if (lane == 0) { idx[c] = rec; w.st[ST_POT] = pot; }
}

// D2 of every record under centre c as well, and the sum of every tile
__global__ __launch_bounds__(KT) void admpc_quad_kmeans_update_kernel(long long M, int d, int c, int first, const double* __restrict__ packed,
                                                                      double* __restrict__ dist, double* __restrict__ work, const int32_t* __restrict__ info)
{
    __shared__ double red[4];
    if (info[2]) return;
    const Work w = work_of(work, M);
    const int tid = (int)threadIdx.x;
    const long long nt = (M + KT - 1) / KT;
    const double* cc = w.st + ST_CUR + c * d;
    const double c0 = cc[0], c1 = d > 1 ? cc[1] : 0.0, c2 = d > 2 ? cc[2] : 0.0;
    for (long long tile = blockIdx.x; tile < nt; tile += gridDim.x) {
        const long long i = tile * KT + tid;
        double v = 0.0;
        if (i < M) {
            const double* p = packed + i * 4;
            if (p[3] == 1.0) {
                const double e = dsq(p[0], p[1], p[2], c0, c1, c2), D = first ? INFINITY : dist[i];
                v = e < D ? e : D;
            }
            dist[i] = v;
        }
        const double s = block_sum(v, red, tid);
        if (tid == 0) w.tsum[tile] = s;
    }
}

// one wave: the T candidates of round c
__global__ __launch_bounds__(64) void admpc_quad_kmeans_pick_kernel(long long M, int c, int T, uint64_t seed, uint32_t draw, const double* __restrict__ packed,
                                                                    const double* __restrict__ dist, double* __restrict__ work, const int32_t* __restrict__ info)
{
    if (info[2]) return;
    const Work w = work_of(work, M);
    const int lane = (int)threadIdx.x;
    const long long nt = (M + KT - 1) / KT;
    const double pot = w.st[ST_POT];
    const long long per = (nt + 63) / 64, lo = lane * per, hi = lo + per < nt ? lo + per : nt;
    double mine = 0.0;
    for (long long t = lo; t < hi; ++t) mine += w.tsum[t];
    const double incl = wave_scan(mine, lane), excl = __shfl_up(incl, 1);
    for (int t = 0; t < T; ++t) {
        uint32_t o[4];
        philox4x32_10((uint32_t)c, draw, (uint32_t)(t / 2), ADMPC_KMEANS_PHILOX_WORD, (uint32_t)seed, (uint32_t)(seed >> 32), o);
        const uint64_t wd = t % 2 ? (uint64_t)o[2] | (uint64_t)o[3] << 32 : (uint64_t)o[0] | (uint64_t)o[1] << 32;
        const double tau = (((double)(wd >> 11) + 0.5) * 0x1p-53) * pot;
        long long pickd = w.sti[ST_LAST];
        const unsigned long long reach = __ballot(lo < hi && incl >= tau);
        if (reach) {
            const int L = __ffsll((long long)reach) - 1;
            // lane L walks its tiles; if rounding hides the tile from the walk, the last of them is taken
            double before = lane == 0 ? 0.0 : excl;
            long long tt = hi - 1;
            if (lane == L) {
                double run = before;
                for (long long q = lo; q < hi; ++q) {
                    const double nx = run + w.tsum[q];
                    if (nx >= tau || q == hi - 1) { tt = q; before = run; break; }
                    run = nx;
                }
            }
            const long long tile = __shfl(tt, L);
            const double base = __shfl(before, L);
            // inside the tile: four consecutive records per lane
            const long long i0 = tile * KT + 4 * lane;
            double v[4], tot = 0.0;
            int f[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in = i0 + q < M;
                f[q] = in && packed[(i0 + q) * 4 + 3] == 1.0;
                v[q] = f[q] ? dist[i0 + q] : 0.0;
                tot += v[q];
            }
            const double li = wave_scan(tot, lane);
            const double up = __shfl_up(li, 1);               // by every lane: lane 1 reads lane 0, which a select around the shuffle would switch off
            double run = base + (lane == 0 ? 0.0 : up);
            int hit = -1, lastq = -1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                run += v[q];
                if (f[q] && run >= tau && hit < 0) hit = q;
                if (f[q]) lastq = q;
            }
            // if rounding hides the crossing inside the tile too, the tile's last counting record is next to it
            const unsigned long long who = __ballot(hit >= 0), have = __ballot(lastq >= 0);
            const long long found = __shfl((long long)(i0 + hit), who ? __ffsll((long long)who) - 1 : 0);
            const long long tail = __shfl((long long)(i0 + lastq), have ? 63 - __clzll((long long)have) : 0);
            if (who) pickd = found;
            else if (have) pickd = tail;
        }
        if (lane == 0) w.sti[t] = pickd;
    }
}

// labels under the current centres, and per cluster the count and the first moment about its centre.  FINAL: the pass behind the last
// iteration, which labels again unless the labels stood still (converged == 2), and whose sums give the inertia
template <int K, bool FINAL>
__global__ __launch_bounds__(KT) void admpc_quad_kmeans_assign_kernel(long long M, int d, const double* __restrict__ packed, int32_t* __restrict__ labels,
                                                                      double* __restrict__ work, const int32_t* __restrict__ info)
{
    __shared__ double cen[K * 3];
    __shared__ double red[4];
    const int conv = info[1];
    if (info[2] || (!FINAL && conv)) return;
    const Work w = work_of(work, M);
    const int tid = (int)threadIdx.x;
    if (tid < K * d) cen[tid] = w.st[ST_CUR + tid];
    __syncthreads();
    double acc[K][4], inertia = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[k][j] = 0.0;
    int changed = 0;
    const bool keep = FINAL && conv == 2;
    for (long long i = (long long)blockIdx.x * KT + tid; i < M; i += (long long)gridDim.x * KT) {
        const double* p = packed + i * 4;
        if (p[3] != 1.0) continue;
        const double z[3] = { p[0], p[1], p[2] };
        const int was = labels[i];
        const int c = keep ? was : quad_nearest(z, d, K, cen);
        if (!keep) { changed += c != was; labels[i] = c; }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double D0 = z[0] - cen[k * d], D1 = d > 1 ? z[1] - cen[k * d + 1] : 0.0, D2 = d > 2 ? z[2] - cen[k * d + 2] : 0.0;
            const bool in = c == k;
            acc[k][0] += in ? 1.0 : 0.0; acc[k][1] += in ? D0 : 0.0; acc[k][2] += in ? D1 : 0.0; acc[k][3] += in ? D2 : 0.0;
            inertia += in ? (D0 * D0 + D1 * D1) + D2 * D2 : 0.0;
        }
    }
    if (!FINAL) {
        for (int o = 32; o > 0; o >>= 1) changed += __shfl_xor(changed, o);
        if (tid % 64 == 0 && changed) atomicAdd(w.changed, changed);
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double v = block_sum(acc[k][j], red, tid);
            if (tid == 0) w.partial[(size_t)blockIdx.x * KPART + 4 * k + j] = v;
        }
    const double v = block_sum(inertia, red, tid);
    if (tid == 0) w.partial[(size_t)blockIdx.x * KPART + 4 * K] = v;
}

// one wave: every centre to the mean of its records, the shift, and scikit-learn's two stops in its order
__global__ __launch_bounds__(64) void admpc_quad_kmeans_move_kernel(long long M, int nblk, int K, int d, const double* __restrict__ cent, double* __restrict__ work,
                                                                    double* __restrict__ centers, int32_t* __restrict__ info)
{
    __shared__ double sum[64];
    if (info[1] | info[2]) return;
    const Work w = work_of(work, M);
    const int lane = (int)threadIdx.x, k = lane < K ? lane : 0;
    add_rows(w.partial, nblk, 4 * K + 1, lane, sum);
    const double N = sum[4 * k];
    const unsigned long long empty = __ballot(lane < K && !(N > 0.0));
    if (empty) { fail(-(__ffsll((long long)empty)), K * d, cent, centers, info, lane); return; }
    double sh = 0.0;
    if (lane < K) {
#pragma clang fp contract(off)
        double* c = w.st + ST_CUR + k * d;
        double df[3] = { 0.0, 0.0, 0.0 };
        for (int j = 0; j < d; ++j) {
            const double was = c[j], now = was + sum[4 * k + 1 + j] / N;
            df[j] = now - was;
            c[j] = now;
        }
        sh = (df[0] * df[0] + df[1] * df[1]) + df[2] * df[2];
    }
    double shift = 0.0;
    for (int q = 0; q < K; ++q) shift += __shfl(sh, q);
    if (lane == 0) {
        const int changed = w.changed[0];
        w.changed[0] = 0;
        w.st[ST_SHIFT] = shift;
        info[0] = info[0] + 1;
        info[1] = changed == 0 ? 2 : (shift <= w.st[ST_TOL] ? 1 : 0);
    }
}

__global__ __launch_bounds__(64) void admpc_quad_kmeans_end_kernel(long long M, int nblk, int K, int d, const double* __restrict__ cent, double* __restrict__ work,
                                                                   double* __restrict__ centers, double* __restrict__ stats, int32_t* __restrict__ info)
{
    __shared__ double sum[64];
    if (info[2]) return;
    const Work w = work_of(work, M);
    const int lane = (int)threadIdx.x, k = lane < K ? lane : 0;
    add_rows(w.partial, nblk, 4 * K + 1, lane, sum);
    const unsigned long long empty = __ballot(lane < K && !(sum[4 * k] > 0.0));
    if (empty) { fail(-(__ffsll((long long)empty)), K * d, cent, centers, info, lane); return; }
    if (lane < K * d) centers[lane] = w.st[ST_CUR + lane];
    if (lane == 0) { stats[0] = sum[4 * K]; stats[1] = w.st[ST_TOL]; stats[2] = w.st[ST_SHIFT]; stats[3] = w.st[ST_POT]; }
}

// one wave: scikit-learn's n_init rule.  kept [1]: the draw whose fit `best` holds, -1 while it holds none
__global__ __launch_bounds__(64) void admpc_quad_clusters_keep_kernel(int K, int draw, const double* __restrict__ gmm_try, const int32_t* __restrict__ info_try,
                                                                      double* __restrict__ gmm_best, int32_t* __restrict__ info_best, int32_t* __restrict__ kept)
{
    const int lane = (int)threadIdx.x;
    const int has = draw == 0 ? -1 : kept[0];
    const double lb = gmm_try[0], lb_best = gmm_best[0];
    const bool good = info_try[2] == 0 && isfinite(lb), take = good && (has < 0 || lb > lb_best);
    if (take || draw == 0) {
        for (int e = lane; e < (1 + K) * ADMPC_GMM_ROW; e += 64) gmm_best[e] = gmm_try[e];
        if (lane < 4) info_best[lane] = info_try[lane];
    }
    if (lane == 0) kept[0] = take ? draw : has;
}

// the k-means results of a try into those of the best where admpc_quad_clusters_keep_kernel has just kept that try's mixture (kept ==
// draw) or started a series (draw == 0)
__global__ __launch_bounds__(KT) void admpc_quad_kmeans_keep_kernel(long long M, int K, int d, int draw, const int32_t* __restrict__ kept,
                                                                    const double* __restrict__ centers_try, const int64_t* __restrict__ idx_try,
                                                                    const int32_t* __restrict__ labels_try, const double* __restrict__ stats_try,
                                                                    const int32_t* __restrict__ info_try, double* __restrict__ centers, int64_t* __restrict__ idx,
                                                                    int32_t* __restrict__ labels, double* __restrict__ stats, int32_t* __restrict__ info)
{
    if (draw != 0 && kept[0] != draw) return;
    const int tid = (int)threadIdx.x;
    for (long long i = (long long)blockIdx.x * KT + tid; i < M; i += (long long)gridDim.x * KT) labels[i] = labels_try[i];
    if (blockIdx.x == 0) {
        if (tid < K * d) centers[tid] = centers_try[tid];
        if (tid < K) idx[tid] = idx_try[tid];
        if (tid < 4) { stats[tid] = stats_try[tid]; info[tid] = info_try[tid]; }
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

// the grid of every kernel over the records: a function of M alone, the EM's
int km_blocks(long long M)
{
    const long long n = (M + KT - 1) / KT;
    return (int)(n < ADMPC_GMM_BLOCKS_MAX ? n : ADMPC_GMM_BLOCKS_MAX);
}

template <bool FINAL>
void assign_launch(int K, int nblk, long long M, int d, const double* packed, int32_t* labels, double* work, const int32_t* info, hipStream_t st)
{
#define A_CASE(k) case k: hipLaunchKernelGGL((admpc_quad_kmeans_assign_kernel<k, FINAL>), dim3(nblk), dim3(KT), 0, st, M, d, packed, labels, work, info); break;
    switch (K) { A_CASE(1) A_CASE(2) A_CASE(3) A_CASE(4) A_CASE(5) A_CASE(6) A_CASE(7) A_CASE(8) }
#undef A_CASE
}

}  // namespace

extern "C" {

int admpc_quad_kmeans_fit(const AdmpcQuadEnsemble* e, uint64_t seed, uint32_t draw, int max_iter, double tol, int64_t M, const double* records,
                          double* packed, double* dist, int32_t* labels, double* work, double* centers, int64_t* idx, double* stats,
                          int32_t* info, void* stream)
{
    const char* who = "admpc_quad_kmeans_fit";
    if (!e) return admpc_refuse(who, "null ensemble");
    QuadEnsembleView v;
    admpc_quad_ensemble_view(e, &v);
    for (int j = 0; j < v.n_feat; ++j)
        if (v.feat[j] < FEAT_LO) return admpc_refuse(who, "the clustering features must lie in [7, 16]: the sample record holds no others");
    if (max_iter < 1 || max_iter > 1000) return admpc_refuse(who, "max_iter must be in [1, 1000]");
    if (!(tol >= 0.0) || !isfinite(tol)) return admpc_refuse(who, "tol must be finite and not negative");
    if (M < 0) return admpc_refuse(who, "negative number of records");
    if (M == 0) return ADMPC_OK;
    if (!records || !packed || !dist || !labels || !work || !centers || !idx || !stats || !info) return admpc_refuse(who, "null array argument");
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    const int K = v.K, d = v.n_feat, nblk = km_blocks(M);
    const long long m = M, pblk = (m + KT - 1) / KT;
    int T = 2;                                          // 2 + int(ln K)
    if (K >= 3) T = 3;
    if (K >= 8) T = 4;
    hipLaunchKernelGGL(admpc_quad_gmm_pack_kernel, dim3((unsigned)(pblk < 65536 ? pblk : 65536)), dim3(KT), 0, st, m, d, v.feat[0], v.feat[1], v.feat[2],
                       records, packed);
    int rc = launched("admpc_quad_gmm_pack_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(admpc_quad_kmeans_prep_kernel, dim3(nblk), dim3(KT), 0, st, m, (const double*)packed, labels, work);
    if ((rc = launched("admpc_quad_kmeans_prep_kernel"))) return rc;
    hipLaunchKernelGGL(admpc_quad_kmeans_seed0_kernel, dim3(1), dim3(64), 0, st, m, nblk, K, d, seed, draw, tol, (const double*)packed, (const double*)v.cent, work,
                       centers, stats, info);
    if ((rc = launched("admpc_quad_kmeans_seed0_kernel"))) return rc;
    for (int c = 0; c < K; ++c) {
        const int first = c == 0, trials = first ? 1 : T;
        if (!first) {
            hipLaunchKernelGGL(admpc_quad_kmeans_pick_kernel, dim3(1), dim3(64), 0, st, m, c, trials, seed, draw, (const double*)packed, (const double*)dist, work,
                               (const int32_t*)info);
            if ((rc = launched("admpc_quad_kmeans_pick_kernel"))) return rc;
        }
        hipLaunchKernelGGL(admpc_quad_kmeans_cand_kernel, dim3(nblk), dim3(KT), 0, st, m, trials, first, (const double*)packed, (const double*)dist, work,
                           (const int32_t*)info);
        if ((rc = launched("admpc_quad_kmeans_cand_kernel"))) return rc;
        hipLaunchKernelGGL(admpc_quad_kmeans_finish_kernel, dim3(1), dim3(64), 0, st, m, nblk, K, d, c, trials, (const double*)packed, (const double*)v.cent, work,
                           centers, idx, info);
        if ((rc = launched("admpc_quad_kmeans_finish_kernel"))) return rc;
        if (c + 1 < K) {
            hipLaunchKernelGGL(admpc_quad_kmeans_update_kernel, dim3(nblk), dim3(KT), 0, st, m, d, c, first, (const double*)packed, dist, work, (const int32_t*)info);
            if ((rc = launched("admpc_quad_kmeans_update_kernel"))) return rc;
        }
    }
    for (int it = 0; it < max_iter; ++it) {
        assign_launch<false>(K, nblk, m, d, packed, labels, work, info, st);
        if ((rc = launched("admpc_quad_kmeans_assign_kernel"))) return rc;
        hipLaunchKernelGGL(admpc_quad_kmeans_move_kernel, dim3(1), dim3(64), 0, st, m, nblk, K, d, (const double*)v.cent, work, centers, info);
        if ((rc = launched("admpc_quad_kmeans_move_kernel"))) return rc;
    }
    assign_launch<true>(K, nblk, m, d, packed, labels, work, info, st);
    if ((rc = launched("admpc_quad_kmeans_assign_kernel"))) return rc;
    hipLaunchKernelGGL(admpc_quad_kmeans_end_kernel, dim3(1), dim3(64), 0, st, m, nblk, K, d, (const double*)v.cent, work, centers, stats, info);
    return launched("admpc_quad_kmeans_end_kernel");
}

int admpc_quad_clusters_keep(const AdmpcQuadEnsemble* e, int draw, const double* gmm_try, const int32_t* info_try, double* gmm_best, int32_t* info_best,
                             int32_t* kept, void* stream)
{
    const char* who = "admpc_quad_clusters_keep";
    if (!e) return admpc_refuse(who, "null ensemble");
    if (draw < 0) return admpc_refuse(who, "negative draw");
    if (!gmm_try || !info_try || !gmm_best || !info_best || !kept) return admpc_refuse(who, "null array argument");
    QuadEnsembleView v;
    admpc_quad_ensemble_view(e, &v);
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_quad_clusters_keep_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, v.K, draw, gmm_try, info_try, gmm_best, info_best, kept);
    return launched("admpc_quad_clusters_keep_kernel");
}

int admpc_quad_kmeans_keep(const AdmpcQuadEnsemble* e, int draw, int64_t M, const int32_t* kept, const double* centers_try, const int64_t* idx_try,
                           const int32_t* labels_try, const double* stats_try, const int32_t* info_try, double* centers, int64_t* idx,
                           int32_t* labels, double* stats, int32_t* info, void* stream)
{
    const char* who = "admpc_quad_kmeans_keep";
    if (!e) return admpc_refuse(who, "null ensemble");
    if (draw < 0) return admpc_refuse(who, "negative draw");
    if (M < 0) return admpc_refuse(who, "negative number of records");
    if (M == 0) return ADMPC_OK;
    if (!kept || !centers_try || !idx_try || !labels_try || !stats_try || !info_try || !centers || !idx || !labels || !stats || !info)
        return admpc_refuse(who, "null array argument");
    QuadEnsembleView v;
    admpc_quad_ensemble_view(e, &v);
    DeviceGuard guard(v.device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    hipLaunchKernelGGL(admpc_quad_kmeans_keep_kernel, dim3(km_blocks(M)), dim3(KT), 0, (hipStream_t)stream, (long long)M, v.K, v.n_feat, draw, kept, centers_try,
                       idx_try, labels_try, stats_try, info_try, centers, idx, labels, stats, info);
    return launched("admpc_quad_kmeans_keep_kernel");
}

}  // extern "C"
