// admpc_hyper.hip -- searching the hyperparameters of a handle's residual GP on the device (include/admpc_hyper.h): a zooming grid
// search of the negative log marginal likelihood (NLL) of a regressor's points, and the fit at the optimum.
//
//   init   admpc_gp_search_init_kernel  a block per regressor: centre and step as the host formed them, v = exp(centre), best = +inf
//   nll    admpc_gp_nll_kernel          a candidate per HALF wave, 8 candidates per block of 4 waves.  The points of the regressor are
//                                       formed once per block (gp_fit_dev.h: gp_points, as the fit forms them) and shared in LDS; each half
//                                       wave keeps its own K as a PACKED lower triangle (row r at r (r + 1) / 2: 528 doubles, 4224 bytes;
//                                       the triangular numbers are distinct mod 32, so the 32 rows start on 32 different 8-byte banks and
//                                       a column is read without a conflict) -- 35 KB a block, four blocks a CU.  The Cholesky is the
//                                       fit's, a column per step, the pivot passed within the half by a lane read of width 32.  A half
//                                       whose pivot fails is MASKED: it goes on through every barrier and reports +inf at the end.
//   pick   admpc_gp_pick_kernel         a wave per regressor: the lowest index of the minimum, the new centre by the NLL kernel's own
//                                       decoding of it (search_candidate), the step shrunk
//   refit  admpc_gp_refit_kernel        the fit's body (gp_fit_dev.h) at the natural values the search left in `hyper`
#include <stdio.h>
#include <math.h>
#include "admpc_host.h"
#include "../../include/admpc_hyper.h"

#define NX ADMPC_NX
#define NU ADMPC_NU
#define NY ADMPC_NY
#include "gp_fit_dev.h"
#define NLL_WAVES 4                          // waves per block of the NLL kernel
#define NLL_CAND (2 * NLL_WAVES)             // candidates per block: one per half wave
#define TRI (NPT * (NPT + 1) / 2)            // doubles of a packed lower triangle
#define NSLOT 5                              // length[0 .. 2], sigma_f, noise
#define HYP ADMPC_GP_HYPER

static_assert(HYP == 3 * NSLOT + 1, "centre, step and natural value per slot, and the best NLL");
static_assert(NLL_CAND * TRI * 8 + 6 * NPT * 8 <= 80 * 1024, "two blocks of the NLL kernel fit the LDS of a CU");

// the search of one regressor as the kernels read it (passed by value)
struct SearchGp {
    int C, free_[NSLOT];                     // candidates per round; which slots are searched
    double loglo[NSLOT], loghi[NSLOT];       // the box in log units (0 for a slot that is not used)
    double centre0[NSLOT], step0[NSLOT];     // the start, for resume == 0
};

struct SearchArgs {
    int grid, half;                          // half = (grid - 1) / 2
    double shrink;
    SearchGp s[ADMPC_GP_MAX];
    double* hyper;                           // [n_gp][HYP]
    double* nll;                             // [n_gp][ADMPC_GP_SEARCH_MAX]
    int32_t* info;                           // [n_gp][2]
};

namespace {

#include "model_dev.h"

// Candidate c of a round around the centre hy[0 .. 4] with the steps hy[5 .. 9]: theta and v = exp(theta) of the five slots.  The NLL
// kernel and the pick kernel both decode a candidate by this function, every operation of theta rounded on its own.
__device__ __forceinline__ void search_candidate(const SearchGp& S, const int grid, const int half, const double* hy, const int c,
                                                 double (&th)[NSLOT], double (&v)[NSLOT])
{
#pragma clang fp contract(off)
    int rem = c;
#pragma unroll
    for (int d = NSLOT - 1; d >= 0; --d) {                  // the last free slot is the fastest digit
        double t = hy[d];
        if (S.free_[d]) {
            const int digit = rem % grid;
            rem = rem / grid;
            const double off = (double)(digit - half) * hy[NSLOT + d];
            t = fmin(fmax(t + off, S.loglo[d]), S.loghi[d]);
        }
        th[d] = t;
        v[d] = exp(t);
    }
}

}  // namespace

// grid n_gp, one wave each; lane 0 writes the 16 doubles of the regressor
__global__ __launch_bounds__(WAVE) void admpc_gp_search_init_kernel(const SearchArgs q)
{
    const int g = (int)blockIdx.x;
    const SearchGp& S = q.s[g];
    if (threadIdx.x != 0) return;
    double* hy = q.hyper + (long)g * HYP;
#pragma unroll
    for (int d = 0; d < NSLOT; ++d) {
        const double c = S.centre0[d];
        hy[d] = c;
        hy[NSLOT + d] = S.step0[d];
        hy[2 * NSLOT + d] = exp(c);
    }
    hy[3 * NSLOT] = INFINITY;
}

// grid (ceil(max C_g / 8), n_gp), 4 waves each: candidate 8 * blockIdx.x + 2 * wave + half of regressor blockIdx.y.
__global__ __launch_bounds__(NLL_WAVES * WAVE) void admpc_gp_nll_kernel(const LearnArgs a, const SearchArgs q)
{
    __shared__ double Zs[3][NPT], ts[NPT], cs[NPT], As[NLL_CAND][TRI];
    __shared__ int ns;
    const int g = (int)blockIdx.y;
    const SearchGp& S = q.s[g];
    const LearnGp& G = a.gp[g];
    const int c0 = (int)blockIdx.x * NLL_CAND;
    if (c0 >= S.C) return;                                 // uniform over the block, in front of every barrier: a regressor with fewer candidates
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & (WAVE - 1), r = lane & (NPT - 1);
    const int slot = 2 * wave + (lane >> 5), c = c0 + slot;
    const bool live = c < S.C;                             // a half past the last candidate works on candidate 0 and stores nothing
    if (wave == 0) {
        const int n0 = gp_points(a, g, lane, Zs, ts, cs);
        if (lane == 0) ns = n0;
    }
    __syncthreads();
    const int n = ns, nf = G.n_feat;
    const double ymean = gp_ymean(ts, n);
    double th[NSLOT], v[NSLOT];
    search_candidate(S, q.grid, q.half, q.hyper + (long)g * HYP, live ? c : 0, th, v);
    double il0, il1, il2;
    {
#pragma clang fp contract(off)
        il0 = 1.0 / (v[0] * v[0]);
        il1 = nf > 1 ? 1.0 / (v[1] * v[1]) : 0.0;
        il2 = nf > 2 ? 1.0 / (v[2] * v[2]) : 0.0;
    }
    const double sf = v[3];
    double* A = As[slot];
    const int row = r * (r + 1) / 2;
    // row r of K, packed
    const double z0 = Zs[0][r], z1 = Zs[1][r], z2 = Zs[2][r];
    const double diag = v[4] + G.count_noise / cs[r];
    if (r < n) {
#pragma unroll 1
        for (int j = 0; j <= r; ++j) {
            const double e0 = z0 - Zs[0][j], e1 = z1 - Zs[1][j], e2 = z2 - Zs[2][j];
            A[row + j] = sf * exp_nonpos(-0.5 * (e0 * e0 * il0 + e1 * e1 * il1 + e2 * e2 * il2)) + (j == r ? diag : 0.0);
        }
    }
    __syncthreads();
    // the Cholesky of the fit.  n is uniform over the block, so every half reaches every barrier; a failed half computes on, masked.
    bool dead = false;
    double lown = 1.0;                                     // L[r][r]
#pragma unroll 1
    for (int k = 0; k < n; ++k) {
        const int rowk = k * (k + 1) / 2;
        double s = 0.0;
        if (r >= k && r < n) {
            s = A[row + k];
#pragma unroll 1
            for (int j = 0; j < k; ++j) s = s - A[row + j] * A[rowk + j];
        }
        const double d = __shfl(s, k, NPT), tk = ts[k];   // lane k of this half
        dead = dead || !(d > 0.0 && isfinite(d) && isfinite(tk));
        const double l = sqrt(d);
        if (r >= k && r < n) A[row + k] = r == k ? l : s / l;
        if (r == k) lown = l;
        __syncthreads();
    }
    double bb = r < n ? ts[r] - ymean : 0.0;
#pragma unroll 1
    for (int k = 0; k < n; ++k) {                          // L w = t - ymean
        const double wk = __shfl(bb, k, NPT) / A[k * (k + 1) / 2 + k];
        if (r == k) bb = wk;
        else if (r > k && r < n) bb = bb - A[row + k] * wk;
    }
    double part = r < n ? log(lown) + 0.5 * bb * bb : 0.0;
#pragma unroll
    for (int w = NPT / 2; w > 0; w >>= 1) part += __shfl_xor(part, w);     // stays inside the half
    const double val = dead ? INFINITY : part + 0.5 * (double)n * 1.8378770664093454836;      // log(2 pi)
    if (live && r == 0) q.nll[(long)g * ADMPC_GP_SEARCH_MAX + c] = val;
}

// grid n_gp, one wave each
__global__ __launch_bounds__(WAVE) void admpc_gp_pick_kernel(const SearchArgs q)
{
    const int g = (int)blockIdx.x, lane = gp_lane_id();
    const SearchGp& S = q.s[g];
    const double* x = q.nll + (long)g * ADMPC_GP_SEARCH_MAX;
    double* hy = q.hyper + (long)g * HYP;
    double best = INFINITY;
    int at = lane < S.C ? lane : 0x7fffffff, finite = 0;
    for (int c = lane; c < S.C; c += WAVE) {
        const double y = x[c];
        const bool f = isfinite(y);                        // NaN and +-inf count as +inf
        finite += f ? 1 : 0;
        if (f && y < best) { best = y; at = c; }
    }
#pragma unroll
    for (int w = WAVE / 2; w > 0; w >>= 1) {
        const double ob = __shfl_xor(best, w);
        const int oa = __shfl_xor(at, w);
        finite += __shfl_xor(finite, w);
        if (ob < best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    double th[NSLOT], v[NSLOT];
    search_candidate(S, q.grid, q.half, hy, at, th, v);
    const bool better = best < hy[3 * NSLOT];
    double step[NSLOT];
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int d = 0; d < NSLOT; ++d) step[d] = hy[NSLOT + d] * q.shrink;
    }
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < NSLOT; ++d) {
            if (better) { hy[d] = th[d]; hy[2 * NSLOT + d] = v[d]; }
            hy[NSLOT + d] = step[d];
        }
        if (better) hy[3 * NSLOT] = best;
        q.info[2 * g] = better ? at : -1;
        q.info[2 * g + 1] = finite;
    }
}

// grid n_gp, one wave each: the fit at the natural values of the search's centre
__global__ __launch_bounds__(WAVE) void admpc_gp_refit_kernel(const LearnArgs a, const double* __restrict__ hyper)
{
    const int g = (int)blockIdx.x, nf = a.gp[g].n_feat;
    const double* hy = hyper + (long)g * HYP;
    GpHyper h;
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double l = hy[2 * NSLOT + d];
            h.inv_l2[d] = d < nf ? 1.0 / (l * l) : 0.0;
        }
    }
    h.sigma_f = hy[2 * NSLOT + 3];
    h.noise = hy[2 * NSLOT + 4];
    h.no_optimum = isfinite(hy[3 * NSLOT]) ? 0 : 1;
    gp_fit_body(a, g, h);
}

namespace {

int refuse(const char* what)
{
    char msg[200];
    snprintf(msg, sizeof msg, "admpc_gp_search: %s", what);
    return admpc_set_error(ADMPC_EINVAL, msg);
}

}  // namespace

extern "C" {

int admpc_gp_search(int device, const AdmpcObserveParams* obs, const AdmpcGpSearchParams* sp, int min_count, int resume,
                    const double* bins, double* hyper, double* nll, int32_t* search_info, void* stream)
{
    const int rc = admpc_observe_params_check("admpc_gp_search", obs);
    if (rc) return rc;
    if (!sp) return refuse("the search parameters are not set");
    if (sp->grid != 3 && sp->grid != 5 && sp->grid != 7 && sp->grid != 9) return refuse("grid must be 3, 5, 7 or 9");
    if (sp->rounds < 1 || sp->rounds > 64) return refuse("rounds must be in [1, 64]");
    if (!(sp->shrink > 0.0 && sp->shrink < 1.0)) return refuse("shrink must be in (0, 1)");
    SearchArgs q = SearchArgs();
    q.grid = sp->grid; q.half = (sp->grid - 1) / 2; q.shrink = sp->shrink;
    int cmax = 1;
    for (int g = 0; g < obs->n_gp; ++g) {
        const AdmpcGpSearchBox& b = sp->box[g];
        SearchGp& S = q.s[g];
        char what[120];
        for (int d = 0; d < NSLOT; ++d) {
            if (d < 3 && d >= obs->gp[g].n_feat) continue;             // the slot of an unused feature is not read: theta 0, step 0, v 1
            if (!(b.lo[d] > 0.0) || !(b.hi[d] >= b.lo[d]) || !isfinite(b.lo[d]) || !isfinite(b.hi[d])) {
                snprintf(what, sizeof what, "regressor %d: slot %d of the box needs 0 < lo <= hi, finite", g, d);
                return refuse(what);
            }
            S.free_[d] = b.hi[d] != b.lo[d];
            S.loglo[d] = log(b.lo[d]); S.loghi[d] = log(b.hi[d]);
            S.centre0[d] = 0.5 * (S.loglo[d] + S.loghi[d]);
            S.step0[d] = S.free_[d] ? (S.loghi[d] - S.loglo[d]) / (double)(sp->grid - 1) : 0.0;
        }
    }
    for (int g = 0; g < obs->n_gp; ++g) {
        SearchGp& S = q.s[g];
        char what[120];
        long C = 1;
        for (int d = 0; d < NSLOT; ++d) if (S.free_[d]) C *= sp->grid;
        if (C > ADMPC_GP_SEARCH_MAX) {
            snprintf(what, sizeof what, "regressor %d: %ld candidates per round, at most %d (fix a slot or take a smaller grid)", g, C, ADMPC_GP_SEARCH_MAX);
            return refuse(what);
        }
        S.C = (int)C;
        if (S.C > cmax) cmax = S.C;
    }
    if (min_count < 1) return refuse("min_count must be at least 1");
    if (resume != 0 && resume != 1) return refuse("resume must be 0 or 1");
    if (!bins || !hyper || !nll || !search_info) return refuse("null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    LearnArgs l = LearnArgs();
    admpc_learn_fill(l, obs->n_gp, obs->gp, CAR_LEARN.feat_lo);
    l.min_count = (double)min_count; l.bins = const_cast<double*>(bins);
    q.hyper = hyper; q.nll = nll; q.info = search_info;
    const dim3 one((unsigned)obs->n_gp), cand((unsigned)((cmax + NLL_CAND - 1) / NLL_CAND), (unsigned)obs->n_gp);
    if (!resume) {
        hipLaunchKernelGGL(admpc_gp_search_init_kernel, one, dim3(WAVE), 0, (hipStream_t)stream, q);
        if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_gp_search_init_kernel: launch failed");
    }
    for (int it = 0; it < sp->rounds; ++it) {
        hipLaunchKernelGGL(admpc_gp_nll_kernel, cand, dim3(NLL_WAVES * WAVE), 0, (hipStream_t)stream, l, q);
        if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_gp_nll_kernel: launch failed");
        hipLaunchKernelGGL(admpc_gp_pick_kernel, one, dim3(WAVE), 0, (hipStream_t)stream, q);
        if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_gp_pick_kernel: launch failed");
    }
    return ADMPC_OK;
}

int admpc_gp_refit(int device, const AdmpcObserveParams* obs, int min_count, const double* bins, const double* hyper,
                   AdmpcGp* gp_out, int32_t* info, void* stream)
{
    const int rc = admpc_observe_params_check("admpc_gp_refit", obs);
    if (rc) return rc;
    if (min_count < 1) return admpc_set_error(ADMPC_EINVAL, "admpc_gp_refit: min_count must be at least 1");
    if (!bins || !hyper || !gp_out || !info) return admpc_set_error(ADMPC_EINVAL, "admpc_gp_refit: null array argument");
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    LearnArgs l = LearnArgs();
    admpc_learn_fill(l, obs->n_gp, obs->gp, CAR_LEARN.feat_lo);
    l.min_count = (double)min_count; l.bins = const_cast<double*>(bins); l.out = gp_out; l.info = info;
    hipLaunchKernelGGL(admpc_gp_refit_kernel, dim3((unsigned)obs->n_gp), dim3(WAVE), 0, (hipStream_t)stream, l, hyper);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_gp_refit_kernel: launch failed");
    return ADMPC_OK;
}

}  // extern "C"
