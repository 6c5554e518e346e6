// gp_search_dev.h -- the bodies of the hyperparameter search (include/admpc_hyper.h: admpc_gp_search, admpc_gp_refit), shared by the kernels
// that take their regressors and search descriptors BY VALUE (admpc_hyper.hip: one handle, at most ADMPC_GP_MAX regressors) and the ones
// that take them BY POINTER (admpc_quad_hyper.hip: the K * n_gp regressors of a clustered ensemble in one launch, which no longer fit the
// kernel arguments); and the declarations of the search's host side that admpc_hyper.hip defines for both vehicles and for the ensemble.
// Include at file scope behind gp_fit_dev.h, whose conventions hold (the translation unit includes model_dev.h in its anonymous namespace).
//
//   init   gp_search_init_body  lane 0 of a wave: centre and step as the host formed them, v = exp(centre), best = +inf
//   nll    gp_nll_body          a candidate per HALF wave, 8 candidates per block of 4 waves.  The points of the regressor are formed once
//                               per block (gp_fit_dev.h: gp_points, as the fit forms them) and shared in LDS; each half wave keeps its own
//                               K as a PACKED lower triangle (row r at r (r + 1) / 2: 528 doubles, 4224 bytes; the triangular numbers are
//                               distinct mod 32, so the 32 rows start on 32 different 8-byte banks and a column is read without a conflict)
//                               -- 35 KB a block, four blocks a CU.  The Cholesky is the fit's, a column per step, the pivot passed within
//                               the half by a lane read of width 32.  A half whose pivot fails is MASKED: it goes on through every barrier
//                               and reports +inf at the end.  A block past the regressor's last candidate returns in front of every barrier.
//   pick   gp_pick_body         a wave: the lowest index of the minimum, the new centre by the NLL body's own decoding of it
//                               (search_candidate), the step shrunk
//   refit  gp_refit_body        the fit's body (gp_fit_dev.h) at the natural values the search left in `hyper`
#pragma once
#include "gp_fit_dev.h"

#define NLL_WAVES 4                          // waves per block of the NLL kernel
#define NLL_CAND (2 * NLL_WAVES)             // candidates per block: one per half wave
#define TRI (NPT * (NPT + 1) / 2)            // doubles of a packed lower triangle
#define NSLOT 5                              // length[0 .. 2], sigma_f, noise
#define HYP ADMPC_GP_HYPER

static_assert(HYP == 3 * NSLOT + 1, "centre, step and natural value per slot, and the best NLL");
static_assert(NLL_CAND * TRI * 8 + 6 * NPT * 8 <= 80 * 1024, "two blocks of the NLL kernel fit the LDS of a CU");

// the search of one regressor as the kernels read it: 184 bytes
struct SearchGp {
    int C, free_[NSLOT];                     // candidates per round; which slots are searched
    double loglo[NSLOT], loghi[NSLOT];       // the box in log units (0 for a slot that is not used)
    double centre0[NSLOT], step0[NSLOT];     // the start, for resume == 0
};

// admpc_hyper.hip: the host side that the search of both vehicles shares (`who` leads a message).  The refusals of a search block behind
// those of its observe parameters -- sp null, grid, rounds, shrink, per regressor a bad used slot, then a candidate count above
// ADMPC_GP_SEARCH_MAX -- with the descriptors s [n_gp] formed on the way, in double, and the largest candidate count; the two entries
// behind the check of their parameter block, which launch the kernels of admpc_hyper.hip for either vehicle (an unused feature slot names
// `unused_feat`): a __global__ function is launched from the unit that defines it.
ADMPC_HIDDEN int admpc_hyper_form(const char* who, int n_gp, const AdmpcGpBins* gp, const AdmpcGpSearchParams* sp, SearchGp* s, int* cmax);
ADMPC_HIDDEN int admpc_hyper_search(const char* who, int device, int n_gp, const AdmpcGpBins* gp, int unused_feat, const AdmpcGpSearchParams* sp,
                                    int min_count, int resume, const double* bins, double* hyper, double* nll, int32_t* search_info, void* stream);
ADMPC_HIDDEN int admpc_hyper_refit(const char* who, int device, int n_gp, const AdmpcGpBins* gp, int unused_feat, int min_count, const double* bins,
                                   const double* hyper, AdmpcGp* gp_out, int32_t* info, void* stream);

// Candidate c of a round around the centre hy[0 .. 4] with the steps hy[5 .. 9]: theta and v = exp(theta) of the five slots.  The NLL
// body and the pick body both decode a candidate by this function, every operation of theta rounded on its own.
static __device__ __forceinline__ void search_candidate(const SearchGp& S, const int grid, const int half, const double* hy, const int c,
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

// one wave; lane 0 writes the 16 doubles of the regressor at hy
static __device__ __forceinline__ void gp_search_init_body(const SearchGp& S, double* hy)
{
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int d = 0; d < NSLOT; ++d) {
        const double c = S.centre0[d];
        hy[d] = c;
        hy[NSLOT + d] = S.step0[d];
        hy[2 * NSLOT + d] = exp(c);
    }
    hy[3 * NSLOT] = INFINITY;
}

// A block of 4 waves: candidate 8 * blockIdx.x + 2 * wave + half of regressor g of a, searched as S says around the state hy [HYP]; its
// NLL goes to nll [ADMPC_GP_SEARCH_MAX], the regressor's own row.
static __device__ __forceinline__ void gp_nll_body(const LearnArgs& a, const int g, const SearchGp& S, const int grid, const int half,
                                                   const double* hy, double* nll)
{
    __shared__ double Zs[3][NPT], ts[NPT], cs[NPT], As[NLL_CAND][TRI];
    __shared__ int ns;
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
    search_candidate(S, grid, half, hy, live ? c : 0, th, v);
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
    if (live && r == 0) nll[c] = val;
}

// one wave: the pick over x [S.C], the NLLs of the round, into the state hy [HYP] and info [2]
static __device__ __forceinline__ void gp_pick_body(const SearchGp& S, const int grid, const int half, const double shrink, double* hy,
                                                    const double* x, int32_t* info)
{
    const int lane = gp_lane_id();
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
    search_candidate(S, grid, half, hy, at, th, v);
    const bool better = best < hy[3 * NSLOT];
    double step[NSLOT];
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int d = 0; d < NSLOT; ++d) step[d] = hy[NSLOT + d] * shrink;
    }
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < NSLOT; ++d) {
            if (better) { hy[d] = th[d]; hy[2 * NSLOT + d] = v[d]; }
            hy[NSLOT + d] = step[d];
        }
        if (better) hy[3 * NSLOT] = best;
        info[0] = better ? at : -1;
        info[1] = finite;
    }
}

// one wave: the fit of regressor g of a at the natural values of the search's centre, hy [HYP]
// the natural values a search left in hy [HYP] as the fit takes its hyperparameters (the re-fit and the factor of the evaluation,
// admpc_quad_eval.hip, read them here)
static __device__ __forceinline__ GpHyper gp_hyper_natural(const int nf, const double* __restrict__ hy)
{
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
    return h;
}

static __device__ __forceinline__ void gp_refit_body(const LearnArgs& a, const int g, const double* __restrict__ hy)
{
    gp_fit_body(a, g, gp_hyper_natural(a.gp[g].n_feat, hy));
}
