// gp_fit_dev.h -- the body of the GP fit (include/admpc_learn.h: admpc_gp_fit), shared by the kernel that fits at the hyperparameters
// GIVEN to it (admpc_learn.hip) and the one that fits at the hyperparameters a search has found (admpc_hyper.hip: admpc_gp_refit), and
// the formation of a regressor's points from its bins, which the search's NLL kernel shares with both; the bodies of the bin kernel and
// of the install kernel, which the car (admpc_learn.hip) and the quadrotor (admpc_quad_learn.hip) share; and the declarations of the
// learning host side that admpc_learn.hip defines for the quadrotor and the search (they speak of LearnArgs, which admpc_host.h does
// not know).  Include at file scope behind admpc_host.h; the translation unit includes model_dev.h in its anonymous namespace
// (exp_nonpos, declared below).  NPT, ACC and WAVE are defined here.
#pragma once
#include "../../include/admpc_hyper.h"
#include "../../include/admpc_quad.h"

namespace { __device__ __forceinline__ double exp_nonpos(const double x); }      // model_dev.h

#define WAVE 64
#define NPT ADMPC_GP_MAX_POINTS
#define ACC 5            // doubles per bin
#define GP_WORDS (sizeof(AdmpcGp) / 8)

static_assert(NPT == 32, "the fit maps one row to each lane of half a wave");
static_assert(sizeof(AdmpcGp) % 8 == 0 && offsetof(AdmpcConfig, gp) % 8 == 0 && offsetof(AdmpcQuadConfig, gp) % 8 == 0,
              "the install copies an AdmpcGp in 8-byte words");

// one regressor as the bin kernel and the fit kernel read it
struct LearnGp {
    int n_feat, feat[3], out, nb[3], nbins;
    double lo[3], scale[3];      // scale_d = nb_d / (hi_d - lo_d)
    double sigma_f, inv_l2[3], noise, count_noise;
};

struct LearnArgs {
    int B, n_gp;
    double min_count;
    LearnGp gp[ADMPC_GP_MAX];
    const double* samples;       // [B][REC] of the vehicle: 10 doubles a record for the car, 14 for the quadrotor
    double* bins;                // [n_gp][NPT][ACC]
    int32_t* dropped;            // [ADMPC_GP_MAX + 1]; the quadrotor: [ADMPC_QUAD_GP_MAX + 1]
    AdmpcGp* out;                // [n_gp]
    int32_t* info;               // [n_gp]
};

// what differs between the vehicles in a regressor to learn: how many a handle holds, the feature indices and the output rows it may name
struct LearnRanges { int n_gp_max, feat_lo, feat_hi, out_lo, out_hi; };
constexpr LearnRanges CAR_LEARN = { ADMPC_GP_MAX, 3, 8, 3, 5 }, QUAD_LEARN = { ADMPC_QUAD_GP_MAX, 7, ADMPC_QUAD_NY - 1, 7, 9 };
static_assert(ADMPC_QUAD_GP_MAX <= ADMPC_GP_MAX, "LearnArgs holds the regressors of either vehicle");

// admpc_learn.hip: the host side that the learning of both vehicles shares (`who` leads a message).  A refusal under the caller's name;
// the refusals of a parameter block's regressors, behind those of its head, which is the vehicle's own; the regressors as the kernels read
// them (an unused feature slot names `unused_feat`); and the fit entry behind the check of its parameter block, which launches
// admpc_gp_fit_kernel for either vehicle: a __global__ function is launched from the unit that defines it.
ADMPC_HIDDEN int admpc_learn_refuse(const char* who, const char* what);
ADMPC_HIDDEN int admpc_learn_regressors_check(const char* who, int n_gp, const AdmpcGpBins* gp, const LearnRanges& r);
ADMPC_HIDDEN void admpc_learn_fill(LearnArgs& a, int n_gp, const AdmpcGpBins* gp, int unused_feat);
ADMPC_HIDDEN int admpc_learn_fit(const char* who, int device, int n_gp, const AdmpcGpBins* gp, int unused_feat, int min_count, const double* bins,
                                 AdmpcGp* gp_out, int32_t* info, void* stream);

// where a fit takes its hyperparameters from: the regressor's own (given), or the natural values a search left in device memory
struct GpHyper {
    double sigma_f, inv_l2[3], noise;
    int no_optimum;              // the search found no finite NLL: the empty GP, info ADMPC_GP_NO_OPTIMUM (0 for a fit at given values)
};

static __device__ __forceinline__ int gp_lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// The points of regressor g, by ONE wave: the bins with enough samples, in ascending order, into Zs [3][NPT], ts, cs (LDS); the rows
// past the last point are filled with zeros and a count of 1.  Returns n, the same on every lane.  Lane r < 32 reads bin r.
static __device__ __forceinline__ int gp_points(const LearnArgs& a, const int g, const int lane, double (*Zs)[NPT], double* ts, double* cs)
{
    const LearnGp& G = a.gp[g];
    const int r = lane & (NPT - 1), nf = G.n_feat;
    const bool act = lane < NPT;
    const double* bn = a.bins + ((long)g * NPT + r) * ACC;
    double cnt = 0.0;
    bool ok = false;
    if (act && r < G.nbins) { cnt = bn[0]; ok = cnt >= a.min_count; }
    const unsigned long long m = __ballot(ok);
    const int n = __popcll(m), pos = __popcll(m & ((1ull << lane) - 1ull));
    if (ok) {
#pragma clang fp contract(off)
#pragma unroll
        for (int d = 0; d < 3; ++d) Zs[d][pos] = d < nf ? bn[1 + d] / cnt : 0.0;
        ts[pos] = bn[4] / cnt;
        cs[pos] = cnt;
    }
    if (act && r >= n) { Zs[0][r] = 0.0; Zs[1][r] = 0.0; Zs[2][r] = 0.0; ts[r] = 0.0; cs[r] = 1.0; }
    return n;
}

// the serial sum of the targets, divided by n; every operation rounded on its own
static __device__ __forceinline__ double gp_ymean(const double* ts, const int n)
{
#pragma clang fp contract(off)
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum = sum + ts[i];
    return n > 0 ? sum / (double)n : 0.0;
}

// The statistics of bin `bin` of regressor g, by ONE wave (a block of its own; include/admpc_learn.h, admpc_bin_kernel, has the contract:
// acceptance, the bin index, the lane-ordered sums).  The record layout is the caller's: REC_ doubles, the last of them the flag; feature
// index f reads entry f - FEAT0_, output `out` reads entry Y0_ + out - FEAT0_; the records that are not valid go into dropped[INVALID_].
// Bin 0 of a regressor also counts what fell outside its box, regressor 0 also what was not valid.
// `takes` is the routing predicate of a clustered ensemble (admpc_quad_ensemble.hip): a valid record it does not take is absent to this
// wave -- not added, not counted as dropped -- and keeps its lane; the wave tallies the records that are not valid only if the predicate
// says so.  The default takes every record, and the kernels that use it are what they were without it.
struct GpBinTakesAll {
    __device__ __forceinline__ constexpr bool operator()(const double*) const { return true; }
    __device__ __forceinline__ constexpr bool tallies_invalid() const { return true; }
};
template <int REC_, int FEAT0_, int Y0_, int INVALID_, class Takes_ = GpBinTakesAll>
static __device__ __forceinline__ void gp_bin_body(const LearnArgs& a, const int g, const int bin, const Takes_ takes = Takes_())
{
#pragma clang fp contract(off)
    const LearnGp& G = a.gp[g];
    if (bin >= G.nbins) return;
    const int lane = gp_lane_id();
    double part[ACC] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    int outside = 0, invalid = 0;
    for (long b = lane; b < a.B; b += WAVE) {
        const double* r = a.samples + b * REC_;
        if (!(r[REC_ - 1] == 1.0)) { ++invalid; continue; }
        if (!takes(r)) continue;
        double z[3] = { 0.0, 0.0, 0.0 };
        bool in = true;
        int k = 0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (d < G.n_feat) {
                z[d] = r[G.feat[d] - FEAT0_];
                const double t = (z[d] - G.lo[d]) * G.scale[d];
                const double kd = floor(t);
                const bool ok = t >= 0.0 && kd < (double)G.nb[d];
                in = in && ok;
                k = k * G.nb[d] + (ok ? (int)kd : 0);
            }
        }
        if (!in) { ++outside; continue; }
        if (k == bin) {
            part[0] = part[0] + 1.0;
            part[1] = part[1] + z[0]; part[2] = part[2] + z[1]; part[3] = part[3] + z[2];
            part[4] = part[4] + r[Y0_ + G.out - FEAT0_];
        }
    }
    double* o = a.bins + ((long)g * NPT + bin) * ACC;
    double acc[ACC];
#pragma unroll
    for (int c = 0; c < ACC; ++c) acc[c] = o[c];
    for (int l = 0; l < WAVE; ++l) {
#pragma unroll
        for (int c = 0; c < ACC; ++c) acc[c] = acc[c] + __shfl(part[c], l);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < ACC; ++c) o[c] = acc[c];
    }
    if (bin == 0) {
        for (int w = WAVE / 2; w > 0; w >>= 1) { outside += __shfl_xor(outside, w); invalid += __shfl_xor(invalid, w); }
        if (lane == 0) {
            a.dropped[g] = a.dropped[g] + outside;
            if (g == 0 && takes.tallies_invalid()) a.dropped[INVALID_] = a.dropped[INVALID_] + invalid;
        }
    }
}

// One wave installs src [n_gp] as dst [0 .. n_gp), the GPs of a handle's device configuration; a record that fails the check (the
// vehicle's ranges of a feature index and of the output row, the counts, every number finite) is replaced by the empty GP.
template <int FEAT_LO_, int FEAT_HI_, int OUT_LO_, int OUT_HI_>
static __device__ __forceinline__ void gp_install_body(AdmpcGp* dst, const int n_gp, const AdmpcGp* src, int32_t* installed)
{
    const int lane = gp_lane_id();
    for (int g = 0; g < n_gp; ++g) {
        const AdmpcGp* s = src + g;
        const int nf = s->n_feat, n = s->n_points, out = s->out;
        bool head = nf >= 1 && nf <= ADMPC_GP_MAX_FEAT && out >= OUT_LO_ && out <= OUT_HI_ && n >= 0 && n <= NPT;
        head = head && isfinite(s->sigma_f) && isfinite(s->ymean);
#pragma unroll
        for (int d = 0; d < ADMPC_GP_MAX_FEAT; ++d)
            if (d < nf) head = head && s->feat[d] >= FEAT_LO_ && s->feat[d] <= FEAT_HI_ && isfinite(s->inv_l2[d]);
        bool bad = false;
        if (head && lane < n) {
            bad = !isfinite(s->alpha[lane]);
#pragma unroll
            for (int d = 0; d < ADMPC_GP_MAX_FEAT; ++d)
                if (d < nf) bad = bad || !isfinite(s->Z[d][lane]);
        }
        const bool take = head && __ballot(bad) == 0ull;
        const uint64_t* sw = (const uint64_t*)s;
        uint64_t* dw = (uint64_t*)(dst + g);
        for (int w = lane; w < (int)GP_WORDS; w += WAVE) {
            // the empty GP: n_feat 1, feat FEAT_LO_ 0 0, out OUT_LO_, n_points 0, every double zero (the six int32 of the head are words 0 .. 2)
            const uint64_t empty = w == 0 ? (1ull | ((uint64_t)FEAT_LO_ << 32)) : (w == 2 ? (uint64_t)OUT_LO_ : 0ull);
            dw[w] = take ? sw[w] : empty;
        }
        if (lane == 0) installed[g] = take ? 1 : 0;
    }
}

// K of regressor G at the hyperparameters h over the n points of Zs, cs (gp_points), and its Cholesky factor L in its place, by ONE
// wave: As (LDS) leaves with L in the lower triangle and on the diagonal.  Returns 0, k + 1 for pivot k that is not positive and finite
// (or whose target ts[k] is not finite), or -ADMPC_GP_NO_OPTIMUM for a search without an optimum, the same on every lane; then As is
// not a factor.  The fit (gp_fit_body) and the factor of the evaluation (admpc_quad_eval.hip) share this text: the same bits.
static __device__ __forceinline__ int gp_chol(const LearnGp& G, const GpHyper& h, const int n, const int lane, const double (*Zs)[NPT], const double* ts,
                                              const double* cs, double (*As)[NPT + 1])
{
    const int r = lane & (NPT - 1), nf = G.n_feat;
    const bool act = lane < NPT;
    // row r of K in LDS (lower triangle and diagonal: what the factorisation reads)
    const double il0 = h.inv_l2[0], il1 = nf > 1 ? h.inv_l2[1] : 0.0, il2 = nf > 2 ? h.inv_l2[2] : 0.0;
    const double z0 = Zs[0][r], z1 = Zs[1][r], z2 = Zs[2][r];
    const double diag = h.noise + G.count_noise / cs[r];
    if (act && r < n) {
#pragma unroll 1
        for (int j = 0; j <= r; ++j) {
            const double e0 = z0 - Zs[0][j], e1 = z1 - Zs[1][j], e2 = z2 - Zs[2][j];
            As[r][j] = h.sigma_f * exp_nonpos(-0.5 * (e0 * e0 * il0 + e1 * e1 * il1 + e2 * e2 * il2)) + (j == r ? diag : 0.0);
        }
    }
    __syncthreads();
    // left-looking Cholesky, a column per step: lane r >= k forms L[r][k] from row r and row k of the columns already there
    int fail = h.no_optimum ? -ADMPC_GP_NO_OPTIMUM : 0;
    const int steps = h.no_optimum ? 0 : n;
#pragma unroll 1
    for (int k = 0; k < steps; ++k) {
        double s = 0.0;
        if (r >= k && r < n) {
            s = As[r][k];
#pragma unroll 1
            for (int j = 0; j < k; ++j) s = s - As[r][j] * As[k][j];
        }
        const double d = __shfl(s, k), tk = ts[k];
        if (!(d > 0.0 && isfinite(d) && isfinite(tk))) { fail = k + 1; break; }      // uniform over the wave
        const double l = sqrt(d);
        if (act && r >= k && r < n) As[r][k] = r == k ? l : s / l;
        __syncthreads();
    }
    return fail;
}

// alpha = K^-1 (t - ymean) through the factor gp_chol left in As, by ONE wave: lane r < n returns alpha_r (every lane its right-hand
// side where `fail` is set)
static __device__ __forceinline__ double gp_alpha(const int fail, const int n, const int lane, const double* ts, const double ymean,
                                                  const double (*As)[NPT + 1])
{
    const int r = lane & (NPT - 1);
    double bb = r < n ? ts[r] - ymean : 0.0;
    if (!fail) {
#pragma unroll 1
        for (int k = 0; k < n; ++k) {                      // L w = t - ymean
            const double wk = __shfl(bb, k) / As[k][k];
            if (r == k) bb = wk;
            else if (r > k && r < n) bb = bb - As[r][k] * wk;
        }
#pragma unroll 1
        for (int k = n - 1; k >= 0; --k) {                 // L' alpha = w
            const double ak = __shfl(bb, k) / As[k][k];
            if (r == k) bb = ak;
            else if (r < k) bb = bb - As[k][r] * ak;
        }
    }
    return bb;
}

// One wave (a block of its own) fits regressor g at the hyperparameters h.  Lane r < 32 owns point r and row r of K; lanes 32 .. 63
// mirror lanes 0 .. 31 and store nothing.
static __device__ __forceinline__ void gp_fit_body(const LearnArgs& a, const int g, const GpHyper& h)
{
    __shared__ double Zs[3][NPT], ts[NPT], cs[NPT], As[NPT][NPT + 1];
    const LearnGp& G = a.gp[g];
    const int lane = gp_lane_id(), r = lane & (NPT - 1);
    const bool act = lane < NPT;
    const int nf = G.n_feat;
    const int n = gp_points(a, g, lane, Zs, ts, cs);
    __syncthreads();
    const double ymean = gp_ymean(ts, n);
    const int fail = gp_chol(G, h, n, lane, Zs, ts, cs, As);
    const double bb = gp_alpha(fail, n, lane, ts, ymean, As);
    const int np = fail ? 0 : n;
    AdmpcGp* o = a.out + g;
    if (act) {
#pragma unroll
        for (int d = 0; d < 3; ++d) o->Z[d][r] = (r < np && d < nf) ? Zs[d][r] : 0.0;
        o->alpha[r] = r < np ? bb : 0.0;
    }
    if (lane == 0) {
        o->n_feat = nf;
#pragma unroll
        for (int d = 0; d < 3; ++d) { o->feat[d] = d < nf ? G.feat[d] : 0; o->inv_l2[d] = d < nf ? h.inv_l2[d] : 0.0; }
        o->out = G.out;
        o->n_points = np;
        o->sigma_f = h.sigma_f;
        o->ymean = fail ? 0.0 : ymean;
        a.info[g] = fail ? -fail : n;
    }
}
