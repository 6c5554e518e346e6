// admpc_lane.hip -- the lane generator of the fleet step along a route (include/admpc_lane.h: admpc_waypoints_lane_batch).
//
// The reference node never hands its generator a route.  Its path is the autoware Lane of waypoint_callback
// (nodes/gp_ad_mpc_node.py:351-378): a short local lane that begins at the vehicle, clamped at the vehicle's speed (resample_vel,
// :344-349), padded with its last waypoint (:372-376) and handed to RefTrajectory.set_traj (ref_traj.py:67-86) with every message;
// get_waypoints (ref_traj.py:89-171) then lays its window from the lane's first waypoint on.  This unit does that per vehicle and per
// step on the device, one wave per vehicle, with the route taken from a bank of paths (admpc_path_bank_create):
//
//   search     nearest waypoint of the route, over all of it or over a window around the last answer        (the cut of the lane)
//   cut        waypoints i0 .. i0 + L - 1 of the route, the last one repeated past the route's end            :372-376
//   clamp      vel[i] = min(vel[i], bound), bound = |v| + i * (acc_max * dt * 0.8) by repeated addition       :344-349
//   set_traj   serial cdist, np.unwrap(psi), compute_curvature with filtfilt(ones(11) / 11, 1, .)              ref_traj.py:10-25, :67-86
//   window     waypoints_one (waypoints_dev.h) on the lane's seven columns, M = L                              ref_traj.py:89-171
//
// The lane lives in LDS (LANE_LDS_DOUBLES doubles, static); there is no per-vehicle workspace in global memory.  Every serial sum of the
// reference (cdist, the unwrap's cumsum, the clamp's bound) is summed serially, in the reference's order: the terms are computed by all
// lanes in parallel, the running sum is carried by every lane in registers, and lane i % 64 keeps element i.
#include <math.h>
#include <stdio.h>
#include "admpc_host.h"

#define WAVE 64
#define LANE_MIN_L 34                 // scipy's filtfilt refuses inputs of 3 * 11 = 33 samples or fewer
#define LANE_MAX_L 256
#define LANE_ROUNDS (LANE_MAX_L / WAVE)   // waypoints a lane of the wave owns at most
#define LANE_PAD 33                   // filtfilt's default padlen, 3 * max(len(a), len(b))
#define LANE_TAPS 11
#define LANE_GRID 4096                // as admpc_waypoints_batch
#define LANE_LDS_DOUBLES (7 * LANE_MAX_L + 2 * (LANE_MAX_L + 2 * LANE_PAD) + WAVE)

namespace {

#include "waypoints_dev.h"

// One wave per vehicle.  path_of[b] and lane_idx[b] are uniform over the block, so is every barrier.
__global__ __launch_bounds__(WAVE) void admpc_waypoints_lane_kernel(int K, int H, double dt, int B, int L, int back, int ahead,
        const PathDesc* __restrict__ desc, const double* __restrict__ cols, const int32_t* __restrict__ path_of, int32_t* __restrict__ lane_idx,
        const double* __restrict__ Xi, const double* __restrict__ Yi, const double* __restrict__ Pi,
        const double* __restrict__ vx, const double* __restrict__ vy, int clamp, double acc_max, double clamp_dt,
        double* __restrict__ out_ref, double* __restrict__ out_err, int32_t* __restrict__ out_stop)
{
#pragma clang fp contract(off)      // every operation rounded on its own, as the reference's Python / numpy arithmetic does
    __shared__ double col[7][LANE_MAX_L];                  // vel, x, y, psi, unwrapped psi, cdist, curv: the columns waypoints_one reads
    __shared__ double ext[LANE_MAX_L + 2 * LANE_PAD];      // the filter's input, extended by LANE_PAD samples at both ends
    __shared__ double fwd[LANE_MAX_L + 2 * LANE_PAD];      // the forward pass
    __shared__ double sh[WAVE];
    const int lane = threadIdx.x;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const int k = path_of[b];
        if (k < 0 || k >= K) {                             // the bank step's rule: NaN rows, stop 0; lane_idx[b] stays
            double* o = out_ref + (size_t)b * 6 * H;
            if (lane < H)
                for (int r = 0; r < 6; ++r) o[r * H + lane] = NAN;
            if (lane < 3) out_err[b * 3 + lane] = NAN;
            if (lane == 0) out_stop[b] = 0;
            continue;
        }
        const PathDesc d = desc[k];
        const int M = (int)d.M;
        const double* __restrict__ rv = cols + d.off[0];
        const double* __restrict__ rx = cols + d.off[1];
        const double* __restrict__ ry = cols + d.off[2];
        const double* __restrict__ rp = cols + d.off[3];
        // (1) where the lane starts: first index of the smallest sqrt(dx^2 + dy^2) over [lo, hi]; lo where every distance is NaN
        int lo = 0, hi = M - 1;
        const int prev = lane_idx[b];
        if (prev >= 0) {
            const long i = prev < M - 1 ? prev : M - 1;
            lo = (int)(i - back > 0 ? i - back : 0);
            hi = (int)(i + ahead < M - 1 ? i + ahead : M - 1);
        }
        const double X0 = Xi[b], Y0 = Yi[b];
        double best = INFINITY; int bi = 0x7fffffff;
        for (int m = lo + lane; m <= hi; m += WAVE) {
            const double dx = rx[m] - X0, dy = ry[m] - Y0;
            const double dist = __dsqrt_rn(dx * dx + dy * dy);
            if (dist < best) { best = dist; bi = m; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(best, o, WAVE); const int oi = __shfl_xor(bi, o, WAVE);
            if (ov < best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        const int i0 = bi <= hi ? bi : lo;
        __syncthreads();                                   // every lane has read lane_idx[b]
        if (lane == 0) lane_idx[b] = i0;
        // (2) the cut, the last waypoint repeated past the route's end (:372-376).  Waypoint i belongs to lane i % 64, round i / 64.
        for (int i = lane; i < L; i += WAVE) {
            const long at = (long)i0 + i;
            const int src = (int)(at < M - 1 ? at : M - 1);
            col[0][i] = rv[src]; col[1][i] = rx[src]; col[2][i] = ry[src]; col[3][i] = rp[src];
        }
        // the node's clamp on it (:344-349): the bound grows by repeated addition, every lane carries it and keeps its own waypoints'
        if (clamp) {
            const double sx = vx[b] * vx[b], sy = vy[b] * vy[b];
            double bound = __dsqrt_rn(sx + sy);
            const double inc = (acc_max * clamp_dt) * 0.8;
            double mine[LANE_ROUNDS];
#pragma unroll
            for (int r = 0; r < LANE_ROUNDS; ++r) {
                mine[r] = 0.0;
                if (r * WAVE < L)
                    for (int j = 0; j < WAVE; ++j) {
                        if (j == lane) mine[r] = bound;
                        bound = bound + inc;
                    }
            }
#pragma unroll
            for (int r = 0; r < LANE_ROUNDS; ++r) {
                const int i = r * WAVE + lane;
                if (i < L && col[0][i] > mine[r]) col[0][i] = mine[r];
            }
        }
        __syncthreads();
        // (3) set_traj: the terms of the two running sums in parallel (segment lengths into ext, the unwrap's corrections into fwd) ...
        for (int i = lane; i < L; i += WAVE) {
            double seg = 0.0, corr = 0.0;
            if (i >= 1) {
                const double dx = col[1][i] - col[1][i - 1], dy = col[2][i] - col[2][i - 1];
                seg = __dsqrt_rn(dx * dx + dy * dy);
                const double dd = col[3][i] - col[3][i - 1];                   // numpy.unwrap, as in waypoints_one
                double ddmod = fmod(dd + M_PI, 2.0 * M_PI);
                if (ddmod < 0.0) ddmod += 2.0 * M_PI;
                ddmod -= M_PI;
                if (ddmod == -M_PI && dd > 0.0) ddmod = M_PI;
                corr = fabs(dd) < M_PI ? 0.0 : ddmod - dd;
            }
            ext[i] = seg; fwd[i] = corr;
        }
        __syncthreads();
        // ... and the sums themselves, serial from element 0 (0 + x is x): cdist[i] = seg[i] + cdist[i-1] (ref_traj.py:77), and
        // unwrapped[i] = psi[i] + cumsum(corr)[i]
        {
            double cd = 0.0, cum = 0.0, kcd[LANE_ROUNDS], kcum[LANE_ROUNDS];
#pragma unroll
            for (int r = 0; r < LANE_ROUNDS; ++r) {
                kcd[r] = 0.0; kcum[r] = 0.0;
                if (r * WAVE < L)
                    for (int j = 0; j < WAVE; ++j) {
                        const int i = r * WAVE + j;
                        if (i < L) { cd = ext[i] + cd; cum = cum + fwd[i]; }
                        if (j == lane) { kcd[r] = cd; kcum[r] = cum; }
                    }
            }
#pragma unroll
            for (int r = 0; r < LANE_ROUNDS; ++r) {
                const int i = r * WAVE + lane;
                if (i < L) { col[5][i] = kcd[r]; col[4][i] = col[3][i] + kcum[r]; }
            }
        }
        __syncthreads();
        // (4) compute_curvature (ref_traj.py:10-25): diff(unwrapped psi) / max(diff(cdist), 0.1), the last value repeated ...
        for (int i = lane; i < L; i += WAVE) {
            const int j = i < L - 1 ? i : L - 2;
            const double ds = col[5][j + 1] - col[5][j];
            col[6][i] = (col[4][j + 1] - col[4][j]) / (ds < 0.1 ? 0.1 : ds);       // np.maximum: a NaN difference stays NaN
        }
        __syncthreads();
        // ... through filtfilt(ones(11) / 11, 1, .): odd extension by LANE_PAD samples, the 11-tap mean forwards from the steady state of
        // its first sample, the same backwards, the middle L samples kept.  The taps are summed oldest first, as lfilter's transposed
        // direct form does.  (The kept samples lie more than 10 taps inside the extension, so neither initial state reaches them.)
        const int n = L + 2 * LANE_PAD;
        for (int i = lane; i < n; i += WAVE) {
            double v;
            if (i < LANE_PAD) v = 2.0 * col[6][0] - col[6][LANE_PAD - i];
            else if (i < LANE_PAD + L) v = col[6][i - LANE_PAD];
            else v = 2.0 * col[6][L - 1] - col[6][L - 2 - (i - LANE_PAD - L)];
            ext[i] = v;
        }
        __syncthreads();
        const double tap = 1.0 / LANE_TAPS;
        for (int i = lane; i < n; i += WAVE) {
            double acc = 0.0;
            for (int t = LANE_TAPS - 1; t >= 0; --t) {
                const double term = tap * ext[i - t > 0 ? i - t : 0];
                acc = t == LANE_TAPS - 1 ? term : term + acc;
            }
            fwd[i] = acc;
        }
        __syncthreads();
        for (int i = lane; i < L; i += WAVE) {
            const int at = i + LANE_PAD;
            double acc = 0.0;
            for (int t = LANE_TAPS - 1; t >= 0; --t) {
                const double term = tap * fwd[at + t < n - 1 ? at + t : n - 1];
                acc = t == LANE_TAPS - 1 ? term : term + acc;
            }
            col[6][i] = acc;
        }
        __syncthreads();
        // (5) get_waypoints on the lane
        waypoints_one(L, H, dt, b, col[0], col[1], col[2], col[3], col[4], col[5], col[6], Xi, Yi, Pi, out_ref, out_err, out_stop, sh);
        __syncthreads();
    }
}

static_assert(LANE_LDS_DOUBLES * sizeof(double) < 64 * 1024, "the lane fits the static LDS limit");

}  // namespace

extern "C" {

// the refusals every entry point of admpc_lane.h shares; they touch neither the device nor another argument
int admpc_lane_params_check(const char* who, const AdmpcLaneParams* lane, const int32_t* lane_idx)
{
    char msg[160];
    const char* what = nullptr;
    if (!lane) what = "the lane parameters are not set";
    else if (lane->L < LANE_MIN_L || lane->L > LANE_MAX_L) what = "L must be in [34, 256]";
    else if (lane->back < 0 || lane->ahead < 0) what = "back and ahead must not be negative";
    else if (!lane_idx) what = "null lane_idx";
    if (!what) return ADMPC_OK;
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return admpc_set_error(ADMPC_EINVAL, msg);
}

int admpc_waypoints_lane_batch(const AdmpcPathBank* bank, const AdmpcLaneParams* lane, int B, const int32_t* path_of, int32_t* lane_idx,
                               const double* X_init, const double* Y_init, const double* psi_init,
                               const double* vx, const double* vy, int clamp, double acc_max, double clamp_dt,
                               double* out_ref, double* out_err, int32_t* out_stop, void* stream)
{
    const int rc = admpc_lane_params_check("admpc_waypoints_lane_batch", lane, lane_idx);
    if (rc) return rc;
    if (!bank || B < 0) return admpc_set_error(ADMPC_EINVAL, "admpc_waypoints_lane_batch: null bank or negative batch");
    if (B == 0) return ADMPC_OK;
    if (!path_of || !X_init || !Y_init || !psi_init || !vx || !vy || !out_ref || !out_err || !out_stop)
        return admpc_set_error(ADMPC_EINVAL, "admpc_waypoints_lane_batch: null array argument");
    int device = 0, K = 0;
    double dt = 0.0;
    const void* desc = nullptr;
    const double* cols = nullptr;
    const int H = admpc_path_bank_table(bank, &device, &K, &dt, &desc, &cols);
    DeviceGuard guard(device);
    if (!guard.ok()) return admpc_set_error(ADMPC_EHIP, "hipSetDevice failed");
    const int grid = B < LANE_GRID ? B : LANE_GRID;
    hipLaunchKernelGGL(admpc_waypoints_lane_kernel, dim3(grid), dim3(WAVE), 0, (hipStream_t)stream, K, H, dt, B, lane->L, lane->back, lane->ahead,
                       (const PathDesc*)desc, cols, path_of, lane_idx, X_init, Y_init, psi_init, vx, vy, clamp ? 1 : 0, acc_max, clamp_dt,
                       out_ref, out_err, out_stop);
    if (hipGetLastError() != hipSuccess) return admpc_set_error(ADMPC_EHIP, "admpc_waypoints_lane_kernel: launch failed");
    return ADMPC_OK;
}

}  // extern "C"
