// cond_common.h -- what the condensed car kernels (kernel F in admpc_fused20.hip, kernel S in admpc_seg.hip) share: the problem's
// dimensions, the model and the 40 x 40 linear algebra (model_dev.h, dense40.h), the laundering of lane id and config pointer,
// lane-scan primitives, HBM <-> LDS staging of one instance and the LDS-DMA fetch of a wave's H from its slot.
// Include inside the translation unit's anonymous namespace, after include/admpc.h.
#pragma once

#define NX ADMPC_NX
#define NU ADMPC_NU
#define NY ADMPC_NY
#define WAVE 64
#define IPM_FLOOR 1e-40
#define GTS 42           // values per stage of the packed linearisation (see kernel A in admpc_kernels.hip)

#include "model_dev.h"
#include "dense40.h"

// Every phase of a persistent kernel derives its per-lane quantities from a freshly laundered lane id and reads its constants through a
// freshly laundered config pointer: what is loop-invariant across instances must be recomputed in place -- hoisted out of the persistent
// loop it was parked in scratch (257 SGPR lanes and 89 VGPRs in the first build of kernel F) and reloaded inside the stage loops.
// lane id from v_mbcnt (lane within the wave), never from threadIdx.x: v0 would stay live (and be spilled) across the whole kernel
#define LAUNDER_LANE(v) int v = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); asm volatile("" : "+v"(v))
// an opaque zero offset, not an opaque pointer: the compiler keeps knowing that the config is uniform, read-only global memory (s_load);
// reads the kernel's parameter `cfg`
#define LAUNDER_CFG(c) int c##_z = 0; asm volatile("" : "+s"(c##_z)); const AdmpcConfig* __restrict__ c = cfg + c##_z

// the two clocks of the optional phase timers / instance traces (100 MHz): shader clock, constant-rate real-time clock
#if defined(ADMPC_PHASE_TIMERS) || defined(ADMPC_F20_TRACE)
__device__ __forceinline__ unsigned long long clock_ticks() { unsigned long long t; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)); return t; }
__device__ __forceinline__ unsigned long long clock_real() { unsigned long long t; asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)); return t; }
#endif

// x / 7 for 0 <= x < 13107 as a 32-bit multiply-shift: hipcc 7.2 narrows small non-negative ints to 16 bits and its backend
// cannot select the 16-bit udivrem by 7 at -Oz ("Cannot select: i16 udivrem"); there is no `/ 7` or `% 7` on the device.
__device__ __forceinline__ int div7(int x) { return (int)(((unsigned)x * 9363u) >> 16); }


template <class Op>
__device__ __forceinline__ double wave_scan_incl(double v) {      // inclusive prefix over lanes 0..lane
    v = Op::f(v, dpp_shr<0x111, Op::zf>(Op::id(), v));
    v = Op::f(v, dpp_shr<0x112, Op::zf>(Op::id(), v));
    v = Op::f(v, dpp_shr<0x114, Op::zf>(Op::id(), v));
    v = Op::f(v, dpp_shr<0x118, Op::zf>(Op::id(), v));
    v = Op::f(v, dpp_mov<0x142, 0xa>(Op::id(), v));
    v = Op::f(v, dpp_mov<0x143, 0xc>(Op::id(), v));
    return v;
}
// The same for an operand that holds the operation's identity in lanes 32..63 (kernel F: per-stage quantities, lanes 0..19): without the
// row_bcast:31 step, which changes lanes 32..63 only.  Lanes 0..31 hold the bits wave_scan_incl gives them, lane 31 the total; lanes
// 32..63 are NOT the prefix (rows 2 and 3 never see the lower half).
template <class Op>
__device__ __forceinline__ double wave_scan_incl32(double v) {
    v = Op::f(v, dpp_shr<0x111, Op::zf>(Op::id(), v));
    v = Op::f(v, dpp_shr<0x112, Op::zf>(Op::id(), v));
    v = Op::f(v, dpp_shr<0x114, Op::zf>(Op::id(), v));
    v = Op::f(v, dpp_shr<0x118, Op::zf>(Op::id(), v));
    v = Op::f(v, dpp_mov<0x142, 0xa>(Op::id(), v));
    return v;
}

__device__ __forceinline__ int wave_scan_incl_int(int v) {        // inclusive prefix sum over lanes 0..lane
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    return v;
}


// ---- staging of one instance between HBM and LDS.  All loads of a block are issued before the first use, so a wave pays
//      one memory round trip per block instead of one per 64 elements (the plain copy loop serialises load -> ds_write).
//      CNT doubles, CNT even, both sides 16-byte aligned; the clamped tail re-copies the last element pair (same value).
template <int CNT>
__device__ __forceinline__ void stage_in(double* __restrict__ dst, const double* __restrict__ src, const int lane) {
    static_assert(CNT % 2 == 0, "stage_in copies double2");
    constexpr int C2 = CNT / 2, IT = (C2 + WAVE - 1) / WAVE;
    double2 tmp[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) { int i = lane + WAVE * it; i = i < C2 ? i : C2 - 1; tmp[it] = reinterpret_cast<const double2*>(src)[i]; }
#pragma unroll
    for (int it = 0; it < IT; ++it) { int i = lane + WAVE * it; i = i < C2 ? i : C2 - 1; reinterpret_cast<double2*>(dst)[i] = tmp[it]; }
}
// A wave's H (kernel S at S = 4: and Hb behind it) from its slot in global memory (L2) straight into LDS: LDS-DMA (global_load_lds_dwordx4:
// destination = wave-uniform base + lane * 16, no staging registers), issued as soon as the factor that occupies the buffer is dead -- behind the
// last back substitution of an iteration -- so that the round trip hides under the step-length computations.  The caller waits vmcnt(0) before
// the first read (and before any LDS store into the destination).  AUX: the loads' cache policy bits (16 = sc1: served by the L2,
// never by a line the CU's vector L1 may still hold).
template <int CNT, int AUX = 0>
__device__ __forceinline__ void slot_fetch(double* lds_dst, const double* gsrc, const int lane) {
    constexpr int BYTES = CNT * 8, FULL = BYTES / 1024, REM = (BYTES % 1024) / 16;
    static_assert(BYTES % 16 == 0, "slot_fetch copies 16 bytes per lane");
    // 1 KiB pieces; four per base address (the instruction's 12-bit offset moves both the source and the LDS destination).  The base is laundered
    // where the copy is issued: hipcc otherwise hoists one 64-bit address per piece out of the interior-point loop and spills them.
    const char* g = reinterpret_cast<const char*>(gsrc) + lane * 16;
    asm volatile("" : "+v"(g));
    char* l = reinterpret_cast<char*>(lds_dst);
    static_for<0, FULL + (REM > 0 ? 1 : 0)>([&](auto pc) __attribute__((always_inline)) {
        constexpr int p = decltype(pc)::value, grp = p / 4, off = (p % 4) * 1024;
        if (p < FULL || lane < REM)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + grp * 4096), (__attribute__((address_space(3))) void*)(l + grp * 4096), 16, off, AUX);
    });
}
// dq[k][c] = xbar[k][c] - (k < N ? yref[k][c] : yref_e[c]), k = 0..N: the same, for the tracking-error block
template <int NN>
__device__ __forceinline__ void stage_dq(double* __restrict__ dq, const double* __restrict__ xb, const double* __restrict__ yr,
                                         const double* __restrict__ yre, const int lane) {
    constexpr int CNT = (NN + 1) * NX, IT = (CNT + WAVE - 1) / WAVE;
    double xv[IT], yv[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        int i = lane + WAVE * it; i = i < CNT ? i : CNT - 1;
        const int k = div7(i), c = i - 7 * k;
        xv[it] = *(xb + i);
        yv[it] = k < NN ? *(yr + k * 9 + c) : *(yre + c);
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) { int i = lane + WAVE * it; i = i < CNT ? i : CNT - 1; dq[i] = xv[it] - yv[it]; }
}

