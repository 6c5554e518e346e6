// admpc_fused20.hip -- the N = 20 fp64 SQP-RTI step (BASELINE configs[1..3]) as ONE persistent kernel for gfx950.
//
// One wavefront (= one workgroup of 64 lanes) owns one MPC instance from its inputs to its outputs and then draws the next one
// from a ticket counter.  The packed linearisation (7.8 KB), the condensed Hessian H and its factor L (6.6 KB: one buffer, they are
// never live together) and every intermediate live in the wave's 19.1 KB of LDS or in registers -- eight instances per CU, two waves
// per SIMD; H waits in a per-wave slot of global memory (L2) while L occupies its buffer and comes back by LDS-DMA in front of every
// interior-point iteration.  Phase A runs once per instance.  Phases of an instance (reference = data_driven_mpc/ros_gp_mpc/src/ad_mpc/...):
//   A  H0/H1  ERK4 + forward sensitivities of all 20 stages           ad_3d_optimizer.py:280-310, acados ERK
//             (A1: lanes (stage, third) integrate the state and table      (acados_solver_sim_car.c:655-665)
//              the Jacobian entries of the four RK stages in LDS; A2: the same lanes integrate their 2-3 sensitivity columns
//              from the tables -- the split keeps the phase inside the 256-register budget of two waves per SIMD)
//   C  H2-H4  Gauss-Newton cost, bounds, full condensing                ad_3d_optimizer.py:146-199; acados_solver_sim_car.c:145
//   D  H5     unconstrained trial, Mehrotra predictor-corrector on the dense 40-input QP (reference: HPIPM, :688-692);
//             the 40 x 40 LDL' and its solve are dense40.h's dense40_factorise / dense40_solve (shared with admpc_quad.hip); the
//             right-hand sides that are known in front of a factorisation (the trial's, the predictor's) go through it as row 40
//             of the matrix and are finished by dense40_solve_back: no forward substitution for them
//   E  H6     state expansion, full step, cost, status                  acados_solver_sim_car.c:647-648,677
// The phase bodies descend from the four-kernel pipeline of rounds 1-2 (kernels A, C, D, E; C, D, E removed, last
// present at commit a808f29); what changed is where the data lives and that no instance waits for a kernel boundary: the slowest instance
// of a batch starts at once instead of after everybody's linearisation and condensing.  What this kernel shares with the segmented
// kernel (admpc_seg.hip) -- dimensions, lane / config laundering, staging, slot fetch, the timers' clocks -- is cond_common.h.
//
// Alternatives that were built, measured and removed (compile-time switches, last present at commit a808f29):
//   - H = sum_k Gamma_k' Q Gamma_k on the vector pipe (v_fmac_f64_dpp rows) instead of MFMA tiles: 13.4 against 10.1 us per instance
//     in isolation (profiles/r3/mfma_condense_ab.txt).
//   - the whole condensing -- recursion Gamma_{k+1} = A_k Gamma_k, free response, Hessian, reduced gradient -- in MFMA tiles: correct
//     (106 GPU tests green) but 1 % SLOWER: a 16 x 16 x 4 tile carries 7 x 7 useful products in the recursion and the dependent chain
//     of 42 of them is latency-bound (scripts/probes/mfma_condense_probe.hip, profiles/r3/mfma_condense_ab.txt).
//   - the LDS reads of a condensing stage where hipcc puts them: 458 instead of 97 s_waitcnt in the phase (an instruction of any kind
//     costs its wave an issue slot, and the single-wave time is what the end of a launch runs at).
//   - the free response xhat_k propagated redundantly by all 64 lanes instead of riding in lane 40 as a 41st column of Gamma: 30 more
//     multiply-adds per stage, the same bits.
//   - the 30 entries of A_k by fifteen ds_read_b128 that hand all 64 lanes the same 16 bytes instead of two ds_read_b64 per stage and
//     DPP row broadcasts: 15 KB of LDS return traffic per stage for 240 bytes of information, on an LDS pipe that was 76 % busy over
//     the whole launch (SQ_ACTIVE_INST_LDS).  The same bits.
//   - inputs and outputs loaded and stored non-temporally (to keep the slot buffers in the L2): no effect on traffic, 0.5 % slower.
//   - the next ticket drawn between instances instead of under phase E: 3-4 us of a 36 us cheap instance in the drain.
//   - deferred expansions: instances drawn by ticket pushed their expansion (phase A once more and phase E) into queues that the waves
//     popped when the ticket queue was dry (jobs of 15 us instead of 54 at the end of a launch).  Bit-identical, and SLOWER: 19.2 M
//     against 20.9 M solves/s at configs[1], 22.1 against 24.1 M at B = 8192, two batches in flight 20.6 against 23.1 M -- an expansion
//     that changes waves pays ~6 us of dependent trips to the memory side (queue scan, pop, entry, du; the instance's inputs miss the
//     other XCD's L2) on a 15 us job, more than the shorter ramp returns.  With ONE queue the counter line was the bottleneck
//     (same-line atomics retire at ~10 ns: 35 % slower), and compare-and-swap pops took 35 ms per step.
//   - the expansion's LDS reads where hipcc puts them, three waits for reads of its own stage in every stage of the recursion: 40 % more
//     wave time in phase E on a lone wave, 1.2 % per step at configs[1] (profiles/r4/f20_expand_ring.txt).
//   - the predictor and the corrector of an interior-point iteration as two straight-line sections of one always-inline lambda instead of a
//     loop of two trips (whose carried state hipcc moves through 18 + 18 + 13 v_mov_b64 per iteration): the copies fall to 10, but the
//     results are no longer the parent's bits (1e-13 on u; statuses and iteration counts identical).  The loop keeps six pass-invariant
//     products (G0 rd0 ... G6 Drd1) hoisted and rounded on their own and computes t lam of the centring step in a block of its own;
//     straight-line, hipcc contracts them into other multiply-adds.  Pinning the six products was not enough; reproducing every
//     contraction by hand was not attempted.  Laundering the state at the back edge moves the copies (8 + 36 + 8), it does not remove them
//     (profiles/r4/f20_valu_diet.txt).
//   - wave-priority classes, a reversed ticket order for the second wave of a SIMD, a trap on the never-taken side of the per-stage
//     block test, other rungs of the priority ladder (see phase D for the measured ones).
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>
#include <math.h>
#include "../../include/admpc.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

#include "cond_common.h"      // dimensions, model_dev.h, dense40.h, LAUNDER_LANE / LAUNDER_CFG, staging, slot fetch

// LDS access through a byte address held in a register plus a compile-time byte offset (the instruction's offset: field): the stage chains
// of phases C and E form their per-lane addresses once per instance and launder them -- built from indices into lds_raw, hipcc
// rematerialises every address from literals in every stage block (machine LICM is off for this unit, see the Makefile)
typedef __attribute__((address_space(3))) double lds_f64;
typedef double d2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) d2 lds_f64x2;
__device__ __forceinline__ double lds_ld(const unsigned a, const int off) { return *reinterpret_cast<const lds_f64*>((size_t)(a + (unsigned)off)); }
__device__ __forceinline__ double2 lds_ld2(const unsigned a, const int off) { const d2 v = *reinterpret_cast<const lds_f64x2*>((size_t)(a + (unsigned)off)); return make_double2(v.x, v.y); }
__device__ __forceinline__ void lds_st(const unsigned a, const int off, const double v) { *reinterpret_cast<lds_f64*>((size_t)(a + (unsigned)off)) = v; }

// ---- optional per-phase wave-time accounting (build with -DADMPC_PHASE_TIMERS: `make timers`): s_memtime ticks (100 MHz) summed
//      over all waves: 0 ticket draw, 1 A1 (state RK4 + model), 2 A2 (sensitivity columns), 3 C (condensing), 4 D trial,
//      5 D interior-point iterations, 6 E (expansion + outputs); [8] wave-time from kernel start to the wave's exit
#if defined(ADMPC_PHASE_TIMERS) || defined(ADMPC_F20_TRACE)
__device__ unsigned long long g_f20_trace[4 * 8192];      // per instance (first 8192): start, end (s_memrealtime, 100 MHz), block, IPM start
#define F20_TRACE_BEGIN() const unsigned long long tr_t0 = clock_real(); unsigned long long tr_t1 = 0
#define F20_TRACE_MID() tr_t1 = clock_real()
#define F20_TRACE_END(inst) do { if (threadIdx.x == 0 && (inst) < 8192) { g_f20_trace[4 * (inst)] = tr_t0; g_f20_trace[4 * (inst) + 1] = clock_real(); g_f20_trace[4 * (inst) + 2] = blockIdx.x; g_f20_trace[4 * (inst) + 3] = tr_t1; } } while (0)
#else
#define F20_TRACE_BEGIN() do { } while (0)
#define F20_TRACE_MID() do { } while (0)
#define F20_TRACE_END(inst) do { } while (0)
#endif
#ifdef ADMPC_PHASE_TIMERS
__device__ unsigned long long g_f20_ticks[16];
#define F20_DECL() unsigned long long ph_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; const unsigned long long ph_t0 = clock_ticks(); unsigned long long ph_last = ph_t0
#define F20_STAMP(k) do { const unsigned long long t_ = clock_ticks(); ph_acc[k] += t_ - ph_last; ph_last = t_; } while (0)
#define F20_FLUSH() do { if (threadIdx.x == 0) { for (int q_ = 0; q_ < 8; ++q_) atomicAdd(&g_f20_ticks[q_], ph_acc[q_]); atomicAdd(&g_f20_ticks[8], clock_ticks() - ph_t0); atomicMax(&g_f20_ticks[9], clock_ticks() - ph_t0); } } while (0)
#elif defined(F20_MARKS)      // listing with phase markers for scripts/asm_phase_stats.py (hipcc -S -DF20_MARKS): the code after stamp k is phase k + 1
#define F20_DECL() do { } while (0)
#define F20_STAMP(k) asm volatile("; MARK_after" #k)
#define F20_FLUSH() do { } while (0)
#else
#define F20_DECL() do { } while (0)
#define F20_STAMP(k) do { } while (0)
#define F20_FLUSH() do { } while (0)
#endif

// LDS map of one instance (doubles), 19.1 KB, eight instances per CU (two waves per SIMD):
//   GT [0, 840)  packed linearisation, written at the end of phase A, read by phases C and E
//   H/L [840, 1660)  H (from phase C's row store to the row build of a factorisation) and the factor L (from there to the last
//        substitution of the iteration) in ONE buffer: H waits in the wave's slot of global memory and is fetched back (slot_fetch)
//   park [1660, 1980), cb / invd / sb / sb2 [1980, 2236)  per-lane constants and exchange buffers of phase D (the relative layout
//        dense40.h's col_head assumes: sb = cb + 128); sb2 doubles as the right-hand-side row of the factorisations (Dense40Lds::rhs:
//        y in, D^-1 L^-1 y out), invd carries the suffix sums of e from the residual pass to the predictor's right-hand side
//   bl [2236, 2376)  defects b_k, written by phase A, read by phases C and E;  scheduler table [2376, 2440)
// The other phases alias it:
//   A   JT [0, 1960) Jacobian tables of the RK stages (over GT, H/L, park; clear of bl and the scheduler table); GT is written when the
//       tables are dead
//   C   dq [860, 1008), gam [1008, 1520) in the H/L buffer (dead until the row store of H behind the last stage)
//   E   dq -> dx [860, 1008), du [1008, 1072), dump [1072, 1276), zeros [1276, 1468) in the H/L buffer (dead behind the interior point)
// Banks: the tables keep stride 98; GT, dq, gam keep their offsets; H/L moves by 840 doubles as a whole (16-byte aligned: the
// LDS-DMA destination), which keeps the triangular row starts' conflict-free pattern.
struct FusedLds {
    static constexpr int N = 20, NTRI = 820;
    static constexpr int oGT = 0, oH = oGT + N * GTS, oL = oH, oPark = oH + NTRI, oCb = oPark + 5 * 64;
    static constexpr int oBl = oCb + 4 * 64;
    static constexpr int oSch = oBl + N * NX;                           // [2][64] ints: inclusive scan of the bin counts (most expensive bin first), the counts
    static constexpr int total = oSch + 64;                             // 2440 doubles = 19 520 B
    static constexpr int JTS = 24, JTK = 4 * JTS + 2;                   // Jacobian entries per (stage, RK stage); doubles per stage: 98, not 96 --
                                                                        // 768 B apart the 20 stages of a table access all hit one bank group
    static constexpr int oJT = 0, oDqC = 860, oGam = oDqC + 148;
    static constexpr int oDumpE = oGam + 64;                            // phase E: where lanes that hold no state store (behind du, per stage + 7)
    static constexpr int oZeroE = oDumpE + 64 + N * NX, nZeroE = 192;   // phase E: zeros, what lanes >= 7 read for b_k and du (offsets up to (N - 1) * NX)
    static_assert(oJT + N * JTK <= oBl, "LDS aliases: phase A's tables end before bl and the scheduler table");
    static_assert(oGT + N * GTS <= oH, "LDS aliases: GT survives phases C, D, E (clear of H/L, park and the exchange buffers)");
    static_assert(oDqC >= oH && oDqC + (N + 1) * NX <= oGam && oGam + (NX + 1) * 64 <= oH + NTRI, "LDS aliases: dq, gam (phase C), dx, du (phase E) inside H/L");
    static_assert(oDumpE >= oGam + 64 && oDumpE + 64 + N * NX <= oH + NTRI, "LDS aliases: phase E's dump area behind du, inside H/L");
    static_assert(oZeroE >= oDumpE + 64 + N * NX && oZeroE + nZeroE <= oH + NTRI && (N - 1) * NX + 1 <= nZeroE && 2 * N <= nZeroE, "LDS aliases: phase E's zeros behind the dump area, inside H/L");
    static_assert(oBl >= oCb + 4 * 64 && oBl + N * NX <= oSch && oSch + 64 <= total, "LDS aliases: bl, scheduler table");
    static_assert(oH % 2 == 0 && oCb % 2 == 0, "16-byte alignment: LDS-DMA destination, double2 exchange");
    static_assert(8 * total * 8 <= 160 * 1024, "eight instances per CU");
};

// ---- work order.  A wave owns an instance for 40 us (the trial solves it) up to 200 us (13 interior-point iterations), and a batch
// of 4096 is two rounds of the 2048 resident waves: an expensive instance that is drawn late IS the kernel's run time.  A pre-pass
// (one thread per instance, a few loads) bins the instances by a kinematic estimate of how far the longitudinal input has to leave
// its box: the constant acceleration that carries the vehicle from x0 to the along-track position of the terminal reference,
// a = 2 (s_ref - v_x T) / T^2, against [lbu_0, ubu_0].  On the config-2 scenarios every instance that needs 8 or more iterations
// is in the first round with it, and 1837 of the 1841 that need the interior point at all (correlation with the iteration count
// 0.80).  A heuristic: it orders work and nothing else -- results do not depend on the draw order.
//   sched: [0] ticket counter, [1] exit counter, [F20_BINS0 + q] instances in bin q, [F20_HDR + q * cap + j] j-th instance of bin q
#include "work_order.h"

static_assert(WAVE == 64, "one wavefront per workgroup: WSYNC is a wave-level fence in this build");
template <int QMASK>
__global__ __launch_bounds__(WAVE, 2) void admpc_fused20_kernel(const AdmpcConfig* __restrict__ cfg, int B,
                                                                const double* __restrict__ x0g, const double* __restrict__ yrefg,
                                                                const double* __restrict__ yrefeg, const double* __restrict__ pg,
                                                                double* __restrict__ xbarg, double* __restrict__ ubarg,
                                                                double* __restrict__ costg, int32_t* __restrict__ statusg,
                                                                int32_t* __restrict__ itersg, int first_pass, int* __restrict__ sched, int cap,
                                                                double* __restrict__ slotbuf)
{
    constexpr int N = 20, n = 40;
    extern __shared__ double lds_raw[];
    double* const Hp = lds_raw + FusedLds::oH;          // packed lower-triangular rows of H
    double* const Lp = lds_raw + FusedLds::oL;          // packed strictly-lower rows of the unit factor L (M = L D L'): H's buffer
    double* const park = lds_raw + FusedLds::oPark;     // [5][64] per-lane constants (registers are the scarce resource)
    double* const cb = lds_raw + FusedLds::oCb;         // [64] step broadcast buffer
    double* const invd = cb + 64;                       // [64] 1 / D_jj
    double* const sb = invd + 64;                       // [64] per-stage exchange
    double* const sb2 = sb + 64;                        // [64]
    double* const JT = lds_raw + FusedLds::oJT;         // phase A: [N][4][24] Jacobian entries of the RK stages
    double* const GT = lds_raw + FusedLds::oGT;         // phases A (end), C, E: packed linearisation of the instance
    double* const bl = lds_raw + FusedLds::oBl;         // phases A, C, E: defects b_k
    double* const dqC = lds_raw + FusedLds::oDqC;       // phase C: xbar_k - xref_k
    double* const gam = lds_raw + FusedLds::oGam;       // phase C: [NX][64] Gamma components of the current stage
    double* const dqE = lds_raw + FusedLds::oDqC;       // phase E: xbar_k - xref_k, overwritten by dx_k
    double* const dus = lds_raw + FusedLds::oGam;       // phase E: [64] du per input
    // H's slot: NTRI doubles of global memory that belong to the WAVE (grid x 820 doubles), rewritten for every instance the wave draws.
    // Phase C stores H there behind its row store; the trial factorises in place; an instance that iterates fetches H back by LDS-DMA in
    // front of iteration 0 and behind the corrector's last substitution of every iteration (the factor is dead there).  The lines stay in
    // the L2 (no release fence: it would write them back to HBM; no acquire either: the fetches do not read through the L1).
    double* const slot = slotbuf + (size_t)blockIdx.x * FusedLds::NTRI;
    constexpr int slot_aux = 16;                    // cache policy of the fetches: sc1 (L2-served; see the first fetch in phase D)
#define PK_DL   park[0 * 64 + lane]
#define PK_DUU  park[1 * 64 + lane]
#define PK_G0   park[2 * 64 + lane]
#define PK_DDL  park[3 * 64 + lane]
#define PK_DDU  park[4 * 64 + lane]

    // Factorisation of the Newton matrix M = H + diag(dbar) + (s_odd on the odd columns of the u1 rows) into L D L' (LDS: Lp, invd) and
    // the solve M x = y through the factor: dense40.h, the functions the quadrotor's kernel calls.
    // Both factorisations of this kernel know their first right-hand side before they start (the trial's -g0, the predictor's, a function of
    // the iterate): it is published in sb2 and rides through the factorisation as row 40 (dense40.h), which leaves D^-1 L^-1 y in sb2 -- the
    // forward substitution and the scaling of that solve are never run.  The corrector's right-hand side needs the predictor's result and
    // takes the whole solve.
    const Dense40Lds W{Hp, Lp, cb, invd, sb2};
    // The row build pulls H unmasked and takes the diagonal term through LDS where that is exact (dense40.h, PULL: 2 the trial, s_odd = 0
    // in every lane; 1 the iterations, s_odd = 0 in the even lanes).  H's diagonal slots are rewritten in place: the buffer turns into
    // the factor's right behind, and H comes back from the slot -- phase C's stage_in(slot, Hp) has read H from LDS before the trial's
    // rewrite (program order, one wave), and every fetch lands before the mat-vec in front of the next rewrite.
    auto factorise = [&](const double dbar_, const double sodd_, const int lz_, auto pull) __attribute__((always_inline)) {
        dense40_factorise(W, lz_, dbar_, sodd_, lz_, [&](double (&)[n]) __attribute__((always_inline)) {
            // H's rows are in registers: its buffer becomes the factor's.  Diagonal slots of the packed factor: 0.0 (the factorisation stores the
            // strictly-lower part only; the substitution assembly lets the source lane of a step take part with this multiplier)
            if (lz_ < n) Lp[lz_ * (lz_ + 1) / 2 + lz_] = 0.0;
        }, std::true_type{}, pull);
    };

    // ---------------- persistent loop: first ticket = block index, later ones from one global counter ----------------
    F20_DECL();
    bool first_ticket = true;
    // Tickets.  Between two instances f20_next is three dependent trips to the L2 (the ticket counter, the bin counts, the bin's list) in
    // front of the instance's own loads -- 3-4 us of a 36 us cheap instance when the wave is alone on its SIMD (the drain).  The bin counts
    // do not change while the kernel runs: every wave scans them once into LDS.  The next ticket is drawn at the top of phase E and resolved
    // behind its recursion, so both remaining trips run under the expansion.
    int* const sch_incl = reinterpret_cast<int*>(lds_raw + FusedLds::oSch);
    int* const sch_cnt = sch_incl + 64;
    if (cap != 0) {
        LAUNDER_LANE(lane_s);
        const int c = sched[F20_BINS0 + F20_NB - 1 - lane_s];
        sch_cnt[lane_s] = c;
        sch_incl[lane_s] = wave_scan_incl_int(c);
        WSYNC();
    }
    // instance of ticket t (wave-uniform), -1 behind the batch: f20_next's walk over the bins, the counts from LDS
    auto ticket_entry_addr = [&](const int t, const int lane_) __attribute__((always_inline)) -> const int* {
        const int incl = sch_incl[lane_], c = sch_cnt[lane_];
        const unsigned long long m = __ballot(incl > t);
        if (m == 0ull) return nullptr;
        const int l = __ffsll((long long)m) - 1;
        const int base = __builtin_amdgcn_readlane(incl - c, l);
        return sched + F20_HDR + (size_t)(F20_NB - 1 - l) * cap + (t - base);
    };
    int next_inst = -2;                                                 // -2: not drawn yet
    const int grid = (int)gridDim.x;
    for (;;) {
        LAUNDER_LANE(lane0);
        int inst;
        if (cap == 0) inst = first_ticket ? (int)blockIdx.x : -1;
        if (cap == 0) { }                                               // (kept apart from the test above: merging them changes the listing)
        else if (next_inst != -2) inst = next_inst;
        else {
            int t = (int)blockIdx.x;
            if (!first_ticket) { int v = 0; if (lane0 == 0) v = atomicAdd(sched, 1); t = grid + __builtin_amdgcn_readfirstlane(v); }
            const int* const e = ticket_entry_addr(t, lane0);
            inst = e ? __builtin_amdgcn_readfirstlane(*e) : -1;
        }
        next_inst = -2;
        first_ticket = false;
        if (inst < 0) break;
        F20_TRACE_BEGIN();
        if (!first_pass && statusg[inst] != 0) continue;    // failed / converged in an earlier SQP iteration of this call
        double* const xbg = xbarg + (size_t)inst * (N + 1) * NX;
        double* const ubg = ubarg + (size_t)inst * N * NU;
        const double* yrg = yrefg + (size_t)inst * N * NY;

        // =================================================================================================================
        // phase A (H0/H1): ERK4 + forward sensitivities.  Lane 3k + g <-> (stage k, column group g) as in kernel A:
        // g = 0: x-columns 2,3,4; g = 1: x-columns 5,6; g = 2: u-columns 0,1.  Lanes 60..63 shadow task 59 and store nothing.
        // =================================================================================================================
        double du = 0.0;
        bool failed = false;
        int it = 0;
        {
            LAUNDER_LANE(lane); LAUNDER_CFG(cf);
            const double h = cf->Ts;
            const int tsk = lane < 3 * N ? lane : 3 * N - 1;
            const int k = (int)(((unsigned)tsk * 21846u) >> 16), g = tsk - 3 * k;      // tsk / 3, tsk % 3 without a narrow udivrem
            const bool live = lane < 3 * N;
        F20_STAMP(0);
            // ---- A1: the state through the four RK stages (all three lanes of a stage, redundantly: they share the GP sums);
            //      lane g == 0 tables the Jacobian entries of every RK stage and writes the defect
            {
                const double pin = pg[inst];
                double x[NX], u[NU], xn1[NX];
#pragma unroll
                for (int i = 0; i < NX; ++i) { x[i] = *(xbg + k * NX + i); xn1[i] = *(xbg + (k + 1) * NX + i); }
                u[0] = *(ubg + k * NU); u[1] = *(ubg + k * NU + 1);
                double kx[NX], accx[NX];
#pragma unroll
                for (int i = 0; i < NX; ++i) { kx[i] = 0.0; accx[i] = 0.0; }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const double cs = (s == 0) ? 0.0 : (s == 3 ? 1.0 : 0.5);
                    const double ws = (s == 0 || s == 3) ? (1.0 / 6.0) : (2.0 / 6.0);
                    double X[NX];
#pragma unroll
                    for (int i = 0; i < NX; ++i) X[i] = x[i] + cs * h * kx[i];
                    ModelEvalT<double> e;
                    model_eval<double>(cf, X, u, pin, e);
#pragma unroll
                    for (int i = 0; i < NX; ++i) { kx[i] = e.f[i]; accx[i] += ws * e.f[i]; }
                    if (live && g == 0) {
                        double2* jt = reinterpret_cast<double2*>(JT + k * FusedLds::JTK + s * FusedLds::JTS);
                        jt[0] = make_double2(e.j0[0], e.j0[1]); jt[1] = make_double2(e.j0[2], e.j1[0]); jt[2] = make_double2(e.j1[1], e.j1[2]);
#pragma unroll
                        for (int r = 0; r < 3; ++r) { jt[3 + 2 * r] = make_double2(e.a[r][0], e.a[r][1]); jt[4 + 2 * r] = make_double2(e.a[r][2], e.a[r][3]); }
#pragma unroll
                        for (int r = 0; r < 3; ++r) jt[9 + r] = make_double2(e.bu[r][0], e.bu[r][1]);
                    }
                }
                if (live && g == 0) {
#pragma unroll
                    for (int i = 0; i < NX; ++i) bl[k * NX + i] = (x[i] + h * accx[i]) - xn1[i];
                }
            }
            WSYNC();
        F20_STAMP(1);
            // ---- A2: the sensitivity columns of the lane's group from the tabled Jacobians (text of rk4_group / sens_rhs)
            {
                const int xcol0 = g == 0 ? 2 : 5;
                double kS[3][NX], accS[3][NX];
#pragma unroll
                for (int cc = 0; cc < 3; ++cc)
#pragma unroll
                    for (int i = 0; i < NX; ++i) { kS[cc][i] = 0.0; accS[cc][i] = 0.0; }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const double cs = (s == 0) ? 0.0 : (s == 3 ? 1.0 : 0.5);
                    const double ws = (s == 0 || s == 3) ? (1.0 / 6.0) : (2.0 / 6.0);
                    double S[3][NX];
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc)
#pragma unroll
                        for (int i = 0; i < NX; ++i) {
                            const double id = (g < 2 && i == xcol0 + cc) ? 1.0 : 0.0;
                            S[cc][i] = id + cs * h * kS[cc][i];
                        }
                    ModelEvalT<double> e;
                    {
                        const double2* jt = reinterpret_cast<const double2*>(JT + k * FusedLds::JTK + s * FusedLds::JTS);
                        double2 q;
                        q = jt[0]; e.j0[0] = q.x; e.j0[1] = q.y; q = jt[1]; e.j0[2] = q.x; e.j1[0] = q.y; q = jt[2]; e.j1[1] = q.x; e.j1[2] = q.y;
#pragma unroll
                        for (int r = 0; r < 3; ++r) { q = jt[3 + 2 * r]; e.a[r][0] = q.x; e.a[r][1] = q.y; q = jt[4 + 2 * r]; e.a[r][2] = q.x; e.a[r][3] = q.y; }
#pragma unroll
                        for (int r = 0; r < 3; ++r) { q = jt[9 + r]; e.bu[r][0] = q.x; e.bu[r][1] = q.y; }
                    }
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) {
                        sens_rhs<double>(e, S[cc], g == 2 ? cc : -1, kS[cc]);
#pragma unroll
                        for (int i = 0; i < NX; ++i) accS[cc][i] += ws * kS[cc][i];
                    }
                }
                // packed stage record: stored columns c = 0..6 <-> (A[:,2..6], B[:,0..1]), rows 0..5 of each
                const int c0 = g == 0 ? 0 : (g == 1 ? 3 : 5);
                const int nc = g == 0 ? 3 : 2;
                WSYNC();                                   // REQUIRED: GT overlays the Jacobian tables (FusedLds: oGT = oJT = 0) -- every lane has read its
                                                           // tables before the first store.  With ADMPC_WSYNC_FENCE_ONLY this is a wave-level fence: the
                                                           // kernel must stay ONE wave per workgroup (launch bounds below)
                double* Gk = GT + k * GTS;
#pragma unroll
                for (int cc = 0; cc < 3; ++cc)
                    if (live && cc < nc)
#pragma unroll
                        for (int i = 0; i < 6; ++i) {
                            const double id = (g < 2 && i == xcol0 + cc) ? 1.0 : 0.0;
                            Gk[(c0 + cc) * 6 + i] = id + h * accS[cc][i];
                        }
            }
            WSYNC();
        }

        // =================================================================================================================
        // phase C (H2-H4): condensing, lane i <-> input i = 2k + j.  Leaves the packed
        // Hessian rows in Hp and, in registers, g0 (reduced gradient at du = 0) and xhat6 of the lane's stage.
        // =================================================================================================================
        F20_STAMP(2);
        double g0, xh6_own = 0.0;
        {
            LAUNDER_LANE(lane); LAUNDER_CFG(cf);
            const int ki = lane >> 1, ji = lane & 1;
            const bool uact = lane < n;
            const int sc = uact ? lane : 0;
            const double Ts = cf->Ts, h = cf->Ts;
            const double Rj = Ts * cf->W[NX + ji];
            stage_dq<N>(dqC, xbg, yrg, yrefeg + (size_t)inst * NX, lane);
            const double ubar_i = ubg[sc];
            const double r_i = Rj * (ubar_i - yrg[(sc >> 1) * 9 + 7 + (sc & 1)]);
            double Qd[NX], Qe[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) { Qd[i] = Ts * cf->W[i]; Qe[i] = cf->We[i]; }
            // the carried columns in two sets used alternately (stage k reads set k & 1 and writes the other one): with one set the
            // results of a stage were copied into it behind every stage (the stages are separate basic blocks: ten v_mov_b64 each)
            double xh0[NX], g2[2][NX];
#pragma unroll
            for (int c = 0; c < NX; ++c) xh0[c] = x0g[(size_t)inst * NX + c] - xbg[c];      // uniform
            WSYNC();
#pragma unroll
            for (int c = 0; c < NX; ++c) { g2[0][c] = lane == n ? xh0[c] : 0.0; g2[1][c] = 0.0; }      // lane 40: xhat_0 = x0 - xbar_0
            // H on the matrix pipe: six 16 x 16 tiles (I >= J) of v_mfma_f64_16x16x4_f64.  One MFMA step takes K = 4 rows of the
            // 60 x 40 matrix G whose rows are the weighted components of Gamma_k: per stage the components of QMASK, four at a time
            // (QMASK 7: x, y, psi + a zero row).  Operand layout: lane = index + 16 * k  ->  lane >> 4 picks the component, lane & 15
            // the column inside the block; operands come from the LDS exchange buffer gam.  The matrix
            // pipe is otherwise idle and runs under the propagation FMAs: 1260 v_fmac_f64_dpp per instance leave the vector pipe
            // (measured in isolation: 13.4 -> 10.1 us per instance, profiles/r3/mfma_condense_ab.txt).
            constexpr int NCOMP = ((QMASK >> 0) & 1) + ((QMASK >> 1) & 1) + ((QMASK >> 2) & 1) + ((QMASK >> 3) & 1) + ((QMASK >> 4) & 1) + ((QMASK >> 5) & 1) + ((QMASK >> 6) & 1);
            constexpr int NSTEP = (NCOMP + 3) / 4;
            const int r16 = lane & 15, kq = lane >> 4;
            int crow[NSTEP]; double wq_l[NSTEP], we_l[NSTEP];       // per MFMA step: this lane's component (7 = the zero row) and its weights
            {
                int seen = 0;
#pragma unroll
                for (int st_ = 0; st_ < NSTEP; ++st_) { crow[st_] = 7; wq_l[st_] = 0.0; we_l[st_] = 0.0; }
                static_for<0, NX>([&](auto cc) __attribute__((always_inline)) {
                    constexpr int c = decltype(cc)::value;
                    if constexpr ((QMASK >> c) & 1) {
                        const int st_ = seen >> 2, kk = seen & 3;          // compile-time after unrolling
#pragma unroll
                        for (int q_ = 0; q_ < NSTEP; ++q_) if (q_ == st_ && kq == kk) { crow[q_] = c; wq_l[q_] = Qd[c]; we_l[q_] = Qe[c]; }
                        ++seen;
                    }
                });
            }
            gam[7 * 64 + lane] = 0.0;                                // the zero row (gam has room for an eighth row)
            // What a stage addresses per lane does not change during the instance, or changes from stage to stage by a compile-time
            // constant: formed here once, as LDS byte addresses, and laundered; a stage adds offsets only and keeps one compare and one
            // select for "is this my stage".
            //   a_bown  the lane's own column of B_k (its stage is ki), a_zero the zero row, a_bl / a_bls base and stride of lane 40's b_k
            //   (the zero row and 0 elsewhere), a_aq the two A_k operand reads, a_gst the gam store, a_uni the uniform reads (dq, what lane 40
            //   published in gam), a_cr the MFMA operand reads crow * 64 + r16, h6 the lane's entry of row 6 of B
            unsigned a_bown = lds_byte_addr(GT + ki * GTS + 5 * 6 + 6 * ji), a_zero = lds_byte_addr(gam + 7 * 64);
            unsigned a_bl = lane == n ? lds_byte_addr(bl) : a_zero;
            int a_bls = lane == n ? 7 * 8 : 0;
            unsigned a_aq0 = lds_byte_addr(GT + r16), a_aq1 = lds_byte_addr(GT + 16 + (r16 < 14 ? r16 : 13));
            unsigned a_gst = lds_byte_addr(gam + lane), a_uni = lds_byte_addr(gam + n) - 3 * 512;
            unsigned a_cr[NSTEP];
#pragma unroll
            for (int st_ = 0; st_ < NSTEP; ++st_) { a_cr[st_] = lds_byte_addr(gam + crow[st_] * 64 + r16); asm volatile("" : "+v"(a_cr[st_])); }
            double h6 = ji ? h : 0.0;
            asm volatile("" : "+v"(a_bown), "+v"(a_zero), "+v"(a_bl), "+v"(a_bls), "+v"(a_aq0), "+v"(a_aq1), "+v"(a_gst), "+v"(a_uni), "+v"(h6));
            // (a_uni: three rows of gam in front of gam[0][n], so that the reads of gam[c][n] are whole multiples of 512 B away from it -- what
            // ds_read2st64_b64 encodes without an address add -- and dq stays inside the 8-bit offsets of ds_read2_b64)
            constexpr int oUniGam = (3 * 64 - n) * 8, oUniDq = oUniGam - (FusedLds::oGam - FusedLds::oDqC) * 8;      // gam[0][0] and dq[0] seen from a_uni
            static_assert(oUniDq >= 0 && oUniDq + ((N + 1) * NX - 1) * 8 <= 255 * 8, "phase C: dq within ds_read2_b64's offsets from a_uni");
            d4 acc[3][3];
#pragma unroll
            for (int I = 0; I < 3; ++I)
#pragma unroll
                for (int J = 0; J < 3; ++J) acc[I][J] = d4{0.0, 0.0, 0.0, 0.0};
            g0 = r_i;
            static_for<0, N + 1>([&](auto kc) __attribute__((always_inline)) {
                constexpr int k = decltype(kc)::value;
                constexpr int lim = 2 * k < n ? 2 * k : n;        // inputs of stages < k (even)
                constexpr int nblk = (lim + 15) / 16;             // 16-lane blocks of Gamma that are non-zero at this stage
                double (&g)[NX] = g2[k & 1];
                double (&gn)[NX] = g2[(k + 1) & 1];
                // One stage = one basic block (an always-true test the compiler cannot see through): merged into one 21-stage block,
                // hipcc hoists every LDS load of the whole instance and spills ~1600 registers.
                int tok = B; asm volatile("" : "+s"(tok));
                if (tok > 0) {
                double wg[NX];
                double blk[NSTEP][3];
                // Every LDS read of the stage's record is issued before anything else of the stage: left to itself hipcc keeps one or two
                // ds_read_b128 in flight and the propagation (60 multiply-adds behind 21 reads) waits on each of them in turn.
                double2 Bv[3]; double blv[NX], Aq[2];
                const bool mine_p = ki == k;
                if constexpr (k < N) {
                    // (32-bit LDS addresses, not selected pointers: hipcc turns a select of two LDS pointers into flat pointers and
                    // converts every element address back with a null check -- five scalar instructions per load)
                    const unsigned baddr = mine_p ? a_bown : a_zero;
                    Aq[0] = lds_ld(a_aq0, k * GTS * 8); Aq[1] = lds_ld(a_aq1, k * GTS * 8);
#pragma unroll
                    for (int q_ = 0; q_ < 3; ++q_) Bv[q_] = lds_ld2(baddr, 16 * q_);
                    const unsigned laddr = a_bl + (unsigned)__mul24(a_bls, k);      // b_k for the column of the free response, zeros for the others
#pragma unroll
                    for (int r = 0; r < NX; ++r) blv[r] = lds_ld(laddr, 8 * r);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (k >= 1) {
                    static_for<0, NX>([&](auto cc) __attribute__((always_inline)) {
                        constexpr int c = decltype(cc)::value;
                        if constexpr ((QMASK >> c) & 1) {
                            const double w = k < N ? Qd[c] : Qe[c];
                            wg[c] = w * g[c];
                            lds_st(a_gst, c * 512, g[c]);
                        }
                    });
                    if constexpr (!((QMASK >> 6) & 1)) lds_st(a_gst, 6 * 512, g[6]);      // xhat_k[6] for the steering rows
                    static_for<0, NX>([&](auto cc) __attribute__((always_inline)) {
                        constexpr int c = decltype(cc)::value;
                        if constexpr ((QMASK >> c) & 1) g0 += wg[c] * (lds_ld(a_uni, oUniGam + (c * 64 + n) * 8) + lds_ld(a_uni, oUniDq + (k * 7 + c) * 8));      // lane 40 has just published xhat_k[c]
                    });
                    { double x6 = lds_ld(a_uni, oUniGam + (6 * 64 + n) * 8); asm volatile("" : "+v"(x6)); xh6_own = lane == k ? x6 : xh6_own; }      // (an unconditional load)
#pragma unroll
                    for (int st_ = 0; st_ < NSTEP; ++st_)
#pragma unroll
                        for (int m = 0; m < nblk; ++m) blk[st_][m] = lds_ld(a_cr[st_], 16 * m * 8);
                }
                if constexpr (k < N) {
                    // The inputs of stage k enter with B_k: lanes 2k, 2k + 1 (whose column of Gamma is still zero) start the product from
                    // their column of B_k, every other lane from the zero row of gam -- one per-lane LDS address instead of 28 selects
                    // per stage (560 vector instructions per instance); 0 + A_k 0 = 0 exactly: the same bits as the selects gave.
                    const bool mine = ki == k;
#pragma unroll
                    for (int r = 0; r < 6; r += 2) { gn[r] = Bv[r / 2].x; gn[r + 1] = Bv[r / 2].y; }
                    gn[0] += g[0]; gn[1] += g[1];
                    gn[6] = mine ? h6 : g[6];
#pragma unroll
                    for (int r = 0; r < NX; ++r) gn[r] += blv[r];                  // b_k in lane 40, + 0.0 elsewhere
                    static_for<0, 5>([&](auto cc) __attribute__((always_inline)) {
                        constexpr int c = decltype(cc)::value;
                        static_for<0, 6>([&](auto rc) __attribute__((always_inline)) {
                            constexpr int r = decltype(rc)::value, q_ = c * 6 + r;
                            fmac_rowbc_ld<q_ % 16>(gn[r], Aq[q_ / 16], g[c + 2]);      // gn[r] += A_k[r][c + 2] g[c + 2]
                        });
                    });
                }
                if constexpr (k >= 1) {
                    // H[I][J] += (W G_I)' G_J for the tiles whose columns are non-zero already (inputs of stages < k): I, J < nblk, I >= J
#pragma unroll
                    for (int st_ = 0; st_ < NSTEP; ++st_) {
                        const double wl = k < N ? wq_l[st_] : we_l[st_];
                        static_for<0, nblk>([&](auto Ic) __attribute__((always_inline)) {
                            constexpr int I = decltype(Ic)::value;
                            const double a = wl * blk[st_][I];
                            static_for<0, I + 1>([&](auto Jc) __attribute__((always_inline)) {
                                constexpr int J = decltype(Jc)::value;
                                acc[I][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, blk[st_][J], acc[I][J], 0, 0, 0);
                            });
                        });
                    }
                }
                }
            });
            // the tiles into the packed lower-triangular rows: element (row = lane >> 4 + 4 v, column = lane & 15) of tile (I, J)
#pragma unroll
            for (int I = 0; I < 3; ++I)
#pragma unroll
                for (int J = 0; J <= I; ++J)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int row = 16 * I + kq + 4 * v, col = 16 * J + r16;
                        if (row < n && col <= row) Hp[row * (row + 1) / 2 + col] = acc[I][J][v];
                    }
            WSYNC();
            // H to the wave's slot: the factor of the trial takes its buffer.  The stores retire under the trial; the first fetch (phase D)
            // waits for them.
            stage_in<FusedLds::NTRI>(slot, Hp, lane);
        }

        // =================================================================================================================
        // phase D (H5): unconstrained trial + interior point on the condensed QP
        // =================================================================================================================
        F20_STAMP(3);
        {
            LAUNDER_LANE(lane); LAUNDER_CFG(cf);
            const int ki = lane >> 1, ji = lane & 1;
            const bool uact = lane < n;
            const bool dact = lane >= 1 && lane < N;
            const int sc = uact ? lane : 0;
            const double Ts = cf->Ts, h = cf->Ts;
            const double Rj = Ts * cf->W[NX + ji];
            const double rho_l = Ts * cf->zl, rho_u = Ts * cf->zu;
            const double thr = cf->ipm_thr0, mu0 = cf->ipm_mu0;
            const double tol_comp = cf->ipm_tol_comp, tol_res = cf->ipm_tol_res, tol_step = cf->ipm_tol_step;
            const int itmax = cf->ipm_iter_max;
            const bool try_unc = cf->ipm_try_unconstrained != 0.0;
            const double thw = cf->ipm_warm_thr, wrest = cf->ipm_warm_restart;
            const int fbit = (int)cf->ipm_fallback_iter;
            const double inv_nineq = 1.0 / (double)(8 * N + 2 * (N - 1));
            const double ubar_i = ubg[sc];
            const double dl_i = cf->lbu[ji] - ubar_i, duu_i = cf->ubu[ji] - ubar_i;
            double t[4], lam[4], sl = thr, su = thr;
            {
                const double r0[4] = { thr - dl_i, thr + duu_i, thr, thr };
#pragma unroll
                for (int i = 0; i < 4; ++i) { t[i] = r0[i] > thr ? r0[i] : thr; lam[i] = mu0 * rcp_nr(t[i]); }
            }
            double Dt[2] = {1.0, 1.0}, Dlam[2] = {0.0, 0.0}, Ddl = 0.0, Ddu = 0.0, dx6 = 0.0;
            if (dact) {
                const double x6 = xbg[lane * 7 + 6];
                Ddl = cf->lbx_delta - x6; Ddu = cf->ubx_delta - x6;
                dx6 = xh6_own;
                const double r0[2] = { dx6 - Ddl, Ddu - dx6 };
#pragma unroll
                for (int i = 0; i < 2; ++i) { Dt[i] = r0[i] > thr ? r0[i] : thr; Dlam[i] = mu0 * rcp_nr(Dt[i]); }
            }
            PK_DL = dl_i; PK_DUU = duu_i; PK_G0 = g0; PK_DDL = Ddl; PK_DDU = Ddu;      // parked in LDS: registers are the scarce resource
            if (try_unc) sb2[lane] = uact ? -g0 : 0.0;                                 // the trial's right-hand side: row 40 of its factorisation
            WSYNC();

            double rmax_prev = 0.0, stp_local = 1e300, alpha_prev = 1.0;
            bool solved = false, warmed = false, cons = false;
            if (try_unc) {
                int lt = lane; asm volatile("" : "+v"(lt));
                factorise(uact ? Rj : 1.0, 0.0, lt, std::integral_constant<int, 2>{});
                const double xt = dense40_solve_back(W, lt);
                const double duc = uact ? xt : 0.0;
                cb[lane] = duc;
                WSYNC();
                const double du1_stage = lane < N ? cb[2 * lane + 1] : 0.0;
                const double pre = wave_scan_incl32<OpSum>(du1_stage);       // lanes >= 20 hold 0.0; used in lanes < 20
                const double dx6c = xh6_own + h * (pre - du1_stage);
                const bool ok = (!uact || (duc >= dl_i && duc <= duu_i)) && (!dact || (dx6c >= Ddl && dx6c <= Ddu));
                WSYNC();
                if (__all(ok)) { du = duc; solved = true; }
                else if (thw > 0.0) {
                    warmed = true;
                    du = duc;
                    sl = fmax(dl_i - duc, 0.0) + thw; su = fmax(duc - duu_i, 0.0) + thw;
                    const double r0[4] = { duc + sl - dl_i, su + duu_i - duc, sl, su };
#pragma unroll
                    for (int i = 0; i < 4; ++i) { t[i] = r0[i] > thw ? r0[i] : thw; lam[i] = mu0 * rcp_nr(t[i]); }
                    if (dact) {
                        dx6 = dx6c;
                        const double q0[2] = { dx6 - Ddl, Ddu - dx6 };
#pragma unroll
                        for (int i = 0; i < 2; ++i) { Dt[i] = q0[i] > thw ? q0[i] : thw; Dlam[i] = mu0 * rcp_nr(Dt[i]); }
                    }
                }
            }
            auto cold_start = [&]() __attribute__((always_inline)) {
                const double dlc = PK_DL, duc2 = PK_DUU;
                du = 0.0; sl = thr; su = thr;
                const double r0[4] = { thr - dlc, thr + duc2, thr, thr };
#pragma unroll
                for (int i = 0; i < 4; ++i) { t[i] = r0[i] > thr ? r0[i] : thr; lam[i] = mu0 * rcp_nr(t[i]); }
                dx6 = dact ? xh6_own : 0.0;
                const double q0[2] = { dx6 - PK_DDL, PK_DDU - dx6 };
#pragma unroll
                for (int i = 0; i < 2; ++i) { Dt[i] = dact ? (q0[i] > thr ? q0[i] : thr) : 1.0; Dlam[i] = dact ? mu0 * rcp_nr(Dt[i]) : 0.0; }
                alpha_prev = 1.0; stp_local = 1e300;
            };
        F20_STAMP(4);
            F20_TRACE_MID();
            if (!solved && try_unc) {
                // H back from the slot: the trial's factor is dead.  Phase C's slot stores have retired (under the trial): the L2 holds this
                // instance's H.  The CU's vector L1 does not follow the wave's stores and may still hold the slot's lines that the PREVIOUS
                // instance of this wave fetched -- so every fetch is an sc1 load (slot_aux), served by the L2 without consulting the L1.
                // (Plain loads behind an agent-scope acquire, as kernel S reads its slot, measured 2 % slower at configs[1]: the L1 invalidate
                // is waited for by every iterating instance and drops the lines of the CU's other seven waves.)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                slot_fetch<FusedLds::NTRI, slot_aux>(Hp, slot, lane);
            }
            if (!solved)
            for (; it < itmax + (cons ? fbit : 0); ++it) {
                // An instance that is still iterating is on its way to becoming the batch's straggler: give its wave the issue slots of the
                // SIMD it shares (the partner is a fresh instance of the second round, which is not on anybody's critical path)
                // (priority 1 / 2 / 3 from iteration 0 / 2 / 4; measured: 0/2/4 -> 0.250 ms per step, 1/3/6 0.254, 3/6 only 0.255, none 0.269)
                if (it == 0) __builtin_amdgcn_s_setprio(1);
                if (it == 2) __builtin_amdgcn_s_setprio(2);
                if (it == 4) __builtin_amdgcn_s_setprio(3);
                int lz = lane;                          // laundered lane id: per-lane addresses / predicates derived from it are recomputed in
                asm volatile("" : "+v"(lz));            // place instead of being hoisted out of the loops
                const int trz = lz * (lz + 1) / 2;
                const bool uz = lz < n;
                double ru, mu, Dbar, S_i;
                {
                    double musum = 0.0, cmax = 0.0, rmax = 0.0;
                    const double i0 = rcp_nr(t[0]), i1 = rcp_nr(t[1]), i2_ = rcp_nr(t[2]), i3 = rcp_nr(t[3]);
                    const double G0 = lam[0] * i0, G1 = lam[1] * i1, G2 = lam[2] * i2_, G3 = lam[3] * i3;
#pragma unroll
                    for (int i = 0; i < 4; ++i) { const double rci = t[i] * lam[i]; musum += uact ? rci : 0.0; cmax = fmax(cmax, uact ? rci : 0.0); }
#pragma unroll
                    for (int i = 0; i < 2; ++i) { const double rci = Dt[i] * Dlam[i]; musum += dact ? rci : 0.0; cmax = fmax(cmax, dact ? rci : 0.0); }
                    const double Di0 = rcp_nr(Dt[0]), Di1 = rcp_nr(Dt[1]);
                    const double G56 = Dlam[0] * Di0 + Dlam[1] * Di1;
                    const double iG02 = rcp_nr(G0 + G2), iG13 = rcp_nr(G1 + G3);
                    Dbar = uact ? Rj + G0 * G2 * iG02 + G1 * G3 * iG13 : 1.0;       // idle lanes: identity rows
                    // The predictor's right-hand side depends on the iterate alone (pass 0 below: rc = t lam, the same formulas): all of it but
                    // ru and the suffix sum of e is ready here, and only these two values live across the mat-vec
                    double etal, etau;
                    {
                        const double rd0 = du + sl - PK_DL - t[0], rd1 = -du + su + PK_DUU - t[1], rd2 = sl - t[2], rd3 = su - t[3];
                        const double rsl = rho_l - lam[0] - lam[2], rsu = rho_u - lam[1] - lam[3];
                        const double c0 = (t[0] * lam[0]) * i0, c1 = (t[1] * lam[1]) * i1, c2 = (t[2] * lam[2]) * i2_, c3 = (t[3] * lam[3]) * i3;
                        const double e1 = rsl + c0 + c2 + G0 * rd0 + G2 * rd2;
                        const double e2 = rsu + c1 + c3 + G1 * rd1 + G3 * rd3;
                        etal = c0 + G0 * rd0 - G0 * e1 * iG02;
                        etau = -c1 - G1 * rd1 + G1 * e2 * iG13;
                        const double Drd0 = dx6 - PK_DDL - Dt[0], Drd1 = PK_DDU - dx6 - Dt[1];
                        const double ek = dact ? ((Dt[0] * Dlam[0]) * Di0 + (Dlam[0] * Di0) * Drd0) - ((Dt[1] * Dlam[1]) * Di1 + (Dlam[1] * Di1) * Drd1) : 0.0;
                        const double epref = wave_scan_incl32<OpSum>(ek);   // (the scans' operands are 0.0 from lane 20 on: five steps, total in lane 31)
                        invd[lane] = rdlane(epref, 31) - epref;             // suffix over stages > lane (read by lanes < 20); invd is free up to the factorisation
                    }
                    cb[lane] = uact ? du : 0.0;
                    const double dlam_pref = wave_scan_incl32<OpSum>(dact ? (Dlam[1] - Dlam[0]) : 0.0);     // lanes = stages
                    sb[lane] = rdlane(dlam_pref, 31) - dlam_pref;           // suffix over stages > lane
                    const double Ssuf_incl = wave_scan_incl32<OpSum>(dact ? G56 : 0.0);
                    sb2[lane] = rdlane(Ssuf_incl, 31) - Ssuf_incl;          // lane = stage: sum over stages > lane
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // H has landed (fetched in front of the loop or behind the last solve)
                    WSYNC();
                    double hdu = 0.0;
                    {
                        double Rd3[3];
#pragma unroll
                        for (int m = 0; m < 3; ++m) Rd3[m] = cb[16 * m + (lane & 15)];
                        double hv[n];
                        // no presets: lanes >= 40 load nothing, their hv, hdu and ru are stale register contents (possibly NaN).  Every use of
                        // ru is a select on uact: rmax, the predictor's and the corrector's right-hand side
                        sym_row_40_np(hv, lds_byte_addr(Hp + (uz ? trz : 0)), lds_byte_addr(Hp + (uz ? lz : 0)));
                        static_for<0, n>([&](auto cc) __attribute__((always_inline)) {
                            constexpr int c = decltype(cc)::value;
                            fmac_rowbc_ld<c % 16>(hdu, Rd3[c / 16], hv[c]);
                        });
                    }
                    ru = hdu + Rj * du + PK_G0 - lam[0] + lam[1] + (ji ? h * sb[uact ? ki : 0] : 0.0);
                    S_i = h * h * sb2[uact ? ki : 0];                        // lane = input: S_{k_i}
                    const double esuf = invd[uact ? ki : 0];
                    {
                        const double rd0 = du + sl - PK_DL - t[0], rd1 = -du + su + PK_DUU - t[1], rd2 = sl - t[2], rd3 = su - t[3];
                        const double rsl = rho_l - lam[0] - lam[2], rsu = rho_u - lam[1] - lam[3];
                        const double Drd0 = dx6 - PK_DDL - Dt[0], Drd1 = PK_DDU - dx6 - Dt[1];
                        double ra = OpMaxNan::f(fabs(ru), fabs(rsl)); ra = OpMaxNan::f(ra, fabs(rsu));
                        ra = OpMaxNan::f(ra, fabs(rd0)); ra = OpMaxNan::f(ra, fabs(rd1)); ra = OpMaxNan::f(ra, fabs(rd2)); ra = OpMaxNan::f(ra, fabs(rd3));
                        const double rb = OpMaxNan::f(fabs(Drd0), fabs(Drd1));
                        rmax = OpMaxNan::f(uact ? ra : 0.0, dact ? rb : 0.0);
                    }
                    mu = wave_reduce<OpSum>(musum) * inv_nineq;
                    rmax = wave_reduce<OpMaxNan0>(rmax);
                    // complementarity and step are only compared with their tolerances: a wave vote instead of a max-reduction each.  The
                    // reduction's fmax skips NaN operands and starts from 0.0, so a NaN lane must not veto (the negated greater-than) and the
                    // idle lanes' 0.0 and the first iteration's 1e300 vote like everybody else
                    const bool comp_ok = __all(!(cmax > tol_comp)), step_ok = __all(!(stp_local > tol_step));
                    if (!(mu == mu) || !(rmax == rmax)) { failed = true; break; }
                    if (comp_ok && step_ok &&
                        (rmax <= tol_res || (it > 0 && rmax > 0.1 * rmax_prev && rmax <= ADMPC_IPM_FLOOR_CAP * tol_res))) break;      // admpc.h: stopping test
                    rmax_prev = rmax;
                    // published behind the read of S_i (same wave, LDS in program order); the WSYNC in front of the factorisation orders
                    // it against lane 40's row build
                    sb2[lane] = uact ? -(ru + etal + etau + (ji ? h * esuf : 0.0)) : 0.0;
                }
                if (fbit > 0 && !cons && it >= fbit) {            // (no factorisation behind the fetch yet: H stays in LDS for the restart)
                    cons = true; warmed = false;
                    cold_start();
                    rmax_prev = 0.0;
                    --it;
                    continue;
                }
                WSYNC();
                factorise(Dbar, (uz && ji) ? S_i : 0.0, lz, std::integral_constant<int, 1>{});
#pragma unroll
                for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(t[i]), "+v"(lam[i]));
#pragma unroll
                for (int i = 0; i < 2; ++i) asm volatile("" : "+v"(Dt[i]), "+v"(Dlam[i]));
                double it_[4], il_[4], rc[4], Dit[2], Dil[2], Drc[2];
#pragma unroll
                for (int i = 0; i < 4; ++i) { it_[i] = rcp_nr(t[i]); il_[i] = rcp_nr(lam[i]); rc[i] = t[i] * lam[i]; }
#pragma unroll
                for (int i = 0; i < 2; ++i) { Dit[i] = rcp_nr(Dt[i]); Dil[i] = rcp_nr(Dlam[i]); Drc[i] = Dt[i] * Dlam[i]; }
                const double G0 = lam[0] * it_[0], G1 = lam[1] * it_[1], G2 = lam[2] * it_[2], G3 = lam[3] * it_[3];
                const double iG02 = rcp_nr(G0 + G2), iG13 = rcp_nr(G1 + G3);
                const double G5 = Dlam[0] * Dit[0], G6 = Dlam[1] * Dit[1];
                const double rd0 = du + sl - PK_DL - t[0], rd1 = -du + su + PK_DUU - t[1], rd2 = sl - t[2], rd3 = su - t[3];
                const double rsl = rho_l - lam[0] - lam[2], rsu = rho_u - lam[1] - lam[3];
                const double Drd0 = dx6 - PK_DDL - Dt[0], Drd1 = PK_DDU - dx6 - Dt[1];

                double mu_aff = 0.0, dsl = 0.0, dsu = 0.0, ddu = 0.0, dt[4], dlam[4], Ddt[2], Ddlam[2];
#pragma unroll 1
                for (int pass = 0; pass < 2; ++pass) {
                    const double c0 = rc[0] * it_[0], c1 = rc[1] * it_[1], c2 = rc[2] * it_[2], c3 = rc[3] * it_[3];
                    const double e1 = rsl + c0 + c2 + G0 * rd0 + G2 * rd2;
                    const double e2 = rsu + c1 + c3 + G1 * rd1 + G3 * rd3;
                    double z;
                    if (pass == 0) z = dense40_rhs_row(W, lz);                 // the predictor's forward solve came with the factorisation
                    else {
                        const double etal = c0 + G0 * rd0 - G0 * e1 * iG02;
                        const double etau = -c1 - G1 * rd1 + G1 * e2 * iG13;
                        const double ek = dact ? (Drc[0] * Dit[0] + G5 * Drd0) - (Drc[1] * Dit[1] + G6 * Drd1) : 0.0;
                        const double epref = wave_scan_incl32<OpSum>(ek);
                        sb[lane] = rdlane(epref, 31) - epref;
                        WSYNC();
                        const double y = uact ? -(ru + etal + etau + (ji ? h * sb[ki] : 0.0)) : 0.0;
                        z = dense40_solve_fwd(W, y, lz);
                    }
                    const double x = dense40_solve_bwd(W, z, lz);
                    if (pass == 1) slot_fetch<FusedLds::NTRI, slot_aux>(Hp, slot, lz);     // the factor is dead: next iteration's H under the step-length work
                    ddu = uact ? x : 0.0;
                    cb[lane] = ddu;
                    WSYNC();
                    const double du1_stage = lane < N ? cb[2 * lane + 1] : 0.0;
                    const double pre = wave_scan_incl32<OpSum>(du1_stage);       // lanes >= 20 hold 0.0; used in lanes < 20
                    const double ddx6 = h * (pre - du1_stage);
                    dsl = -(e1 + G0 * ddu) * iG02;
                    dsu = -(e2 - G1 * ddu) * iG13;
                    dt[0] = ddu + dsl + rd0; dt[1] = -ddu + dsu + rd1; dt[2] = dsl + rd2; dt[3] = dsu + rd3;
                    const double Gs[4] = { G0, G1, G2, G3 };
                    double rr = 0.0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        dlam[i] = -rc[i] * it_[i] - Gs[i] * dt[i];
                        rr = fmax(rr, uact ? fmax(-dt[i] * it_[i], -dlam[i] * il_[i]) : 0.0);
                    }
                    Ddt[0] = ddx6 + Drd0;  Ddlam[0] = -Drc[0] * Dit[0] - G5 * Ddt[0];
                    Ddt[1] = -ddx6 + Drd1; Ddlam[1] = -Drc[1] * Dit[1] - G6 * Ddt[1];
#pragma unroll
                    for (int i = 0; i < 2; ++i) rr = fmax(rr, dact ? fmax(-Ddt[i] * Dit[i], -Ddlam[i] * Dil[i]) : 0.0);
                    rr = wave_reduce<OpMax0>(rr);
                    const double amax = rr > 1.0 ? rcp_nr(rr) : 1.0;
                    if (pass == 0) {
                        double s_aff = 0.0;
#pragma unroll
                        for (int i = 0; i < 4; ++i) s_aff += uact ? (t[i] + amax * dt[i]) * (lam[i] + amax * dlam[i]) : 0.0;
#pragma unroll
                        for (int i = 0; i < 2; ++i) s_aff += dact ? (Dt[i] + amax * Ddt[i]) * (Dlam[i] + amax * Ddlam[i]) : 0.0;
                        mu_aff = wave_reduce<OpSum>(s_aff) * inv_nineq;
                        double sigma = mu_aff * rcp_nr(mu); sigma = sigma * sigma * sigma;
                        if (alpha_prev < ADMPC_IPM_BLOCKED_STEP) sigma = 1.0;      // centring safeguard (admpc.h)
                        const double smu = fmax(sigma * mu, ADMPC_IPM_MU_FLOOR * tol_comp);      // admpc.h: centring target floor
                        if (!cons) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) rc[i] = t[i] * lam[i] + dt[i] * dlam[i] - smu;
#pragma unroll
                            for (int i = 0; i < 2; ++i) Drc[i] = Dt[i] * Dlam[i] + Ddt[i] * Ddlam[i] - smu;
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i) rc[i] = t[i] * lam[i] - smu;
#pragma unroll
                            for (int i = 0; i < 2; ++i) Drc[i] = Dt[i] * Dlam[i] - smu;
                        }
                    } else {
                        double tau = 1.0 - mu_aff; tau = fmax(tau, 0.995); tau = fmin(tau, 0.999999);
                        const double alpha = fmin(tau * amax, 1.0);
                        if (it == 0 && warmed && alpha < wrest) {      // (H is on its way from the slot, as for any next iteration)
                            warmed = false;
                            cold_start();
                        } else {
                        alpha_prev = alpha;
                        stp_local = uact ? fabs(alpha * ddu) : 0.0;
#pragma unroll
                        for (int i = 0; i < 4; ++i) { t[i] = fmax(t[i] + alpha * dt[i], IPM_FLOOR); lam[i] = fmax(lam[i] + alpha * dlam[i], IPM_FLOOR); }
                        du += alpha * ddu; sl += alpha * dsl; su += alpha * dsu;
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            Dt[i] = dact ? fmax(Dt[i] + alpha * Ddt[i], IPM_FLOOR) : 1.0;
                            Dlam[i] = dact ? fmax(Dlam[i] + alpha * Ddlam[i], IPM_FLOOR) : 1.0;
                        }
                        dx6 += dact ? alpha * ddx6 : 0.0;
                        }
                    }
                    WSYNC();
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // an iteration limit leaves the last fetch in flight: phase E (dx, du)
        }                                                                   // and the next instance's phase A write into its destination
        F20_STAMP(5);
        { LAUNDER_LANE(lw); if (lw == 0 && itersg) itersg[inst] = it; }
        if (failed) {
            // non-finite QP data: acados returns before the update -- the iterate stays as it is, status 4, cost +inf
            { LAUNDER_LANE(lw); if (lw == 0) { statusg[inst] = ADMPC_STATUS_QP_FAILURE; if (costg) costg[inst] = INFINITY; } }
            WSYNC();
            __builtin_amdgcn_s_setprio(0);
            continue;
        }

        // =================================================================================================================
        // phase E (H6): expand the states through the linearised dynamics, full step, cost, status
        // =================================================================================================================
        {
            LAUNDER_LANE(lane); LAUNDER_CFG(cf);
            const int ji = lane & 1;
            const bool uact = lane < n;
            const int sc = uact ? lane : 0;
            const double Ts = cf->Ts, h = cf->Ts;
            const double Rj = Ts * cf->W[NX + ji];
            const double rho_l = Ts * cf->zl, rho_u = Ts * cf->zu;
            const int r6 = lane < 6 ? lane : 0;                     // row of the packed linearisation this lane reads
            const int r7 = lane < NX ? lane : 0;
            const double wq = lane < NX ? Ts * cf->W[r7] : 0.0, wqe = lane < NX ? cf->We[r7] : 0.0;
            int tk_v = 0;
            if (cap != 0 && lane == 0) tk_v = atomicAdd(sched, 1);       // the next ticket: its trip to the L2 runs under the expansion
            WSYNC();
            stage_dq<N>(dqE, xbg, yrg, yrefeg + (size_t)inst * NX, lane);
            du = uact ? du : 0.0;
            dus[lane] = du;
#pragma unroll
            for (int q_ = 0; q_ < FusedLds::nZeroE; q_ += WAVE) lds_raw[FusedLds::oZeroE + q_ + lane] = 0.0;
            const double ubar_i = ubg[sc];
            const double uref_i = yrg[(sc >> 1) * 9 + 7 + (sc & 1)];
            double dx = lane < NX ? x0g[(size_t)inst * NX + r7] - xbg[r7] : 0.0;      // dx_0 (lanes 0..6)
            WSYNC();
            bool bad = false;
            double J = 0.0;
            // Nothing a stage reads from LDS depends on the recursion: du, b_k and GT are final, and slot k of dq is read before dx_k
            // goes into it.  The operands of stage k are therefore read E_AHEAD stages ahead of it into a register ring (stage j issues the
            // reads of stage j + E_AHEAD in front of its own arithmetic; LDS answers in order, so the wait in front of stage k's arithmetic
            // is an lgkmcnt(n) that leaves the younger reads in flight): the chain dx_k -> dx_{k+1} -- a select, two adds, five
            // v_fmac_f64_dpp, two selects -- never waits for a read of its own stage.  Left to hipcc every stage issued its reads and waited
            // for them three times in a row, ~60 dependent LDS round trips per instance.  Every lane stores its dx (lanes >= 7 into a dump
            // area): a store under an EXEC mask made every stage a basic block of its own.  The sched_barriers keep each stage's reads and
            // the chain dx_k -> dx_{k+1} in their stage.  What is not on the chain hipcc sinks behind the recursion: the cost terms (e, J) and the
            // 21 tests of `bad` run there on the 21 dq and 21 dx register pairs it keeps live across the recursion (as in the build before the ring;
            // phase D's 248 VGPRs remain the kernel's peak, no spill).
            // One stage ahead: 7 reads of stage k, the store of stage k - 1 and 7 reads of stage k + 1 are 15 LDS instructions in flight, the most
            // lgkmcnt can count -- two stages ahead saturates the counter (the waits then cover younger reads too) and measured the same.
            constexpr int E_AHEAD = 1, E_RING = E_AHEAD + 1;
            struct ERing { double dq, bk, g[5], b0, b1, u0, u1; };
            ERing ring[E_RING];
            const int sidx = lane < NX ? FusedLds::oDqC + lane : FusedLds::oDumpE + lane;
            // Lanes >= 7 read b_k and du from the zeros and hold 0.0 in h6: their row-6 value fma(0.0, 0.0, 0.0 + 0.0) is exactly 0.0 whatever the
            // other lanes hold, so the next dx is ONE select (rows 0..5 or row 6) instead of two.  The addresses are formed once and laundered.
            unsigned a_bk = lds_byte_addr(lane < NX ? bl + lane : lds_raw + FusedLds::oZeroE);
            unsigned a_du = lds_byte_addr(lane < NX ? dus : lds_raw + FusedLds::oZeroE);
            double h6 = lane == 6 ? h : 0.0;
            asm volatile("" : "+v"(a_bk), "+v"(a_du), "+v"(h6));
            auto e_read = [&](auto kc) __attribute__((always_inline)) {
                constexpr int k = decltype(kc)::value;
                ERing& r = ring[k % E_RING];
                r.dq = dqE[k * 7 + r7];
                if constexpr (k < N) {
                    const double* Gk = GT + k * GTS;
                    // rows 0..5 from the packed record; every lane loads (lanes >= 6 read row 0 and drop the result): seven loads under their
                    // own EXEC masks were 18 scalar instructions per stage.  Row 6 of [A B] is [e6, 0, h]: one multiply-add in lane 6.
                    r.u0 = lds_ld(a_du, 16 * k); r.u1 = lds_ld(a_du, 16 * k + 8);
                    r.bk = lds_ld(a_bk, 56 * k);
#pragma unroll
                    for (int c = 0; c < 5; ++c) r.g[c] = Gk[c * 6 + r6];
                    r.b0 = Gk[5 * 6 + r6]; r.b1 = Gk[6 * 6 + r6];
                }
            };
            static_for<0, E_AHEAD>([&](auto kc) __attribute__((always_inline)) { e_read(kc); });
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, N + 1>([&](auto kc) __attribute__((always_inline)) {
                constexpr int k = decltype(kc)::value;
                if constexpr (k + E_AHEAD <= N) e_read(std::integral_constant<int, (k + E_AHEAD <= N ? k + E_AHEAD : N)>{});
                __builtin_amdgcn_sched_barrier(0);
                const ERing& r = ring[k % E_RING];
                const double e = dx + r.dq;
                J += 0.5 * (k < N ? wq : wqe) * e * e;
                if (!(fabs(dx) <= 1e300)) bad = true;
                lds_raw[sidx + k * 7] = dx;                       // slot k now holds dx_k
                if constexpr (k < N) {
                    const double u0 = r.u0, u1 = r.u1, bk = r.bk, b0 = r.b0, b1 = r.b1;
                    double acc = bk + (lane < 2 ? dx : 0.0);
                    acc += b0 * u0 + b1 * u1;
                    const double acc6 = fma(h6, u1, bk + dx);                 // lane 6; exactly 0.0 in lanes >= 7 (dx = 0.0 there, by induction)
                    // (the pad of the first multiply-add covers the write of dx; the others follow it through acc)
                    fmac_rowbc<2>(acc, dx, r.g[0]); fmac_rowbc_ld<3>(acc, dx, r.g[1]); fmac_rowbc_ld<4>(acc, dx, r.g[2]);
                    fmac_rowbc_ld<5>(acc, dx, r.g[3]); fmac_rowbc_ld<6>(acc, dx, r.g[4]);
                    dx = lane < 6 ? acc : acc6;
                }
                __builtin_amdgcn_sched_barrier(0);
            });
            int tk_e = -1;                                                // the list entry of the next ticket: loaded under the output stores
            if (cap != 0) {
                const int* const e = ticket_entry_addr(grid + __builtin_amdgcn_readfirstlane(tk_v), lane);
                if (e) tk_e = *e;
            }
            const double unew = ubar_i + du;
            if (uact && !(fabs(unew) <= 1e300)) bad = true;
            const int status = __any(bad) ? ADMPC_STATUS_QP_FAILURE : ADMPC_STATUS_SUCCESS;
            double Ju = 0.0;
            WSYNC();
            if (status == 0) {
#pragma unroll
                for (int i0 = 0; i0 < (N + 1) * NX; i0 += WAVE) { const int i = i0 + lane; if (i < (N + 1) * NX) xbg[i] = xbg[i] + dqE[i]; }
                if (uact) {
                    const double e = unew - uref_i;
                    Ju = 0.5 * Rj * e * e;
                    if (unew < cf->lbu[ji]) Ju += rho_l * (cf->lbu[ji] - unew);
                    if (unew > cf->ubu[ji]) Ju += rho_u * (unew - cf->ubu[ji]);
                    ubg[lane] = unew;
                }
            }
            const double Jt = wave_reduce<OpSum>(J + Ju);
            if (lane == 0) {
                if (costg) costg[inst] = status == 0 ? Jt : INFINITY;
                statusg[inst] = status;
            }
            WSYNC();
            if (cap != 0) next_inst = __builtin_amdgcn_readfirstlane(tk_e);
            F20_STAMP(6);
            F20_TRACE_END(inst);
        }
        __builtin_amdgcn_s_setprio(0);
    }
    F20_FLUSH();
    // ---- every wave has drawn exactly one ticket beyond the batch; the last one to leave clears tickets and bins for the next launch
    {
        LAUNDER_LANE(lane0);
        int gone = 0;
        if (lane0 == 0) gone = atomicAdd(sched + 1, 1);
        gone = __builtin_amdgcn_readfirstlane(gone);
        if (gone == grid - 1) { sched[lane0] = 0; sched[64 + lane0] = 0; __threadfence(); }
    }
#undef PK_DL
#undef PK_DUU
#undef PK_G0
#undef PK_DDL
#undef PK_DDU
}

}  // namespace

// ---- host side (called by admpc_solve_batch_ex in admpc_kernels.hip)
extern "C" {

__attribute__((visibility("hidden"))) int admpc_fused20_lds_bytes(void) { return FusedLds::total * (int)sizeof(double); }
// doubles of the per-wave slot buffers: one packed H per workgroup of the persistent grid (at most num_cu * 8)
__attribute__((visibility("hidden"))) size_t admpc_fused20_slot_doubles(int num_cu) { return (size_t)num_cu * 8 * FusedLds::NTRI; }

// debug builds only: read and clear the phase counters (all zero in the shipped build)
int admpc_debug_f20_ticks(unsigned long long* out16)
{
#ifdef ADMPC_PHASE_TIMERS
    unsigned long long z[16] = {0};
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_f20_ticks), sizeof z) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_f20_ticks), z, sizeof z) != hipSuccess) return -1;
    return 0;
#else
    for (int i = 0; i < 16; ++i) out16[i] = 0;
    return 1;
#endif
}

int admpc_debug_f20_trace(unsigned long long* out, int n_inst)
{
#if defined(ADMPC_PHASE_TIMERS) || defined(ADMPC_F20_TRACE)
    if (n_inst > 8192) n_inst = 8192;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_f20_trace), (size_t)n_inst * 4 * sizeof(unsigned long long)) != hipSuccess) return -1;
    return 0;
#else
    (void)out; (void)n_inst;
    return 1;
#endif
}

__attribute__((visibility("hidden"))) void admpc_fused20_prepare(void)
{
    // 19.1 KB per workgroup: below the 64 KB default, no opt-in needed; kept for symmetry with the other units
}

// sched ints of a handle that solves up to `cap` instances per call: TWO scheduler states used alternately (zeroed at allocation; the order kernel of a
// launch zeroes the header of the next launch's state, the last workgroup to leave re-arms its own: no memset in front of a launch -- a hipMemsetAsync
// there cost 2 us per step at configs[1] and 26 us at N = 40)
// one state: header and the bins' lists
__attribute__((visibility("hidden"))) size_t admpc_fused20_state_ints(int cap) { return (size_t)F20_HDR + (size_t)F20_NB * (size_t)cap; }
__attribute__((visibility("hidden"))) size_t admpc_fused20_sched_ints(int cap) { return 2 * admpc_fused20_state_ints(cap); }      // two states (work_order.h)

// grid: persistent, eight one-wave workgroups per CU (two waves per SIMD); slotbuf: admpc_fused20_slot_doubles(num_cu) doubles
__attribute__((visibility("hidden"))) void admpc_fused20_launch(int num_cu, hipStream_t st, const AdmpcConfig* d_cfg, int B, int qmask,
        const double* x0, const double* yref, const double* yref_e, const double* p, double* xbar, double* ubar,
        double* cost, int32_t* stat, int32_t* iters, int first, int* sched2, int cap, int flip, double* slotbuf)
{
    const int lds = FusedLds::total * (int)sizeof(double);
    int grid = num_cu * 8; if (grid > B) grid = B;
    // every launch pair is self-contained: ticket counter, exit counter and bin counts start from zero on the caller's stream (the last
    // workgroup to leave re-arms them as well; a launch that failed half-way, or a handle misused from two streams, cannot poison the next)
    const size_t one = admpc_fused20_state_ints(cap);
    int* const sched = sched2 + (flip ? one : 0);
    int* const sched_next = sched2 + (flip ? 0 : one);
    const int kcap = grid == B ? 0 : cap;      // the batch fits the grid: no work order (work_order.h: f20_next)
    if (kcap) hipLaunchKernelGGL(admpc_f20_order_kernel, dim3((B + 255) / 256), dim3(256), 0, st, d_cfg, B, x0, yref, yref_e, sched, cap, sched_next);
    if (qmask == 7)
        hipLaunchKernelGGL((admpc_fused20_kernel<7>), dim3(grid), dim3(WAVE), lds, st, d_cfg, B, x0, yref, yref_e, p, xbar, ubar, cost, stat, iters, first, sched, kcap, slotbuf);
    else
        hipLaunchKernelGGL((admpc_fused20_kernel<127>), dim3(grid), dim3(WAVE), lds, st, d_cfg, B, x0, yref, yref_e, p, xbar, ubar, cost, stat, iters, first, sched, kcap, slotbuf);
}

}
