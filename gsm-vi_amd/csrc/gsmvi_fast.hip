// Guard-free fast paths of the dense-covariance GSM update for gfx950.
//
// Selected by the ABI when D % 64 == 0, every leading dimension is even, every base pointer is
// 16-byte aligned and B is one of {16,32,64} for the covariance kernel (BASELINE configs c3, c5).  Everything else
// runs the guarded generic kernels of gsmvi_kernels.hip (same arithmetic, same reduction order
// inside a kernel family is NOT promised across the two families).
//
// These kernels are latency-bound at D=1024 (8 MB of covariance over 256 CUs = 32 KB per CU), so
// the design rule is: issue every global load of a workgroup in ONE batch, wait once, then MFMA,
// then store.  No data-dependent branch sits between a load and its use.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_small16.h"
#include <hip/hip_ext.h>

#define GSMVI_LAUNCH(kern, grid, block, shmem, st, ev, ...)                                         \
    do {                                                                                           \
        if (ev)                                                                                    \
            hipExtLaunchKernelGGL(kern, grid, block, shmem, st, (ev)[0], (ev)[1], 0, __VA_ARGS__); \
        else                                                                                       \
            hipLaunchKernelGGL(kern, grid, block, shmem, st, __VA_ARGS__);                         \
    } while (0)

// =====================================================================================
// Panel product partials:  Pp[kc][r][j] = sum_{i in rows(kc)} alpha (A[r][i] - shift[i]) M[i][j]
// Workgroup (512 threads) = 16 columns of M x 256-row chunks; wave w of 8 owns rows 32w..32w+31 of
// the chunk (two waves per SIMD: the fp64 MFMA pipe needs two to reach its ~46 TF) and MFMA k-slot
// ks of step s is row 32w + 4s + ks.  M (the D x D covariance / precision / factor) is
// streamed once from HBM as 128-B row segments straight into registers.  The left operand chunk
// A[:, 256 rows] (16*MT x 256 doubles) is loaded by the whole workgroup with fully coalesced 16-B
// accesses and staged in LDS ([row][258]: conflict-free ds_read_b64 for the MFMA A operand), because
// fragment-shaped loads of it touch 64 cache lines per instruction.
// Any even D (round 5; D % 64 == 0 until round 4): the one wave whose rows straddle row D re-reads row D - 1 for the rows
// beyond it (the A chunk is staged with zeros there).  M has ncols columns (any; ncols = D for the square matrices);
// slabs are nrows x ncols.
// =====================================================================================
// EXTRA = true adds the two optional pieces of gsmvi_panel_extras (gsmvi_ctx.h): right-operand rows taken from split-K slabs
// of a previous product (summed while they are loaded, so that product needs no finish launch), and a slab-summing side
// job shared by all workgroups (finishes the small Gram matrix of the factor path beside this launch's own work).
// RIDER = true (factor path, round 3): the launch carries ONE more workgroup -- x index gridDim.x - 1, (y, z) = (0, 0) -- that
// runs the 2B x 2B chain of the factor update (gsmf_small16_body) while the other workgroups form V Fm: the chain (31 us on one
// CU) does not depend on this product, only the update kernel behind both does, so the product and one launch boundary
// disappear from the iteration's critical path.  The chain's 142 KB of LDS become the launch's LDS size (one workgroup per
// CU for the product: it finishes long before the chain either way).
// RAG (round 5) = the clamped form for D % 64 != 0 or ncols % 16 != 0; RAG = false is the round-4 code, instruction for
// instruction (the clamps and the straddling-wave branch cost 6 - 11 % on the grid shapes when they were unconditional:
// scripts/cov_ab_rounds.py).
// PART (two-launch dense GSM update; A = G, M = S0, row blocks of NR samples with nrows % NR == 0, on the grid) = the launch also leaves
// PARTIAL DOTS beside its slab (arguments: the last comment of gsmvi_panel_extras): per (sample, strip of 16 columns, slab) the sum of G slab over the
// strip, and from the workgroups of slab 0 the sum of (mu0 - x) G.  The covariance kernel behind this launch re-reduces them in
// every workgroup (k_gsm_cov_sym<.., FROM_SLABS>), so the per-sample launch between the two and its record round trip are gone;
// the only ordering is the kernel boundary.  PART = false is the code as it was, instruction for instruction.
// QMW (round 10; PART on the 512-row-chunk grid (D / 16, 2, B / 16) only, knob "panel_qm_whole") = ONE Qm value per sample instead
// of D / 16 pieces that every covariance workgroup re-sums: the slab-1 workgroups with blockIdx.x < 16 have no Qm work, so
// workgroup (x, 1, z) takes sample b = 16 z + x, thread tid the 16-byte unit tid of G[b], X[b] and mu0 (loaded behind the M stream,
// where the pq_* loads are), forms (mu0 - x) g over its pair behind the store loop and the workgroup sums in a fixed order:
// row16_sum, the 32 row sums through LDS (the reduction buffer is free by then), one thread adds them in index order and writes
// Qm[b].  The slab-0 workgroups neither load X and mu0 nor form their pieces.
// STREAM (round 12; PART on the 512-row-chunk grid only, knob "panel_stream") = NSTAGE in {2, 4}: a wave loads the part of the left
// operand that it multiplies, in NSTAGE pieces along K, and starts each piece's MFMAs behind that piece alone -- no workgroup
// barrier and no wait for the other seven waves in front of the first MFMA (panel_stream_chunk below; two stages ship, DESIGN 8.1
// round 12).  0 = the code as it was, instruction for instruction; -1 = that code with its landing profile in the timeline's stamps.
// The chunk of a STREAM > 0 instance: wave w multiplies columns 64 w .. 64 w + 63 of the staged 16 x 512 chunk (ap = As + c * LDG +
// 64 w + ks, MFMA step s = columns 4 s .. 4 s + 3 of them), so stage q = steps q * 16 / NS .. is the block of 16 sample rows x
// 64 / NS columns at column 64 w + q * 64 / NS.  A wave-instruction loads RPI rows x UPR 16-byte units of it: lane l takes row
// i * RPI + l / UPR, unit l % UPR (NS = 4: 8 rows x 128 B), and writes it to the position the operand reads use.  The eight
// lanes of one ds_write_b128 group write eight consecutive units of one row = all 32 banks once: conflict-free.
// Issue order: G of stage 0, S0 of stage 0, G of stage 1, ... , the three partial-dot loads last; vmcnt counts in issue order, so
// the wait in front of stage q's staging leaves every load of the later stages outstanding.  Within a wave LDS operations
// execute in order and no wave reads what another wrote before the barrier in front of the cross-wave reduction, so a stage
// needs lgkmcnt(0) and a compiler barrier between its writes and its operand reads, nothing more.  The products enter the
// accumulator in the order s = 0 .. 15 as they do without STREAM: bit-identical slabs.
// Preconditions (the launcher checks them): D == 512 * gridDim.y (every wave's rows exist), nrows % 16 == 0.
// Stamp words 4 - 7 (thread 0): stage 0 staged, first MFMA issued, last stage staged (also word 1), last MFMA done.
template <int NS>
__device__ __forceinline__ void panel_stream_chunk(double* As, int D, int nrows, const double* __restrict__ A, int lda, double alpha,
                                                   const double* __restrict__ M, int ldm, const gsmvi_panel_extras& px,
                                                   unsigned long long* __restrict__ stamps, const unsigned long long t0, v4d& acc,
                                                   double& pq_g, double& pq_x, double& pq_m) {
    static_assert(NS == 2 || NS == 4, "stages of the streamed left operand");
    constexpr int LDG = 514;                       // as k_panel_fast<.., 512, ..>
    constexpr int UPR = 32 / NS;                   // 16-B units per row and stage
    constexpr int RPI = 64 / UPR;                  // rows per wave-instruction
    constexpr int IPS = 16 / RPI;                  // wave-instructions (units per lane) per stage
    constexpr int SPS = 16 / NS;                   // MFMA steps per stage
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, c = l & 15, ks = l >> 4;
    const int cbase = blockIdx.y * 512, r0 = blockIdx.z * 16, j = blockIdx.x * 16 + c;
    const int lrow = l / UPR, lcol = 64 * w + 2 * (l % UPR);       // this lane's row within an instruction, column within stage 0
    unsigned long long t4 = 0, t5 = 0, t6 = 0;
    v2d ga[NS][IPS];
    double m[16];
    unsigned okbits = 0;
    const double* mp = M + (size_t)(cbase + 64 * w + ks) * ldm + j;
#pragma unroll
    for (int q = 0; q < NS; ++q) {
#pragma unroll
        for (int i = 0; i < IPS; ++i) {
            const int grow = r0 + i * RPI + lrow, col = cbase + lcol + q * (64 / NS);
            const bool ok = grow < nrows && col < D;
            ga[q][i] = *reinterpret_cast<const v2d*>(A + (size_t)(grow < nrows ? grow : nrows - 1) * lda + (col < D ? col : 0));
            okbits |= (ok ? 1u : 0u) << (q * IPS + i);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = q * SPS; s < (q + 1) * SPS; ++s) m[s] = mp[(size_t)(4 * s) * ldm];
        __builtin_amdgcn_sched_barrier(0);
    }
    {                                              // the partial-dot loads, as k_panel_fast<.., PART> issues them: last
        const int prow = r0 + ((tid >> 4) & 15), pcol = blockIdx.x * 16 + (tid & 15);
        pq_g = A[(size_t)prow * lda + pcol];
        pq_x = px.sj_src[(size_t)prow * px.sj_len + pcol];     // X, ldx
        pq_m = px.msl[pcol];                                   // mu0
    }
    __builtin_amdgcn_sched_barrier(0);
    const double* ap = As + c * LDG + 64 * w + ks;
#pragma unroll
    for (int q = 0; q < NS; ++q) {
#pragma unroll
        for (int i = 0; i < IPS; ++i) {
            v2d v = ga[q][i];
            if (!((okbits >> (q * IPS + i)) & 1u)) v = (v2d){0.0, 0.0};
            v.x *= alpha; v.y *= alpha;
            *reinterpret_cast<v2d*>(&As[(i * RPI + lrow) * LDG + lcol + q * (64 / NS)]) = v;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // this wave's writes are in LDS; no other wave's are read
        __builtin_amdgcn_wave_barrier();
        if (stamps) { if (q == 0) t4 = __builtin_amdgcn_s_memrealtime(); if (q == NS - 1) t6 = __builtin_amdgcn_s_memrealtime(); }
        double av[SPS];
#pragma unroll
        for (int s = 0; s < SPS; ++s) av[s] = ap[q * (64 / NS) + 4 * s];
#pragma unroll
        for (int s = 0; s < SPS; ++s) {
            acc = GSMVI_MFMA_F64(av[s], m[q * SPS + s], acc);
            if (stamps && q == 0 && s == 0) t5 = __builtin_amdgcn_s_memrealtime();
        }
        __builtin_amdgcn_sched_barrier(0);         // stage q + 1's staging stays behind stage q's MFMAs
    }
    if (stamps) {                                  // (times are kept in registers until here: a stamp store would count in vmcnt)
        asm volatile("" ::"s"(__builtin_amdgcn_readfirstlane(__double2loint(acc[0]))) : "memory");   // the last MFMA's result exists
        const unsigned long long t7 = __builtin_amdgcn_s_memrealtime();
        const unsigned wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        if (tid == 0 && wg < GSMVI_STAMP_WG) {
            stamps[(size_t)wg * 8] = t0;           // the kernel's first instruction (round 15)
            stamps[(size_t)wg * 8 + 1] = t6;       // "left operand staged", as without STREAM: wave 0's last stage
            stamps[(size_t)wg * 8 + 4] = t4;
            stamps[(size_t)wg * 8 + 5] = t5;
            stamps[(size_t)wg * 8 + 6] = t6;
            stamps[(size_t)wg * 8 + 7] = t7;
        }
    }
}

template <int MT, bool HAS_SHIFT, int CHW, bool EXTRA, bool RIDER = false, bool RAG = false, bool PART = false, bool QMW = false,
          int STREAM = 0>
__device__ __forceinline__ void panel_fast_body(const unsigned long long t0, int D, int nrows, const double* __restrict__ A, int lda,
                                                const double* __restrict__ shift, double alpha,
                                                const double* __restrict__ M, int ldm,
                                                double* Pp, int chunks_per_wg, int ncols,
                                                unsigned long long* __restrict__ stamps, double* __restrict__ Out,
                                                int ldo, const double* __restrict__ addvec, const gsmvi_panel_extras& px) {
    // The body of k_panel_fast and of the preloaded entry points of gsmvi_fast_hot.hip (round 15).  t0 = the clock at the kernel's
    // first instruction: stamp word 0, written with the first later stamp -- no test of `stamps` stands in front of the loads.
    // timeline diagnostic: a kernel's slot holds GSMVI_STAMP_WG workgroups x 8 words; workgroups beyond it write nothing
    // (the empty asm keeps the test of `stamps` at the stamp: hoisted out of the chunk loop it stood, with a wait for the argument,
    // in front of the loads)
#define PSTAMP(k)                                                                                              \
    do {                                                                                                       \
        const unsigned wg_ = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;                   \
        unsigned long long* sp_ = stamps;                                                                      \
        asm volatile("" : "+s"(sp_));                                                                          \
        if (sp_ && threadIdx.x == 0 && wg_ < GSMVI_STAMP_WG) {                                                 \
            if ((k) == 1) sp_[(size_t)wg_ * 8] = t0;                                                           \
            sp_[(size_t)wg_ * 8 + (k)] = __builtin_amdgcn_s_memrealtime();                                     \
        }                                                                                                      \
    } while (0)
    constexpr int LDG = CHW + 2;                   // LDS row stride of the staged A chunk (doubles)
    constexpr int NR = 16 * MT;
    constexpr int RW = CHW / 8;                    // rows of the chunk per wave (8 waves)
    constexpr int NST = RW / 4;                    // MFMA steps per wave and chunk
    constexpr int U16 = CHW / 2;                   // 16-B units per staged row
    constexpr int UPT = NR * U16 / 512;            // staging units per thread
    constexpr int SMEM_P = (NR * LDG > 8 * NR * 17) ? NR * LDG : 8 * NR * 17;
    constexpr int SMEM = (RIDER && GSMF_SMALL16_LDS > SMEM_P) ? GSMF_SMALL16_LDS : SMEM_P;
    __shared__ __attribute__((aligned(16))) double As[SMEM];       // staging buffer, reused for the reduction
    if (RIDER && blockIdx.x == gridDim.x - 1) {                     // block-uniform
        if (blockIdx.y == 0 && blockIdx.z == 0)
            gsmf_small16_body(As, px.rd_n, px.rd_B, px.rd_Gp, px.rd_kcg, px.rd_Kmat, px.rd_coef, px.rd_bad, px.rd_stamps,
                              px.rd_jmode, px.rd_prior, px.rd_Pi, px.rd_R11, px.rd_W11);
        return;
    }
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, c = l & 15, ks = l >> 4;
    // (round 5: any even D and any ncols -- a column beyond the matrix is a clamped re-read whose result is not stored, a
    // row of M beyond D is a clamped re-read multiplied by the zeros the A chunk is staged with beyond D)
    const int jx = blockIdx.x * 16 + c;
    const int j = (RAG && jx >= ncols) ? ncols - 1 : jx;
    const int r0 = blockIdx.z * NR;

    v4d acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (v4d){0.0, 0.0, 0.0, 0.0};
    static_assert(!PART || (MT <= 2 && !RAG && !RIDER && !HAS_SHIFT), "partial dots: one pass of the store loop, on the grid");
    static_assert(!QMW || (PART && CHW == 512 && MT == 1), "whole-sample Qm: the 512-row-chunk product of the two-launch form");
    static_assert(STREAM == 0 || (PART && CHW == 512 && MT == 1 && !RAG && !RIDER && !EXTRA && !HAS_SHIFT && !QMW),
                  "streamed left operand: the 512-row-chunk product of the two-launch form");
    // STREAM = -1: the code of STREAM = 0 with the landing profile of its one load batch in stamp words 4 - 7 (launched only with the
    // timeline diagnostic on and "panel_stream" = 0, so that the instance without stamps stays what it was)
    constexpr bool LANDING = STREAM == -1;
    [[maybe_unused]] unsigned long long tl_first = 0, tl_last = 0, tl_s0 = 0;
    double pq_g = 0.0, pq_x = 0.0, pq_m = 0.0;     // PART: G, X, mu0 at this thread's (sample, column) of the store loop
    [[maybe_unused]] v2d wq_g, wq_x, wq_m;         // QMW: unit tid of G[b], X[b], mu0 in the workgroup that sums Qm[b]

    for (int ch = 0; ch < chunks_per_wg; ++ch) {
        if constexpr (STREAM > 0) {        // one chunk per workgroup (the launcher checks it)
            panel_stream_chunk<STREAM>(As, D, nrows, A, lda, alpha, M, ldm, px, stamps, t0, acc[0], pq_g, pq_x, pq_m);
            break;
        }
        const int cbase = (blockIdx.y * chunks_per_wg + ch) * CHW;          // block-uniform
        if (cbase >= D) break;
        const int wbase = cbase + w * RW;                                   // wave-uniform: 8 waves x RW rows
        const bool wave_in = wbase < D;
        // ---- every global load of this chunk in one batch: the left-operand chunk FIRST (it comes from L2 / the
        // Infinity Cache and has to pass through LDS and a barrier), the HBM stream of M behind it.  vmcnt counts in
        // issue order, so the staging below waits only for the A loads and MFMA step s only for m[0..s]: the LDS
        // staging and the first MFMA steps overlap the tail of the M stream (measured with the in-kernel timeline,
        // scripts/timeline2.py: the load phase and the MFMA phase used to be strictly serial).
        v2d ga[UPT];
        v2d gs[UPT];
        unsigned okbits = 0;
#pragma unroll
        for (int q = 0; q < UPT; ++q) {
            const int u = q * 512 + tid;
            const int row = u / U16, c16 = u % U16;
            const int grow = r0 + row;
            const int col = cbase + 2 * c16;
            const bool ok = grow < nrows && col < D;
            ga[q] = *reinterpret_cast<const v2d*>(A + (size_t)(grow < nrows ? grow : nrows - 1) * lda +
                                                  (col < D ? col : 0));
            if (HAS_SHIFT) gs[q] = *reinterpret_cast<const v2d*>(shift + (col < D ? col : 0));
            okbits |= (ok ? 1u : 0u) << q;     // the out-of-range select is applied at staging time: no use of a
        }                                      // loaded value may sit in front of the M stream's issue
        __builtin_amdgcn_sched_barrier(0);
        double m[NST];
        if (EXTRA && px.msl != nullptr && (wave_in ? wbase : 0) + ks >= px.msplit) {
            // wave-uniform when msplit is a multiple of the wave's row count (it is for B % 16 == 0); rows come in steps of 4,
            // so ks >= ... holds for all s of this lane once it holds for s = 0
            // (D % 16 == 0 on this path: the callers' K'' Tm product has D = 2B with B % 16 == 0)
            const double* sp = px.msl + (size_t)((wave_in ? wbase : 0) + ks - px.msplit) * px.ldsl + j;
            // (two compile-time bounds on the slab count, chosen block-uniformly: with the clamp to GSMVI_MAX_KC alone every
            // entry cost 8 loads whatever the count)
            if (px.kcm <= 4) {
                double t[NST][4];
#pragma unroll
                for (int s = 0; s < NST; ++s)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        t[s][q] = sp[(size_t)(q < px.kcm ? q : px.kcm - 1) * px.mstride + (size_t)(4 * s) * px.ldsl];
#pragma unroll
                for (int s = 0; s < NST; ++s) {
                    double a = 0.0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) a += (q < px.kcm) ? t[s][q] : 0.0;
                    m[s] = a;
                }
            } else {
                double t[NST][GSMVI_MAX_KC];
#pragma unroll
                for (int s = 0; s < NST; ++s)
#pragma unroll
                    for (int q = 0; q < GSMVI_MAX_KC; ++q)
                        t[s][q] = sp[(size_t)(q < px.kcm ? q : px.kcm - 1) * px.mstride + (size_t)(4 * s) * px.ldsl];
#pragma unroll
                for (int s = 0; s < NST; ++s) {
                    double a = 0.0;
#pragma unroll
                    for (int q = 0; q < GSMVI_MAX_KC; ++q) a += (q < px.kcm) ? t[s][q] : 0.0;
                    m[s] = a;
                }
            }
            if (px.mfin != nullptr && blockIdx.z == 0 && wave_in) {
                double* fp = px.mfin + (size_t)(wbase + ks - px.msplit) * px.ldfin + j;
#pragma unroll
                for (int s = 0; s < NST; ++s) fp[(size_t)(4 * s) * px.ldfin] = m[s];
            }
        } else if (!RAG || wbase + RW <= D) {      // wave-uniform: all RW rows of this wave exist (!RAG: D % 64 == 0, so a wave
            // beyond row D -- its values are unused -- re-reads rows 0 .. RW - 1, which exist)
            const double* mp = M + (size_t)((wave_in ? wbase : 0) + ks) * ldm + j;
#pragma unroll
            for (int s = 0; s < NST; ++s) m[s] = mp[(size_t)(4 * s) * ldm];
        } else {                                   // the wave that straddles row D (D % RW != 0) and, for D < RW, the waves beyond it:
            // clamped rows.  (Round 6: the waves beyond row D used to take the unclamped branch with base row 0 -- for D < 32 that
            // read rows D .. 31 of a D-row matrix, past the END of the caller's array; harmless inside an allocator block, a
            // memory access fault when the array ends its mapping: found by the whole suite in one process)
            const int rb = wave_in ? wbase : 0;
#pragma unroll
            for (int s = 0; s < NST; ++s) {
                const int r = rb + ks + 4 * s;
                m[s] = M[(size_t)(r < D ? r : D - 1) * ldm + j];
            }
        }
        if constexpr (PART) {              // BEHIND the M stream: consumed only by the epilogue, nothing waits for them before
            const int prow = r0 + ((tid >> 4) & (NR - 1)), pcol = blockIdx.x * 16 + (tid & 15);
            pq_g = A[(size_t)prow * lda + pcol];
            if constexpr (!QMW) {
                pq_x = px.sj_src[(size_t)prow * px.sj_len + pcol];     // X, ldx
                pq_m = px.msl[pcol];                                   // mu0
            } else if (blockIdx.y == 1 && blockIdx.x < 16) {           // block-uniform: this workgroup sums Qm of sample qm_b
                const int qm_b = 16 * blockIdx.z + blockIdx.x, qm_c = 2 * tid < D ? 2 * tid : 0;
                wq_g = *reinterpret_cast<const v2d*>(A + (size_t)qm_b * lda + qm_c);
                wq_x = *reinterpret_cast<const v2d*>(px.sj_src + (size_t)qm_b * px.sj_len + qm_c);
                wq_m = *reinterpret_cast<const v2d*>(px.msl + qm_c);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (ch > 0) __syncthreads();       // previous chunk's MFMA reads of As are done
#pragma unroll
        for (int q = 0; q < UPT; ++q) {
            const int u = q * 512 + tid;
            const int row = u / U16, c16 = u % U16;
            if constexpr (LANDING) {       // this wave's first / last G unit landed (8 G units, 16 S0 loads and 3 partial-dot loads
                if (stamps && q == 0) { asm volatile("s_waitcnt vmcnt(26)" ::: "memory"); tl_first = __builtin_amdgcn_s_memrealtime(); }     // in flight:
                if (stamps && q == UPT - 1) { asm volatile("s_waitcnt vmcnt(19)" ::: "memory"); tl_last = __builtin_amdgcn_s_memrealtime(); }   // issue order)
            }
            v2d v = ga[q];
            if (!((okbits >> q) & 1u)) v = HAS_SHIFT ? gs[q] : (v2d){0.0, 0.0};   // contributes alpha*(x-x) = 0
            if (HAS_SHIFT) { v.x -= gs[q].x; v.y -= gs[q].y; }
            v.x *= alpha; v.y *= alpha;
            *reinterpret_cast<v2d*>(&As[row * LDG + 2 * c16]) = v;
        }
        __syncthreads();
        PSTAMP(1);                         // left operand staged (the M stream may still be in flight)
        if constexpr (LANDING) {           // words 4 - 6: wave 0's first G unit, last G unit and last S0 load landed (wave 0 alone waits for
            if (stamps && w == 0) {        // its S0 in front of its MFMAs); word 7: wave 7's last G unit -- the skew the barrier above absorbs.
                asm volatile("s_waitcnt vmcnt(3)" ::: "memory");       // Kept in registers until here: a stamp store would count in vmcnt.
                tl_s0 = __builtin_amdgcn_s_memrealtime();
            }
            const unsigned wg_ = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
            if (stamps && wg_ < GSMVI_STAMP_WG) {
                if (tid == 0) { stamps[(size_t)wg_ * 8 + 4] = tl_first; stamps[(size_t)wg_ * 8 + 5] = tl_last; stamps[(size_t)wg_ * 8 + 6] = tl_s0; }
                if (tid == 448) stamps[(size_t)wg_ * 8 + 7] = tl_last;
            }
        }
        if (wave_in) {
            const double* ap = As + c * LDG + RW * w + ks;
            double av[MT][NST];                     // operands to registers first: no LDS round trip per MFMA step
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int s = 0; s < NST; ++s) av[mt][s] = ap[mt * 16 * LDG + 4 * s];
#pragma unroll
            for (int s = 0; s < NST; ++s) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = GSMVI_MFMA_F64(av[mt][s], m[s], acc[mt]);
            }
        }
    }

    // cross-wave reduction through LDS (fixed order => deterministic), red[w][row][17], w = 0..7
    __syncthreads();
    PSTAMP(2);
    double* red = As;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(w * NR + 16 * mt + ks + 4 * r) * 17 + c] = acc[mt][r];
    __syncthreads();
    // Out == nullptr: the slab Pp[kc] is the result (a finish pass or a consumer sums the KC slabs).
    // Out != nullptr (only launched with KC == 1): FINISHED output Out = addvec + slab, no finish pass.
    for (int idx = tid; idx < NR * 16; idx += 512) {
        const int rr = idx >> 4, cc = idx & 15;
        const int row = r0 + rr;
        if (row < nrows && (!RAG || (int)blockIdx.x * 16 + cc < ncols)) {
            double s = 0.0;
#pragma unroll
            for (int ww = 0; ww < 8; ww += 2) s += red[(ww * NR + rr) * 17 + cc] + red[((ww + 1) * NR + rr) * 17 + cc];
            if (Out == nullptr) Pp[((size_t)blockIdx.y * nrows + row) * ncols + blockIdx.x * 16 + cc] = s;
            else Out[(size_t)row * ldo + blockIdx.x * 16 + cc] = s + (addvec ? addvec[blockIdx.x * 16 + cc] : 0.0);
            if constexpr (PART) {          // (nrows % NR == 0: the 16 lanes of a DPP row are the 16 columns of sample row; whole waves run)
                const double pg = row16_sum(pq_g * s);
                if (cc == 0) px.sj_dst[((size_t)row * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = pg;      // Qg
                if (!QMW && blockIdx.y == 0) {
                    const double pm = row16_sum((pq_m - pq_x) * pq_g);
                    if (cc == 0) px.mfin[(size_t)row * gridDim.x + blockIdx.x] = pm;                             // Qm
                }
            }
        }
    }
    if constexpr (QMW) {
        if (blockIdx.y == 1 && blockIdx.x < 16) {  // (mu0 - x_b) . g_b of sample qm_b, fixed order
            const int qm_b = 16 * blockIdx.z + blockIdx.x;
            const double pr = 2 * tid < D ? (wq_m.x - wq_x.x) * wq_g.x + (wq_m.y - wq_x.y) * wq_g.y : 0.0;
            const double rs = row16_sum(pr);
            __syncthreads();                       // the store loop's reads of red are done
            if ((tid & 15) == 0) red[tid >> 4] = rs;
            __syncthreads();
            if (tid == 0) {
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < 32; ++i) s += red[i];
                px.mfin[qm_b] = s;                 // Qm[b]
            }
        }
    }
    if (EXTRA && px.sj_src != nullptr) {            // side job: this workgroup's slice of a slab sum
        const int nwg = gridDim.x * gridDim.y * gridDim.z;
        const int wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        const int per = (px.sj_len + nwg - 1) / nwg;
        // (round 5: a LOOP over the slice.  With one element per thread a launch of fewer than sj_len / 512 workgroups left the
        // tail of every slice unsummed -- D < 256 with 2B = 128: 12 - 24 workgroups for 16384 entries -- and the factor update
        // reported a failure it did not have, on every call: GSM.fit(method="auto") at D = 192, B = 64 reverted every iteration)
        const int i_end = (wg + 1) * per < px.sj_len ? (wg + 1) * per : px.sj_len;
        for (int i = wg * per + tid; i < i_end; i += (int)blockDim.x) {
            double t[GSMVI_MAX_KC];
#pragma unroll
            for (int q = 0; q < GSMVI_MAX_KC; ++q) t[q] = px.sj_src[(size_t)(q < px.sj_kc ? q : px.sj_kc - 1) * px.sj_stride + i];
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < GSMVI_MAX_KC; ++q) a += (q < px.sj_kc) ? t[q] : 0.0;
            px.sj_dst[i] = a;
        }
    }
    if (stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); PSTAMP(3); }
#undef PSTAMP
}

template <int MT, bool HAS_SHIFT, int CHW, bool EXTRA, bool RIDER = false, bool RAG = false, bool PART = false, bool QMW = false,
          int STREAM = 0>
__global__ __launch_bounds__(512) void k_panel_fast(int D, int nrows, const double* __restrict__ A, int lda,
                                                    const double* __restrict__ shift, double alpha,
                                                    const double* __restrict__ M, int ldm,
                                                    double* Pp, int chunks_per_wg, int ncols,
                                                    unsigned long long* __restrict__ stamps, double* __restrict__ Out,
                                                    int ldo, const double* __restrict__ addvec, gsmvi_panel_extras px) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    panel_fast_body<MT, HAS_SHIFT, CHW, EXTRA, RIDER, RAG, PART, QMW, STREAM>(t0, D, nrows, A, lda, shift, alpha, M, ldm, Pp, chunks_per_wg,
                                                                              ncols, stamps, Out, ldo, addvec, px);
}

// =====================================================================================
// k_panel_fast with the NEXT chunk's loads in flight (round 6; D >= 2048, rows <= 32, on the grid, plain products).
// At D = 4096 a workgroup of k_panel_fast walks eight 256-row chunks, and each chunk is a serial chain: issue the loads (64 KB of
// left operand from L2, 32 KB of M from HBM) -> wait -> LDS staging -> barrier -> operand reads -> MFMAs -> next chunk's loads.
// Two resident workgroups per CU overlap each other and nothing else: 5.9 us per chunk, 47 - 50 us for the 134 MB of M at
// (4096, 32) = 2.8 TB/s (round-5 verdict, weak 6).  [A first attempt blamed the left operand's re-reads and gave every
// workgroup four 16-column tiles per staged chunk (a quarter of the re-reads): 47.1 us against 47.1 -- the chain, not the bytes.]
// Here the loads of chunk ch + 1 are issued as soon as chunk ch has gone to LDS -- two register sets, alternating -- so they fly
// during chunk ch's operand reads and MFMAs and the barriers around them; the barriers wait for LDS only (s_waitcnt lgkmcnt(0);
// s_barrier: __syncthreads() would drain the prefetch, as in k_gsm_cov_sym_p).  Same arithmetic and the same summation order as
// k_panel_fast with the same chunks_per_wg: bit-identical slabs.
// =====================================================================================
template <int MT, bool HAS_SHIFT>
__global__ __launch_bounds__(512) void k_panel_fast_p(int D, int nrows, const double* __restrict__ A, int lda,
                                                      const double* __restrict__ shift, double alpha,
                                                      const double* __restrict__ M, int ldm, double* __restrict__ Pp,
                                                      int chunks_per_wg, int ncols, double* __restrict__ Out, int ldo,
                                                      const double* __restrict__ addvec) {
#define LDS_BARRIER_P() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
    constexpr int CHW = 256;
    constexpr int LDG = CHW + 2;
    constexpr int NR = 16 * MT;
    constexpr int RW = CHW / 8;
    constexpr int NST = RW / 4;
    constexpr int U16 = CHW / 2;
    constexpr int UPT = NR * U16 / 512;
    constexpr int SMEM = (NR * LDG > 8 * NR * 17) ? NR * LDG : 8 * NR * 17;
    __shared__ __attribute__((aligned(16))) double As[SMEM];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, c = l & 15, ks = l >> 4;
    const int j = blockIdx.x * 16 + c;
    const int r0 = blockIdx.z * NR;
    const int ch0 = blockIdx.y * chunks_per_wg;
    int nch = (D - ch0 * CHW + CHW - 1) / CHW;                  // chunks this workgroup owns (D % 256 == 0 on this path)
    if (nch > chunks_per_wg) nch = chunks_per_wg;
    v4d acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (v4d){0.0, 0.0, 0.0, 0.0};
    // one set of left-operand registers (they are consumed by the staging, in front of the next issue), two sets for M (chunk ch's
    // rows feed the MFMAs behind the issue of chunk ch + 1's): 2 workgroups per CU stay resident (<= 128 VGPRs)
    v2d ga[UPT], gs[UPT];
    auto issue = [&](int ch, double (&m)[NST]) {
        const int cbase = (ch0 + ch) * CHW;
#pragma unroll
        for (int q = 0; q < UPT; ++q) {
            const int u = q * 512 + tid;
            const int row = u / U16, c16 = u % U16;
            const int grow = r0 + row;
            ga[q] = *reinterpret_cast<const v2d*>(A + (size_t)(grow < nrows ? grow : nrows - 1) * lda + cbase + 2 * c16);
            if (HAS_SHIFT) gs[q] = *reinterpret_cast<const v2d*>(shift + cbase + 2 * c16);
        }
        __builtin_amdgcn_sched_barrier(0);
        const double* mp = M + (size_t)(cbase + w * RW + ks) * ldm + j;
#pragma unroll
        for (int s = 0; s < NST; ++s) m[s] = mp[(size_t)(4 * s) * ldm];
        __builtin_amdgcn_sched_barrier(0);
    };
    auto chunk = [&](int ch, double (&m)[NST], double (&mn)[NST]) {
        if (ch > 0) LDS_BARRIER_P();                              // the previous chunk's operand reads are done
#pragma unroll
        for (int q = 0; q < UPT; ++q) {
            const int u = q * 512 + tid;
            const int row = u / U16, c16 = u % U16;
            v2d v = ga[q];
            if (r0 + row >= nrows) v = HAS_SHIFT ? gs[q] : (v2d){0.0, 0.0};
            if (HAS_SHIFT) { v.x -= gs[q].x; v.y -= gs[q].y; }
            v.x *= alpha; v.y *= alpha;
            *reinterpret_cast<v2d*>(&As[row * LDG + 2 * c16]) = v;
        }
        LDS_BARRIER_P();
        if (ch + 1 < nch) issue(ch + 1, mn);                     // next chunk's loads fly during this chunk's operand reads and MFMAs
        const double* ap = As + c * LDG + RW * w + ks;
        double av[MT][NST];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int s = 0; s < NST; ++s) av[mt][s] = ap[mt * 16 * LDG + 4 * s];
#pragma unroll
        for (int s = 0; s < NST; ++s)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = GSMVI_MFMA_F64(av[mt][s], m[s], acc[mt]);
    };
    double mA[NST], mB[NST];
    if (nch > 0) issue(0, mA);
    for (int ch = 0; ch < nch; ch += 2) {
        chunk(ch, mA, mB);
        if (ch + 1 < nch) chunk(ch + 1, mB, mA);
    }
    __syncthreads();
    double* red = As;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(w * NR + 16 * mt + ks + 4 * r) * 17 + c] = acc[mt][r];
    __syncthreads();
    for (int idx = tid; idx < NR * 16; idx += 512) {
        const int rr = idx >> 4, cc = idx & 15;
        const int row = r0 + rr;
        if (row < nrows) {
            double sm_ = 0.0;
#pragma unroll
            for (int ww = 0; ww < 8; ww += 2) sm_ += red[(ww * NR + rr) * 17 + cc] + red[((ww + 1) * NR + rr) * 17 + cc];
            if (Out == nullptr) Pp[((size_t)blockIdx.y * nrows + row) * ncols + blockIdx.x * 16 + cc] = sm_;
            else Out[(size_t)row * ldo + blockIdx.x * 16 + cc] = sm_ + (addvec ? addvec[blockIdx.x * 16 + cc] : 0.0);
        }
    }
#undef LDS_BARRIER_P
}

// =====================================================================================
// Per-sample stage (gsm_numpy.py:8-18): one 1024-thread workgroup per sample, every thread owns
// EPT elements of the row; all loads first, one block reduction, then the record
// rec[b] = [ d_b | e_b | dmu_b ] is written (see k_gsm_scalars for the algebra).
// =====================================================================================
template <int EPT, int KCT, int NT>
__global__ __launch_bounds__(NT) void k_gsm_scalars_fast(int D, int B, int KC, const double* __restrict__ X,
                                                         int ldx, const double* __restrict__ G, int ldg,
                                                         const double* __restrict__ mu0,
                                                         const double* __restrict__ Pp,
                                                         double* __restrict__ rec, int ldrec,
                                                         unsigned long long* __restrict__ stamps) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();   // stamp word 0, written with word 1 (round 15)
    if (blockIdx.x >= GSMVI_STAMP_WG) stamps = nullptr;          // timeline diagnostic: slot capacity
    constexpr int NW = NT / 64;
    __shared__ double lds[2 * NW];
    const int b = blockIdx.x, tid = threadIdx.x;
    double pp[EPT][KCT], xv[EPT], gv[EPT], mv0[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int i = tid + NT * e;
        const int ic = i < D ? i : D - 1;
#pragma unroll
        for (int kc = 0; kc < KCT; ++kc)
            pp[e][kc] = Pp[((size_t)(kc < KC ? kc : KC - 1) * B + b) * D + ic];
        xv[e] = X[(size_t)b * ldx + ic];
        gv[e] = G[(size_t)b * ldg + ic];
        mv0[e] = mu0[ic];
    }
    double p0 = 0.0, p1 = 0.0, sg[EPT], dd[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int i = tid + NT * e;
        double t = 0.0;
#pragma unroll
        for (int kc = 0; kc < KCT; ++kc) t += (kc < KC) ? pp[e][kc] : 0.0;
        sg[e] = t;
        dd[e] = mv0[e] - xv[e];
        if (i < D) {
            p0 += gv[e] * t;
            p1 += dd[e] * gv[e];
        }
    }
    if (stamps && threadIdx.x == 0) {
        stamps[(size_t)blockIdx.x * 8] = t0;
        stamps[(size_t)blockIdx.x * 8 + 1] = __builtin_amdgcn_s_memrealtime();
    }
    p0 = wave_sum(p0);
    p1 = wave_sum(p1);
    const int w = tid >> 6;
    if ((tid & 63) == 0) {
        lds[2 * w] = p0;
        lds[2 * w + 1] = p1;
    }
    __syncthreads();
    // every thread finishes the reduction and the scalar algebra itself (same operations, same order):
    // cheaper than a second barrier around a one-thread section
    double gSg = 0.0, mv = 0.0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        gSg += lds[2 * k];
        mv += lds[2 * k + 1];
    }
    const double rho = 0.5 * sqrt(1.0 + 4.0 * (gSg + mv * mv)) - 0.5;
    const double den = 1.0 + rho + mv;
    const double beta = 1.0 / (1.0 + rho), c = (gSg - mv) / den;
    double* rb = rec + (size_t)b * ldrec;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int i = tid + NT * e;
        if (i < D) {
            const double dmu = beta * ((sg[e] - dd[e]) - c * dd[e]);
            rb[i] = dd[e];
            rb[D + i] = dd[e] + dmu;
            rb[2 * D + i] = dmu;
        }
    }
    if (stamps) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0) stamps[(size_t)blockIdx.x * 8 + 3] = __builtin_amdgcn_s_memrealtime();
    }
}

// =====================================================================================
// Symmetric rank-2B covariance update (gsm_numpy.py:21-23,50-53) from the per-sample records.
//   W = S0[I,J] + (1/B) ( Dm[:,I]^T Dm[:,J] - E[:,I]^T E[:,J] ),  S[I,J] = W,  S[J,I] = W^T
// One 512-thread workgroup owns the row block I (32 rows) and TWO adjacent column blocks J0, J1 >= I
// of the upper triangle (waves 0-3 compute tile 0, waves 4-7 tile 1: two waves per SIMD, where the
// fp64 MFMA pipe delivers ~46 TF chip-wide instead of ~34 TF with one), so the I tiles are staged
// once and every global load of the workgroup is issued in one batch.  Factor tiles are copied verbatim (16-B loads -> 16-B LDS writes, no arithmetic,
// no transposition) into LDS as [k = sample][32 columns], row stride 48 doubles: the MFMA operand
// reads (lane = column, k-slot = sample) are bank-conflict free for both operands.  The d-part and
// the e-part run as two independent accumulator chains (acc_d - acc_e), which also hides the MFMA
// latency.  S0 must be symmetric (only its upper triangle is read); S comes out exactly symmetric.
// Bytes moved: 4 D^2 read + 8 D^2 written (algorithmic count of SURVEY 8(d): 16 D^2).
// The workgroup whose first tile is diagonal also writes mu = mu0 + mean_b dmu_b.
// =====================================================================================
// RAG (round 5) = edge tiles (D % 32 != 0) and / or fewer than SB samples (B < SB): clamped re-reads, zero-staged sample rows,
// guarded stores.  RAG = false is the round-4 code plus the run-time 1/B (the clamps cost 6 % on the grid shapes when unconditional).
// FROM_SLABS (two-launch dense GSM update; B == SB in {16, 32}, D % 256 == 0, D <= 1024) = there are no records: the factor
// tiles are formed HERE from the samples, the split-K slabs of G S0 and the partial dots that the product launch left beside
// them (k_panel_fast<.., PART>), by the arithmetic of k_gsm_scalars_fast element for element.  Thread -> (sample b = unit >> 4,
// column pair) is the same for the partial dots and for every staged tile, so the 16 lanes of a DPP row reduce sample b's
// partials (fixed order: each lane its units ln, ln + 16, .. sequentially, then row16_sum) and hold beta_b, c_b for exactly the
// units they stage: no LDS hand-off, no barrier, and nothing that waits on another workgroup.  Every workgroup repeats the
// reduction (B x (KC + 1) x D / 16 doubles from L2) -- that is the price of dropping a launch.  Items, tile layout, MFMA chains
// and the store path are those of FROM_SLABS = false, which is the code as it was, instruction for instruction.
// Registers: S0, the partials and the column blocks I, J0, J1 are 29 16-B units per thread, 116 VGPRs if all were in flight at
// once, and two workgroups per CU need <= 128 in all.  So the loads go out in TWO batches: S0, the partials (right behind S0:
// vmcnt counts in issue order, they come back first) and blocks I, J0; then, once the partials are summed, block J1, whose
// latency hides behind the scalar algebra and the staging of the other two blocks.
// (FROM_SLABS holds 29 16-B units per thread in flight; it is compiled for four waves per SIMD -- at most 128 VGPRs -- because the
// 16 late single-tile workgroups cost nothing only while they share a CU with a resident two-tile one; 2 is what
// __launch_bounds__(512) alone implies, so the other instances are compiled as before.)
// KCT (round 8) = how many slabs the FROM_SLABS form is compiled for.  4 is the form above (any KC <= 4 at run time, the absent
// slabs and partials are clamped re-reads).  2 serves the 512-row split of D = 1024 (k_panel_fast<.., 512, .., PART>: exactly two
// slabs, 128 Qg and 64 Qm partials per sample): 4 + 2 units of partials and two slab units per column block are 20 units per
// thread, so ALL loads go out in one batch and both slabs exist.  Same unit order in the sums, slabs added as p0 + p1.
// FOLD (round 9; FROM_SLABS only) = the grid is the n_two two-tile workgroups alone (256 at D = 1024: one per CU, nothing shares a
// CU).  The diagonal tile (r, r) of a row r with an odd tile count, which used to be a workgroup of its own, is a THIRD tile of a
// workgroup that has staged block r anyway:
//   rows with >= 3 tiles: the first pair workgroup of row r, tiles (r, r + 1), (r, r + 2) -- both operands are its staged I tiles;
//   the last row (1 tile): the pair workgroup of row nt - 2, tiles (nt - 2, nt - 2), (nt - 2, nt - 1) -- both are its staged J1 tiles.
// The host adds one S0 unit per thread (the 32 x 32 tile is 512 units), four 16 x 16 MFMA blocks on waves 0-3 (chains as in a
// diagonal workgroup: the same staged values in the same order), a third LW buffer behind the two (inside the LDS it has), one
// 8 KB store without a mirror behind the mirror stores, and mu of block r from the dmu units it staged that block from, in the
// two-level order of the diagonal workgroups, on the barriers the store path has anyway.
typedef unsigned int v4u __attribute__((ext_vector_type(4)));   // the payload type of a 16-B buffer store
// S0L (round 10; the KCT = 2 forms only, knob "cov_s0_last") = the S0 tile is the LAST thing loaded and the last thing waited
// for.  It is the only operand that comes from HBM or the Infinity Cache (everything else was written or read by the product
// launch just before), it is used only in W = S0 + U behind the MFMAs, and vector loads come back in issue order: issued first,
// it stood in front of the partial sums, the rho / beta / c chain and the staging of all three column blocks.  Here the
// partials go out first, then blocks I, J0, J1, then s0v[0..1] and s0x between two sched_barriers; every wait in front of the
// W step is counted so that those three stay outstanding (a non-host re-reads its own s0v[1] unit as s0x: a load under the
// block-uniform branch would make the compiler's waits at the join cover one S0 unit in the hosts), and the barriers between
// staging and the W step are s_waitcnt lgkmcnt(0); s_barrier, which cannot drain the vector-memory counter whatever the
// compiler makes of __syncthreads().  That is safe: no thread reads global data that another thread of its workgroup wrote.
// Same values, same operations, same order: results are those of S0L = false bit for bit.
// WT (round 10; the KCT = 2 forms only, knob "cov_store_wt") = the stores of S (tiles, mirrors, the folded tile; not mu) are 16-B
// write-through stores (buffer stores with sc1): the lines leave the L2 while other workgroups still compute instead of being
// written back at the end of the launch, and they do not stay in the L2.  32-bit byte offsets: the launcher checks the extent.
// QMW (round 10; the KCT = 2 forms only, knob "panel_qm_whole") = the product launch left ONE Qm value per sample
// (k_panel_fast<.., PART, QMW>): mv is one 8-byte load issued with the Qg units; the two Qm units, their sum and the second
// row16_sum are gone from the chain.  mv is summed in another order than the per-strip pieces: mu and S move at rounding level.
// QUAD (round 13; FROM_SLABS, even nt; knob "cov_diag_quad") = another item map with no hosts.  The first nt/2 workgroups are
// QUADS: quad p owns the upper triangle of the diagonal 64 x 64 block, tiles (2p, 2p), (2p, 2p + 1), (2p + 1, 2p + 1), stages the
// column blocks A = 2p and B = 2p + 1 alone (four LDS tiles) and writes mu of both.  Every other tile (i, j) has j/2 > i/2 and
// belongs to the pair (i; 2 (j/2), 2 (j/2) + 1): nt/2 - i/2 - 1 pairs in row i, never diagonal, never a host, the two-tile code
// below as it is.  (nt/2)^2 workgroups in all -- 256 at D = 1024, one per CU as with FOLD -- the quads first.
// A quad is this function.  Its ten 16 x 16 blocks (block (1, 0) of a diagonal tile is the transpose of block (0, 1): the same
// products in the same k order, so it is written, not computed) are twenty chains of SB/4 MFMAs, five per SIMD (waves s, s + 4):
//   waves 4-7: the four blocks of tile (A, B), block (wr, wc) as in a pair: d- and e-chain each;
//   wave 0: (A, A) block (0, 0); wave 1: (A, A) (0, 1); wave 2: (A, A) (1, 1); wave 3: (B, B) (0, 0): d- and e-chain each;
//   (B, B) block (0, 1): d-chain on wave 0, e-chain on wave 1;  (B, B) block (1, 1): d-chain on wave 2, e-chain on wave 3.
// A split block's d-accumulator goes through LDS outside the staged tiles, so the barrier that ends the operand reads also hands
// it over, and the e wave forms (accd - acce) * invB from the same values.  Every chain runs s = 0 .. NS - 1 from zero as in a
// host or a diagonal workgroup, W = S0 + U reads the whole S0 tile (its lower-left block too), and the means take the two-level
// order of the record form: mu and S are those of FOLD and of the plain grid bit for bit.  Stores: tile (A, A) by waves 0-3,
// tile (A, B) by waves 4-7, tile (B, B) one unit per thread, then the mirror of (A, B) by waves 4-7 -- four tile stores, as a pair.
// LDS behind the MFMAs: three LW buffers, the two dmu tiles, their 2 x [8][32] partial sums; the 2 x 256 handed-over accumulators
// lie behind those and behind the staged tiles (COV_QUAD_LDS doubles: 41 728 B at SB = 16, inside the six tiles at SB = 32).
template <int SB>
constexpr int COV_QUAD_SCR = (3 * 32 * 33 + 2 * SB * 32 + 512 > 4 * SB * 48) ? 3 * 32 * 33 + 2 * SB * 32 + 512 : 4 * SB * 48;
template <int SB>
constexpr int COV_QUAD_LDS = COV_QUAD_SCR<SB> + 512;

// WST (round 14; the QUAD instances only, knob "cov_wave_store") = the store path per WAVE.  A wave holds a whole 16 x 16 block of
// U = (acc_d - acc_e) / B in accumulator layout (lane (c = l & 15, ks = l >> 4): rows ks + 4 r, r = 0 .. 3, of column c), and the
// store path above spread the 16-B store units of a tile over the four waves that computed its blocks -- hence accumulators -> LW,
// barrier, W = S0 + U in store layout -> LW, barrier, mirror by columns: three workgroup barriers and two LDS round trips behind
// the last MFMA, no arithmetic in them, every wave waiting three times for the slowest of eight.  Here a wave forms, stores and
// mirrors its block alone:
//   S0 in the wave's own layout: lane (c, ks) loads the units (row ks + 4 (c & 1) [+ 8], columns c & ~1, + 1) of its block -- two
//     16-B loads per thread as before, issued where s0v[] was;
//   exchange: lanes c and c ^ 1 swap through DPP quad_perm [1, 0, 3, 2]: an even lane sends u[1], u[3] and receives u[0], u[2] of
//     its neighbour (the same rows ks, ks + 8, column c + 1), an odd lane the reverse -- every lane then holds the two
//     row-contiguous units it loaded S0 for, W = S0 + U by the same additions on the same values, and a wave instruction stores
//     eight 128-B row segments;
//   mirror: the block goes to a wave-private [16][18] LDS buffer (two ds_write_b128: the eight lanes of a write group cover the 32
//     banks once) and comes back by columns (lane (j = (l >> 3) + 8 q, i2 = l & 7) reads rows 2 i2, 2 i2 + 1 of column j: 72 i2 + 2 j
//     mod 64 over a half wave's 8 x 4 lanes is a permutation) as units S[J + j][I + 2 i2 ..].  Row stride 18, not 17: with 17 the
//     four columns a half wave reads in one ds_read_b64 land on offsets j + {0, 2, .., 14} + 17 (row parity) mod 32, and no choice
//     of four (column, parity) pairs that the second read can complement tiles the 32 double-banks -- a two-way conflict on every
//     read; 18 is conflict free both ways and keeps the units 16-B aligned.
// The eight buffers (8 x 288 doubles = 18 432 B) lie BEHIND the staged tiles and a quad's LDS, so a wave that is done with its MFMAs
// writes nothing another wave may still be reading: no barrier behind the one that ends the staging, the only LDS a wave reads
// behind its MFMAs is what it wrote itself (s_waitcnt lgkmcnt(0) + a wave barrier), and a wave leaves when its four stores are out.
// Same chains, same (acc_d - acc_e) * invB, same S0 + U, copies for the mirror: mu and S are those of WST = false bit for bit.
constexpr int COV_WST_RS = 18, COV_WST_PB = 16 * COV_WST_RS;
// The two halves of that path.  gsm_cov_wave_direct: exchange, W = S0 + U, the block's two direct stores (STORE), and the block into a
// [16][18] buffer -- PBW 1: W, for a mirror that is a copy; 2: U, for a transpose inside a diagonal tile, which is S0's own lower-left
// block plus U^T; 0: nothing.  gsm_cov_wave_mirror: the buffer by columns, S0 units in that layout added where ADD, two stores.
template <bool WT>
__device__ __forceinline__ void gsm_cov_wave_st(double* __restrict__ S, [[maybe_unused]] __amdgpu_buffer_rsrc_t srs, size_t off, v2d v) {
    if constexpr (WT) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v), srs, (int)(off * sizeof(double)), 0, 16);
    else *reinterpret_cast<v2d*>(S + off) = v;
}
template <bool WT, int PBW, bool STORE = true>
__device__ __forceinline__ void gsm_cov_wave_direct(const v4d u, [[maybe_unused]] const v2d s0a, [[maybe_unused]] const v2d s0b,
                                                    [[maybe_unused]] double* __restrict__ PB, double* __restrict__ S,
                                                    __amdgpu_buffer_rsrc_t srs, [[maybe_unused]] size_t doff, int lds, int l) {
    const int c = l & 15, ks = l >> 4;
    const bool odd = c & 1;
    const double x0 = dpp_f64<0xB1>(odd ? u[0] : u[1]);      // quad_perm [1, 0, 3, 2]: the neighbour's half of this lane's units
    const double x1 = dpp_f64<0xB1>(odd ? u[2] : u[3]);
    v2d ua, ub;
    ua.x = odd ? x0 : u[0];
    ua.y = odd ? u[1] : x0;
    ub.x = odd ? x1 : u[2];
    ub.y = odd ? u[3] : x1;
    const int ra = ks + 4 * (c & 1), ca = c & ~1;
    [[maybe_unused]] v2d w0, w1;
    if constexpr (STORE) {
        w0.x = s0a.x + ua.x;
        w0.y = s0a.y + ua.y;
        w1.x = s0b.x + ub.x;
        w1.y = s0b.y + ub.y;
        gsm_cov_wave_st<WT>(S, srs, doff + (size_t)ra * lds + ca, w0);
        gsm_cov_wave_st<WT>(S, srs, doff + (size_t)(ra + 8) * lds + ca, w1);
    }
    static_assert(PBW != 1 || STORE, "a mirror that is a copy needs W");
    if constexpr (PBW == 1) {
        *reinterpret_cast<v2d*>(PB + ra * COV_WST_RS + ca) = w0;
        *reinterpret_cast<v2d*>(PB + (ra + 8) * COV_WST_RS + ca) = w1;
    } else if constexpr (PBW == 2) {
        *reinterpret_cast<v2d*>(PB + ra * COV_WST_RS + ca) = ua;
        *reinterpret_cast<v2d*>(PB + (ra + 8) * COV_WST_RS + ca) = ub;
    }
}
template <bool WT, bool ADD>
__device__ __forceinline__ void gsm_cov_wave_mirror(const double* PB, [[maybe_unused]] const v2d s0ma, [[maybe_unused]] const v2d s0mb,
                                                    double* __restrict__ S, __amdgpu_buffer_rsrc_t srs, size_t moff, int lds, int l) {
    const int i2 = l & 7, jj = l >> 3;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int j = jj + 8 * q;
        v2d m2;
        m2.x = PB[(2 * i2) * COV_WST_RS + j];
        m2.y = PB[(2 * i2 + 1) * COV_WST_RS + j];
        if constexpr (ADD) {
            m2.x = (q ? s0mb : s0ma).x + m2.x;
            m2.y = (q ? s0mb : s0ma).y + m2.y;
        }
        gsm_cov_wave_st<WT>(S, srs, moff + (size_t)j * lds + 2 * i2, m2);
    }
}
// a wave's own LDS writes are done (its stores stay in flight); nothing moves across
#define COV_WAVE_SYNC()                                             \
    do {                                                            \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          \
        __builtin_amdgcn_wave_barrier();                            \
    } while (0)

template <int SB, int KCT, bool S0L, bool WT, bool WST = false>
__device__ __forceinline__ void gsm_cov_quad(double* __restrict__ smem, int p, int D, int B, const double& invB, const double* __restrict__ mu0,
                                             const double* __restrict__ S0, int lds0, double* __restrict__ const& S, const int& lds,
                                             double* __restrict__ const& mu_out, unsigned long long* __restrict__ const& stamps,
                                             const unsigned long long t0, const gsm_slab_src& fs) {
    // (invB, S, lds, mu_out, stamps by reference: as gsm_cov_sym_body takes them)
#define QBARRIER()                                                                       \
    do {                                                                                  \
        if constexpr (S0L) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); \
        else __syncthreads();                                                             \
    } while (0)
#define QSTAMP(k)                                                                         \
    do {                                                                                  \
        if (stamps && threadIdx.x == 0) {                                                 \
            if ((k) == 1) stamps[(size_t)blockIdx.x * 8] = t0;                            \
            stamps[(size_t)blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime();      \
        }                                                                                 \
    } while (0)
    constexpr int RS = 48, TILE = SB * RS, NU = SB * 16, NS = SB / 4, NQG = 2 * KCT;
    constexpr int LWS = 32 * 33, MUO = 3 * LWS, PAO = MUO + 2 * SB * 32, SCO = COV_QUAD_SCR<SB>;
    static_assert(512 % NU == 0 && (KCT == 2 || KCT == 4), "two-launch form: B == SB in {16, 32}");
    static_assert(SCO >= 4 * TILE && SCO >= PAO + 512, "handed-over accumulators outside the staged tiles and the store path's LDS");
    // WST: the waves' private buffers (QPB: where the kernel puts them); the dmu tiles and their partial sums OUTSIDE the staged tiles
    // (they are written at staging time): where they were at SB = 16, in the gap between a quad's LDS and the pairs' six tiles at SB = 32
    constexpr int QPB = 6 * TILE >= COV_QUAD_LDS<SB> ? 6 * TILE : COV_QUAD_LDS<SB>;
    constexpr int MUW = MUO >= 4 * TILE ? MUO : COV_QUAD_LDS<SB>, PAW = MUW + 2 * SB * 32;
    static_assert(!WST || (MUW >= 4 * TILE && PAW + 512 <= (MUO >= 4 * TILE ? SCO : QPB)), "WST: the means' LDS outside the staged tiles, the hand-over and the private buffers");
    const int A0 = 64 * p, B0 = A0 + 32;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, c = l & 15, ks = l >> 4;
    const int t = w >> 2, wr = (w >> 1) & 1, wc = w & 1, tl = tid & 255;
    const int Jt = t ? B0 : A0;                  // S0 and store units of waves 0-3: tile (A, A); of waves 4-7: tile (A, B)
    const int u = tid & (NU - 1), b = u >> 4, ln = u & 15, c2 = 2 * ln;
    const bool st_d = (NU == 512) || tid < NU, st_e = (NU == 512) || tid >= NU;
    const int nqg = (fs.KC * fs.strips) >> 1, nqm = fs.strips >> 1;
    auto ld16 = [](const double* base, unsigned byte_off) {
        return *reinterpret_cast<const v2d*>(reinterpret_cast<const char*>(base) + byte_off);
    };
    v2d s0v[2], s0x;
    // WST: FOUR S0 units per lane, in the layout of the blocks the wave stores (the same count on every wave, so that every wait in
    // front of them stays counted): s0w[0..1] its whole block (waves 4-7: block (wr, wc) of tile (A, B); wave 0: (A, A) (0, 0); 1:
    // (A, A) (0, 1); 2: (A, A) (1, 1); 3: (B, B) (0, 0)); s0w[2..3] its second block -- wave 0: (B, B) (0, 1); 1: (A, A) (1, 0) in the
    // mirror's layout; 2: (B, B) (1, 0) in the mirror's layout; 3: (B, B) (1, 1); waves 4-7 re-read s0w[0..1]
    [[maybe_unused]] v2d s0w[4];
    auto load_s0 = [&]() {
        if constexpr (WST) {
            const int r0 = (w >= 4) ? A0 + 16 * wr : (w == 3 ? B0 : (w == 2 ? A0 + 16 : A0));
            const int c0 = (w >= 4) ? B0 + 16 * wc : (w == 3 ? B0 : (w == 0 ? A0 : A0 + 16));
            const int r1 = (w >= 4) ? r0 : (w == 0 ? B0 : (w == 1 ? A0 + 16 : B0 + 16));
            const int c1 = (w >= 4) ? c0 : (w == 1 ? A0 : (w == 2 ? B0 : B0 + 16));
            const bool mir = w == 1 || w == 2;   // wave-uniform
            const int dr = ks + 4 * (c & 1), dc = c & ~1, lr = mir ? (l >> 3) : dr, lc = mir ? 2 * (l & 7) : dc;
#pragma unroll
            for (int q = 0; q < 2; ++q) s0w[q] = *reinterpret_cast<const v2d*>(S0 + (size_t)(r0 + dr + 8 * q) * lds0 + c0 + dc);
#pragma unroll
            for (int q = 0; q < 2; ++q) s0w[2 + q] = *reinterpret_cast<const v2d*>(S0 + (size_t)(r1 + lr + 8 * q) * lds0 + c1 + lc);
            return;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int unit = q * 256 + tl;
            s0v[q] = *reinterpret_cast<const v2d*>(S0 + (size_t)(A0 + (unit >> 4)) * lds0 + Jt + 2 * (unit & 15));
        }
        s0x = *reinterpret_cast<const v2d*>(S0 + (size_t)(B0 + (tid >> 4)) * lds0 + B0 + 2 * (tid & 15));
    };
    if constexpr (!S0L) {
        load_s0();
        __builtin_amdgcn_sched_barrier(0);
    }
    const unsigned qg0 = (unsigned)(b * nqg) * 16u, qm0 = (unsigned)(b * nqm) * 16u;
    v2d qg[NQG], qm[2];
#pragma unroll
    for (int k = 0; k < NQG; ++k) qg[k] = ld16(fs.Qg, qg0 + 16u * (unsigned)(ln + 16 * k < nqg ? ln + 16 * k : nqg - 1));
#pragma unroll
    for (int k = 0; k < 2; ++k) qm[k] = ld16(fs.Qm, qm0 + 16u * (unsigned)(ln + 16 * k < nqm ? ln + 16 * k : nqm - 1));
    double mu0q = 0.0;                           // mu0 of the mean epilogue: entries A0 .. A0 + 63 on wave 0
    if (w == 0) mu0q = mu0[A0 + l];
    const int col[2] = {A0 + c2, B0 + c2};
    const size_t slab = (size_t)B * D;
    v2d xv[2], m0[2], sl[2][KCT];
    auto load_block = [&](int cb) {
        xv[cb] = *reinterpret_cast<const v2d*>(fs.X + (size_t)b * fs.ldx + col[cb]);
        m0[cb] = ld16(mu0, 8u * (unsigned)col[cb]);
#pragma unroll
        for (int kc = 0; kc < KCT; ++kc)
            sl[cb][kc] = *reinterpret_cast<const v2d*>(fs.Pp + (size_t)(KCT == 2 ? kc : (kc < fs.KC ? kc : fs.KC - 1)) * slab + (size_t)b * D + col[cb]);
    };
    load_block(0);
    if constexpr (KCT == 2) load_block(1);
    if constexpr (S0L) {                         // the three S0 units: the last global loads
        __builtin_amdgcn_sched_barrier(0);
        load_s0();
        __builtin_amdgcn_sched_barrier(0);
    }
    double gs = 0.0, ms = 0.0;
#pragma unroll
    for (int k = 0; k < NQG; ++k) {
        const bool in = ln + 16 * k < nqg;
        gs += in ? qg[k].x : 0.0;
        gs += in ? qg[k].y : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const bool in = ln + 16 * k < nqm;
        ms += in ? qm[k].x : 0.0;
        ms += in ? qm[k].y : 0.0;
    }
    if constexpr (KCT == 4) {                    // second batch behind the sums, as in the pairs
        asm volatile("" : "+v"(gs), "+v"(ms) : : "memory");
        load_block(1);
    }
    const double gSg = row16_sum(gs);
    const double mv = row16_sum(ms);
    const double rho = 0.5 * sqrt(1.0 + 4.0 * (gSg + mv * mv)) - 0.5;
    const double den = 1.0 + rho + mv;
    double beta = 1.0 / (1.0 + rho), cc = (gSg - mv) / den;
    if (stamps) {
        if constexpr (S0L && WST) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if constexpr (S0L) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        QSTAMP(1);
    }
    v2d dmuq[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        v2d sg = {0.0, 0.0}, dd, dm, ee;
        if constexpr (KCT == 2) {
            if (cb == 0) asm volatile("" : "+v"(beta), "+v"(cc), "+v"(xv[0]), "+v"(m0[0]), "+v"(sl[0][0]), "+v"(sl[0][1]));
            else asm volatile("" : "+v"(xv[cb]), "+v"(m0[cb]), "+v"(sl[cb][0]), "+v"(sl[cb][1]));
            sg.x = sl[cb][0].x + sl[cb][1].x;
            sg.y = sl[cb][0].y + sl[cb][1].y;
        } else {
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                sg.x += (kc < fs.KC) ? sl[cb][kc].x : 0.0;
                sg.y += (kc < fs.KC) ? sl[cb][kc].y : 0.0;
            }
        }
        dd.x = m0[cb].x - xv[cb].x;
        dd.y = m0[cb].y - xv[cb].y;
        dm.x = beta * ((sg.x - dd.x) - cc * dd.x);
        dm.y = beta * ((sg.y - dd.y) - cc * dd.y);
        ee.x = dd.x + dm.x;
        ee.y = dd.y + dm.y;
        if (st_d) *reinterpret_cast<v2d*>(smem + (2 * cb) * TILE + b * RS + c2) = dd;
        if (st_e) *reinterpret_cast<v2d*>(smem + (2 * cb + 1) * TILE + b * RS + c2) = ee;
        dmuq[cb] = dm;
        if constexpr (WST) {                     // the dmu tile [SB][32] of this block goes out with the staging: the barrier below covers it
            if (tid < NU) *reinterpret_cast<v2d*>(smem + MUW + cb * SB * 32 + (tid >> 4) * 32 + 2 * (tid & 15)) = dm;
        }
    }
    QBARRIER();
    QSTAMP(2);
    // ---- the chains: a whole block per wave (LDS tiles: 0 = D_A, 1 = E_A, 2 = D_B, 3 = E_B), then one chain of a split block
    v4d accd = {0.0, 0.0, 0.0, 0.0}, acce = {0.0, 0.0, 0.0, 0.0}, xacc = {0.0, 0.0, 0.0, 0.0};
    // ---- WST: the split chains FIRST, and the quad's one barrier between them and the whole blocks.  Waves 0-3 run their chain of a
    // split block (the same operands in the same order, from zero) and leave its accumulator in LDS -- the d-chains where they
    // always went, the e-chain of (B, B) (0, 1) in wave 0's private buffer, that of (B, B) (1, 1) in wave 3's --, all eight waves
    // sum the first level of the means (the dmu tiles were staged), and the barrier hands all of it over.  Behind it nobody waits
    // for anybody: a wave runs the chains of its whole block and then forms, stores and mirrors TWO blocks alone (below).
    if constexpr (WST) {
        if (w < 4) {
            const double* xp = smem + (2 + (w & 1)) * TILE + ks * RS + c;
            double xa[NS], xb[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                xa[s] = xp[4 * s * RS + 16 * (w >> 1)];
                xb[s] = xp[4 * s * RS + 16];
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) xacc = GSMVI_MFMA_F64(xa[s], xb[s], xacc);
            double* xo = (w & 1) ? smem + QPB + (w == 1 ? 0 : 3) * COV_WST_PB : smem + SCO + (w >> 1) * 256;
#pragma unroll
            for (int r = 0; r < 4; ++r) xo[r * 64 + l] = xacc[r];
        }
        {                                        // first level of the means: block tid >> 8, row group (tid >> 5) & 7, column tid & 31
            const double* mt = smem + MUW + (tid >> 8) * SB * 32;
            double part = 0.0;
#pragma unroll
            for (int k = 0; k < SB / 8; ++k) part += mt[(((tid >> 5) & 7) + 8 * k) * 32 + (tid & 31)];
            smem[PAW + tid] = part;              // 2 x [8][32]
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS only: the S0 loads stay in flight
    }
    {
        const int ta = (w == 3) ? 2 : 0, tb = (w >= 3) ? 2 : 0;                  // wave-uniform
        const int br = (w >= 4) ? wr : (w == 2 ? 1 : 0), bc = (w >= 4) ? wc : ((w == 1 || w == 2) ? 1 : 0);
        const double* adp = smem + ta * TILE + ks * RS + 16 * br + c;
        const double* bdp = smem + tb * TILE + ks * RS + 16 * bc + c;
        double ad[NS], ae[NS], bd[NS], be[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            ad[s] = adp[4 * s * RS];
            ae[s] = adp[TILE + 4 * s * RS];
            bd[s] = bdp[4 * s * RS];
            be[s] = bdp[TILE + 4 * s * RS];
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            accd = GSMVI_MFMA_F64(ad[s], bd[s], accd);
            acce = GSMVI_MFMA_F64(ae[s], be[s], acce);
        }
        if constexpr (!WST) {
        if (w < 4) {                             // (B, B) block (w >> 1, 1): the d-chain on the even wave, the e-chain on the odd one
            const double* xp = smem + (2 + (w & 1)) * TILE + ks * RS + c;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                ad[s] = xp[4 * s * RS + 16 * (w >> 1)];
                bd[s] = xp[4 * s * RS + 16];
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) xacc = GSMVI_MFMA_F64(ad[s], bd[s], xacc);
            if (!(w & 1)) {
#pragma unroll
                for (int r = 0; r < 4; ++r) smem[SCO + (w >> 1) * 256 + r * 64 + l] = xacc[r];
            }
        }
        }
    }
    // ---- WST: no barrier behind the MFMAs.  Every wave forms, stores and mirrors two blocks alone, four stores of S each:
    //   waves 4-7: block (wr, wc) of tile (A, B) and its mirror, as a pair's;
    //   wave 0: (A, A) (0, 0); (B, B) (0, 1) from the handed-over d- and e-chain;  wave 3: (B, B) (0, 0); (B, B) (1, 1) likewise;
    //   wave 1: (A, A) (0, 1) and its transpose (A, A) (1, 0) = S0's own lower-left block + U(0, 1)^T, through its buffer;
    //   wave 2: (A, A) (1, 1); the transpose (B, B) (1, 0) from the same two handed-over chains as wave 0 reads -- the same
    //           (d - e) * invB on the same values -- through its buffer;  wave 0 then adds the second level of the means.
    if constexpr (WST) {
        double* PBQ = smem + QPB;
        v4d u;
#pragma unroll
        for (int r = 0; r < 4; ++r) u[r] = (accd[r] - acce[r]) * invB;
        if (stamps) {                            // [3] wave 0's MFMAs done, [6] S0 landed
            asm volatile("" : "+v"(u));
            QSTAMP(3);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            QSTAMP(6);
        }
        __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(S, 0, 0, 0);   // (plain stores: not used)
        if constexpr (WT) srs = __builtin_amdgcn_make_buffer_rsrc(S, 0, (int)(((size_t)(D - 1) * lds + D) * sizeof(double)), 0x00020000);
        // all four S0 units are waited for HERE, in front of the first store: s0w[2..3] came in right behind s0w[0..1], and a wait
        // for them behind the first stores is a vmcnt(1) at the join of these branches (the waves have issued two or four stores by
        // then), which waits for all but one of the write-through stores to be acknowledged
        asm volatile("" : "+v"(s0w[0]), "+v"(s0w[1]), "+v"(s0w[2]), "+v"(s0w[3]));
        if (w >= 4) {
            double* PB = PBQ + w * COV_WST_PB;
            gsm_cov_wave_direct<WT, 1>(u, s0w[0], s0w[1], PB, S, srs, (size_t)(A0 + 16 * wr) * lds + B0 + 16 * wc, lds, l);
            COV_WAVE_SYNC();
            gsm_cov_wave_mirror<WT, false>(PB, s0w[0], s0w[1], S, srs, (size_t)(B0 + 16 * wc) * lds + A0 + 16 * wr, lds, l);
        } else if (w == 1) {
            double* PB = PBQ + COV_WST_PB;
            gsm_cov_wave_direct<WT, 2>(u, s0w[0], s0w[1], PB, S, srs, (size_t)A0 * lds + A0 + 16, lds, l);
            COV_WAVE_SYNC();
            gsm_cov_wave_mirror<WT, true>(PB, s0w[2], s0w[3], S, srs, (size_t)(A0 + 16) * lds + A0, lds, l);
        } else {
            const int X0 = (w == 3) ? B0 : (w == 2 ? A0 + 16 : A0), bi = (w == 3) ? 1 : 0;
            gsm_cov_wave_direct<WT, 0>(u, s0w[0], s0w[1], nullptr, S, srs, (size_t)X0 * lds + X0, lds, l);
            const double* xd = smem + SCO + bi * 256;              // the handed-over chains of (B, B) (bi, 1)
            const double* xe = PBQ + (bi ? 3 : 0) * COV_WST_PB;
            v4d xu;
#pragma unroll
            for (int r = 0; r < 4; ++r) xu[r] = (xd[r * 64 + l] - xe[r * 64 + l]) * invB;
            if (w == 2) {
                double* PB = PBQ + 2 * COV_WST_PB;
                gsm_cov_wave_direct<WT, 2, false>(xu, s0w[2], s0w[3], PB, S, srs, 0, lds, l);
                COV_WAVE_SYNC();
                gsm_cov_wave_mirror<WT, true>(PB, s0w[2], s0w[3], S, srs, (size_t)(B0 + 16) * lds + B0, lds, l);
            } else {
                gsm_cov_wave_direct<WT, 0>(xu, s0w[2], s0w[3], nullptr, S, srs, (size_t)(B0 + 16 * bi) * lds + B0 + 16, lds, l);
            }
            if (w == 0) {                        // second level: mu of blocks A (lanes 0-31) and B (lanes 32-63)
                double s = 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q) s += smem[PAW + (l >> 5) * 256 + q * 32 + (l & 31)];
                mu_out[A0 + l] = mu0q + s * invB;
            }
        }
        if (stamps) __syncthreads();             // [4]: every wave has issued its last store (the timeline instance only)
        QSTAMP(4);
        if (stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); QSTAMP(5); }
        return;
    }
    QBARRIER();                                  // the factor tiles are read, the d-accumulators of the split blocks are in LDS
    {
        const int lw = (w >= 4) ? 1 : (w == 3 ? 2 : 0);
        const int br = (w >= 4) ? wr : (w == 2 ? 1 : 0), bc = (w >= 4) ? wc : ((w == 1 || w == 2) ? 1 : 0);
        double* LW = smem + lw * LWS;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double v = (accd[r] - acce[r]) * invB;
            LW[(16 * br + ks + 4 * r) * 33 + 16 * bc + c] = v;
            if (w == 1) LW[(16 + c) * 33 + ks + 4 * r] = v;                      // (A, A) block (1, 0) = block (0, 1)^T
        }
        if (w < 4 && (w & 1)) {
            double* LX = smem + 2 * LWS;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = (smem[SCO + (w >> 1) * 256 + r * 64 + l] - xacc[r]) * invB;
                LX[(16 * (w >> 1) + ks + 4 * r) * 33 + 16 + c] = v;
                if (w == 1) LX[(16 + c) * 33 + ks + 4 * r] = v;                  // (B, B) block (1, 0) = block (0, 1)^T
            }
        }
    }
    if (tid < NU) {                              // the dmu tiles of blocks A and B, [SB][32] each
        *reinterpret_cast<v2d*>(smem + MUO + (tid >> 4) * 32 + 2 * (tid & 15)) = dmuq[0];
        *reinterpret_cast<v2d*>(smem + MUO + SB * 32 + (tid >> 4) * 32 + 2 * (tid & 15)) = dmuq[1];
    }
    QSTAMP(3);
    QBARRIER();
    if constexpr (S0L) {
        if (stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); QSTAMP(6); }
    }
    [[maybe_unused]] __amdgpu_buffer_rsrc_t srs;
    if constexpr (WT) srs = __builtin_amdgcn_make_buffer_rsrc(S, 0, (int)(((size_t)(D - 1) * lds + D) * sizeof(double)), 0x00020000);
    auto store_s = [&](size_t off, v2d v) {
        if constexpr (WT) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v), srs, (int)(off * sizeof(double)), 0, 16);
        else *reinterpret_cast<v2d*>(S + off) = v;
    };
    {                                            // first level of the means: block tid >> 8, row group (tid >> 5) & 7, column tid & 31
        const double* mt = smem + MUO + (tid >> 8) * SB * 32;
        double part = 0.0;
#pragma unroll
        for (int k = 0; k < SB / 8; ++k) part += mt[(((tid >> 5) & 7) + 8 * k) * 32 + (tid & 31)];
        smem[PAO + tid] = part;                  // 2 x [8][32]
    }
    {
        double* LW = smem + t * LWS;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int unit = q * 256 + tl, i = unit >> 4, j2 = unit & 15;
            v2d wv2;
            wv2.x = s0v[q].x + LW[i * 33 + 2 * j2];
            wv2.y = s0v[q].y + LW[i * 33 + 2 * j2 + 1];
            store_s((size_t)(A0 + i) * lds + Jt + 2 * j2, wv2);
            if (t) {                             // tile (A, B) goes back to LDS for its mirror
                LW[i * 33 + 2 * j2] = wv2.x;
                LW[i * 33 + 2 * j2 + 1] = wv2.y;
            }
        }
    }
    {                                            // tile (B, B): one unit per thread, no mirror
        const int i = tid >> 4, j2 = tid & 15;
        v2d wv2;
        wv2.x = s0x.x + smem[2 * LWS + i * 33 + 2 * j2];
        wv2.y = s0x.y + smem[2 * LWS + i * 33 + 2 * j2 + 1];
        store_s((size_t)(B0 + i) * lds + B0 + 2 * j2, wv2);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS only: the stores above stay in flight
    if (t) {
        const double* LW = smem + LWS;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int unit = q * 256 + tl, j = unit >> 4, i2 = unit & 15;
            v2d m2;
            m2.x = LW[(2 * i2) * 33 + j];
            m2.y = LW[(2 * i2 + 1) * 33 + j];
            store_s((size_t)(B0 + j) * lds + A0 + 2 * i2, m2);
        }
    }
    if (w == 0) {                                // second level: mu of blocks A (lanes 0-31) and B (lanes 32-63)
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) s += smem[PAO + (l >> 5) * 256 + q * 32 + (l & 31)];
        mu_out[A0 + l] = mu0q + s * invB;
    }
    QSTAMP(4);
    if (stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); QSTAMP(5); }
#undef QSTAMP
#undef QBARRIER
}

template <int SB, bool RAG, bool FROM_SLABS = false, int KCT = 4, bool FOLD = false, bool S0L = false, bool WT = false, bool QMW = false, bool QUAD = false,
          bool WST = false>
__device__ __forceinline__ void gsm_cov_sym_body(const unsigned long long t0, int D, int B, const double& invB, const double* __restrict__ rec, int ldrec,
                                                 const double* __restrict__ mu0,
                                                 const double* __restrict__ S0, int lds0,
                                                 double* __restrict__ const& S, const int& lds,
                                                 double* __restrict__ const& mu_out, int dbg,
                                                 unsigned long long* __restrict__ const& stamps_arg, const gsm_slab_src& fs) {
    // The body of k_gsm_cov_sym and of the preloaded entry points of gsmvi_fast_hot.hip (round 15).  t0 = the clock at the kernel's
    // first instruction: stamp word 0, written with stamp 1.  What no load of the first batch needs -- 1 / B, the outputs, the stamps --
    // comes by reference: k_gsm_cov_sym passes its own parameters (values, as before), a preloaded entry point members of a by-value
    // struct behind its hot block, which are then fetched where they are first used and not in front of the loads.
    static_assert(!FOLD || FROM_SLABS, "folded diagonal tiles: the two-launch form only");
    static_assert(!(S0L || WT || QMW) || (FROM_SLABS && KCT == 2 && !RAG), "S0 last / write-through stores / whole-sample Qm: the two-slab two-launch form only, on the grid");
    static_assert(!QUAD || (FROM_SLABS && !FOLD && !QMW && !RAG && (SB == 16 || SB == 32)), "quads: the two-launch form, in place of the fold");
    static_assert(!WST || QUAD, "per-wave store path: the quad / pair map only (no diagonal pair, no host, no edge tile)");
    // barriers between staging and the W step: LDS-only where S0 is in flight across them
#define PRE_W_BARRIER()                                                                   \
    do {                                                                                  \
        if constexpr (S0L) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); \
        else __syncthreads();                                                             \
    } while (0)
#define STAMP(k)                                                                          \
    do {                                                                                  \
        if (stamps && threadIdx.x == 0) {                                                 \
            if ((k) == 1) stamps[(size_t)blockIdx.x * 8] = t0;                            \
            stamps[(size_t)blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime();      \
        }                                                                                 \
    } while (0)
    // (Round 4 tried LDS-only barriers here -- s_waitcnt lgkmcnt(0); s_barrier instead of __syncthreads(), whose workgroup fence
    // also drains the vector-memory counter: 6.45 against 6.38 us at D = 1024, B = 32, no effect; they matter in the persistent
    // form below, where loads of the next item are in flight across the barriers.)
    // timeline diagnostic: slot capacity (D >= 2048 has more workgroups; the two-launch form has D <= 1024, at most 272 workgroups,
    // and no use of `stamps` in front of its loads)
    unsigned long long* const stamps_slot = (!FROM_SLABS && blockIdx.x < GSMVI_STAMP_WG) ? stamps_arg : nullptr;
    unsigned long long* __restrict__ const& stamps = FROM_SLABS ? stamps_arg : stamps_slot;
    constexpr int RS = 48;                      // LDS row stride (doubles): 32 columns + 16 pad
    constexpr int NPASS = (SB > 32) ? SB / 32 : 1;   // samples are staged 32 at a time: <= 74 KB of LDS, so
    constexpr int SBP = SB / NPASS;              //   two workgroups fit per CU also at B = 64
    constexpr int TILE = SBP * RS;               // one staged tile (per pass)
    constexpr int NU = SB * 16;                  // 16-B units per tile over all samples
    constexpr int UPT = (6 * NU) / 512;          // units per thread over the six tiles
    static_assert((6 * NU) % 512 == 0, "tile units must divide over 512 threads");
    constexpr int QLDS = QUAD ? COV_QUAD_LDS<SB> : 0;   // (a quad's LDS: more than the six tiles at SB = 16)
    constexpr int PBO = 6 * TILE >= 2 * 32 * 33 ? (6 * TILE >= QLDS ? 6 * TILE : QLDS) : 2 * 32 * 33;   // WST: the waves' private buffers behind it
    static_assert(!WST || (PBO % 2 == 0 && PBO >= 6 * TILE && PBO >= QLDS), "private buffers: 16-B aligned, behind the staged tiles and a quad's LDS");
    __shared__ __attribute__((aligned(16))) double smem[PBO + (WST ? 8 * COV_WST_PB : 0)];
    // staged tiles, in this order: DI, EI, DJ0, EJ0, DJ1, EJ1

    // ---- which tiles: row block ti, column blocks tj0, tj0+1 ------------------------------------
    // Row ti of the upper triangle has m = nt - ti tiles: floor(m/2) two-tile workgroups and, for odd
    // m, one single-tile workgroup (its last tile).  The two-tile workgroups come FIRST in the grid
    // (exactly 256 of them at D = 1024: one per CU); the light single-tile ones are dispatched last
    // and share a CU with a resident workgroup without stretching the kernel's tail.
    const int nt = (D + 31) >> 5;                                // any even D (round 5): edge tiles re-read clamped rows / columns
    const int n_two = ((nt >> 1) * ((nt + 1) >> 1));             // sum_m floor(m/2), m = 1..nt   // and store only what lies inside
    int ti, tj0;
    bool two;
    int fold = 0;                                                // FOLD: 1 = hosts the diagonal tile of its own row, 2 = that of the last row
    if constexpr (QUAD) {                                        // quads first (gsm_cov_quad above), then the pairs right of them
        if ((int)blockIdx.x < (nt >> 1)) {
            gsm_cov_quad<SB, KCT, S0L, WT, WST>(smem, blockIdx.x, D, B, invB, mu0, S0, lds0, S, lds, mu_out, stamps, t0, fs);
            return;
        }
        int rem = blockIdx.x - (nt >> 1);
        ti = 0;
        for (;;) {
            const int inrow = (nt >> 1) - (ti >> 1) - 1;
            if (rem < inrow) break;
            rem -= inrow;
            ++ti;
        }
        tj0 = 2 * ((ti >> 1) + 1) + 2 * rem;
        two = true;
    } else if (FOLD || (int)blockIdx.x < n_two) {
        int rem = blockIdx.x;
        ti = 0;
        for (;;) {
            const int inrow = (nt - ti) >> 1;
            if (rem < inrow) break;
            rem -= inrow;
            ++ti;
        }
        tj0 = ti + ((nt - ti) & 1) + 2 * rem;                    // odd tile count: the pairs start right of the diagonal tile
        two = true;
        if constexpr (FOLD) fold = (((nt - ti) & 1) && rem == 0) ? 1 : (ti == nt - 2 ? 2 : 0);   // block-uniform
    } else {
        const int k = blockIdx.x - n_two;                        // k-th row with an odd tile count: its DIAGONAL tile (no
        ti = ((nt & 1) ? 0 : 1) + 2 * k;                         // mirror store, so the late single-tile workgroups are light)
        tj0 = ti;
        two = false;
    }
    const bool diag = (tj0 == ti);
    const int I0 = ti * 32, J0 = tj0 * 32;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, c = l & 15, ks = l >> 4;
    const int t = w >> 2;                        // which tile this wave computes (two waves per SIMD)
    const int wr = (w >> 1) & 1, wc = w & 1;
    const bool mine = (t == 0) || two;           // does this wave's tile exist

    // ---- every global load of this workgroup, in one batch --------------------------------
    // S0 tile of this wave's tile t in STORE layout: 16-B units, unit = (row i, column pair j2), two per thread -- a row of
    // the tile is one 256-B segment.  (Round 2 loaded and stored 8 B per lane in accumulator layout.)
    const int Jt = J0 + 32 * ((t == 1 && two) ? 1 : 0);
    const int tl = tid & 255;
    v2d s0v[2];
    if constexpr (!S0L && WST) {                 // WST: the lane's two units of block (wr, wc), rows ks + 4 (c & 1) [+ 8], columns c & ~1, + 1
#pragma unroll
        for (int q = 0; q < 2; ++q)
            s0v[q] = *reinterpret_cast<const v2d*>(S0 + (size_t)(I0 + 16 * wr + ks + 4 * (c & 1) + 8 * q) * lds0 + Jt + 16 * wc + (c & ~1));
    } else if constexpr (!S0L) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int unit = q * 256 + tl, i = unit >> 4, j2 = unit & 15;
            const int gr = (RAG && I0 + i >= D) ? D - 1 : I0 + i, gc = (RAG && Jt + 2 * j2 >= D) ? D - 2 : Jt + 2 * j2;
            s0v[q] = (dbg & 2) ? (v2d){1.0, 1.0} : *reinterpret_cast<const v2d*>(S0 + (size_t)gr * lds0 + gc);
        }
    }
    const int X0 = (fold == 2) ? J0 + 32 : I0;   // FOLD: the folded diagonal tile is S[X0 .. X0 + 31][X0 .. X0 + 31], unit = tid
    v2d s0x = {0.0, 0.0};
    if constexpr (FOLD && !S0L) {
        if (fold) s0x = *reinterpret_cast<const v2d*>(S0 + (size_t)(X0 + (tid >> 4)) * lds0 + X0 + 2 * (tid & 15));
    }
    if constexpr (!S0L) __builtin_amdgcn_sched_barrier(0);   // keep the HBM loads of S0 ahead of the L2-resident staging loads
    v2d stg[UPT];
    double dmu_part = 0.0;
    v2d dmuI = {0.0, 0.0};                       // FROM_SLABS: dmu of this thread's unit of block I (the mean, diagonal workgroups)
    v2d dmuX = {0.0, 0.0};                       // FOLD: the same of the folded tile's block (I, or J1 for the last row)
    [[maybe_unused]] double mu0I = 0.0, mu0X = 0.0;   // FROM_SLABS: mu0 of the mean epilogues (block I; FOLD: block X), entry tid & 31
    if constexpr (FROM_SLABS) {
        static_assert(!RAG && NPASS == 1 && 512 % NU == 0, "two-launch form: B == SB in {16, 32}, on the grid");
        static_assert(KCT == 2 || KCT == 4, "slab count of the two-launch form");
        constexpr int NQG = 2 * KCT;             // 16-B units of Qg per lane: KCT * strips / 2 <= 16 * NQG at strips <= 64
        // SB = 16: the two halves of the workgroup hold the same units; half 0 stages the d tiles, half 1 the e tiles
        const int u = tid & (NU - 1), b = u >> 4, ln = u & 15, c2 = 2 * ln;
        const bool st_d = (NU == 512) || tid < NU, st_e = (NU == 512) || tid >= NU;
        const int nqg = (fs.KC * fs.strips) >> 1, nqm = fs.strips >> 1;       // 16-B units of partials per sample (<= 128, <= 32)
        // (workspace addresses as a uniform base + a 32-bit byte offset per lane -- all of it is < 2 MB here: one VGPR per address)
        auto ld16 = [](const double* base, unsigned byte_off) {
            return *reinterpret_cast<const v2d*>(reinterpret_cast<const char*>(base) + byte_off);
        };
        const unsigned qg0 = (unsigned)(b * nqg) * 16u, qm0 = (unsigned)(b * nqm) * 16u;
        v2d qg[NQG], qm[2];
#pragma unroll
        for (int k = 0; k < NQG; ++k) qg[k] = ld16(fs.Qg, qg0 + 16u * (unsigned)(ln + 16 * k < nqg ? ln + 16 * k : nqg - 1));
        [[maybe_unused]] double mvq = 0.0;
        if constexpr (QMW) mvq = fs.Qm[b];
        else {
#pragma unroll
            for (int k = 0; k < 2; ++k) qm[k] = ld16(fs.Qm, qm0 + 16u * (unsigned)(ln + 16 * k < nqm ? ln + 16 * k : nqm - 1));
        }
        // (round 11) mu0 of the mean epilogues, 8 B per lane, with this first batch, on wave 0 (whose lanes tid < 32 use it) whatever
        // the workgroup is: every vector load that a later wait is counted against is issued behind the join, so the branch costs
        // no wait, and with S0L the loads stand in front of the S0 units.  (On all eight waves: the same tail, 0.04 us more in
        // every workgroup's load and staging phases.)  Loaded where it is used -- behind the stores of S -- it put s_waitcnt
        // vmcnt(0) between the mirror stores and the mu store, and with it a full drain of the write-through stores in front of
        // the folded tile's store.
        if (w == 0) {
            mu0I = mu0[I0 + (tid & 31)];
            if constexpr (FOLD) mu0X = mu0[X0 + (tid & 31)];
        }
        const int col[3] = {I0 + c2, J0 + c2, J0 + 32 + c2};
        const size_t slab = (size_t)B * D;
        v2d xv[3], m0[3], sl[3][KCT];
        auto load_block = [&](int cb) {          // X, mu0 and the slabs (beyond KC: a re-read of the last one, dropped below) of one column block
            xv[cb] = *reinterpret_cast<const v2d*>(fs.X + (size_t)b * fs.ldx + col[cb]);
            m0[cb] = ld16(mu0, 8u * (unsigned)col[cb]);
#pragma unroll
            for (int kc = 0; kc < KCT; ++kc)
                sl[cb][kc] = *reinterpret_cast<const v2d*>(fs.Pp + (size_t)(KCT == 2 ? kc : (kc < fs.KC ? kc : fs.KC - 1)) * slab + (size_t)b * D + col[cb]);
        };
        load_block(0);
        load_block(1);
        if constexpr (KCT == 2) {                // one batch: the second column block goes out with everything else
            if (two) load_block(2);
        }
        if constexpr (S0L) {                     // the S0 units: the last global loads of the kernel (2, and a third with FOLD);
            // (the dbg & 2 ablation of the record form is not honoured here: the "cov_dbg" diagnostic never takes this route)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                [[maybe_unused]] const int unit = q * 256 + tl;
                if constexpr (WST)               // (block (wr, wc) in the wave's own layout; the lane column c is shadowed below, not here)
                    s0v[q] = *reinterpret_cast<const v2d*>(S0 + (size_t)(I0 + 16 * wr + ks + 4 * (l & 1) + 8 * q) * lds0 + Jt + 16 * wc + (l & 14));
                else s0v[q] = *reinterpret_cast<const v2d*>(S0 + (size_t)(I0 + (unit >> 4)) * lds0 + Jt + 2 * (unit & 15));
            }
            if constexpr (FOLD) {
                const int xr = fold ? X0 + (tid >> 4) : I0 + ((256 + tl) >> 4), xc = fold ? X0 + 2 * (tid & 15) : Jt + 2 * (tl & 15);
                s0x = *reinterpret_cast<const v2d*>(S0 + (size_t)xr * lds0 + xc);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        double gs = 0.0, ms = 0.0;               // this lane's share of sample b's partial dots, in unit order
#pragma unroll
        for (int k = 0; k < NQG; ++k) {
            const bool in = ln + 16 * k < nqg;
            gs += in ? qg[k].x : 0.0;
            gs += in ? qg[k].y : 0.0;
        }
        if constexpr (!QMW) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const bool in = ln + 16 * k < nqm;
                ms += in ? qm[k].x : 0.0;
                ms += in ? qm[k].y : 0.0;
            }
        }
        // SECOND batch (KCT = 4), behind the sums (the empty asm pins them in front of it): the second column block, which is staged
        // last, takes the registers the partials held.  (block-uniform: the single-tile workgroups have no second column block)
        if constexpr (KCT == 4) {
            asm volatile("" : "+v"(gs), "+v"(ms) : : "memory");
            if (two) load_block(2);
        }
        // the scalars of sample b, by the expressions of k_gsm_scalars_fast
        const double gSg = row16_sum(gs);
        double mv;
        if constexpr (QMW) mv = mvq;
        else mv = row16_sum(ms);
        const double rho = 0.5 * sqrt(1.0 + 4.0 * (gSg + mv * mv)) - 0.5;
        const double den = 1.0 + rho + mv;
        double beta = 1.0 / (1.0 + rho), c = (gSg - mv) / den;
        if (stamps) {                            // "loads landed": with S0 last, the staged units -- the S0 units stay outstanding
            if constexpr (!S0L) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if constexpr (FOLD) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            STAMP(1);
        }
#pragma unroll
        for (int cb = 0; cb < 3; ++cb)
            if (cb < 2 || two) {
                v2d sg = {0.0, 0.0}, dd, dm, ee;
                // (round 9) the square root and the two divisions need the partials only, which come back first: the empty asm makes
                // every slab, X and mu0 unit pass through a statement that takes beta and c, so that no slab add -- and with it the
                // wait for all 20 units -- can be scheduled in front of that chain (it was); block by block, in staging order
                if constexpr (KCT == 2) {
                    if (cb == 0) asm volatile("" : "+v"(beta), "+v"(c), "+v"(xv[0]), "+v"(m0[0]), "+v"(sl[0][0]), "+v"(sl[0][1]));
                    else asm volatile("" : "+v"(xv[cb]), "+v"(m0[cb]), "+v"(sl[cb][0]), "+v"(sl[cb][1]));
                }
                if constexpr (KCT == 2) {
                    sg.x = sl[cb][0].x + sl[cb][1].x;
                    sg.y = sl[cb][0].y + sl[cb][1].y;
                } else {
#pragma unroll
                    for (int kc = 0; kc < 4; ++kc) {
                        sg.x += (kc < fs.KC) ? sl[cb][kc].x : 0.0;
                        sg.y += (kc < fs.KC) ? sl[cb][kc].y : 0.0;
                    }
                }
                dd.x = m0[cb].x - xv[cb].x;
                dd.y = m0[cb].y - xv[cb].y;
                dm.x = beta * ((sg.x - dd.x) - c * dd.x);
                dm.y = beta * ((sg.y - dd.y) - c * dd.y);
                ee.x = dd.x + dm.x;
                ee.y = dd.y + dm.y;
                if (st_d) *reinterpret_cast<v2d*>(smem + (2 * cb) * TILE + b * RS + c2) = dd;
                if (st_e) *reinterpret_cast<v2d*>(smem + (2 * cb + 1) * TILE + b * RS + c2) = ee;
                if (cb == 0) dmuI = dm;
                if constexpr (FOLD) {
                    if (cb == (fold == 2 ? 2 : 0)) dmuX = dm;
                }
            }
    } else {
#pragma unroll
        for (int q = 0; q < UPT; ++q) {
            const int g = q * 512 + tid;             // global unit over six tiles
            const int tile = g / NU, u = g % NU;     // NU is a power of two
            const int b = u >> 4, c2 = 2 * (u & 15);
            // tile 0,1: I block (d, e); 2,3: J0 block; 4,5: J1 block (= J0 again when there is no second tile)
            const int colbase = (tile < 2) ? I0 : (J0 + ((tile >= 4 && two) ? 32 : 0));
            const int colc = (RAG && colbase + c2 >= D) ? D - 2 : colbase + c2;   // (a column beyond D only feeds outputs that are not stored)
            // the 16 single-tile workgroups (they share a CU with a two-tile one) neither load nor stage a second column
            // block, and their waves 4-7 issue no MFMA: 32 instead of 64 MFMAs per SIMD on those CUs (they were the
            // kernel's 0.9 us tail: profiles/r02/timeline_cold_three_launch.txt).  tile is wave-uniform.
            // (any B <= SB: sample rows b >= B do not exist -- the address is clamped and the unit is zeroed at staging time,
            // so that no use of a loaded value sits between the loads)
            stg[q] = (two || tile < 4) ? *reinterpret_cast<const v2d*>(rec + (size_t)((RAG && b >= B) ? B - 1 : b) * ldrec + (tile & 1) * D + colc)
                                       : (v2d){0.0, 0.0};
        }
        if (diag && tid < 256) {                     // dmu tile for the new mean: column = tid & 31, samples tid>>5 + 8k
            double dv[SB / 8];
#pragma unroll
            for (int k = 0; k < SB / 8; ++k) {
                const int b = (tid >> 5) + 8 * k, ci = I0 + (tid & 31);
                dv[k] = rec[(size_t)((RAG && b >= B) ? B - 1 : b) * ldrec + 2 * D + ((RAG && ci >= D) ? D - 1 : ci)];
            }
#pragma unroll
            for (int k = 0; k < SB / 8; ++k) dmu_part += (!RAG || (tid >> 5) + 8 * k < B) ? dv[k] : 0.0;
        }
    }
    if (!FROM_SLABS && stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); STAMP(1); }

    // ---- per pass of SBP samples: factor tiles -> LDS verbatim, then MFMA.  One 16x16 block per wave;
    // chain 0 = d-part, chain 1 = e-part; operands go to registers first so the chains issue back to back.
    constexpr int NS = SBP / 4;
    v4d accd = {0.0, 0.0, 0.0, 0.0}, acce = {0.0, 0.0, 0.0, 0.0};
    v4d xaccd = {0.0, 0.0, 0.0, 0.0}, xacce = {0.0, 0.0, 0.0, 0.0};   // FOLD: the folded tile's chains
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
        if (pass > 0) PRE_W_BARRIER();           // the previous pass's operand reads are done
        if constexpr (!FROM_SLABS) {             // (FROM_SLABS staged its tiles above)
#pragma unroll
            for (int q = 0; q < UPT; ++q) {
                const int g = q * 512 + tid;
                const int tile = g / NU, u = g % NU;
                const int b = u >> 4;
                if (b / SBP == pass && (two || tile < 4))
                    *reinterpret_cast<v2d*>(smem + tile * TILE + (b % SBP) * RS + 2 * (u & 15)) = (!RAG || b < B) ? stg[q] : (v2d){0.0, 0.0};
            }
        }
        PRE_W_BARRIER();
        if (pass == 0) STAMP(2);
        double ad[NS], ae[NS], bd[NS], be[NS];
        if (mine) {
            const double* adp = smem + ks * RS + 16 * wr + c;
            const double* aep = adp + TILE;
            const double* bdp = smem + (2 + 2 * t) * TILE + ks * RS + 16 * wc + c;
            const double* bep = bdp + TILE;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                ad[s] = adp[4 * s * RS];
                ae[s] = aep[4 * s * RS];
                bd[s] = bdp[4 * s * RS];
                be[s] = bep[4 * s * RS];
            }
        }
        if (mine && !(dbg & 8)) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                accd = GSMVI_MFMA_F64(ad[s], bd[s], accd);
                acce = GSMVI_MFMA_F64(ae[s], be[s], acce);
            }
        }
        if constexpr (FOLD) {                    // the folded diagonal tile: block (wr, wc) on wave w < 4, both operands from block X,
            if (fold && t == 0) {                // (wave-uniform) behind the wave's own block, in the registers that one has freed.
                // (Reading these operands between the MFMA steps of tile 0 let the compiler interleave all four chains: 128 VGPRs
                // and 68 B of scratch; one tile after the other keeps 97 VGPRs and no scratch.)
                const double* xdp = smem + (fold == 2 ? 4 : 0) * TILE + ks * RS + c;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    ad[s] = xdp[4 * s * RS + 16 * wr];
                    ae[s] = xdp[TILE + 4 * s * RS + 16 * wr];
                    bd[s] = xdp[4 * s * RS + 16 * wc];
                    be[s] = xdp[TILE + 4 * s * RS + 16 * wc];
                }
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    xaccd = GSMVI_MFMA_F64(ad[s], bd[s], xaccd);
                    xacce = GSMVI_MFMA_F64(ae[s], be[s], xacce);
                }
            }
        }
    }
    // ---- WST: every wave forms, stores and mirrors its own block (gsm_cov_wave_store); no barrier, no shared LDS.  A pair of the
    // quad map is never diagonal: no mean here.
    if constexpr (WST) {
        v4d u;
#pragma unroll
        for (int r = 0; r < 4; ++r) u[r] = (accd[r] - acce[r]) * invB;
        if (stamps) {                            // [3] "MFMAs done" (wave 0's), [6] "S0 landed", as without the flag
            asm volatile("" : "+v"(u));
            STAMP(3);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            STAMP(6);
        }
        __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(S, 0, 0, 0);   // (plain stores: not used)
        if constexpr (WT) wrs = __builtin_amdgcn_make_buffer_rsrc(S, 0, (int)(((size_t)(D - 1) * lds + D) * sizeof(double)), 0x00020000);
        double* PB = smem + PBO + w * COV_WST_PB;
        gsm_cov_wave_direct<WT, 1>(u, s0v[0], s0v[1], PB, S, wrs, (size_t)(I0 + 16 * wr) * lds + Jt + 16 * wc, lds, l);
        COV_WAVE_SYNC();
        gsm_cov_wave_mirror<WT, false>(PB, s0v[0], s0v[1], S, wrs, (size_t)(Jt + 16 * wc) * lds + I0 + 16 * wr, lds, l);
        if (stamps) __syncthreads();             // [4] still means "every wave has issued its last store" (the timeline instance only)
        STAMP(4);
        if (stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); STAMP(5); }
        return;
    }
    // ---- stores through LDS, 16 B per lane: the update tile U_t = (D_I^T D_J - E_I^T E_J)/B goes to LDS in accumulator
    // layout; W_t = S0[I, J_t] + U_t is formed in store layout (row segments of 256 B), stored, written back to LDS, and
    // the mirror S[J_t, I] = W_t^T is read from there by columns (row stride 33: conflict-free both ways)
    PRE_W_BARRIER();                             // everyone is done reading the factor tiles
    double* LW = smem + t * 32 * 33;             // [2][32 x 33]
    if (mine) {
#pragma unroll
        for (int r = 0; r < 4; ++r) LW[(16 * wr + ks + 4 * r) * 33 + 16 * wc + c] = (accd[r] - acce[r]) * invB;
    }
    // FOLD: the folded tile's update goes behind the two, [3][32 x 33], and the dmu tile of its block behind that -- both inside
    // the staged tiles' LDS and outside everything the two tiles use below, so the folded tile's mean rides on the barriers that
    // are here anyway (two-level order of the record form, as for block I below) and its store goes out last, behind the mirror
    constexpr int LXO = 2 * 32 * 33, MUO = 3 * 32 * 33;
    if constexpr (FOLD) {
        static_assert(!FOLD || MUO + SB * 32 + 256 <= 6 * TILE, "third LW buffer and the dmu tile inside the staged tiles");
        if (fold && t == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) smem[LXO + (16 * wr + ks + 4 * r) * 33 + 16 * wc + c] = (xaccd[r] - xacce[r]) * invB;
        }
        if (fold && tid < NU) *reinterpret_cast<v2d*>(smem + MUO + (tid >> 4) * 32 + 2 * (tid & 15)) = dmuX;
    }
    if (stamps) STAMP(3);
    PRE_W_BARRIER();
    if constexpr (S0L) {                         // "S0 landed": the first wait that reaches 0 stands here, in front of the W step
        if (stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); STAMP(6); }
    }
    // WT: the stores of S go write-through through a buffer descriptor over S (aux 16 = sc1)
    [[maybe_unused]] __amdgpu_buffer_rsrc_t srs;
    if constexpr (WT) srs = __builtin_amdgcn_make_buffer_rsrc(S, 0, (int)(((size_t)(D - 1) * lds + D) * sizeof(double)), 0x00020000);
    [[maybe_unused]] auto store_wt = [&](size_t off, v2d v) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v), srs, (int)(off * sizeof(double)), 0, 16);
    };
    if constexpr (FOLD) {
        if (fold && tid < 256) {
            double part = 0.0;
#pragma unroll
            for (int k = 0; k < SB / 8; ++k) part += smem[MUO + ((tid >> 5) + 8 * k) * 32 + (tid & 31)];
            smem[MUO + SB * 32 + tid] = part;    // [8][32] behind the tile
        }
    }
    if (mine) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int unit = q * 256 + tl, i = unit >> 4, j2 = unit & 15;
            v2d wv2;
            wv2.x = s0v[q].x + LW[i * 33 + 2 * j2];
            wv2.y = s0v[q].y + LW[i * 33 + 2 * j2 + 1];
            if constexpr (WT) store_wt((size_t)(I0 + i) * lds + Jt + 2 * j2, wv2);
            else if (!RAG || (I0 + i < D && Jt + 2 * j2 < D)) *reinterpret_cast<v2d*>(S + (size_t)(I0 + i) * lds + Jt + 2 * j2) = wv2;
            LW[i * 33 + 2 * j2] = wv2.x;
            LW[i * 33 + 2 * j2 + 1] = wv2.y;
        }
    }
    const bool need = mine && !(t == 0 && diag) && !(dbg & 1);
    // (round 11) S0 last: the folded tile's S0 unit came in right behind the two above.  Waited for HERE the wait is counted and
    // free; left to its use behind the mirror branch it is a vmcnt(2) at the join (the path without mirror stores has two
    // stores behind the unit), which in a host waits for three of the four write-through stores to be acknowledged.
    if constexpr (FOLD && S0L) asm volatile("" : "+v"(s0x));
    __syncthreads();
    if (need) {
        // unit = (row j of J_t, column pair i2 of I): S[J_t + j][I0 + 2 i2 .. + 1] = W_t[2 i2 .. + 1][j]
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int unit = q * 256 + tl, j = unit >> 4, i2 = unit & 15;
            v2d m2;
            m2.x = LW[(2 * i2) * 33 + j];
            m2.y = LW[(2 * i2 + 1) * 33 + j];
            if constexpr (WT) store_wt((size_t)(Jt + j) * lds + I0 + 2 * i2, m2);
            else if (!RAG || (Jt + j < D && I0 + 2 * i2 < D)) *reinterpret_cast<v2d*>(S + (size_t)(Jt + j) * lds + I0 + 2 * i2) = m2;
        }
    }
    if constexpr (FOLD) {
        if (fold) {
            // W = S0 + U in store layout, one unit per thread; a diagonal tile has no mirror
            const int i = tid >> 4, j2 = tid & 15;
            v2d wv2;
            wv2.x = s0x.x + smem[LXO + i * 33 + 2 * j2];
            wv2.y = s0x.y + smem[LXO + i * 33 + 2 * j2 + 1];
            if constexpr (WT) store_wt((size_t)(X0 + i) * lds + X0 + 2 * j2, wv2);
            else *reinterpret_cast<v2d*>(S + (size_t)(X0 + i) * lds + X0 + 2 * j2) = wv2;
            // (round 11) the mean BEHIND the folded tile's store: the 8 KB of S are what the launch ends on, the eight LDS reads
            // and adds of these 32 lanes stood in front of wave 0's share of them
            if (tid < 32) {
                double s = 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q) s += smem[MUO + SB * 32 + q * 32 + tid];
                mu_out[X0 + tid] = mu0X + s * invB;
            }
        }
    }
    if (diag) {
        __syncthreads();
        if constexpr (FROM_SLABS) {              // the dmu tile of block I [SB][32] through LDS: the two-level order of the record form
            if (tid < NU) *reinterpret_cast<v2d*>(smem + (tid >> 4) * 32 + 2 * (tid & 15)) = dmuI;
            __syncthreads();
            if (tid < 256) {
#pragma unroll
                for (int k = 0; k < SB / 8; ++k) dmu_part += smem[((tid >> 5) + 8 * k) * 32 + (tid & 31)];
                smem[SB * 32 + tid] = dmu_part;  // [8][32] behind the tile
            }
        } else {
            if (tid < 256) smem[tid] = dmu_part; // [8][32]
        }
        __syncthreads();
        if (tid < 32) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) s += smem[(FROM_SLABS ? SB * 32 : 0) + q * 32 + tid];
            if (!RAG || I0 + tid < D) mu_out[I0 + tid] = (FROM_SLABS ? mu0I : mu0[I0 + tid]) + s * invB;
        }
    }
    STAMP(4);
    if (stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); STAMP(5); }
#undef STAMP
#undef PRE_W_BARRIER
}

template <int SB, bool RAG, bool FROM_SLABS = false, int KCT = 4, bool FOLD = false, bool S0L = false, bool WT = false, bool QMW = false, bool QUAD = false,
          bool WST = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(FROM_SLABS && !(WST && SB == 32) ? 4 : 2))) void k_gsm_cov_sym(int D, int B, double invB, const double* __restrict__ rec, int ldrec,
                                                     const double* __restrict__ mu0,
                                                     const double* __restrict__ S0, int lds0,
                                                     double* __restrict__ S, int lds,
                                                     double* __restrict__ mu_out, int dbg,
                                                     unsigned long long* __restrict__ stamps, gsm_slab_src fs) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    gsm_cov_sym_body<SB, RAG, FROM_SLABS, KCT, FOLD, S0L, WT, QMW, QUAD, WST>(t0, D, B, invB, rec, ldrec, mu0, S0, lds0, S, lds, mu_out, dbg, stamps, fs);
}

// =====================================================================================
// PERSISTENT form of k_gsm_cov_sym for large D (round 4).  Same tiles, same arithmetic, same results bit for bit: a work ITEM
// is what one workgroup of k_gsm_cov_sym does (row block I of 32 rows x two adjacent column tiles, or a lone diagonal tile).
// At D = 4096 there are 4160 items and the one-item kernel ran them as 4160 workgroups, two resident per CU, each a serial
// chain load (16 KB of S0 from HBM + 48 KB of record tiles from L2) -> LDS -> MFMA -> stores (32 KB): 53.9 us for 201 MB =
// 3.7 TB/s, 0.59 of what a plain copy reaches on the box -- the memory pipes of a CU idle while its workgroups compute.
// Here 2 workgroups per CU stay resident and walk the item list (item = blockIdx.x, + gridDim.x, ...); the NEXT item's global
// loads (8 v2d per thread: two S0 units, six record units) are issued as soon as the current item's record tiles have gone
// to LDS, so they are in flight during the current item's operand reads, MFMAs, LDS round trips and stores (loads and stores
// share the in-order vmcnt counter: the next iteration waits for the loads only, the stores behind them stay in flight).
// =====================================================================================
template <int SB, bool RAG>
__global__ __launch_bounds__(512) void k_gsm_cov_sym_p(int D, int B, double invB, const double* __restrict__ rec, int ldrec,
                                                       const double* __restrict__ mu0,
                                                       const double* __restrict__ S0, int lds0,
                                                       double* __restrict__ S, int lds,
                                                       double* __restrict__ mu_out) {
    // Workgroup barrier that waits for this wave's LDS operations ONLY.  __syncthreads() carries a workgroup-scope fence, which
    // on gfx950 drains the vector-memory counter as well (s_waitcnt vmcnt(0)): every one of the five barriers of an item would
    // wait for the NEXT item's loads issued in front of it -- the first version of this kernel did exactly that and ran 27 %
    // slower than the one-item kernel.  No thread of the workgroup reads global data another thread of it wrote, so the barriers
    // only have to order LDS.
#define LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
    constexpr int RS = 48;
    constexpr int NPASS = (SB > 32) ? SB / 32 : 1;
    constexpr int SBP = SB / NPASS;
    constexpr int TILE = SBP * RS;
    constexpr int NU = SB * 16;
    constexpr int UPT = (6 * NU) / 512;
    static_assert((6 * NU) % 512 == 0, "tile units must divide over 512 threads");
    __shared__ __attribute__((aligned(16))) double smem[6 * TILE >= 2 * 32 * 33 ? 6 * TILE : 2 * 32 * 33];
    const int nt = (D + 31) >> 5;                            // (any even D: edge tiles as in k_gsm_cov_sym)
    const int n_two = ((nt >> 1) * ((nt + 1) >> 1));
    const int n_items = n_two + ((nt + 1) >> 1);             // + one lone diagonal tile per row with an odd tile count
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, c = l & 15, ks = l >> 4;
    const int t = w >> 2;
    const int wr = (w >> 1) & 1, wc = w & 1;
    const int tl = tid & 255;

    struct Item { int ti, tj0; bool two; };
    // incremental decode of the two-tile items (row ti holds (nt - ti) >> 1 of them): the scan continues where the last one stopped
    int scan_ti = 0, scan_base = 0;                          // scan_base = first item index of row scan_ti
    auto decode = [&](int item) -> Item {
        Item it;
        if (item < n_two) {
            for (;;) {
                const int inrow = (nt - scan_ti) >> 1;
                if (item - scan_base < inrow) break;
                scan_base += inrow;
                ++scan_ti;
            }
            it.ti = scan_ti;
            it.tj0 = scan_ti + ((nt - scan_ti) & 1) + 2 * (item - scan_base);
            it.two = true;
        } else {
            const int k = item - n_two;
            it.ti = ((nt & 1) ? 0 : 1) + 2 * k;
            it.tj0 = it.ti;
            it.two = false;
        }
        return it;
    };
    v2d s0v[2], stg[UPT];
    double dmuv[SB / 8];                                     // (kept as loaded: summing here would wait for the loads just issued)
    auto issue_loads = [&](const Item& it, v2d (&s0)[2], double (&dmu)[SB / 8]) {
        const int I0 = it.ti * 32, J0 = it.tj0 * 32;
        const int Jt = J0 + 32 * ((t == 1 && it.two) ? 1 : 0);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int unit = q * 256 + tl, i = unit >> 4, j2 = unit & 15;
            const int gr = (RAG && I0 + i >= D) ? D - 1 : I0 + i, gc = (RAG && Jt + 2 * j2 >= D) ? D - 2 : Jt + 2 * j2;
            s0[q] = *reinterpret_cast<const v2d*>(S0 + (size_t)gr * lds0 + gc);
        }
        __builtin_amdgcn_sched_barrier(0);                   // the HBM loads of S0 ahead of the L2-resident record loads
#pragma unroll
        for (int q = 0; q < UPT; ++q) {
            const int g = q * 512 + tid;
            const int tile = g / NU, u = g % NU;
            const int b = u >> 4, c2 = 2 * (u & 15);
            const int colbase = (tile < 2) ? I0 : (J0 + ((tile >= 4 && it.two) ? 32 : 0));
            const int colc = (RAG && colbase + c2 >= D) ? D - 2 : colbase + c2;
            stg[q] = (it.two || tile < 4) ? *reinterpret_cast<const v2d*>(rec + (size_t)((RAG && b >= B) ? B - 1 : b) * ldrec + (tile & 1) * D + colc)
                                          : (v2d){0.0, 0.0};
        }
#pragma unroll
        for (int k = 0; k < SB / 8; ++k) dmu[k] = 0.0;
        if (it.tj0 == it.ti && tid < 256) {
#pragma unroll
            for (int k = 0; k < SB / 8; ++k) {
                const int b = (tid >> 5) + 8 * k, ci = I0 + (tid & 31);
                dmu[k] = rec[(size_t)((RAG && b >= B) ? B - 1 : b) * ldrec + 2 * D + ((RAG && ci >= D) ? D - 1 : ci)];
            }
        }
    };
    int item = blockIdx.x;
    if (item >= n_items) return;
    Item cur = decode(item);
    issue_loads(cur, s0v, dmuv);
    while (true) {
        const bool two = cur.two, diag = (cur.tj0 == cur.ti);
        const int I0 = cur.ti * 32, J0 = cur.tj0 * 32;
        const int Jt = J0 + 32 * ((t == 1 && two) ? 1 : 0);
        const bool mine = (t == 0) || two;
        constexpr int NS = SBP / 4;
        v4d accd = {0.0, 0.0, 0.0, 0.0}, acce = {0.0, 0.0, 0.0, 0.0};
        const int nxt = item + gridDim.x;
        Item nx = cur;
        v2d s0n[2] = {s0v[0], s0v[1]};
        double dmun[SB / 8];
#pragma unroll
        for (int k = 0; k < SB / 8; ++k) dmun[k] = 0.0;
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) {
            if (pass > 0) LDS_BARRIER();
#pragma unroll
            for (int q = 0; q < UPT; ++q) {
                const int g = q * 512 + tid;
                const int tile = g / NU, u = g % NU;
                const int b = u >> 4;
                if (b / SBP == pass && (two || tile < 4))
                    *reinterpret_cast<v2d*>(smem + tile * TILE + (b % SBP) * RS + 2 * (u & 15)) = (!RAG || b < B) ? stg[q] : (v2d){0.0, 0.0};
            }
            LDS_BARRIER();
            if (pass == NPASS - 1 && nxt < n_items) {        // the staging registers are free: the next item's loads go out now
                nx = decode(nxt);
                issue_loads(nx, s0n, dmun);
            }
            double ad[NS], ae[NS], bd[NS], be[NS];
            if (mine) {
                const double* adp = smem + ks * RS + 16 * wr + c;
                const double* aep = adp + TILE;
                const double* bdp = smem + (2 + 2 * t) * TILE + ks * RS + 16 * wc + c;
                const double* bep = bdp + TILE;
#pragma unroll
                for (int sI = 0; sI < NS; ++sI) {
                    ad[sI] = adp[4 * sI * RS];
                    ae[sI] = aep[4 * sI * RS];
                    bd[sI] = bdp[4 * sI * RS];
                    be[sI] = bep[4 * sI * RS];
                }
#pragma unroll
                for (int sI = 0; sI < NS; ++sI) {
                    accd = GSMVI_MFMA_F64(ad[sI], bd[sI], accd);
                    acce = GSMVI_MFMA_F64(ae[sI], be[sI], acce);
                }
            }
        }
        LDS_BARRIER();                                     // everyone is done reading the factor tiles
        double* LW = smem + t * 32 * 33;
        if (mine) {
#pragma unroll
            for (int r = 0; r < 4; ++r) LW[(16 * wr + ks + 4 * r) * 33 + 16 * wc + c] = (accd[r] - acce[r]) * invB;
        }
        LDS_BARRIER();
        if (mine) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int unit = q * 256 + tl, i = unit >> 4, j2 = unit & 15;
                v2d wv2;
                wv2.x = s0v[q].x + LW[i * 33 + 2 * j2];
                wv2.y = s0v[q].y + LW[i * 33 + 2 * j2 + 1];
                if (!RAG || (I0 + i < D && Jt + 2 * j2 < D)) *reinterpret_cast<v2d*>(S + (size_t)(I0 + i) * lds + Jt + 2 * j2) = wv2;
                LW[i * 33 + 2 * j2] = wv2.x;
                LW[i * 33 + 2 * j2 + 1] = wv2.y;
            }
        }
        const bool need = mine && !(t == 0 && diag);
        LDS_BARRIER();
        if (need) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int unit = q * 256 + tl, j = unit >> 4, i2 = unit & 15;
                v2d m2;
                m2.x = LW[(2 * i2) * 33 + j];
                m2.y = LW[(2 * i2 + 1) * 33 + j];
                if (!RAG || (Jt + j < D && I0 + 2 * i2 < D)) *reinterpret_cast<v2d*>(S + (size_t)(Jt + j) * lds + I0 + 2 * i2) = m2;
            }
        }
        if (diag) {                                          // (block-uniform)
            LDS_BARRIER();
            if (tid < 256) {
                double dsum = 0.0;
#pragma unroll
                for (int k = 0; k < SB / 8; ++k) dsum += (!RAG || (tid >> 5) + 8 * k < B) ? dmuv[k] : 0.0;
                smem[tid] = dsum;
            }
            LDS_BARRIER();
            if (tid < 32) {
                double sm_ = 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q) sm_ += smem[q * 32 + tid];
                if (!RAG || I0 + tid < D) mu_out[I0 + tid] = mu0[I0 + tid] + sm_ * invB;
            }
        }
        if (nxt >= n_items) break;
        LDS_BARRIER();                                     // the LDS tiles of this item are dead: the next item may stage
        item = nxt;
        cur = nx;
        s0v[0] = s0n[0];
        s0v[1] = s0n[1];
#pragma unroll
        for (int k = 0; k < SB / 8; ++k) dmuv[k] = dmun[k];
    }
}

// gsmvi_fast_hot.hip includes this file for the templates above (the shared bodies) and stops here: the kernel and the launch
// helpers below belong to this translation unit alone.
#ifndef GSMVI_FAST_BODIES_ONLY
// =====================================================================================
// k_gsm_cov_sym for ANY batch size (round 6; until then B <= 128 only and B = 130 fell to the guarded kernel of
// gsmvi_kernels.hip).  Same items, same tile layout, same store path as k_gsm_cov_sym; the samples come in a RUN-TIME loop of
// 32-sample passes instead of SB / 32 compile-time passes over registers loaded up front:
//   * the six record tiles of a pass are exactly one 16-byte unit per thread and tile (32 samples x 16 units = 512);
//   * two register sets (even / odd passes): the loads of pass p + 2 are issued as soon as pass p has gone to LDS, so they fly
//     during two passes of operand reads and MFMAs (~1 us each on a CU: 16 fp64 MFMAs per wave, two waves per SIMD);
//   * LDS-only barriers (s_waitcnt lgkmcnt(0); s_barrier) as in the persistent form: __syncthreads() would drain the prefetch;
//   * sample rows b >= B of the last pass are clamped re-reads staged as zeros; edge tiles (D % 32 != 0) as RAG = true above.
// MFMA-bound (2 B D^2 flop on the upper triangle: 1.07 GFLOP at D = 1024, B = 512 against 17 MB of covariance), one item per
// workgroup; the mean's dmu tile rides in the same passes on the diagonal workgroups.
// =====================================================================================
__global__ __launch_bounds__(512) void k_gsm_cov_sym_big(int D, int B, double invB, const double* __restrict__ rec, int ldrec,
                                                         const double* __restrict__ mu0,
                                                         const double* __restrict__ S0, int lds0,
                                                         double* __restrict__ S, int lds,
                                                         double* __restrict__ mu_out) {
    constexpr int RS = 48;
    constexpr int TILE = 32 * RS;
    __shared__ __attribute__((aligned(16))) double smem[6 * TILE];
    const int nt = (D + 31) >> 5;
    const int n_two = ((nt >> 1) * ((nt + 1) >> 1));
    int ti, tj0;
    bool two;
    if ((int)blockIdx.x < n_two) {
        int rem = blockIdx.x;
        ti = 0;
        for (;;) {
            const int inrow = (nt - ti) >> 1;
            if (rem < inrow) break;
            rem -= inrow;
            ++ti;
        }
        tj0 = ti + ((nt - ti) & 1) + 2 * rem;
        two = true;
    } else {
        const int k = blockIdx.x - n_two;
        ti = ((nt & 1) ? 0 : 1) + 2 * k;
        tj0 = ti;
        two = false;
    }
    const bool diag = (tj0 == ti);
    const int I0 = ti * 32, J0 = tj0 * 32;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, c = l & 15, ks = l >> 4;
    const int t = w >> 2;
    const int wr = (w >> 1) & 1, wc = w & 1;
    const bool mine = (t == 0) || two;
    const int Jt = J0 + 32 * ((t == 1 && two) ? 1 : 0);
    const int tl = tid & 255;
    v2d s0v[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int unit = q * 256 + tl, i = unit >> 4, j2 = unit & 15;
        const int gr = (I0 + i >= D) ? D - 1 : I0 + i, gc = (Jt + 2 * j2 >= D) ? D - 2 : Jt + 2 * j2;
        s0v[q] = *reinterpret_cast<const v2d*>(S0 + (size_t)gr * lds0 + gc);
    }
    __builtin_amdgcn_sched_barrier(0);
    const int npass = (B + 31) >> 5;
    const int sb = tid >> 4, sc2 = 2 * (tid & 15);               // this thread's unit of every tile: sample row, column pair
    const int dcol = (I0 + (tid & 31) >= D) ? D - 1 : I0 + (tid & 31);
    auto issue = [&](int pass, v2d (&sg)[6], double (&dm)[4]) {
        const int bb = pass * 32 + sb;
        const double* rp = rec + (size_t)(bb < B ? bb : B - 1) * ldrec;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int colbase = (q < 2) ? I0 : (J0 + ((q >= 4 && two) ? 32 : 0));
            const int colc = (colbase + sc2 >= D) ? D - 2 : colbase + sc2;
            sg[q] = (two || q < 4) ? *reinterpret_cast<const v2d*>(rp + (q & 1) * D + colc) : (v2d){0.0, 0.0};
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) dm[k] = 0.0;
        if (diag && tid < 256) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int b = pass * 32 + (tid >> 5) + 8 * k;
                dm[k] = rec[(size_t)(b < B ? b : B - 1) * ldrec + 2 * D + dcol];
            }
        }
    };
    v4d accd = {0.0, 0.0, 0.0, 0.0}, acce = {0.0, 0.0, 0.0, 0.0};
    double dmu_part = 0.0;
    auto do_pass = [&](int pass, v2d (&sg)[6], double (&dm)[4]) {
        if (pass > 0) LDS_BARRIER();                             // the previous pass's operand reads are done
        const bool live = pass * 32 + sb < B;
#pragma unroll
        for (int q = 0; q < 6; ++q)
            if (two || q < 4) *reinterpret_cast<v2d*>(smem + q * TILE + sb * RS + sc2) = live ? sg[q] : (v2d){0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 4; ++k) dmu_part += (pass * 32 + (tid >> 5) + 8 * k < B) ? dm[k] : 0.0;
        LDS_BARRIER();
        if (pass + 2 < npass) issue(pass + 2, sg, dm);           // this register set is free: two passes ahead
        if (mine) {
            double ad[8], ae[8], bd[8], be[8];
            const double* adp = smem + ks * RS + 16 * wr + c;
            const double* aep = adp + TILE;
            const double* bdp = smem + (2 + 2 * t) * TILE + ks * RS + 16 * wc + c;
            const double* bep = bdp + TILE;
#pragma unroll
            for (int sI = 0; sI < 8; ++sI) {
                ad[sI] = adp[4 * sI * RS];
                ae[sI] = aep[4 * sI * RS];
                bd[sI] = bdp[4 * sI * RS];
                be[sI] = bep[4 * sI * RS];
            }
#pragma unroll
            for (int sI = 0; sI < 8; ++sI) {
                accd = GSMVI_MFMA_F64(ad[sI], bd[sI], accd);
                acce = GSMVI_MFMA_F64(ae[sI], be[sI], acce);
            }
        }
    };
    v2d stgA[6], stgB[6];
    double dmA[4], dmB[4];
    issue(0, stgA, dmA);
    if (npass > 1) issue(1, stgB, dmB);
    for (int pass = 0; pass < npass; pass += 2) {
        do_pass(pass, stgA, dmA);
        if (pass + 1 < npass) do_pass(pass + 1, stgB, dmB);
    }
    // ---- stores: as k_gsm_cov_sym (update tile through LDS, S0 added in store layout, mirror by columns) ----
    LDS_BARRIER();
    double* LW = smem + t * 32 * 33;
    if (mine) {
#pragma unroll
        for (int r = 0; r < 4; ++r) LW[(16 * wr + ks + 4 * r) * 33 + 16 * wc + c] = (accd[r] - acce[r]) * invB;
    }
    LDS_BARRIER();
    if (mine) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int unit = q * 256 + tl, i = unit >> 4, j2 = unit & 15;
            v2d wv2;
            wv2.x = s0v[q].x + LW[i * 33 + 2 * j2];
            wv2.y = s0v[q].y + LW[i * 33 + 2 * j2 + 1];
            if (I0 + i < D && Jt + 2 * j2 < D) *reinterpret_cast<v2d*>(S + (size_t)(I0 + i) * lds + Jt + 2 * j2) = wv2;
            LW[i * 33 + 2 * j2] = wv2.x;
            LW[i * 33 + 2 * j2 + 1] = wv2.y;
        }
    }
    const bool need = mine && !(t == 0 && diag);
    LDS_BARRIER();
    if (need) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int unit = q * 256 + tl, j = unit >> 4, i2 = unit & 15;
            v2d m2;
            m2.x = LW[(2 * i2) * 33 + j];
            m2.y = LW[(2 * i2 + 1) * 33 + j];
            if (Jt + j < D && I0 + 2 * i2 < D) *reinterpret_cast<v2d*>(S + (size_t)(Jt + j) * lds + I0 + 2 * i2) = m2;
        }
    }
    if (diag) {
        LDS_BARRIER();
        if (tid < 256) smem[tid] = dmu_part;
        LDS_BARRIER();
        if (tid < 32) {
            double sm_ = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) sm_ += smem[q * 32 + tid];
            if (I0 + tid < D) mu_out[I0 + tid] = mu0[I0 + tid] + sm_ * invB;
        }
    }
}
#undef LDS_BARRIER

// ---- launch helpers ------------------------------------------------------------------------
void gsmvi_launch_panel_fast(hipStream_t st, hipEvent_t* ev, int MT, dim3 grid, int D, int nrows, const double* A,
                             int lda, const double* shift, double alpha, const double* M, int ldm, double* Pp,
                             int chunks_per_wg, int ncols, unsigned long long* stamps, double* Out, int ldo,
                             const double* addvec, const gsmvi_panel_extras* px) {
    const gsmvi_panel_extras none;
    const bool rider = px && px->rd_on && !shift;
    const bool extra = px && (px->msl || px->sj_src || rider);
    const gsmvi_panel_extras pxv = extra ? *px : none;
    const bool rag = D % 64 != 0 || ncols % 16 != 0;           // off the grid: the clamped instantiation (round 5)
    if (grid.x == 0) return;
    if (px && px->w4 && !rider && !extra && MT <= 2) {           // the prefetching form (the caller checked its preconditions)
#define PFP(MTV, HS) GSMVI_LAUNCH((k_panel_fast_p<MTV, HS>), grid, dim3(512), 0, st, ev, D, nrows, A, lda, shift, alpha, M, ldm, \
                                  Pp, chunks_per_wg, ncols, Out, ldo, addvec)
        if (shift) { if (MT == 1) PFP(1, true); else PFP(2, true); }
        else { if (MT == 1) PFP(1, false); else PFP(2, false); }
#undef PFP
        return;
    }
    if (rider) {
        grid.x += 1;
#define PFR(MTV, CW, RG)                                                                                                 \
    GSMVI_LAUNCH((k_panel_fast<MTV, false, CW, true, true, RG>), grid, dim3(512), 0, st, ev, D, nrows, A, lda, shift, alpha, M, \
                 ldm, Pp, chunks_per_wg, ncols, stamps, Out, ldo, addvec, pxv)
        if (rag) { if (MT == 1) PFR(1, 256, true); else if (MT == 2) PFR(2, 256, true); else PFR(4, 128, true); }
        else { if (MT == 1) PFR(1, 256, false); else if (MT == 2) PFR(2, 256, false); else PFR(4, 128, false); }
#undef PFR
        return;
    }
#define PF(MTV, HS, CW, EX, RG)                                                                                          \
    GSMVI_LAUNCH((k_panel_fast<MTV, HS, CW, EX, false, RG>), grid, dim3(512), 0, st, ev, D, nrows, A, lda, shift, alpha, M, ldm, \
                 Pp, chunks_per_wg, ncols, stamps, Out, ldo, addvec, pxv)
#define PFE(MTV, HS, CW)                                                                \
    do {                                                                                \
        if (rag) { if (extra) PF(MTV, HS, CW, true, true); else PF(MTV, HS, CW, false, true); } \
        else { if (extra) PF(MTV, HS, CW, true, false); else PF(MTV, HS, CW, false, false); }   \
    } while (0)
    if (shift) {
        if (MT == 1) PFE(1, true, 256); else if (MT == 2) PFE(2, true, 256); else PFE(4, true, 128);
    } else {
        if (MT == 1) PFE(1, false, 256); else if (MT == 2) PFE(2, false, 256); else PFE(4, false, 128);
    }
#undef PFE
#undef PF
}

// The product launch of the two-launch dense GSM update: slabs Pp[kc][B][D] of G S0 (grid (D / 16, kc, 1), chunks of 256 rows)
// plus the partial dots Qg, Qm (the caller checked the gate: B in {16, 32} = one row block, D % 256 == 0, aligned operands).
// chw = 512 (round 8; D = 1024 only): grid (D / 16, 2, B / 16), ONE 512-row chunk and 16 samples per workgroup (MT = 1 also at
// B = 32), so the whole split of a workgroup is one load batch (64 KB of G through LDS, 64 KB of S0), there are two slabs and
// 2 D / 16 Qg partials per sample, and B = 32 still fills 256 workgroups.  The two sample halves of a (strip, slab) read the
// same S0 rows; their linear ids differ by 128, the same XCD, and the second read is served from its L2 (DESIGN 8.1, round 8:
// the MT = 2 form on 128 workgroups staged 128 KB per workgroup and was 2 us slower per launch).
// preload (round 15, knob "kernarg_preload"): the entry points of gsmvi_fast_hot.hip, whose first load batch takes its arguments from
// preloaded SGPRs, where they cover the form; returns whether they ran.  The same body, the same bytes.
bool gsmvi_launch_panel_part_hot(hipStream_t st, hipEvent_t* ev, dim3 grid, int D, int B, const double* G, int ldg, const double* S0,
                                 int lds0, double* Pp, int chunks_per_wg, const double* X, int ldx, const double* mu0, double* Qg,
                                 double* Qm, int chw, int stream, unsigned long long* stamps);
bool gsmvi_launch_gsm_cov_slabs_hot(hipStream_t st, hipEvent_t* ev, dim3 grid, int D, int B, const gsm_slab_src& fs, const double* mu0,
                                    const double* S0, int lds0, double* S, int lds, double* mu_out, int kct, bool fold, bool quad,
                                    bool wave_store, unsigned long long* stamps);

bool gsmvi_launch_panel_fast_part(hipStream_t st, hipEvent_t* ev, dim3 grid, int D, int B, const double* G, int ldg,
                                  const double* S0, int lds0, double* Pp, int chunks_per_wg, const double* X, int ldx,
                                  const double* mu0, double* Qg, double* Qm, int chw, bool qm_whole, int stream,
                                  unsigned long long* stamps, bool preload) {
    if (preload && !(chw == 512 && qm_whole)) {    // the instance the chain below would pick, behind the preloaded entry point
        const bool streamed = chw == 512 && stream != 0 && chunks_per_wg == 1 && D == 512 * (int)grid.y && B % 16 == 0;
        const int inst = streamed ? (stream == 4 ? 4 : 2) : ((chw == 512 && stamps != nullptr && chunks_per_wg == 1) ? -1 : 0);
        if (gsmvi_launch_panel_part_hot(st, ev, grid, D, B, G, ldg, S0, lds0, Pp, chunks_per_wg, X, ldx, mu0, Qg, Qm, chw, inst, stamps))
            return true;
    }
    gsmvi_panel_extras px;                     // (PART's arguments ride in free members: gsmvi_ctx.h)
    px.sj_src = X;
    px.sj_len = ldx;
    px.msl = mu0;
    px.sj_dst = Qg;
    px.mfin = Qm;
#define PFQ(MTV, CW) GSMVI_LAUNCH((k_panel_fast<MTV, false, CW, false, false, false, true>), grid, dim3(512), 0, st, ev, D, B, G, ldg, \
                                  nullptr, 1.0, S0, lds0, Pp, chunks_per_wg, D, stamps, nullptr, 0, nullptr, px)
    if (chw == 512 && qm_whole)             // one Qm value per sample from the idle slab-1 workgroups (QMW above)
        GSMVI_LAUNCH((k_panel_fast<1, false, 512, false, false, false, true, true>), grid, dim3(512), 0, st, ev, D, B, G, ldg, nullptr, 1.0, S0,
                     lds0, Pp, chunks_per_wg, D, stamps, nullptr, 0, nullptr, px);
    else if (chw == 512 && stream != 0 && chunks_per_wg == 1 && D == 512 * (int)grid.y && B % 16 == 0) {
        // the left operand streamed per wave (STREAM above; knob "panel_stream"): the same slabs and partials, bit for bit
#define PFS(NS) GSMVI_LAUNCH((k_panel_fast<1, false, 512, false, false, false, true, false, NS>), grid, dim3(512), 0, st, ev, D, B, G, ldg, \
                             nullptr, 1.0, S0, lds0, Pp, chunks_per_wg, D, stamps, nullptr, 0, nullptr, px)
        if (stream == 4) PFS(4); else PFS(2);
    } else if (chw == 512 && stamps != nullptr && chunks_per_wg == 1) {
        PFS(-1);                            // timeline diagnostic: the unstreamed code with its landing profile in words 4 - 7
#undef PFS
    } else if (chw == 512) PFQ(1, 512);
    else { if (B == 16) PFQ(1, 256); else PFQ(2, 256); }
#undef PFQ
    return false;
}

// column width of one staged chunk for a given MT (the ABI's chunk arithmetic must agree)
int gsmvi_panel_fast_chunk(int MT) { return MT == 4 ? 128 : 256; }

// returns false when (D, KC) has no instantiation.  nt = threads per sample-workgroup (tuning knob scalars_nt)
bool gsmvi_launch_gsm_scalars_fast(hipStream_t st, hipEvent_t* ev, int D, int B, int KC, const double* X, int ldx,
                                   const double* G, int ldg, const double* mu0, const double* Pp, double* rec,
                                   int ldrec, int nt, unsigned long long* stamps) {
    if (nt != 256 && nt != 512 && nt != 1024) nt = 512;   // 512 measured best at D=1024 (fewer waves to reduce)
    const int ept = (D + nt - 1) / nt;
#define SF(E, K, N)                                                                                              \
    GSMVI_LAUNCH((k_gsm_scalars_fast<E, K, N>), dim3(B), dim3(N), 0, st, ev, D, B, KC, X, ldx, G, ldg, mu0, Pp, rec, \
                 ldrec, stamps)
#define SFK(E, N) do { if (kct == 1) SF(E, 1, N); else if (kct == 2) SF(E, 2, N); else if (kct == 4) SF(E, 4, N); else SF(E, 8, N); } while (0)
#define SFE(N) do { if (e == 1) SFK(1, N); else if (e == 2) SFK(2, N); else if (e == 4) SFK(4, N); else SFK(8, N); } while (0)
    if (KC > 8 || ept > 8) return false;
    const int kct = KC <= 1 ? 1 : (KC <= 2 ? 2 : (KC <= 4 ? 4 : 8));
    const int e = ept <= 1 ? 1 : (ept <= 2 ? 2 : (ept <= 4 ? 4 : 8));
    if (nt == 256) SFE(256); else if (nt == 512) SFE(512); else SFE(1024);
#undef SFE
#undef SFK
#undef SF
    return true;
}

// number of workgroups of k_gsm_cov_sym: row ti of the upper triangle holds ceil((nt - ti)/2)
static int cov_sym_grid(int nt) {
    int n = 0;
    for (int ti = 0; ti < nt; ++ti) n += (nt - ti + 1) / 2;
    return n;
}

// the two-tile workgroups among them (the kernel's n_two): all of the grid when the diagonal leftovers are folded
int gsmvi_cov_sym_pairs(int nt) { return (nt >> 1) * ((nt + 1) >> 1); }

// the quad / pair map (QUAD of k_gsm_cov_sym; even nt): nt / 2 quads, then nt / 2 - i / 2 - 1 pairs in row i
static int cov_sym_quad_grid(int nt) { return (nt >> 1) * (nt >> 1); }

bool gsmvi_launch_gsm_cov_sym(hipStream_t st, hipEvent_t* ev, int D, int B, const double* rec, int ldrec,
                              const double* mu0, const double* S0, int lds0, double* S, int lds, double* mu_out,
                              int dbg, unsigned long long* stamps, int num_cu) {
    // Any batch size up to 128 (round 5): the kernel is instantiated for SB = 16, 32, 64, 128 staged sample rows and takes the
    // actual B and 1/B at run time -- rows b >= B are staged as zeros (they add nothing to either accumulator chain), so
    // B = 20 runs the SB = 32 instance at the speed of B = 32.  (Until round 4: B in {16, 32, 64} only, everything else fell to
    // the guarded kernel of gsmvi_kernels.hip.)
    if (B < 1) return false;
    if (B > 128) {          // round 6: any batch size -- the run-time pass loop (k_gsm_cov_sym_big); B <= 128 keeps the instances below
        GSMVI_LAUNCH(k_gsm_cov_sym_big, dim3(cov_sym_grid((D + 31) / 32)), dim3(512), 0, st, ev, D, B, 1.0 / (double)B, rec, ldrec,
                     mu0, S0, lds0, S, lds, mu_out);
        return true;
    }
    const int SB = B <= 16 ? 16 : (B <= 32 ? 32 : (B <= 64 ? 64 : 128));
    const double invB = 1.0 / (double)B;
    const bool rag = D % 32 != 0 || B != SB;                     // off the grid: the clamped instantiation
    // large D: the persistent form (2 resident workgroups per CU walk the item list, the next item's loads in flight during
    // the current item's MFMAs and stores); "cov_dbg" bit 512 keeps the one-item-per-workgroup kernel for A/B runs
    const int n_items = cov_sym_grid((D + 31) / 32);
    if (n_items >= 2048 && SB <= 32 && !stamps && dbg == 0) {    // (B = 64: two staging passes, MFMA-bound -- the one-item kernel is faster there)
        const dim3 pgrid(2 * (num_cu > 0 ? num_cu : 256));       // two resident workgroups per CU of THIS device (a partitioned device has fewer)
#define CSP(SBV, RG) GSMVI_LAUNCH((k_gsm_cov_sym_p<SBV, RG>), pgrid, dim3(512), 0, st, ev, D, B, invB, rec, ldrec, mu0, S0, lds0, S, lds, mu_out)
        if (rag) { if (SB == 16) CSP(16, true); else CSP(32, true); }
        else { if (SB == 16) CSP(16, false); else CSP(32, false); }
        return true;
#undef CSP
    }
    if (dbg & 512) dbg &= ~512;
    const dim3 grid(n_items);
#define CS(SBV, RG)                                                                                         \
    GSMVI_LAUNCH((k_gsm_cov_sym<SBV, RG>), grid, dim3(512), 0, st, ev, D, B, invB, rec, ldrec, mu0, S0, lds0, S, lds, mu_out, dbg, \
                 stamps, gsm_slab_src())
    if (rag) {
        switch (SB) {
            case 16: CS(16, true); break;
            case 32: CS(32, true); break;
            case 64: CS(64, true); break;
            default: CS(128, true); break;
        }
    } else {
        switch (SB) {
            case 16: CS(16, false); break;
            case 32: CS(32, false); break;
            case 64: CS(64, false); break;
            default: CS(128, false); break;
        }
    }
#undef CS
    return true;
}

// The covariance launch of the two-launch dense GSM update (the caller checked the gate: B in {16, 32}, D % 256 == 0, D <= 1024,
// KC <= 4, even leading dimensions, 16-byte aligned bases).  Same grid as above.  kct = 2: the instance compiled for exactly two
// slabs (the caller's product ran the 512-row split: fs.KC == 2, D == 1024); kct = 4: any KC <= 4.
// fold (round 9): the grid is the two-tile workgroups alone, the diagonal leftovers are third tiles of their hosts (FOLD above).
// preload: as gsmvi_launch_panel_fast_part (the quad map only); returns whether the preloaded entry point ran.
bool gsmvi_launch_gsm_cov_sym_slabs(hipStream_t st, hipEvent_t* ev, int D, int B, const gsm_slab_src& fs, const double* mu0,
                                    const double* S0, int lds0, double* S, int lds, double* mu_out, int kct, bool fold,
                                    bool s0_last, bool store_wt, bool qm_whole, bool quad, bool wave_store, unsigned long long* stamps,
                                    bool preload) {
    const double invB = 1.0 / (double)B;
    if (preload && !qm_whole &&
        gsmvi_launch_gsm_cov_slabs_hot(st, ev, dim3(quad ? cov_sym_quad_grid(D / 32) : (fold ? gsmvi_cov_sym_pairs(D / 32) : cov_sym_grid(D / 32))),
                                       D, B, fs, mu0, S0, lds0, S, lds, mu_out, kct, fold, quad, wave_store, stamps))
        return true;
    // quad (round 13; the caller passes it for the shipped two-slab form -- S0 last, write-through stores, per-strip Qm -- and for
    // the plain kct = 4 form only): the quad / pair map, (nt / 2)^2 workgroups
    if (quad) {
        const dim3 qgrid(cov_sym_quad_grid(D / 32));
#define CSE(SBV, KV, LV, WV, SV)                                                                                          \
    GSMVI_LAUNCH((k_gsm_cov_sym<SBV, false, true, KV, false, LV, WV, false, true, SV>), qgrid, dim3(512), 0, st, ev, D, B, invB, nullptr, 0, mu0, \
                 S0, lds0, S, lds, mu_out, 0, stamps, fs)
        // round 14 ("cov_wave_store"): the same four instances with the per-wave store path
#define CSD(SBV, KV, LV, WV) do { if (wave_store) CSE(SBV, KV, LV, WV, true); else CSE(SBV, KV, LV, WV, false); } while (0)
        if (kct == 2) { if (B == 16) CSD(16, 2, true, true); else CSD(32, 2, true, true); }
        else { if (B == 16) CSD(16, 4, false, false); else CSD(32, 4, false, false); }
#undef CSD
#undef CSE
        return false;
    }
    const dim3 grid(fold ? gsmvi_cov_sym_pairs(D / 32) : cov_sym_grid(D / 32));
#define CSQ(SBV, KV, FV, LV, WV, QV)                                                                                      \
    GSMVI_LAUNCH((k_gsm_cov_sym<SBV, false, true, KV, FV, LV, WV, QV>), grid, dim3(512), 0, st, ev, D, B, invB, nullptr, 0, mu0, S0, lds0, S, \
                 lds, mu_out, 0, stamps, fs)
    // (whole-sample Qm, "panel_qm_whole": kct == 2 only, the caller passes false otherwise)
#define CSS(SBV, KV, FV, LV, WV) do { if (KV == 2 && qm_whole) CSQ(SBV, 2, FV, LV, WV, true); else CSQ(SBV, KV, FV, LV, WV, false); } while (0)
#define CSF(SBV, KV, LV, WV) do { if (fold) CSS(SBV, KV, true, LV, WV); else CSS(SBV, KV, false, LV, WV); } while (0)
    // round 10 (kct == 2 only; the caller passes false otherwise): S0 issued and waited for last, write-through stores of S
#define CSL(SBV)                                                                                                          \
    do {                                                                                                                  \
        if (s0_last && store_wt) CSF(SBV, 2, true, true);                                                                 \
        else if (s0_last) CSF(SBV, 2, true, false);                                                                       \
        else if (store_wt) CSF(SBV, 2, false, true);                                                                      \
        else CSF(SBV, 2, false, false);                                                                                   \
    } while (0)
    if (kct == 2) { if (B == 16) CSL(16); else CSL(32); }
    else { if (B == 16) CSF(16, 4, false, false); else CSF(32, 4, false, false); }
#undef CSL
#undef CSF
#undef CSS
#undef CSQ
    return false;
}
#endif   // GSMVI_FAST_BODIES_ONLY
