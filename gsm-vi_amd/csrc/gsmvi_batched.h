// Shared pieces of the batched kernels (gsmvi_batched.hip: GSM, gsmvi_bam_batched.hip: BaM, gsmvi_kl_batched.hip: the KL
// monitor; the GLM, L-BFGS, Laplace, predictive and PSIS files): the bounds, the argument block, the wave
// butterflies, the in-LDS Cholesky, the host-side argument checks, and the tail of a fit step that both
// methods run on their new covariance S' -- the Cholesky test, per-problem accept or revert of (mean, cov, sampling factor),
// and the next samples from the problem's Philox stream -- and the slot sum and log-density sum that end a draw.
#pragma once
#include <hip/hip_runtime.h>
#include "gsmvi_philox.h"
#include "gsmvi_ctx.h"
#include "../../include/gsmvi_hip.h"
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#define GB_MAX_D 64
#define GB_MAX_B 32

struct gb_args {
    long long K;
    int D, B;
    const double* X;     // UPDATE, STEP: (K, B, D) samples
    const double* V;     // UPDATE, STEP: (K, B, D) scores
    const double* mu0;   // UPDATE: (K, D)
    const double* S0;    // UPDATE: (K, D, D)
    double* mu;          // UPDATE: output; STEP: the state's mean (in / out); INIT: the mean (in)
    double* S;           // UPDATE: output; STEP: the state's covariance (in / out); INIT: the covariance (in)
    double* R;           // STEP, INIT: the sampling factor, (K, D, D) upper triangular (in / out); may be null in STEP
    int* info;           // STEP, INIT: (K) 0 = positive definite, else 1 + the first bad pivot; may be null
    int* n_rev;          // STEP: (K) incremented on a revert; may be null
    const unsigned long long* seeds;   // STEP, INIT: (K) the problems' draw keys; null = no draw
    unsigned long long call;           // draw number of the samples written
    double* Xout;        // STEP, INIT: (K, B, D) next samples (may alias X: each slot reads its X before it writes)
    // BaM only (gsmvi_bam_batched.hip)
    double reg;          // the regulariser of every problem ...
    const double* reg_dev;   // ... or (K) per-problem values on the device (null: `reg`)
    double jitter;       // added to the diagonal of S' (bam.py:198)
    int ld, ldn;         // LDS row strides of the D x D and n x n arrays
};

// padded draw row: an odd-D problem takes B x (D + 1) normals per draw, column D dropped (the layout of the single fit, _oddpad.py)
__host__ __device__ inline int gb_dz(int D) { return D + (D & 1); }
// threads per problem: four problems (one wave each) per 256-thread workgroup for D <= 16, one problem above
static inline int gb_nt(int D) { return D <= 16 ? 64 : 256; }

// The 64-lane butterflies of the kernels that keep a vector of D <= 64 components one wave wide (L-BFGS, Laplace): a fixed
// order that depends on nothing but the lanes' values, and no barrier
__device__ __forceinline__ double gb_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double gb_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ bool gb_finite(double v) { return fabs(v) < __builtin_huge_val(); }

// Upper Cholesky factor of the problem of one workgroup slot, in place in LDS (S: D x D, row stride ld; only its upper
// triangle is read).  Right-looking, one pivot per barrier (unscaled rows: row c is final after step c and is scaled by
// 1 / sqrt(a_cc) at the end); pv (LDS, D) receives the pivots sqrt(a_cc) = R_cc.  Every thread of a slot reads the same
// pivot, so the result -- 0, or 1 + the first pivot that is not > 0 and finite (NaN included: any NaN of S reaches a later
// pivot), as np.linalg.cholesky fails or the reference's NaN test catches (gsm_numpy.py:139-146) -- is uniform in it.  The
// loop always runs D steps (uniform barriers); no barrier follows the scaling (a thread rewrites only its own entries).
template <int NT, int MAXE>
__device__ __forceinline__ int gb_chol_lds(bool valid, int D, int l, int ld, double* S, double* pv) {
    const int DD = D * D;
    int info = 0;
    for (int c = 0; c < D; ++c) {
        const double acc_ = S[c * ld + c];
        if (info == 0 && !(acc_ > 0.0 && acc_ < __builtin_huge_val())) info = c + 1;
        const double piv = sqrt(acc_), inv = 1.0 / piv;
        if (l == 0) pv[c] = piv;
        if (valid) {
#pragma unroll
            for (int q = 0; q < MAXE; ++q) {
                const int e = l + q * NT;
                if (e < DD) {
                    const int i = e / D, j = e - i * D;
                    if (i > c && j >= i) S[i * ld + j] -= (S[c * ld + i] * inv) * (S[c * ld + j] * inv);
                }
            }
        }
        __syncthreads();
    }
    if (valid) {
#pragma unroll
        for (int q = 0; q < MAXE; ++q) {
            const int e = l + q * NT;
            if (e < DD) {
                const int i = e / D, j = e - i * D;
                S[i * ld + j] = j > i ? S[i * ld + j] / pv[i] : (j == i ? pv[i] : 0.0);
            }
        }
    }
    return info;
}

// The tail of a fit step (MODE_INIT = false) or of the fit's start (MODE_INIT = true), for the problem of one workgroup slot:
//   S    (LDS, D x D, row stride ld)  S' on entry (only the upper triangle is used), its upper Cholesky factor on exit
//   sreg (registers) the entries e = l + q NT of S' (row-major, stride D): what an accept writes to the state's covariance
//   pv   (LDS, D) pivots;  Zb (LDS, B x Dz) the draws;  m0 the kept mean, m1 the new mean (LDS, D each)
// The Cholesky test is gb_chol_lds.  Then per problem: accept -> mean, cov, factor written; revert -> nothing of the state
// is written, n_rev[k] += 1.  With a.seeds: X = m + z R, z = draw a.call of the problem's stream (element n = b Dz + j,
// pair n / 2, gsmvi_rng.hip), from the kept or accepted state.
template <int NT, int MAXE, bool MODE_INIT>
__device__ __forceinline__ void gb_fit_tail(const gb_args& a, bool valid, long long k, int l, int ld, double* S,
                                            const double (&sreg)[MAXE], double* pv, double* Zb, const double* m0, double* m1) {
    const int D = a.D, B = a.B, Dz = gb_dz(D), DD = D * D, BD = B * D;
    const size_t kd = (size_t)(valid ? k : 0) * D, kdd = (size_t)(valid ? k : 0) * DD, kbd = (size_t)(valid ? k : 0) * BD;
    const int info = gb_chol_lds<NT, MAXE>(valid, D, l, ld, S, pv);

    if (valid) {
        if (MODE_INIT) {
            if (a.R)
#pragma unroll
                for (int q = 0; q < MAXE; ++q) {
                    const int e = l + q * NT;
                    if (e < DD) {
                        const int i = e / D, j = e - i * D;
                        a.R[kdd + e] = S[i * ld + j];
                    }
                }
        } else if (info == 0) {                                         // accept: mean, cov, factor   (gsm_numpy.py:121-123)
            for (int i = l; i < D; i += NT) a.mu[kd + i] = m1[i];
#pragma unroll
            for (int q = 0; q < MAXE; ++q) {
                const int e = l + q * NT;
                if (e < DD) {
                    const int i = e / D, j = e - i * D;
                    a.S[kdd + e] = sreg[q];
                    if (a.R) a.R[kdd + e] = S[i * ld + j];
                }
            }
        } else {                                                        // revert: nothing of the state is written (:124-125)
            if (l == 0 && a.n_rev) a.n_rev[k] += 1;
            for (int i = l; i < D; i += NT) m1[i] = m0[i];              // the next samples come from the kept state
            if (a.R && a.seeds)
#pragma unroll
                for (int q = 0; q < MAXE; ++q) {
                    const int e = l + q * NT;
                    if (e < DD) {
                        const int i = e / D, j = e - i * D;
                        S[i * ld + j] = a.R[kdd + e];
                    }
                }
        }
        if (l == 0 && a.info) a.info[k] = info;
    }
    if (!a.seeds) return;                                               // (uniform: no barrier follows)

    __syncthreads();
    if (valid) {
        const unsigned long long seed = a.seeds[k], call = a.call;
        for (int p = l; p < (B * Dz) / 2; p += NT) {
            unsigned w[4];
            philox4x32_10((unsigned)p, 0u, (unsigned)call, (unsigned)(call >> 32), (unsigned)seed, (unsigned)(seed >> 32), w);
            philox_normal_pair(w, Zb[2 * p], Zb[2 * p + 1]);
        }
    }
    __syncthreads();
    if (valid) {
        for (int e = l; e < BD; e += NT) {
            const int b = e / D, j = e - b * D;
            double s = 0.0;
            for (int i = 0; i <= j; ++i) s += Zb[b * Dz + i] * S[i * ld + j];
            a.Xout[kbd + e] = s + m1[j];
        }
    }
}

// ---- the two sums at the end of a Gaussian draw or evaluation (KL monitor, Pathfinder, ADVI), for one workgroup slot ---------

// The sum of v over the slot: a fixed butterfly in each wave, then the four waves in order through red (LDS, 4).  The result is
// in thread l == 0 (in every thread of a one-wave slot).  Every thread of every slot calls it (one barrier for NT > 64).
template <int NT>
__device__ __forceinline__ double gb_slot_sum(double v, int l, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (NT > 64) {
        if ((l & 63) == 0) red[l >> 6] = v;
        __syncthreads();
        if (l == 0) v = red[0] + red[1] + red[2] + red[3];
    }
    return v;
}

// sum over `rows` rows of log N(x; m, R^T R) from acc = sum |z|^2 of the rows and the pivots pv = diag R; NaN when not `ok`
__device__ __forceinline__ double gb_logq_sum(bool ok, double acc, long long rows, int D, const double* pv) {
    double lg = 0.0;
    for (int i = 0; i < D; ++i) lg += log(pv[i]);
    const double n = (double)rows;
    return ok ? -0.5 * acc - n * lg - 0.5 * n * D * 1.8378770664093454836 : __longlong_as_double(0x7ff8000000000000LL);   // log 2 pi
}

// ---- host side: the argument checks and the launch pieces shared by the batched entry points --------------------------
// Every entry point checks, before anything is enqueued: the shapes (gb_check_shape), its NULL arrays and own conditions
// (GB_BAD), the overlaps (gb_check_overlaps), and the context last.  A failure returns GSMVI_ERR_BAD_ARG.
#define GB_LDS_MAX (160 * 1024)   // dynamic LDS per workgroup that a batched kernel may request (gb_allow_lds)

static inline bool gb_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

static inline int gb_bad(const char* fn, const char* msg) {
    gsmvi_set_error("%s: %s", fn, msg);
    return GSMVI_ERR_BAD_ARG;
}

#define GB_BAD(cond, msg)                           \
    do {                                            \
        if (cond) return gb_bad(__func__, msg);     \
    } while (0)

// problems per 256-thread workgroup of k_gsm_batched and k_kl_batched (B plays no part)
static inline int gb_ppw(int D, int) { return 256 / gb_nt(D); }

// 1 <= D <= 64; 1 <= B <= 32 (an entry point without B leaves the default); K >= 1 and, at ppw(D, B) problems per
// workgroup (asked only for D and B in bounds), fewer than 2^32 threads in one launch: K <= ppw (2^24 - 1)
static inline int gb_check_shape(const char* fn, int64_t K, int D, int (*ppw)(int D, int B), int B = 1) {
    if (D < 1 || D > GB_MAX_D) return gb_bad(fn, "D must be in [1, 64]");
    if (B < 1 || B > GB_MAX_B) return gb_bad(fn, "B must be in [1, 32]");
    if (K < 1 || K > (int64_t)ppw(D, B) * 16777215)
        return gb_bad(fn, "K must be in [1, 2^24 - 1] (one problem per workgroup) or [1, 2^26 - 4] (four)");
    return GSMVI_OK;
}

// one array of an entry point's overlap table: written (GB_WR) if a kernel may store to it, else read-only (GB_RD)
constexpr bool GB_RD = false, GB_WR = true;
struct gb_arr {
    const void* p;
    size_t bytes;
    const char* name;
    bool written;
};

// The overlap rule of every batched entry point: an array that is written must not overlap any other listed array; read-only
// arrays may overlap each other; NULL entries are skipped.  The message names both arrays.
static inline int gb_check_overlaps(const char* fn, const gb_arr* first, const gb_arr* last) {
    for (const gb_arr* a = first; a != last; ++a)
        for (const gb_arr* b = first; b != a; ++b)
            if (a->p && b->p && (a->written || b->written) && gb_overlap(a->p, a->bytes, b->p, b->bytes)) {
                char msg[96];
                snprintf(msg, sizeof msg, "%s overlaps %s", (a->written ? a : b)->name, (a->written ? b : a)->name);
                return gb_bad(fn, msg);
            }
    return GSMVI_OK;
}
static inline int gb_check_overlaps(const char* fn, std::initializer_list<gb_arr> arrs) {
    return gb_check_overlaps(fn, arrs.begin(), arrs.end());
}

// the end of every batched launch: a launch error -> GSMVI_ERR_HIP, else the kernel family's path bit is recorded
static inline int gb_launched(gsmvi_ctx* ctx, unsigned path, const char* kernel) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        gsmvi_set_error("launch of %s failed: %s", kernel, hipGetErrorString(e));
        return GSMVI_ERR_HIP;
    }
    ctx->path |= path;
    return GSMVI_OK;
}

// lets every given kernel request up to GB_LDS_MAX of dynamic LDS (one problem of D = 64, B = 32 takes up to 145 KB)
template <typename... F>
static hipError_t gb_allow_lds(F*... kernels) {
    for (const void* f : {reinterpret_cast<const void*>(kernels)...}) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, GB_LDS_MAX);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
