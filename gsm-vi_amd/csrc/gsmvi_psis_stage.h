// The PSIS stage of the batched diagnostics: steps 1-8 of the definition in include/gsmvi_hip.h (gsmvi_psis_weights_batched_f64)
// on the S log ratios that one 256-thread workgroup holds in LDS.  One copy, called by k_psis_batched<PS_WEIGHTS>,
// k_psis_batched<PS_FUSED> (gsmvi_psis_batched.hip: once per problem) and, once per observation, by ps_loo_stage of
// gsmvi_psis_loo_tile.h, the observation stage of the leave-one-out kernels; DESIGN.md section 9.
// In LDS: the S ratios padded with +inf to S2 = the next power of two, their S2 indices, the S normalised weights in row order,
// the tail (at most 192 exceedances) and the 43 candidates of its fit.  Two reductions (non-finite count, maximum); a bitonic
// network on (value, index) pairs, ascending by value then by index -- numpy's stable argsort, so ties fall the same way on
// every run; the tail lies at the end of the sorted array, the fit runs on it with four lanes per candidate (each sums every
// fourth exceedance in order; the four partial sums are added in order), the smoothed values overwrite it in place; truncation,
// log-sum-exp and the effective sample size are sums over the sorted array; the weights return to row order through the
// indices.  Every sum is a fixed tree -- a thread's own entries in order, a butterfly within each wave, then the four waves in
// order -- and there are no atomics.  Every thread runs every barrier whatever the verdict: the verdict only selects what the
// caller writes.
#pragma once
#include <hip/hip_runtime.h>
#include "gsmvi_batched.h"   // GB_LDS_MAX
#include <cfloat>
#include <cmath>

#define PS_MIN_S 5
#define PS_MAX_S 4096
#define PS_MAX_M 192    // the longest tail: ceil(3 sqrt(4096))
#define PS_MAX_J 44     // candidates of the tail fit: 30 + floor(sqrt(n)) <= 43

// LDS doubles of the PSIS stage: sorted values (S2), weights in row order (S), the tail, b_j, L_j, omega_j, 4 partial sums per
// candidate, 8 for the reductions.  The S2 indices (ints) are the caller's to place.
__host__ __device__ inline int ps_lds_doubles(int S, int S2) { return S2 + S + PS_MAX_M + 7 * PS_MAX_J + 8; }
// S2: S rounded up to a power of two, at least 8;  M = ceil(min(S / 5, 3 sqrt(S))): the tail's size before ties are taken out
static inline void ps_sizes(int S, int* S2, int* M) {
    int s2 = 8;
    while (s2 < S) s2 <<= 1;
    const int m5 = (S + 4) / 5, m3 = (int)ceil(3.0 * sqrt((double)S));
    *S2 = s2;
    *M = m5 < m3 ? m5 : m3;
}

struct ps_lds {
    double* val;    // S2     log ratios, shifted, sorted, smoothed, truncated
    double* lwu;    // S      normalised log weights in row order
    double* xs;     // 192    the tail's exceedances, ascending
    double* bs;     // 44     b_j
    double* Ls;     // 44     L_j
    double* ws;     // 44     omega_j
    double* part;   // 4 x 44 partial sums of kappa_j
    double* red;    // 8      per-wave partial results
    int* idx;       // S2     row numbers
};

// the arrays of the stage in ps_lds_doubles(S, S2) doubles at sm; idx wherever the caller keeps S2 ints
__device__ __forceinline__ ps_lds ps_carve(double* sm, int* idx, int S, int S2) {
    ps_lds p;
    p.val = sm;
    p.lwu = p.val + S2;
    p.xs = p.lwu + S;
    p.bs = p.xs + PS_MAX_M;
    p.Ls = p.bs + PS_MAX_J;
    p.ws = p.Ls + PS_MAX_J;
    p.part = p.ws + PS_MAX_J;
    p.red = p.part + 4 * PS_MAX_J;
    p.idx = idx;
    return p;
}

// what the stage leaves in registers, the same in every thread: khat (+inf without a fit), the effective sample size, the
// log-sum-exp of the truncated shifted ratios, their shift max(logr), `bad` (step 1 refuses the ratios: info = -1) and `fit`
// (false: info = -2)
struct ps_verdict {
    double khat, ess, lse, vmax;
    bool bad, fit;
};

// the block's sum, to every thread: a butterfly within each wave, then the four waves in order
__device__ __forceinline__ double ps_sum(double v, double* red, int l) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                    // the readers of the previous reduction are done
    if ((l & 63) == 0) red[l >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ double ps_max(double v, double* red, int l) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((l & 63) == 0) red[l >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// Steps 1-8 on the ratios p.val[0 .. S) (written and published by a barrier before the call).  On return p.lwu[0 .. S) holds the
// normalised smoothed log weights in row order, published to every thread (whatever the verdict: with `bad` they are not to be
// used).  `refused`: the caller's own reason to refuse the problem (the fused entry's pivot code), folded into `bad`.
__device__ __forceinline__ ps_verdict ps_stage(const ps_lds p, int S, int S2, int M, int l, bool refused) {
    double* val = p.val;
    double* lwu = p.lwu;
    double* xs = p.xs;
    double* bs = p.bs;
    double* Ls = p.Ls;
    double* ws = p.ws;
    double* part = p.part;
    double* red = p.red;
    int* idx = p.idx;
    const double inf = __builtin_huge_val();

    // ---- 1-2: non-finite input, the shift --------------------------------------------------------------------------------
    double nb = 0.0, vmax = -inf;
    for (int s = l; s < S; s += 256) {
        const double v = val[s];
        if (!(v < inf)) nb += 1.0;            // NaN or +inf
        vmax = fmax(vmax, v);
    }
    nb = ps_sum(nb, red, l);
    vmax = ps_max(vmax, red, l);
    const bool bad = refused || nb > 0.0 || vmax == -inf;
    for (int q = l; q < S2; q += 256) {       // (each thread rewrites the entries it read)
        val[q] = q < S ? val[q] - vmax : inf;
        idx[q] = q;
    }
    __syncthreads();

    // ---- 3: ascending by (value, index): a bitonic network on the S2 pairs, one barrier per stage ---------------------------
    for (int kk = 2; kk <= S2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = l; t < (S2 >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), q = i | j;
                const double va = val[i], vb = val[q];
                const int ia = idx[i], ib = idx[q];
                const bool after = va > vb || (va == vb && ia > ib);
                if (after == ((i & kk) == 0)) {
                    val[i] = vb; val[q] = va;
                    idx[i] = ib; idx[q] = ia;
                }
            }
            __syncthreads();
        }
    const double LOG_DBL_MIN = -708.39641853226410622;
    double cut = val[S - M - 1];
    cut = cut > LOG_DBL_MIN ? cut : LOG_DBL_MIN;
    const double ec = exp(cut);
    const int n = (int)ps_sum(l < M && val[S - M + l] > cut ? 1.0 : 0.0, red, l);   // the tail: the last n sorted entries
    if (l < n) xs[l] = exp(val[S - n + l]) - ec;
    __syncthreads();

    // ---- 4-5: the tail fit (n > 4) -----------------------------------------------------------------------------------------
    const bool fit = n > 4;
    const int mj = 30 + (int)sqrt((double)n);
    const double dn = (double)n;
    {
        const int jj = l >> 2, q = l & 3;
        if (fit && jj < mj) {
            const double b = (1.0 - sqrt((double)mj / ((double)(jj + 1) - 0.5))) / (3.0 * xs[(n + 2) / 4 - 1]) + 1.0 / xs[n - 1];
            double s = 0.0;
            for (int i = q; i < n; i += 4) s += log1p(-b * xs[i]);
            part[l] = s;
            if (q == 0) bs[jj] = b;
        }
    }
    __syncthreads();
    if (fit && l < mj) {
        const double kap = (((part[4 * l] + part[4 * l + 1]) + part[4 * l + 2]) + part[4 * l + 3]) / dn;
        Ls[l] = dn * (log(-bs[l] / kap) - kap - 1.0);
    }
    __syncthreads();
    if (fit && l < mj) {
        double s = 0.0;
        for (int i = 0; i < mj; ++i) s += exp(Ls[i] - Ls[l]);
        const double om = 1.0 / s;
        ws[l] = om < 10.0 * DBL_EPSILON ? 0.0 : om;
    }
    __syncthreads();
    double bb = 0.0, kh = inf, sigma = 0.0;
    if (fit) {                                // (every thread, the same order)
        double sw = 0.0;
        for (int j = 0; j < mj; ++j) sw += ws[j];
        for (int j = 0; j < mj; ++j) bb += (ws[j] / sw) * bs[j];
    }
    const double kap = ps_sum(fit && l < n ? log1p(-bb * xs[l]) : 0.0, red, l) / dn;
    if (fit) {
        sigma = -kap / bb;
        kh = (dn * kap + 5.0) / (dn + 10.0);
    }

    // ---- 6: the smoothed tail ------------------------------------------------------------------------------------------------
    if (fit && kh - kh == 0.0 && l < n) {     // (khat finite)
        const double lq = log1p(-((double)l + 0.5) / dn);
        const double q = kh == 0.0 ? -sigma * lq : sigma * expm1(-kh * lq) / kh;
        val[S - n + l] = log(q + ec);
    }
    __syncthreads();

    // ---- 7-8: truncate, normalise, summarise --------------------------------------------------------------------------------
    double s1 = 0.0;
    for (int q = l; q < S; q += 256) {
        double v = val[q];
        v = v > 0.0 ? 0.0 : v;
        val[q] = v;
        s1 += exp(v);
    }
    const double lse = log(ps_sum(s1, red, l));
    double s2 = 0.0;
    for (int q = l; q < S; q += 256) {
        const double v = val[q] - lse;
        const int s = idx[q];
        if (s < S) lwu[s] = v;                // (always, unless the ratios held a NaN: then nothing of lwu is used)
        s2 += exp(2.0 * v);
    }
    const double ess = 1.0 / ps_sum(s2, red, l);   // (its barriers also publish lwu)
    return ps_verdict{kh, ess, lse, vmax, bad, fit};
}
