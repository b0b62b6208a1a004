// Batched Pareto-smoothed importance diagnostic: is the Gaussian q_k = N(mean_k, cov_k) of K problems of one D, D <= 64, a usable
// importance proposal for its target?  One launch after the target's lp (the definition of every step is
// in include/gsmvi_hip.h: Vehtari, Simpson, Gelman, Yao, Gabry, JMLR 2024, with the tail fit of Zhang & Stephens 2009).
//   k_psis_batched<PS_FUSED>   : (a) R_k = chol(cov_k) (upper) in LDS; for the rows x_s of X_k: w = the solution of
//                                R_k^T w = x_s - mean_k (forward substitution over tiles of rows, as k_kl_batched<., KB_EVAL>),
//                                logq_s = -|w|^2 / 2 - sum_i log R_ii - D / 2 log 2 pi, logr_s = lp_s - logq_s -> LDS and out;
//                                (b) the PSIS stage on the S ratios; (c) with mean_is: a second walk over X_k for the
//                                importance-weighted mean and covariance
//   k_psis_batched<PS_WEIGHTS> : stage (b) alone on the caller's ratios
// Work mapping: one problem per 256-thread workgroup at every D -- the sort wants the whole workgroup.  In LDS: the S ratios
// padded with +inf to S2 = the next power of two, their S2 indices, the S normalised weights in row order, the tail (at most
// 192 exceedances) and the 43 candidates of its fit, and for the fused entry R (D x ld), mean, pivots and a tile of rows
// (tr x ldy, odd strides D | 1): at most 134 KB (D = 64, S = 4096), inside GB_LDS_MAX.
// Stage (b): two reductions (non-finite count, maximum); a bitonic network on (value, index) pairs, ascending by value then by
// index -- numpy's stable argsort, so ties fall the same way on every run; the tail lies at the end of the sorted array, the
// fit runs on it with four lanes per candidate (each sums every fourth exceedance in order; the four partial sums are added in
// order), the smoothed values overwrite it in place; truncation, log-sum-exp and the effective sample size are sums over the
// sorted array; the weights return to row order through the indices.  Every sum is a fixed tree -- a thread's own entries
// in order, a butterfly within each wave, then the four waves in order -- and there are no atomics: the outputs are
// bit-identical from run to run.  Every thread runs every barrier whatever its problem's verdict (the verdicts only select what
// is written), and a workgroup reads and writes only its own problem's slices.  Inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "../../include/gsmvi_hip.h"
#include <cfloat>
#include <cmath>
#include <cstdint>

enum { PS_WEIGHTS = 0, PS_FUSED = 1 };
#define PS_Q 8          // tile elements per thread: tr = max(1, 256 PS_Q / D) rows, at most S
#define PS_MIN_S 5
#define PS_MAX_S 4096
#define PS_MAX_M 192    // the longest tail: ceil(3 sqrt(4096))
#define PS_MAX_J 44     // candidates of the tail fit: 30 + floor(sqrt(n)) <= 43

struct ps_args {
    long long K;
    int S, S2, M;                       // rows, rows padded to a power of two, tail size ceil(min(S / 5, 3 sqrt(S)))
    int D, ld, ldy, tr;                 // FUSED: dimension, row strides of R and of the tile, rows per tile
    const double* mean;                 // FUSED: (K, D)
    const double* cov;                  // FUSED: (K, D, D)
    const double* X;                    // FUSED: (K, S, D) the draws of q_k
    const double* lp;                   // FUSED: (K, S) the target's values at them
    const double* logr_in;              // WEIGHTS: (K, S) the caller's log ratios
    double* logr;                       // FUSED: (K, S) lp - log q out
    double* lw;                         // (K, S) normalised smoothed log weights
    double* khat;                       // (K) each
    double* ess;
    double* log_z;
    double* mean_is;                    // FUSED: (K, D) or null
    double* cov_is;                     // FUSED: (K, D, D) or null
    int* info;                          // (K) 0; -1 non-finite ratios; -2 tail too short; FUSED: 1 + the first bad pivot
};

__host__ __device__ inline int ps_tile_rows(int D, int S) {
    const int t = (256 * PS_Q) / D;
    return t < S ? t : S;
}
// LDS doubles of the PSIS stage: sorted values (S2), weights in row order (S), the tail, b_j, L_j, omega_j, 4 partial sums per
// candidate, 8 for the reductions; of the fused entry also R (D x ld), mean, pivots, first moments (D each), the tile
__host__ __device__ inline int ps_lds_doubles(int S, int S2) { return S2 + S + PS_MAX_M + 7 * PS_MAX_J + 8; }
__host__ __device__ inline int ps_lds_fused(int D, int ld, int ldy, int tr) { return D * ld + 3 * D + tr * ldy; }

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

template <int MODE>
__global__ __launch_bounds__(256) void k_psis_batched(ps_args a) {
    extern __shared__ double ps_sm[];
    const int l = threadIdx.x, S = a.S, S2 = a.S2, M = a.M;
    const int D = a.D, ld = a.ld, ldy = a.ldy, TR = a.tr, DD = D * D;
    const size_t k = blockIdx.x;              // one problem per workgroup: the grid is K
    double* val = ps_sm;                      // S2     log ratios, shifted, sorted, smoothed, truncated
    double* lwu = val + S2;                   // S      normalised log weights in row order, then the weights
    double* xs = lwu + S;                     // 192    the tail's exceedances, ascending
    double* bs = xs + PS_MAX_M;               // 44     b_j
    double* Ls = bs + PS_MAX_J;               // 44     L_j
    double* ws = Ls + PS_MAX_J;               // 44     omega_j
    double* part = ws + PS_MAX_J;             // 4 x 44 partial sums of kappa_j
    double* red = part + 4 * PS_MAX_J;        // 8      per-wave partial results
    double* R = red + 8;                      // FUSED: D x ld
    double* m = R + D * ld;                   // D      mean
    double* pv = m + D;                       // D      pivots R_cc
    double* mom = pv + D;                     // D      sum w d
    double* T = mom + D;                      // TR x ldy  x - mean, then w
    int* idx = reinterpret_cast<int*>(MODE == PS_FUSED ? T + TR * ldy : R);   // S2 row numbers
    const size_t ks = k * (size_t)S;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL), inf = __builtin_huge_val();

    // ---- (a) the log ratios ----------------------------------------------------------------------------------------------
    int cinfo = 0;
    if (MODE == PS_FUSED) {
        const size_t kd = k * D, kdd = k * DD, krow = ks * D;
        for (int i = l; i < D; i += 256) m[i] = a.mean[kd + i];
        for (int e = l; e < DD; e += 256) {
            const int i = e / D, j = e - i * D;
            R[i * ld + j] = a.cov[kdd + e];
        }
        __syncthreads();
        cinfo = gb_chol_lds<256, (GB_MAX_D * GB_MAX_D) / 256>(true, D, l, ld, R, pv);
        __syncthreads();
        double lg = 0.0;                      // sum log R_ii, by every thread in the same order
        for (int i = 0; i < D; ++i) lg += log(pv[i]);
        const double cst = lg + 0.5 * D * 1.8378770664093454836;   // log 2 pi
        for (int t0 = 0; t0 < S; t0 += TR) {
            const int tr = S - t0 < TR ? S - t0 : TR, te = tr * D;
            for (int e = l; e < te; e += 256) {
                const int r = e / D, j = e - r * D;
                T[r * ldy + j] = a.X[krow + (size_t)(t0 + r) * D + j] - m[j];
            }
            __syncthreads();
            // R^T w = x - mean by rows, right-looking, one pivot per barrier (k_kl_batched<., KB_EVAL>)
            for (int c = 0; c < D; ++c) {
                const double inv = 1.0 / pv[c];
                for (int e = l; e < te; e += 256) {
                    const int r = e / D, j = e - r * D;
                    if (j > c) T[r * ldy + j] -= (T[r * ldy + c] * inv) * R[c * ld + j];
                }
                __syncthreads();
            }
            for (int r = l; r < tr; r += 256) {   // one thread per row: |w|^2 in column order
                double s = 0.0;
                for (int j = 0; j < D; ++j) {
                    const double w = T[r * ldy + j] * (1.0 / pv[j]);
                    s += w * w;
                }
                const double lr = a.lp[ks + t0 + r] - (-0.5 * s - cst);
                val[t0 + r] = lr;
                a.logr[ks + t0 + r] = cinfo == 0 ? lr : qnan;
            }
            __syncthreads();                  // the next tile overwrites T
        }
    } else {
        for (int s = l; s < S; s += 256) val[s] = a.logr_in[ks + s];
        __syncthreads();
    }

    // ---- (b) 1-2: non-finite input, the shift ----------------------------------------------------------------------------
    double nb = 0.0, vmax = -inf;
    for (int s = l; s < S; s += 256) {
        const double v = val[s];
        if (!(v < inf)) nb += 1.0;            // NaN or +inf
        vmax = fmax(vmax, v);
    }
    nb = ps_sum(nb, red, l);
    vmax = ps_max(vmax, red, l);
    const bool bad = cinfo != 0 || nb > 0.0 || vmax == -inf;
    for (int p = l; p < S2; p += 256) {       // (each thread rewrites the entries it read)
        val[p] = p < S ? val[p] - vmax : inf;
        idx[p] = p;
    }
    __syncthreads();

    // ---- 3: ascending by (value, index): a bitonic network on the S2 pairs, one barrier per stage ---------------------------
    for (int kk = 2; kk <= S2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = l; t < (S2 >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const double va = val[i], vb = val[p];
                const int ia = idx[i], ib = idx[p];
                const bool after = va > vb || (va == vb && ia > ib);
                if (after == ((i & kk) == 0)) {
                    val[i] = vb; val[p] = va;
                    idx[i] = ib; idx[p] = ia;
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
    for (int p = l; p < S; p += 256) {
        double v = val[p];
        v = v > 0.0 ? 0.0 : v;
        val[p] = v;
        s1 += exp(v);
    }
    const double lse = log(ps_sum(s1, red, l));
    double s2 = 0.0;
    for (int p = l; p < S; p += 256) {
        const double v = val[p] - lse;
        const int s = idx[p];
        if (s < S) lwu[s] = v;                // (always, unless the ratios held a NaN: then nothing of lwu is used)
        s2 += exp(2.0 * v);
    }
    const double ess = 1.0 / ps_sum(s2, red, l);   // (its barriers also publish lwu)
    for (int s = l; s < S; s += 256) a.lw[ks + s] = bad ? qnan : lwu[s];
    if (l == 0) {
        a.khat[k] = bad ? qnan : kh;
        a.ess[k] = bad ? qnan : ess;
        a.log_z[k] = bad ? qnan : lse + vmax - log((double)S);
        a.info[k] = cinfo != 0 ? cinfo : (bad ? -1 : (fit ? 0 : -2));
    }

    // ---- (c) the importance-weighted moments: a second walk over X ------------------------------------------------------------
    if (MODE == PS_FUSED) {
        if (!a.mean_is) return;               // (uniform: no barrier follows)
        const size_t kd = k * D, kdd = k * DD, krow = ks * D;
        __syncthreads();
        for (int s = l; s < S; s += 256) lwu[s] = exp(lwu[s]);
        // D <= 16: one entry (i, j >= i) per thread; above: a 4 x 4 block of entries per thread, the blocks on and above the diagonal
        const bool small = D <= 16;
        const int i0 = small ? l / D : 4 * (l >> 4), j0 = small ? l - i0 * D : 4 * (l & 15);
        const bool act = i0 < D && j0 < D && (small ? j0 >= i0 : (l & 15) >= (l >> 4));
        double acc[4][4] = {}, macc = 0.0;
        for (int t0 = 0; t0 < S; t0 += TR) {
            const int tr = S - t0 < TR ? S - t0 : TR, te = tr * D;
            __syncthreads();                  // the previous tile's readers are done (the first: the weights are in place)
            for (int e = l; e < te; e += 256) {
                const int r = e / D, j = e - r * D;
                T[r * ldy + j] = a.X[krow + (size_t)(t0 + r) * D + j] - m[j];
            }
            __syncthreads();
            if (l < D)
                for (int r = 0; r < tr; ++r) macc += lwu[t0 + r] * T[r * ldy + l];
            if (act) {
                if (small) {
                    for (int r = 0; r < tr; ++r) acc[0][0] += (lwu[t0 + r] * T[r * ldy + i0]) * T[r * ldy + j0];
                } else {
                    for (int r = 0; r < tr; ++r) {
                        const double w = lwu[t0 + r];
                        double di[4], dj[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            di[q] = i0 + q < D ? w * T[r * ldy + i0 + q] : 0.0;
                            dj[q] = j0 + q < D ? T[r * ldy + j0 + q] : 0.0;
                        }
#pragma unroll
                        for (int p = 0; p < 4; ++p)
#pragma unroll
                            for (int q = 0; q < 4; ++q) acc[p][q] += di[p] * dj[q];
                    }
                }
            }
        }
        if (l < D) mom[l] = macc;
        __syncthreads();
        if (l < D) a.mean_is[kd + l] = bad ? qnan : m[l] + mom[l];
        if (act) {
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) {     // (unrolled: acc stays in registers)
                    const int i = i0 + p, j = j0 + q;
                    if ((!small || p + q == 0) && i < D && j < D && j >= i) {
                        const double v = bad ? qnan : acc[p][q] - mom[i] * mom[j];
                        a.cov_is[kdd + (size_t)i * D + j] = v;
                        a.cov_is[kdd + (size_t)j * D + i] = v;
                    }
                }
        }
    }
}

hipError_t gsmvi_psis_batched_prepare() { return gb_allow_lds(k_psis_batched<PS_WEIGHTS>, k_psis_batched<PS_FUSED>); }

static int ps_ppw(int, int) { return 1; }     // one problem per workgroup at every D

static int ps_launch(gsmvi_ctx* ctx, void* stream, int mode, ps_args& a, const char* fn) {
    const int S = a.S;
    a.S2 = 8;
    while (a.S2 < S) a.S2 <<= 1;
    const int m5 = (S + 4) / 5, m3 = (int)ceil(3.0 * sqrt((double)S));
    a.M = m5 < m3 ? m5 : m3;
    size_t lds = (size_t)ps_lds_doubles(S, a.S2) * sizeof(double) + (size_t)a.S2 * sizeof(int);
    if (mode == PS_FUSED) {
        a.ld = a.D | 1;
        a.ldy = a.D | 1;
        a.tr = ps_tile_rows(a.D, S);
        lds += (size_t)ps_lds_fused(a.D, a.ld, a.ldy, a.tr) * sizeof(double);   // in all <= 134 KB (D = 64, S = 4096)
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (mode == PS_FUSED)
        hipLaunchKernelGGL((k_psis_batched<PS_FUSED>), dim3((unsigned)a.K), dim3(256), lds, st, a);
    else
        hipLaunchKernelGGL((k_psis_batched<PS_WEIGHTS>), dim3((unsigned)a.K), dim3(256), lds, st, a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_PSIS, fn);
}

extern "C" {

int gsmvi_psis_weights_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int64_t S, const double* logr, double* lw,
                                   double* khat, double* ess, double* log_z, int* info) {
    if (int st = gb_check_shape(__func__, K, 1, ps_ppw)) return st;
    GB_BAD(S < PS_MIN_S || S > PS_MAX_S, "S must be in [5, 4096]");
    GB_BAD(!logr || !lw || !khat || !ess || !log_z || !info, "NULL array");
    const size_t ns = (size_t)K * S * 8, nk = (size_t)K * 8, ni = (size_t)K * 4;
    if (int st = gb_check_overlaps(__func__, {{logr, ns, "logr", GB_RD}, {lw, ns, "lw", GB_WR}, {khat, nk, "khat", GB_WR},
                                              {ess, nk, "ess", GB_WR}, {log_z, nk, "log_z", GB_WR}, {info, ni, "info", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    ps_args a = {};
    a.K = K; a.S = (int)S; a.logr_in = logr; a.lw = lw; a.khat = khat; a.ess = ess; a.log_z = log_z; a.info = info;
    return ps_launch(ctx, stream, PS_WEIGHTS, a, "k_psis_batched (weights)");
}

int gsmvi_psis_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t S, const double* mean, const double* cov,
                           const double* X, const double* lp, double* logr, double* lw, double* khat, double* ess,
                           double* log_z, double* mean_is, double* cov_is, int* info) {
    if (int st = gb_check_shape(__func__, K, D, ps_ppw)) return st;
    GB_BAD(S < PS_MIN_S || S > PS_MAX_S, "S must be in [5, 4096]");
    GB_BAD(!mean || !cov || !X || !lp || !logr || !lw || !khat || !ess || !log_z || !info, "NULL array");
    GB_BAD((mean_is == nullptr) != (cov_is == nullptr), "mean_is and cov_is must be given both or neither");
    const size_t nv = (size_t)K * D * 8, nm = (size_t)K * D * D * 8, nx = (size_t)K * S * D * 8, ns = (size_t)K * S * 8,
                 nk = (size_t)K * 8, ni = (size_t)K * 4;
    if (int st = gb_check_overlaps(__func__, {{mean, nv, "mean", GB_RD}, {cov, nm, "cov", GB_RD}, {X, nx, "X", GB_RD},
                                              {lp, ns, "lp", GB_RD}, {logr, ns, "logr", GB_WR}, {lw, ns, "lw", GB_WR},
                                              {khat, nk, "khat", GB_WR}, {ess, nk, "ess", GB_WR}, {log_z, nk, "log_z", GB_WR},
                                              {mean_is, nv, "mean_is", GB_WR}, {cov_is, nm, "cov_is", GB_WR},
                                              {info, ni, "info", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    ps_args a = {};
    a.K = K; a.D = D; a.S = (int)S; a.mean = mean; a.cov = cov; a.X = X; a.lp = lp; a.logr = logr; a.lw = lw; a.khat = khat;
    a.ess = ess; a.log_z = log_z; a.mean_is = mean_is; a.cov_is = cov_is; a.info = info;
    return ps_launch(ctx, stream, PS_FUSED, a, "k_psis_batched (fused)");
}

}  // extern "C"
