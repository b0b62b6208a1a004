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
// Stage (b) is ps_stage of gsmvi_psis_stage.h (shared with the leave-one-out kernel, gsmvi_psis_loo_batched.hip): every sum is a
// fixed tree and there are no atomics, so the outputs are bit-identical from run to run.  Every thread runs every barrier
// whatever its problem's verdict (the verdicts only select what is written), and a workgroup reads and writes only its own
// problem's slices.  Inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_psis_stage.h"
#include "../../include/gsmvi_hip.h"
#include <cfloat>
#include <cmath>
#include <cstdint>

enum { PS_WEIGHTS = 0, PS_FUSED = 1 };
#define PS_Q 8          // tile elements per thread: tr = max(1, 256 PS_Q / D) rows, at most S

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
// LDS doubles of the fused entry beside the stage's (ps_lds_doubles): R (D x ld), mean, pivots, first moments (D each), the tile
__host__ __device__ inline int ps_lds_fused(int D, int ld, int ldy, int tr) { return D * ld + 3 * D + tr * ldy; }

template <int MODE>
__global__ __launch_bounds__(256) void k_psis_batched(ps_args a) {
    extern __shared__ double ps_sm[];
    const int l = threadIdx.x, S = a.S, S2 = a.S2, M = a.M;
    const int D = a.D, ld = a.ld, ldy = a.ldy, TR = a.tr, DD = D * D;
    const size_t k = blockIdx.x;              // one problem per workgroup: the grid is K
    double* R = ps_sm + ps_lds_doubles(S, S2);   // FUSED: D x ld
    double* m = R + D * ld;                   // D      mean
    double* pv = m + D;                       // D      pivots R_cc
    double* mom = pv + D;                     // D      sum w d
    double* T = mom + D;                      // TR x ldy  x - mean, then w
    const ps_lds sm = ps_carve(ps_sm, reinterpret_cast<int*>(MODE == PS_FUSED ? T + TR * ldy : R), S, S2);
    double* val = sm.val;                     // S2     the log ratios
    double* lwu = sm.lwu;                     // S      normalised log weights in row order, then the weights
    const size_t ks = k * (size_t)S;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

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

    // ---- (b) the PSIS stage -------------------------------------------------------------------------------------------------
    const ps_verdict v = ps_stage(sm, S, S2, M, l, cinfo != 0);
    const bool bad = v.bad;
    for (int s = l; s < S; s += 256) a.lw[ks + s] = bad ? qnan : lwu[s];
    if (l == 0) {
        a.khat[k] = bad ? qnan : v.khat;
        a.ess[k] = bad ? qnan : v.ess;
        a.log_z[k] = bad ? qnan : v.lse + v.vmax - log((double)S);
        a.info[k] = cinfo != 0 ? cinfo : (bad ? -1 : (v.fit ? 0 : -2));
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
    ps_sizes(S, &a.S2, &a.M);
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
