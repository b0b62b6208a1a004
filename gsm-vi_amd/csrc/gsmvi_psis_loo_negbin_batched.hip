// Batched negative binomial PSIS leave-one-out: for K fitted Gaussians q_k over (beta, theta = log r) of K overdispersed count
// regressions of one (N, P), D = P + 1 <= 64, the pointwise leave-one-out log predictive density of every observation from S draws
// of q_k, one launch ("Batched negative binomial PSIS-LOO"; the definition is in include/gsmvi_hip.h, above
// gsmvi_psis_loo_negbin_batched_f64).  The reference has no twin.
//   k_psis_loo_negbin_batched       (a sibling of k_psis_loo_batched, not one more family of it: a draw is not only coefficients)
// Work mapping: one 256-thread workgroup per (problem k, tile of NI = gsmvi_psis_loo_negbin_tile(P, S) observations).
//   (1) l_si of the tile, per tile of PS_LOO_TR = 64 draws, in three steps between barriers:
//       (a) the tile of X_k into LDS: 64 rows of Pp = 4 ceil(P / 4) columns (row stride Pp + 1).  Only the columns j < P of a draw
//           are copied; column P of the draw (theta) never enters the operand, and every padded position (j >= P, rows past S)
//           holds 0.0.  The NI rows of A_k sit beside it zero-padded to 16 rows of the same Pp columns, loaded once.
//       (b) eta = X_tile A_tile^T on the fp64 MFMA (16 x 16 x 4): wave w takes the 16 draws 16 w .. 16 w + 15 of the tile, the A
//           operand x_{s, 4 j + kq}, the B operand a_{i, 4 j + kq}, Pp / 4 steps; a lane whose column is a valid observation
//           leaves eta_si in the cell of l_si.  Meanwhile thread s < 64 forms the per-draw values of draw s of the tile: theta_s
//           (read from X_k, not from the operand), r_s = e^theta_s and the flag -- from the LOADED values: a non-finite beta_sj
//           (0 x beta_sj summed over the row in LDS) or theta_s, or an r_s that is not a positive normal number (the score
//           kernel's row flag).  Not from the product: there a padded zero of A would meet a non-finite x as 0 x inf = NaN only
//           where x is in the operand, and theta is not.
//       (c) the link, re-mapped so that every lane works: entry e = l, l + 256, ... of the tile's nv x 64 (observation, draw)
//           pairs -- one per thread at NI <= 4 -- reads eta_si + o_i, runs nb_link<false, true> (gsmvi_negbin_link.h, unchanged:
//           t is bit for bit the score launch's at the same eta) and stores l_si = t + c_i, c_i = -lgamma(y_i + 1), or NaN for a
//           flagged draw.  (In the MFMA's own layout only the NI <= 4 of 16 columns would run the link's up to twelve log1p.)
//       y_i, o_i and c_i go into LDS once per workgroup.  The tile's l_si stay in LDS (NI x S doubles).
//   (2) per observation of the tile: ps_loo_stage (gsmvi_psis_stage.h, shared with the two sibling kernels): rho_s = logr_s - l_si
//       into the PSIS stage's array, ps_stage, then the two log-sum-exps.
// The tiles of (1) lie over the stage's LDS (dead before the first stage starts).  NI is the largest count, at most PLN_NI_CAP,
// whose l_si fit beside that region in GB_LDS_MAX.  Every sum is a fixed tree or chain and there are no atomics; every thread of a
// workgroup runs the same barriers whatever the verdicts (the number of valid observations of a tile is uniform in it); a
// workgroup reads only slice k of the inputs and writes only its own (k, i) entries.  Inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_glm_model.h"                 // glm_model's overlap table
#include "gsmvi_negbin_link.h"
#include "gsmvi_psis_stage.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

// observations per workgroup at most (as PL_NI_CAP and PLS_NI_CAP of gsmvi_psis_stage.h); a diagnostic build changes it with
// -DPLN_NI_CAP=n, 1 <= n <= 16
#ifndef PLN_NI_CAP
#define PLN_NI_CAP 4
#endif
static_assert(PLN_NI_CAP >= 1 && PLN_NI_CAP <= PS_LOO_NB, "the tile's observations are columns of one 16-column MFMA block");

struct pln_args {
    long long K, N;
    int P, D;                   // columns of A, P + 1
    int S, S2, M;               // draws, draws padded to a power of two, the tail size before ties
    int NI, U;                  // observations per tile; doubles of the region the stage and the MFMA tiles share
    unsigned ntile;             // tiles per problem: ceil(N / NI)
    const double* A;            // (K, N, P)
    const double* y;            // (K, N)
    const double* offset;       // (K, N) added to eta, or null
    const int* counts;          // (K) valid rows, clamped to 0 .. N (null: N)
    const double* X;            // (K, S, D) the draws of q_k: beta, then theta
    ps_loo_io o;                // the ratios and weights of the problem-level run, the outputs
};

__host__ __device__ inline int pln_pp(int P) { return (P + 3) & ~3; }

// doubles of the kernel's own use of the shared region: the X tile, the A tile, three per-observation and three per-draw arrays
static inline int pln_tiles_doubles(int P) { return (PS_LOO_TR + PS_LOO_NB) * (pln_pp(P) + 1) + 3 * PS_LOO_NB + 3 * PS_LOO_TR; }

static int pln_tile(int P, int S) { return ps_loo_tile(pln_tiles_doubles(P), S, PLN_NI_CAP); }

__global__ __launch_bounds__(256) void k_psis_loo_negbin_batched(pln_args a) {
    extern __shared__ double pln_sm[];
    const int l = threadIdx.x, S = a.S, S2 = a.S2, M = a.M, NI = a.NI;
    const int P = a.P, D = a.D, Pp = pln_pp(P), lda = Pp + 1;
    const long long N = a.N;
    const size_t k = blockIdx.x / a.ntile;
    const long long i0 = (long long)(blockIdx.x - (unsigned)k * a.ntile) * NI;       // the tile's first observation
    const int ni = (int)(N - i0 < NI ? N - i0 : NI);
    long long nk = N;
    if (a.counts) {
        const long long c = a.counts[k];
        nk = c < 0 ? 0 : (c > N ? N : c);
    }
    const int nv = (int)(nk - i0 < 0 ? 0 : (nk - i0 < ni ? nk - i0 : ni));            // its valid observations: the first nv
    const ps_lds sm = ps_carve(pln_sm, reinterpret_cast<int*>(pln_sm + ps_lds_doubles(S, S2)), S, S2);
    double* Xs = pln_sm;                      // 64 x lda      the beta part of a tile of draws   (over the stage's arrays)
    double* As = Xs + PS_LOO_TR * lda;        // 16 x lda      the tile's rows of A_k, zero-padded
    double* ys = As + PS_LOO_NB * lda;        // 16 each: y_i, offset_i, -lgamma(y_i + 1)
    double* os = ys + PS_LOO_NB;
    double* cs = os + PS_LOO_NB;
    double* ths = cs + PS_LOO_NB;             // 64 each: theta_s, r_s = e^theta_s, 1.0 or 0.0 (a flagged draw) of the tile's draws
    double* rs = ths + PS_LOO_TR;
    double* fs = rs + PS_LOO_TR;
    double* ell = pln_sm + a.U;               // NI x S        l_si of the tile
    const size_t ks = k * (size_t)S, kn = k * (size_t)N + (size_t)i0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    // ---- (1) l_si of the tile's valid observations ------------------------------------------------------------------------
    if (nv > 0) {                             // (uniform in the workgroup)
        const double* Ak = a.A + kn * P;
        for (int e = l; e < PS_LOO_NB * lda; e += 256) {
            const int r = e / lda, j = e - r * lda;
            As[e] = r < nv && j < P ? Ak[(size_t)r * P + j] : 0.0;
        }
        if (l < PS_LOO_NB) {
            const double yv = l < nv ? a.y[kn + l] : 0.0;
            ys[l] = yv;
            os[l] = a.offset && l < nv ? a.offset[kn + l] : 0.0;
            cs[l] = -lgamma(yv + 1.0);
        }
        const double* Xk = a.X + ks * D;
        const int wv = l >> 6, ln = l & 63, cc = ln & 15, kq = ln >> 4;
        for (int t0 = 0; t0 < S; t0 += PS_LOO_TR) {
            __syncthreads();                  // the previous tile's readers are done
            for (int e = l; e < PS_LOO_TR * lda; e += 256) {                       // (a)
                const int r = e / lda, j = e - r * lda;
                Xs[e] = t0 + r < S && j < P ? Xk[(size_t)(t0 + r) * D + j] : 0.0;
            }
            const double th = l < PS_LOO_TR && t0 + l < S ? Xk[(size_t)(t0 + l) * D + P] : 0.0;
            __syncthreads();
            if (l < PS_LOO_TR) {                                                   // (b) the per-draw values ...
                const double* xr = Xs + l * lda;
                double z = 0.0;
                for (int j = 0; j < P; ++j) z += xr[j] * 0.0;                      // (NaN for a non-finite beta_sj)
                const double r = exp(th);                                          // (a NaN theta gives a NaN r: flagged)
                ths[l] = th;
                rs[l] = r;
                fs[l] = r >= 2.2250738585072014e-308 && r < __builtin_huge_val() && z == 0.0 ? 1.0 : 0.0;
            }
            if (t0 + 16 * wv < S) {           // ... and eta (wave-uniform)
                const double* pa = Xs + (16 * wv + cc) * lda + kq;
                const double* pb = As + cc * lda + kq;
                v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
                for (int j = 0; j < Pp; j += 4) acc = GSMVI_MFMA_F64(pa[j], pb[j], acc);
                if (cc < nv) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int s = t0 + 16 * wv + kq + 4 * r;    // the draw; cc is the observation
                        if (s < S) ell[cc * S + s] = acc[r];
                    }
                }
            }
            __syncthreads();
            for (int e = l; e < nv * PS_LOO_TR; e += 256) {                        // (c)
                const int i = e >> 6, q = e & 63, s = t0 + q;
                if (s < S) {
                    double re = 0.0, rt = 0.0, t = 0.0;
                    nb_link<false, true>(ell[i * S + s] + os[i], ths[q], rs[q], ys[i], re, rt, t);
                    ell[i * S + s] = fs[q] != 0.0 ? t + cs[i] : qnan;
                }
            }
        }
    }
    __syncthreads();                          // l_si is published; the tiles are dead, the stage may take their place

    ps_loo_stage(a.o, sm, ell, ni, nv, nullptr, ks, kn, S, S2, M, l);     // (2)
}

hipError_t gsmvi_psis_loo_negbin_batched_prepare() { return gb_allow_lds(k_psis_loo_negbin_batched); }

extern "C" {

int gsmvi_psis_loo_negbin_tile(int P, int64_t S) {
    if (P < 1 || P > GB_MAX_D - 1 || S < PS_MIN_S || S > PS_MAX_S) return 0;
    return pln_tile(P, (int)S);
}

int gsmvi_psis_loo_negbin_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int64_t N, int64_t S, const double* A,
                                      const double* y, const double* offset, const int* counts_dev, const double* X,
                                      const double* logr, const double* lw, double* loglik, double* elpd, double* lpd,
                                      double* khat, double* ess, int* info) {
    GB_BAD(P < 1 || P > GB_MAX_D - 1, "P must be in [1, 63] (D = P + 1 <= 64)");
    const int D = P + 1;
    GB_BAD(K < 1 || K > 16777215, "K must be in [1, 2^24 - 1]");
    GB_BAD(N < 1, "N must be at least 1");
    GB_BAD(S < PS_MIN_S || S > PS_MAX_S, "S must be in [5, 4096]");
    GB_BAD(!A || !y || !X || !logr || !lw || !elpd || !lpd || !khat || !ess || !info, "NULL array");
    GB_BAD(N > (INT64_MAX / 8 / S) / K, "K N S is too large");
    GB_BAD(N > (INT64_MAX / 8 / P) / K, "K N P is too large");
    const int NI = pln_tile(P, (int)S);
    const int64_t ntile = (N + NI - 1) / NI;
    GB_BAD(ntile > 16777215 / K,
           "K ceil(N / gsmvi_psis_loo_negbin_tile(P, S)) must be at most 2^24 - 1 (one tile per workgroup)");
    const glm_model m = {K, N, P, A, y, offset, counts_dev, 0.0, nullptr, 1.0, nullptr};
    const size_t nn = (size_t)K * N * 8, ns = (size_t)K * S * 8;
    if (int st = gb_check_overlaps(__func__, m, {{X, ns * D, "X", GB_RD}, {logr, ns, "logr", GB_RD}, {lw, ns, "lw", GB_RD},
                                                 {loglik, nn * S, "loglik", GB_WR}, {elpd, nn, "elpd", GB_WR}, {lpd, nn, "lpd", GB_WR},
                                                 {khat, nn, "khat", GB_WR}, {ess, nn, "ess", GB_WR},
                                                 {info, (size_t)K * N * 4, "info", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    pln_args a = {};
    a.K = K; a.N = N; a.P = P; a.D = D;
    a.S = (int)S;
    ps_sizes(a.S, &a.S2, &a.M);
    a.NI = NI;
    a.U = ps_loo_region_doubles(pln_tiles_doubles(P), a.S, a.S2);
    a.ntile = (unsigned)ntile;
    a.A = A; a.y = y; a.offset = offset; a.counts = counts_dev;
    a.X = X;
    a.o = {logr, lw, loglik, elpd, lpd, khat, ess, info};
    const size_t lds = ((size_t)a.U + (size_t)NI * a.S) * sizeof(double);      // <= GB_LDS_MAX by the choice of NI
    const unsigned grid = (unsigned)(K * ntile);
    hipLaunchKernelGGL(k_psis_loo_negbin_batched, dim3(grid), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_TARGET, "k_psis_loo_negbin_batched");
}

}  // extern "C"
