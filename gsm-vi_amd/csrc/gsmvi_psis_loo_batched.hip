// Batched PSIS leave-one-out: for K fitted Gaussians q_k over the coefficients of K GLMs of one (N, D), D <= 64, the pointwise
// leave-one-out log predictive density of every observation from S draws of q_k, one launch ("Batched
// PSIS-LOO"; the definition is in include/gsmvi_hip.h: Vehtari, Gelman, Gabry 2017 with the correction for draws of an
// approximation, Magnusson, Andersen, Jonasson, Vehtari 2019).  The reference has no twin.
//   k_psis_loo_batched<FAM>
// Work mapping: one 256-thread workgroup per (problem k, tile of NI = gsmvi_psis_loo_tile(D, S) observations).
//   (1) eta = X_k A_tile^T (S x NI) on the fp64 MFMA (16 x 16 x 4): the NI rows of A_k sit in LDS zero-padded to 16 rows of
//       Dp = glm_dp(D) columns (row stride Dp + 1); X_k streams through LDS once in tiles of 64 draws, zero-padded the same
//       way; wave w takes the 16 draws 16 w .. 16 w + 15 of the tile, the A operand x_{s, 4 j + ks}, the B operand
//       a_{i, 4 j + ks}, Dp / 4 steps.  Each accumulator entry gets its offset, goes through lb_link (gsmvi_glm_link.h) and is
//       normalised as the predictive's lpd is; the tile's l_si stay in LDS (NI x S doubles).
//   (2) per observation of the tile: ps_loo_stage (gsmvi_psis_stage.h, shared with k_psis_loo_softmax_batched): rho_s = logr_s -
//       l_si into the PSIS stage's array, ps_stage, then the two log-sum-exps -- elpd from the stage's weights, lpd from the
//       problem-level weights lw.
// The tiles of (1) lie over the stage's LDS (they are dead before the first stage starts).  NI is the largest count, at most
// PL_NI_CAP, whose l_si fit beside that region in GB_LDS_MAX.  Every sum is a fixed tree and there are no atomics; every thread
// of a workgroup runs the same barriers whatever the verdicts (the number of valid observations of a tile is uniform in it); a
// workgroup reads only slice k of the inputs and writes only its own (k, i) entries.  Inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_glm_model.h"
#include "gsmvi_psis_stage.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

struct pl_args {
    glm_model m;                // the fitted model: A, y, offset, counts, noise precision; no prior
    int S, S2, M;               // draws, draws padded to a power of two, the tail size before ties
    int NI, U;                  // observations per tile; doubles of the region the stage and the MFMA tiles share
    unsigned ntile;             // tiles per problem: ceil(N / NI)
    const double* X;            // (K, S, D) the draws of q_k
    ps_loo_io o;                // the ratios and weights of the problem-level run, the outputs
};

// doubles of the kernel's own use of the shared region: the two MFMA tiles and three per-observation arrays
static inline int pl_tiles_doubles(int D) { return (PS_LOO_TR + PS_LOO_NB) * (glm_dp(D) + 1) + 3 * PS_LOO_NB; }

static int pl_tile(int D, int S) { return ps_loo_tile(pl_tiles_doubles(D), S, PL_NI_CAP); }

template <int FAM>
__global__ __launch_bounds__(256) void k_psis_loo_batched(pl_args a) {
    extern __shared__ double pl_sm[];
    const int l = threadIdx.x, S = a.S, S2 = a.S2, M = a.M, NI = a.NI;
    const int D = a.m.D, Dp = glm_dp(D), lda = Dp + 1;
    const long long N = a.m.N;
    const size_t k = blockIdx.x / a.ntile;
    const long long i0 = (long long)(blockIdx.x - (unsigned)k * a.ntile) * NI;       // the tile's first observation
    const int ni = (int)(N - i0 < NI ? N - i0 : NI);
    const glm_problem pk = glm_problem_of<FAM>(a.m, (long long)k, true);
    const int nv = (int)(pk.nk - i0 < 0 ? 0 : (pk.nk - i0 < ni ? pk.nk - i0 : ni));  // its valid observations: the first nv
    const ps_lds sm = ps_carve(pl_sm, reinterpret_cast<int*>(pl_sm + ps_lds_doubles(S, S2)), S, S2);
    double* Xs = pl_sm;                       // 64 x lda      a tile of draws          (over the stage's arrays)
    double* As = Xs + PS_LOO_TR * lda;        // 16 x lda      the tile's rows of A_k
    double* ys = As + PS_LOO_NB * lda;        // 16 each: y_i, offset_i, the normalising term of l_si
    double* os = ys + PS_LOO_NB;
    double* cs = os + PS_LOO_NB;
    double* ell = pl_sm + a.U;                // NI x S        l_si of the tile
    const size_t ks = k * (size_t)S, kn = k * (size_t)N + (size_t)i0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    // ---- (1) l_si of the tile's valid observations ------------------------------------------------------------------------
    if (nv > 0) {                             // (uniform in the workgroup)
        const double* Ak = a.m.A + kn * D;
        for (int e = l; e < PS_LOO_NB * lda; e += 256) {
            const int r = e / lda, j = e - r * lda;
            As[e] = r < nv && j < D ? Ak[(size_t)r * D + j] : 0.0;
        }
        if (l < PS_LOO_NB) {
            const double yv = l < nv ? a.m.y[kn + l] : 0.0;
            ys[l] = yv;
            os[l] = a.m.offset && l < nv ? a.m.offset[kn + l] : 0.0;
            cs[l] = FAM == LB_POISSON ? -lgamma(yv + 1.0) : (FAM == LB_GAUSSIAN ? 0.5 * log(pk.tau / 6.28318530717958647692) : 0.0);
        }
        const double* Xk = a.X + ks * D;
        const int wv = l >> 6, ln = l & 63, cc = ln & 15, kq = ln >> 4;
        for (int t0 = 0; t0 < S; t0 += PS_LOO_TR) {
            __syncthreads();                  // the previous tile's readers are done
            for (int e = l; e < PS_LOO_TR * lda; e += 256) {
                const int r = e / lda, j = e - r * lda;
                Xs[e] = t0 + r < S && j < D ? Xk[(size_t)(t0 + r) * D + j] : 0.0;
            }
            __syncthreads();
            if (t0 + 16 * wv < S) {           // (wave-uniform)
                const double* pa = Xs + (16 * wv + cc) * lda + kq;
                const double* pb = As + cc * lda + kq;
                v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
                for (int j = 0; j < Dp; j += 4) acc = GSMVI_MFMA_F64(pa[j], pb[j], acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = t0 + 16 * wv + kq + 4 * r;    // the draw; cc is the observation
                    if (s < S && cc < nv) {
                        double g = 0.0, t = 0.0;
                        const bool ok = lb_link<FAM, false, true>(acc[r] + os[cc], ys[cc], pk.tau, g, t);
                        ell[cc * S + s] = ok ? t + cs[cc] : qnan;
                    }
                }
            }
        }
    }
    __syncthreads();                          // l_si is published; the tiles are dead, the stage may take their place

    ps_loo_stage(a.o, sm, ell, ni, nv, nullptr, ks, kn, S, S2, M, l);     // (2)
}

hipError_t gsmvi_psis_loo_batched_prepare() {
    return gb_allow_lds(k_psis_loo_batched<LB_LOGISTIC>, k_psis_loo_batched<LB_POISSON>, k_psis_loo_batched<LB_PROBIT>,
                        k_psis_loo_batched<LB_GAUSSIAN>);
}

extern "C" {

int gsmvi_psis_loo_tile(int D, int64_t S) {
    if (D < 1 || D > GB_MAX_D || S < PS_MIN_S || S > PS_MAX_S) return 0;
    return pl_tile(D, (int)S);
}

int gsmvi_psis_loo_batched_f64(gsmvi_ctx* ctx, void* stream, int family, int64_t K, int64_t N, int D, int64_t S, const double* A,
                               const double* y, const double* offset, const int* counts_dev, double noise_prec,
                               const double* noise_prec_dev, const double* X, const double* logr, const double* lw,
                               double* loglik, double* elpd, double* lpd, double* khat, double* ess, int* info) {
    const glm_model m = {K, N, D, A, y, offset, counts_dev, 0.0, nullptr, noise_prec, noise_prec_dev};
    if (int st = glm_check_model(__func__, m, family, "N", false)) return st;
    GB_BAD(S < PS_MIN_S || S > PS_MAX_S, "S must be in [5, 4096]");
    GB_BAD(!A || !y || !X || !logr || !lw || !elpd || !lpd || !khat || !ess || !info, "NULL array");
    GB_BAD(N > (INT64_MAX / 8 / S) / K, "K N S is too large");
    const int NI = pl_tile(D, (int)S);
    const int64_t ntile = (N + NI - 1) / NI;
    GB_BAD(ntile > 16777215 / K, "K ceil(N / gsmvi_psis_loo_tile(D, S)) must be at most 2^24 - 1 (one tile per workgroup)");
    const size_t nn = (size_t)K * N * 8, ns = (size_t)K * S * 8;
    if (int st = gb_check_overlaps(__func__, m, {{X, ns * D, "X", GB_RD}, {logr, ns, "logr", GB_RD}, {lw, ns, "lw", GB_RD},
                                                 {loglik, nn * S, "loglik", GB_WR}, {elpd, nn, "elpd", GB_WR}, {lpd, nn, "lpd", GB_WR},
                                                 {khat, nn, "khat", GB_WR}, {ess, nn, "ess", GB_WR},
                                                 {info, (size_t)K * N * 4, "info", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    pl_args a = {};
    a.m = m;
    a.S = (int)S;
    ps_sizes(a.S, &a.S2, &a.M);
    a.NI = NI;
    a.U = ps_loo_region_doubles(pl_tiles_doubles(D), a.S, a.S2);
    a.ntile = (unsigned)ntile;
    a.X = X;
    a.o = {logr, lw, loglik, elpd, lpd, khat, ess, info};
    const size_t lds = ((size_t)a.U + (size_t)NI * a.S) * sizeof(double);      // <= GB_LDS_MAX by the choice of NI
    const unsigned grid = (unsigned)(K * ntile);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    glm_for_family(family, [&](auto fam) {
        hipLaunchKernelGGL((k_psis_loo_batched<decltype(fam)::value>), dim3(grid), dim3(256), lds, st, a);
    });
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LOO, "k_psis_loo_batched");
}

}  // extern "C"
