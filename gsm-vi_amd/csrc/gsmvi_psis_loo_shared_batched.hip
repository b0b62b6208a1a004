// Shared-design PSIS leave-one-out: for K fitted Gaussians q_k over the coefficients of K GLMs on ONE design matrix A (N, D),
// D <= 64, with observation weights, the pointwise leave-one-out log predictive density of every observation from S draws of q_k,
// one launch ("Shared-design PSIS-LOO"; the definition is in include/gsmvi_hip.h, above
// gsmvi_psis_loo_shared_batched_f64).  The reference has no twin.
//   k_psis_loo_shared_batched<FAM>   (k_psis_loo_batched of gsmvi_psis_loo_batched.hip with the A tile read from the one A and the
//                                     valid rows selected by their weights)
// Work mapping: one 256-thread workgroup per (problem k, tile of NI = gsmvi_psis_loo_tile(D, S) consecutive observations),
// k-major: the workgroups of one tile of A are ntile apart, those of one problem are neighbours, as in the per-problem launch.
//   (1) eta = X_k A_tile^T (S x NI) on the fp64 MFMA (16 x 16 x 4), exactly k_psis_loo_batched's: the tile's rows of A sit in LDS
//       zero-padded to 16 rows of Dp = glm_dp(D) columns (row stride Dp + 1), read at row i0 of A -- there is no k term --; X_k
//       streams through LDS once in tiles of 64 draws; the same operand order and K-loop, so eta has that launch's bits.  y_i, o_i
//       and the normalising term go into LDS for the valid rows only (0 for the others: what an invalid row holds in y and offset
//       never reaches the link); a lane whose column has v_ki <= 0 or NaN skips the link and stores nothing.  l_si is the
//       UNWEIGHTED log density of one unit observation; the tile's l_si stay in LDS (NI x S doubles).
//   (2) per observation of the tile: ps_loo_stage (gsmvi_psis_stage.h, the one copy all four leave-one-out kernels share) with the
//       tile's weights: row i is valid iff v_ki > 0, rho_s = logr_s - v_ki l_si, then ps_stage and the two log-sum-exps.
// Row validity is read from the weights in global memory, the same values by every thread, so it is uniform in the workgroup and
// every thread runs the same barriers; the weights are not staged in LDS because stage (2), which needs them again, runs after the
// tiles are dead.  The LDS layout, and so NI, is k_psis_loo_batched's.  Every sum is a fixed tree and there are no atomics; a
// workgroup reads only slice k of the per-problem inputs and writes only its own (k, i) entries.  Inputs are only read; no context
// workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_glm_model.h"
#include "gsmvi_psis_stage.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

struct plw_args {
    long long K, N;
    int D;
    int S, S2, M;               // draws, draws padded to a power of two, the tail size before ties
    int NI, U;                  // observations per tile; doubles of the region the stage and the MFMA tiles share
    unsigned ntile;             // tiles per problem: ceil(N / NI)
    const double* A;            // (N, D) the one design matrix
    const double* y;            // (K, N)
    const double* offset;       // (K, N) added to eta, or null
    const double* w;            // (K, N) observation weights, or null: 1
    double tau;                 // gaussian family: the noise precision of every problem ...
    const double* tau_dev;      // ... or (K) per-problem values on the device (null: `tau`)
    const double* X;            // (K, S, D) the draws of q_k
    ps_loo_io o;                // the ratios and weights of the problem-level run, the outputs
};

// doubles of the kernel's own use of the shared region: k_psis_loo_batched's two MFMA tiles and three per-observation arrays, so
// that NI is gsmvi_psis_loo_tile(D, S)
static inline int plw_tiles_doubles(int D) { return (PS_LOO_TR + PS_LOO_NB) * (glm_dp(D) + 1) + 3 * PS_LOO_NB; }

static int plw_tile(int D, int S) { return ps_loo_tile(plw_tiles_doubles(D), S, PL_NI_CAP); }

template <int FAM>
__global__ __launch_bounds__(256) void k_psis_loo_shared_batched(plw_args a) {
    extern __shared__ double plw_sm[];
    const int l = threadIdx.x, S = a.S, S2 = a.S2, M = a.M, NI = a.NI;
    const int D = a.D, Dp = glm_dp(D), lda = Dp + 1;
    const long long N = a.N;
    const size_t k = blockIdx.x / a.ntile;
    const long long i0 = (long long)(blockIdx.x - (unsigned)k * a.ntile) * NI;       // the tile's first observation
    const int ni = (int)(N - i0 < NI ? N - i0 : NI);
    const size_t ks = k * (size_t)S, kn = k * (size_t)N + (size_t)i0;
    const double* wk = a.w ? a.w + kn : nullptr;                                     // the tile's weights (ni of them)
    bool any = wk == nullptr;                 // a valid row in the tile (uniform in the workgroup: the same loads in every thread)
    for (int i = 0; i < ni && !any; ++i) any = wk[i] > 0.0;
    double tau = 1.0;
    if (FAM == LB_GAUSSIAN) tau = a.tau_dev ? a.tau_dev[k] : a.tau;
    const ps_lds sm = ps_carve(plw_sm, reinterpret_cast<int*>(plw_sm + ps_lds_doubles(S, S2)), S, S2);
    double* Xs = plw_sm;                      // 64 x lda      a tile of draws          (over the stage's arrays)
    double* As = Xs + PS_LOO_TR * lda;        // 16 x lda      the tile's rows of A
    double* ys = As + PS_LOO_NB * lda;        // 16 each: y_i, offset_i, the normalising term of l_si
    double* os = ys + PS_LOO_NB;
    double* cs = os + PS_LOO_NB;
    double* ell = plw_sm + a.U;               // NI x S        l_si of the tile
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    // ---- (1) l_si of the tile's valid observations ------------------------------------------------------------------------
    if (any) {
        const double* At = a.A + (size_t)i0 * D;
        for (int e = l; e < PS_LOO_NB * lda; e += 256) {
            const int r = e / lda, j = e - r * lda;
            As[e] = r < ni && j < D ? At[(size_t)r * D + j] : 0.0;
        }
        if (l < PS_LOO_NB) {
            const bool on = l < ni && (!wk || wk[l] > 0.0);
            const double yv = on ? a.y[kn + l] : 0.0;
            ys[l] = yv;
            os[l] = a.offset && on ? a.offset[kn + l] : 0.0;
            cs[l] = FAM == LB_POISSON ? -lgamma(yv + 1.0) : (FAM == LB_GAUSSIAN ? 0.5 * log(tau / 6.28318530717958647692) : 0.0);
        }
        const double* Xk = a.X + ks * D;
        const int wv = l >> 6, ln = l & 63, cc = ln & 15, kq = ln >> 4;
        const bool von = cc < ni && (!wk || wk[cc] > 0.0);      // this lane's column is a valid observation
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
                    if (s < S && von) {
                        double g = 0.0, t = 0.0;
                        const bool ok = lb_link<FAM, false, true>(acc[r] + os[cc], ys[cc], tau, g, t);
                        ell[cc * S + s] = ok ? t + cs[cc] : qnan;
                    }
                }
            }
        }
    }
    __syncthreads();                          // l_si is published; the tiles are dead, the stage may take their place

    ps_loo_stage(a.o, sm, ell, ni, ni, wk, ks, kn, S, S2, M, l);     // (2)
}

hipError_t gsmvi_psis_loo_shared_batched_prepare() {
    return gb_allow_lds(k_psis_loo_shared_batched<LB_LOGISTIC>, k_psis_loo_shared_batched<LB_POISSON>,
                        k_psis_loo_shared_batched<LB_PROBIT>, k_psis_loo_shared_batched<LB_GAUSSIAN>);
}

extern "C" {

int gsmvi_psis_loo_shared_batched_f64(gsmvi_ctx* ctx, void* stream, int family, int64_t K, int64_t N, int D, int64_t S,
                                      const double* A, const double* y, const double* offset, const double* weights,
                                      double noise_prec, const double* noise_prec_dev, const double* X, const double* logr,
                                      const double* lw, double* loglik, double* elpd, double* lpd, double* khat, double* ess,
                                      int* info) {
    // the model's checks are the per-problem entry's (its "K N D is too large" bounds y, offset and weights, and A a fortiori)
    const glm_model m = {K, N, D, A, y, offset, nullptr, 0.0, nullptr, noise_prec, noise_prec_dev};
    if (int st = glm_check_model(__func__, m, family, "N", false)) return st;
    GB_BAD(S < PS_MIN_S || S > PS_MAX_S, "S must be in [5, 4096]");
    GB_BAD(!A || !y || !X || !logr || !lw || !elpd || !lpd || !khat || !ess || !info, "NULL array");
    GB_BAD(N > (INT64_MAX / 8 / S) / K, "K N S is too large");
    const int NI = plw_tile(D, (int)S);
    const int64_t ntile = (N + NI - 1) / NI;
    GB_BAD(ntile > 16777215 / K, "K ceil(N / gsmvi_psis_loo_tile(D, S)) must be at most 2^24 - 1 (one tile per workgroup)");
    const size_t nn = (size_t)K * N * 8, ns = (size_t)K * S * 8;
    const gb_arr all[] = {{A, (size_t)N * D * 8, "A", GB_RD},       // (one (N, D) matrix here)
                          {y, nn, "y", GB_RD},
                          {offset, nn, "offset", GB_RD},
                          {weights, nn, "weights", GB_RD},
                          {noise_prec_dev, (size_t)K * 8, "noise_prec_dev", GB_RD},
                          {X, ns * D, "X", GB_RD},
                          {logr, ns, "logr", GB_RD},
                          {lw, ns, "lw", GB_RD},
                          {loglik, nn * S, "loglik", GB_WR},
                          {elpd, nn, "elpd", GB_WR},
                          {lpd, nn, "lpd", GB_WR},
                          {khat, nn, "khat", GB_WR},
                          {ess, nn, "ess", GB_WR},
                          {info, (size_t)K * N * 4, "info", GB_WR}};
    if (int st = gb_check_overlaps(__func__, all, all + sizeof all / sizeof all[0])) return st;
    GB_BAD(!ctx, "ctx is NULL");
    plw_args a = {};
    a.K = K; a.N = N; a.D = D;
    a.S = (int)S;
    ps_sizes(a.S, &a.S2, &a.M);
    a.NI = NI;
    a.U = ps_loo_region_doubles(plw_tiles_doubles(D), a.S, a.S2);
    a.ntile = (unsigned)ntile;
    a.A = A; a.y = y; a.offset = offset; a.w = weights;
    a.tau = noise_prec; a.tau_dev = noise_prec_dev;
    a.X = X;
    a.o = {logr, lw, loglik, elpd, lpd, khat, ess, info};
    const size_t lds = ((size_t)a.U + (size_t)NI * a.S) * sizeof(double);      // <= GB_LDS_MAX by the choice of NI
    const unsigned grid = (unsigned)(K * ntile);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    glm_for_family(family, [&](auto fam) {
        hipLaunchKernelGGL((k_psis_loo_shared_batched<decltype(fam)::value>), dim3(grid), dim3(256), lds, st, a);
    });
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_TARGET, "k_psis_loo_shared_batched");
}

}  // extern "C"
