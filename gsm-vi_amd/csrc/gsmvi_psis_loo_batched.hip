// Batched PSIS leave-one-out: for K fitted Gaussians q_k over the coefficients of K GLMs of one (N, D), D <= 64, the pointwise
// leave-one-out log predictive density of every observation from S draws of q_k, one launch ("Batched
// PSIS-LOO" and "Shared-design PSIS-LOO"; the definitions are in include/gsmvi_hip.h: Vehtari, Gelman, Gabry 2017 with the
// correction for draws of an approximation, Magnusson, Andersen, Jonasson, Vehtari 2019).  The reference has no twin.
//   k_psis_loo_batched<FAM, SHARED>   SHARED = false: a design matrix A_k and a count of valid rows per problem
//                                     (gsmvi_psis_loo_batched_f64); true: ONE design matrix A (N, D) and observation weights
//                                     (gsmvi_psis_loo_shared_batched_f64, recorded as k_psis_loo_shared_batched)
// The work mapping, the LDS and stage (2) are the tile block's (gsmvi_psis_loo_tile.h), NI = gsmvi_psis_loo_tile(D, S) for both.
//   (1) eta = X_k A_tile^T (S x NI): the A tile has Dp = glm_dp(D) columns (row stride Dp + 1), the draw tiles the same, Dp / 4
//       steps of ps_loo_eta.  Each accumulator entry of a valid observation gets its offset, goes through lb_link
//       (gsmvi_glm_link.h) and is normalised as the predictive's lpd is; l_si is the UNWEIGHTED log density of one unit observation.
// The two forms differ in four places and nowhere else.  The A tile: read at row k N + i0 of A, rows past nv zero -- or at row i0
// of the one A (no k term), rows past ni zero.  The valid rows: the first nv = min(counts_k - i0, ni) -- or those with a weight
// v_ki > 0 (not 0, not NaN; no weights: all ni), read from global memory, the same values by every thread, so that either rule is
// uniform in the workgroup; the weights are not staged in LDS because stage (2), which needs them again, runs after the tiles are
// dead.  y_i, o_i and the normalising term go into LDS for the valid rows only (0 for the others: what an invalid row holds in y
// and offset never reaches the link), and a lane whose column is not valid skips the link and stores nothing.  tau: the same
// expression, there being no counts to read with it.  Stage (2): (nv, no weights) -- or (ni, the tile's weights): rho_s = logr_s -
// v_ki l_si.  Operand order and K-loop are one text: with A_k = A, all rows valid and no weights the two launches give the same bits.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_glm_model.h"
#include "gsmvi_psis_loo_tile.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

struct pl_args {
    glm_model m;                // the fitted model: A ((K, N, D), or the one (N, D)), y, offset, counts, noise precision; no prior
    const double* w;            // SHARED: (K, N) observation weights, or null: 1
    ps_loo_args c;
};

// doubles of the kernel's own use of the shared region: the two MFMA tiles and three per-observation arrays
static inline int pl_tiles_doubles(int D) { return (PS_LOO_TR + PS_LOO_NB) * (glm_dp(D) + 1) + 3 * PS_LOO_NB; }

template <int FAM, bool SHARED>
__global__ __launch_bounds__(256) void k_psis_loo_batched(pl_args a) {
    const int l = threadIdx.x, S = a.c.S;
    const int D = a.m.D, Dp = glm_dp(D), lda = Dp + 1;
    const ps_loo_pos p = ps_loo_pos_of(a.c, a.m.N);
    const glm_problem pk = glm_problem_of<FAM>(a.m, (long long)p.k, true);
    const double* wk = SHARED && a.w ? a.w + p.kn : nullptr;                         // the tile's weights (ni of them)
    const int nv = SHARED ? p.ni : ps_loo_valid(pk.nk, p);
    const auto on = [&](int i) { return i < nv && (!wk || wk[i] > 0.0); };           // row i of the tile is a valid observation
    bool any = SHARED ? wk == nullptr : nv > 0;                                      // a valid row in the tile
    if (SHARED)
        for (int i = 0; i < nv && !any; ++i) any = wk[i] > 0.0;
    const ps_loo_lds lds = ps_loo_carve(a.c);
    double* Xs = lds.tiles;                   // 64 x lda      a tile of draws          (over the stage's arrays)
    double* As = Xs + PS_LOO_TR * lda;        // 16 x lda      the tile's rows of A
    double* ys = As + PS_LOO_NB * lda;        // 16 each: y_i, offset_i, the normalising term of l_si
    double* os = ys + PS_LOO_NB;
    double* cs = os + PS_LOO_NB;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    // ---- (1) l_si of the tile's valid observations ------------------------------------------------------------------------
    if (any) {                                // (uniform in the workgroup)
        ps_loo_load_rows(As, lda, a.m.A + (SHARED ? (size_t)p.i0 : p.kn) * D, D, nv, D, l);
        if (l < PS_LOO_NB) {
            const bool v = on(l);
            const double yv = v ? a.m.y[p.kn + l] : 0.0;
            ys[l] = yv;
            os[l] = a.m.offset && v ? a.m.offset[p.kn + l] : 0.0;
            cs[l] = FAM == LB_POISSON ? -lgamma(yv + 1.0) : (FAM == LB_GAUSSIAN ? 0.5 * log(pk.tau / 6.28318530717958647692) : 0.0);
        }
        const double* Xk = a.c.X + p.ks * D;
        const ps_loo_lane ln = ps_loo_lane_of(l);
        const bool von = on(ln.cc);           // this lane's column is a valid observation
        for (int t0 = 0; t0 < S; t0 += PS_LOO_TR) {
            __syncthreads();                  // the previous tile's readers are done
            ps_loo_load_draws(Xs, lda, Xk, D, D, t0, S, l);
            __syncthreads();
            if (t0 + 16 * ln.wv < S) {        // (wave-uniform)
                const v4d acc = ps_loo_eta(Xs, As, lda, Dp, ln);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = ps_loo_draw(t0, ln, r);
                    if (s < S && von) {
                        double g = 0.0, t = 0.0;
                        const bool ok = lb_link<FAM, false, true>(acc[r] + os[ln.cc], ys[ln.cc], pk.tau, g, t);
                        lds.ell[ln.cc * S + s] = ok ? t + cs[ln.cc] : qnan;
                    }
                }
            }
        }
    }
    __syncthreads();                          // l_si is published; the tiles are dead, the stage may take their place

    ps_loo_stage(a.c.o, lds.sm, lds.ell, p.ni, nv, wk, p.ks, p.kn, S, a.c.S2, a.c.M, l);     // (2)
}

template <bool SHARED>
static hipError_t pl_prepare() {
    return gb_allow_lds(k_psis_loo_batched<LB_LOGISTIC, SHARED>, k_psis_loo_batched<LB_POISSON, SHARED>,
                        k_psis_loo_batched<LB_PROBIT, SHARED>, k_psis_loo_batched<LB_GAUSSIAN, SHARED>);
}
hipError_t gsmvi_psis_loo_batched_prepare() { return pl_prepare<false>(); }
hipError_t gsmvi_psis_loo_shared_batched_prepare() { return pl_prepare<true>(); }

template <bool SHARED>
static void pl_launch(int family, const glm_model& m, const double* w, const ps_loo_launch& p, void* stream) {
    const pl_args a = {m, w, p.c};
    glm_for_family(family, [&](auto fam) {
        hipLaunchKernelGGL((k_psis_loo_batched<decltype(fam)::value, SHARED>), dim3(p.grid), dim3(256), p.lds,
                           reinterpret_cast<hipStream_t>(stream), a);
    });
}

extern "C" {

int gsmvi_psis_loo_tile(int D, int64_t S) {
    if (D < 1 || D > GB_MAX_D || S < PS_MIN_S || S > PS_MAX_S) return 0;
    return ps_loo_tile(pl_tiles_doubles(D), (int)S, PL_NI_CAP);
}

int gsmvi_psis_loo_batched_f64(gsmvi_ctx* ctx, void* stream, int family, int64_t K, int64_t N, int D, int64_t S, const double* A,
                               const double* y, const double* offset, const int* counts_dev, double noise_prec,
                               const double* noise_prec_dev, const double* X, const double* logr, const double* lw,
                               double* loglik, double* elpd, double* lpd, double* khat, double* ess, int* info) {
    const glm_model m = {K, N, D, A, y, offset, counts_dev, 0.0, nullptr, noise_prec, noise_prec_dev};
    if (int st = glm_check_model(__func__, m, family, "N", false)) return st;
    ps_loo_launch p = {};
    if (int st = ps_loo_plan(__func__, K, N, S, 0, !A || !y, X, {logr, lw, loglik, elpd, lpd, khat, ess, info},
                             pl_tiles_doubles(D), PL_NI_CAP, "gsmvi_psis_loo_tile(D, S)", &p))
        return st;
    gb_arr own[PS_LOO_ROWS];
    ps_loo_overlap_rows(own, K, N, D, p.c);
    if (int st = gb_check_overlaps(__func__, m, own)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    pl_launch<false>(family, m, nullptr, p, stream);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LOO, "k_psis_loo_batched");
}

int gsmvi_psis_loo_shared_batched_f64(gsmvi_ctx* ctx, void* stream, int family, int64_t K, int64_t N, int D, int64_t S,
                                      const double* A, const double* y, const double* offset, const double* weights,
                                      double noise_prec, const double* noise_prec_dev, const double* X, const double* logr,
                                      const double* lw, double* loglik, double* elpd, double* lpd, double* khat, double* ess,
                                      int* info) {
    // the model's checks are the per-problem entry's (its "K N D is too large" bounds y, offset and weights, and A a fortiori)
    const glm_model m = {K, N, D, A, y, offset, nullptr, 0.0, nullptr, noise_prec, noise_prec_dev};
    if (int st = glm_check_model(__func__, m, family, "N", false)) return st;
    ps_loo_launch p = {};
    if (int st = ps_loo_plan(__func__, K, N, S, 0, !A || !y, X, {logr, lw, loglik, elpd, lpd, khat, ess, info},
                             pl_tiles_doubles(D), PL_NI_CAP, "gsmvi_psis_loo_tile(D, S)", &p))
        return st;
    const size_t nn = (size_t)K * N * 8;
    gb_arr all[5 + PS_LOO_ROWS] = {{A, (size_t)N * D * 8, "A", GB_RD},       // (one (N, D) matrix here)
                                   {y, nn, "y", GB_RD},
                                   {offset, nn, "offset", GB_RD},
                                   {weights, nn, "weights", GB_RD},
                                   {noise_prec_dev, (size_t)K * 8, "noise_prec_dev", GB_RD}};
    ps_loo_overlap_rows(all + 5, K, N, D, p.c);
    if (int st = gb_check_overlaps(__func__, all, all + 5 + PS_LOO_ROWS)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    pl_launch<true>(family, m, weights, p, stream);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_TARGET, "k_psis_loo_shared_batched");
}

}  // extern "C"
