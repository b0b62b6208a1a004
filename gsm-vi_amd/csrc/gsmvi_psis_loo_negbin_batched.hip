// Batched negative binomial PSIS leave-one-out: for K fitted Gaussians q_k over (beta, theta = log r) of K overdispersed count
// regressions of one (N, P), D = P + 1 <= 64, the pointwise leave-one-out log predictive density of every observation from S draws
// of q_k, one launch ("Batched negative binomial PSIS-LOO"; the definition is in include/gsmvi_hip.h, above
// gsmvi_psis_loo_negbin_batched_f64).  The reference has no twin.
//   k_psis_loo_negbin_batched       (a sibling of k_psis_loo_batched, not one more family of it: a draw is not only coefficients)
// The work mapping, the LDS, the loaders, the MFMA chain and stage (2) are the tile block's (gsmvi_psis_loo_tile.h), with
// NI = gsmvi_psis_loo_negbin_tile(P, S) and the first nv rows of a tile valid (counts, clamped by glm_problem_of).
//   (1) l_si of the tile, per tile of PS_LOO_TR = 64 draws, in three steps between barriers:
//       (a) the tile of X_k into LDS: 64 rows of Pp = 4 ceil(P / 4) columns (row stride Pp + 1).  Only the columns j < P of a draw
//           are copied; column P of the draw (theta) never enters the operand, and every padded position (j >= P, rows past S)
//           holds 0.0.  The NI rows of A_k sit beside it zero-padded to 16 rows of the same Pp columns, loaded once.
//       (b) eta = X_tile A_tile^T, Pp / 4 steps; a lane whose column is a valid observation leaves eta_si in the cell of l_si.
//           Meanwhile thread s < 64 forms the per-draw values of draw s of the tile: theta_s
//           (read from X_k, not from the operand), r_s = e^theta_s and the flag -- from the LOADED values: a non-finite beta_sj
//           (0 x beta_sj summed over the row in LDS) or theta_s, or an r_s that is not a positive normal number (the score
//           kernel's row flag).  Not from the product: there a padded zero of A would meet a non-finite x as 0 x inf = NaN only
//           where x is in the operand, and theta is not.
//       (c) the link, re-mapped so that every lane works: entry e = l, l + 256, ... of the tile's nv x 64 (observation, draw)
//           pairs -- one per thread at NI <= 4 -- reads eta_si + o_i, runs nb_link<false, true> (gsmvi_negbin_link.h, unchanged:
//           t is bit for bit the score launch's at the same eta) and stores l_si = t + c_i, c_i = -lgamma(y_i + 1), or NaN for a
//           flagged draw.  (In the MFMA's own layout only the NI <= 4 of 16 columns would run the link's up to twelve log1p.)
//       y_i, o_i and c_i go into LDS once per workgroup.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_glm_model.h"                 // glm_model: the model's fields, its rows that count, its overlap table
#include "gsmvi_negbin_link.h"
#include "gsmvi_psis_loo_tile.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

struct pln_args {
    glm_model m;                // A (K, N, P), y, offset, counts; D = P, the columns of A; no prior, no noise precision
    ps_loo_args c;              // (X (K, S, P + 1): beta, then theta)
};

__host__ __device__ inline int pln_pp(int P) { return (P + 3) & ~3; }

// doubles of the kernel's own use of the shared region: the X tile, the A tile, three per-observation and three per-draw arrays
static inline int pln_tiles_doubles(int P) { return (PS_LOO_TR + PS_LOO_NB) * (pln_pp(P) + 1) + 3 * PS_LOO_NB + 3 * PS_LOO_TR; }

__global__ __launch_bounds__(256) void k_psis_loo_negbin_batched(pln_args a) {
    const int l = threadIdx.x, S = a.c.S;
    const int P = a.m.D, D = P + 1, Pp = pln_pp(P), lda = Pp + 1;
    const ps_loo_pos p = ps_loo_pos_of(a.c, a.m.N);
    const int nv = ps_loo_valid(glm_problem_of<LB_POISSON>(a.m, (long long)p.k, true).nk, p);
    const ps_loo_lds lds = ps_loo_carve(a.c);
    double* Xs = lds.tiles;                   // 64 x lda      the beta part of a tile of draws   (over the stage's arrays)
    double* As = Xs + PS_LOO_TR * lda;        // 16 x lda      the tile's rows of A_k, zero-padded
    double* ys = As + PS_LOO_NB * lda;        // 16 each: y_i, offset_i, -lgamma(y_i + 1)
    double* os = ys + PS_LOO_NB;
    double* cs = os + PS_LOO_NB;
    double* ths = cs + PS_LOO_NB;             // 64 each: theta_s, r_s = e^theta_s, 1.0 or 0.0 (a flagged draw) of the tile's draws
    double* rs = ths + PS_LOO_TR;
    double* fs = rs + PS_LOO_TR;
    double* ell = lds.ell;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    // ---- (1) l_si of the tile's valid observations ------------------------------------------------------------------------
    if (nv > 0) {                             // (uniform in the workgroup)
        ps_loo_load_rows(As, lda, a.m.A + p.kn * P, P, nv, P, l);
        if (l < PS_LOO_NB) {
            const double yv = l < nv ? a.m.y[p.kn + l] : 0.0;
            ys[l] = yv;
            os[l] = a.m.offset && l < nv ? a.m.offset[p.kn + l] : 0.0;
            cs[l] = -lgamma(yv + 1.0);
        }
        const double* Xk = a.c.X + p.ks * D;
        const ps_loo_lane ln = ps_loo_lane_of(l);
        for (int t0 = 0; t0 < S; t0 += PS_LOO_TR) {
            __syncthreads();                  // the previous tile's readers are done
            ps_loo_load_draws(Xs, lda, Xk, D, P, t0, S, l);                        // (a)
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
            if (t0 + 16 * ln.wv < S) {        // ... and eta (wave-uniform)
                const v4d acc = ps_loo_eta(Xs, As, lda, Pp, ln);
                if (ln.cc < nv) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int s = ps_loo_draw(t0, ln, r);
                        if (s < S) ell[ln.cc * S + s] = acc[r];
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

    ps_loo_stage(a.c.o, lds.sm, ell, p.ni, nv, nullptr, p.ks, p.kn, S, a.c.S2, a.c.M, l);     // (2)
}

hipError_t gsmvi_psis_loo_negbin_batched_prepare() { return gb_allow_lds(k_psis_loo_negbin_batched); }

extern "C" {

int gsmvi_psis_loo_negbin_tile(int P, int64_t S) {
    if (P < 1 || P > GB_MAX_D - 1 || S < PS_MIN_S || S > PS_MAX_S) return 0;
    return ps_loo_tile(pln_tiles_doubles(P), (int)S, PLN_NI_CAP);
}

int gsmvi_psis_loo_negbin_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int64_t N, int64_t S, const double* A,
                                      const double* y, const double* offset, const int* counts_dev, const double* X,
                                      const double* logr, const double* lw, double* loglik, double* elpd, double* lpd,
                                      double* khat, double* ess, int* info) {
    GB_BAD(P < 1 || P > GB_MAX_D - 1, "P must be in [1, 63] (D = P + 1 <= 64)");
    GB_BAD(K < 1 || K > 16777215, "K must be in [1, 2^24 - 1]");
    GB_BAD(N < 1, "N must be at least 1");
    ps_loo_launch p = {};
    if (int st = ps_loo_plan(__func__, K, N, S, P, !A || !y, X, {logr, lw, loglik, elpd, lpd, khat, ess, info},
                             pln_tiles_doubles(P), PLN_NI_CAP, "gsmvi_psis_loo_negbin_tile(P, S)", &p))
        return st;
    const pln_args a = {{K, N, P, A, y, offset, counts_dev, 0.0, nullptr, 1.0, nullptr}, p.c};
    gb_arr own[PS_LOO_ROWS];
    ps_loo_overlap_rows(own, K, N, P + 1, p.c);
    if (int st = gb_check_overlaps(__func__, a.m, own)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    hipLaunchKernelGGL(k_psis_loo_negbin_batched, dim3(p.grid), dim3(256), p.lds, reinterpret_cast<hipStream_t>(stream), a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_TARGET, "k_psis_loo_negbin_batched");
}

}  // extern "C"
