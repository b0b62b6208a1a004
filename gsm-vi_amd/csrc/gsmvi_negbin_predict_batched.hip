// Batched negative binomial posterior predictive: for K fitted Gaussians q_k over (beta, theta = log r) of K overdispersed count
// regressions of one P, D = P + 1 <= 64, three log moments of the predictive of M new rows per problem and, with their counts, the
// log predictive density of every row, from S (optionally weighted) draws of q_k, one launch ("Batched
// negative binomial predictive"; the definition is in include/gsmvi_hip.h, above gsmvi_negbin_predict_batched_f64).  The reference
// has no twin.
//   k_negbin_predict_batched
// Work mapping (the draw-predictive block's, gsmvi_predict_draws.h): one 256-thread workgroup per (problem k, tile of NBP_NB = 16
// new rows): all 16 columns of the fp64 MFMA (16 x 16 x 4) carry a row.  The tile's rows of A_k sit in LDS zero-padded to Pp = 4
// ceil(P / 4) columns (row stride Pp + 1) with y_i, o_i and c_i = -lgamma(y_i + 1) beside them; X_k streams through LDS once in
// tiles of 64 draws.  Wave w takes the 16 draws 16 w .. 16 w + 15 of the tile, and a lane holds four (draw, row) pairs in the MFMA's
// own accumulator layout: row cc = lane & 15, draws kq + 4 r, kq = lane >> 4.  With 16 rows every lane is busy, so the link runs
// where eta comes out. The operand (k_psis_loo_negbin_batched's rules): only the columns j < P of a draw are copied into the tile;
// column P (theta) is read beside it and never enters the operand; every padded position (j >= P, draws past S) holds 0.0.  theta_s
// and r_s = e^theta_s of the tile sit in LDS, written by thread s while the tile is loaded.  The draw flag is thread s's, from the
// LOADED values (0 x beta_sj summed over the draw's row in LDS, theta_s, r_s a positive normal number), not from the product; it is
// carried in a register from tile to tile and reduced once at the end, since it refuses the whole problem and no lane needs it
// before.
// The four outputs are log-sum-exps over the draws of
//   lw_s + eta_si,   lw_s + 2 eta_si,   lw_s + 2 eta_si - theta_s,   lw_s + t(eta_si, theta_s, y_i) + c_i
// each kept as a (maximum, scaled sum) pair: the lane's four entries (their maximum, then the sum in order), the row's four lanes
// by a butterfly (xor 16, xor 32), then the tile's pair merged into the pair the lane carries from tile to tile; at the end the
// four waves' pairs in wave order: pd_fold, pd_publish and pd_lse of gsmvi_predict_draws.h with four pairs (pd_merge: a pair whose
// maximum is -inf contributes 0, so no inf - inf is formed).  e^eta is never formed.  t is nb_link<false, true> of
// gsmvi_negbin_link.h, unchanged and whole: the score launch's bits at the same eta.  Without y the link is not run.
// The verdicts are flags, not arithmetic: a flagged draw s < S, or an lw that holds a NaN or +inf or only -inf, refuses every row
// of the problem; a non-finite eta_si at a draw s < S refuses row i.  Every sum is a fixed tree or chain and there are no atomics;
// every thread of a workgroup runs the same barriers whatever the verdicts; a workgroup reads only slice k of the inputs and
// writes only its own (k, i) entries.  Inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_glm_model.h"                 // glm_model's overlap table
#include "gsmvi_negbin_link.h"
#include "gsmvi_predict_draws.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

#define NBP_TR PD_TR     // draws per tile of X_k: one 16-row MFMA block per wave
#define NBP_NB PD_NB     // new rows per workgroup: the MFMA's 16 columns
#define NBP_NOUT 4       // the log-sum-exps of a row: three moments and lpd

struct nbp_args {
    long long K, M;
    int P, D;                   // columns of A, P + 1
    int S;                      // draws
    unsigned ntile;             // tiles per problem: ceil(M / 16)
    const double* A;            // (K, M, P)
    const double* y;            // (K, M) or null
    const double* offset;       // (K, M) added to eta, or null
    const int* counts;          // (K) valid rows, clamped to 0 .. M (null: M)
    const double* X;            // (K, S, D) the draws of q_k: beta, then theta
    const double* lw;           // (K, S) normalised log weights, or null: uniform
    double* lmom;               // (K, M, 3)
    double* lpd;                // (K, M) or null
};

// doubles of the launch's LDS: the X tile and the A tile, y_i, o_i and c_i of the 16 rows, theta_s, r_s and lw_s of the tile, the
// four waves' pairs of the four outputs, their row flags, the 8 words of the block reductions: 48192 bytes at P = 63
__host__ __device__ inline int nbp_lds_doubles(int P) {
    return (NBP_TR + NBP_NB) * (pd_pp(P) + 1) + 3 * NBP_NB + 3 * NBP_TR + pd_tail_doubles(0, NBP_NOUT);
}

__global__ __launch_bounds__(256) void k_negbin_predict_batched(nbp_args a) {
    extern __shared__ double nbp_sm[];
    const int l = threadIdx.x, S = a.S, P = a.P, D = a.D, Pp = pd_pp(P), lda = Pp + 1;
    const long long M = a.M;
    const ps_loo_pos pos = pd_pos_of(a.ntile, M, S);
    const int nv = pd_valid(a.counts, M, pos), ni = pos.ni;
    const size_t k = pos.k;
    const long long i0 = pos.i0;
    double* Xs = nbp_sm;                       // NBP_TR x lda   the beta part of a tile of draws
    double* As = Xs + NBP_TR * lda;            // NBP_NB x lda   the tile's rows of A_k, zero-padded
    double* ys = As + NBP_NB * lda;            // NBP_NB each: y_i, offset_i, -lgamma(y_i + 1)
    double* os = ys + NBP_NB;
    double* cs = os + NBP_NB;
    double* ths = cs + NBP_NB;                 // NBP_TR each: theta_s, r_s = e^theta_s, lw_s of the tile's draws
    double* rs = ths + NBP_TR;
    double* lws = rs + NBP_TR;
    double* pm = lws + NBP_TR;                 // NBP_NOUT x 4 x NBP_NB   the waves' pairs: maxima (output, wave, row)
    double* psum = pm + NBP_NOUT * 4 * NBP_NB;  // NBP_NOUT x 4 x NBP_NB                     scaled sums
    int* pbad = reinterpret_cast<int*>(psum + NBP_NOUT * 4 * NBP_NB);      // 4 x NBP_NB row flags (in 4 x NBP_NB doubles)
    double* red = psum + NBP_NOUT * 4 * NBP_NB + 4 * NBP_NB;               // 8    the block reductions
    const pd_tail tl = {nullptr, pm, psum, pbad, red};
    const size_t ks = pos.ks, km = pos.kn;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL), inf = __builtin_huge_val();
    const ps_loo_lane ln = ps_loo_lane_of(l);
    const int wv = ln.wv, cc = ln.cc, kq = ln.kq;

    if (nv == 0) {                            // no valid row (uniform in the workgroup): nothing is loaded
        pd_no_rows(a.lmom, 3, a.lpd, ps_loo_pos{k, i0, ni, ks, km}, l);
        return;
    }

    // ---- the problem's weights: a NaN or +inf, or nothing but -inf, refuses every row --------------------------------------
    const double lwu = -log((double)S);       // the uniform weights of lw = null
    const bool wbad = pd_weights_bad(a.lw, ks, S, red, l);

    ps_loo_load_rows(As, lda, a.A + km * P, P, nv, P, l);
    if (l < NBP_NB) {
        const double yv = a.y && l < nv ? a.y[km + l] : 0.0;
        ys[l] = yv;
        os[l] = a.offset && l < nv ? a.offset[km + l] : 0.0;
        cs[l] = -lgamma(yv + 1.0);
    }

    const double* Xk = a.X + ks * D;
    const bool live = cc < nv;                // the lane's column is a valid row
    double lm[NBP_NOUT], ls[NBP_NOUT];          // lane kq = 0: the row's pairs over the wave's draws so far
#pragma unroll
    for (int o = 0; o < NBP_NOUT; ++o) {
        lm[o] = -inf;
        ls[o] = 0.0;
    }
    bool rbad = false;                        // a non-finite eta of the lane's row at one of its draws
    bool dbad = false;                        // thread s < 64: a flagged draw among s, s + 64, ...
    for (int t0 = 0; t0 < S; t0 += NBP_TR) {
        __syncthreads();                      // the previous tile's readers are done (first pass: As, ys, os, cs are published below)
        ps_loo_load_draws(Xs, lda, Xk, D, P, t0, S, l);
        double th = 0.0, rr = 1.0;
        if (l < NBP_TR) {
            if (t0 + l < S) th = Xk[(size_t)(t0 + l) * D + P];
            rr = exp(th);                     // (a NaN theta gives a NaN r: flagged)
            ths[l] = th;
            rs[l] = rr;
            lws[l] = t0 + l < S ? (a.lw ? a.lw[ks + t0 + l] : lwu) : -inf;
        }
        __syncthreads();
        if (l < NBP_TR) {                      // the draw flag, from the loaded values
            const double z = pd_beta_flag(Xs + l * lda, P);
            dbad = dbad || !(pd_pos_normal(rr) && z == 0.0);
        }
        if (t0 + 16 * wv < S) {               // (wave-uniform)
            const v4d acc = ps_loo_eta(Xs, As, lda, Pp, ln);
            const double ov = os[cc];
            bool in[4];                       // the draw exists: s < S
            double h[4], lwv[4], t[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                in[r] = t0 + 16 * wv + kq + 4 * r < S;
                h[r] = acc[r] + ov;
                lwv[r] = lws[16 * wv + kq + 4 * r];
                if (live) rbad = rbad || (in[r] && !gb_finite(h[r]));
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = in[r] ? lwv[r] + h[r] : -inf;
            pd_fold(lm[0], ls[0], t, live);
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = in[r] ? lwv[r] + 2.0 * h[r] : -inf;
            pd_fold(lm[1], ls[1], t, live);
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = in[r] ? lwv[r] + (2.0 * h[r] - ths[16 * wv + kq + 4 * r]) : -inf;
            pd_fold(lm[2], ls[2], t, live);
            if (a.lpd) {                      // (uniform in the grid)
                const double yv = ys[cc], cv = cs[cc];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    t[r] = -inf;
                    if (live && in[r]) {
                        const int q = 16 * wv + kq + 4 * r;
                        double re = 0.0, rt = 0.0, tt = 0.0;
                        nb_link<false, true>(h[r], ths[q], rs[q], yv, re, rt, tt);
                        t[r] = lwv[r] + (tt + cv);
                    }
                }
                pd_fold(lm[3], ls[3], t, live);
            }
        }
    }
    pd_publish(tl, lm, ls, rbad, ln);
    const bool kbad = pd_draws_bad(dbad ? 1.0 : 0.0, red, l) || wbad;      // (its barriers publish the pairs too)

    // ---- the tile's outputs: the waves in order ------------------------------------------------------------------------------
    for (int e = l; e < ni * NBP_NOUT; e += 256) {
        const int r = e >> 2, o = e & 3;
        if (o == 3 && !a.lpd) continue;
        const bool bad = r >= nv || kbad || pd_row_bad(pbad, r);
        const double lse = pd_lse(tl, o, r);
        const double v = bad ? qnan : lse;
        if (o == 3)
            a.lpd[km + r] = v;
        else
            a.lmom[(km + r) * 3 + o] = v;
    }
}

extern "C" {

int gsmvi_negbin_predict_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int64_t M, int64_t S, const double* A,
                                     const double* y, const double* offset, const int* counts_dev, const double* X,
                                     const double* lw, double* lmom, double* lpd) {
    GB_BAD(P < 1 || P > GB_MAX_D - 1, "P must be in [1, 63] (D = P + 1 <= 64)");
    const int D = P + 1;
    GB_BAD(K < 1 || K > 16777215, "K must be in [1, 2^24 - 1]");
    GB_BAD(M < 1, "M must be at least 1");
    pd_launch pl;                                                             // K M P and K M 3 doubles addressable (P <= 63)
    if (int st = pd_plan(__func__, K, M, S, 64, !A || !X || !lmom, y, lpd, "y and lpd are given together or not at all", &pl)) return st;
    const glm_model m = {K, M, P, A, y, offset, counts_dev, 0.0, nullptr, 1.0, nullptr};
    const size_t nm = (size_t)K * M * 8, ns = (size_t)K * S * 8;
    if (int st = gb_check_overlaps(__func__, m, {{X, ns * D, "X", GB_RD}, {lw, ns, "lw", GB_RD}, {lmom, nm * 3, "lmom", GB_WR},
                                                 {lpd, nm, "lpd", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    nbp_args a = {};
    a.K = K; a.M = M; a.P = P; a.D = D;
    a.S = (int)S;
    a.ntile = pl.ntile;
    a.A = A; a.y = y; a.offset = offset; a.counts = counts_dev; a.X = X; a.lw = lw; a.lmom = lmom; a.lpd = lpd;
    const size_t lds = (size_t)nbp_lds_doubles(P) * sizeof(double);    // <= 48192 bytes: below the 64 KB a launch may ask for without
    hipLaunchKernelGGL(k_negbin_predict_batched, dim3(pl.grid), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);   // the attribute
    return gb_launched(ctx, GSMVI_PATH_BATCHED_PREDICT | GSMVI_PATH_BATCHED_TARGET, "k_negbin_predict_batched");
}

}  // extern "C"
