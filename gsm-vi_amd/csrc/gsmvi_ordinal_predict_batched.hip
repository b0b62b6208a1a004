// Batched ordinal posterior predictive: for K fitted Gaussians q_k over x = (beta, delta) of K cumulative-logit (proportional odds)
// regressions of one (P, C), D = P + C - 1 <= 64, the class probabilities of M new rows per problem and, with their labels, the log
// predictive density of every row, from S (optionally weighted) draws of q_k, one launch ("Batched ordinal
// predictive"; the definition is in include/gsmvi_hip.h, above gsmvi_ordinal_predict_batched_f64).  The reference has no twin.
//   k_ordinal_predict_batched       (not a template over C: the class walk is rolled)
// Work mapping (the draw-predictive block's, gsmvi_predict_draws.h): one 256-thread workgroup per (problem k, tile of OP_NB = 16
// new rows): all 16 columns of the fp64 MFMA (16 x 16 x 4) carry a row.  X_k streams through LDS once in tiles of 64 draws, in three
// steps between barriers (steps (1)(a)-(b) of k_psis_loo_ordinal_batched, with its loaders, lane map and MFMA chain:
// gsmvi_psis_loo_tile.h):
//   (a) the beta columns j < P of the tile's draws into the operand tile, 64 rows of Pp = 4 ceil(P / 4) columns (row stride Pp + 1);
//       every padded position (j >= P, rows past S) holds 0.0 and loads nothing, and the C - 1 delta columns never enter the
//       operand (at C = 2 delta_0 sits right behind beta in memory: it is not read through the operand).  The 16 rows of A_k sit
//       beside it, zero-padded the same way, loaded once.  The deltas go from X_k straight into the per-draw table T (64 rows of
//       C - 1, row stride (C - 1) | 1): delta_0 as it is, w_j = e^{delta_j} for j >= 1, and g_j = -expm1(-w_j) = 1 - e^{-w_j} into
//       the table G of the same shape -- the two exponentials of a (draw, interior class) are spread over the whole workgroup.
//   (b) eta = X_tile A_tile^T, Pp / 4 steps, once per draw tile (one linear predictor per (draw, row): the accumulator stays in
//       registers).  Meanwhile thread s < 64 walks row s of T once: the draw's flag from the loaded values (a non-finite beta_sj or
//       delta_0, or a w_j, j >= 1, that is not a positive normal number: the leave-one-out kernel's rule) and the cutpoints
//       cut_0 = delta_0, cut_j = cut_{j-1} + w_j as one chain in ascending j, each written over the w_j it has just consumed
//       (k_ordinal_batched's prologue: the same bits).
//   (c) each lane walks j = 0 .. C - 2 for its four (draw, row) pairs: z_j = cut_j - eta, sigma(z_j) and sigma(-z_j) from one
//       exp(-|z_j|) (op_sig2), p_0 = sigma(z_0), p_c = sigma(z_c) sigma(-z_{c-1}) g_c for an interior class, p_{C-1} =
//       sigma(-z_{C-2}): no two probabilities are subtracted.  Per class the lane's four w_s p in order, draws s >= S left out,
//       then the four lanes of the row by a butterfly (xor 16, xor 32); lane kq = 0 adds the sum to the LDS slot of (wave, class,
//       row).  With labels, l_si = t of ord_link<false, true> (gsmvi_ordinal_link.h, unchanged) at the label, its gap term
//       formed as in the leave-one-out kernel (ord_gap of e^{delta_y} read from X_k again: the same bits), and lw_s + l_si goes
//       into the row's log-sum-exp pair.
// The slots (4 x C x 16 doubles) are the per-class accumulators: each is updated by one thread alone, tile after tile.  lpd is a
// log-sum-exp kept as (maximum, scaled sum) pairs (pd_fold and pd_merge of gsmvi_predict_draws.h: a pair whose maximum is -inf
// contributes 0).  At the end the four waves' slots and pairs are added in wave order.  Every sum is a fixed tree and there are no
// atomics.  The verdicts are flags, not arithmetic: a row with a non-finite eta at a draw s < S; a problem with a flagged draw s <
// S, whatever its weight; a problem whose lw holds a NaN or +inf or only -inf.  Everything around steps (a)-(c) is the block's (the
// tile position, the weight verdict and tile, the slots, the fold, the flags, the outputs).  Every thread of a workgroup runs the
// same barriers whatever the verdicts; a workgroup reads only slice k of the inputs and writes only its own (k, i) entries.  A label
// is compared and clamped, never used as an unchecked index.  Inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_ordinal_link.h"
#include "gsmvi_predict_draws.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

#define OP_TR PD_TR     // draws per tile of X_k: one 16-row MFMA block per wave
#define OP_NB PD_NB     // new rows per workgroup: the MFMA's 16 columns

struct op_args {
    long long M;
    int P, C;                   // columns of A, classes (D = P + C - 1)
    int S;                      // draws
    unsigned ntile;             // tiles per problem: ceil(M / 16)
    const double* A;            // (K, M, P)
    const int* y;               // (K, M) labels, or null
    const double* offset;       // (K, M) added to eta, or null
    const int* counts;          // (K) valid rows, clamped to 0 .. M (null: M)
    const double* X;            // (K, S, P + C - 1): beta, then delta
    const double* lw;           // (K, S) normalised log weights, or null: uniform
    double* prob;               // (K, M, C)
    double* lpd;                // (K, M) or null
};

__host__ __device__ inline int op_ldc(int C) { return (C - 1) | 1; }

// doubles of the launch's LDS: the X tile and the A tile (80 rows of Pp + 1), the tables T and G (64 rows of (C - 1) | 1 each), the
// 16 offsets, the 16 labels, lw_s and w_s of the tile, one cell per thread for the gap term, the accumulator slots, the four
// waves' lpd pairs and row flags, the 8 words of the block reductions
__host__ __device__ inline int op_lds_doubles(int P, int C) {
    return (OP_TR + OP_NB) * (pd_pp(P) + 1) + 2 * OP_TR * op_ldc(C) + 2 * OP_NB + 2 * OP_TR + 256 + pd_tail_doubles(C, 1);
}

__host__ __device__ inline bool op_shape_ok(int P, int C) { return C >= 2 && C <= GB_MAX_D && P >= 1 && P <= GB_MAX_D - (C - 1); }

// sigma(z) and sigma(-z) from one exponential (the two branches of ord_sps's sg): e^{+|z|} is never formed
__device__ __forceinline__ void op_sig2(double z, double& sp, double& sn) {
    const double e = exp(-fabs(z));
    const double q = 1.0 + e, big = 1.0 / q, small = e / q;
    sp = z >= 0.0 ? big : small;
    sn = z >= 0.0 ? small : big;
}

__global__ __launch_bounds__(256) void k_ordinal_predict_batched(op_args a) {
    extern __shared__ double op_sm[];
    const int l = threadIdx.x, S = a.S, C = a.C, P = a.P, lc = C - 1, D = P + lc, Pp = pd_pp(P), lda = Pp + 1, ldc = op_ldc(C);
    const ps_loo_pos pos = pd_pos_of(a.ntile, a.M, S);
    const int nv = pd_valid(a.counts, a.M, pos);               // the tile's valid rows: the first nv
    double* Xs = op_sm;                      // OP_TR x lda   the beta part of a tile of draws
    double* As = Xs + OP_TR * lda;            // OP_NB x lda   the tile's rows of A_k, zero-padded
    double* Ct = As + OP_NB * lda;            // OP_TR x ldc   delta_0 and w_j of the tile's draws, then their cutpoints
    double* Gt = Ct + OP_TR * ldc;            // OP_TR x ldc   g_j = -expm1(-w_j), j >= 1
    double* os = Gt + OP_TR * ldc;            // OP_NB         offset_i
    int* ys = reinterpret_cast<int*>(os + OP_NB);           // OP_NB labels as given (in OP_NB doubles)
    double* lws = os + 2 * OP_NB;             // OP_TR         lw_s of the tile
    double* wts = lws + OP_TR;                // OP_TR         w_s = exp(lw_s)
    double* gs = wts + OP_TR;                 // 256           the gap term of the thread's pair
    const pd_tail tl = pd_carve_tail(gs + 256, C, 1);
    const double inf = __builtin_huge_val();
    const ps_loo_lane ln = ps_loo_lane_of(l);
    const int wv = ln.wv, cc = ln.cc, kq = ln.kq;

    if (nv == 0) {                            // no valid row (uniform in the workgroup)
        pd_no_rows(a.prob, C, a.lpd, pos, l);
        return;
    }
    const double lwu = -log((double)S), wu = 1.0 / (double)S;      // the uniform weights of lw = null
    const bool wbad = pd_weights_bad(a.lw, pos.ks, S, tl.red, l);

    ps_loo_load_rows(As, lda, a.A + pos.kn * P, P, nv, P, l);
    if (l < OP_NB) {
        ys[l] = a.y && l < nv ? a.y[pos.kn + l] : 0;
        os[l] = a.offset && l < nv ? a.offset[pos.kn + l] : 0.0;
    }
    pd_zero_slots(tl.pac, C, l);

    const double* Xk = a.X + pos.ks * D;
    const bool live = cc < nv;                // the lane's column is a valid row
    double lm[1] = {-inf}, ls[1] = {0.0};     // lane kq = 0: the row's lpd pair over the wave's draws so far
    bool rbad = false;                        // a non-finite eta of the lane's row at one of its draws
    double dbad = 0.0;                        // thread s < 64: the flagged draws among s, s + 64, ...
    for (int t0 = 0; t0 < S; t0 += OP_TR) {
        __syncthreads();                      // the previous tile's readers are done (first pass: As, ys, os, pac are published below)
        ps_loo_load_draws(Xs, lda, Xk, D, P, t0, S, l);                            // (a)
        for (int e = l; e < OP_TR * lc; e += 256) {
            const int r = e / lc, j = e - r * lc;
            const double d = t0 + r < S ? Xk[(size_t)(t0 + r) * D + P + j] : 0.0;
            if (j == 0) {
                Ct[r * ldc] = d;
            } else {
                const double w = exp(d);
                Ct[r * ldc + j] = w;                                               // (a NaN delta gives a NaN w: flagged)
                Gt[r * ldc + j] = -expm1(-w);                                      // (entry 0 of G is neither written nor read)
            }
        }
        pd_load_weights(lws, wts, a.lw, pos.ks, t0, S, lwu, wu, l);
        __syncthreads();
        if (l < OP_TR) {                                                           // (b) the per-draw values ...
            double* cr = Ct + l * ldc;
            double z = pd_beta_flag(Xs + l * lda, P);
            double cut = cr[0];
            z += cut * 0.0;
            bool okw = true;
            for (int j = 1; j < lc; ++j) {
                const double w = cr[j];
                okw = okw && pd_pos_normal(w);
                cut += w;
                cr[j] = cut;                                                       // (over the w_j just read)
            }
            if (!(okw && z == 0.0)) dbad += 1.0;                                   // (a row past S holds zeros: never flagged)
        }
        const bool work = t0 + 16 * wv < S;   // ... and eta (wave-uniform)
        v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
        if (work) acc = ps_loo_eta(Xs, As, lda, Pp, ln);
        __syncthreads();
        if (work) {                                                                // (c)
            const double o = os[cc];
            const int yraw = ys[cc], yv = yraw < 0 ? 0 : (yraw > lc ? lc : yraw);
            double eta[4], w[4], sn[4] = {0.0, 0.0, 0.0, 0.0};
            bool in[4];                       // the draw exists: s < S
            const double* cr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = 16 * wv + kq + 4 * r;
                in[r] = t0 + q < S;
                w[r] = wts[q];
                eta[r] = acc[r] + o;
                cr[r] = Ct + q * ldc;
                if (live) rbad = rbad || (in[r] && !gb_finite(eta[r]));
            }
            const int go = Gt - Ct;
#pragma unroll 1
            for (int c = 0; c < C; ++c) {                   // class by class; the last one has no cutpoint of its own
                double v = 0.0;
                if (live) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double p = sn[r];                   // c = C - 1: sigma(-z_{C-2})
                        if (c < lc) {
                            double sp, sm;
                            op_sig2(cr[r][c] - eta[r], sp, sm);
                            p = c == 0 ? sp : (sp * sn[r]) * cr[r][go + c];
                            sn[r] = sm;
                        }
                        v += in[r] ? w[r] * p : 0.0;
                    }
                }
                pd_add_slot(tl.pac, C, c, v, live, ln);
            }
            if (a.lpd) {                                    // (uniform in the grid)
                double t[4] = {-inf, -inf, -inf, -inf};
                if (live) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (in[r]) {
                            const int q = 16 * wv + kq + 4 * r;
                            double glm = 0.0, qe = 0.0;
                            if (yv >= 1 && yv <= C - 2) ord_gap(exp(Xk[(size_t)(t0 + q) * D + P + yv]), glm, qe);   // w of (a), again
                            gs[l] = glm;      // the link reads lm[y]: the thread's own cell stands at index y of its table
                            double re = 0.0, ulo = 0.0, uhi = 0.0, tt = 0.0;
                            ord_link<false, true>(eta[r], yv, C, cr[r], gs + l - yv, nullptr, re, ulo, uhi, tt);
                            t[r] = lws[q] + tt;
                        }
                    }
                }
                pd_fold(lm[0], ls[0], t, live);
            }
        }
    }
    pd_publish(tl, lm, ls, rbad, ln);
    const bool kbad = pd_draws_bad(dbad, tl.red, l) || wbad;               // (its barriers publish the slots, the pairs and the flags)
    pd_write_classes(a.prob, a.lpd, tl, ys, C, nv, kbad, pos, l);
}

hipError_t gsmvi_ordinal_predict_batched_prepare() { return gb_allow_lds(k_ordinal_predict_batched); }

extern "C" {

int gsmvi_ordinal_predict_lds_bytes(int P, int C) {
    if (!op_shape_ok(P, C)) return 0;
    return op_lds_doubles(P, C) * (int)sizeof(double);
}

int gsmvi_ordinal_predict_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int C, int64_t M, int64_t S, const double* A,
                                      const int* y, const double* offset, const int* counts_dev, const double* X,
                                      const double* lw, double* prob, double* lpd) {
    GB_BAD(C < 2 || C > GB_MAX_D, "C must be in [2, 64]");
    GB_BAD(P < 1 || P > GB_MAX_D - (C - 1), "P must be in [1, 65 - C] (D = P + C - 1 <= 64)");
    GB_BAD(K < 1 || K > 16777215, "K must be in [1, 2^24 - 1]");
    GB_BAD(M < 1, "M must be at least 1");
    pd_launch pl;                                                             // K M P and K M C doubles addressable (P, C <= 64)
    if (int st = pd_plan(__func__, K, M, S, 64, !A || !X || !prob, y, lpd, "labels and lpd are given together or not at all", &pl))
        return st;
    const int D = P + C - 1;
    const size_t nm = (size_t)K * M, ns = (size_t)K * S * 8;
    if (int st = gb_check_overlaps(__func__, {{A, nm * P * 8, "A", GB_RD},
                                              {y, nm * 4, "y", GB_RD},
                                              {offset, nm * 8, "offset", GB_RD},
                                              {counts_dev, (size_t)K * 4, "counts_dev", GB_RD},
                                              {X, ns * D, "X", GB_RD},
                                              {lw, ns, "lw", GB_RD},
                                              {prob, nm * C * 8, "prob", GB_WR},
                                              {lpd, nm * 8, "lpd", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    op_args a = {};
    a.M = M; a.P = P; a.C = C;
    a.S = (int)S;
    a.ntile = pl.ntile;
    a.A = A; a.y = y; a.offset = offset; a.counts = counts_dev; a.X = X; a.lw = lw; a.prob = prob; a.lpd = lpd;
    // <= 105408 bytes, reached at (1, 64): the kernel attribute of ..._prepare() allows it
    const size_t lds = (size_t)gsmvi_ordinal_predict_lds_bytes(P, C);
    hipLaunchKernelGGL(k_ordinal_predict_batched, dim3(pl.grid), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_PREDICT | GSMVI_PATH_BATCHED_TARGET, "k_ordinal_predict_batched");
}

}  // extern "C"
