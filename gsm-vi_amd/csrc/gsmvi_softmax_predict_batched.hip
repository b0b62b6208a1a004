// Batched softmax posterior predictive: for K fitted Gaussians q_k over the coefficients of K multinomial logit regressions of one
// (C, P), D = (C - 1) P <= 64, the class probabilities of M new rows per problem and, with their labels, the log predictive density
// of every row, from S (optionally weighted) draws of q_k, one launch ("Batched softmax predictive"; the
// definition is in include/gsmvi_hip.h, above gsmvi_softmax_predict_batched_f64).  The reference has no twin.
//   k_softmax_predict_batched       (not a template over C: the class loops are rolled, as in k_psis_loo_softmax_batched)
// Work mapping: one 256-thread workgroup per (problem k, tile of SP_NB = 16 new rows): all 16 columns of the fp64 MFMA
// (16 x 16 x 4) carry a row.  The tile's rows of A_k sit in LDS zero-padded to Pp = 4 ceil(P / 4) columns (row stride Pp + 1); X_k
// streams through LDS once in tiles of 64 draws, rows as in memory (class-major, row stride D | 1, rows past S zero), with the
// tile's lw_s and w_s = exp(lw_s) beside it; wave w takes the 16 draws 16 w .. 16 w + 15 of the tile, and a lane holds four
// (draw, row) pairs: row cc = lane & 15, draws kq + 4 r, kq = lane >> 4.  Three sweeps over the classes, the MFMA chain recomputed
// in each (the same instructions on the same LDS values: the same bits), so no eta is stored and the registers do not depend
// on C:
//   sweep 1  m = max(0, eta_c), eta_y by comparison with the label, a non-finite eta noted
//   sweep 2  z = sum_c exp(eta_c - m) in class order, the reference class's exp(-m) last, as 1 + rest (sm_add_term of
//            gsmvi_softmax_model.h); the lpd's log z is log1p(rest) (sm_log_s: log(z) is 0 where rest < eps / 2)
//   sweep 3  per class (the reference class last) the lane's four exp(eta_c - m) (w_s / z) in order, draws s >= S left out, then
//            the slot of (wave, class, row) takes their sum (pd_add_slot)
// Everything around the sweeps is the draw-predictive block's (gsmvi_predict_draws.h: the tile position, the weight verdict and
// tile, the class slots, the log-sum-exp pair of lw_s + l_si and its fold, the row flags, the outputs; its comment gives the sum
// orders and the barrier rule).  The verdicts are flags, not arithmetic: a row with a non-finite eta at a draw s < S, and a problem
// whose lw holds a NaN or +inf or only -inf, write NaN.  Only the draw tile is this kernel's own.
// The padding rule is k_psis_loo_softmax_batched's: a k position 4 j + kq >= P feeds 0.0 from the X side and loads nothing, so a
// padded position is 0 x 0 and no LDS word outside the row's D entries is read (sm_eta of gsmvi_softmax_model.h, shared with it).
// Every thread of a workgroup runs the same barriers whatever the verdicts; a workgroup reads only slice k of the inputs and
// writes only its own (k, i) entries.  A label is compared, never used as an index.  Inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_predict_draws.h"
#include "gsmvi_softmax_model.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

#define SP_TR PD_TR     // draws per tile of X_k: one 16-row MFMA block per wave
#define SP_NB PD_NB     // new rows per workgroup: the MFMA's 16 columns

struct sp_args {
    long long K, M;
    int C, P, D;                // classes, features, (C - 1) P
    int S;                      // draws
    unsigned ntile;             // tiles per problem: ceil(M / 16)
    const double* A;            // (K, M, P)
    const int* labels;          // (K, M) or null
    const int* counts;          // (K) valid rows, clamped to 0 .. M (null: M)
    const double* X;            // (K, S, D) the draws of q_k, class-major
    const double* lw;           // (K, S) normalised log weights, or null: uniform
    double* prob;               // (K, M, C)
    double* lpd;                // (K, M) or null
};

// doubles of the launch's LDS: the X tile, the A tile, the 16 labels, lw_s and w_s of the tile, the accumulator slots, the four
// waves' lpd pairs and row flags, the 8 words of the block reductions (pd_tail_doubles)
__host__ __device__ inline int sp_lds_doubles(int C, int P) {
    return SP_TR * (((C - 1) * P) | 1) + SP_NB * (sm_pp(P) + 1) + SP_NB + 2 * SP_TR + pd_tail_doubles(C, 1);
}

__global__ __launch_bounds__(256) void k_softmax_predict_batched(sp_args a) {
    extern __shared__ double sp_sm[];
    const int l = threadIdx.x, S = a.S, C = a.C, P = a.P, Cm = C - 1, D = a.D, Pp = sm_pp(P), lda = Pp + 1, ldx = D | 1;
    const ps_loo_pos pos = pd_pos_of(a.ntile, a.M, S);
    const int nv = pd_valid(a.counts, a.M, pos);               // the tile's valid rows: the first nv
    double* Xs = sp_sm;                       // SP_TR x ldx   a tile of draws
    double* As = Xs + SP_TR * ldx;            // SP_NB x lda   the tile's rows of A_k, zero-padded
    int* ys = reinterpret_cast<int*>(As + SP_NB * lda);     // SP_NB labels (in SP_NB doubles)
    double* lws = As + SP_NB * lda + SP_NB;   // SP_TR         lw_s of the tile
    double* wts = lws + SP_TR;                // SP_TR         w_s = exp(lw_s)
    const pd_tail tl = pd_carve_tail(wts + SP_TR, C, 1);
    const double inf = __builtin_huge_val();
    const ps_loo_lane ln = ps_loo_lane_of(l);
    const int wv = ln.wv, cc = ln.cc, kq = ln.kq;

    if (nv == 0) {                            // no valid row (uniform in the workgroup)
        pd_no_rows(a.prob, C, a.lpd, pos, l);
        return;
    }
    const bool wbad = pd_weights_bad(a.lw, pos.ks, S, tl.red, l);
    const double lwu = -log((double)S), wu = 1.0 / (double)S;      // the uniform weights of lw = null

    ps_loo_load_rows(As, lda, a.A + pos.kn * P, P, nv, P, l);
    if (l < SP_NB) ys[l] = a.labels && l < nv ? a.labels[pos.kn + l] : 0;
    pd_zero_slots(tl.pac, C, l);

    const double* Xk = a.X + pos.ks * D;
    const bool live = cc < nv;                // the lane's column is a valid row
    double lm[1] = {-inf}, ls[1] = {0.0};     // lane kq = 0: the row's lpd pair over the wave's draws so far
    bool rbad = false;                        // a non-finite eta of the lane's row at one of its draws
    for (int t0 = 0; t0 < S; t0 += SP_TR) {
        __syncthreads();                      // the previous tile's readers are done (first pass: As, ys, pac are published below)
        for (int e = l; e < SP_TR * ldx; e += 256) {
            const int r = e / ldx, j = e - r * ldx;
            Xs[e] = t0 + r < S && j < D ? Xk[(size_t)(t0 + r) * D + j] : 0.0;
        }
        pd_load_weights(lws, wts, a.lw, pos.ks, t0, S, lwu, wu, l);
        __syncthreads();
        if (t0 + 16 * wv < S) {               // (wave-uniform)
            const double* px = Xs + (16 * wv + cc) * ldx + kq;
            const double* pb = As + cc * lda + kq;
            const int yv = ys[cc];
            double m[4] = {0.0, 0.0, 0.0, 0.0}, ey[4] = {0.0, 0.0, 0.0, 0.0};       // the reference class: eta = 0
            bool in[4];                       // the draw exists: s < S
            double w[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                in[r] = t0 + 16 * wv + kq + 4 * r < S;
                w[r] = wts[16 * wv + kq + 4 * r];
            }
#pragma unroll 1
            for (int c = 0; c < Cm; ++c) {                  // sweep 1: the maximum, eta_y, the finiteness
                const v4d acc = sm_eta(px, pb, c, P, Pp, kq);
                if (live) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        rbad = rbad || (in[r] && !gb_finite(acc[r]));
                        m[r] = fmax(m[r], acc[r]);
                        ey[r] = c == yv ? acc[r] : ey[r];
                    }
                }
            }
            double rest[4] = {0.0, 0.0, 0.0, 0.0}, nt[4] = {0.0, 0.0, 0.0, 0.0};      // z = 1 + rest: sm_add_term
#pragma unroll 1
            for (int c = 0; c < Cm; ++c) {                  // sweep 2: the same chain, the sum in class order
                const v4d acc = sm_eta(px, pb, c, P, Pp, kq);
                if (live) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) sm_add_term(rest[r], nt[r], exp(acc[r] - m[r]));
                }
            }
            double e0[4], z[4], g[4];                       // the reference class's term; z; the draw's weight over z, 0 for s >= S
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                e0[r] = exp(0.0 - m[r]);
                sm_add_term(rest[r], nt[r], e0[r]);
                rest[r] = sm_rest(rest[r], nt[r]);
                z[r] = 1.0 + rest[r];
                g[r] = in[r] ? w[r] / z[r] : 0.0;           // w_s / z_si once: p_sic w_s = exp(eta_sic - m_si) (w_s / z_si)
            }
#pragma unroll 1
            for (int c = 0; c < C; ++c) {                   // sweep 3: the probabilities, class by class, the reference class last
                v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
                if (c < Cm) acc = sm_eta(px, pb, c, P, Pp, kq);     // (uniform in the wave)
                double v = 0.0;
                if (live) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v += g[r] * (c < Cm ? exp(acc[r] - m[r]) : e0[r]);
                }
                pd_add_slot(tl.pac, C, c, v, live, ln);
            }
            if (a.lpd) {                                    // (uniform in the grid)
                double t[4];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    t[r] = live && in[r] ? lws[16 * wv + kq + 4 * r] + (ey[r] - m[r] - sm_log_s(rest[r], z[r])) : -inf;
                pd_fold(lm[0], ls[0], t, live);
            }
        }
    }
    pd_publish(tl, lm, ls, rbad, ln);
    __syncthreads();
    pd_write_classes(a.prob, a.lpd, tl, ys, C, nv, wbad, pos, l);
}

hipError_t gsmvi_softmax_predict_batched_prepare() { return gb_allow_lds(k_softmax_predict_batched); }

extern "C" {

int gsmvi_softmax_predict_lds_bytes(int C, int P) {
    if (!sm_shape_ok(C, P)) return 0;
    return sp_lds_doubles(C, P) * (int)sizeof(double);
}

int gsmvi_softmax_predict_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int C, int P, int64_t M, int64_t S,
                                      const double* A, const int* labels, const int* counts_dev, const double* X,
                                      const double* lw, double* prob, double* lpd) {
    const sm_model m = sm_model_of(K, M, C, P, A, labels, counts_dev);
    if (int st = sm_check_model(__func__, m, false, "M")) return st;
    const int D = m.D;
    pd_launch pl;                                                            // K M P and K M C doubles addressable (C <= 65)
    if (int st = pd_plan(__func__, K, M, S, 128, !A || !X || !prob, labels, lpd, "labels and lpd are given together or not at all", &pl))
        return st;
    const size_t nm = (size_t)K * M * 8, ns = (size_t)K * S * 8;
    if (int st = gb_check_overlaps(__func__, m, {{X, ns * D, "X", GB_RD}, {lw, ns, "lw", GB_RD}, {prob, nm * C, "prob", GB_WR},
                                                 {lpd, nm, "lpd", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    sp_args a = {};
    a.K = K; a.M = M; a.C = C; a.P = P; a.D = D;
    a.S = (int)S;
    a.ntile = pl.ntile;
    a.A = A; a.labels = labels; a.counts = counts_dev; a.X = X; a.lw = lw; a.prob = prob; a.lpd = lpd;
    const size_t lds = (size_t)gsmvi_softmax_predict_lds_bytes(C, P);                  // <= 69 KB, reached at (65, 1)
    hipLaunchKernelGGL(k_softmax_predict_batched, dim3(pl.grid), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_PREDICT | GSMVI_PATH_BATCHED_SOFTMAX, "k_softmax_predict_batched");
}

}  // extern "C"
