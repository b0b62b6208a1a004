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
//            the four lanes of the row by a butterfly (xor 16, xor 32); lane kq = 0 adds the sum to the LDS slot of (wave, class, row)
// The slots (4 x C x 16 doubles) are the per-class accumulators: each is updated by one thread alone, tile after tile.  lpd is a
// log-sum-exp of lw_s + l_si kept as a (maximum, scaled sum) pair: the lane's four entries (their maximum, then the sum in
// order), the butterfly, then lane kq = 0 merges the tile's pair into the pair it carries from tile to tile; a pair whose
// maximum is -inf contributes 0, so no inf - inf is formed.  At the end the four waves' slots and pairs are added in wave order.
// Every sum is a fixed tree and there are no atomics.  The verdicts are flags, not arithmetic: a row with a non-finite eta at a
// draw s < S, and a problem whose lw holds a NaN or +inf or only -inf (two block reductions over lw_k before the first tile:
// ps_sum and ps_max of gsmvi_psis_stage.h, the only use of that header here), write NaN.
// The padding rule is k_psis_loo_softmax_batched's: a k position 4 j + kq >= P feeds 0.0 from the X side and loads nothing, so a
// padded position is 0 x 0 and no LDS word outside the row's D entries is read (sm_eta of gsmvi_softmax_model.h, shared with it).
// Every thread of a workgroup runs the same barriers whatever the verdicts; a workgroup reads only slice k of the inputs and
// writes only its own (k, i) entries.  A label is compared, never used as an index.  Inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_psis_stage.h"
#include "gsmvi_softmax_model.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

#define SP_TR 64        // draws per tile of X_k: one 16-row MFMA block per wave
#define SP_NB 16        // new rows per workgroup: the MFMA's 16 columns
#define SP_MAX_S 4096

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
// waves' lpd pairs and row flags, the 8 words of the block reductions
__host__ __device__ inline int sp_lds_doubles(int C, int P) {
    return SP_TR * (((C - 1) * P) | 1) + SP_NB * (sm_pp(P) + 1) + SP_NB + 2 * SP_TR + 4 * SP_NB * C + 3 * 4 * SP_NB + 8;
}

// (m1, s1) + (m2, s2) of two log-sum-exp pairs, into the first: (M, s1 e^(m1 - M) + s2 e^(m2 - M)) with M the larger maximum, whose
// own factor e^0 is exactly 1 and is not computed; a pair whose maximum is -inf contributes 0 (two of them: no inf - inf is formed)
__device__ __forceinline__ void sp_merge(double& m1, double& s1, double m2, double s2) {
    const double mm = fmax(m1, m2);
    const double e = mm == -__builtin_huge_val() ? 0.0 : exp(fmin(m1, m2) - mm);
    s1 = m1 >= m2 ? s1 + s2 * e : s1 * e + s2;
    m1 = mm;
}

__global__ __launch_bounds__(256) void k_softmax_predict_batched(sp_args a) {
    extern __shared__ double sp_sm[];
    const int l = threadIdx.x, S = a.S, C = a.C, P = a.P, Cm = C - 1, D = a.D, Pp = sm_pp(P), lda = Pp + 1, ldx = D | 1;
    const long long M = a.M;
    const size_t k = blockIdx.x / a.ntile;
    const long long i0 = (long long)(blockIdx.x - (unsigned)k * a.ntile) * SP_NB;    // the tile's first row
    const int ni = (int)(M - i0 < SP_NB ? M - i0 : SP_NB);
    const long long nk = sm_rows_of(a.counts, (long long)k, M);
    const int nv = (int)(nk - i0 < 0 ? 0 : (nk - i0 < ni ? nk - i0 : ni));           // its valid rows: the first nv
    double* Xs = sp_sm;                       // SP_TR x ldx   a tile of draws
    double* As = Xs + SP_TR * ldx;            // SP_NB x lda   the tile's rows of A_k, zero-padded
    int* ys = reinterpret_cast<int*>(As + SP_NB * lda);     // SP_NB labels (in SP_NB doubles)
    double* lws = As + SP_NB * lda + SP_NB;   // SP_TR         lw_s of the tile
    double* wts = lws + SP_TR;                // SP_TR         w_s = exp(lw_s)
    double* pac = wts + SP_TR;                // 4 x C x SP_NB the accumulator slots: (wave, class, row)
    double* pm = pac + 4 * SP_NB * C;         // 4 x SP_NB     the waves' lpd pairs: maxima
    double* psum = pm + 4 * SP_NB;            // 4 x SP_NB                           scaled sums
    int* pbad = reinterpret_cast<int*>(psum + 4 * SP_NB);   // 4 x SP_NB row flags (in 4 x SP_NB doubles)
    double* red = psum + 2 * 4 * SP_NB;       // 8             the block reductions
    const size_t ks = k * (size_t)S, km = k * (size_t)M + (size_t)i0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL), inf = __builtin_huge_val();
    const int wv = l >> 6, ln = l & 63, cc = ln & 15, kq = ln >> 4;

    if (nv == 0) {                            // no valid row (uniform in the workgroup): nothing is loaded
        for (int e = l; e < ni * C; e += 256) a.prob[km * C + e] = qnan;
        if (a.lpd && l < ni) a.lpd[km + l] = qnan;
        return;
    }

    // ---- the problem's weights: a NaN or +inf, or nothing but -inf, refuses every row --------------------------------------
    bool wbad = false;
    const double lwu = -log((double)S), wu = 1.0 / (double)S;      // the uniform weights of lw = null
    if (a.lw) {
        double nb = 0.0, vmax = -inf;
        for (int s = l; s < S; s += 256) {
            const double v = a.lw[ks + s];
            if (!(v < inf)) nb += 1.0;        // NaN or +inf
            vmax = fmax(vmax, v);
        }
        nb = ps_sum(nb, red, l);
        vmax = ps_max(vmax, red, l);
        wbad = nb > 0.0 || vmax == -inf;
    }

    const double* Ak = a.A + km * P;
    for (int e = l; e < SP_NB * lda; e += 256) {
        const int r = e / lda, j = e - r * lda;
        As[e] = r < nv && j < P ? Ak[(size_t)r * P + j] : 0.0;
    }
    if (l < SP_NB) ys[l] = a.labels && l < nv ? a.labels[km + l] : 0;
    for (int e = l; e < 4 * SP_NB * C; e += 256) pac[e] = 0.0;

    const double* Xk = a.X + ks * D;
    const bool live = cc < nv;                // the lane's column is a valid row
    double lm = -inf, ls = 0.0;               // lane kq = 0: the row's lpd pair over the wave's draws so far
    bool rbad = false;                        // a non-finite eta of the lane's row at one of its draws
    for (int t0 = 0; t0 < S; t0 += SP_TR) {
        __syncthreads();                      // the previous tile's readers are done (first pass: As, ys, pac are published below)
        for (int e = l; e < SP_TR * ldx; e += 256) {
            const int r = e / ldx, j = e - r * ldx;
            Xs[e] = t0 + r < S && j < D ? Xk[(size_t)(t0 + r) * D + j] : 0.0;
        }
        if (l < SP_TR) {
            const double v = t0 + l < S ? (a.lw ? a.lw[ks + t0 + l] : lwu) : -inf;
            lws[l] = v;
            wts[l] = t0 + l < S ? (a.lw ? exp(v) : wu) : 0.0;
        }
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
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (live && kq == 0) pac[(wv * C + c) * SP_NB + cc] += v;
            }
            if (a.lpd) {                                    // (uniform in the grid)
                double tm = -inf, ts = 0.0;                 // the lane's four entries: their maximum, then the sum in order
                if (live) {
                    double t[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        t[r] = in[r] ? lws[16 * wv + kq + 4 * r] + (ey[r] - m[r] - sm_log_s(rest[r], z[r])) : -inf;
                        tm = fmax(tm, t[r]);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) ts += tm == -inf ? 0.0 : exp(t[r] - tm);
                }
#pragma unroll
                for (int o = 16; o <= 32; o <<= 1) {
                    const double om = __shfl_xor(tm, o), os = __shfl_xor(ts, o);
                    sp_merge(tm, ts, om, os);
                }
                sp_merge(lm, ls, tm, ts);                   // (used from lane kq = 0 alone)
            }
        }
    }
    // a row's flag: its four lanes, then its four waves
    int fl = rbad ? 1 : 0;
    fl |= __shfl_xor(fl, 16);
    fl |= __shfl_xor(fl, 32);
    if (kq == 0) {
        pm[wv * SP_NB + cc] = lm;
        psum[wv * SP_NB + cc] = ls;
        pbad[wv * SP_NB + cc] = fl;
    }
    __syncthreads();

    // ---- the tile's outputs: the waves in order ------------------------------------------------------------------------------
    for (int e = l; e < ni * C; e += 256) {
        const int r = e / C, c = e - r * C;
        const bool bad = r >= nv || wbad || (pbad[r] | pbad[SP_NB + r] | pbad[2 * SP_NB + r] | pbad[3 * SP_NB + r]) != 0;
        const double* q = pac + c * SP_NB + r;
        a.prob[km * C + e] = bad ? qnan : ((q[0] + q[C * SP_NB]) + q[2 * C * SP_NB]) + q[3 * C * SP_NB];
    }
    if (a.lpd && l < ni) {
        const int yv = ys[l];
        const bool bad = l >= nv || wbad || yv < 0 || yv > Cm ||
                         (pbad[l] | pbad[SP_NB + l] | pbad[2 * SP_NB + l] | pbad[3 * SP_NB + l]) != 0;
        double mm = pm[l], ss = psum[l];
        for (int w = 1; w < 4; ++w) sp_merge(mm, ss, pm[w * SP_NB + l], psum[w * SP_NB + l]);
        a.lpd[km + l] = bad ? qnan : mm + log(ss);
    }
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
    GB_BAD(S < 1 || S > SP_MAX_S, "S must be in [1, 4096]");
    GB_BAD(!A || !X || !prob, "NULL array");
    GB_BAD((labels != nullptr) != (lpd != nullptr), "labels and lpd are given together or not at all");
    GB_BAD(M > (INT64_MAX / 8 / 128) / K, "K M is too large");               // K M P and K M C doubles addressable (C <= 65)
    const int64_t ntile = (M + SP_NB - 1) / SP_NB;
    GB_BAD(ntile > 16777215 / K, "K ceil(M / 16) must be at most 2^24 - 1 (one tile of 16 rows per workgroup)");
    const size_t nm = (size_t)K * M * 8, ns = (size_t)K * S * 8;
    if (int st = gb_check_overlaps(__func__, m, {{X, ns * D, "X", GB_RD}, {lw, ns, "lw", GB_RD}, {prob, nm * C, "prob", GB_WR},
                                                 {lpd, nm, "lpd", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    sp_args a = {};
    a.K = K; a.M = M; a.C = C; a.P = P; a.D = D;
    a.S = (int)S;
    a.ntile = (unsigned)ntile;
    a.A = A; a.labels = labels; a.counts = counts_dev; a.X = X; a.lw = lw; a.prob = prob; a.lpd = lpd;
    const size_t lds = (size_t)gsmvi_softmax_predict_lds_bytes(C, P);                  // <= 69 KB, reached at (65, 1)
    const unsigned grid = (unsigned)(K * ntile);
    hipLaunchKernelGGL(k_softmax_predict_batched, dim3(grid), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_PREDICT | GSMVI_PATH_BATCHED_SOFTMAX, "k_softmax_predict_batched");
}

}  // extern "C"
