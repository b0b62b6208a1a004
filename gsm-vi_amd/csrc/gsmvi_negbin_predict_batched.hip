// Batched negative binomial posterior predictive: for K fitted Gaussians q_k over (beta, theta = log r) of K overdispersed count
// regressions of one P, D = P + 1 <= 64, three log moments of the predictive of M new rows per problem and, with their counts, the
// log predictive density of every row, from S (optionally weighted) draws of q_k, one launch ("Batched
// negative binomial predictive"; the definition is in include/gsmvi_hip.h, above gsmvi_negbin_predict_batched_f64).  The reference
// has no twin.
//   k_negbin_predict_batched
// Work mapping (k_softmax_predict_batched's): one 256-thread workgroup per (problem k, tile of NBP_NB = 16 new rows): all 16 columns
// of the fp64 MFMA (16 x 16 x 4) carry a row.  The tile's rows of A_k sit in LDS zero-padded to Pp = 4 ceil(P / 4) columns (row
// stride Pp + 1) with y_i, o_i and c_i = -lgamma(y_i + 1) beside them; X_k streams through LDS once in tiles of 64 draws.  Wave w
// takes the 16 draws 16 w .. 16 w + 15 of the tile, and a lane holds four (draw, row) pairs in the MFMA's own accumulator layout:
// row cc = lane & 15, draws kq + 4 r, kq = lane >> 4.  With 16 rows every lane is busy, so the link runs where eta comes out.
// The operand (k_psis_loo_negbin_batched's rules): only the columns j < P of a draw are copied into the tile; column P (theta)
// is read beside it and never enters the operand; every padded position (j >= P, draws past S) holds 0.0.  theta_s and r_s =
// e^theta_s of the tile sit in LDS, written by thread s while the tile is loaded.  The draw flag is thread s's, from the LOADED
// values (0 x beta_sj summed over the draw's row in LDS, theta_s, r_s a positive normal number), not from the product; it is
// carried in a register from tile to tile and reduced once at the end, since it refuses the whole problem and no lane needs it
// before.
// The four outputs are log-sum-exps over the draws of
//   lw_s + eta_si,   lw_s + 2 eta_si,   lw_s + 2 eta_si - theta_s,   lw_s + t(eta_si, theta_s, y_i) + c_i
// each kept as a (maximum, scaled sum) pair: the lane's four entries (their maximum, then the sum in order), the row's four lanes
// by a butterfly (xor 16, xor 32), then the tile's pair merged into the pair the lane carries from tile to tile; at the end the
// four waves' pairs in wave order.  nbp_merge is sp_merge of gsmvi_softmax_predict_batched.hip (a pair whose maximum is -inf
// contributes 0, so no inf - inf is formed).  e^eta is never formed.  t is nb_link<false, true> of gsmvi_negbin_link.h, unchanged
// and whole: the score launch's bits at the same eta.  Without y the link is not run.
// The verdicts are flags, not arithmetic: a flagged draw s < S, or an lw that holds a NaN or +inf or only -inf, refuses every row
// of the problem; a non-finite eta_si at a draw s < S refuses row i.  Every sum is a fixed tree or chain and there are no atomics;
// every thread of a workgroup runs the same barriers whatever the verdicts; a workgroup reads only slice k of the inputs and
// writes only its own (k, i) entries.  Inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_glm_model.h"                 // glm_model's overlap table
#include "gsmvi_negbin_link.h"
#include "gsmvi_psis_stage.h"                // ps_sum, ps_max: the block reductions
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

#define NBP_TR 64        // draws per tile of X_k: one 16-row MFMA block per wave
#define NBP_NB 16        // new rows per workgroup: the MFMA's 16 columns
#define NBP_MAX_S 4096
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

__host__ __device__ inline int nbp_pp(int P) { return (P + 3) & ~3; }

// doubles of the launch's LDS: the X tile and the A tile, y_i, o_i and c_i of the 16 rows, theta_s, r_s and lw_s of the tile, the
// four waves' pairs of the four outputs, their row flags, the 8 words of the block reductions: 48192 bytes at P = 63
__host__ __device__ inline int nbp_lds_doubles(int P) {
    return (NBP_TR + NBP_NB) * (nbp_pp(P) + 1) + 3 * NBP_NB + 3 * NBP_TR + 2 * NBP_NOUT * 4 * NBP_NB + 4 * NBP_NB + 8;
}

// (m1, s1) + (m2, s2) of two log-sum-exp pairs, into the first: sp_merge's rule
__device__ __forceinline__ void nbp_merge(double& m1, double& s1, double m2, double s2) {
    const double mm = fmax(m1, m2);
    const double e = mm == -__builtin_huge_val() ? 0.0 : exp(fmin(m1, m2) - mm);
    s1 = m1 >= m2 ? s1 + s2 * e : s1 * e + s2;
    m1 = mm;
}

// the pair of a lane's four entries, then of the row's four lanes, merged into the pair (lm, ls) carried from tile to tile
__device__ __forceinline__ void nbp_fold(double& lm, double& ls, const double (&t)[4], bool live) {
    const double inf = __builtin_huge_val();
    double tm = -inf, ts = 0.0;
    if (live) {
#pragma unroll
        for (int r = 0; r < 4; ++r) tm = fmax(tm, t[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) ts += tm == -inf ? 0.0 : exp(t[r] - tm);
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const double om = __shfl_xor(tm, o), os = __shfl_xor(ts, o);
        nbp_merge(tm, ts, om, os);
    }
    nbp_merge(lm, ls, tm, ts);                 // (used from lane kq = 0 alone)
}

__global__ __launch_bounds__(256) void k_negbin_predict_batched(nbp_args a) {
    extern __shared__ double nbp_sm[];
    const int l = threadIdx.x, S = a.S, P = a.P, D = a.D, Pp = nbp_pp(P), lda = Pp + 1;
    const long long M = a.M;
    const size_t k = blockIdx.x / a.ntile;
    const long long i0 = (long long)(blockIdx.x - (unsigned)k * a.ntile) * NBP_NB;    // the tile's first row
    const int ni = (int)(M - i0 < NBP_NB ? M - i0 : NBP_NB);
    long long nk = M;
    if (a.counts) {
        const long long c = a.counts[k];
        nk = c < 0 ? 0 : (c > M ? M : c);
    }
    const int nv = (int)(nk - i0 < 0 ? 0 : (nk - i0 < ni ? nk - i0 : ni));           // its valid rows: the first nv
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
    const size_t ks = k * (size_t)S, km = k * (size_t)M + (size_t)i0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL), inf = __builtin_huge_val();
    const int wv = l >> 6, ln = l & 63, cc = ln & 15, kq = ln >> 4;

    if (nv == 0) {                            // no valid row (uniform in the workgroup): nothing is loaded
        for (int e = l; e < ni * 3; e += 256) a.lmom[km * 3 + e] = qnan;
        if (a.lpd && l < ni) a.lpd[km + l] = qnan;
        return;
    }

    // ---- the problem's weights: a NaN or +inf, or nothing but -inf, refuses every row --------------------------------------
    bool wbad = false;
    const double lwu = -log((double)S);       // the uniform weights of lw = null
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
    for (int e = l; e < NBP_NB * lda; e += 256) {
        const int r = e / lda, j = e - r * lda;
        As[e] = r < nv && j < P ? Ak[(size_t)r * P + j] : 0.0;
    }
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
        for (int e = l; e < NBP_TR * lda; e += 256) {
            const int r = e / lda, j = e - r * lda;
            Xs[e] = t0 + r < S && j < P ? Xk[(size_t)(t0 + r) * D + j] : 0.0;
        }
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
            const double* xr = Xs + l * lda;
            double z = 0.0;
            for (int j = 0; j < P; ++j) z += xr[j] * 0.0;                          // (NaN for a non-finite beta_sj)
            dbad = dbad || !(rr >= 2.2250738585072014e-308 && rr < inf && z == 0.0);
        }
        if (t0 + 16 * wv < S) {               // (wave-uniform)
            const double* pa = Xs + (16 * wv + cc) * lda + kq;
            const double* pb = As + cc * lda + kq;
            v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
            for (int j = 0; j < Pp; j += 4) acc = GSMVI_MFMA_F64(pa[j], pb[j], acc);
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
            nbp_fold(lm[0], ls[0], t, live);
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = in[r] ? lwv[r] + 2.0 * h[r] : -inf;
            nbp_fold(lm[1], ls[1], t, live);
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = in[r] ? lwv[r] + (2.0 * h[r] - ths[16 * wv + kq + 4 * r]) : -inf;
            nbp_fold(lm[2], ls[2], t, live);
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
                nbp_fold(lm[3], ls[3], t, live);
            }
        }
    }
    // a row's flag: its four lanes, then its four waves; the problem's: a flagged draw of any thread s
    int fl = rbad ? 1 : 0;
    fl |= __shfl_xor(fl, 16);
    fl |= __shfl_xor(fl, 32);
    if (kq == 0) {
#pragma unroll
        for (int o = 0; o < NBP_NOUT; ++o) {
            pm[(o * 4 + wv) * NBP_NB + cc] = lm[o];
            psum[(o * 4 + wv) * NBP_NB + cc] = ls[o];
        }
        pbad[wv * NBP_NB + cc] = fl;
    }
    const bool kbad = ps_sum(dbad ? 1.0 : 0.0, red, l) > 0.0 || wbad;      // (its barriers publish the pairs too)

    // ---- the tile's outputs: the waves in order ------------------------------------------------------------------------------
    for (int e = l; e < ni * NBP_NOUT; e += 256) {
        const int r = e >> 2, o = e & 3;
        if (o == 3 && !a.lpd) continue;
        const bool bad = r >= nv || kbad || (pbad[r] | pbad[NBP_NB + r] | pbad[2 * NBP_NB + r] | pbad[3 * NBP_NB + r]) != 0;
        const double* qm = pm + o * 4 * NBP_NB + r;
        const double* qs = psum + o * 4 * NBP_NB + r;
        double mm = qm[0], ss = qs[0];
        for (int w = 1; w < 4; ++w) nbp_merge(mm, ss, qm[w * NBP_NB], qs[w * NBP_NB]);
        const double v = bad ? qnan : mm + log(ss);
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
    GB_BAD(S < 1 || S > NBP_MAX_S, "S must be in [1, 4096]");
    GB_BAD(!A || !X || !lmom, "NULL array");
    GB_BAD((y != nullptr) != (lpd != nullptr), "y and lpd are given together or not at all");
    GB_BAD(M > (INT64_MAX / 8 / 64) / K, "K M is too large");                 // K M P and K M 3 doubles addressable (P <= 63)
    const int64_t ntile = (M + NBP_NB - 1) / NBP_NB;
    GB_BAD(ntile > 16777215 / K, "K ceil(M / 16) must be at most 2^24 - 1 (one tile of 16 rows per workgroup)");
    const glm_model m = {K, M, P, A, y, offset, counts_dev, 0.0, nullptr, 1.0, nullptr};
    const size_t nm = (size_t)K * M * 8, ns = (size_t)K * S * 8;
    if (int st = gb_check_overlaps(__func__, m, {{X, ns * D, "X", GB_RD}, {lw, ns, "lw", GB_RD}, {lmom, nm * 3, "lmom", GB_WR},
                                                 {lpd, nm, "lpd", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    nbp_args a = {};
    a.K = K; a.M = M; a.P = P; a.D = D;
    a.S = (int)S;
    a.ntile = (unsigned)ntile;
    a.A = A; a.y = y; a.offset = offset; a.counts = counts_dev; a.X = X; a.lw = lw; a.lmom = lmom; a.lpd = lpd;
    const size_t lds = (size_t)nbp_lds_doubles(P) * sizeof(double);            // <= 48192 bytes: below the 64 KB a launch may ask
    const unsigned grid = (unsigned)(K * ntile);                              // for without the kernel attribute
    hipLaunchKernelGGL(k_negbin_predict_batched, dim3(grid), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_PREDICT | GSMVI_PATH_BATCHED_TARGET, "k_negbin_predict_batched");
}

}  // extern "C"
