// Negative binomial Laplace initialiser: the negative Hessian of K negative binomial posteriors of one (N, P), D = P + 1 <= 64, its
// inverse, and one damped Newton round per launch for every running problem ("Negative binomial Laplace
// initialiser").
//
// The reference has no Laplace initialiser: it starts its fits from the L-BFGS-B maximiser of lp and the optimiser's dense
// inverse-Hessian estimate (gsmvi/initializers.py:5-17), for a model given as log_prob and jit(grad(...)) of it
// (examples/example_gsm.py:34-35).  For the model of gsmvi_negbin_batched_f64 at x = (beta, theta), with eta_n = a_n . beta + o_kn,
// the link (t, r_eta, r_theta) and its curvature (w_ee, w_et, w_tt) of gsmvi_negbin_link.h:
//   f_k(x) = -( sum_n t_n - lam_k |beta|^2 / 2 - kap_k (theta - m_k)^2 / 2 )
//   g_k(x) = -( sum_n r_eta,n a_n - lam_k beta,  sum_n r_theta,n - kap_k (theta - m_k) )
//   H_k(x)[:P, :P] = sum_n w_ee,n a_n a_n^T + lam_k I     H_k(x)[:P, P] = sum_n w_et,n a_n     H_k(x)[P, P] = sum_n w_tt,n + kap_k
// H is bordered and NOT positive semi-definite in general: w_tt has any sign and the posterior is not log-concave in theta.
//   k_negbin_laplace_batched<NT, OFF, LP_HESS> : H_k at the rows of X, cov_k = H_k^{-1} and info_k
//   k_negbin_laplace_batched<NT, OFF, LP_STEP> : f, g and H at the trial point Xt_k in ONE sweep over A_k, then the round's decision
// Work mapping: k_laplace_batched's (the slots of gsmvi_batched.h: gb_nt(D) threads per problem, four problems -- one wave each --
// per 256-thread workgroup for D <= 16; tiles of LB_TN = 32 rows staged in LDS zero-padded to Dp = 16 ceil(D / 16) columns, row
// stride Dp + 1; the next tile's loads in flight while the current one is consumed; NT / 32 adjacent lanes share a row's eta, one of
// them applies the link).  Column P of the staged tile holds 1.0 in every row.  The Gram product runs on the fp64 MFMA
// (16 x 16 x 4): for the 16 x 16 block (bi, bj), bi <= bj, the A operand is a_{n, 16 bi + c} and the B operand
// w_n a_{n, 16 bj + c} with w_n = w_ee,n for a column below P and w_et,n for column P (times the 1.0 held there), so the border
// column rides in the same product; eight steps per tile, at most three blocks per wave, accumulators in registers across all
// of N.  Entry (P, P) of the product is not used: thread P sums w_tt,n in order beside g_P = sum_n r_theta,n (the chain of g_j with
// the 1.0 of column P in the place of a_nj), and H[P, P] = that sum + kap.
// After the sweep the upper triangle goes to LDS, the priors are added to the diagonal, and the rest is gsmvi_laplace_stage.h: H
// written mirrored (exactly symmetric), the factorisation with the relative pivot rule 64 eps H_jj, then the inverse R^{-1} R^{-T}
// or the state machine of gsmvi_laplace_step_batched_f64 -- with one rule of this kernel's own in LP_STEP:
// The last-pivot rule.  The factorisation runs unchanged.  A failed pivot before the last ends the round with status 5, as in every
// other Laplace kernel.  When exactly the last pivot fails (info = D: the theta direction, given beta, has no positive curvature),
// with R the factor already in LDS,
//   s = H[P, P] - sum_{c < P} R[c, P]^2  (in c order),     m = |H[P, P]| + sum_{c < P} R[c, P]^2,
// and if |s| is finite and > 64 eps m the last pivot and R[P, P] become sqrt|s|, the round goes on as if info were 0 and the state
// word ist[4] (rounds with a modified pivot) grows by one; otherwise status 5.  The modified matrix R^T R is positive definite, so
// d is a descent direction and the Armijo search does the rest.  LP_HESS never modifies: a Hessian that is not positive definite
// gives info != 0 and the identity.
// Order: every sum over n runs n = 0 .. n_k - 1 in tiles of 32, eight MFMA steps of four rows per tile; it depends on (N, P) alone,
// not on K, the slot packing or the neighbours.  Rows n >= n_k are never loaded.  A non-finite x, or an e^theta that is not a
// positive normal number (the row flag of gsmvi_negbin_batched_f64), sets the slot's flag: H = NaN, info = 1 and cov = I, or status 4
// / a rejected trial.  A slot reads and writes only slice k of every array and every slot of a workgroup runs the same barriers.
// A problem whose status is not 0 is frozen: its slot loads nothing of A_k, does none of the per-tile work and writes nothing; a
// workgroup all of whose problems are frozen leaves at once.  No atomics but the *stopped_dev counter; inputs are only read; no
// context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_laplace_stage.h"
#include "gsmvi_glm_model.h"                 // glm_model's overlap table, glm_dp, LB_TN
#include "gsmvi_negbin_link.h"
#include "../../include/gsmvi_hip.h"
#include "../../include/gsmvi_hip_debug.h"   // gsmvi_debug_negbin_laplace_lds
#include <cmath>
#include <cstdint>

#define NL_AQ 8        // tile elements per thread: LB_TN P / NT <= 8 in both packings
#define NL_NROW 8      // per-row arrays of a tile: y, offset, r_eta, r_theta, t, w_ee, w_et, w_tt
#define NL_MOD 4       // ist[4]: the rounds with a modified last pivot

struct nl_args {
    long long K, N;
    int P;
    const double* A;            // (K, N, P)
    const double* y;            // (K, N)
    const double* offset;       // (K, N) added to eta, or null
    const int* counts;          // (K) valid rows, clamped to 0 .. N (null: N)
    double lam;                 // the prior precision of beta of every problem ...
    const double* lam_dev;      // ... or (K) per-problem values on the device (null: `lam`)
    double tm;                  // the prior mean of theta ...
    const double* tm_dev;       // ... or (K)
    double tk;                  // the prior precision of theta ...
    const double* tk_dev;       // ... or (K)
    lp_io io;
};

// LDS doubles per problem: the A tile (32 x (Dp + 1)), eight per-row arrays (32 each), x, g, pivots, the diagonal of H and of
// R^{-1} (Dp each), four cells, H (D x (D | 1)).  D = 64: 6820 doubles, 53.3 KB; four problems of D = 16: 4 x 1156 doubles, 36.1 KB
__host__ __device__ inline int nl_lds_doubles(int D) {
    const int Dp = glm_dp(D);
    return LB_TN * (Dp + 1) + NL_NROW * LB_TN + 5 * Dp + 4 + D * (D | 1);
}

template <int NT, bool OFF, int MODE>
__global__ __launch_bounds__(256) void k_negbin_laplace_batched(nl_args a) {
    extern __shared__ double nl_sm[];
    constexpr int PPW = 256 / NT, NW = NT / 64, NG = NT / LB_TN;
    constexpr int MAXT = NT == 256 ? 3 : 1;       // 16 x 16 blocks of H per wave
    constexpr int MAXE = NT == 256 ? 16 : 4;      // entries of H per thread
    constexpr bool STEP = MODE == LP_STEP;
    const int P = a.P, D = P + 1, nb = (D + 15) >> 4, Dp = nb * 16, lda = Dp + 1, ldh = D | 1;
    const long long N = a.N;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;
    const size_t kk = (size_t)(valid ? k : 0), kd = kk * D;
    double* As = nl_sm + (size_t)slot * nl_lds_doubles(D);
    double* Ys = As + LB_TN * lda;
    double* Os = Ys + LB_TN;
    double* Rs = Os + LB_TN;                  // r_eta
    double* Qs = Rs + LB_TN;                  // r_theta
    double* Ts = Qs + LB_TN;                  // t
    double* We = Ts + LB_TN;                  // w_ee
    double* Wc = We + LB_TN;                  // w_et
    double* Wt = Wc + LB_TN;                  // w_tt
    double* xs = Wt + LB_TN;                  // Dp  the point (zeros beyond D)
    double* gs = xs + Dp;                     // Dp  g = -score there
    double* pv = gs + Dp;                     // Dp  pivots R_cc
    double* dg = pv + Dp;                     // Dp  the diagonal of H
    double* rd = dg + Dp;                     // Dp  the diagonal of R^{-1}
    double* cell = rd + Dp;                   // [1] f
    double* Hs = cell + 4;                    // D x ldh

    int* is = STEP ? a.io.ist + kk * LP_NIS : nullptr;
    double* sc = STEP ? a.io.sc + kk * LP_NSC : nullptr;
    lp_run s;
    bool live = valid;
    if (STEP) {
        lp_load_state(a.io, valid, is, sc, s);
        live = valid && s.status == 0;
        if (!__syncthreads_or(live)) return;  // every problem of the workgroup is frozen (uniform)
    }

    const double* Ak = a.A + kk * (size_t)N * P;
    const double* yk = a.y + kk * (size_t)N;
    const double* ok_ = OFF ? a.offset + kk * (size_t)N : nullptr;
    long long nk = 0;                         // the rows that count (a frozen slot: none, so nothing of A_k is loaded)
    double lam = 0.0, tm = 0.0, tk = 0.0;
    if (live) {
        nk = N;
        if (a.counts) {
            const long long c = a.counts[k];
            nk = c < 0 ? 0 : (c > N ? N : c);
        }
        lam = a.lam_dev ? a.lam_dev[k] : a.lam;
        tm = a.tm_dev ? a.tm_dev[k] : a.tm;
        tk = a.tk_dev ? a.tk_dev[k] : a.tk;
    }
    for (int e = l; e < LB_TN * lda; e += NT) {                     // the padding columns stay zero, column P holds 1.0
        const int r = e / lda;
        As[e] = e - r * lda == P ? 1.0 : 0.0;
    }
    if (l < Dp) {
        const double* xsrc = STEP ? a.io.Xt : a.io.X;
        xs[l] = live && l < D ? xsrc[kd + l] : 0.0;
    }
    __syncthreads();                          // the zeros are in place before any thread writes the first tile
    const double theta = xs[P], rsz = exp(theta);                   // (a NaN theta gives a NaN size: flagged below)

    // the blocks of the upper triangle that this wave accumulates: block w + q NW in the order (0,0) (0,1) .. (0,nb-1) (1,1) ..
    const int wv = l >> 6, ln = l & 63, cc = ln & 15, ks = ln >> 4, ntiles = nb * (nb + 1) / 2;
    int ti[MAXT], tj[MAXT];
    v4d acc[MAXT];
#pragma unroll
    for (int q = 0; q < MAXT; ++q) {
        int tt = wv + q * NW, bi = 0;
        if (tt >= ntiles) {
            ti[q] = -1;
            tj[q] = 0;
        } else {
            while (tt >= nb - bi) {
                tt -= nb - bi;
                ++bi;
            }
            ti[q] = 16 * bi;
            tj[q] = 16 * (bi + tt);
        }
        acc[q] = v4d{0.0, 0.0, 0.0, 0.0};
    }
    // the tile elements e = l + q NT of this thread as (row, column) of the (32 x P) tile, stepped without a division
    const int row0 = l / P, col0 = l - row0 * P, dr = NT / P, dc = NT - dr * P;
    const int en = l / NG, eg = l % NG;       // the eta pass: row en of the tile, columns eg, eg + NG, ..

    double pre[NL_AQ], ypre = 0.0, opre = 0.0;
    {
        const int tnv = (int)(nk < LB_TN ? nk : LB_TN), te = tnv * P;
#pragma unroll
        for (int q = 0; q < NL_AQ; ++q) {
            const int e = l + q * NT;
            pre[q] = e < te ? Ak[e] : 0.0;
        }
        if (l < tnv) {
            ypre = yk[l];
            if (OFF) opre = ok_[l];
        }
    }
    double gacc = 0.0, facc = 0.0, hacc = 0.0;
    const double* Rg = l == P ? Qs : Rs;      // thread P sums r_theta against the 1.0 of column P

    for (long long n0 = 0; n0 < N; n0 += LB_TN) {
        const long long left = nk - n0;
        const int tnv = left < 0 ? 0 : (int)(left < LB_TN ? left : LB_TN);
        // a tile without a row that counts (past n_k; every tile of a frozen slot) does none of the work below: it only runs
        // the barriers, which must stay uniform across the slots of a workgroup (tnv is uniform in the slot)
        if (tnv > 0) {                        // registers -> LDS: the whole tile, zeros in the rows that do not count
            int r = row0, c = col0;
#pragma unroll
            for (int q = 0; q < NL_AQ; ++q) {
                if (l + q * NT < LB_TN * P) As[r * lda + c] = pre[q];
                r += dr;
                c += dc;
                if (c >= P) {
                    c -= P;
                    ++r;
                }
            }
            if (l < LB_TN) {
                Ys[l] = ypre;
                Os[l] = opre;
            }
        }
        __syncthreads();
        {                                     // the next tile's loads: in flight while this one is consumed
            const long long left2 = left - LB_TN;
            const int tnv2 = left2 < 0 ? 0 : (int)(left2 < LB_TN ? left2 : LB_TN), te2 = tnv2 * P;
            const double* An = Ak + (size_t)(n0 + LB_TN) * P;
#pragma unroll
            for (int q = 0; q < NL_AQ; ++q) {
                const int e = l + q * NT;
                pre[q] = e < te2 ? An[e] : 0.0;
            }
            ypre = 0.0;
            opre = 0.0;
            if (l < tnv2) {
                ypre = yk[n0 + LB_TN + l];
                if (OFF) opre = ok_[n0 + LB_TN + l];
            }
        }
        if (tnv > 0) {                        // eta of row en: NG adjacent lanes take the columns eg + i NG, then a butterfly
            const double* ar = As + en * lda;
            double eta = 0.0;
            for (int j = eg; j < P; j += NG) eta = fma(ar[j], xs[j], eta);
#pragma unroll
            for (int o = NG / 2; o > 0; o >>= 1) eta += __shfl_xor(eta, o);
            if (OFF) eta += Os[en];
            if (eg == 0) {
                double re = 0.0, rt = 0.0, tt = 0.0, wee = 0.0, wet = 0.0, wtt = 0.0;
                nb_link_curv<STEP>(eta, theta, rsz, Ys[en], re, rt, tt, wee, wet, wtt);
                const bool on = en < tnv;
                We[en] = on ? wee : 0.0;
                Wc[en] = on ? wet : 0.0;
                Wt[en] = on ? wtt : 0.0;
                if (STEP) {
                    Rs[en] = on ? re : 0.0;
                    Qs[en] = on ? rt : 0.0;
                    Ts[en] = on ? tt : 0.0;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < MAXT; ++q) {
            if (ti[q] >= 0 && tnv > 0) {      // (wave-uniform)
                const double* pa = As + ks * lda + ti[q] + cc;
                const double* pb = As + ks * lda + tj[q] + cc;
                const double* pw = (tj[q] + cc == P ? Wc : We) + ks;
#pragma unroll
                for (int st = 0; st < LB_TN / 4; ++st) {
                    const double av = pa[4 * st * lda], bv = pw[4 * st] * pb[4 * st * lda];
                    acc[q] = GSMVI_MFMA_F64(av, bv, acc[q]);
                }
            }
        }
        if (l < D) {
            if (STEP)
                for (int n = 0; n < tnv; ++n) gacc = fma(Rg[n], As[n * lda + l], gacc);
            if (l == P)
                for (int n = 0; n < tnv; ++n) hacc += Wt[n];
        }
        if (STEP && l == NT - 1)
            for (int n = 0; n < tnv; ++n) facc += Ts[n];
        __syncthreads();                      // the next tile overwrites As, Ys, Os and the per-row results
    }

    // the upper triangle of the product -> LDS, g and f of phi = -lp
#pragma unroll
    for (int q = 0; q < MAXT; ++q) {
        if (ti[q] >= 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ti[q] + ks + 4 * r, j = tj[q] + cc;
                if (i <= j && j < D) Hs[i * ldh + j] = acc[q][r];
            }
        }
    }
    if (STEP) {
        if (l < Dp) gs[l] = l < P ? -(gacc - lam * xs[l]) : l == P ? -(gacc - tk * (theta - tm)) : 0.0;
        if (l == NT - 1) {
            double bb = 0.0;
            for (int j = 0; j < P; ++j) bb += xs[j] * xs[j];
            const double dm = theta - tm;
            cell[1] = -(facc - 0.5 * lam * bb - 0.5 * tk * (dm * dm));
        }
    }
    __syncthreads();
    if (l < D) {                              // (entry (P, P) of the product, sum_n w_et,n, is replaced here)
        const double v = l == P ? hacc + tk : Hs[l * ldh + l] + lam;
        Hs[l * ldh + l] = v;
        dg[l] = v;
    }
    __syncthreads();
    // a non-finite x or a size that is not a positive normal number (uniform in the slot: every wave forms it from the same numbers)
    const bool bad = !(gb_wave_sum(ln < D ? xs[ln] * 0.0 : 0.0) == 0.0) ||
                     !(rsz >= 2.2250738585072014e-308 && rsz < __builtin_huge_val());

    lp_verdict v;
    bool need;
    if (STEP) {
        lp_step_test(a.io, live, bad, D, ln, gs, cell, s, v);
        need = v.need;
    } else {
        need = live && !bad && a.io.cov != nullptr;
        lp_write_h<NT, MAXE>(a.io, live, bad, kk, D, l, ldh, Hs);
    }

    int info = lp_chol_lds<NT, MAXE>(need, D, l, ldh, Hs, pv, dg);     // (its last barrier publishes R and the pivots)

    if (!STEP) {
        if (!a.io.cov) return;                   // (uniform)
        lp_inverse_tail<NT, MAXE>(a.io, live, bad, need, info, k, kk, D, l, ldh, Hs, pv, rd);
        return;
    }
    // the last-pivot rule (every thread of the slot forms s and m from the same cells of LDS, which nothing writes here)
    bool mod = false;
    double lastp = 0.0;
    if (need && info == D) {
        double s2 = 0.0;
        for (int c = 0; c < P; ++c) {
            const double rc = Hs[c * ldh + P];
            s2 += rc * rc;
        }
        double sp = dg[P];
        for (int c = 0; c < P; ++c) {
            const double rc = Hs[c * ldh + P];
            sp -= rc * rc;
        }
        const double m = fabs(dg[P]) + s2, as = fabs(sp);
        mod = as < __builtin_huge_val() && as > LP_PIVOT_REL * m;
        lastp = sqrt(as);
    }
    if (mod && l == 0) {
        pv[P] = lastp;
        Hs[P * ldh + P] = lastp;
    }
    __syncthreads();                          // (uniform: every slot of the workgroup is here)
    if (mod) info = 0;
    if (!live || l >= 64) return;             // the rest is the first wave's: component l of every vector in lane l
    lp_step_tail(a.io, s, v, info, kd, D, l, ldh, Hs, pv, xs, sc, is);
    if (mod && l == 0) is[NL_MOD] = (a.io.start ? 0 : is[NL_MOD]) + 1;    // (after the tail's own writes of the state words)
}

template <int MODE>
static int nl_go(gsmvi_ctx* ctx, void* stream, const nl_args& a) {
    int ppw;
    unsigned grid;
    const size_t lds = lp_slot_launch(a.K, a.P + 1, nl_lds_doubles(a.P + 1), 0, &ppw, &grid);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (ppw == 4) {
        if (a.offset) hipLaunchKernelGGL((k_negbin_laplace_batched<64, true, MODE>), dim3(grid), dim3(256), lds, st, a);
        else hipLaunchKernelGGL((k_negbin_laplace_batched<64, false, MODE>), dim3(grid), dim3(256), lds, st, a);
    } else {
        if (a.offset) hipLaunchKernelGGL((k_negbin_laplace_batched<256, true, MODE>), dim3(grid), dim3(256), lds, st, a);
        else hipLaunchKernelGGL((k_negbin_laplace_batched<256, false, MODE>), dim3(grid), dim3(256), lds, st, a);
    }
    // the pair of bits is shared with k_laplace_shared_batched alone (include/gsmvi_hip.h): no new bit is left to take
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LAPLACE | GSMVI_PATH_BATCHED_TARGET, "k_negbin_laplace_batched");
}

static bool nl_fin(double v) { return v > -__builtin_huge_val() && v < __builtin_huge_val(); }

static nl_args nl_args_of(int64_t K, int P, int64_t N, const double* A, const double* y, const double* offset, const int* counts_dev,
                          double theta_mean, const double* theta_mean_dev, double theta_prec, const double* theta_prec_dev,
                          double prior_prec, const double* prior_prec_dev, const lp_io& io) {
    return {K, N, P, A, y, offset, counts_dev, prior_prec, prior_prec_dev, theta_mean, theta_mean_dev, theta_prec, theta_prec_dev, io};
}

// the model's checks of both entry points, those of gsmvi_negbin_batched_f64 at nc = 1
static int nl_check_model(const char* fn, const nl_args& a) {
#define NL_BAD(cond, msg) \
    if (cond) return gb_bad(fn, msg)
    NL_BAD(a.P < 1 || a.P > GB_MAX_D - 1, "P must be in [1, 63] (D = P + 1 <= 64)");
    if (int st = gb_check_shape(fn, a.K, a.P + 1, gb_ppw)) return st;
    NL_BAD(a.N < 1, "N must be at least 1");
    NL_BAD(a.N > (INT64_MAX / 8 / a.P) / a.K, "K N P is too large");
    NL_BAD(!a.lam_dev && !(a.lam >= 0.0 && a.lam < __builtin_huge_val()), "prior_prec must be finite and >= 0");
    NL_BAD(!a.tm_dev && !nl_fin(a.tm), "theta_mean must be finite");
    NL_BAD(!a.tk_dev && !(a.tk >= 0.0 && a.tk < __builtin_huge_val()), "theta_prec must be finite and >= 0");
    NL_BAD(!a.A || !a.y, "NULL array");
#undef NL_BAD
    return GSMVI_OK;
}

// gb_check_overlaps over the model's eight read-only arrays followed by the entry point's own, which stand at own + 2
template <size_t NOWN>
static int nl_check_overlaps(const char* fn, const nl_args& a, gb_arr (&own)[NOWN]) {
    const glm_model m = {a.K, a.N, a.P, a.A, a.y, a.offset, a.counts, a.lam, a.lam_dev, 1.0, nullptr};
    own[0] = {a.tm_dev, (size_t)a.K * 8, "theta_mean_dev", GB_RD};
    own[1] = {a.tk_dev, (size_t)a.K * 8, "theta_prec_dev", GB_RD};
    return gb_check_overlaps(fn, m, own);
}

extern "C" {

int gsmvi_negbin_hessian_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int64_t N, const double* A, const double* y,
                                     const double* offset, const int* counts_dev, double theta_mean, const double* theta_mean_dev,
                                     double theta_prec, const double* theta_prec_dev, double prior_prec,
                                     const double* prior_prec_dev, const double* X, double* H, double* cov, int* info_dev) {
    const nl_args a = nl_args_of(K, P, N, A, y, offset, counts_dev, theta_mean, theta_mean_dev, theta_prec, theta_prec_dev, prior_prec,
                                 prior_prec_dev, lp_hess_io(X, H, cov, info_dev));
    if (int st = nl_check_model(__func__, a)) return st;
    if (int st = lp_check_hess(__func__, a.io)) return st;
    gb_arr own[2 + LP_HESS_ROWS];
    lp_hess_rows(own + 2, K, P + 1, a.io);
    if (int st = nl_check_overlaps(__func__, a, own)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    return nl_go<LP_HESS>(ctx, stream, a);
}

int gsmvi_negbin_laplace_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int64_t N, const double* A,
                                          const double* y, const double* offset, const int* counts_dev, double theta_mean,
                                          const double* theta_mean_dev, double theta_prec, const double* theta_prec_dev,
                                          double prior_prec, const double* prior_prec_dev, int start, double* x, double* g,
                                          double* d, double* sc, int* ist, double* Xt, int* stopped_dev, int maxiter, int maxfun,
                                          double gtol) {
    const nl_args a = nl_args_of(K, P, N, A, y, offset, counts_dev, theta_mean, theta_mean_dev, theta_prec, theta_prec_dev, prior_prec,
                                 prior_prec_dev, lp_step_io(start, x, g, d, sc, ist, Xt, stopped_dev, maxiter, maxfun, gtol));
    if (int st = nl_check_model(__func__, a)) return st;
    if (int st = lp_check_step(__func__, a.io)) return st;
    gb_arr own[2 + LP_STEP_ROWS];
    lp_step_rows(own + 2, K, P + 1, a.io);
    if (int st = nl_check_overlaps(__func__, a, own)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    return nl_go<LP_STEP>(ctx, stream, a);
}

// include/gsmvi_hip_debug.h: what a launch of either entry point at D = P + 1 requests (exported by the debug library only)
int gsmvi_debug_negbin_laplace_lds(int D, size_t* bytes, int* problems_per_workgroup) {
    GB_BAD(D < 2 || D > GB_MAX_D || !bytes || !problems_per_workgroup, "bad shape or NULL output");
    unsigned grid;
    *bytes = lp_slot_launch(1, D, nl_lds_doubles(D), 0, problems_per_workgroup, &grid);
    return GSMVI_OK;
}

}  // extern "C"
