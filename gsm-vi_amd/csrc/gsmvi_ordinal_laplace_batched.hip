// Ordinal Laplace initialiser: the negative Hessian of K cumulative-logit posteriors of one (N, P, C), D = P + C - 1 <= 64, its
// inverse, and one damped Newton round per launch for every running problem ("Ordinal Laplace initialiser").
//
// The reference has no Laplace initialiser: it starts its fits from the L-BFGS-B maximiser of lp and the optimiser's dense
// inverse-Hessian estimate (gsmvi/initializers.py:5-17), for a model given as log_prob and jit(grad(...)) of it
// (examples/example_gsm.py:34-35).  For the model of gsmvi_ordinal_batched_f64 at x = (beta, delta), with w_0 = 1, w_i = e^{delta_i}
// (i >= 1), q_i = 1 / expm1(w_i), eta_n = a_n . beta + o_kn, the link (t, r_eta, sigma(-b), fa + fb, fb) of gsmvi_ordinal_link.h and,
// per (row n, cutpoint i),
//   e_ni = fa + fb (i < y_n), fb (i = y_n), 0 (i > y_n)        s_ni = -r_eta,n (i < y_n), sigma(-b_n) (i = y_n), 0 (i > y_n)
//   F(i) = sum_n e_ni     S_i = sum_n s_ni + q_i cnt_i     cnt_i = #{n < n_k : y_n = i}  (1 <= i <= C - 2; q_0 cnt_0 := 0)
//   f_k(x) = -( sum_n t_n - lam_k |beta|^2 / 2 - kap_k |delta|^2 / 2 )
//   g_k(x) = -( sum_n r_eta,n a_n - lam_k beta,  w_i S_i - kap_k delta_i )
//   H_k[:P, :P] = sum_n (fa + fb)_n a_n a_n^T + lam_k I            H_k[:P, P + i] = -w_i sum_n e_ni a_n
//   H_k[P + i, P + i'] = w_i w_i' F(max(i, i'))  (i != i')
//   H_k[P + i, P + i]  = w_i^2 F(i) + (w_i q_i) (w_i + w_i q_i) cnt_i + c_i + kap_k,       c_i = -w_i S_i (i >= 1), c_0 = 0
// Without the chain terms c_i (the second derivative of e^{delta_i} times the gradient) H is J^T (PSD) J + priors; they are the
// only source of indefiniteness.  For C = 2 the model is logistic regression on [A, -1].
//   k_ordinal_laplace_batched<NT, OFF, LP_HESS> : H_k at the rows of X, cov_k = H_k^{-1} and info_k
//   k_ordinal_laplace_batched<NT, OFF, LP_STEP> : f, g and H at the trial point Xt_k in ONE sweep over A_k, then the round's decision
// Work mapping: k_negbin_laplace_batched's (the slots of gsmvi_batched.h: gb_nt(D) threads per problem, four problems -- one wave
// each -- per 256-thread workgroup for D <= 16; tiles of LB_TN = 32 rows staged in LDS zero-padded to Dp = 16 ceil(D / 16) columns,
// row stride Dp + 1; the next tile's loads in flight while the current one is consumed; NT / 32 adjacent lanes share a row's eta,
// one of them applies the link and leaves the row's cells y, r_eta, sigma(-b), fa + fb, fb (and t) in LDS).  A prologue leaves
// w_i, q_i, log1mexp(w_i) and the cutpoints (one chain in i) in LDS.  The Gram product runs on the fp64 MFMA (16 x 16 x 4): for the
// 16 x 16 block (bi, bj), bi <= bj, the A operand is a_{n, 16 bi + c} (zero in the columns from P on) and the B operand
// (fa + fb)_n a_{n, j'} for a column j' < P and -e_ni for column P + i, formed from the row's cells and its label: no indicator
// columns are staged.  Entries of the product with both indices >= P are not used.  Thread P + i sums e_ni, s_ni and [y_n = i] over
// n in order: F(i), S_i and cnt_i.  The delta-delta block, the w_i scalings, the chain terms and the priors are applied in the
// epilogue in LDS, before the diagonal copy dg is taken.  The rest is gsmvi_laplace_stage.h: H written mirrored (exactly symmetric),
// the factorisation with the relative pivot rule 64 eps H_jj, then the inverse R^{-1} R^{-T} or the state machine of
// gsmvi_laplace_step_batched_f64 -- with one rule of this kernel's own in LP_STEP:
// The retry rule.  Before the factorisation the strict upper triangle of H is mirrored into the free lower triangle of Hs
// (lp_chol_lds and lp_step_tail touch only j >= i, dg holds the diagonal).  The factorisation runs unchanged.  If it fails and some
// c_i < 0, the upper triangle is restored with the diagonal dg[P + i] - min(c_i, 0) (dg follows) and factored once more; on success
// the round goes on as if info were 0 and the state word ist[4] (rounds whose direction came from the retried matrix) grows by one.
// If no c_i is negative, or the second factorisation fails: status 5.  The retried matrix is positive semi-definite plus the
// priors, so d is a descent direction and the Armijo search does the rest.  LP_HESS never modifies: a Hessian that is not positive
// definite gives info != 0 and the identity.
// Order: every sum over n runs n = 0 .. n_k - 1 in tiles of 32, eight MFMA steps of four rows per tile; it depends on (N, P, C)
// alone, not on K, the slot packing or the neighbours.  Rows n >= n_k are never loaded.  A label is clamped to 0 .. C - 1 when its
// tile is staged.  A non-finite x, or some e^{delta_j}, j >= 1, that is not a positive normal number (the row flag of
// gsmvi_ordinal_batched_f64), sets the slot's flag: H = NaN, info = 1 and cov = I, or status 4 / a rejected trial.  A slot reads and
// writes only slice k of every array and every slot of a workgroup runs the same barriers.  A problem whose status is not 0 is
// frozen: its slot loads nothing of A_k, does none of the per-tile work and writes nothing; a workgroup all of whose problems are
// frozen leaves at once.  No atomics but the *stopped_dev counter; inputs are only read; no context workspace.  Plain HIP C++ and
// GSMVI_MFMA_F64: no inline assembly.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_laplace_stage.h"
#include "gsmvi_glm_model.h"                 // glm_dp, LB_TN
#include "gsmvi_ordinal_link.h"
#include "../../include/gsmvi_hip.h"
#include "../../include/gsmvi_hip_debug.h"   // gsmvi_debug_ordinal_laplace_lds
#include <cmath>
#include <cstdint>

#define OL_AQ 8        // tile elements per thread: LB_TN P / NT <= 8 in both packings
#define OL_NROW 7      // per-row arrays of a tile: y, offset, r_eta, sigma(-b), t, fa + fb, fb
#define OL_NVEC 11     // per-problem vectors of Dp doubles
#define OL_MOD 4       // ist[4]: the rounds whose direction came from the retried matrix

struct ol_args {
    long long K, N;
    int P, C;
    const double* A;            // (K, N, P)
    const int* y;               // (K, N) labels
    const double* offset;       // (K, N) added to eta, or null
    const int* counts;          // (K) valid rows, clamped to 0 .. N (null: N)
    double lam;                 // the prior precision of beta of every problem ...
    const double* lam_dev;      // ... or (K) per-problem values on the device (null: `lam`)
    double kap;                 // the prior precision of delta ...
    const double* kap_dev;      // ... or (K)
    lp_io io;
};

// LDS doubles per problem: the A tile (32 x (Dp + 1)), seven per-row arrays (32 each), eleven vectors (Dp each: x, g, pivots, the
// diagonal of H and of R^{-1}, w, q, log1mexp(w), the cutpoints, F, c), four cells, H (D x (D | 1)).  D = 64: 7172 doubles,
// 56.0 KB; four problems of D = 16: 4 x 1220 doubles, 38.1 KB
__host__ __device__ inline int ol_lds_doubles(int D) {
    const int Dp = glm_dp(D);
    return LB_TN * (Dp + 1) + OL_NROW * LB_TN + OL_NVEC * Dp + 4 + D * (D | 1);
}

template <int NT, bool OFF, int MODE>
__global__ __launch_bounds__(256) void k_ordinal_laplace_batched(ol_args a) {
    extern __shared__ double ol_sm[];
    constexpr int PPW = 256 / NT, NW = NT / 64, NG = NT / LB_TN;
    constexpr int MAXT = NT == 256 ? 3 : 1;       // 16 x 16 blocks of H per wave
    constexpr int MAXE = NT == 256 ? 16 : 4;      // entries of H per thread
    constexpr bool STEP = MODE == LP_STEP;
    const int P = a.P, C = a.C, lc = C - 1, D = P + lc, nb = (D + 15) >> 4, Dp = nb * 16, lda = Dp + 1, ldh = D | 1, DD = D * D;
    const long long N = a.N;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;
    const size_t kk = (size_t)(valid ? k : 0), kd = kk * D;
    double* As = ol_sm + (size_t)slot * ol_lds_doubles(D);
    double* Ys = As + LB_TN * lda;            // the label, clamped to 0 .. C - 1
    double* Os = Ys + LB_TN;
    double* Rs = Os + LB_TN;                  // r_eta
    double* Sb = Rs + LB_TN;                  // sigma(-b)
    double* Ts = Sb + LB_TN;                  // t
    double* Wf = Ts + LB_TN;                  // fa + fb
    double* Wb = Wf + LB_TN;                  // fb
    double* xs = Wb + LB_TN;                  // Dp  the point (zeros beyond D)
    double* gs = xs + Dp;                     // Dp  g = -score there
    double* pv = gs + Dp;                     // Dp  pivots R_cc
    double* dg = pv + Dp;                     // Dp  the diagonal of H
    double* rd = dg + Dp;                     // Dp  the diagonal of R^{-1}
    double* wv = rd + Dp;                     // Dp  w_i (entry 0: 1.0), i = 0 .. C - 2
    double* qv = wv + Dp;                     // Dp  q_i = 1 / expm1(w_i) (entry 0: 0.0)
    double* lm = qv + Dp;                     // Dp  log1mexp(w_i) (entry 0: 0.0)
    double* ct = lm + Dp;                     // Dp  the cutpoints
    double* Fv = ct + Dp;                     // Dp  F(i)
    double* cv = Fv + Dp;                     // Dp  the chain terms c_i
    double* cell = cv + Dp;                   // [1] f
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
    const int* yk = a.y + kk * (size_t)N;
    const double* ok_ = OFF ? a.offset + kk * (size_t)N : nullptr;
    long long nk = 0;                         // the rows that count (a frozen slot: none, so nothing of A_k is loaded)
    double lam = 0.0, kap = 0.0;
    if (live) {
        nk = N;
        if (a.counts) {
            const long long c = a.counts[k];
            nk = c < 0 ? 0 : (c > N ? N : c);
        }
        lam = a.lam_dev ? a.lam_dev[k] : a.lam;
        kap = a.kap_dev ? a.kap_dev[k] : a.kap;
    }
    for (int e = l; e < LB_TN * lda; e += NT) As[e] = 0.0;          // the padding columns (from P on) stay zero
    if (l < Dp) {
        const double* xsrc = STEP ? a.io.Xt : a.io.X;
        const double xv = live && l < D ? xsrc[kd + l] : 0.0;
        xs[l] = xv;
        // the gap terms of cutpoint parameter i = l - P (a NaN delta gives a NaN w: flagged below)
        const int i = l - P;
        if (i >= 0) {
            double w = 1.0, lmv = 0.0, qe = 0.0;
            if (i >= 1 && i < lc) {
                w = exp(xv);
                ord_gap(w, lmv, qe);
            }
            wv[i] = w;
            lm[i] = lmv;
            qv[i] = qe;
        }
    }
    __syncthreads();                          // the zeros are in place before any thread writes the first tile
    if (l == 0) {                             // the cutpoints as one chain in i
        double cut = xs[P];
        ct[0] = cut;
        for (int i = 1; i < lc; ++i) {
            cut += wv[i];
            ct[i] = cut;
        }
    }

    // the blocks of the upper triangle that this wave accumulates: block w + q NW in the order (0,0) (0,1) .. (0,nb-1) (1,1) ..
    const int wvi = l >> 6, ln = l & 63, cc = ln & 15, ks = ln >> 4, ntiles = nb * (nb + 1) / 2;
    int ti[MAXT], tj[MAXT];
    v4d acc[MAXT];
#pragma unroll
    for (int q = 0; q < MAXT; ++q) {
        int tt = wvi + q * NW, bi = 0;
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
        if (ti[q] >= P) ti[q] = -1;           // a block whose rows are all cutpoint parameters: not used
        acc[q] = v4d{0.0, 0.0, 0.0, 0.0};
    }
    // the tile elements e = l + q NT of this thread as (row, column) of the (32 x P) tile, stepped without a division
    const int row0 = l / P, col0 = l - row0 * P, dr = NT / P, dc = NT - dr * P;
    const int en = l / NG, eg = l % NG;       // the eta pass: row en of the tile, columns eg, eg + NG, ..

    double pre[OL_AQ], opre = 0.0;
    int ypre = 0;
    {
        const int tnv = (int)(nk < LB_TN ? nk : LB_TN), te = tnv * P;
#pragma unroll
        for (int q = 0; q < OL_AQ; ++q) {
            const int e = l + q * NT;
            pre[q] = e < te ? Ak[e] : 0.0;
        }
        if (l < tnv) {
            ypre = yk[l];
            if (OFF) opre = ok_[l];
        }
    }
    double gacc = 0.0, facc = 0.0, Facc = 0.0, Sacc = 0.0, cnt = 0.0;
    const int ci = l - P;                     // the cutpoint parameter of thread P + i

    for (long long n0 = 0; n0 < N; n0 += LB_TN) {
        const long long left = nk - n0;
        const int tnv = left < 0 ? 0 : (int)(left < LB_TN ? left : LB_TN);
        // a tile without a row that counts (past n_k; every tile of a frozen slot) does none of the work below: it only runs
        // the barriers, which must stay uniform across the slots of a workgroup (tnv is uniform in the slot)
        if (tnv > 0) {                        // registers -> LDS: the whole tile, zeros in the rows that do not count
            int r = row0, c = col0;
#pragma unroll
            for (int q = 0; q < OL_AQ; ++q) {
                if (l + q * NT < LB_TN * P) As[r * lda + c] = pre[q];
                r += dr;
                c += dc;
                if (c >= P) {
                    c -= P;
                    ++r;
                }
            }
            if (l < LB_TN) {
                Ys[l] = (double)(ypre < 0 ? 0 : (ypre > lc ? lc : ypre));
                Os[l] = opre;
            }
        }
        __syncthreads();                      // (the first one also publishes the cutpoints)
        {                                     // the next tile's loads: in flight while this one is consumed
            const long long left2 = left - LB_TN;
            const int tnv2 = left2 < 0 ? 0 : (int)(left2 < LB_TN ? left2 : LB_TN), te2 = tnv2 * P;
            const double* An = Ak + (size_t)(n0 + LB_TN) * P;
#pragma unroll
            for (int q = 0; q < OL_AQ; ++q) {
                const int e = l + q * NT;
                pre[q] = e < te2 ? An[e] : 0.0;
            }
            ypre = 0;
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
                const bool on = en < tnv;
                double re = 0.0, sb = 0.0, fab = 0.0, fb = 0.0, tt = 0.0;
                if (on) ord_link_curv<STEP>(eta, (int)Ys[en], C, ct, lm, re, sb, fab, fb, tt);
                Rs[en] = re;
                Sb[en] = sb;
                Wf[en] = fab;
                Wb[en] = fb;
                if (STEP) Ts[en] = tt;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < MAXT; ++q) {
            if (ti[q] >= 0 && tnv > 0) {      // (wave-uniform)
                const int j = tj[q] + cc, jc = j - P;
                const double* pa = As + ks * lda + ti[q] + cc;
                const double* pb = As + ks * lda + (jc < 0 ? j : 0);
#pragma unroll
                for (int st = 0; st < LB_TN / 4; ++st) {
                    const int n = ks + 4 * st;
                    const double av = pa[4 * st * lda], fab = Wf[n];
                    double bv;
                    if (jc < 0) {
                        bv = fab * pb[4 * st * lda];
                    } else {                  // -e_ni from the row's cells and its label
                        const int yn = (int)Ys[n];
                        bv = -(jc < yn ? fab : (jc == yn ? Wb[n] : 0.0));
                    }
                    acc[q] = GSMVI_MFMA_F64(av, bv, acc[q]);
                }
            }
        }
        if (l < D) {
            if (ci < 0) {
                if (STEP)
                    for (int n = 0; n < tnv; ++n) gacc = fma(Rs[n], As[n * lda + l], gacc);
            } else {
                for (int n = 0; n < tnv; ++n) {
                    const int yn = (int)Ys[n];
                    const bool below = ci < yn, at = ci == yn;
                    Facc += below ? Wf[n] : (at ? Wb[n] : 0.0);
                    Sacc += below ? -Rs[n] : (at ? Sb[n] : 0.0);
                    cnt += at ? 1.0 : 0.0;
                }
            }
        }
        if (STEP && l == NT - 1)
            for (int n = 0; n < tnv; ++n) facc += Ts[n];
        __syncthreads();                      // the next tile overwrites As, Ys, Os and the per-row results
    }

    // the upper triangle of the product -> LDS; F, the chain terms, g and f of phi = -lp
#pragma unroll
    for (int q = 0; q < MAXT; ++q) {
        if (ti[q] >= 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ti[q] + ks + 4 * r, j = tj[q] + cc;
                if (i <= j && j < D && i < P) Hs[i * ldh + j] = acc[q][r];
            }
        }
    }
    double dterm = 0.0;                       // thread P + i: what the diagonal gets beside w_i^2 F(i)
    if (l < D && ci >= 0) {
        const double w = wv[ci], qe = qv[ci], wq = w * qe;
        const bool gapc = ci >= 1;            // (q_0 = 0: cutpoint 0 has no gap term and no chain term)
        const double Sv = gapc ? Sacc + qe * cnt : Sacc;
        const double c = gapc ? -(w * Sv) : 0.0;
        Fv[ci] = Facc;
        cv[ci] = c;
        dterm = (gapc ? (wq * (w + wq)) * cnt : 0.0) + c + kap;
        if (STEP) gs[l] = -(w * Sv - kap * xs[l]);
    }
    if (STEP) {
        if (l < P) gs[l] = -(gacc - lam * xs[l]);
        else if (l >= D && l < Dp) gs[l] = 0.0;
        if (l == NT - 1) {
            double bb = 0.0, dd = 0.0;
            for (int j = 0; j < P; ++j) bb += xs[j] * xs[j];
            for (int j = P; j < D; ++j) dd += xs[j] * xs[j];
            cell[1] = -((facc - 0.5 * lam * bb) - 0.5 * kap * dd);
        }
    }
    __syncthreads();
    // the epilogue on the upper triangle: the w_i scalings of the border block, the delta-delta block, the priors, then dg
#pragma unroll
    for (int q = 0; q < MAXE; ++q) {
        const int e = l + q * NT;
        if (e < DD) {
            const int i = e / D, j = e - i * D;
            if (j >= P && i < j) {
                const int jc = j - P;
                Hs[i * ldh + j] = i < P ? wv[jc] * Hs[i * ldh + j] : wv[i - P] * (wv[jc] * Fv[jc]);
            }
        }
    }
    if (l < D) {
        const double v = ci < 0 ? Hs[l * ldh + l] + lam : wv[ci] * (wv[ci] * Fv[ci]) + dterm;
        Hs[l * ldh + l] = v;
        dg[l] = v;
    }
    __syncthreads();
    // a non-finite x or a gap that is not a positive normal number (uniform in the slot: every wave forms it from the same numbers)
    const double wl = ln >= 1 && ln < lc ? wv[ln] : 1.0;
    const bool bad = !(gb_wave_sum(ln < D ? xs[ln] * 0.0 : 0.0) == 0.0) ||
                     !__all(wl >= 2.2250738585072014e-308 && wl < __builtin_huge_val());

    lp_verdict v;
    bool need;
    if (STEP) {
        lp_step_test(a.io, live, bad, D, ln, gs, cell, s, v);
        need = v.need;
        if (need) {                           // the strict upper triangle into the free lower one: what a retry restores
#pragma unroll
            for (int q = 0; q < MAXE; ++q) {
                const int e = l + q * NT;
                if (e < DD) {
                    const int i = e / D, j = e - i * D;
                    if (i < j) Hs[j * ldh + i] = Hs[i * ldh + j];
                }
            }
        }
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
    // the retry rule (every thread of the slot reads the same cells of LDS, so `retry` is uniform in it)
    bool retry = false;
    if (need && info != 0)
        for (int i = 1; i < lc; ++i) retry = retry || cv[i] < 0.0;
    if (__syncthreads_or(retry)) {            // (uniform in the workgroup: every slot runs the second factorisation's barriers)
        if (retry) {
#pragma unroll
            for (int q = 0; q < MAXE; ++q) {
                const int e = l + q * NT;
                if (e < DD) {
                    const int i = e / D, j = e - i * D;
                    if (i < j) Hs[i * ldh + j] = Hs[j * ldh + i];
                }
            }
            if (l < D) {
                const double c = ci >= 1 ? cv[ci] : 0.0, dv = dg[l] - (c < 0.0 ? c : 0.0);
                Hs[l * ldh + l] = dv;
                dg[l] = dv;
            }
        }
        __syncthreads();
        const int info2 = lp_chol_lds<NT, MAXE>(retry, D, l, ldh, Hs, pv, dg);
        if (retry) {
            info = info2;
            retry = info2 == 0;               // from here: the round's direction comes from the retried matrix
        }
    }
    if (!live || l >= 64) return;             // the rest is the first wave's: component l of every vector in lane l
    lp_step_tail(a.io, s, v, info, kd, D, l, ldh, Hs, pv, xs, sc, is);
    if (retry && l == 0) is[OL_MOD] = (a.io.start ? 0 : is[OL_MOD]) + 1;  // (after the tail's own writes of the state words)
}

template <int MODE>
static int ol_go(gsmvi_ctx* ctx, void* stream, const ol_args& a) {
    int ppw;
    unsigned grid;
    const int D = a.P + a.C - 1;
    const size_t lds = lp_slot_launch(a.K, D, ol_lds_doubles(D), 0, &ppw, &grid);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (ppw == 4) {
        if (a.offset) hipLaunchKernelGGL((k_ordinal_laplace_batched<64, true, MODE>), dim3(grid), dim3(256), lds, st, a);
        else hipLaunchKernelGGL((k_ordinal_laplace_batched<64, false, MODE>), dim3(grid), dim3(256), lds, st, a);
    } else {
        if (a.offset) hipLaunchKernelGGL((k_ordinal_laplace_batched<256, true, MODE>), dim3(grid), dim3(256), lds, st, a);
        else hipLaunchKernelGGL((k_ordinal_laplace_batched<256, false, MODE>), dim3(grid), dim3(256), lds, st, a);
    }
    // the pair of bits is shared with k_laplace_shared_batched and k_negbin_laplace_batched (include/gsmvi_hip.h): no new bit is
    // left to take
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LAPLACE | GSMVI_PATH_BATCHED_TARGET, "k_ordinal_laplace_batched");
}

static ol_args ol_args_of(int64_t K, int P, int C, int64_t N, const double* A, const int* y, const double* offset,
                          const int* counts_dev, double prior_prec, const double* prior_prec_dev, double cut_prec,
                          const double* cut_prec_dev, const lp_io& io) {
    return {K, N, P, C, A, y, offset, counts_dev, prior_prec, prior_prec_dev, cut_prec, cut_prec_dev, io};
}

// the model's checks of both entry points, those of gsmvi_ordinal_batched_f64 at nc = 1
static int ol_check_model(const char* fn, const ol_args& a) {
#define OL_BAD(cond, msg) \
    if (cond) return gb_bad(fn, msg)
    OL_BAD(a.C < 2 || a.C > GB_MAX_D, "C must be in [2, 64]");
    OL_BAD(a.P < 1 || a.P > GB_MAX_D - (a.C - 1), "P must be in [1, 65 - C] (D = P + C - 1 <= 64)");
    if (int st = gb_check_shape(fn, a.K, a.P + a.C - 1, gb_ppw)) return st;
    OL_BAD(a.N < 1, "N must be at least 1");
    OL_BAD(a.N > (INT64_MAX / 8 / a.P) / a.K, "K N P is too large");
    OL_BAD(!a.lam_dev && !(a.lam >= 0.0 && a.lam < __builtin_huge_val()), "prior_prec must be finite and >= 0");
    OL_BAD(!a.kap_dev && !(a.kap >= 0.0 && a.kap < __builtin_huge_val()), "cut_prec must be finite and >= 0");
    OL_BAD(!a.A || !a.y, "NULL array");
#undef OL_BAD
    return GSMVI_OK;
}

// gb_check_overlaps over the model's six read-only arrays followed by the entry point's own, which stand at own + 6
template <size_t NOWN>
static int ol_check_overlaps(const char* fn, const ol_args& a, gb_arr (&own)[NOWN]) {
    const size_t nn = (size_t)a.K * a.N, nkb = (size_t)a.K * 8;
    const gb_arr model[6] = {{a.A, nn * a.P * 8, "A", GB_RD},          {a.y, nn * 4, "y", GB_RD},
                             {a.offset, nn * 8, "offset", GB_RD},      {a.counts, (size_t)a.K * 4, "counts_dev", GB_RD},
                             {a.lam_dev, nkb, "prior_prec_dev", GB_RD}, {a.kap_dev, nkb, "cut_prec_dev", GB_RD}};
    for (int i = 0; i < 6; ++i) own[i] = model[i];
    return gb_check_overlaps(fn, own, own + NOWN);
}

extern "C" {

int gsmvi_ordinal_hessian_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int C, int64_t N, const double* A,
                                      const int* y, const double* offset, const int* counts_dev, double prior_prec,
                                      const double* prior_prec_dev, double cut_prec, const double* cut_prec_dev, const double* X,
                                      double* H, double* cov, int* info_dev) {
    const ol_args a = ol_args_of(K, P, C, N, A, y, offset, counts_dev, prior_prec, prior_prec_dev, cut_prec, cut_prec_dev,
                                 lp_hess_io(X, H, cov, info_dev));
    if (int st = ol_check_model(__func__, a)) return st;
    if (int st = lp_check_hess(__func__, a.io)) return st;
    gb_arr own[6 + LP_HESS_ROWS];
    lp_hess_rows(own + 6, K, P + C - 1, a.io);
    if (int st = ol_check_overlaps(__func__, a, own)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    return ol_go<LP_HESS>(ctx, stream, a);
}

int gsmvi_ordinal_laplace_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int C, int64_t N, const double* A,
                                           const int* y, const double* offset, const int* counts_dev, double prior_prec,
                                           const double* prior_prec_dev, double cut_prec, const double* cut_prec_dev, int start,
                                           double* x, double* g, double* d, double* sc, int* ist, double* Xt, int* stopped_dev,
                                           int maxiter, int maxfun, double gtol) {
    const ol_args a = ol_args_of(K, P, C, N, A, y, offset, counts_dev, prior_prec, prior_prec_dev, cut_prec, cut_prec_dev,
                                 lp_step_io(start, x, g, d, sc, ist, Xt, stopped_dev, maxiter, maxfun, gtol));
    if (int st = ol_check_model(__func__, a)) return st;
    if (int st = lp_check_step(__func__, a.io)) return st;
    gb_arr own[6 + LP_STEP_ROWS];
    lp_step_rows(own + 6, K, P + C - 1, a.io);
    if (int st = ol_check_overlaps(__func__, a, own)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    return ol_go<LP_STEP>(ctx, stream, a);
}

// include/gsmvi_hip_debug.h: what a launch of either entry point at D = P + C - 1 requests (exported by the debug library only)
int gsmvi_debug_ordinal_laplace_lds(int D, size_t* bytes, int* problems_per_workgroup) {
    GB_BAD(D < 2 || D > GB_MAX_D || !bytes || !problems_per_workgroup, "bad shape or NULL output");
    unsigned grid;
    *bytes = lp_slot_launch(1, D, ol_lds_doubles(D), 0, problems_per_workgroup, &grid);
    return GSMVI_OK;
}

}  // extern "C"
