// Batched softmax Laplace initialiser: the negative Hessian of K multinomial logit posteriors of one (N, C, P), D = (C - 1) P <= 64,
// its inverse, and one damped Newton round per launch for every running problem ("Batched softmax Laplace
// initialiser").
//
// The reference has no Laplace initialiser: it starts its fits from the L-BFGS-B maximiser of lp and the optimiser's dense
// inverse-Hessian estimate (gsmvi/initializers.py:5-17), for a model given as log_prob and jit(grad(...)) of it
// (examples/example_gsm.py:34-35).  For the model of gsmvi_softmax_batched.hip (class C - 1 the reference class with eta = 0,
// x[c P + j] = W_cj, m_n = max_c eta_nc, s_n = sum_c exp(eta_nc - m_n), p_nc = exp(eta_nc - m_n) / s_n) the second derivative is
// closed-form: for d = c P + i, d' = c' P + j, c, c' < C - 1,
//   H_k(x)[d, d'] = sum_{n < n_k} w_n,cc' a_ni a_nj + lam_k [d = d'],   w_n,cc = p_nc (1 - p_nc),   w_n,cc' = -p_nc p_nc'  (c != c')
// (the negative Hessian of lp_k: positive semi-definite), and the Newton direction of phi = -lp is d = -H^{-1} g, g = -score.
//   k_softmax_laplace_batched<NT, LP_HESS> : H_k at the rows of X, cov_k = H_k^{-1} and info_k
//   k_softmax_laplace_batched<NT, LP_STEP> : f, g and H at the trial point Xt_k in ONE sweep over A_k, then the round's decision
// 1 - p is a sum over the other classes, never 1.0 - p and never a difference of two Gram sums (a saturated class would lose every
// digit of its diagonal block): with c* the first class that attains m (e_c* = 1 exactly), s_rest = sum_{c != c*} e_c and
// s = 1 + s_rest,   1 - p_c* = s_rest / s,   1 - p_c = (s - e_c) / s  (c != c*; s - e_c >= 1).  The reference class takes part in m, s
// and s_rest like any other (it is the last candidate for c*).  The residual is r_nc = 1 - p_nc in that form where y_n = c and
// -p_nc elsewhere; the density's term is eta_n,y_n - m_n - log s_n with log s_n as log1p(s_rest) (sm_log_s of gsmvi_softmax_model.h:
// log(s_n) is 0 where s_rest < eps / 2).
// Work mapping: the slots of gsmvi_batched.h (gb_nt(D) threads per problem, four problems -- one wave each -- per 256-thread
// workgroup for D <= 16).  A slot walks the rows of A_k in tiles of SL_TN = 32 (row stride P | 1, all 32 rows written, zeros in the
// rows that do not count); the next tile's loads are in flight while the current one is consumed.  Per tile: NT / 32 adjacent lanes
// share a row; lane eg of them takes the classes eg, eg + NT / 32, .. (at most eight) and forms their dots of length P into its own
// cells of Pb; m, c*, s_rest and eta_y come from butterflies over the row's lanes; the lane leaves p and 1 - p of its classes in
// the two (C - 1) x 33 blocks Pb, Qb.  Then the Gram product runs on the fp64 MFMA (16 x 16 x 4).  delta_cc' does not depend on n, so the
// 16 x 16 block (bi, bj), bi <= bj, of H carries two accumulators over all of N,
//   G1 = sum_n u_nd t_nd',   G2 = sum_n u_nd u_nd',   u_nd = p_nc a_ni,   t_nd' = (1 - p_nc') a_nj,
// with the operands formed on the fly from the A tile and Pb, Qb (a lane's class and feature of its operand column are fixed for
// the whole sweep), and after the sweep entry (d, d') is G1 where c(d) = c(d') and -G2 elsewhere.  At most three blocks per wave
// (ten blocks of the upper triangle over four waves at 64 columns).  In step mode thread d < D sums g_d over the tile's rows in
// order and one thread sums the density's terms.
// After the sweep the upper triangle goes to LDS -- H aliases the tile and the two blocks, which are dead by then -- lam is added to
// the diagonal, and the rest is gsmvi_laplace_stage.h: H written mirrored (exactly symmetric), the Cholesky factorisation with the
// relative pivot rule 64 eps H_jj, then the inverse R^{-1} R^{-T} or the state machine of gsmvi_laplace_step_batched_f64.
// Order: every sum over n runs n = 0 .. n_k - 1 in tiles of 32, eight MFMA steps of four rows per tile; s_rest is summed per lane in
// class order, then by the butterfly; all of it depends on (N, C, P) alone, not on K, the slot packing or the neighbours.  Rows
// n >= n_k are never loaded.  A label is used in comparisons only, never as an index.  A non-finite x, or a non-finite valid eta,
// sets a flag: H = NaN, info = 1 and cov = I, or status 4 / a rejected trial.  A slot reads and writes only slice k of every array
// and every slot of a workgroup runs the same barriers; a problem whose status is not 0 is frozen (no loads, no per-tile work, no
// writes), and a workgroup all of whose problems are frozen leaves at once.  Inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_laplace_stage.h"
#include "gsmvi_softmax_model.h"
#include "../../include/gsmvi_hip.h"
#include "../../include/gsmvi_hip_debug.h"   // gsmvi_debug_softmax_laplace_lds
#include <cmath>
#include <cstdint>

#define SL_TN 32       // rows of A_k per tile
#define SL_AQ 8        // tile elements per thread: SL_TN P / NT <= 8 in both packings
#define SL_LDR 33      // row stride of Pb, Qb

struct sl_args {
    long long K, N;
    int C, P, D;
    const double* A;            // (K, N, P)
    const int* labels;          // (K, N)
    const int* counts;          // (K) valid rows, clamped to 0 .. N (null: N)
    double lam;                 // the prior precision of every problem ...
    const double* lam_dev;      // ... or (K) per-problem values on the device (null: `lam`)
    lp_io io;
};

__host__ __device__ inline int sl_dp(int D) { return ((D + 15) >> 4) << 4; }

// LDS doubles per problem: x, g, pivots, the diagonal of H and of R^{-1} (Dp each) and four cells, then one region that holds the
// A tile (32 x (P | 1)), its labels (ints in 32 doubles), the density's terms (32), Pb and Qb ((C - 1) x 33 each) during the sweep
// and H (D x (D | 1)) after it.  (C, P) = (2, 64): 4484 doubles, 35.0 KB; (65, 1): 4644, 36.3 KB; four problems of (17, 1): 38.6 KB
__host__ __device__ inline int sl_lds_doubles(int C, int P) {
    const int D = (C - 1) * P, Dp = sl_dp(D);
    const int sweep = SL_TN * (P | 1) + 2 * SL_TN + 2 * (C - 1) * SL_LDR, h = D * (D | 1);
    return 5 * Dp + 4 + (sweep > h ? sweep : h);
}

template <int NT, int MODE>
__global__ __launch_bounds__(256) void k_softmax_laplace_batched(sl_args a) {
    extern __shared__ double sl_sm[];
    constexpr int PPW = 256 / NT, NW = NT / 64, NG = NT / SL_TN;
    constexpr int MAXT = NT == 256 ? 3 : 1;       // 16 x 16 blocks of H per wave
    constexpr int MAXE = NT == 256 ? 16 : 4;      // entries of H per thread
    constexpr bool STEP = MODE == LP_STEP;
    const int P = a.P, Cm = a.C - 1, D = a.D, nb = (D + 15) >> 4, Dp = nb * 16, lda = P | 1, ldh = D | 1;
    const long long N = a.N;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;
    const size_t kk = (size_t)(valid ? k : 0), kd = kk * D;
    double* xs = sl_sm + (size_t)slot * sl_lds_doubles(a.C, P);   // Dp  the point (zeros beyond D)
    double* gs = xs + Dp;                     // Dp  g = -score there
    double* pv = gs + Dp;                     // Dp  pivots R_cc
    double* dg = pv + Dp;                     // Dp  the diagonal of H
    double* rd = dg + Dp;                     // Dp  the diagonal of R^{-1}
    double* cell = rd + Dp;                   // [0] NaN when a row is flagged, [1] f
    double* As = cell + 4;                    // 32 x lda          the sweep's region ...
    int* Ys = reinterpret_cast<int*>(As + SL_TN * lda);           // 32 labels (in 32 doubles)
    double* Ts = As + SL_TN * lda + SL_TN;    // 32                the density's terms
    double* Pb = Ts + SL_TN;                  // Cm x 33           p
    double* Qb = Pb + Cm * SL_LDR;            // Cm x 33           1 - p
    double* Hs = As;                          // D x ldh           ... and H after it
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

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
    const int* yk = a.labels + kk * (size_t)N;
    const sm_problem pk = sm_problem_of(a.counts, a.lam, a.lam_dev, N, k, live);
    const long long nk = pk.nk;               // the rows that count (a frozen slot: none, so nothing of A_k is loaded)
    const double lam = pk.lam;
    if (l < Dp) {
        const double* xsrc = STEP ? a.io.Xt : a.io.X;
        xs[l] = live && l < D ? xsrc[kd + l] : 0.0;
    }
    if (l == 0) cell[0] = 0.0;

    // the blocks of the upper triangle that this wave accumulates: block w + q NW in the order (0,0) (0,1) .. (0,nb-1) (1,1) ..;
    // the lane's operand columns 16 bi + cc and 16 bj + cc of a block as (offset of the class in Pb / Qb, feature), fixed for the sweep
    const int wv = l >> 6, ln = l & 63, cc = ln & 15, ks = ln >> 4, ntiles = nb * (nb + 1) / 2;
    int ti[MAXT], tj[MAXT], pa[MAXT], fa[MAXT], pb[MAXT], fb[MAXT];
    bool va[MAXT], vb[MAXT];
    v4d g1[MAXT], g2[MAXT];
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
        const int da = (ti[q] < 0 ? 0 : ti[q]) + cc, db = tj[q] + cc;
        va[q] = ti[q] >= 0 && da < D;
        vb[q] = ti[q] >= 0 && db < D;
        const int ca = va[q] ? da / P : 0, cb = vb[q] ? db / P : 0;
        pa[q] = ca * SL_LDR;
        fa[q] = va[q] ? da - ca * P : 0;
        pb[q] = cb * SL_LDR;
        fb[q] = vb[q] ? db - cb * P : 0;
        g1[q] = v4d{0.0, 0.0, 0.0, 0.0};
        g2[q] = v4d{0.0, 0.0, 0.0, 0.0};
    }
    // the tile elements e = l + q NT of this thread as (row, column), stepped without a division
    const int row0 = l / P, col0 = l - row0 * P, dr = NT / P, dc = NT - dr * P;
    const int en = l / NG, eg = l % NG;       // the row pass: row en of the tile, classes eg, eg + NG, ..
    const int gc = l < D ? l / P : 0, gf = l < D ? l - gc * P : 0;      // the g pass: class and feature of component l

    double pre[SL_AQ];
    int ypre = 0;
    {
        const int tnv = (int)(nk < SL_TN ? nk : SL_TN), te = tnv * P;
#pragma unroll
        for (int q = 0; q < SL_AQ; ++q) {
            const int e = l + q * NT;
            pre[q] = e < te ? Ak[e] : 0.0;
        }
        if (l < tnv) ypre = yk[l];
    }
    double gacc = 0.0, facc = 0.0;
    __syncthreads();                          // xs and cell[0] are in place

    for (long long n0 = 0; n0 < N; n0 += SL_TN) {
        const long long left = nk - n0;
        const int tnv = left < 0 ? 0 : (int)(left < SL_TN ? left : SL_TN);
        // a tile without a row that counts (past n_k; every tile of a frozen slot) does none of the work below: it only runs
        // the barriers, which must stay uniform across the slots of a workgroup (tnv is uniform in the slot)
        if (tnv > 0) {                        // registers -> LDS: the whole tile, zeros in the rows that do not count
            int r = row0, c = col0;
#pragma unroll
            for (int q = 0; q < SL_AQ; ++q) {
                if (l + q * NT < SL_TN * P) As[r * lda + c] = pre[q];
                r += dr;
                c += dc;
                if (c >= P) {
                    c -= P;
                    ++r;
                }
            }
            if (l < SL_TN) Ys[l] = ypre;
        }
        __syncthreads();
        {                                     // the next tile's loads: in flight while this one is consumed
            const long long left2 = left - SL_TN;
            const int tnv2 = left2 < 0 ? 0 : (int)(left2 < SL_TN ? left2 : SL_TN), te2 = tnv2 * P;
            const double* An = Ak + (size_t)(n0 + SL_TN) * P;
#pragma unroll
            for (int q = 0; q < SL_AQ; ++q) {
                const int e = l + q * NT;
                pre[q] = e < te2 ? An[e] : 0.0;
            }
            ypre = 0;
            if (l < tnv2) ypre = yk[n0 + SL_TN + l];
        }
        if (tnv > 0) {                        // row en: the dots of this lane's classes, then m, c*, s_rest, eta_y over the row's lanes
            const double* ar = As + en * lda;
            const int yv = Ys[en];
            double* pr = Pb + en;             // this lane's cells of Pb hold eta, then e, then p of its classes
            double m = -__builtin_huge_val(), etay = 0.0;
            int cs = 0x7fffffff;
            bool fine = true;
#pragma unroll 1
            for (int c = eg; c < Cm; c += NG) {
                const double* xc = xs + c * P;
                double eta = 0.0;
#pragma unroll 4
                for (int j = 0; j < P; ++j) eta = fma(ar[j], xc[j], eta);
                pr[c * SL_LDR] = eta;
                fine = fine && gb_finite(eta);
                if (eta > m) {                // (strict: the first class that attains the maximum)
                    m = eta;
                    cs = c;
                }
                etay = c == yv ? eta : etay;
            }
#pragma unroll
            for (int o = NG / 2; o > 0; o >>= 1) {
                const double om = __shfl_xor(m, o);
                const int oc = __shfl_xor(cs, o);
                const bool take = om > m || (om == m && oc < cs);
                m = take ? om : m;
                cs = take ? oc : cs;
                etay += __shfl_xor(etay, o);  // (one lane's term is not zero)
                fine = __shfl_xor((int)fine, o) != 0 && fine;
            }
            if (m < 0.0) {                    // the reference class, eta = 0: the last candidate
                m = 0.0;
                cs = Cm;
            }
            double rest = 0.0;
#pragma unroll 1
            for (int c = eg; c < Cm; c += NG) {
                const double e = c == cs ? 1.0 : exp(pr[c * SL_LDR] - m);
                pr[c * SL_LDR] = e;
                rest += c == cs ? 0.0 : e;
            }
#pragma unroll
            for (int o = NG / 2; o > 0; o >>= 1) rest += __shfl_xor(rest, o);
            if (cs != Cm) rest += exp(0.0 - m);
            const double sn = 1.0 + rest;
            const bool on = en < tnv;
#pragma unroll 1
            for (int c = eg; c < Cm; c += NG) {
                const double e = pr[c * SL_LDR];
                pr[c * SL_LDR] = on ? e / sn : 0.0;
                Qb[c * SL_LDR + en] = on ? (c == cs ? rest : sn - e) / sn : 0.0;
            }
            if (eg == 0) {
                if (STEP) Ts[en] = on ? etay - m - sm_log_s(rest, sn) : 0.0;
                if (on && !fine) cell[0] = qnan;      // (any number of threads, the same value)
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < MAXT; ++q) {
            if (ti[q] >= 0 && tnv > 0) {      // (wave-uniform)
                const double* ra = As + ks * lda + fa[q];
                const double* rb = As + ks * lda + fb[q];
                const double* ppa = Pb + pa[q] + ks;
                const double* ppb = Pb + pb[q] + ks;
                const double* pqb = Qb + pb[q] + ks;
#pragma unroll
                for (int st = 0; st < SL_TN / 4; ++st) {
                    const double aa = ra[4 * st * lda], ab = rb[4 * st * lda];
                    const double u = va[q] ? ppa[4 * st] * aa : 0.0;
                    const double ub = vb[q] ? ppb[4 * st] * ab : 0.0;
                    const double tb = vb[q] ? pqb[4 * st] * ab : 0.0;
                    g1[q] = GSMVI_MFMA_F64(u, tb, g1[q]);
                    g2[q] = GSMVI_MFMA_F64(u, ub, g2[q]);
                }
            }
        }
        if (STEP) {
            if (l < D)
                for (int n = 0; n < tnv; ++n) {
                    const double r = Ys[n] == gc ? Qb[gc * SL_LDR + n] : -Pb[gc * SL_LDR + n];
                    gacc = fma(r, As[n * lda + gf], gacc);
                }
            if (l == NT - 1)
                for (int n = 0; n < tnv; ++n) facc += Ts[n];
        }
        __syncthreads();                      // the next tile overwrites As, Ys, Ts, Pb, Qb; after the last one H does
    }

    // the upper triangle of H -> LDS (G1 within a class, -G2 across classes), g and f of phi = -lp
#pragma unroll
    for (int q = 0; q < MAXT; ++q) {
        if (ti[q] >= 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ti[q] + ks + 4 * r, j = tj[q] + cc;
                if (i <= j && j < D) Hs[i * ldh + j] = i / P == j / P ? g1[q][r] : -g2[q][r];
            }
        }
    }
    if (STEP) {
        if (l < Dp) gs[l] = l < D ? -(gacc - lam * xs[l]) : 0.0;
        if (l == NT - 1) {
            double xx = 0.0;
            for (int j = 0; j < D; ++j) xx += xs[j] * xs[j];
            cell[1] = -(facc - 0.5 * lam * xx);
        }
    }
    __syncthreads();
    if (l < D) {
        const double v = Hs[l * ldh + l] + lam;
        Hs[l * ldh + l] = v;
        dg[l] = v;
    }
    __syncthreads();
    // a non-finite x or a flagged row (uniform in the slot: every wave forms it from the same numbers)
    const bool bad = !(gb_wave_sum(ln < D ? xs[ln] * 0.0 : 0.0) == 0.0) || !(cell[0] == 0.0);

    lp_verdict v;
    bool need;
    if (STEP) {
        lp_step_test(a.io, live, bad, D, ln, gs, cell, s, v);
        need = v.need;
    } else {
        need = live && !bad && a.io.cov != nullptr;
        lp_write_h<NT, MAXE>(a.io, live, bad, kk, D, l, ldh, Hs);
    }

    const int info = lp_chol_lds<NT, MAXE>(need, D, l, ldh, Hs, pv, dg);     // (its last barrier publishes R and the pivots)

    if (!STEP) {
        if (!a.io.cov) return;                   // (uniform)
        lp_inverse_tail<NT, MAXE>(a.io, live, bad, need, info, k, kk, D, l, ldh, Hs, pv, rd);
        return;
    }
    if (!live || l >= 64) return;             // the rest is the first wave's: component l of every vector in lane l
    lp_step_tail(a.io, s, v, info, kd, D, l, ldh, Hs, pv, xs, sc, is);
}

template <int MODE>
static int sl_go(gsmvi_ctx* ctx, void* stream, const sl_args& a) {
    int ppw;
    unsigned grid;
    const size_t lds = lp_slot_launch(a.K, a.D, sl_lds_doubles(a.C, a.P), 0, &ppw, &grid);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (ppw == 4)
        hipLaunchKernelGGL((k_softmax_laplace_batched<64, MODE>), dim3(grid), dim3(256), lds, st, a);
    else
        hipLaunchKernelGGL((k_softmax_laplace_batched<256, MODE>), dim3(grid), dim3(256), lds, st, a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_SOFTMAX_LAPLACE, "k_softmax_laplace_batched");
}

extern "C" {

int gsmvi_softmax_hessian_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int C, int P, int64_t N, const double* A,
                                      const int* labels, const int* counts_dev, double prior_prec, const double* prior_prec_dev,
                                      const double* X, double* H, double* cov, int* info_dev) {
    const sm_model m = sm_model_of(K, N, C, P, A, labels, counts_dev, prior_prec, prior_prec_dev);
    if (int st = sm_check_model(__func__, m, true, "N")) return st;
    const sl_args a = {K, N, C, P, m.D, A, labels, counts_dev, prior_prec, prior_prec_dev, lp_hess_io(X, H, cov, info_dev)};
    GB_BAD(!A || !labels, "NULL array");
    if (int st = lp_check_hess(__func__, a.io)) return st;
    gb_arr own[LP_HESS_ROWS];
    lp_hess_rows(own, K, m.D, a.io);
    if (int st = gb_check_overlaps(__func__, m, own)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    return sl_go<LP_HESS>(ctx, stream, a);
}

int gsmvi_softmax_laplace_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int C, int P, int64_t N, const double* A,
                                           const int* labels, const int* counts_dev, double prior_prec,
                                           const double* prior_prec_dev, int start, double* x, double* g, double* d, double* sc,
                                           int* ist, double* Xt, int* stopped_dev, int maxiter, int maxfun, double gtol) {
    const sm_model m = sm_model_of(K, N, C, P, A, labels, counts_dev, prior_prec, prior_prec_dev);
    if (int st = sm_check_model(__func__, m, true, "N")) return st;
    const sl_args a = {K, N, C, P, m.D, A, labels, counts_dev, prior_prec, prior_prec_dev,
                       lp_step_io(start, x, g, d, sc, ist, Xt, stopped_dev, maxiter, maxfun, gtol)};
    GB_BAD(!A || !labels, "NULL array");
    if (int st = lp_check_step(__func__, a.io)) return st;
    gb_arr own[LP_STEP_ROWS];
    lp_step_rows(own, K, m.D, a.io);
    if (int st = gb_check_overlaps(__func__, m, own)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    return sl_go<LP_STEP>(ctx, stream, a);
}

// include/gsmvi_hip_debug.h: what a launch at (C, P) requests (exported by the debug library only)
int gsmvi_debug_softmax_laplace_lds(int C, int P, size_t* bytes, int* problems_per_workgroup) {
    GB_BAD(!sm_shape_ok(C, P) || !bytes || !problems_per_workgroup, "bad shape or NULL output");
    unsigned grid;
    *bytes = lp_slot_launch(1, (C - 1) * P, sl_lds_doubles(C, P), 0, problems_per_workgroup, &grid);
    return GSMVI_OK;
}

}  // extern "C"
