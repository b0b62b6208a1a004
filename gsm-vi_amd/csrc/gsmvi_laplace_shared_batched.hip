// Shared-design Laplace initialiser: the negative Hessian of K GLM posteriors over ONE design matrix A (N, D), D <= 64, with
// observation weights, its inverse, and one damped Newton (IRLS) round per launch for every running problem (DESIGN.md section 9,
// "Shared-design Laplace initialiser").
//
// The reference has no Laplace initialiser: it starts its fits from the L-BFGS-B maximiser of lp and the optimiser's dense
// inverse-Hessian estimate (gsmvi/initializers.py:5-17), for a model given as log_prob and jit(grad(...)) of it
// (examples/example_gsm.py:34-35).  For the model of gsmvi_glm_shared_batched_f64 (problem k: responses y_k, offsets o_k, observation
// weights v_k >= 0, precisions lam_k, tau_k; every problem the rows a_n of the same A) the second derivative is closed-form: with
// eta_n = a_n . x + o_kn, the link (r, t) = lb_link<FAM> and the weight w = lb_weight<FAM> = -dr / d eta of gsmvi_glm_link.h,
//   f_k(x) = -( sum_n v_kn t(eta_n, y_kn) - lam_k |x|^2 / 2 )
//   g_k(x) = -( sum_n v_kn r(eta_n, y_kn) a_n - lam_k x )
//   H_k(x) =    sum_n v_kn w(eta_n, y_kn) a_n a_n^T + lam_k I          (positive semi-definite: v >= 0)
//   k_laplace_shared_batched<NT, FAM, LP_HESS> : H_k at the rows of X, cov_k = H_k^{-1} and info_k
//   k_laplace_shared_batched<NT, FAM, LP_STEP> : f, g and H at the trial point Xt_k in ONE sweep over A, then the round's decision
// Work mapping: the slots of gsmvi_batched.h (gb_nt(D) threads per problem, four problems -- one wave each -- per 256-thread
// workgroup for D <= 16), the per-slot form of k_laplace_batched, with ONE tile of A per workgroup: all 256 threads stage the rows
// n0 .. n0 + 31 of A in LDS once (zero-padded to Dp = 16 ceil(D / 16) columns, row stride Dp + 1, and to 32 rows; the next tile's
// loads are in flight while the current one is consumed) and every slot of the workgroup reads that one copy.  A is never held
// per problem, in device memory or in LDS.  Per tile a slot stages y, o and v of its own 32 observations; NT / 32 adjacent lanes
// share a row's eta (a butterfly over them), one of them applies the link and leaves v r, v t, v w of the row in the slot's LDS;
// then the Gram product runs on the fp64 MFMA (16 x 16 x 4): for the 16 x 16 block (bi, bj), bi <= bj, of H the A operand is
// (v w)_n a_{n, 16 bi + c} and the B operand a_{n, 16 bj + c}, eight steps per tile, the accumulators (at most three blocks per
// wave) in registers across all of N.  Thread j < D of a slot sums g_j over the tile's rows in order, one thread sums f.
// After the sweep the upper triangle goes to the slot's LDS, lam is added to the diagonal, and the rest is gsmvi_laplace_stage.h:
// H written mirrored (exactly symmetric), the Cholesky factorisation with the relative pivot rule 64 eps H_jj, then the inverse
// R^{-1} R^{-T} or the state machine of gsmvi_laplace_step_batched_f64.
// Order: every sum over n runs n = 0 .. N - 1 in tiles of 32, eight MFMA steps of four rows per tile; it depends on (N, D) alone,
// not on K, the slot, the workgroup's other problems or the weights.  No atomics but the *stopped_dev counter.
// Selection: an observation whose weight is not > 0 (0, NaN), like a row n >= N of the last tile, gets v r = v t = v w = 0 by a
// select, whatever y, o and eta hold there (a NaN y, an infinite offset, an e^eta that overflows), and flags nothing; weights =
// NULL is v = 1, and v w = w then exactly.  A non-finite x, or a poisson e^eta that is not finite at a v > 0 observation, sets the
// slot's flag: H = NaN, info = 1 and cov = I, or status 4 / a rejected trial.  A slot writes only slice k of every array and its own
// LDS; A is shared, so a non-finite entry of A reaches every problem.  A problem whose status is not 0 is frozen: its slot loads
// nothing of y, o, v, does none of the per-tile work and writes nothing; its threads still help to stage the workgroup's tile (a
// tile is staged when any problem of the workgroup runs) and run the barriers, which are uniform across the workgroup.  A
// workgroup all of whose problems are frozen leaves after reading the status words.  Inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_laplace_stage.h"
#include "gsmvi_glm_model.h"                 // glm_check_model, glm_dp, glm_for_family; gsmvi_glm_link.h: lb_link, lb_weight
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

#define LS_TN 32       // rows of A per tile
#define LS_AQ 8        // tile elements per thread: LS_TN D / 256 <= 8

struct ls_args {
    long long K, N;
    int D;
    const double* A;            // (N, D), shared
    const double* y;            // (K, N)
    const double* offset;       // (K, N) added to eta, or null
    const double* w;            // (K, N) observation weights, or null (1 everywhere)
    double lam;                 // the prior precision of every problem ...
    const double* lam_dev;      // ... or (K) per-problem values on the device (null: `lam`)
    double tau;                 // gaussian family: the noise precision of every problem ...
    const double* tau_dev;      // ... or (K) per-problem values on the device (null: `tau`)
    lp_io io;
};

// LDS doubles of the workgroup's one tile of A (32 x (Dp + 1)) and of one problem: y, o, v, v r, v w, v t of its rows (32 each), x,
// g, pivots, the diagonal of H and of R^{-1} (Dp each), four cells, H (D x (D | 1)).  D = 64: 2080 + 4676 doubles, 52.8 KB; four
// problems of D = 16: 528 + 4 x 548 doubles, 21.3 KB
__host__ __device__ inline int ls_tile_doubles(int D) { return LS_TN * (glm_dp(D) + 1); }
__host__ __device__ inline int ls_slot_doubles(int D) { return 6 * LS_TN + 5 * glm_dp(D) + 4 + D * (D | 1); }

template <int NT, int FAM, int MODE>
__global__ __launch_bounds__(256) void k_laplace_shared_batched(ls_args a) {
    extern __shared__ double ls_sm[];
    constexpr int PPW = 256 / NT, NW = NT / 64, NG = NT / LS_TN;
    constexpr int MAXT = NT == 256 ? 3 : 1;       // 16 x 16 blocks of H per wave
    constexpr int MAXE = NT == 256 ? 16 : 4;      // entries of H per thread
    constexpr bool STEP = MODE == LP_STEP;
    const int D = a.D, nb = (D + 15) >> 4, Dp = nb * 16, lda = Dp + 1, ldh = D | 1;
    const long long N = a.N;
    const int t = threadIdx.x, slot = t / NT, l = t % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;
    const size_t kk = (size_t)(valid ? k : 0), kd = kk * D;
    double* As = ls_sm;                       // 32 x lda  the workgroup's tile of A
    double* Ys = As + ls_tile_doubles(D) + (size_t)slot * ls_slot_doubles(D);
    double* Os = Ys + LS_TN;
    double* Vs = Os + LS_TN;
    double* Rs = Vs + LS_TN;
    double* Ws = Rs + LS_TN;
    double* Ts = Ws + LS_TN;
    double* xs = Ts + LS_TN;                  // Dp  the point (zeros beyond D)
    double* gs = xs + Dp;                     // Dp  g = -score there
    double* pv = gs + Dp;                     // Dp  pivots R_cc
    double* dg = pv + Dp;                     // Dp  the diagonal of H
    double* rd = dg + Dp;                     // Dp  the diagonal of R^{-1}
    double* cell = rd + Dp;                   // [0] NaN when a poisson row is flagged, [1] f
    double* Hs = cell + 4;                    // D x ldh
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

    const double* yk = a.y + kk * (size_t)N;
    const double* ok_ = a.offset ? a.offset + kk * (size_t)N : nullptr;
    const double* wk = a.w ? a.w + kk * (size_t)N : nullptr;
    double lam = 0.0, tau = 1.0;
    if (live) {
        lam = a.lam_dev ? a.lam_dev[k] : a.lam;
        if (FAM == LB_GAUSSIAN) tau = a.tau_dev ? a.tau_dev[k] : a.tau;
    }
    for (int e = t; e < LS_TN * lda; e += 256) As[e] = 0.0;         // the padding columns stay zero
    if (l < Dp) {
        const double* xsrc = STEP ? a.io.Xt : a.io.X;
        xs[l] = live && l < D ? xsrc[kd + l] : 0.0;
    }
    if (l == 0) cell[0] = 0.0;
    __syncthreads();                          // the zeros are in place before any thread writes the first tile

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
    // the tile elements e = t + 256 q of this thread as (row, column), stepped without a division: the whole workgroup stages A
    const int row0 = t / D, col0 = t - row0 * D, dr = 256 / D, dc = 256 - dr * D;
    const int en = l / NG, eg = l % NG;       // the eta pass: row en of the tile, columns eg, eg + NG, ..

    double pre[LS_AQ], ypre = 0.0, opre = 0.0, vpre = 0.0;
    {
        const int tnv = (int)(N < LS_TN ? N : LS_TN), te = tnv * D;
#pragma unroll
        for (int q = 0; q < LS_AQ; ++q) {
            const int e = t + q * 256;
            pre[q] = e < te ? a.A[e] : 0.0;
        }
        if (live && l < tnv) {                // (v = 0 in the rows beyond N: they are not selected)
            ypre = yk[l];
            if (ok_) opre = ok_[l];
            vpre = wk ? wk[l] : 1.0;
        }
    }
    double gacc = 0.0, facc = 0.0;

    for (long long n0 = 0; n0 < N; n0 += LS_TN) {
        const long long left = N - n0;
        const int tnv = (int)(left < LS_TN ? left : LS_TN);
        {                                     // registers -> LDS: the whole tile, zeros in the rows beyond N
            int r = row0, c = col0;
#pragma unroll
            for (int q = 0; q < LS_AQ; ++q) {
                if (t + q * 256 < LS_TN * D) As[r * lda + c] = pre[q];
                r += dr;
                c += dc;
                if (c >= D) {
                    c -= D;
                    ++r;
                }
            }
        }
        if (live && l < LS_TN) {              // a frozen slot does none of the work below: it stages A and runs the barriers
            Ys[l] = ypre;
            Os[l] = opre;
            Vs[l] = vpre;
        }
        __syncthreads();
        {                                     // the next tile's loads: in flight while this one is consumed
            const long long left2 = left - LS_TN;
            const int tnv2 = left2 < 0 ? 0 : (int)(left2 < LS_TN ? left2 : LS_TN), te2 = tnv2 * D;
            const double* An = a.A + (size_t)(n0 + LS_TN) * D;
#pragma unroll
            for (int q = 0; q < LS_AQ; ++q) {
                const int e = t + q * 256;
                pre[q] = e < te2 ? An[e] : 0.0;
            }
            ypre = 0.0;
            opre = 0.0;
            vpre = 0.0;
            if (live && l < tnv2) {
                ypre = yk[n0 + LS_TN + l];
                if (ok_) opre = ok_[n0 + LS_TN + l];
                vpre = wk ? wk[n0 + LS_TN + l] : 1.0;
            }
        }
        if (live) {                           // eta of row en: NG adjacent lanes take the columns eg + i NG, then a butterfly
            const double* ar = As + en * lda;
            double eta = 0.0;
            for (int j = eg; j < D; j += NG) eta = fma(ar[j], xs[j], eta);
#pragma unroll
            for (int o = NG / 2; o > 0; o >>= 1) eta += __shfl_xor(eta, o);
            eta += Os[en];
            if (eg == 0) {
                double r = 0.0, tt = 0.0, w = 0.0;
                const double yv = Ys[en], v = Vs[en];
                bool fine = lb_weight<FAM>(eta, yv, tau, w);
                if (STEP) fine = lb_link<FAM, true, true>(eta, yv, tau, r, tt) && fine;
                const bool on = v > 0.0;      // (false for a NaN weight and for the rows beyond N)
                Ws[en] = on ? v * w : 0.0;
                if (STEP) {
                    Rs[en] = on ? v * r : 0.0;
                    Ts[en] = on ? v * tt : 0.0;
                }
                if (FAM == LB_POISSON && on && !fine) cell[0] = qnan;   // (any number of threads, the same value)
            }
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int q = 0; q < MAXT; ++q) {
                if (ti[q] >= 0) {             // (wave-uniform)
                    const double* pa = As + ks * lda + ti[q] + cc;
                    const double* pb = As + ks * lda + tj[q] + cc;
#pragma unroll
                    for (int st = 0; st < LS_TN / 4; ++st) {
                        const double av = Ws[4 * st + ks] * pa[4 * st * lda], bv = pb[4 * st * lda];
                        acc[q] = GSMVI_MFMA_F64(av, bv, acc[q]);
                    }
                }
            }
            if (STEP) {
                if (l < D)
                    for (int n = 0; n < tnv; ++n) gacc = fma(Rs[n], As[n * lda + l], gacc);
                if (l == NT - 1)
                    for (int n = 0; n < tnv; ++n) facc += Ts[n];
            }
        }
        __syncthreads();                      // the next tile overwrites As, Ys, Os, Vs, Rs, Ws, Ts
    }

    // the upper triangle of sum_n v w a a^T -> LDS, g and f of phi = -lp
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
    // a non-finite x or a flagged poisson row (uniform in the slot: every wave forms it from the same numbers)
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
static int ls_go(gsmvi_ctx* ctx, void* stream, int family, const ls_args& a) {
    int ppw;
    unsigned grid;
    const size_t lds = lp_slot_launch(a.K, a.D, ls_slot_doubles(a.D), ls_tile_doubles(a.D), &ppw, &grid);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    glm_for_family(family, [&](auto fam) {
        if (ppw == 4)
            hipLaunchKernelGGL((k_laplace_shared_batched<64, decltype(fam)::value, MODE>), dim3(grid), dim3(256), lds, st, a);
        else
            hipLaunchKernelGGL((k_laplace_shared_batched<256, decltype(fam)::value, MODE>), dim3(grid), dim3(256), lds, st, a);
    });
    // the pair of bits is this kernel's alone (include/gsmvi_hip.h)
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LAPLACE | GSMVI_PATH_BATCHED_TARGET, "k_laplace_shared_batched");
}

// gb_check_overlaps over the model's six read-only arrays (A is one (N, D) matrix here) followed by the entry point's own
template <size_t NOWN>
static int ls_check_overlaps(const char* fn, const glm_model& m, const double* weights, const gb_arr (&own)[NOWN]) {
    const size_t ny = (size_t)m.K * m.N * 8, nk = (size_t)m.K * 8;
    gb_arr all[6 + NOWN] = {{m.A, (size_t)m.N * m.D * 8, "A", GB_RD},
                            {m.y, ny, "y", GB_RD},
                            {m.offset, ny, "offset", GB_RD},
                            {weights, ny, "weights", GB_RD},
                            {m.tau_dev, nk, "noise_prec_dev", GB_RD},
                            {m.lam_dev, nk, "prior_prec_dev", GB_RD}};
    for (size_t i = 0; i < NOWN; ++i) all[6 + i] = own[i];
    return gb_check_overlaps(fn, all, all + 6 + NOWN);
}

static ls_args ls_args_of(const glm_model& m, const double* weights, const lp_io& io) {
    return {m.K, m.N, m.D, m.A, m.y, m.offset, weights, m.lam, m.lam_dev, m.tau, m.tau_dev, io};
}

extern "C" {

// the model's checks are the per-problem entry's (its "K N D is too large" bounds y, offset and weights here, and A a fortiori; K
// is bounded by the slot packing, which is tighter than the row bound of gsmvi_glm_shared_batched_f64 at nc = 1)
int gsmvi_glm_shared_hessian_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t N, int family, const double* A,
                                         const double* y, const double* offset, const double* weights, double noise_prec,
                                         const double* noise_prec_dev, double prior_prec, const double* prior_prec_dev,
                                         const double* X, double* H, double* cov, int* info_dev) {
    const glm_model m = {K, N, D, A, y, offset, nullptr, prior_prec, prior_prec_dev, noise_prec, noise_prec_dev};
    if (int st = glm_check_model(__func__, m, family, "N", true)) return st;
    const ls_args a = ls_args_of(m, weights, lp_hess_io(X, H, cov, info_dev));
    GB_BAD(!A || !y, "NULL array");
    if (int st = lp_check_hess(__func__, a.io)) return st;
    gb_arr own[LP_HESS_ROWS];
    lp_hess_rows(own, K, D, a.io);
    if (int st = ls_check_overlaps(__func__, m, weights, own)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    return ls_go<LP_HESS>(ctx, stream, family, a);
}

int gsmvi_laplace_shared_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t N, int family, const double* A,
                                          const double* y, const double* offset, const double* weights, double noise_prec,
                                          const double* noise_prec_dev, double prior_prec, const double* prior_prec_dev, int start,
                                          double* x, double* g, double* d, double* sc, int* ist, double* Xt, int* stopped_dev,
                                          int maxiter, int maxfun, double gtol) {
    const glm_model m = {K, N, D, A, y, offset, nullptr, prior_prec, prior_prec_dev, noise_prec, noise_prec_dev};
    if (int st = glm_check_model(__func__, m, family, "N", true)) return st;
    const ls_args a = ls_args_of(m, weights, lp_step_io(start, x, g, d, sc, ist, Xt, stopped_dev, maxiter, maxfun, gtol));
    GB_BAD(!A || !y, "NULL array");
    if (int st = lp_check_step(__func__, a.io)) return st;
    gb_arr own[LP_STEP_ROWS];
    lp_step_rows(own, K, D, a.io);
    if (int st = ls_check_overlaps(__func__, m, weights, own)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    return ls_go<LP_STEP>(ctx, stream, family, a);
}

}  // extern "C"
