// Batched Laplace initialiser: the negative Hessian of K GLM posteriors of one (N, D), D <= 64, its inverse, and one damped
// Newton (IRLS) round per launch for every running problem ("Batched Laplace initialiser").
//
// The reference has no Laplace initialiser: it starts its fits from the L-BFGS-B maximiser of lp and the optimiser's dense
// inverse-Hessian estimate (gsmvi/initializers.py:5-17), for a model given as log_prob and jit(grad(...)) of it
// (examples/example_gsm.py:34-35).  For the four GLM families of gsmvi_glm_batched_f64 the second derivative is closed-form:
// with eta_n = a_n . x + o_kn and the weight w = -dr / d eta of gsmvi_glm_link.h,
//   H_k(x) = sum_{n < n_k} w(eta_n, y_n) a_n a_n^T + lam_k I          (the negative Hessian of lp_k: positive semi-definite)
// and the Newton direction of phi = -lp is d = -H^{-1} g, g = -score.
//   k_laplace_batched<NT, FAM, LP_HESS> : H_k at the rows of X, cov_k = H_k^{-1} and info_k
//   k_laplace_batched<NT, FAM, LP_STEP> : f, g and H at the trial point Xt_k in ONE sweep over A_k, then the accept / reject
//                                         decision of the line search, the stopping tests, the factorisation, d, and the next
//                                         trial point
// Work mapping: the slots of gsmvi_batched.h (gb_nt(D) threads per problem, four problems -- one wave each -- per 256-thread
// workgroup for D <= 16).  A slot walks the rows of A_k in tiles of LB_TN = 32, staged in LDS zero-padded to Dp = 16 ceil(D / 16)
// columns (row stride Dp + 1) and to 32 rows; the next tile's loads are in flight while the current one is consumed, as in
// k_logistic_batched.  Per tile: NT / 32 adjacent lanes share a row's eta (a butterfly over them), one of them applies the link
// and leaves r, t, w of the row in LDS; then the Gram product runs on the fp64 MFMA (16 x 16 x 4): for the 16 x 16 block (bi, bj),
// bi <= bj, of H the A operand is w_n a_{n, 16 bi + c} and the B operand a_{n, 16 bj + c}, both from the tile, eight steps per
// tile, and the accumulators (at most three blocks per wave: ten blocks of the upper triangle over four waves at Dp = 64) stay in
// registers across all of N.  Thread j < D sums g_j = sum_n r_n a_nj over the tile's rows in order, one thread sums t.
// After the sweep the upper triangle (i <= j; of a diagonal block too: (w a_i) a_j and (w a_j) a_i round differently) goes to LDS,
// lam is added to the diagonal, and H is written mirrored: exactly symmetric.  The Cholesky factorisation is the right-looking
// one of gb_chol_lds with a relative pivot rule: pivot j fails when it is not finite or not > 64 eps H_jj, so a rank-deficient
// H fails whatever the rounding.  The Newton direction is two triangular solves in the slot's first wave (component l in lane
// l, one broadcast per column).  The inverse is R^{-1} R^{-T}: thread j back-substitutes column j of R^{-1} into row j of the
// (free) lower triangle, then entry (i, j), i <= j, is one dot product, written to (i, j) and (j, i).
// Order: every sum over n runs n = 0 .. n_k - 1 in tiles of 32, eight MFMA steps of four rows per tile; it depends on (N, D)
// alone, not on K, the slot packing or the neighbours.  Rows n >= n_k are never loaded.  A slot reads and writes only slice k of
// every array and every slot of a workgroup runs the same barriers.  A problem whose status is not 0 is frozen: its slot loads
// nothing of A_k, does none of the per-tile work (as every slot does for the tiles past n_k) and writes nothing; it still runs
// the barriers of the sweep beside its running neighbours.  A workgroup all of whose problems are frozen leaves at once.
// Ordering in the Hessian entry: H is written from LDS (the lower triangle from the mirrored cells, which other threads own),
// then a barrier, then the factorisation overwrites those cells in place.  Inputs are only read; no context workspace.
// The model's fields (lp_args::m), their checks, their overlap entries, the dispatch on the family and the per-problem prologue
// are gsmvi_glm_model.h's, shared with the score and predictive entries; the butterflies are gsmvi_batched.h's.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_laplace_stage.h"
#include "gsmvi_glm_model.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

#define LP_AQ 8        // tile elements per thread: LB_TN D / NT <= 8 in both packings

struct lp_args {
    glm_model m;
    lp_io io;
};

// LDS doubles per problem: the A tile (32 x (Dp + 1)), y, offset, r, w, t of its rows (32 each), x, g, pivots, the diagonal of H
// and the diagonal of R^{-1} (Dp each), four cells, H (D x (D | 1)).  D = 64: 6724 doubles, 52.5 KB; four problems of D = 16: 33 KB
__host__ __device__ inline int lp_lds_doubles(int D) {
    const int Dp = glm_dp(D);
    return LB_TN * (Dp + 1) + 5 * LB_TN + 5 * Dp + 4 + D * (D | 1);
}

template <int NT, int FAM, int MODE>
__global__ __launch_bounds__(256) void k_laplace_batched(lp_args a) {
    extern __shared__ double lp_sm[];
    constexpr int PPW = 256 / NT, NW = NT / 64, NG = NT / LB_TN;
    constexpr int MAXT = NT == 256 ? 3 : 1;       // 16 x 16 blocks of H per wave
    constexpr int MAXE = NT == 256 ? 16 : 4;      // entries of H per thread
    constexpr bool STEP = MODE == LP_STEP;
    const int D = a.m.D, nb = (D + 15) >> 4, Dp = nb * 16, lda = Dp + 1, ldh = D | 1, DD = D * D;
    const long long N = a.m.N;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.m.K;
    const size_t kk = (size_t)(valid ? k : 0), kd = kk * D;
    double* As = lp_sm + (size_t)slot * lp_lds_doubles(D);
    double* Ys = As + LB_TN * lda;
    double* Os = Ys + LB_TN;
    double* Rs = Os + LB_TN;
    double* Ws = Rs + LB_TN;
    double* Ts = Ws + LB_TN;
    double* xs = Ts + LB_TN;                  // Dp  the point (zeros beyond D)
    double* gs = xs + Dp;                     // Dp  g = -score there
    double* pv = gs + Dp;                     // Dp  pivots R_cc
    double* dg = pv + Dp;                     // Dp  the diagonal of H
    double* rd = dg + Dp;                     // Dp  the diagonal of R^{-1}
    double* cell = rd + Dp;                   // [0] NaN when a poisson row is flagged, [1] f
    double* Hs = cell + 4;                    // D x ldh
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    int* is = STEP ? a.io.ist + kk * LP_NIS : nullptr;
    double* sc = STEP ? a.io.sc + kk * LP_NSC : nullptr;
    int status = 0, nit = 0, nfev = 0, nls = 0;
    double f = 0.0, t = 0.0, gd = 0.0;
    bool live = valid;
    if (STEP) {
        if (valid && !a.io.start) {
            status = is[LP_STATUS]; nit = is[LP_NIT]; nfev = is[LP_NFEV]; nls = is[LP_NLS];
            f = sc[LP_F]; t = sc[LP_T]; gd = sc[LP_GD];
        }
        live = valid && status == 0;
        if (!__syncthreads_or(live)) return;  // every problem of the workgroup is frozen (uniform)
    }

    const double* Ak = a.m.A + kk * (size_t)N * D;
    const double* yk = a.m.y + kk * (size_t)N;
    const double* ok_ = a.m.offset ? a.m.offset + kk * (size_t)N : nullptr;
    const glm_problem pk = glm_problem_of<FAM>(a.m, k, live);
    const long long nk = pk.nk;               // the rows that count (a frozen slot: none, so nothing of A_k is loaded)
    const double lam = pk.lam, tau = pk.tau;
    for (int e = l; e < LB_TN * lda; e += NT) As[e] = 0.0;          // the padding columns stay zero
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
    // the tile elements e = l + q NT of this thread as (row, column), stepped without a division
    const int row0 = l / D, col0 = l - row0 * D, dr = NT / D, dc = NT - dr * D;
    const int en = l / NG, eg = l % NG;       // the eta pass: row en of the tile, columns eg, eg + NG, ..

    double pre[LP_AQ], ypre = 0.0, opre = 0.0;
    {
        const int tnv = (int)(nk < LB_TN ? nk : LB_TN), te = tnv * D;
#pragma unroll
        for (int q = 0; q < LP_AQ; ++q) {
            const int e = l + q * NT;
            pre[q] = e < te ? Ak[e] : 0.0;
        }
        if (l < tnv) {
            ypre = yk[l];
            if (ok_) opre = ok_[l];
        }
    }
    double gacc = 0.0, facc = 0.0;

    for (long long n0 = 0; n0 < N; n0 += LB_TN) {
        const long long left = nk - n0;
        const int tnv = left < 0 ? 0 : (int)(left < LB_TN ? left : LB_TN);
        // a tile without a row that counts (past n_k; every tile of a frozen slot) does none of the work below: it only runs
        // the barriers, which must stay uniform across the slots of a workgroup (tnv is uniform in the slot)
        if (tnv > 0) {                        // registers -> LDS: the whole tile, zeros in the rows that do not count
            int r = row0, c = col0;
#pragma unroll
            for (int q = 0; q < LP_AQ; ++q) {
                if (l + q * NT < LB_TN * D) As[r * lda + c] = pre[q];
                r += dr;
                c += dc;
                if (c >= D) {
                    c -= D;
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
            const int tnv2 = left2 < 0 ? 0 : (int)(left2 < LB_TN ? left2 : LB_TN), te2 = tnv2 * D;
            const double* An = Ak + (size_t)(n0 + LB_TN) * D;
#pragma unroll
            for (int q = 0; q < LP_AQ; ++q) {
                const int e = l + q * NT;
                pre[q] = e < te2 ? An[e] : 0.0;
            }
            ypre = 0.0;
            opre = 0.0;
            if (l < tnv2) {
                ypre = yk[n0 + LB_TN + l];
                if (ok_) opre = ok_[n0 + LB_TN + l];
            }
        }
        if (tnv > 0) {                        // eta of row en: NG adjacent lanes take the columns eg + i NG, then a butterfly
            const double* ar = As + en * lda;
            double eta = 0.0;
            for (int j = eg; j < D; j += NG) eta = fma(ar[j], xs[j], eta);
#pragma unroll
            for (int o = NG / 2; o > 0; o >>= 1) eta += __shfl_xor(eta, o);
            eta += Os[en];
            if (eg == 0) {
                double r = 0.0, tt = 0.0, w = 0.0;
                const double yv = Ys[en];
                bool fine = lb_weight<FAM>(eta, yv, tau, w);
                if (STEP) fine = lb_link<FAM, true, true>(eta, yv, tau, r, tt) && fine;
                const bool on = en < tnv;
                Ws[en] = on ? w : 0.0;
                if (STEP) {
                    Rs[en] = on ? r : 0.0;
                    Ts[en] = on ? tt : 0.0;
                }
                if (FAM == LB_POISSON && on && !fine) cell[0] = qnan;   // (any number of threads, the same value)
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < MAXT; ++q) {
            if (ti[q] >= 0 && tnv > 0) {      // (wave-uniform)
                const double* pa = As + ks * lda + ti[q] + cc;
                const double* pb = As + ks * lda + tj[q] + cc;
#pragma unroll
                for (int s = 0; s < LB_TN / 4; ++s) {
                    const double av = Ws[4 * s + ks] * pa[4 * s * lda], bv = pb[4 * s * lda];
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
        __syncthreads();                      // the next tile overwrites As, Ys, Os, Rs, Ws, Ts
    }

    // the upper triangle of sum_n w a a^T -> LDS, g and f of phi = -lp
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

    double ft = 0.0, gtl = 0.0, gmax = 0.0;
    bool fin = false, ok = false, need = false;
    if (STEP) {
        ft = bad ? qnan : cell[1];
        gtl = ln < D ? (bad ? qnan : gs[ln]) : 0.0;
        fin = !bad && gb_finite(ft) && __all(gb_finite(gtl));
        gmax = gb_wave_max(fabs(gtl));
        if (live) {
            if (a.io.start)
                need = fin && !(gmax <= a.io.gtol);
            else {
                ok = fin && ft <= (f + (1e-4 * t) * gd) + 1e-10 * fmax(1.0, fabs(f));
                need = ok && !(gmax <= a.io.gtol) && !(nit + 1 >= a.io.maxiter || nfev + 1 >= a.io.maxfun);
            }
        }
    } else {
        need = live && !bad && a.io.cov != nullptr;
        if (live && a.io.H) {
#pragma unroll
            for (int q = 0; q < MAXE; ++q) {
                const int e = l + q * NT;
                if (e < DD) {
                    const int i = e / D, j = e - i * D;
                    a.io.H[kk * DD + e] = bad ? qnan : (i <= j ? Hs[i * ldh + j] : Hs[j * ldh + i]);
                }
            }
        }
        // entry (i, j), i > j, was read from another thread's cell (j, i): every read of H is done before the factorisation
        // below starts to overwrite it in place
        __syncthreads();
    }

    int info = lp_chol_lds<NT, MAXE>(need, D, l, ldh, Hs, pv, dg);     // (its last barrier publishes R and the pivots)

    if (!STEP) {
        if (!a.io.cov) return;                   // (uniform)
        if (live && bad) info = 1;
        const bool inv = need && info == 0;
        if (inv && l < D) {                   // column l of R^{-1} into row l of the lower triangle, its diagonal into rd
            const int j = l;
            const double xj = 1.0 / pv[j];
            rd[j] = xj;
            for (int i = j - 1; i >= 0; --i) {
                double s = 0.0;
                for (int c = i + 1; c < j; ++c) s += Hs[i * ldh + c] * Hs[j * ldh + c];
                s += Hs[i * ldh + j] * xj;
                Hs[j * ldh + i] = -s / pv[i];
            }
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int q = 0; q < MAXE; ++q) {
                const int e = l + q * NT;
                if (e < DD) {
                    const int i = e / D, j = e - i * D;
                    if (i <= j) {
                        double s;
                        if (inv) {
                            s = (i == j ? rd[j] : Hs[j * ldh + i]) * rd[j];
                            for (int c = j + 1; c < D; ++c) s += Hs[c * ldh + i] * Hs[c * ldh + j];
                        } else
                            s = i == j ? 1.0 : 0.0;                     // nothing is known: the identity
                        a.io.cov[kk * DD + e] = s;
                        a.io.cov[kk * DD + (size_t)j * D + i] = s;
                    }
                }
            }
            if (l == 0) a.io.info[k] = info;
        }
        return;
    }

    if (!live || l >= 64) return;             // the rest is the first wave's: component l of every vector in lane l
    const bool act = l < D;
    double xl = act ? xs[l] : 0.0, gl = gtl, dl = 0.0;
    bool newdir = false;
    if (a.io.start) {
        nfev = 1;
        nit = 0;
        nls = 0;
        f = ft;
        t = 0.0;
        gd = 0.0;
        if (!fin) status = 4;
        else if (gmax <= a.io.gtol) status = 1;
        else if (info != 0) status = 5;
        else newdir = true;
    } else {
        nfev += 1;
        if (!ok) {
            t = 0.5 * t;
            nls += 1;
            if (nls > 20) status = 3;
            else if (nfev >= a.io.maxfun) status = 2;
            else if (act) a.io.Xt[kd + l] = a.io.x[kd + l] + t * a.io.d[kd + l];
            if (l == 0) {
                sc[LP_T] = t;
                is[LP_NLS] = nls; is[LP_NFEV] = nfev; is[LP_STATUS] = status;
                if (status != 0 && a.io.stopped) atomicAdd(a.io.stopped, 1);
            }
            return;
        }
        f = ft;
        nit += 1;
        if (gmax <= a.io.gtol) status = 1;
        else if (nit >= a.io.maxiter || nfev >= a.io.maxfun) status = 2;
        else if (info != 0) status = 5;
        else newdir = true;
    }
    if (newdir) {                             // d = -H^{-1} g: R^T z = g, R s = z (R upper, R^T R = H)
        double b = gl;
        for (int c = 0; c < D; ++c) {
            const double zc = __shfl(b, c) / pv[c];
            if (l == c) b = zc;
            else if (l > c && act) b -= Hs[c * ldh + l] * zc;
        }
        for (int c = D - 1; c >= 0; --c) {
            const double sc_ = __shfl(b, c) / pv[c];
            if (l == c) b = sc_;
            else if (l < c) b -= Hs[l * ldh + c] * sc_;
        }
        dl = act ? -b : 0.0;
        t = 1.0;
        gd = gb_wave_sum(gl * dl);
        nls = 0;
    }
    if (act) {
        a.io.x[kd + l] = xl;
        a.io.g[kd + l] = gl;
        if (newdir || a.io.start) a.io.d[kd + l] = dl;
        if (newdir) a.io.Xt[kd + l] = xl + dl;
    }
    if (l == 0) {
        sc[LP_F] = f;
        if (newdir || a.io.start) {
            sc[LP_T] = t;
            sc[LP_GD] = gd;
        }
        if (a.io.start) sc[3] = 0.0;
        is[LP_STATUS] = status; is[LP_NIT] = nit; is[LP_NFEV] = nfev; is[LP_NLS] = nls;
        if (a.io.start) { is[4] = 0; is[5] = 0; is[6] = 0; is[7] = 0; }
        if (status != 0 && a.io.stopped) atomicAdd(a.io.stopped, 1);
    }
}

template <int MODE>
static int lp_go(gsmvi_ctx* ctx, void* stream, int family, const lp_args& a) {
    int ppw;
    unsigned grid;
    const size_t lds = lp_slot_launch(a.m.K, a.m.D, lp_lds_doubles(a.m.D), 0, &ppw, &grid);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    glm_for_family(family, [&](auto fam) {
        if (ppw == 4)
            hipLaunchKernelGGL((k_laplace_batched<64, decltype(fam)::value, MODE>), dim3(grid), dim3(256), lds, st, a);
        else
            hipLaunchKernelGGL((k_laplace_batched<256, decltype(fam)::value, MODE>), dim3(grid), dim3(256), lds, st, a);
    });
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LAPLACE, "k_laplace_batched");
}

extern "C" {

int gsmvi_glm_hessian_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t N, int family, const double* A,
                                  const double* y, const double* offset, const int* counts_dev, double noise_prec,
                                  const double* noise_prec_dev, double prior_prec, const double* prior_prec_dev, const double* X,
                                  double* H, double* cov, int* info_dev) {
    const lp_args a = {{K, N, D, A, y, offset, counts_dev, prior_prec, prior_prec_dev, noise_prec, noise_prec_dev},
                       lp_hess_io(X, H, cov, info_dev)};
    if (int st = glm_check_model(__func__, a.m, family, "N", true)) return st;
    GB_BAD(!A || !y, "NULL array");
    if (int st = lp_check_hess(__func__, a.io)) return st;
    gb_arr own[LP_HESS_ROWS];
    lp_hess_rows(own, K, D, a.io);
    if (int st = gb_check_overlaps(__func__, a.m, own)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    return lp_go<LP_HESS>(ctx, stream, family, a);
}

int gsmvi_laplace_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t N, int family, const double* A,
                                   const double* y, const double* offset, const int* counts_dev, double noise_prec,
                                   const double* noise_prec_dev, double prior_prec, const double* prior_prec_dev, int start,
                                   double* x, double* g, double* d, double* sc, int* ist, double* Xt, int* stopped_dev, int maxiter,
                                   int maxfun, double gtol) {
    const lp_args a = {{K, N, D, A, y, offset, counts_dev, prior_prec, prior_prec_dev, noise_prec, noise_prec_dev},
                       lp_step_io(start, x, g, d, sc, ist, Xt, stopped_dev, maxiter, maxfun, gtol)};
    if (int st = glm_check_model(__func__, a.m, family, "N", true)) return st;
    GB_BAD(!A || !y, "NULL array");
    if (int st = lp_check_step(__func__, a.io)) return st;
    gb_arr own[LP_STEP_ROWS];
    lp_step_rows(own, K, D, a.io);
    if (int st = gb_check_overlaps(__func__, a.m, own)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    return lp_go<LP_STEP>(ctx, stream, family, a);
}

}  // extern "C"
