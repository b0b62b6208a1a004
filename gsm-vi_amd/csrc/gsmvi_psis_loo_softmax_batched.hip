// Batched softmax PSIS leave-one-out: for K fitted Gaussians q_k over the coefficients of K multinomial logit regressions of one
// (N, C, P), D = (C - 1) P <= 64, the pointwise leave-one-out log predictive density of every observation from S draws of q_k, one
// launch ("Batched softmax PSIS-LOO"; the definition is in include/gsmvi_hip.h, above
// gsmvi_psis_loo_softmax_batched_f64).  The reference has no twin.
//   k_psis_loo_softmax_batched      (not a template over C: the class loops are rolled, as in k_softmax_batched)
// The work mapping, the LDS, the loaders, the lane map and stage (2) are the tile block's (gsmvi_psis_loo_tile.h), with
// NI = gsmvi_psis_loo_softmax_tile(C, P, S) and the first nv rows of a tile valid (counts).
//   (1) l_si of the tile on the fp64 MFMA (16 x 16 x 4), class by class: the A tile has Pp = 4 ceil(P / 4) columns (row stride
//       Pp + 1); the draw tiles keep their rows as in memory (class-major, row stride D | 1, rows past S zero).  For class c
//       the A operand is x_{s, c P + 4 j + kq}, the B operand a_{i, 4 j + kq}, Pp / 4 steps.  Two sweeps over the classes, the
//       MFMA chain recomputed in the second (the same instructions on the same LDS values: the same bits): sweep 1 takes
//       m = max(0, eta_c), selects eta_y and notes a non-finite eta; sweep 2 sums exp(eta_c - m) in class order and adds the
//       reference class's exp(-m) last, as z = 1 + rest (sm_add_term of gsmvi_softmax_model.h: the terms below 1, then the count
//       of the terms that are 1), and log z is log1p(rest) (sm_log_s: log(z) is 0 where rest < eps / 2).  No eta is stored and
//       the registers do not depend on C.  Only lanes whose column is a valid observation run the comparisons and exponentials.
//       The padding rule: with P % 4 != 0 the k positions 4 j + kq >= P of class c would address x entries of class c + 1 (past
//       column D - 1 at the last class), and there the B operand holds a padded zero: 0 x non-finite = NaN would flag a draw
//       that the definition does not.  The X tile keeps the memory layout and the A operand is MASKED instead: a lane whose k
//       position is >= P feeds 0.0 and loads nothing, so a padded position is 0 x 0 on both sides and no LDS word outside the
//       row's D entries is read.  (A padded layout, Pp columns per class, takes up to 64 x 257 doubles at (65, 1): it would not
//       leave room for one observation at S = 4096.)  A non-finite x_{s, c P + j} needs no flag of its own: it meets a_ij in the
//       dot of class c of every valid row, the product is +-inf or NaN (0 x inf included), and so is the sum: the draw's l_si is
//       NaN for every valid observation of the problem, by the non-finite-eta rule.
// A label is compared, never used as an index.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_psis_loo_tile.h"
#include "gsmvi_softmax_model.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

struct pls_args {
    long long N;
    int C, P, D;                // classes, features, (C - 1) P
    const double* A;            // (K, N, P)
    const int* labels;          // (K, N)
    const int* counts;          // (K) valid rows, clamped to 0 .. N (null: N)
    ps_loo_args c;              // (X class-major)
};

// doubles of the kernel's own use of the shared region: the X tile, the A tile and the 16 labels
static inline int pls_tiles_doubles(int C, int P) {
    return PS_LOO_TR * (((C - 1) * P) | 1) + PS_LOO_NB * (sm_pp(P) + 1) + PS_LOO_NB;
}

__global__ __launch_bounds__(256) void k_psis_loo_softmax_batched(pls_args a) {
    const int l = threadIdx.x, S = a.c.S;
    const int P = a.P, Cm = a.C - 1, D = a.D, Pp = sm_pp(P), lda = Pp + 1, ldx = D | 1;
    const ps_loo_pos p = ps_loo_pos_of(a.c, a.N);
    const int nv = ps_loo_valid(sm_rows_of(a.counts, (long long)p.k, a.N), p);
    const ps_loo_lds lds = ps_loo_carve(a.c);
    double* Xs = lds.tiles;                   // 64 x ldx      a tile of draws          (over the stage's arrays)
    double* As = Xs + PS_LOO_TR * ldx;        // 16 x lda      the tile's rows of A_k, zero-padded
    int* ys = reinterpret_cast<int*>(As + PS_LOO_NB * lda);     // 16 labels (in 16 doubles)
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    // ---- (1) l_si of the tile's valid observations ------------------------------------------------------------------------
    if (nv > 0) {                             // (uniform in the workgroup)
        ps_loo_load_rows(As, lda, a.A + p.kn * P, P, nv, P, l);
        if (l < PS_LOO_NB) ys[l] = l < nv ? a.labels[p.kn + l] : 0;
        const double* Xk = a.c.X + p.ks * D;
        const ps_loo_lane ln = ps_loo_lane_of(l);
        const int cc = ln.cc, kq = ln.kq;
        for (int t0 = 0; t0 < S; t0 += PS_LOO_TR) {
            __syncthreads();                  // the previous tile's readers are done
            ps_loo_load_draws(Xs, ldx, Xk, D, D, t0, S, l);
            __syncthreads();
            if (t0 + 16 * ln.wv < S) {        // (wave-uniform)
                const double* px = Xs + (16 * ln.wv + cc) * ldx + kq;
                const double* pb = As + cc * lda + kq;
                const bool live = cc < nv;    // the lane's column is a valid observation
                const int yv = live ? ys[cc] : 0;
                double m[4] = {0.0, 0.0, 0.0, 0.0}, ey[4] = {0.0, 0.0, 0.0, 0.0};   // the reference class: eta = 0
                bool fine[4] = {true, true, true, true};
#pragma unroll 1
                for (int c = 0; c < Cm; ++c) {                  // sweep 1: the maximum, eta_y, the finiteness
                    const v4d acc = sm_eta(px, pb, c, P, Pp, kq);
                    if (live) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            fine[r] = fine[r] && gb_finite(acc[r]);
                            m[r] = fmax(m[r], acc[r]);
                            ey[r] = c == yv ? acc[r] : ey[r];
                        }
                    }
                }
                double z[4] = {0.0, 0.0, 0.0, 0.0}, nt[4] = {0.0, 0.0, 0.0, 0.0};      // z = 1 + rest: sm_add_term
#pragma unroll 1
                for (int c = 0; c < Cm; ++c) {                  // sweep 2: the same chain, the sum in class order
                    const v4d acc = sm_eta(px, pb, c, P, Pp, kq);
                    if (live) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) sm_add_term(z[r], nt[r], exp(acc[r] - m[r]));
                    }
                }
                if (live) {
                    const bool yok = yv >= 0 && yv <= Cm;       // (yv = C - 1: the reference class, eta_y = 0)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int s = ps_loo_draw(t0, ln, r);
                        sm_add_term(z[r], nt[r], exp(0.0 - m[r]));
                        const double rest = sm_rest(z[r], nt[r]);
                        if (s < S) lds.ell[cc * S + s] = yok && fine[r] ? ey[r] - m[r] - sm_log_s(rest, 1.0 + rest) : qnan;
                    }
                }
            }
        }
    }
    __syncthreads();                          // l_si is published; the tiles are dead, the stage may take their place

    ps_loo_stage(a.c.o, lds.sm, lds.ell, p.ni, nv, nullptr, p.ks, p.kn, S, a.c.S2, a.c.M, l);     // (2)
}

hipError_t gsmvi_psis_loo_softmax_batched_prepare() { return gb_allow_lds(k_psis_loo_softmax_batched); }

extern "C" {

int gsmvi_psis_loo_softmax_tile(int C, int P, int64_t S) {
    if (!sm_shape_ok(C, P) || S < PS_MIN_S || S > PS_MAX_S) return 0;
    return ps_loo_tile(pls_tiles_doubles(C, P), (int)S, PLS_NI_CAP);
}

int gsmvi_psis_loo_softmax_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int C, int P, int64_t N, int64_t S,
                                       const double* A, const int* labels, const int* counts_dev, const double* X,
                                       const double* logr, const double* lw, double* loglik, double* elpd, double* lpd,
                                       double* khat, double* ess, int* info) {
    const sm_model m = sm_model_of(K, N, C, P, A, labels, counts_dev);
    if (int st = sm_check_model(__func__, m, false, "N")) return st;
    ps_loo_launch p = {};
    if (int st = ps_loo_plan(__func__, K, N, S, P, !A || !labels, X, {logr, lw, loglik, elpd, lpd, khat, ess, info},
                             pls_tiles_doubles(C, P), PLS_NI_CAP, "gsmvi_psis_loo_softmax_tile(C, P, S)", &p))
        return st;
    gb_arr own[PS_LOO_ROWS];
    ps_loo_overlap_rows(own, K, N, m.D, p.c);
    if (int st = gb_check_overlaps(__func__, m, own)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    const pls_args a = {N, C, P, m.D, A, labels, counts_dev, p.c};
    hipLaunchKernelGGL(k_psis_loo_softmax_batched, dim3(p.grid), dim3(256), p.lds, reinterpret_cast<hipStream_t>(stream), a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_SOFTMAX, "k_psis_loo_softmax_batched");
}

}  // extern "C"
