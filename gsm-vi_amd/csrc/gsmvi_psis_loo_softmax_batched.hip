// Batched softmax PSIS leave-one-out: for K fitted Gaussians q_k over the coefficients of K multinomial logit regressions of one
// (N, C, P), D = (C - 1) P <= 64, the pointwise leave-one-out log predictive density of every observation from S draws of q_k, one
// launch ("Batched softmax PSIS-LOO"; the definition is in include/gsmvi_hip.h, above
// gsmvi_psis_loo_softmax_batched_f64).  The reference has no twin.
//   k_psis_loo_softmax_batched      (not a template over C: the class loops are rolled, as in k_softmax_batched)
// Work mapping: one 256-thread workgroup per (problem k, tile of NI = gsmvi_psis_loo_softmax_tile(C, P, S) observations).
//   (1) l_si of the tile on the fp64 MFMA (16 x 16 x 4), class by class: the NI rows of A_k sit in LDS zero-padded to 16 rows of
//       Pp = 4 ceil(P / 4) columns (row stride Pp + 1); X_k streams through LDS once in tiles of 64 draws, rows as in memory
//       (class-major, row stride D | 1, rows past S zero); wave w takes the 16 draws 16 w .. 16 w + 15 of the tile.  For class c
//       the A operand is x_{s, c P + 4 j + kq}, the B operand a_{i, 4 j + kq}, Pp / 4 steps.  Two sweeps over the classes, the
//       MFMA chain recomputed in the second (the same instructions on the same LDS values: the same bits): sweep 1 takes
//       m = max(0, eta_c), selects eta_y and notes a non-finite eta; sweep 2 sums exp(eta_c - m) in class order and adds the
//       reference class's exp(-m) last, as z = 1 + rest (sm_add_term of gsmvi_softmax_model.h: the terms below 1, then the count
//       of the terms that are 1), and log z is log1p(rest) (sm_log_s: log(z) is 0 where rest < eps / 2).  No eta is stored and
//       the registers do not depend on C.  Only lanes whose column is a valid observation run the comparisons and exponentials.
//       The tile's l_si stay in LDS (NI x S doubles).
//       The padding rule: with P % 4 != 0 the k positions 4 j + kq >= P of class c would address x entries of class c + 1 (past
//       column D - 1 at the last class), and there the B operand holds a padded zero: 0 x non-finite = NaN would flag a draw
//       that the definition does not.  The X tile keeps the memory layout and the A operand is MASKED instead: a lane whose k
//       position is >= P feeds 0.0 and loads nothing, so a padded position is 0 x 0 on both sides and no LDS word outside the
//       row's D entries is read.  (A padded layout, Pp columns per class, takes up to 64 x 257 doubles at (65, 1): it would not
//       leave room for one observation at S = 4096.)  A non-finite x_{s, c P + j} needs no flag of its own: it meets a_ij in the
//       dot of class c of every valid row, the product is +-inf or NaN (0 x inf included), and so is the sum: the draw's l_si is
//       NaN for every valid observation of the problem, by the non-finite-eta rule.
//   (2) per observation of the tile: ps_loo_stage (gsmvi_psis_stage.h, shared with k_psis_loo_batched): rho_s = logr_s - l_si
//       into the PSIS stage's array, ps_stage, then the two log-sum-exps through ps_max and ps_sum.
// The tiles of (1) lie over the stage's LDS (dead before the first stage starts).  NI is the largest count, at most PLS_NI_CAP,
// whose l_si fit beside that region in GB_LDS_MAX.  Every sum is a fixed tree and there are no atomics; every thread of a
// workgroup runs the same barriers whatever the verdicts; a workgroup reads only slice k of the inputs and writes only its own
// (k, i) entries.  A label is compared, never used as an index.  Inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_psis_stage.h"
#include "gsmvi_softmax_model.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

struct pls_args {
    long long K, N;
    int C, P, D;                // classes, features, (C - 1) P
    int S, S2, M;               // draws, draws padded to a power of two, the tail size before ties
    int NI, U;                  // observations per tile; doubles of the region the stage and the MFMA tiles share
    unsigned ntile;             // tiles per problem: ceil(N / NI)
    const double* A;            // (K, N, P)
    const int* labels;          // (K, N)
    const int* counts;          // (K) valid rows, clamped to 0 .. N (null: N)
    const double* X;            // (K, S, D) the draws of q_k, class-major
    ps_loo_io o;                // the ratios and weights of the problem-level run, the outputs
};

// doubles of the kernel's own use of the shared region: the X tile, the A tile and the 16 labels
static inline int pls_tiles_doubles(int C, int P) {
    return PS_LOO_TR * (((C - 1) * P) | 1) + PS_LOO_NB * (sm_pp(P) + 1) + PS_LOO_NB;
}

static int pls_tile(int C, int P, int S) { return ps_loo_tile(pls_tiles_doubles(C, P), S, PLS_NI_CAP); }

__global__ __launch_bounds__(256) void k_psis_loo_softmax_batched(pls_args a) {
    extern __shared__ double pls_sm[];
    const int l = threadIdx.x, S = a.S, S2 = a.S2, M = a.M, NI = a.NI;
    const int P = a.P, Cm = a.C - 1, D = a.D, Pp = sm_pp(P), lda = Pp + 1, ldx = D | 1;
    const long long N = a.N;
    const size_t k = blockIdx.x / a.ntile;
    const long long i0 = (long long)(blockIdx.x - (unsigned)k * a.ntile) * NI;       // the tile's first observation
    const int ni = (int)(N - i0 < NI ? N - i0 : NI);
    const long long nk = sm_rows_of(a.counts, (long long)k, N);
    const int nv = (int)(nk - i0 < 0 ? 0 : (nk - i0 < ni ? nk - i0 : ni));            // its valid observations: the first nv
    const ps_lds sm = ps_carve(pls_sm, reinterpret_cast<int*>(pls_sm + ps_lds_doubles(S, S2)), S, S2);
    double* Xs = pls_sm;                      // 64 x ldx      a tile of draws          (over the stage's arrays)
    double* As = Xs + PS_LOO_TR * ldx;        // 16 x lda      the tile's rows of A_k, zero-padded
    int* ys = reinterpret_cast<int*>(As + PS_LOO_NB * lda);     // 16 labels (in 16 doubles)
    double* ell = pls_sm + a.U;               // NI x S        l_si of the tile
    const size_t ks = k * (size_t)S, kn = k * (size_t)N + (size_t)i0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    // ---- (1) l_si of the tile's valid observations ------------------------------------------------------------------------
    if (nv > 0) {                             // (uniform in the workgroup)
        const double* Ak = a.A + kn * P;
        for (int e = l; e < PS_LOO_NB * lda; e += 256) {
            const int r = e / lda, j = e - r * lda;
            As[e] = r < nv && j < P ? Ak[(size_t)r * P + j] : 0.0;
        }
        if (l < PS_LOO_NB) ys[l] = l < nv ? a.labels[kn + l] : 0;
        const double* Xk = a.X + ks * D;
        const int wv = l >> 6, ln = l & 63, cc = ln & 15, kq = ln >> 4;
        for (int t0 = 0; t0 < S; t0 += PS_LOO_TR) {
            __syncthreads();                  // the previous tile's readers are done
            for (int e = l; e < PS_LOO_TR * ldx; e += 256) {
                const int r = e / ldx, j = e - r * ldx;
                Xs[e] = t0 + r < S && j < D ? Xk[(size_t)(t0 + r) * D + j] : 0.0;
            }
            __syncthreads();
            if (t0 + 16 * wv < S) {           // (wave-uniform)
                const double* px = Xs + (16 * wv + cc) * ldx + kq;
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
                        const int s = t0 + 16 * wv + kq + 4 * r;    // the draw; cc is the observation
                        sm_add_term(z[r], nt[r], exp(0.0 - m[r]));
                        const double rest = sm_rest(z[r], nt[r]);
                        if (s < S) ell[cc * S + s] = yok && fine[r] ? ey[r] - m[r] - sm_log_s(rest, 1.0 + rest) : qnan;
                    }
                }
            }
        }
    }
    __syncthreads();                          // l_si is published; the tiles are dead, the stage may take their place

    ps_loo_stage(a.o, sm, ell, ni, nv, nullptr, ks, kn, S, S2, M, l);     // (2)
}

hipError_t gsmvi_psis_loo_softmax_batched_prepare() { return gb_allow_lds(k_psis_loo_softmax_batched); }

extern "C" {

int gsmvi_psis_loo_softmax_tile(int C, int P, int64_t S) {
    if (!sm_shape_ok(C, P) || S < PS_MIN_S || S > PS_MAX_S) return 0;
    return pls_tile(C, P, (int)S);
}

int gsmvi_psis_loo_softmax_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int C, int P, int64_t N, int64_t S,
                                       const double* A, const int* labels, const int* counts_dev, const double* X,
                                       const double* logr, const double* lw, double* loglik, double* elpd, double* lpd,
                                       double* khat, double* ess, int* info) {
    const sm_model m = sm_model_of(K, N, C, P, A, labels, counts_dev);
    if (int st = sm_check_model(__func__, m, false, "N")) return st;
    const int D = m.D;
    GB_BAD(S < PS_MIN_S || S > PS_MAX_S, "S must be in [5, 4096]");
    GB_BAD(!A || !labels || !X || !logr || !lw || !elpd || !lpd || !khat || !ess || !info, "NULL array");
    GB_BAD(N > (INT64_MAX / 8 / S) / K, "K N S is too large");
    GB_BAD(N > (INT64_MAX / 8 / P) / K, "K N P is too large");
    const int NI = pls_tile(C, P, (int)S);
    const int64_t ntile = (N + NI - 1) / NI;
    GB_BAD(ntile > 16777215 / K,
           "K ceil(N / gsmvi_psis_loo_softmax_tile(C, P, S)) must be at most 2^24 - 1 (one tile per workgroup)");
    const size_t nn = (size_t)K * N * 8, ns = (size_t)K * S * 8;
    if (int st = gb_check_overlaps(__func__, m, {{X, ns * D, "X", GB_RD}, {logr, ns, "logr", GB_RD}, {lw, ns, "lw", GB_RD},
                                                 {loglik, nn * S, "loglik", GB_WR}, {elpd, nn, "elpd", GB_WR}, {lpd, nn, "lpd", GB_WR},
                                                 {khat, nn, "khat", GB_WR}, {ess, nn, "ess", GB_WR},
                                                 {info, (size_t)K * N * 4, "info", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    pls_args a = {};
    a.K = K; a.N = N; a.C = C; a.P = P; a.D = D;
    a.S = (int)S;
    ps_sizes(a.S, &a.S2, &a.M);
    a.NI = NI;
    a.U = ps_loo_region_doubles(pls_tiles_doubles(C, P), a.S, a.S2);
    a.ntile = (unsigned)ntile;
    a.A = A; a.labels = labels; a.counts = counts_dev;
    a.X = X;
    a.o = {logr, lw, loglik, elpd, lpd, khat, ess, info};
    const size_t lds = ((size_t)a.U + (size_t)NI * a.S) * sizeof(double);      // <= GB_LDS_MAX by the choice of NI
    const unsigned grid = (unsigned)(K * ntile);
    hipLaunchKernelGGL(k_psis_loo_softmax_batched, dim3(grid), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_SOFTMAX, "k_psis_loo_softmax_batched");
}

}  // extern "C"
