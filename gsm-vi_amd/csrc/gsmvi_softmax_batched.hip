// Batched softmax target: score and log-density of K Bayesian multinomial logit regressions of one (N, C, P), D = (C - 1) P <= 64,
// at nc points each, in one launch ("Batched softmax target").
//
// The reference's users hand the fits a model's log_prob and jit(grad(...)) of it (examples/example_gsm.py:34-35).  Here, for
// problem k with design matrix A_k (N rows a_n of P features), integer labels y_kn in 0 .. C - 1, n_k <= N valid rows and prior
// precision lam_k >= 0, class C - 1 the reference class with zero coefficients and x[c P + j] = W_cj, at the rows x of X_k:
//   eta_nc = a_n . w_c  (c < C-1),   eta_n,C-1 = 0
//   m_n    = max_c eta_nc            (over all C values, the 0 included)
//   s_n    = sum_{c=0..C-1} exp(eta_nc - m_n)     (class order; the reference class last)
//          = 1 + rest_n: the terms below 1 in that order, then the count of the terms that are 1 less one (sm_add_term)
//   lp(x)  = sum_{n<n_k} [ eta_n,y_n - m_n - log s_n ] - lam_k |x|^2 / 2     (log s_n as log1p(rest_n): sm_log_s; log(s_n) is 0
//                                                                            where rest_n < eps / 2)
//   g_cj   = sum_{n<n_k} ( [y_n = c] - exp(eta_nc - m_n)/s_n ) a_nj - lam_k x_cj      (c < C-1)
//   k_softmax_batched<NT, WANT> : WANT = SB_G (the score alone: no logarithm), SB_LP (the density alone: no second pass over
//                                 the tile), or both from one pass
// Work mapping: the slots of gsmvi_batched.h (gb_nt(D) threads per problem, four problems per 256-thread workgroup for D <= 16)
// and the two-pass tile of k_logistic_batched.  The launch walks the rows of X_k in tiles of tq = sb_tq(C, P) rows and, per such
// tile, the rows of A_k in tiles of SB_TN = 32.  A tile of A_k is staged in LDS once (row stride P | 1) and used twice: thread
// (n, q-group) forms the C - 1 dots of length P for its row n and each of its rows q of X, leaves them in its own cells of the
// residual block E (C - 1 cells per (q, n), stride 33 between classes), takes m, s and the density's term, and rewrites the cells
// as r_qnc = [y = c] - exp(eta - m) / s; then thread (q, c, j) owns up to MAXO outputs g_qcj and sums r_qnc A_nj over the tile's
// rows in order.  The next tile of A_k (and of its labels) is loaded into registers right after the barrier that publishes the
// current one and is written to LDS only after the current one is consumed.
// LDS budget, in doubles per problem:
//   32 (P | 1)  the A tile  +  32  its labels (ints)  +  tq [ (D | 1)  the row of X  +  1  its flag  +  33 (C - 1)  E  +  33  the density's terms ]
// The block E is C - 1 times the logistic kernel's, so tq is derived from (C, P) by sb_tq: the largest number of rows -- at most 32
// (16 in the four-problem packing), and at most SB_MAXO NT / D, the outputs the score pass has registers for -- for which the sum
// stays within 64 KB / (problems per workgroup), the limit a kernel has without asking for more (below the 160 KB the batched
// context allows): 32 rows at (C, P) = (2, 17), 16 at (2, 64) and (9, 8), 12 at (17, 4), 6 at (33, 2), 3 at (65, 1); 16 at
// (2, 16), 10 at (5, 4), 3 at (17, 1).  The worst case leaves 3 rows, so every shape in bounds has a tile.
// Order: every output row (k, q) sums over n = 0 .. n_k - 1 in that order in one thread, and every (q, n) term is computed by one
// thread from A_n, y_n and row q alone, so the bits do not depend on K, nc, tq or the slot packing.  Rows n >= n_k are never
// loaded.  A row of X with a non-finite entry, or for which some valid eta is not finite, gets NaN outputs (by a flag, not by
// arithmetic).  The maximum is subtracted, so exp cannot overflow and s >= 1.  A label is used in comparisons and selects only,
// never as an index.  A slot reads and writes only its own problem's slices and every slot runs the same barriers (2 + 3 ceil(N /
// 32) per tile of X rows).  All inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_softmax_model.h"
#include "../../include/gsmvi_hip.h"
#include "../../include/gsmvi_hip_debug.h"   // gsmvi_debug_softmax_batched_lds
#include <cstdint>
#include <type_traits>

#define SB_TN 32           // rows of A_k per tile
#define SB_AQ 8            // tile elements per thread: SB_TN P / NT <= 8 in both packings
#define SB_MAXO 4          // outputs g_qcj per thread in the score pass (8 take the 256-thread kernels past 256 registers)
#define SB_G 1
#define SB_LP 2
#define SB_LDS (64 * 1024) // dynamic LDS of a launch: what a kernel may request without an attribute

struct sb_args {
    long long K, N;
    int C, P, D, nc, tqm;       // classes, features, (C - 1) P, rows of X per problem, rows of X held in LDS = min(nc, tq)
    const double* A;            // (K, N, P)
    const int* labels;          // (K, N)
    const int* counts;          // (K) valid rows, clamped to 0 .. N (null: N)
    double lam;                 // the prior precision of every problem ...
    const double* lam_dev;      // ... or (K) per-problem values on the device (null: `lam`)
    const double* X;            // (K, nc, D)
    double* G;                  // (K, nc, D) or null
    double* lp;                 // (K, nc) or null
};

// LDS doubles per problem at tq rows of X (the formula above; the density's terms only when wanted)
__host__ __device__ inline int sb_lds_doubles(int C, int P, int tq, int want) {
    const int D = (C - 1) * P;
    return SB_TN * (P | 1) + SB_TN + tq * ((D | 1) + 1 + (SB_TN | 1) * ((C - 1) + (want & SB_LP ? 1 : 0)));
}

// rows of X per tile: at most 32 (16 in the four-problem packing), at most SB_MAXO outputs per thread in the score pass, and within
// the LDS budget, which is taken with the density's terms, so that the three variants of a shape walk the same tiles
static inline int sb_tq(int C, int P) {
    const int D = (C - 1) * P, nt = gb_nt(D), ppw = 256 / nt;
    const int rows = nt == 256 ? 32 : 16, outs = SB_MAXO * nt / D, cap = rows < outs ? rows : outs;
    const int budget = SB_LDS / 8 / ppw - (SB_TN * (P | 1) + SB_TN);
    const int tq = budget / ((D | 1) + 1 + (SB_TN | 1) * C);
    return tq < cap ? tq : cap;
}

// f(integral_constant<int, n>) for the runtime n in 1 .. MAX: the score pass runs with a compile-time number of outputs per
// thread (the same device as lb_rows of k_logistic_batched)
template <int Q, int MAX, typename F>
__device__ __forceinline__ void sb_rows(int n, F&& f) {
    if constexpr (Q >= MAX) {
        f(std::integral_constant<int, MAX>{});
    } else {
        if (n == Q)
            f(std::integral_constant<int, Q>{});
        else
            sb_rows<Q + 1, MAX>(n, f);
    }
}

template <int NT, int WANT>
__global__ __launch_bounds__(256, 2) void k_softmax_batched(sb_args a) {
    extern __shared__ double sb_sm[];
    constexpr int PPW = 256 / NT;
    constexpr int NG = NT / SB_TN;                      // eta pass: NG groups of 32 threads
    constexpr int MAXO = SB_MAXO;                       // score pass: outputs per thread, tq D <= SB_MAXO NT (sb_tq)
    constexpr bool HAS_G = (WANT & SB_G) != 0, HAS_LP = (WANT & SB_LP) != 0;
    const int P = a.P, Cm = a.C - 1, D = a.D, lda = P | 1, ld = D | 1, ldr = SB_TN | 1, tqm = a.tqm;
    const long long N = a.N;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;               // a tail slot runs every barrier and nothing else
    double* As = sb_sm + (size_t)slot * sb_lds_doubles(a.C, P, tqm, WANT);
    int* Ys = reinterpret_cast<int*>(As + SB_TN * lda);   // 32 labels of the tile's rows (in 32 doubles)
    double* Xs = As + SB_TN * lda + SB_TN;    // tqm x ld          the rows of X
    double* Rb = Xs + tqm * ld;               // tqm               0, or NaN for a flagged row of X
    double* Es = Rb + tqm;                    // tqm x Cm x ldr    eta, then exp(eta - m), then r
    double* Ts = Es + tqm * Cm * ldr;         // tqm x ldr         the density's terms
    const size_t kk = (size_t)(valid ? k : 0);
    const double* Ak = a.A + kk * (size_t)N * P;
    const int* yk = a.labels + kk * (size_t)N;
    const double* Xk = a.X + kk * (size_t)a.nc * D;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    // (the statements of sm_problem_of, written out: built on the helper the six instantiations got other instructions and did
    // not meet the speed bound; gsmvi_softmax_model.h names this kernel as the exception, DESIGN.md has the numbers)
    long long nk = 0;                         // the rows that count
    double lam = 0.0;
    if (valid) {
        nk = N;
        if (a.counts) {
            const long long c = a.counts[k];
            nk = c < 0 ? 0 : (c > N ? N : c);
        }
        lam = a.lam_dev ? a.lam_dev[k] : a.lam;
    }
    // the tile elements e = l + q NT of this thread as (row, column), stepped without a division
    const int row0 = l / P, col0 = l - row0 * P, dr = NT / P, dc = NT - dr * P;
    const int en = l % SB_TN, eg = l / SB_TN; // the eta pass: row en of the tile, rows eg + i NG of X

    for (int c0 = 0; c0 < a.nc; c0 += tqm) {
        const int tq = a.nc - c0 < tqm ? a.nc - c0 : tqm;
        const int nout = tq * D;              // outputs of this tile of X rows: o = q D + c P + j
        if (valid)
            for (int e = l; e < nout; e += NT) {
                const int r = e / D, j = e - r * D;
                Xs[r * ld + j] = Xk[(size_t)(c0 + r) * D + j];
            }
        // the first tile of A_k and of the labels into registers
        double pre[SB_AQ];
        int ypre = 0;
        {
            const int tnv = (int)(nk < SB_TN ? nk : SB_TN), te = tnv * P;
#pragma unroll
            for (int q = 0; q < SB_AQ; ++q) {
                const int e = l + q * NT;
                pre[q] = e < te ? Ak[e] : 0.0;
            }
            if (l < tnv) ypre = yk[l];
        }
        __syncthreads();
        double xx = 0.0;                      // |x|^2 of row l (threads l < tq)
        if (valid && l < tq) {
            double z = 0.0;
            for (int j = 0; j < D; ++j) {
                const double x = Xs[l * ld + j];
                z += x * 0.0;
                xx += x * x;
            }
            Rb[l] = z;
        }

        // the score pass: output o = l + i NT of this thread -> its cells of E and its column of the A tile
        double acc[MAXO], lpacc = 0.0;
        int ro[MAXO], ao[MAXO];
#pragma unroll
        for (int i = 0; i < MAXO; ++i) {
            acc[i] = 0.0;
            const int o = l + i * NT < nout ? l + i * NT : 0, q = o / D, d = o - q * D, c = d / P;
            ro[i] = (q * Cm + c) * ldr;
            ao[i] = d - c * P;
        }
        const int no = (nout - l + NT - 1) / NT;      // outputs of this thread
        const int nom = (nout + NT - 1) / NT;         // ... and of thread 0 (uniform in the slot)

        for (long long n0 = 0; n0 < N; n0 += SB_TN) {
            const long long left = nk - n0;
            const int tnv = left < 0 ? 0 : (int)(left < SB_TN ? left : SB_TN), te = tnv * P;
            {                                 // registers -> LDS (the previous tile was consumed before the last barrier)
                int r = row0, c = col0;
#pragma unroll
                for (int q = 0; q < SB_AQ; ++q) {
                    if (l + q * NT < te) As[r * lda + c] = pre[q];
                    r += dr;
                    c += dc;
                    if (c >= P) {
                        c -= P;
                        ++r;
                    }
                }
                if (l < tnv) Ys[l] = ypre;
            }
            __syncthreads();
            {                                 // the next tile's loads: in flight while this one is consumed
                const long long left2 = left - SB_TN;
                const int tnv2 = left2 < 0 ? 0 : (int)(left2 < SB_TN ? left2 : SB_TN), te2 = tnv2 * P;
                const double* An = Ak + (size_t)(n0 + SB_TN) * P;
#pragma unroll
                for (int q = 0; q < SB_AQ; ++q) {
                    const int e = l + q * NT;
                    if (e < te2) pre[q] = An[e];
                }
                if (l < tnv2) ypre = yk[n0 + SB_TN + l];
            }
            if (en < tnv) {                   // eta, m, s, the residuals and the density's term of (q, en)
                const double* ar = As + en * lda;
                const int yv = Ys[en];
#pragma unroll 1
                for (int q = eg; q < tq; q += NG) {
                    const double* xr = Xs + q * ld;
                    double* er = Es + q * Cm * ldr + en;
                    double m = 0.0, etay = 0.0;       // the reference class: eta = 0
                    bool fine = true;
#pragma unroll 1
                    for (int c = 0; c < Cm; ++c) {
                        double eta = 0.0;
#pragma unroll 4
                        for (int j = 0; j < P; ++j) eta = fma(ar[j], xr[c * P + j], eta);
                        er[c * ldr] = eta;
                        fine = fine && gb_finite(eta);
                        m = fmax(m, eta);
                        etay = c == yv ? eta : etay;
                    }
                    double rest = 0.0, nt = 0.0;      // s = 1 + rest: the terms below 1, and the count of those that are 1 (sm_add_term)
#pragma unroll 1
                    for (int c = 0; c < Cm; ++c) {
                        const double e = exp(er[c * ldr] - m);
                        sm_add_term(rest, nt, e);
                        if (HAS_G) er[c * ldr] = e;
                    }
                    sm_add_term(rest, nt, exp(0.0 - m));
                    rest = sm_rest(rest, nt);
                    const double s = 1.0 + rest;
                    if (HAS_G)
#pragma unroll 2
                        for (int c = 0; c < Cm; ++c) er[c * ldr] = (c == yv ? 1.0 : 0.0) - er[c * ldr] / s;
                    if (HAS_LP) Ts[q * ldr + en] = etay - m - sm_log_s(rest, s);
                    if (!fine) Rb[q] = qnan;          // (any number of threads, the same value)
                }
            }
            __syncthreads();
            if (HAS_G && no > 0) {            // g_qcj += sum over the tile's rows, in order
                sb_rows<1, MAXO>(nom, [&](auto nr) {
#pragma unroll 2
                    for (int n = 0; n < tnv; ++n) {
                        const double* an = As + n * lda;
#pragma unroll
                        for (int i = 0; i < decltype(nr)::value; ++i) acc[i] = fma(Es[ro[i] + n], an[ao[i]], acc[i]);
                    }
                });
            }
            if (HAS_LP && l < tq && valid)
                for (int n = 0; n < tnv; ++n) lpacc += Ts[l * ldr + n];
            __syncthreads();                  // the next tile overwrites As, Ys, Es, Ts
        }

        if (valid) {
            if (HAS_G) {
#pragma unroll
                for (int i = 0; i < MAXO; ++i) {
                    const int o = l + i * NT;
                    if (o < nout) {
                        const int q = o / D, d = o - q * D;
                        const double v = acc[i] - lam * Xs[q * ld + d];
                        a.G[(kk * (size_t)a.nc + (size_t)(c0 + q)) * D + d] = Rb[q] == 0.0 ? v : qnan;
                    }
                }
            }
            if (HAS_LP && l < tq) a.lp[kk * (size_t)a.nc + (size_t)(c0 + l)] = Rb[l] == 0.0 ? lpacc - 0.5 * lam * xx : qnan;
        }
        __syncthreads();                      // the next tile of X rows overwrites Xs and Rb
    }
}

// dynamic LDS bytes of a launch at (C, P, nc, want): at most SB_LDS
static size_t sb_launch_lds(int C, int P, int nc, int want, int* ppw, int* tqm) {
    const int tq = sb_tq(C, P);
    *ppw = 256 / gb_nt((C - 1) * P);
    *tqm = nc < tq ? nc : tq;
    return (size_t)*ppw * sb_lds_doubles(C, P, *tqm, want) * sizeof(double);
}

extern "C" {

int gsmvi_softmax_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int C, int P, int nc, int64_t N, const double* A,
                              const int* labels, const int* counts_dev, double prior_prec, const double* prior_prec_dev,
                              const double* X, double* G, double* lp) {
    const sm_model m = sm_model_of(K, N, C, P, A, labels, counts_dev, prior_prec, prior_prec_dev);
    if (int st = sm_check_model(__func__, m, true, "N")) return st;
    const int D = m.D;
    GB_BAD(nc < 1, "nc must be at least 1");
    GB_BAD(nc > (INT64_MAX / 8 / D) / K, "K nc D is too large");
    GB_BAD(!A || !labels || !X, "NULL array");
    GB_BAD(!G && !lp, "give G or lp (or both)");
    const size_t nx = (size_t)K * nc * D * 8;
    if (int st = gb_check_overlaps(__func__, m, {{X, nx, "X", GB_RD}, {G, nx, "G", GB_WR}, {lp, (size_t)K * nc * 8, "lp", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    const int want = (G ? SB_G : 0) | (lp ? SB_LP : 0);
    sb_args a = {K, N, C, P, D, nc, 0, A, labels, counts_dev, prior_prec, prior_prec_dev, X, G, lp};
    int ppw;
    const size_t lds = sb_launch_lds(C, P, nc, want, &ppw, &a.tqm);
    const unsigned grid = (unsigned)((K + ppw - 1) / ppw);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define SB_GO(NTV)                                                                                         \
    do {                                                                                                   \
        if (want == SB_G) hipLaunchKernelGGL((k_softmax_batched<NTV, SB_G>), dim3(grid), dim3(256), lds, st, a);             \
        else if (want == SB_LP) hipLaunchKernelGGL((k_softmax_batched<NTV, SB_LP>), dim3(grid), dim3(256), lds, st, a);      \
        else hipLaunchKernelGGL((k_softmax_batched<NTV, SB_G | SB_LP>), dim3(grid), dim3(256), lds, st, a);                  \
    } while (0)
    if (ppw == 4)
        SB_GO(64);
    else
        SB_GO(256);
#undef SB_GO
    return gb_launched(ctx, GSMVI_PATH_BATCHED_SOFTMAX, "k_softmax_batched");
}

// include/gsmvi_hip_debug.h: what a launch at (C, P, nc) requests (exported by the debug library only); want: 1 = G, 2 = lp, 3 = both
int gsmvi_debug_softmax_batched_lds(int C, int P, int nc, int want, size_t* bytes, int* problems_per_workgroup, int* x_rows_per_tile) {
    GB_BAD(!sm_shape_ok(C, P) || nc < 1 || want < 1 || want > 3 || !bytes || !problems_per_workgroup || !x_rows_per_tile,
           "bad shape, want or NULL output");
    int tqm;
    *bytes = sb_launch_lds(C, P, nc, want, problems_per_workgroup, &tqm);
    *x_rows_per_tile = sb_tq(C, P);
    return GSMVI_OK;
}

}  // extern "C"
