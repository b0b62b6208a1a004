// Batched ordinal target: score and log-density of K cumulative-logit (proportional odds) regressions of one (N, P, C) at nc points
// each, in one launch ("Batched ordinal target").
//
// The reference's users hand the fits a model's log_prob and jit(grad(...)) of it (examples/example_gsm.py:34-35).  Here, for
// problem k with design matrix A_k (N rows a_n of length P, no intercept column), labels y_kn in 0 .. C - 1, an optional offset
// o_kn, n_k <= N valid rows, at the rows x = (beta, delta) of X_k (length D = P + C - 1 <= 64):
//   cut_0 = delta_0,   cut_j = cut_{j-1} + e^{delta_j}  (j = 1 .. C - 2),   eta_n = a_n . beta + o_n
//   lp(x)      = sum_{n < n_k} t_n - lam_k |beta|^2 / 2 - kap_k |delta|^2 / 2
//   g(x)[:P]   = sum_{n < n_k} r_eta,n a_n - lam_k beta
//   gcut_j     = sum_{n < n_k} ([y_n = j + 1] u_lo,n + [y_n = j] u_hi,n)                       (j = 0 .. C - 2)
//   g(x)[P]    = sum_{j >= 0} gcut_j - kap_k delta_0
//   g(x)[P+i]  = e^{delta_i} sum_{j >= i} gcut_j - kap_k delta_i                               (i = 1 .. C - 2)
// with (t, r_eta, u_lo, u_hi) of gsmvi_ordinal_link.h.  The model has C - 1 extra parameters and every observation sends residuals
// to two of them, chosen by its label, so it is a kernel of its own and not one more lb_link<FAM> of k_logistic_batched.  It is the
// sibling of k_negbin_batched, whose work mapping and promises it keeps:
//   k_ordinal_batched<NT, WANT, OFF> : WANT = LB_G, LB_LP or both from one pass; OFF: the launch carries the offset's tile
// The slots of gsmvi_batched.h (gb_nt(D) threads per problem, four problems per 256-thread workgroup for D <= 16).  The launch
// walks the rows of X_k in tiles of TC (32; 16 in the four-problem packing) and, per such tile, the rows of A_k in tiles of
// LB_TN = 32, so neither nc nor N is bounded by LDS.  Per tile of X rows a prologue leaves, for every row and class, cut_j,
// e^{delta_j}, log1mexp(e^{delta_j}) and 1 / expm1(e^{delta_j}) in LDS (the last three by all threads, then the cutpoints as one
// chain in j per row).  A tile of A_k is staged in LDS once (row stride P | 1) and used twice: thread (n, c-group) forms eta for its
// row n and up to CQ rows of X, applies the link and leaves r_eta, u_lo, u_hi (and t) in LDS (row stride 33); then thread (c, j)
// owns the output component j of up to MAXQ rows c: for j < P it sums r_eta,cn A_nj over the tile's rows in order, for j >= P it
// sums u_lo,cn where y_n = j - P + 1 and u_hi,cn where y_n = j - P (the same chain with 1.0 or 0.0 in the place of A_nj).  The
// next tile of A_k (and of y_k, o_k) is loaded into registers right after the barrier that publishes the current one.  The epilogue
// publishes gcut through LDS and thread (c, P + i) sums it from j = C - 2 down to i and applies the e^{delta_i} factor.
// Order: every output row (k, c) sums over n = 0 .. n_k - 1 in that order in one thread, so it does not depend on K, nc, the
// tiling of nc or the slot packing.  Rows n >= n_k are never loaded.  A label is clamped to 0 .. C - 1 when its tile is staged, so
// it indexes nothing out of bounds (the range is the caller's to keep).  A row of X with a non-finite entry, or in which some
// e^{delta_j}, j >= 1, is not a positive normal number, gets NaN outputs by a flag.  A slot reads and writes only its own problem's
// slices and every slot runs the same barriers, so nothing crosses between problems.  No atomics; all inputs are only read; no
// context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_glm_model.h"                 // LB_G / LB_LP, LB_TN
#include "gsmvi_ordinal_link.h"
#include "../../include/gsmvi_hip.h"
#include "../../include/gsmvi_hip_debug.h"   // gsmvi_debug_ordinal_batched_lds
#include <cstdint>
#include <type_traits>

#define OB_AQ 8    // tile elements per thread: LB_TN P / NT <= 8 in both packings

struct ob_args {
    long long K, N;
    int P, C, nc, tcm;          // columns of A, classes (D = P + C - 1), rows of X per problem, rows of X held in LDS = min(nc, TC)
    const double* A;            // (K, N, P)
    const int* y;               // (K, N) labels
    const double* offset;       // (K, N) added to eta, or null
    const int* counts;          // (K) valid rows, clamped to 0 .. N (null: N)
    double lam;                 // the prior precision of beta of every problem ...
    const double* lam_dev;      // ... or (K) per-problem values on the device (null: `lam`)
    double kap;                 // the prior precision of delta ...
    const double* kap_dev;      // ... or (K)
    const double* X;            // (K, nc, D)
    double* G;                  // (K, nc, D) or null
    double* lp;                 // (K, nc) or null
};

__host__ __device__ inline int ob_tc(int NT) { return NT == 256 ? 32 : 16; }
// LDS doubles per problem: the A tile (32 x (P | 1)) + its labels (32 ints) + its offset (32, when one is given) + the X tile
// (tcm x (D | 1)) + the row flags (tcm) + cut, e^delta, log1mexp and 1 / expm1 (tcm x (C - 1) each) + r_eta, u_lo and u_hi
// (tcm x 33 each, with G) + t (tcm x 33, with lp).
// (C = 64, P = 1, 32 rows, both, offset): 14480 doubles, 113.1 KB, the most; four problems of (C = 16, P = 1, 16 rows, both,
// offset): 4 x 3440 doubles, 107.5 KB
__host__ __device__ inline int ob_lds_doubles(int P, int C, int tcm, int want, bool off) {
    const int D = P + C - 1;
    return LB_TN * (P | 1) + LB_TN / 2 + (off ? LB_TN : 0) +
           tcm * ((D | 1) + 1 + 4 * (C - 1) + (LB_TN | 1) * ((want & LB_G ? 3 : 0) + (want & LB_LP ? 1 : 0)));
}

// f(integral_constant<int, n>) for the runtime n in 1 .. MAX (as nb_rows of gsmvi_negbin_batched.hip): the two inner loops run
// with a compile-time number of rows of X per thread
template <int Q, int MAX, typename F>
__device__ __forceinline__ void ob_rows(int n, F&& f) {
    if constexpr (Q >= MAX) {
        f(std::integral_constant<int, MAX>{});
    } else {
        if (n == Q)
            f(std::integral_constant<int, Q>{});
        else
            ob_rows<Q + 1, MAX>(n, f);
    }
}

template <int NT, int WANT, bool OFF>
__global__ __launch_bounds__(256) void k_ordinal_batched(ob_args a) {
    extern __shared__ double ob_sm[];
    constexpr int PPW = 256 / NT, TC = NT == 256 ? 32 : 16;
    constexpr int NG = NT / LB_TN, CQ = TC / NG;        // eta pass: NG groups of 32 threads, CQ rows of X per thread
    constexpr int MAXQ = TC / 4;                        // score pass: rows of X per thread (NT / D >= 4 rows side by side)
    constexpr bool HAS_G = (WANT & LB_G) != 0, HAS_LP = (WANT & LB_LP) != 0;
    const int P = a.P, C = a.C, lc = C - 1, D = P + lc, lda = P | 1, ld = D | 1, ldr = LB_TN | 1, tcm = a.tcm;
    const long long N = a.N;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;               // a tail slot runs every barrier and nothing else
    double* As = ob_sm + (size_t)slot * ob_lds_doubles(P, C, tcm, WANT, OFF);
    int* Yi = reinterpret_cast<int*>(As + LB_TN * lda);      // 32 ints    the labels of the tile's rows, clamped to 0 .. C - 1
    double* Os = As + LB_TN * lda + LB_TN / 2;               // 32         their offsets, when given
    double* Xs = Os + (OFF ? LB_TN : 0);      // tcm x ld   the rows of X
    double* Rb = Xs + tcm * ld;               // tcm        0, or NaN for a flagged row of X
    double* Ct = Rb + tcm;                    // tcm x lc   the cutpoints of the row
    double* Ws = Ct + tcm * lc;               // tcm x lc   e^{delta_j}, j >= 1 (entry 0: 1.0)
    double* Lm = Ws + tcm * lc;               // tcm x lc   log1mexp(e^{delta_j}), j >= 1; gcut in the epilogue
    double* Qe = Lm + tcm * lc;               // tcm x lc   1 / expm1(e^{delta_j}), j >= 1
    double* Rs = Qe + tcm * lc;               // tcm x ldr  r_eta
    double* Ul = Rs + (HAS_G ? tcm * ldr : 0);   // tcm x ldr  u_lo
    double* Uh = Ul + (HAS_G ? tcm * ldr : 0);   // tcm x ldr  u_hi
    double* Ts = Uh + (HAS_G ? tcm * ldr : 0);   // tcm x ldr  t
    const size_t kk = (size_t)(valid ? k : 0);
    const double* Ak = a.A + kk * (size_t)N * P;
    const int* yk = a.y + kk * (size_t)N;
    // lane l < 32 carries the label of the tile's row l, lane 32 + l its offset
    const int ol = l - LB_TN;
    const double* ok = OFF ? a.offset + kk * (size_t)N : nullptr;
#define OB_OLANE(t) (OFF && ol >= 0 && ol < (t))
    const double* Xk = a.X + kk * (size_t)a.nc * D;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    long long nk = 0;                         // the rows that count
    double lam = 0.0, kap = 0.0;
    if (valid) {
        nk = N;
        if (a.counts) {
            const long long c = a.counts[k];
            nk = c < 0 ? 0 : (c > N ? N : c);
        }
        lam = a.lam_dev ? a.lam_dev[k] : a.lam;
        kap = a.kap_dev ? a.kap_dev[k] : a.kap;
    }
    // the tile elements e = l + q NT of this thread as (row, column) of the A tile, stepped without a division
    const int row0 = l / P, col0 = l - row0 * P, dr = NT / P, dc = NT - dr * P;
    // the eta pass: row en of the tile, rows eg + q NG of X;  the score pass: component gj of the output, rows gc0 + q CW of X
    const int en = l % LB_TN, eg = l / LB_TN;
    const int CW = NT / D, gc0 = l / D, gj = l - gc0 * D;
    const bool gact = l < CW * D, gcut = gj >= P;
    const int gja = gcut ? 0 : gj;            // the column of A this thread reads (a component j >= P reads none)
    const int jc = gj - P;                    // the cutpoint of a component j >= P
    const int rst = tcm * ldr;                // the stride from r_eta to u_lo and from u_lo to u_hi

    for (int c0 = 0; c0 < a.nc; c0 += TC) {
        const int tc = a.nc - c0 < TC ? a.nc - c0 : TC;
        if (valid)
            for (int e = l; e < tc * D; e += NT) {
                const int r = e / D, j = e - r * D;
                Xs[r * ld + j] = Xk[(size_t)(c0 + r) * D + j];
            }
        // the first tile of A_k, y_k and o_k into registers
        double pre[OB_AQ], opre = 0.0;
        int ypre = 0;
        {
            const int tnv = (int)(nk < LB_TN ? nk : LB_TN), te = tnv * P;
#pragma unroll
            for (int q = 0; q < OB_AQ; ++q) {
                const int e = l + q * NT;
                pre[q] = e < te ? Ak[e] : 0.0;
            }
            if (l < tnv) ypre = yk[l];
            if (OB_OLANE(tnv)) opre = ok[ol];
        }
        __syncthreads();
        // the prologue: the gap terms of every (row, class j >= 1) by all threads ...
        if (valid)
            for (int e = l; e < tc * lc; e += NT) {
                const int r = e / lc, j = e - r * lc;
                double w = 1.0, lm = 0.0, qe = 0.0;
                if (j >= 1) {
                    w = exp(Xs[r * ld + P + j]);          // (a NaN delta gives a NaN w: flagged)
                    ord_gap(w, lm, qe);
                }
                Ws[e] = w;
                Lm[e] = lm;
                Qe[e] = qe;
            }
        __syncthreads();
        // ... then row l (threads l < tc): |beta|^2, |delta|^2, the flag and the cutpoints as one chain in j
        double bb = 0.0, dd = 0.0;
        if (valid && l < tc) {
            double z = 0.0;
            for (int j = 0; j < P; ++j) {
                const double x = Xs[l * ld + j];
                z += x * 0.0;
                bb += x * x;
            }
            double cut = 0.0;
            bool okw = true;
            for (int j = 0; j < lc; ++j) {
                const double x = Xs[l * ld + P + j];
                z += x * 0.0;
                dd += x * x;
                if (j == 0) {
                    cut = x;
                } else {
                    const double w = Ws[l * lc + j];
                    okw = okw && w >= 2.2250738585072014e-308 && w < __builtin_huge_val();
                    cut += w;
                }
                Ct[l * lc + j] = cut;
            }
            Rb[l] = okw ? z : qnan;
        }

        double acc[MAXQ], lpacc = 0.0;
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) acc[q] = 0.0;
        const int nq = (tc + CW - 1) / CW;    // rows of X per thread in the score pass and in the eta pass (uniform in the slot)
        const int nqe = (tc + NG - 1) / NG;

        // one problem per workgroup: the walk ends with the rows that count.  Packed slots walk all N, dead tiles included, since
        // their barriers are shared and n_k differs between them (a dead tile stages and sums nothing)
        const long long nend = PPW == 1 ? nk : N;
        for (long long n0 = 0; n0 < nend; n0 += LB_TN) {
            const long long left = nk - n0;
            const int tnv = left < 0 ? 0 : (int)(left < LB_TN ? left : LB_TN), te = tnv * P;
            {                                 // registers -> LDS (the previous tile was consumed before the last barrier)
                int r = row0, c = col0;
#pragma unroll
                for (int q = 0; q < OB_AQ; ++q) {
                    if (l + q * NT < te) As[r * lda + c] = pre[q];
                    r += dr;
                    c += dc;
                    if (c >= P) {
                        c -= P;
                        ++r;
                    }
                }
                if (l < tnv) Yi[l] = ypre < 0 ? 0 : (ypre > lc ? lc : ypre);
                if (OB_OLANE(tnv)) Os[ol] = opre;
            }
            __syncthreads();                  // (also publishes Ct, Ws, Lm and Qe of this tile of X rows)
            {                                 // the next tile's loads: in flight while this one is consumed
                const long long left2 = left - LB_TN;
                const int tnv2 = left2 < 0 ? 0 : (int)(left2 < LB_TN ? left2 : LB_TN), te2 = tnv2 * P;
                const double* An = Ak + (size_t)(n0 + LB_TN) * P;
#pragma unroll
                for (int q = 0; q < OB_AQ; ++q) {
                    const int e = l + q * NT;
                    if (e < te2) pre[q] = An[e];
                }
                if (l < tnv2) ypre = yk[n0 + LB_TN + l];
                if (OB_OLANE(tnv2)) opre = ok[n0 + LB_TN + ol];
            }
            if (en < tnv && eg < tc) {        // eta, the link
                double eta[CQ];
                int xo[CQ];
#pragma unroll
                for (int q = 0; q < CQ; ++q) {
                    eta[q] = 0.0;
                    const int c = eg + q * NG;
                    xo[q] = (c < tc ? c : tc - 1) * ld;
                }
                const double* ar = As + en * lda;
                ob_rows<1, CQ>(nqe, [&](auto nr) {
#pragma unroll 8
                    for (int j = 0; j < P; ++j) {
                        const double av = ar[j];
#pragma unroll
                        for (int q = 0; q < decltype(nr)::value; ++q) eta[q] = fma(av, Xs[xo[q] + j], eta[q]);
                    }
                });
                if (OFF) {
                    const double ov = Os[en];
#pragma unroll
                    for (int q = 0; q < CQ; ++q) eta[q] += ov;
                }
                // eta goes through this thread's own LDS cells, so that the link below is ONE copy in a rolled loop
                double* Es = HAS_G ? Rs : Ts;
#pragma unroll
                for (int q = 0; q < CQ; ++q)
                    if (eg + q * NG < tc) Es[(eg + q * NG) * ldr + en] = eta[q];
                const int yv = Yi[en];
#pragma unroll 1
                for (int c = eg; c < tc; c += NG) {
                    double re = 0.0, ulo = 0.0, uhi = 0.0, t = 0.0;
                    ord_link<HAS_G, HAS_LP>(Es[c * ldr + en], yv, C, Ct + c * lc, Lm + c * lc, Qe + c * lc, re, ulo, uhi, t);
                    if (HAS_G) {
                        Rs[c * ldr + en] = re;
                        Ul[c * ldr + en] = ulo;
                        Uh[c * ldr + en] = uhi;
                    }
                    if (HAS_LP) Ts[c * ldr + en] = t;
                }
            }
            __syncthreads();
            if (HAS_G && gact && gc0 < tc) {  // g_cj += sum over the tile's rows, in order
                int ro[MAXQ];
#pragma unroll
                for (int q = 0; q < MAXQ; ++q) {
                    const int c = gc0 + q * CW;
                    ro[q] = (c < tc ? c : tc - 1) * ldr;
                }
                ob_rows<1, MAXQ>(nq, [&](auto nr) {
#pragma unroll 8
                    for (int n = 0; n < tnv; ++n) {
                        const int yn = Yi[n];
                        const bool hlo = yn == jc + 1, hhi = yn == jc;
                        const double al = As[n * lda + gja];
                        // a component j >= P takes u_lo of the rows labelled j - P + 1 and u_hi of the rows labelled j - P
                        // (Rs, Ul and Uh follow each other at a stride of rst doubles)
                        const double* Rg = Rs + (gcut ? (hlo ? rst : 2 * rst) : 0) + n;
                        const double av = gcut ? (hlo || hhi ? 1.0 : 0.0) : al;
#pragma unroll
                        for (int q = 0; q < decltype(nr)::value; ++q) acc[q] = fma(Rg[ro[q]], av, acc[q]);
                    }
                });
            }
            if (HAS_LP && l < tc && valid)
                for (int n = 0; n < tnv; ++n) lpacc += Ts[l * ldr + n];
            __syncthreads();                  // the next tile overwrites As, Yi, Os, Rs, Ul, Uh, Ts
        }

        if (HAS_G) {                          // gcut through LDS (Lm: the last link has run), for the suffix sums; the barrier
                                              // also publishes Rb and Ws where n_k = 0 left the walk without one
            if (valid && gact && gcut) {
#pragma unroll
                for (int q = 0; q < MAXQ; ++q) {
                    const int c = gc0 + q * CW;
                    if (c < tc) Lm[c * lc + jc] = acc[q];
                }
            }
            __syncthreads();
        }
        if (valid) {
            if (HAS_G && gact) {
#pragma unroll
                for (int q = 0; q < MAXQ; ++q) {
                    const int c = gc0 + q * CW;
                    if (c < tc) {
                        const double x = Xs[c * ld + gj];
                        double v;
                        if (gcut) {
                            double s = 0.0;
                            for (int j = lc - 1; j >= jc; --j) s += Lm[c * lc + j];
                            v = jc == 0 ? s - kap * x : Ws[c * lc + jc] * s - kap * x;
                        } else {
                            v = acc[q] - lam * x;
                        }
                        a.G[(kk * (size_t)a.nc + (size_t)(c0 + c)) * D + gj] = Rb[c] == 0.0 ? v : qnan;
                    }
                }
            }
            if (HAS_LP && l < tc)
                a.lp[kk * (size_t)a.nc + (size_t)(c0 + l)] = Rb[l] == 0.0 ? (lpacc - 0.5 * lam * bb) - 0.5 * kap * dd : qnan;
        }
        __syncthreads();                      // the next tile of X rows overwrites Xs, Rb, Ct, Ws, Lm and Qe
    }
#undef OB_OLANE
}

// dynamic LDS bytes of a launch at (P, C, nc, want, offset): up to 113.1 KB (one problem of C = 64 with both outputs), above the
// 64 KB a kernel gets without an attribute, so gsmvi_ordinal_batched_prepare raises the limit of every instantiation
static size_t ob_launch_lds(int P, int C, int nc, int want, bool off, int* ppw, int* tcm) {
    const int nt = gb_nt(P + C - 1), tc = ob_tc(nt);
    *ppw = 256 / nt;
    *tcm = nc < tc ? nc : tc;
    return (size_t)*ppw * ob_lds_doubles(P, C, *tcm, want, off) * sizeof(double);
}

#define OB_EACH(NTV, W) k_ordinal_batched<NTV, W, false>, k_ordinal_batched<NTV, W, true>
hipError_t gsmvi_ordinal_batched_prepare() {
    return gb_allow_lds(OB_EACH(64, LB_G), OB_EACH(64, LB_LP), OB_EACH(64, LB_G | LB_LP), OB_EACH(256, LB_G), OB_EACH(256, LB_LP),
                        OB_EACH(256, LB_G | LB_LP));
}
#undef OB_EACH

static void ob_go(int ppw, int want, unsigned grid, size_t lds, hipStream_t st, const ob_args& a) {
    const bool off = a.offset != nullptr;
#define OB_GO(NTV, W)                                                                                     \
    do {                                                                                                  \
        if (off)                                                                                          \
            hipLaunchKernelGGL((k_ordinal_batched<NTV, W, true>), dim3(grid), dim3(256), lds, st, a);     \
        else                                                                                              \
            hipLaunchKernelGGL((k_ordinal_batched<NTV, W, false>), dim3(grid), dim3(256), lds, st, a);    \
    } while (0)
    if (ppw == 4) {
        if (want == LB_G) OB_GO(64, LB_G);
        else if (want == LB_LP) OB_GO(64, LB_LP);
        else OB_GO(64, LB_G | LB_LP);
    } else {
        if (want == LB_G) OB_GO(256, LB_G);
        else if (want == LB_LP) OB_GO(256, LB_LP);
        else OB_GO(256, LB_G | LB_LP);
    }
#undef OB_GO
}

// C >= 2, P >= 1 and D = P + C - 1 <= 64
static bool ob_shape_ok(int C, int P) { return C >= 2 && C <= GB_MAX_D && P >= 1 && P <= GB_MAX_D && P + C - 1 <= GB_MAX_D; }

extern "C" {

// Every check (the shape, the priors, the entry's own NULL arrays, overlaps, the context last), then the one launch.
int gsmvi_ordinal_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int C, int nc, int64_t N, const double* A,
                              const int* y, const double* offset, const int* counts_dev, double prior_prec,
                              const double* prior_prec_dev, double cut_prec, const double* cut_prec_dev, const double* X, double* G,
                              double* lp) {
    GB_BAD(C < 2 || C > GB_MAX_D, "C must be in [2, 64]");
    GB_BAD(P < 1 || P > GB_MAX_D - (C - 1), "P must be in [1, 65 - C] (D = P + C - 1 <= 64)");
    const int D = P + C - 1;
    if (int st = gb_check_shape(__func__, K, D, gb_ppw)) return st;
    GB_BAD(N < 1, "N must be at least 1");
    GB_BAD(N > (INT64_MAX / 8 / P) / K, "K N P is too large");
    GB_BAD(!prior_prec_dev && !(prior_prec >= 0.0 && prior_prec < __builtin_huge_val()), "prior_prec must be finite and >= 0");
    GB_BAD(!cut_prec_dev && !(cut_prec >= 0.0 && cut_prec < __builtin_huge_val()), "cut_prec must be finite and >= 0");
    GB_BAD(nc < 1, "nc must be at least 1");
    GB_BAD(nc > (INT64_MAX / 8 / D) / K, "K nc D is too large");
    GB_BAD(!A || !y || !X, "NULL array");
    GB_BAD(!G && !lp, "give G or lp (or both)");
    const size_t nx = (size_t)K * nc * D * 8, nn = (size_t)K * N, nkb = (size_t)K * 8;
    if (int st = gb_check_overlaps(__func__, {{A, nn * P * 8, "A", GB_RD},
                                              {y, nn * 4, "y", GB_RD},
                                              {offset, nn * 8, "offset", GB_RD},
                                              {counts_dev, (size_t)K * 4, "counts_dev", GB_RD},
                                              {prior_prec_dev, nkb, "prior_prec_dev", GB_RD},
                                              {cut_prec_dev, nkb, "cut_prec_dev", GB_RD},
                                              {X, nx, "X", GB_RD},
                                              {G, nx, "G", GB_WR},
                                              {lp, (size_t)K * nc * 8, "lp", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    const int want = (G ? LB_G : 0) | (lp ? LB_LP : 0);
    ob_args a = {K, N, P, C, nc, 0, A, y, offset, counts_dev, prior_prec, prior_prec_dev, cut_prec, cut_prec_dev, X, G, lp};
    int ppw;
    const size_t lds = ob_launch_lds(P, C, nc, want, offset != nullptr, &ppw, &a.tcm);
    const unsigned grid = (unsigned)((K + ppw - 1) / ppw);
    ob_go(ppw, want, grid, lds, reinterpret_cast<hipStream_t>(stream), a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_TARGET, "k_ordinal_batched");
}

// include/gsmvi_hip_debug.h: what a launch at (C, P, nc) requests (exported by the debug library only); want: 1 = G, 2 = lp,
// 3 = both
int gsmvi_debug_ordinal_batched_lds(int C, int P, int nc, int want, int has_offset, size_t* bytes, int* problems_per_workgroup) {
    GB_BAD(!ob_shape_ok(C, P) || nc < 1 || want < 1 || want > 3 || !bytes || !problems_per_workgroup,
           "bad shape, want or NULL output");
    int tcm;
    *bytes = ob_launch_lds(P, C, nc, want, has_offset != 0, problems_per_workgroup, &tcm);
    return GSMVI_OK;
}

}  // extern "C"
