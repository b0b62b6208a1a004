// Batched negative binomial target: score and log-density of K overdispersed count regressions of one (N, P) at nc points each,
// in one launch ("Batched negative binomial target").
//
// The reference's users hand the fits a model's log_prob and jit(grad(...)) of it (examples/example_gsm.py:34-35).  Here, for
// problem k with design matrix A_k (N rows a_n of length P), responses y_kn >= 0, an optional offset o_kn, n_k <= N valid rows,
// at the rows x = (beta, theta) of X_k (length D = P + 1 <= 64; theta = log r, the log of the size: variance mu + mu^2 / r):
//   eta_n = a_n . beta + o_n,   d_n = eta_n - theta,   r = e^theta
//   lp(x)     = sum_{n < n_k} t_n - lam_k |beta|^2 / 2 - kap_k (theta - m_k)^2 / 2
//   g(x)[:P]  = sum_{n < n_k} r_eta,n a_n - lam_k beta
//   g(x)[P]   = sum_{n < n_k} r_theta,n - kap_k (theta - m_k)
// with (t, r_eta, r_theta) of gsmvi_negbin_link.h.  The model has a fitted shape parameter, so it is a kernel of its own and not
// one more lb_link<FAM> of k_logistic_batched, whose work mapping and promises it keeps:
//   k_negbin_batched<NT, WANT, OFF> : WANT = LB_G, LB_LP or both from one pass; OFF: the launch carries the offset's tile
// The slots of gsmvi_batched.h (gb_nt(D) threads per problem, four problems per 256-thread workgroup for D <= 16).  The launch
// walks the rows of X_k in tiles of TC (32; 16 in the four-problem packing) and, per such tile, the rows of A_k in tiles of
// LB_TN = 32, so neither nc nor N is bounded by LDS.  A tile of A_k is staged in LDS once (row stride P | 1) and used twice:
// thread (n, c-group) forms eta for its row n and up to CQ rows of X, applies the link and leaves r_eta, r_theta (and t) in LDS
// (row stride 33); then thread (c, j) owns the output g_cj for up to MAXQ rows c: for j < P it sums r_eta,cn A_nj over the tile's
// rows in order, for j = P it sums r_theta,cn (the same chain with 1.0 in the place of A_nj).  The next tile of A_k (and of y_k,
// o_k) is loaded into registers right after the barrier that publishes the current one.
// Order: every output row (k, c) sums over n = 0 .. n_k - 1 in that order in one thread, so it does not depend on K, nc, the
// tiling of nc or the slot packing.  Rows n >= n_k are never loaded.  A row of X with a non-finite entry, or whose e^theta is not
// a positive normal number, gets NaN outputs by a flag.  A slot reads and writes only its own problem's slices and every slot
// runs the same barriers, so nothing crosses between problems.  No atomics; all inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_glm_model.h"                 // glm_model's overlap table, LB_G / LB_LP, LB_TN
#include "gsmvi_negbin_link.h"
#include "../../include/gsmvi_hip.h"
#include "../../include/gsmvi_hip_debug.h"   // gsmvi_debug_negbin_batched_lds
#include <cstdint>
#include <type_traits>

#define NB_AQ 8    // tile elements per thread: LB_TN P / NT <= 8 in both packings

struct nb_args {
    long long K, N;
    int P, nc, tcm;             // columns of A (D = P + 1), rows of X per problem, rows of X held in LDS = min(nc, TC)
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
    const double* X;            // (K, nc, D)
    double* G;                  // (K, nc, D) or null
    double* lp;                 // (K, nc) or null
};

__host__ __device__ inline int nb_tc(int NT) { return NT == 256 ? 32 : 16; }
// LDS doubles per problem: the A tile (32 x (P | 1)) + its y (32) + its offset (32, when one is given) + the X tile (tcm x
// (D | 1)) + the row flags and e^theta (2 tcm) + r_eta and r_theta (tcm x 33 each, with G) + t (tcm x 33, with lp).
// (D = 64, 32 rows, both, offset): 7392 doubles, 57.75 KB; four problems of (16, 16 rows, both, offset): 4 x 2432 doubles, 76 KB
__host__ __device__ inline int nb_lds_doubles(int P, int tcm, int want, bool off) {
    const int D = P + 1;
    return LB_TN * (P | 1) + LB_TN + (off ? LB_TN : 0) +
           tcm * ((D | 1) + 2 + (LB_TN | 1) * ((want & LB_G ? 2 : 0) + (want & LB_LP ? 1 : 0)));
}

// f(integral_constant<int, n>) for the runtime n in 1 .. MAX (as lb_rows of gsmvi_logistic_batched.hip): the two inner loops
// run with a compile-time number of rows of X per thread
template <int Q, int MAX, typename F>
__device__ __forceinline__ void nb_rows(int n, F&& f) {
    if constexpr (Q >= MAX) {
        f(std::integral_constant<int, MAX>{});
    } else {
        if (n == Q)
            f(std::integral_constant<int, Q>{});
        else
            nb_rows<Q + 1, MAX>(n, f);
    }
}

template <int NT, int WANT, bool OFF>
__global__ __launch_bounds__(256) void k_negbin_batched(nb_args a) {
    extern __shared__ double nb_sm[];
    constexpr int PPW = 256 / NT, TC = NT == 256 ? 32 : 16;
    constexpr int NG = NT / LB_TN, CQ = TC / NG;        // eta pass: NG groups of 32 threads, CQ rows of X per thread
    constexpr int MAXQ = TC / 4;                        // score pass: rows of X per thread (NT / D >= 4 rows side by side)
    constexpr bool HAS_G = (WANT & LB_G) != 0, HAS_LP = (WANT & LB_LP) != 0;
    const int P = a.P, D = P + 1, lda = P | 1, ld = D | 1, ldr = LB_TN | 1, tcm = a.tcm;
    const long long N = a.N;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;               // a tail slot runs every barrier and nothing else
    double* As = nb_sm + (size_t)slot * nb_lds_doubles(P, tcm, WANT, OFF);
    double* Ys = As + LB_TN * lda;            // 32         y of the tile's rows
    double* Os = Ys + LB_TN;                  // 32         their offsets, when given
    double* Xs = Os + (OFF ? LB_TN : 0);      // tcm x ld   the rows of X
    double* Rb = Xs + tcm * ld;               // tcm        0, or NaN for a flagged row of X
    double* Rr = Rb + tcm;                    // tcm        r = e^theta of the row
    double* Rs = Rr + tcm;                    // tcm x ldr  r_eta
    double* Qs = Rs + (HAS_G ? tcm * ldr : 0);   // tcm x ldr  r_theta
    double* Ts = Qs + (HAS_G ? tcm * ldr : 0);   // tcm x ldr  t
    const size_t kk = (size_t)(valid ? k : 0);
    const double* Ak = a.A + kk * (size_t)N * P;
    const double* yk = a.y + kk * (size_t)N;
    // y_k and the offset share the prefetch: lane l < 32 carries y of the tile's row l, lane 32 + l its offset, and Os follows Ys
    const int yl = OFF ? l % LB_TN : l;
    const double* yo = OFF && l >= LB_TN ? a.offset + kk * (size_t)N : yk;
#define NB_YLANE(t) (OFF ? l < 2 * LB_TN && yl < (t) : l < (t))
    const double* Xk = a.X + kk * (size_t)a.nc * D;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    long long nk = 0;                         // the rows that count
    double lam = 0.0, tm = 0.0, tk = 0.0;
    if (valid) {
        nk = N;
        if (a.counts) {
            const long long c = a.counts[k];
            nk = c < 0 ? 0 : (c > N ? N : c);
        }
        lam = a.lam_dev ? a.lam_dev[k] : a.lam;
        tm = a.tm_dev ? a.tm_dev[k] : a.tm;
        tk = a.tk_dev ? a.tk_dev[k] : a.tk;
    }
    // the tile elements e = l + q NT of this thread as (row, column) of the A tile, stepped without a division
    const int row0 = l / P, col0 = l - row0 * P, dr = NT / P, dc = NT - dr * P;
    // the eta pass: row en of the tile, rows eg + q NG of X;  the score pass: component gj of the output, rows gc0 + q CW of X
    const int en = l % LB_TN, eg = l / LB_TN;
    const int CW = NT / D, gc0 = l / D, gj = l - gc0 * D;
    const bool gact = l < CW * D, glast = gj == P;
    const int gja = glast ? 0 : gj;           // the column of A this thread reads (component P reads none: 1.0 stands in)

    for (int c0 = 0; c0 < a.nc; c0 += TC) {
        const int tc = a.nc - c0 < TC ? a.nc - c0 : TC;
        if (valid)
            for (int e = l; e < tc * D; e += NT) {
                const int r = e / D, j = e - r * D;
                Xs[r * ld + j] = Xk[(size_t)(c0 + r) * D + j];
            }
        // the first tile of A_k, y_k and o_k into registers
        double pre[NB_AQ], ypre = 0.0;
        {
            const int tnv = (int)(nk < LB_TN ? nk : LB_TN), te = tnv * P;
#pragma unroll
            for (int q = 0; q < NB_AQ; ++q) {
                const int e = l + q * NT;
                pre[q] = e < te ? Ak[e] : 0.0;
            }
            if (NB_YLANE(tnv)) ypre = yo[yl];
        }
        __syncthreads();
        double bb = 0.0, th = 0.0;            // |beta|^2 and theta of row l (threads l < tc)
        if (valid && l < tc) {
            double z = 0.0;
            for (int j = 0; j < P; ++j) {
                const double x = Xs[l * ld + j];
                z += x * 0.0;
                bb += x * x;
            }
            th = Xs[l * ld + P];
            const double r = exp(th);         // (a NaN theta gives a NaN r: flagged)
            Rr[l] = r;
            Rb[l] = r >= 2.2250738585072014e-308 && r < __builtin_huge_val() ? z : qnan;
        }

        double acc[MAXQ], lpacc = 0.0;
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) acc[q] = 0.0;
        const int nq = (tc + CW - 1) / CW;    // rows of X per thread in the score pass and in the eta pass (uniform in the slot)
        const int nqe = (tc + NG - 1) / NG;

        for (long long n0 = 0; n0 < N; n0 += LB_TN) {
            const long long left = nk - n0;
            const int tnv = left < 0 ? 0 : (int)(left < LB_TN ? left : LB_TN), te = tnv * P;
            {                                 // registers -> LDS (the previous tile was consumed before the last barrier)
                int r = row0, c = col0;
#pragma unroll
                for (int q = 0; q < NB_AQ; ++q) {
                    if (l + q * NT < te) As[r * lda + c] = pre[q];
                    r += dr;
                    c += dc;
                    if (c >= P) {
                        c -= P;
                        ++r;
                    }
                }
                if (NB_YLANE(tnv)) Ys[l] = ypre;
            }
            __syncthreads();                  // (also publishes Rb and Rr of this tile of X rows)
            {                                 // the next tile's loads: in flight while this one is consumed
                const long long left2 = left - LB_TN;
                const int tnv2 = left2 < 0 ? 0 : (int)(left2 < LB_TN ? left2 : LB_TN), te2 = tnv2 * P;
                const double* An = Ak + (size_t)(n0 + LB_TN) * P;
#pragma unroll
                for (int q = 0; q < NB_AQ; ++q) {
                    const int e = l + q * NT;
                    if (e < te2) pre[q] = An[e];
                }
                if (NB_YLANE(tnv2)) ypre = yo[n0 + LB_TN + yl];
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
                nb_rows<1, CQ>(nqe, [&](auto nr) {
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
                const double yv = Ys[en];
#pragma unroll 1
                for (int c = eg; c < tc; c += NG) {
                    double re = 0.0, rt = 0.0, t = 0.0;
                    nb_link<HAS_G, HAS_LP>(Es[c * ldr + en], Xs[c * ld + P], Rr[c], yv, re, rt, t);
                    if (HAS_G) {
                        Rs[c * ldr + en] = re;
                        Qs[c * ldr + en] = rt;
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
                const double* Rg = glast ? Qs : Rs;
                nb_rows<1, MAXQ>(nq, [&](auto nr) {
#pragma unroll 8
                    for (int n = 0; n < tnv; ++n) {
                        const double al = As[n * lda + gja], av = glast ? 1.0 : al;
#pragma unroll
                        for (int q = 0; q < decltype(nr)::value; ++q) acc[q] = fma(Rg[ro[q] + n], av, acc[q]);
                    }
                });
            }
            if (HAS_LP && l < tc && valid)
                for (int n = 0; n < tnv; ++n) lpacc += Ts[l * ldr + n];
            __syncthreads();                  // the next tile overwrites As, Ys, Rs, Qs, Ts
        }

        if (valid) {
            if (HAS_G && gact) {
#pragma unroll
                for (int q = 0; q < MAXQ; ++q) {
                    const int c = gc0 + q * CW;
                    if (c < tc) {
                        const double x = Xs[c * ld + gj];
                        const double v = glast ? acc[q] - tk * (x - tm) : acc[q] - lam * x;
                        a.G[(kk * (size_t)a.nc + (size_t)(c0 + c)) * D + gj] = Rb[c] == 0.0 ? v : qnan;
                    }
                }
            }
            if (HAS_LP && l < tc) {
                const double dm = th - tm;
                a.lp[kk * (size_t)a.nc + (size_t)(c0 + l)] = Rb[l] == 0.0 ? lpacc - 0.5 * lam * bb - 0.5 * tk * (dm * dm) : qnan;
            }
        }
        __syncthreads();                      // the next tile of X rows overwrites Xs, Rb and Rr
    }
#undef NB_YLANE
}

// dynamic LDS bytes of a launch at (P, nc, want, offset): up to 76 KB (four problems of D = 16 with both outputs), above the
// 64 KB a kernel gets without an attribute, so gsmvi_negbin_batched_prepare raises the limit of every instantiation
static size_t nb_launch_lds(int P, int nc, int want, bool off, int* ppw, int* tcm) {
    const int nt = gb_nt(P + 1), tc = nb_tc(nt);
    *ppw = 256 / nt;
    *tcm = nc < tc ? nc : tc;
    return (size_t)*ppw * nb_lds_doubles(P, *tcm, want, off) * sizeof(double);
}

#define NB_EACH(NTV, W) k_negbin_batched<NTV, W, false>, k_negbin_batched<NTV, W, true>
hipError_t gsmvi_negbin_batched_prepare() {
    return gb_allow_lds(NB_EACH(64, LB_G), NB_EACH(64, LB_LP), NB_EACH(64, LB_G | LB_LP), NB_EACH(256, LB_G), NB_EACH(256, LB_LP),
                        NB_EACH(256, LB_G | LB_LP));
}
#undef NB_EACH

static void nb_go(int ppw, int want, unsigned grid, size_t lds, hipStream_t st, const nb_args& a) {
    const bool off = a.offset != nullptr;
#define NB_GO(NTV, W)                                                                                    \
    do {                                                                                                 \
        if (off)                                                                                         \
            hipLaunchKernelGGL((k_negbin_batched<NTV, W, true>), dim3(grid), dim3(256), lds, st, a);     \
        else                                                                                             \
            hipLaunchKernelGGL((k_negbin_batched<NTV, W, false>), dim3(grid), dim3(256), lds, st, a);    \
    } while (0)
    if (ppw == 4) {
        if (want == LB_G) NB_GO(64, LB_G);
        else if (want == LB_LP) NB_GO(64, LB_LP);
        else NB_GO(64, LB_G | LB_LP);
    } else {
        if (want == LB_G) NB_GO(256, LB_G);
        else if (want == LB_LP) NB_GO(256, LB_LP);
        else NB_GO(256, LB_G | LB_LP);
    }
#undef NB_GO
}

static bool nb_fin(double v) { return v > -__builtin_huge_val() && v < __builtin_huge_val(); }

extern "C" {

// Every check (the shape, the priors, the entry's own NULL arrays, overlaps, the context last), then the one launch.
int gsmvi_negbin_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int nc, int64_t N, const double* A, const double* y,
                             const double* offset, const int* counts_dev, double theta_mean, const double* theta_mean_dev,
                             double theta_prec, const double* theta_prec_dev, double prior_prec, const double* prior_prec_dev,
                             const double* X, double* G, double* lp) {
    GB_BAD(P < 1 || P > GB_MAX_D - 1, "P must be in [1, 63] (D = P + 1 <= 64)");
    const int D = P + 1;
    if (int st = gb_check_shape(__func__, K, D, gb_ppw)) return st;
    GB_BAD(N < 1, "N must be at least 1");
    GB_BAD(N > (INT64_MAX / 8 / P) / K, "K N P is too large");
    GB_BAD(!prior_prec_dev && !(prior_prec >= 0.0 && prior_prec < __builtin_huge_val()), "prior_prec must be finite and >= 0");
    GB_BAD(!theta_mean_dev && !nb_fin(theta_mean), "theta_mean must be finite");
    GB_BAD(!theta_prec_dev && !(theta_prec >= 0.0 && theta_prec < __builtin_huge_val()), "theta_prec must be finite and >= 0");
    GB_BAD(nc < 1, "nc must be at least 1");
    GB_BAD(nc > (INT64_MAX / 8 / D) / K, "K nc D is too large");
    GB_BAD(!A || !y || !X, "NULL array");
    GB_BAD(!G && !lp, "give G or lp (or both)");
    const glm_model m = {K, N, P, A, y, offset, counts_dev, prior_prec, prior_prec_dev, 1.0, nullptr};
    const size_t nx = (size_t)K * nc * D * 8, nkb = (size_t)K * 8;
    if (int st = gb_check_overlaps(__func__, m, {{theta_mean_dev, nkb, "theta_mean_dev", GB_RD},
                                                 {theta_prec_dev, nkb, "theta_prec_dev", GB_RD},
                                                 {X, nx, "X", GB_RD},
                                                 {G, nx, "G", GB_WR},
                                                 {lp, (size_t)K * nc * 8, "lp", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    const int want = (G ? LB_G : 0) | (lp ? LB_LP : 0);
    nb_args a = {K, N, P, nc, 0, A, y, offset, counts_dev, prior_prec, prior_prec_dev, theta_mean, theta_mean_dev, theta_prec,
                 theta_prec_dev, X, G, lp};
    int ppw;
    const size_t lds = nb_launch_lds(P, nc, want, offset != nullptr, &ppw, &a.tcm);
    const unsigned grid = (unsigned)((K + ppw - 1) / ppw);
    nb_go(ppw, want, grid, lds, reinterpret_cast<hipStream_t>(stream), a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_TARGET, "k_negbin_batched");
}

// include/gsmvi_hip_debug.h: what a launch at (D = P + 1, nc) requests (exported by the debug library only); want: 1 = G, 2 = lp,
// 3 = both
int gsmvi_debug_negbin_batched_lds(int D, int nc, int want, int has_offset, size_t* bytes, int* problems_per_workgroup) {
    GB_BAD(D < 2 || D > GB_MAX_D || nc < 1 || want < 1 || want > 3 || !bytes || !problems_per_workgroup,
           "bad shape, want or NULL output");
    int tcm;
    *bytes = nb_launch_lds(D - 1, nc, want, has_offset != 0, problems_per_workgroup, &tcm);
    return GSMVI_OK;
}

}  // extern "C"
