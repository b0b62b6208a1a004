// Batched logistic target: score and log-density of K Bayesian logistic regressions of one (N, D), D <= 64, at nc points each,
// in one launch ("Batched logistic target").
//
// The reference's users hand the fits a model's log_prob and jit(grad(...)) of it (examples/example_gsm.py:34-35), which XLA
// fuses into a kernel or two.  Here, for problem k with design matrix A_k (N rows a_n of length D), labels y_kn in [0, 1],
// n_k <= N valid rows and prior precision lam_k >= 0, at the rows x of X_k:
//   eta_n   = a_n . x
//   lp(x)   = sum_{n < n_k} [ y_n eta_n - softplus(eta_n) ] - lam_k |x|^2 / 2
//   g(x)    = sum_{n < n_k} ( y_n - sigma(eta_n) ) a_n - lam_k x
// with e = exp(-|eta|), sigma = 1 / (1 + e) for eta >= 0 and e / (1 + e) otherwise, softplus = max(eta, 0) + log1p(e).
//   k_logistic_batched<NT, WANT> : WANT = LB_G (the score alone: no logarithm), LB_LP (the density alone: no second pass over
//                                  the tile), or both from one pass
// Work mapping: the slots of gsmvi_batched.h (gb_nt(D) threads per problem, four problems per 256-thread workgroup for
// D <= 16).  The launch walks the rows of X_k in tiles of TC (32; 16 in the four-problem packing) and, per such tile, the rows
// of A_k in tiles of LB_TN = 32, so neither nc nor N is bounded by LDS.  A tile of A_k is staged in LDS once (row stride D | 1)
// and used twice: thread (n, c-group) forms eta for its row n and up to CQ rows of X (A_n j read once per CQ products, the x
// broadcast), applies the link and leaves r = y - sigma (and the density's term) in LDS (row stride 33); then thread (c, j)
// owns the outputs g_cj for up to MAXQ rows c and sums r_cn A_nj over the tile's rows in order.  The next tile of A_k (and of
// y_k) is loaded into registers right after the barrier that publishes the current one and is written to LDS only after the
// current one is consumed: A is the only large stream and its loads are in flight during both passes.
// Order: every output row (k, c) sums over n = 0 .. n_k - 1 in that order in one thread, so it does not depend on K, nc, the
// tiling of nc or the slot packing.  Rows n >= n_k are never loaded.  A row of X with a non-finite entry gets NaN outputs (by
// a flag, not by arithmetic: sigma saturates and would hide an infinity).  A slot reads and writes only its own problem's
// slices and every slot runs the same barriers (2 + 3 ceil(N / 32) per tile of X rows), so nothing crosses between problems.
// All inputs are only read; no context workspace.
//
// The same kernel scores a family of generalised linear models (gsmvi_glm_batched_f64; DESIGN.md section 9, "Batched GLM
// targets"): eta_n = a_n . x + o_kn with an optional offset o (K, N), lp = sum_n t(eta_n, y_n) - lam_k |x|^2 / 2 and
// g = sum_n r(eta_n, y_n) a_n - lam_k x, where the link (r, t) is lb_link<FAM>, the third template parameter:
//   logistic  r = y - sigma(eta)                               t = y eta - softplus(eta)            (the forms above)
//   poisson   r = y - e^eta                                    t = y eta - e^eta                    (log link; -log y! dropped)
//   probit    r = y phi/Phi(eta) - (1 - y) phi/Phi(-eta)       t = y log Phi(eta) + (1 - y) log Phi(-eta)
//   gaussian  r = tau_k (y - eta)                              t = -tau_k (y - eta)^2 / 2           (identity link, precision tau_k)
// Everything else -- tiling, prefetch, packing, order of summation, counts, priors, the row flags -- is the one copy below.  The
// offset of a tile rides beside its y (32 more doubles of LDS per problem, only in the kernels with OFF, the fourth template
// parameter: the launches without an offset keep the code and the registers they had before there was one).  A Poisson row for
// which some valid e^eta is not finite gets NaN outputs through the row flag of a non-finite row of X.
// Host side: the model's checks, its overlap entries and the dispatch on the family are gsmvi_glm_model.h's, shared with the
// Laplace and predictive entries; lb_run adds what is this launch's own (nc, X, G, lp).
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_glm_model.h"                 // glm_model and its checks; gsmvi_glm_link.h: lb_link, the families, LB_TN
#include "../../include/gsmvi_hip.h"
#include "../../include/gsmvi_hip_debug.h"   // gsmvi_debug_logistic_batched_lds
#include <cstdint>
#include <type_traits>

#define LB_AQ 8    // tile elements per thread: LB_TN D / NT <= 8 in both packings

// (the model's fields in this kernel's own order, not a glm_model: with the shared block in front, the register allocation of the
// 256-thread gaussian density kernel changes, and the 256-thread kernels sit at a register cliff, see lb_off_tile)
struct lb_args {
    long long K, N;
    int D, nc, tcm;             // dimension, rows of X per problem, rows of X held in LDS = min(nc, TC)
    const double* A;            // (K, N, D)
    const double* y;            // (K, N)
    const int* counts;          // (K) valid rows, clamped to 0 .. N (null: N)
    double lam;                 // the prior precision of every problem ...
    const double* lam_dev;      // ... or (K) per-problem values on the device (null: `lam`)
    const double* X;            // (K, nc, D)
    double* G;                  // (K, nc, D) or null
    double* lp;                 // (K, nc) or null
    // the GLM families (appended: the logistic launches keep the argument block they had)
    const double* offset;       // (K, N) added to eta, or null
    double tau;                 // gaussian family: the noise precision of every problem ...
    const double* tau_dev;      // ... or (K) per-problem values on the device (null: `tau`)
};

__host__ __device__ inline int lb_tc(int NT) { return NT == 256 ? 32 : 16; }
// LDS doubles per problem: the A tile (32 x (D | 1)) + its y (32) + its offset (32, when one is given) + the X tile (tcm x
// (D | 1)) + the row flags (tcm) + r and the density's terms (tcm x 33 each, as wanted).  (64, 32 rows, both): 6336 doubles,
// 49.5 KB; four problems of (16, 16 rows, both): 4 x 1920 doubles, 60 KB; with an offset 32 doubles per problem more: 49.75 KB
// and 61 KB
__host__ __device__ inline int lb_lds_doubles(int D, int tcm, int want, bool off = false) {
    return LB_TN * (D | 1) + LB_TN + (off ? LB_TN : 0) +
           tcm * ((D | 1) + 1 + (LB_TN | 1) * ((want & LB_G ? 1 : 0) + (want & LB_LP ? 1 : 0)));
}

// f(integral_constant<int, n>) for the runtime n in 1 .. MAX: the two inner loops below run with a compile-time number of rows of X
// per thread, so that they are branch-free and their LDS reads are issued in batches (a uniform `if (q < n)` inside them is a
// scalar branch per product, and every product then waits for its own LDS read)
template <int Q, int MAX, typename F>
__device__ __forceinline__ void lb_rows(int n, F&& f) {
    if constexpr (Q >= MAX) {
        f(std::integral_constant<int, MAX>{});
    } else {
        if (n == Q)
            f(std::integral_constant<int, Q>{});
        else
            lb_rows<Q + 1, MAX>(n, f);
    }
}

template <int NT, int WANT, int FAM, bool OFF>
__global__ __launch_bounds__(256) void k_logistic_batched(lb_args a) {
    extern __shared__ double lb_sm[];
    constexpr int PPW = 256 / NT, TC = NT == 256 ? 32 : 16;
    constexpr int NG = NT / LB_TN, CQ = TC / NG;        // eta pass: NG groups of 32 threads, CQ rows of X per thread
    constexpr int MAXQ = TC / 4;                        // score pass: rows of X per thread (NT / D >= 4 rows side by side)
    constexpr bool HAS_G = (WANT & LB_G) != 0, HAS_LP = (WANT & LB_LP) != 0;
    const int D = a.D, ld = D | 1, ldr = LB_TN | 1, tcm = a.tcm;
    const long long N = a.N;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;               // a tail slot runs every barrier and nothing else
    double* As = lb_sm + (size_t)slot * lb_lds_doubles(D, tcm, WANT, OFF);
    double* Ys = As + LB_TN * ld;             // 32         y of the tile's rows
    double* Os = Ys + LB_TN;                  // 32         their offsets, when given
    double* Xs = Os + (OFF ? LB_TN : 0);      // tcm x ld   the rows of X
    double* Rb = Xs + tcm * ld;               // tcm        0, or NaN for a row of X with a non-finite entry
    double* Rs = Rb + tcm;                    // tcm x ldr  r(eta, y) of the link
    double* Ts = Rs + (HAS_G ? tcm * ldr : 0);   // tcm x ldr  t(eta, y) of the link
    const size_t kk = (size_t)(valid ? k : 0);
    const double* Ak = a.A + kk * (size_t)N * D;
    const double* yk = a.y + kk * (size_t)N;
    // y_k and the offset share the prefetch: lane l < 32 carries y of the tile's row l, lane 32 + l its offset, and Os follows Ys
    // (without an offset: lane l < 32 and y alone, as before there was one)
    const int yl = OFF ? l % LB_TN : l;
    // (an OFF launch without an offset -- the poisson family always takes the OFF kernels, see lb_go -- loads nothing in the
    // upper lanes: the offset's tile is zeros)
    const bool yload = !OFF || l < LB_TN || a.offset != nullptr;
    const double* yo = OFF && l >= LB_TN && a.offset ? a.offset + kk * (size_t)N : yk;
#define LB_YLANE(t) (OFF ? l < 2 * LB_TN && yl < (t) : l < (t))
    const double* Xk = a.X + kk * (size_t)a.nc * D;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    long long nk = 0;                         // the rows that count
    double lam = 0.0, tau = 1.0;
    if (valid) {
        nk = N;
        if (a.counts) {
            const long long c = a.counts[k];
            nk = c < 0 ? 0 : (c > N ? N : c);
        }
        lam = a.lam_dev ? a.lam_dev[k] : a.lam;
        if (FAM == LB_GAUSSIAN) tau = a.tau_dev ? a.tau_dev[k] : a.tau;
    }
    // the tile elements e = l + q NT of this thread as (row, column), stepped without a division
    const int row0 = l / D, col0 = l - row0 * D, dr = NT / D, dc = NT - dr * D;
    // the eta pass: row en of the tile, rows eg + q NG of X;  the score pass: column gj, rows gc0 + q CW of X
    const int en = l % LB_TN, eg = l / LB_TN;
    const int CW = NT / D, gj = col0, gc0 = row0;
    const bool gact = l < CW * D;

    for (int c0 = 0; c0 < a.nc; c0 += TC) {
        const int tc = a.nc - c0 < TC ? a.nc - c0 : TC;
        if (valid)
            for (int e = l; e < tc * D; e += NT) {
                const int r = e / D, j = e - r * D;
                Xs[r * ld + j] = Xk[(size_t)(c0 + r) * D + j];
            }
        // the first tile of A_k and y_k into registers
        double pre[LB_AQ], ypre = 0.0;
        {
            const int tnv = (int)(nk < LB_TN ? nk : LB_TN), te = tnv * D;
#pragma unroll
            for (int q = 0; q < LB_AQ; ++q) {
                const int e = l + q * NT;
                pre[q] = e < te ? Ak[e] : 0.0;
            }
            if (LB_YLANE(tnv) && yload) ypre = yo[yl];
        }
        __syncthreads();
        double xx = 0.0;                      // |x|^2 of row l (threads l < tc)
        if (valid && l < tc) {
            double z = 0.0;
            for (int j = 0; j < D; ++j) {
                const double x = Xs[l * ld + j];
                z += x * 0.0;
                xx += x * x;
            }
            Rb[l] = z;
        }

        double acc[MAXQ], lpacc = 0.0;
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) acc[q] = 0.0;
        const int nq = (tc + CW - 1) / CW;    // rows of X per thread in the score pass and in the eta pass (uniform in the slot)
        const int nqe = (tc + NG - 1) / NG;

        for (long long n0 = 0; n0 < N; n0 += LB_TN) {
            const long long left = nk - n0;
            const int tnv = left < 0 ? 0 : (int)(left < LB_TN ? left : LB_TN), te = tnv * D;
            {                                 // registers -> LDS (the previous tile was consumed before the last barrier)
                int r = row0, c = col0;
#pragma unroll
                for (int q = 0; q < LB_AQ; ++q) {
                    if (l + q * NT < te) As[r * ld + c] = pre[q];
                    r += dr;
                    c += dc;
                    if (c >= D) {
                        c -= D;
                        ++r;
                    }
                }
                if (LB_YLANE(tnv)) Ys[l] = ypre;
            }
            __syncthreads();
            {                                 // the next tile's loads: in flight while this one is consumed
                const long long left2 = left - LB_TN;
                const int tnv2 = left2 < 0 ? 0 : (int)(left2 < LB_TN ? left2 : LB_TN), te2 = tnv2 * D;
                const double* An = Ak + (size_t)(n0 + LB_TN) * D;
#pragma unroll
                for (int q = 0; q < LB_AQ; ++q) {
                    const int e = l + q * NT;
                    if (e < te2) pre[q] = An[e];
                }
                if (LB_YLANE(tnv2) && yload) ypre = yo[n0 + LB_TN + yl];
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
                const double* ar = As + en * ld;
                lb_rows<1, CQ>(nqe, [&](auto nr) {
#pragma unroll 8
                    for (int j = 0; j < D; ++j) {
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
                // eta goes through this thread's own LDS cells, so that the link below is ONE copy of exp / log1p in a rolled
                // loop (unrolled over q it takes 170 - 230 VGPRs)
                double* Es = HAS_G ? Rs : Ts;
#pragma unroll
                for (int q = 0; q < CQ; ++q)
                    if (eg + q * NG < tc) Es[(eg + q * NG) * ldr + en] = eta[q];
                const double yv = Ys[en];
#pragma unroll 1
                for (int c = eg; c < tc; c += NG) {
                    double r = 0.0, t = 0.0;
                    const bool fine = lb_link<FAM, HAS_G, HAS_LP>(Es[c * ldr + en], yv, tau, r, t);
                    if (HAS_G) Rs[c * ldr + en] = r;
                    if (HAS_LP) Ts[c * ldr + en] = t;
                    if (FAM == LB_POISSON && !fine) Rb[c] = qnan;     // (any number of threads, the same value)
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
                lb_rows<1, MAXQ>(nq, [&](auto nr) {
#pragma unroll 8
                    for (int n = 0; n < tnv; ++n) {
                        const double av = As[n * ld + gj];
#pragma unroll
                        for (int q = 0; q < decltype(nr)::value; ++q) acc[q] = fma(Rs[ro[q] + n], av, acc[q]);
                    }
                });
            }
            if (HAS_LP && l < tc && valid)
                for (int n = 0; n < tnv; ++n) lpacc += Ts[l * ldr + n];
            __syncthreads();                  // the next tile overwrites As, Ys, Rs, Ts
        }

        if (valid) {
            if (HAS_G && gact) {
#pragma unroll
                for (int q = 0; q < MAXQ; ++q) {
                    const int c = gc0 + q * CW;
                    if (c < tc) {
                        const double v = acc[q] - lam * Xs[c * ld + gj];
                        a.G[(kk * (size_t)a.nc + (size_t)(c0 + c)) * D + gj] = Rb[c] == 0.0 ? v : qnan;
                    }
                }
            }
            if (HAS_LP && l < tc) a.lp[kk * (size_t)a.nc + (size_t)(c0 + l)] = Rb[l] == 0.0 ? lpacc - 0.5 * lam * xx : qnan;
        }
        __syncthreads();                      // the next tile of X rows overwrites Xs and Rb
    }
#undef LB_YLANE
}

// dynamic LDS bytes of a launch at (D, nc, want): at most 60 KB (61 KB with an offset), below the default limit of 64 KB, so no
// kernel attribute is needed
static size_t lb_launch_lds(int D, int nc, int want, bool off, int* ppw, int* tcm) {
    const int nt = gb_nt(D), tc = lb_tc(nt);
    *ppw = 256 / nt;
    *tcm = nc < tc ? nc : tc;
    return (size_t)*ppw * lb_lds_doubles(D, *tcm, want, off) * sizeof(double);
}

// does a launch of `family` carry the offset's tile: with an offset, and always for the poisson family (whose 256-thread score
// kernel without the tile is the one instantiation that needs more than 256 registers and so runs at half the occupancy and
// 1.5 times the time of the one with it; a NULL offset is then a tile of zeros, and eta + 0 changes no bit of r or t)
// This is a choice made for one compiler's register allocation: DESIGN.md says how to re-check it after a toolchain change.
static bool lb_off_tile(int family, bool has_offset) { return has_offset || family == GSMVI_GLM_POISSON; }
static bool lb_off(int family, const double* offset) { return lb_off_tile(family, offset != nullptr); }

template <int FAM>
static void lb_go(int ppw, int want, unsigned grid, size_t lds, hipStream_t st, const lb_args& a) {
    const bool off = lb_off(FAM, a.offset);
#define LB_GO(NTV, W)                                                                                          \
    do {                                                                                                       \
        if (off)                                                                                               \
            hipLaunchKernelGGL((k_logistic_batched<NTV, W, FAM, true>), dim3(grid), dim3(256), lds, st, a);    \
        else if constexpr (FAM != LB_POISSON)                                                                  \
            hipLaunchKernelGGL((k_logistic_batched<NTV, W, FAM, false>), dim3(grid), dim3(256), lds, st, a);   \
    } while (0)
    if (ppw == 4) {
        if (want == LB_G) LB_GO(64, LB_G);
        else if (want == LB_LP) LB_GO(64, LB_LP);
        else LB_GO(64, LB_G | LB_LP);
    } else {
        if (want == LB_G) LB_GO(256, LB_G);
        else if (want == LB_LP) LB_GO(256, LB_LP);
        else LB_GO(256, LB_G | LB_LP);
    }
#undef LB_GO
}

// The body of both entry points: every check (the model, the entry's own shapes and NULL arrays, overlaps, the context last),
// then the one launch.  `fn` names the entry point in the messages.
static int lb_run(const char* fn, gsmvi_ctx* ctx, void* stream, int family, const glm_model& m, int nc, const double* X, double* G,
                  double* lp) {
#define LB_BAD(cond, msg)                     \
    do {                                      \
        if (cond) return gb_bad(fn, msg);     \
    } while (0)
    if (int st = glm_check_model(fn, m, family, "N", true)) return st;
    LB_BAD(nc < 1, "nc must be at least 1");
    LB_BAD(nc > (INT64_MAX / 8 / m.D) / m.K, "K nc D is too large");
    LB_BAD(!m.A || !m.y || !X, "NULL array");
    LB_BAD(!G && !lp, "give G or lp (or both)");
    const size_t nx = (size_t)m.K * nc * m.D * 8;
    if (int st = gb_check_overlaps(fn, m, {{X, nx, "X", GB_RD}, {G, nx, "G", GB_WR}, {lp, (size_t)m.K * nc * 8, "lp", GB_WR}}))
        return st;
    LB_BAD(!ctx, "ctx is NULL");
#undef LB_BAD
    const int want = (G ? LB_G : 0) | (lp ? LB_LP : 0);
    lb_args a = {m.K, m.N, m.D, nc, 0, m.A, m.y, m.counts, m.lam, m.lam_dev, X, G, lp, m.offset, m.tau, m.tau_dev};
    int ppw;
    const size_t lds = lb_launch_lds(m.D, nc, want, lb_off(family, m.offset), &ppw, &a.tcm);
    const unsigned grid = (unsigned)((m.K + ppw - 1) / ppw);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    glm_for_family(family, [&](auto fam) { lb_go<decltype(fam)::value>(ppw, want, grid, lds, st, a); });
    return gb_launched(ctx, GSMVI_PATH_BATCHED_TARGET, "k_logistic_batched");
}

extern "C" {

int gsmvi_logistic_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int nc, int64_t N, const double* A, const double* y,
                               const int* counts_dev, double prior_prec, const double* prior_prec_dev, const double* X, double* G,
                               double* lp) {
    return lb_run(__func__, ctx, stream, GSMVI_GLM_LOGISTIC, {K, N, D, A, y, nullptr, counts_dev, prior_prec, prior_prec_dev, 1.0, nullptr},
                  nc, X, G, lp);
}

int gsmvi_glm_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int nc, int64_t N, int family, const double* A,
                          const double* y, const double* offset, const int* counts_dev, double noise_prec,
                          const double* noise_prec_dev, double prior_prec, const double* prior_prec_dev, const double* X, double* G,
                          double* lp) {
    return lb_run(__func__, ctx, stream, family,
                  {K, N, D, A, y, offset, counts_dev, prior_prec, prior_prec_dev, noise_prec, noise_prec_dev}, nc, X, G, lp);
}

// include/gsmvi_hip_debug.h: what a launch at (D, nc) requests (exported by the debug library only); want: 1 = G, 2 = lp, 3 = both
int gsmvi_debug_logistic_batched_lds(int D, int nc, int want, size_t* bytes, int* problems_per_workgroup) {
    GB_BAD(D < 1 || D > GB_MAX_D || nc < 1 || want < 1 || want > 3 || !bytes || !problems_per_workgroup,
           "bad shape, want or NULL output");
    int tcm;
    *bytes = lb_launch_lds(D, nc, want, false, problems_per_workgroup, &tcm);
    return GSMVI_OK;
}

// the same for a gsmvi_glm_batched_f64 launch of `family`, through the launch's own rule for the offset's tile (lb_off)
int gsmvi_debug_glm_batched_lds(int D, int nc, int want, int family, int has_offset, size_t* bytes,
                                int* problems_per_workgroup) {
    GB_BAD(D < 1 || D > GB_MAX_D || nc < 1 || want < 1 || want > 3 || family < GSMVI_GLM_LOGISTIC ||
               family > GSMVI_GLM_GAUSSIAN || !bytes || !problems_per_workgroup,
           "bad shape, want, family or NULL output");
    int tcm;
    *bytes = lb_launch_lds(D, nc, want, lb_off_tile(family, has_offset != 0), problems_per_workgroup, &tcm);
    return GSMVI_OK;
}

}  // extern "C"
