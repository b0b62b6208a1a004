// Shared-design GLM target: score and log-density of K generalised linear models that share ONE design matrix A (N, D),
// D <= 64, at nc points each, in one launch (gsmvi_glm_shared_batched_f64; DESIGN.md section 9, "Shared-design GLM target").
//
// The reference's users hand the fits a model's log_prob and jit(grad(...)) of it (examples/example_gsm.py:34-35).  Here problem
// k has its own responses y_k, offsets o_k, observation weights w_k >= 0 (K, N each) and precisions lam_k, tau_k, and all K
// problems have the rows a_n of the same A: many responses on one set of covariates, a sweep over lam or tau, the Bayesian
// bootstrap.  With eta_n = a_n . x + o_kn and the link (r, t) = lb_link<FAM> of gsmvi_glm_link.h, at the rows x of X_k:
//   lp(x) = sum_n w_kn t(eta_n, y_kn) - lam_k |x|^2 / 2
//   g(x)  = sum_n w_kn r(eta_n, y_kn) a_n - lam_k x
// With one A the K nc rows of X stack into one tall matrix (row m = k nc + c belongs to problem k = m / nc) and both sums are
// dense float64 products against an operand that stays in L2: eta = X A^T and G = R A, on the 16 x 16 x 4 f64 MFMA.
//   k_glm_shared_batched<NB, WANT, FAM> : NB = glm_dp(D) / 16 column blocks of 16 (1 .. 4); WANT and FAM as in k_logistic_batched
// Work mapping: a 256-thread workgroup takes GS_ROWS = 64 stacked rows, 16 per wave, and walks all N observations in tiles of
// GS_TN = 32.  Each lane holds its wave's X fragments in registers for the whole launch (4 NB doubles, zero-padded beyond D and
// beyond row K nc).  A tile of A goes through LDS once per workgroup, zero-padded to glm_dp(D) columns and to 32 rows, row
// stride glm_dp(D) + 1; the next tile's loads are in flight in registers while the current one is used (two barriers a tile).
// Per 16 observations of the tile, each wave forms
//   eta^T (16 obs x 16 rows) = A_tile X^T : A-operand lane l = a[obs l & 15][kk l >> 4], B-operand lane l = x[kk l >> 4][row l & 15];
//       by the f64 C/D map (gsmvi_common.h) register r of lane l is then eta of row l & 15 at obs (l >> 4) + 4 r,
//   the link on those four entries, with y, o and w of (k(row), obs): the rows of one wave may belong to several problems,
//   G (16 rows x 16 NB) += R A_tile : register r, after the link and the weight, is already the A operand of k-step r (lane l:
//       row l & 15, k = l >> 4, which is obs 4 r + (l >> 4)); the B operand is a[obs 4 r + (l >> 4)][d = (l & 15) + 16 b].
// So the accumulator of the first product is the operand of the second with no LDS transpose and no lane movement.
// Order: every output row sums its observations in an order fixed by N alone -- G: one MFMA accumulation chain over n ascending
// (k-steps of 4); lp: lane group g = l >> 4 sums obs g + 4 r ascending, then the four groups are added 0, 1, 2, 3 -- whatever K,
// nc and the other rows of the launch are.  No atomics; inputs are only read; no context workspace.
// Padding is removed by selection, not by multiplying by zero: a row m >= K nc, an observation n >= N and an observation with
// w = 0 (or a NaN weight) give r = t = 0 whatever eta, y and o hold there (an e^eta that overflows, a NaN y), and flag nothing.
// A row of X with a non-finite entry, and a poisson row for which some e^eta at a w > 0 observation is not finite, get NaN outputs
// by a flag (a ballot over the wave); an MFMA never mixes the rows of X (they are the columns of the first product and the rows of
// the second), so the neighbours of such a row keep their bits.  A is shared, so a non-finite entry of A reaches every problem.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_glm_model.h"                 // glm_check_model, glm_dp, glm_for_family; gsmvi_glm_link.h: lb_link, the families
#include "../../include/gsmvi_hip.h"
#include "../../include/gsmvi_hip_debug.h"   // gsmvi_debug_glm_shared_batched_lds
#include <cstdint>

#define GS_ROWS 64   // stacked rows of X per workgroup: 16 per wave
#define GS_TN 32     // observations per tile of A: two 16-observation MFMA sub-tiles
#define GS_AQ 8      // tile elements per thread: GS_TN D / 256 <= 8

struct gs_args {
    long long M, N;             // stacked rows K nc, observations
    int D, nc;
    const double* A;            // (N, D), shared
    const double* y;            // (K, N)
    const double* offset;       // (K, N) added to eta, or null
    const double* w;            // (K, N) observation weights, or null (1 everywhere)
    double lam;                 // the prior precision of every problem ...
    const double* lam_dev;      // ... or (K) per-problem values on the device (null: `lam`)
    double tau;                 // gaussian family: the noise precision of every problem ...
    const double* tau_dev;      // ... or (K) per-problem values on the device (null: `tau`)
    const double* X;            // (K, nc, D)
    double* G;                  // (K, nc, D) or null
    double* lp;                 // (K, nc) or null
};

// LDS doubles of a launch: the one tile of A, GS_TN x (glm_dp(D) + 1).  D = 64: 2080 doubles, 16.25 KB
__host__ __device__ inline int gs_lds_doubles(int D) { return GS_TN * (glm_dp(D) + 1); }

template <int NB, int WANT, int FAM>
__global__ __launch_bounds__(256) void k_glm_shared_batched(gs_args a) {
    extern __shared__ double gs_sm[];
    constexpr int LD = 16 * NB + 1, KS = 4 * NB;         // row stride of the tile; k-steps of the first product
    constexpr bool HAS_G = (WANT & LB_G) != 0, HAS_LP = (WANT & LB_LP) != 0;
    const int D = a.D, t = threadIdx.x, l = t & 63, li = l & 15, lg = l >> 4;
    const long long N = a.N;
    const long long m0 = (long long)blockIdx.x * GS_ROWS + (t >> 6) * 16, m = m0 + li;   // the wave's first row, this lane's row
    const bool wave_live = m0 < a.M, rv = m < a.M;       // a tail wave runs every barrier and nothing else
    const long long k = rv ? m / a.nc : 0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    double* As = gs_sm;

    // this lane's fragments of X: x[kk = lg + 4 s][row li], zero beyond D and beyond the last row
    double xf[KS];
    bool bad = false;                                    // this lane saw what flags row li
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int kk = lg + 4 * s;
        xf[s] = rv && kk < D ? a.X[(size_t)m * D + kk] : 0.0;
        bad |= !gb_finite(xf[s]);
    }
    double tau = 1.0;
    if (FAM == LB_GAUSSIAN && rv) tau = a.tau_dev ? a.tau_dev[k] : a.tau;
    const double* yk = a.y + (size_t)k * N;
    const double* ok = a.offset ? a.offset + (size_t)k * N : nullptr;
    const double* wk = a.w ? a.w + (size_t)k * N : nullptr;

    // the tile elements e = t + 256 q of this thread as (row, column), stepped without a division
    const int row0 = t / D, col0 = t - row0 * D, dr = 256 / D, dc = 256 - dr * D;
    const int tile_e = GS_TN * D;
    for (int e = t; e < GS_TN * LD; e += 256) As[e] = 0.0;   // the columns D .. glm_dp(D) - 1 stay zero for the whole launch
    double pre[GS_AQ];
    {
        const int te = (int)(N < GS_TN ? N : GS_TN) * D;
#pragma unroll
        for (int q = 0; q < GS_AQ; ++q) {
            const int e = t + q * 256;
            pre[q] = e < te ? a.A[e] : 0.0;
        }
    }
    __syncthreads();

    v4d g[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) g[b] = v4d{0.0, 0.0, 0.0, 0.0};
    double lpacc = 0.0;

    for (long long n0 = 0; n0 < N; n0 += GS_TN) {
        const long long left = N - n0;
        const int tnv = (int)(left < GS_TN ? left : GS_TN);
        {                                     // registers -> LDS, the rows beyond N as zeros (the previous tile was consumed)
            int r = row0, c = col0;
#pragma unroll
            for (int q = 0; q < GS_AQ; ++q) {
                if (t + q * 256 < tile_e) As[r * LD + c] = pre[q];
                r += dr;
                c += dc;
                if (c >= D) {
                    c -= D;
                    ++r;
                }
            }
        }
        __syncthreads();
        {                                     // the next tile's loads: in flight while this one is used
            const long long left2 = left - GS_TN;
            const int te2 = (left2 < 0 ? 0 : (int)(left2 < GS_TN ? left2 : GS_TN)) * D;
            const double* An = a.A + (size_t)(n0 + GS_TN) * D;
#pragma unroll
            for (int q = 0; q < GS_AQ; ++q) {
                const int e = t + q * 256;
                pre[q] = e < te2 ? An[e] : 0.0;
            }
        }
        if (wave_live) {
#pragma unroll
            for (int j = 0; j < GS_TN / 16; ++j) {
                if (16 * j >= tnv) break;     // (uniform)
                // y, o, w of this lane's four entries: row li (problem k), obs n0 + 16 j + lg + 4 r
                double yv[4], ov[4], wv[4];
                bool use[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long n = n0 + 16 * j + lg + 4 * r;
                    const bool live = rv && n < N;
                    yv[r] = live ? yk[n] : 0.0;
                    ov[r] = live && ok ? ok[n] : 0.0;
                    wv[r] = wk ? (live ? wk[n] : 0.0) : 1.0;
                    use[r] = live && wv[r] > 0.0;
                }
                v4d eta = {0.0, 0.0, 0.0, 0.0};
                const double* ar = As + (16 * j + li) * LD + lg;
#pragma unroll
                for (int s = 0; s < KS; ++s) eta = GSMVI_MFMA_F64(ar[4 * s], xf[s], eta);
                v4d R = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double rr = 0.0, tt = 0.0;
                    const bool fine = lb_link<FAM, HAS_G, HAS_LP>(ok ? eta[r] + ov[r] : eta[r], yv[r], tau, rr, tt);
                    if (HAS_G) R[r] = use[r] ? wv[r] * rr : 0.0;
                    if (HAS_LP) lpacc += use[r] ? wv[r] * tt : 0.0;
                    if (FAM == LB_POISSON) bad |= use[r] && !fine;
                }
                if (HAS_G) {
                    const double* br = As + (16 * j + lg) * LD + li;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int b = 0; b < NB; ++b) g[b] = GSMVI_MFMA_F64(R[r], br[4 * r * LD + 16 * b], g[b]);
                }
            }
        }
        __syncthreads();                      // the next tile overwrites As
    }

    // the flags of the wave's 16 rows: bit i = some lane of row i (lanes i, i + 16, i + 32, i + 48) saw what flags it
    const unsigned long long bl = __ballot(bad);
    const unsigned flags = (unsigned)((bl | (bl >> 16) | (bl >> 32) | (bl >> 48)) & 0xffffu);
    if (HAS_G) {                              // register r of lane l: row lg + 4 r, column li + 16 b
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = lg + 4 * r;
            const long long mm = m0 + row;
            if (mm < a.M) {
                const double lam = a.lam_dev ? a.lam_dev[mm / a.nc] : a.lam;
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const int d = li + 16 * b;
                    if (d < D) {
                        const size_t at = (size_t)mm * D + d;
                        const double v = g[b][r] - lam * a.X[at];
                        a.G[at] = (flags >> row) & 1u ? qnan : v;
                    }
                }
            }
        }
    }
    if (HAS_LP) {                             // the four lane groups of a row, added in the order 0, 1, 2, 3
        const double s = ((__shfl(lpacc, li) + __shfl(lpacc, li + 16)) + __shfl(lpacc, li + 32)) + __shfl(lpacc, li + 48);
        if (lg == 0 && rv) {
            const double lam = a.lam_dev ? a.lam_dev[k] : a.lam;
            double xx = 0.0;
            for (int j = 0; j < D; ++j) {
                const double x = a.X[(size_t)m * D + j];
                xx += x * x;
            }
            a.lp[m] = (flags >> li) & 1u ? qnan : s - 0.5 * lam * xx;
        }
    }
}

template <int FAM, int NB>
static void gs_go_nb(int want, unsigned grid, size_t lds, hipStream_t st, const gs_args& a) {
    if (want == LB_G)
        hipLaunchKernelGGL((k_glm_shared_batched<NB, LB_G, FAM>), dim3(grid), dim3(256), lds, st, a);
    else if (want == LB_LP)
        hipLaunchKernelGGL((k_glm_shared_batched<NB, LB_LP, FAM>), dim3(grid), dim3(256), lds, st, a);
    else
        hipLaunchKernelGGL((k_glm_shared_batched<NB, LB_G | LB_LP, FAM>), dim3(grid), dim3(256), lds, st, a);
}

template <int FAM>
static void gs_go(int want, unsigned grid, size_t lds, hipStream_t st, const gs_args& a) {
    switch (glm_dp(a.D) / 16) {
        case 1: gs_go_nb<FAM, 1>(want, grid, lds, st, a); break;
        case 2: gs_go_nb<FAM, 2>(want, grid, lds, st, a); break;
        case 3: gs_go_nb<FAM, 3>(want, grid, lds, st, a); break;
        default: gs_go_nb<FAM, 4>(want, grid, lds, st, a); break;
    }
}

extern "C" {

int gsmvi_glm_shared_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int nc, int64_t N, int family, const double* A,
                                 const double* y, const double* offset, const double* weights, double noise_prec,
                                 const double* noise_prec_dev, double prior_prec, const double* prior_prec_dev, const double* X,
                                 double* G, double* lp) {
    // the model's checks are the per-problem entry's (its "K N D is too large" bounds y, offset and weights here, and A a fortiori)
    const glm_model m = {K, N, D, A, y, offset, nullptr, prior_prec, prior_prec_dev, noise_prec, noise_prec_dev};
    if (int st = glm_check_model(__func__, m, family, "N", true)) return st;
    GB_BAD(nc < 1, "nc must be at least 1");
    GB_BAD(nc > (INT64_MAX / 8 / D) / K, "K nc D is too large");
    GB_BAD(((int64_t)K * nc + GS_ROWS - 1) / GS_ROWS > 2147483647LL, "K nc is too large: at most 64 (2^31 - 1) rows in one launch");
    GB_BAD(!A || !y || !X, "NULL array");
    GB_BAD(!G && !lp, "give G or lp (or both)");
    const size_t ny = (size_t)K * N * 8, nk = (size_t)K * 8, nx = (size_t)K * nc * D * 8;
    if (int st = gb_check_overlaps(__func__, {{A, (size_t)N * D * 8, "A", GB_RD},
                                              {y, ny, "y", GB_RD},
                                              {offset, ny, "offset", GB_RD},
                                              {weights, ny, "weights", GB_RD},
                                              {noise_prec_dev, nk, "noise_prec_dev", GB_RD},
                                              {prior_prec_dev, nk, "prior_prec_dev", GB_RD},
                                              {X, nx, "X", GB_RD},
                                              {G, nx, "G", GB_WR},
                                              {lp, (size_t)K * nc * 8, "lp", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    const int want = (G ? LB_G : 0) | (lp ? LB_LP : 0);
    const gs_args a = {(long long)K * nc, N, D, nc, A, y, offset, weights, prior_prec, prior_prec_dev, noise_prec, noise_prec_dev,
                       X, G, lp};
    const unsigned grid = (unsigned)((a.M + GS_ROWS - 1) / GS_ROWS);
    const size_t lds = (size_t)gs_lds_doubles(D) * sizeof(double);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    glm_for_family(family, [&](auto fam) { gs_go<decltype(fam)::value>(want, grid, lds, st, a); });
    return gb_launched(ctx, GSMVI_PATH_BATCHED_TARGET, "k_glm_shared_batched");
}

// include/gsmvi_hip_debug.h: what a launch at D requests (exported by the debug library only); want: 1 = G, 2 = lp, 3 = both
int gsmvi_debug_glm_shared_batched_lds(int D, int want, int family, size_t* bytes, int* rows_per_workgroup) {
    GB_BAD(D < 1 || D > GB_MAX_D || want < 1 || want > 3 || family < GSMVI_GLM_LOGISTIC || family > GSMVI_GLM_GAUSSIAN || !bytes ||
               !rows_per_workgroup,
           "bad shape, want, family or NULL output");
    *bytes = (size_t)gs_lds_doubles(D) * sizeof(double);
    *rows_per_workgroup = GS_ROWS;
    return GSMVI_OK;
}

}  // extern "C"
