// Batched GLM posterior predictive: for K fitted Gaussians q_k = N(mu_k, Sigma_k) over the coefficients of K GLMs of one D <= 64,
// the predictive of M new rows per problem, one launch ("Batched GLM predictive").
//
// The reference stops at the fitted (mean, cov) (examples/example_gsm.py:34-35 builds the model; nothing uses the fit): no twin.
// Under q_k the linear predictor of a new row a is one-dimensional Gaussian, eta ~ N(m, v) with
//   m = a . mu_k + o,   v = a^T Sigma_k a,   v+ = max(v, 0),   s = sqrt(2 v+),   eta_q = m + s t_q   (Gauss-Hermite nodes t_q)
// so every predictive quantity is the quadratic form followed by a closed form or a sum over Q nodes:
//   family     pmean = E[E[y | eta]]                        lpd = log E[p(y | eta)]  (normalised)
//   gaussian   m                                            -log(2 pi (v+ + 1 / tau)) / 2 - (y - m)^2 / (2 (v+ + 1 / tau))
//   probit     Phi(m / sqrt(1 + v+))  (erfc)                LSE_q(logw_q + t(eta_q, y)) - log(pi) / 2
//   poisson    exp(m + v+ / 2)                              LSE_q(logw_q + y eta_q - e^eta_q) - log(pi) / 2 - lgamma(y + 1)
//   logistic   sum_q exp(logw_q) sigma(eta_q) / sqrt(pi)    LSE_q(logw_q + t(eta_q, y)) - log(pi) / 2
// with t the family's t of lb_link (gsmvi_glm_link.h), sigma(eta) = -r(eta, y = 0) of the same link, LSE = max first, then the
// sum of exp(. - max) in ascending q, and elpd[k] = sum_{n < n_k} lpd[k, n] in row order in one thread.
//   k_glm_predict_batched<NT, FAM>
// Work mapping: the slots of gsmvi_batched.h (gb_nt(D) threads per problem; four problems -- one wave each -- per 256-thread
// workgroup for D <= 16), as k_laplace_batched.  Sigma_k is staged once in LDS, zero-padded to Dp = 16 ceil(D / 16), row stride
// Dp + 1, mu_k beside it.  A slot walks the rows of A_k in tiles of LB_TN = 32, staged zero-padded to Dp columns (row stride
// Dp + 1); the next tile's loads are in flight while the current one is consumed.  Per tile:
//   m     NT / 32 adjacent lanes share a row's dot product (a butterfly over them), one of them adds the offset;
//   v     T = A_tile Sigma_k (32 x Dp by Dp x Dp) on the fp64 MFMA (16 x 16 x 4): block (rb, jb) of T takes the A operand
//         a_{16 rb + c, 4 s + ks} from the tile and the B operand Sigma_{4 s + ks, 16 jb + c}, Dp / 4 steps; 2 Dp / 16 blocks, at
//         most two per wave.  Each accumulator entry T_nj is multiplied by a_nj, the 16 lanes of a row's block are summed by a
//         butterfly, and thread n adds the Dp / 16 partial sums in ascending block order;
//   row   thread n < 32 forms v+, s, the closed forms and the row's NaN rule;
//   quad  the tile's LDS is free by now and holds the node values: 8 adjacent lanes share a row (32 rows at once with 256
//         threads, 8 rows at a time with 64), lane g takes the nodes g, g + 8, ..; the maximum is a butterfly over the 8 lanes,
//         and one of them sums the Q values in ascending q from LDS.
// `row` and `quad` are gp_row_stage of gsmvi_glm_predict_stage.h, the one copy shared with k_glm_shared_predict_batched.
// Order: every sum of a row is taken in an order fixed by D and Q alone; elpd runs n = 0 .. n_k - 1 in one thread.  A slot reads
// and writes only slice k of every array and every slot of a workgroup runs the same barriers.  Rows n >= n_k are never loaded;
// their outputs are NaN.  A row whose m or v is not finite has NaN outputs (and makes elpd[k] NaN).  No context workspace.
// The new rows are a glm_model (gp_args::m: N = M, y or null, no prior): its checks, overlap entries, family dispatch and
// per-problem prologue are gsmvi_glm_model.h's, shared with the score and Laplace entries.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_glm_model.h"
#include "gsmvi_glm_predict_stage.h"      // GP_MAXQ, GP_LF, GP_QL, gp_row_stage
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

#define GP_AQ 8        // tile elements per thread: LB_TN D / NT <= 8 in both packings
#define GP_NROW 6      // per-row LDS arrays of a tile: y, o, m, s, lpd, bad

struct gp_args {
    glm_model m;                // the new rows: N = M, y (K, M) or null, no prior
    const double* mean;         // (K, D)
    const double* cov;          // (K, D, D)
    const double* gh_t;         // (Q)
    const double* gh_logw;      // (Q)
    double* eta_mean;           // (K, M)
    double* eta_var;            // (K, M)
    double* pmean;              // (K, M)
    double* lpd;                // (K, M), with y
    double* elpd;               // (K), with y
    int Q;
};

// doubles of the tile region: the A tile (32 x (Dp + 1)), later the node values of NT / 8 rows (GP_LF each)
__host__ __device__ inline int gp_tile_doubles(int D, int nt) {
    const int t = LB_TN * (glm_dp(D) + 1), f = (nt / GP_QL) * GP_LF;
    return t > f ? t : f;
}
// LDS doubles per problem: Sigma (Dp x (Dp + 1)), mu (Dp), the tile region, six per-row arrays and the Dp / 16 partial sums of v
// (32 each).  D = 64: 6624 doubles; with the workgroup's quadrature table (3 x 64) 53.25 KB.  Four problems of D = 16: 34.5 KB
__host__ __device__ inline int gp_lds_doubles(int D, int nt) {
    const int Dp = glm_dp(D);
    return Dp * (Dp + 1) + Dp + gp_tile_doubles(D, nt) + GP_NROW * LB_TN + (Dp / 16) * LB_TN;
}

template <int NT, int FAM>
__global__ __launch_bounds__(256) void k_glm_predict_batched(gp_args a) {
    extern __shared__ double gp_sm[];
    constexpr int PPW = 256 / NT, NW = NT / 64, NG = NT / LB_TN;
    const int D = a.m.D, Q = a.Q, nb = (D + 15) >> 4, Dp = nb * 16, lda = Dp + 1, DD = D * D;
    const long long M = a.m.N;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.m.K, hasy = a.m.y != nullptr;
    const bool quad = FAM == LB_LOGISTIC || (hasy && FAM != LB_GAUSSIAN);       // (uniform in the launch)
    const size_t kk = (size_t)(valid ? k : 0);
    double* gt = gp_sm;                       // the nodes, the logarithms of the weights, the weights: one copy per workgroup
    double* gl = gt + GP_MAXQ;
    double* gw = gl + GP_MAXQ;
    double* Ss = gw + GP_MAXQ + (size_t)slot * gp_lds_doubles(D, NT);
    double* xs = Ss + Dp * lda;               // Dp  mu_k (zeros beyond D)
    double* As = xs + Dp;                     // the tile; in the quadrature the node values
    double* Ys = As + gp_tile_doubles(D, NT);
    double* Os = Ys + LB_TN;
    double* Ms = Os + LB_TN;                  // m of the tile's rows
    double* Hs = Ms + LB_TN;                  // s = sqrt(2 v+)
    double* Ls = Hs + LB_TN;                  // lpd
    double* Bd = Ls + LB_TN;                  // 1.0 where m or v is not finite
    double* Vp = Bd + LB_TN;                  // nb x 32 partial sums of v
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    const double* Ak = a.m.A + kk * (size_t)M * D;
    const double* yk = hasy ? a.m.y + kk * (size_t)M : nullptr;
    const double* ok_ = a.m.offset ? a.m.offset + kk * (size_t)M : nullptr;
    double* em = a.eta_mean + kk * (size_t)M;
    double* ev = a.eta_var + kk * (size_t)M;
    double* pm = a.pmean + kk * (size_t)M;
    double* lp = hasy ? a.lpd + kk * (size_t)M : nullptr;
    const glm_problem pk = glm_problem_of<FAM>(a.m, k, valid);
    const long long nk = pk.nk;               // the rows that count (a slot without a problem: none, so nothing is loaded)
    const double tau = pk.tau;
    if ((int)threadIdx.x < Q) {
        const double lw = a.gh_logw[threadIdx.x];
        gt[threadIdx.x] = a.gh_t[threadIdx.x];
        gl[threadIdx.x] = lw;
        gw[threadIdx.x] = exp(lw);
    }
    for (int e = l; e < LB_TN * lda; e += NT) As[e] = 0.0;          // the padding columns start at zero
    for (int e = l; e < Dp * Dp; e += NT) {                         // Sigma_k as given, both triangles, zeros beyond D
        const int i = e / Dp, j = e - i * Dp;
        Ss[i * lda + j] = valid && i < D && j < D ? a.cov[kk * DD + (size_t)i * D + j] : 0.0;
    }
    if (l < Dp) xs[l] = valid && l < D ? a.mean[kk * D + l] : 0.0;
    __syncthreads();                          // the zeros are in place before any thread writes the first tile

    const int wv = l >> 6, ln = l & 63, cc = ln & 15, ks = ln >> 4, nblk = 2 * nb;
    // the tile elements e = l + q NT of this thread as (row, column), stepped without a division
    const int row0 = l / D, col0 = l - row0 * D, dr = NT / D, dc = NT - dr * D;
    const int en = l / NG, eg = l % NG;       // the m pass: row en of the tile, columns eg, eg + NG, ..
    const int pad = Dp - D;

    double pre[GP_AQ], ypre = 0.0, opre = 0.0;
    {
        const int tnv = (int)(nk < LB_TN ? nk : LB_TN), te = tnv * D;
#pragma unroll
        for (int q = 0; q < GP_AQ; ++q) {
            const int e = l + q * NT;
            pre[q] = e < te ? Ak[e] : 0.0;
        }
        if (l < tnv) {
            if (hasy) ypre = yk[l];
            if (ok_) opre = ok_[l];
        }
    }
    double eacc = 0.0;

    for (long long n0 = 0; n0 < M; n0 += LB_TN) {
        const long long left = nk - n0;
        const int tnv = left < 0 ? 0 : (int)(left < LB_TN ? left : LB_TN);
        // a tile without a row that counts does none of the work below: it only runs the barriers, which must stay uniform
        // across the slots of a workgroup (tnv is uniform in the slot)
        if (tnv > 0) {                        // registers -> LDS: the whole tile, zeros in the rows that do not count
            int r = row0, c = col0;
#pragma unroll
            for (int q = 0; q < GP_AQ; ++q) {
                if (l + q * NT < LB_TN * D) As[r * lda + c] = pre[q];
                r += dr;
                c += dc;
                if (c >= D) {
                    c -= D;
                    ++r;
                }
            }
            if (quad && pad > 0)              // the node values of the last tile lay over the padding columns
                for (int e = l; e < LB_TN * pad; e += NT) {
                    const int r2 = e / pad;
                    As[r2 * lda + D + (e - r2 * pad)] = 0.0;
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
            for (int q = 0; q < GP_AQ; ++q) {
                const int e = l + q * NT;
                pre[q] = e < te2 ? An[e] : 0.0;
            }
            ypre = 0.0;
            opre = 0.0;
            if (l < tnv2) {
                if (hasy) ypre = yk[n0 + LB_TN + l];
                if (ok_) opre = ok_[n0 + LB_TN + l];
            }
        }
        if (tnv > 0) {                        // m of row en: NG adjacent lanes take the columns eg + i NG, then a butterfly
            const double* ar = As + en * lda;
            double m = 0.0;
            for (int j = eg; j < D; j += NG) m = fma(ar[j], xs[j], m);
#pragma unroll
            for (int o = NG / 2; o > 0; o >>= 1) m += __shfl_xor(m, o);
            m += Os[en];
            if (eg == 0) Ms[en] = m;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {         // v: block (rb, jb) of T = A_tile Sigma, then sum_j T_nj a_nj over the block's columns
            const int tt = wv + q * NW;
            if (tt < nblk && tnv > 0) {       // (wave-uniform)
                const int rb = tt & 1, jb = tt >> 1;
                const double* pa = As + (16 * rb + cc) * lda + ks;
                const double* pb = Ss + ks * lda + 16 * jb + cc;
                v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
                for (int s = 0; s < Dp; s += 4) acc = GSMVI_MFMA_F64(pa[s], pb[s * lda], acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = 16 * rb + ks + 4 * r;
                    double p = acc[r] * As[n * lda + 16 * jb + cc];
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) p += __shfl_xor(p, o);
                    if (cc == 0) Vp[jb * LB_TN + n] = p;
                }
            }
        }
        __syncthreads();
        // the row stage (gsmvi_glm_predict_stage.h, one copy for this kernel and k_glm_shared_predict_batched): v, the NaN rule,
        // the closed forms, then the quadrature over the tile's LDS, where the link is called (lb_link<FAM, ..>), not restated
        gp_row_stage<NT, FAM, false>(hasy, quad, Q, nb, l, tnv, n0, tau, gt, gl, gw, Vp, Ms, Ys, nullptr, Hs, Bd, Ls, As, em, ev, pm,
                                     lp);
        if (hasy && l == NT - 1)
            for (int n = 0; n < tnv; ++n) eacc += Ls[n];
        __syncthreads();                      // the next tile overwrites the tile region and the per-row arrays
    }

    if (!valid) return;
    for (long long n = nk + l; n < M; n += NT) {                    // the rows that do not count
        em[n] = qnan;
        ev[n] = qnan;
        pm[n] = qnan;
        if (hasy) lp[n] = qnan;
    }
    if (hasy && l == NT - 1) a.elpd[k] = eacc;
}

// dynamic LDS bytes of a launch at D: at most 53.25 KB, below the default limit of 64 KB, so no kernel attribute is needed
static size_t gp_launch_lds(int D, int* ppw) {
    const int nt = gb_nt(D);
    *ppw = 256 / nt;
    return ((size_t)3 * GP_MAXQ + (size_t)*ppw * gp_lds_doubles(D, nt)) * sizeof(double);
}

extern "C" {

int gsmvi_glm_predict_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t M, int family, const double* A,
                                  const double* offset, const double* y, const int* counts_dev, double noise_prec,
                                  const double* noise_prec_dev, const double* mean, const double* cov, int Q, const double* gh_t,
                                  const double* gh_logw, double* eta_mean, double* eta_var, double* pmean, double* lpd,
                                  double* elpd) {
    const glm_model m = {K, M, D, A, y, offset, counts_dev, 0.0, nullptr, noise_prec, noise_prec_dev};
    if (int st = glm_check_model(__func__, m, family, "M", false)) return st;
    GB_BAD(Q < 1 || Q > GP_MAXQ, "Q must be in [1, 64]");
    GB_BAD(!A || !mean || !cov || !gh_t || !gh_logw || !eta_mean || !eta_var || !pmean, "NULL array");
    GB_BAD((y != nullptr) != (lpd != nullptr) || (y != nullptr) != (elpd != nullptr),
           "lpd and elpd are required with y and only with it");
    const size_t nm = (size_t)K * M * 8, nx = (size_t)K * D * 8, nq = (size_t)Q * 8;
    if (int st = gb_check_overlaps(__func__, m, {{mean, nx, "mean", GB_RD}, {cov, nx * D, "cov", GB_RD}, {gh_t, nq, "gh_t", GB_RD},
                                                 {gh_logw, nq, "gh_logw", GB_RD}, {eta_mean, nm, "eta_mean", GB_WR},
                                                 {eta_var, nm, "eta_var", GB_WR}, {pmean, nm, "pmean", GB_WR}, {lpd, nm, "lpd", GB_WR},
                                                 {elpd, (size_t)K * 8, "elpd", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    const gp_args a = {m, mean, cov, gh_t, gh_logw, eta_mean, eta_var, pmean, lpd, elpd, Q};
    int ppw;
    const size_t lds = gp_launch_lds(D, &ppw);
    const unsigned grid = (unsigned)((K + ppw - 1) / ppw);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    glm_for_family(family, [&](auto fam) {
        if (ppw == 4)
            hipLaunchKernelGGL((k_glm_predict_batched<64, decltype(fam)::value>), dim3(grid), dim3(256), lds, st, a);
        else
            hipLaunchKernelGGL((k_glm_predict_batched<256, decltype(fam)::value>), dim3(grid), dim3(256), lds, st, a);
    });
    return gb_launched(ctx, GSMVI_PATH_BATCHED_PREDICT, "k_glm_predict_batched");
}

}  // extern "C"
