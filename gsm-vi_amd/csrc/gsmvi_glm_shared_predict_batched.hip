// Shared-design GLM posterior predictive: for K fitted Gaussians q_k = N(mu_k, Sigma_k) over the coefficients of K GLMs of one
// D <= 64, the predictive of the M rows of ONE matrix A_new (M, D) for every problem, with per-problem row weights, one launch
// ("Shared-design GLM predictive").
//
// The reference stops at the fitted (mean, cov) (examples/example_gsm.py:34-35 builds the model; nothing uses the fit): no twin.
// Row m of problem k is valid iff weights is null or v_km > 0 (not for 0 or NaN): the selection rule of
// gsmvi_glm_shared_hessian_batched_f64 and gsmvi_psis_loo_shared_batched_f64.  For a valid row eta_mean, eta_var, pmean and lpd
// are what gsmvi_glm_predict_batched_f64 (gsmvi_glm_predict_batched.hip, where the table of the four families is) defines for row
// m of a problem whose design is A_new; lpd is the density of one unit observation, not weighted; an invalid row has four NaN
// outputs, and its y and offset are never read; elpd[k] = sum over the valid rows of v_km lpd[k, m] in ascending m in one thread
// (v = 1 without weights), 0 for a problem without a valid row.
//   k_glm_shared_predict_batched<NT, FAM>
// Work mapping: k_glm_predict_batched's, with ONE tile of A_new per workgroup as in k_laplace_shared_batched: the slots of
// gsmvi_batched.h (gb_nt(D) threads per problem; four problems -- one wave each -- per 256-thread workgroup for D <= 16); Sigma_k
// and mu_k are staged per slot, zero-padded to Dp = 16 ceil(D / 16), row stride Dp + 1.  All 256 threads stage the rows n0 ..
// n0 + 31 of A_new once (zero-padded to Dp columns and to 32 rows, row stride Dp + 1; the next tile's loads are in flight in
// registers while the current one is consumed) and every slot reads that one copy: A_new is never held per problem, in device
// memory or in LDS.  Per tile a slot stages v, and y and o where v > 0, of its own 32 rows; then, with the operand order of
// k_glm_predict_batched: the butterfly for a . mu; T = A_tile Sigma_k on the fp64 MFMA (16 x 16 x 4), each T_nj multiplied by
// a_nj and butterfly-summed per block; and the row stage of gsmvi_glm_predict_stage.h, the one copy both kernels run.  The dot
// product and the quadratic form are formed for all 32 rows of the tile (a row's values depend on that row of A_new and on the
// slot's Sigma_k and mu_k alone); the row stage selects.  With one slot per workgroup the node values of the quadrature take the
// tile's place in LDS once v is known, as in k_glm_predict_batched; with four slots, which share the tile and run in lockstep,
// each slot has a node buffer of its own (8 rows x 65).
// Order: every sum of a row is taken in an order fixed by (D, Q) alone, so with weights null or 1.0 every output is
// k_glm_predict_batched's on the K-fold replicated A_new bit for bit, and with a 0 / 1 prefix that launch's with counts.
// Isolation: a slot reads and writes only slice k of every per-problem array and its own LDS; no atomics, no context workspace.
// A_new is shared: a non-finite entry in row m of it reaches row m of every problem, and only row m.  All barriers are uniform
// across the workgroup: a slot without a problem (K not a multiple of 4) has no valid row, stages the tile with the others and
// runs the barriers.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_glm_model.h"                 // glm_check_model, glm_dp, glm_for_family
#include "gsmvi_glm_predict_stage.h"         // GP_MAXQ, GP_LF, GP_QL, gp_row_stage
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

#define GSP_AQ 8       // tile elements per thread: LB_TN D / 256 <= 8
#define GSP_NROW 7     // per-row LDS arrays of a slot: y, o, v (the weight), m, s, lpd, bad

struct gsp_args {
    long long K, M;
    int D;
    const double* A;            // (M, D), shared
    const double* y;            // (K, M) or null
    const double* offset;       // (K, M) added to eta, or null
    const double* w;            // (K, M) row weights, or null (1 everywhere)
    double tau;                 // gaussian family: the noise precision of every problem ...
    const double* tau_dev;      // ... or (K) per-problem values on the device (null: `tau`)
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

// LDS doubles of the workgroup (the quadrature table, 3 x 64, and the tile region: the A tile, 32 x (Dp + 1), which with one slot
// also holds the node values of 32 rows, 32 x 65) and of one slot (Sigma, Dp x (Dp + 1); mu, Dp; with four slots the node values
// of 8 rows, 8 x 65; seven per-row arrays and the Dp / 16 partial sums of v, 32 each).
// D = 64: 192 + 2080 + 4576 = 6848 doubles, 53.5 KB.  Four slots of D = 16: 192 + 544 + 4 x 1064 = 4992 doubles, 39 KB
__host__ __device__ inline int gsp_wg_doubles(int D, int nt) {
    const int t = LB_TN * (glm_dp(D) + 1), f = nt == 256 ? LB_TN * GP_LF : 0;
    return 3 * GP_MAXQ + (t > f ? t : f);
}
__host__ __device__ inline int gsp_slot_doubles(int D, int nt) {
    const int Dp = glm_dp(D);
    return Dp * (Dp + 1) + Dp + (nt == 256 ? 0 : (nt / GP_QL) * GP_LF) + GSP_NROW * LB_TN + (Dp / 16) * LB_TN;
}

template <int NT, int FAM>
__global__ __launch_bounds__(256) void k_glm_shared_predict_batched(gsp_args a) {
    extern __shared__ double gsp_sm[];
    constexpr int PPW = 256 / NT, NW = NT / 64, NG = NT / LB_TN;
    const int D = a.D, Q = a.Q, nb = (D + 15) >> 4, Dp = nb * 16, lda = Dp + 1, DD = D * D;
    const long long M = a.M;
    const int t = threadIdx.x, slot = t / NT, l = t % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K, hasy = a.y != nullptr;
    const bool quad = FAM == LB_LOGISTIC || (hasy && FAM != LB_GAUSSIAN);       // (uniform in the launch)
    const size_t kk = (size_t)(valid ? k : 0);
    double* gt = gsp_sm;                      // the nodes, the logarithms of the weights, the weights: one copy per workgroup
    double* gl = gt + GP_MAXQ;
    double* gw = gl + GP_MAXQ;
    double* As = gw + GP_MAXQ;                // 32 x lda  the workgroup's tile of A_new; with one slot later the node values
    double* Ss = gsp_sm + gsp_wg_doubles(D, NT) + (size_t)slot * gsp_slot_doubles(D, NT);
    double* xs = Ss + Dp * lda;               // Dp  mu_k (zeros beyond D)
    double* Fs = xs + Dp;                     // four slots: the node values of 8 rows
    double* Ys = Fs + (NT == 256 ? 0 : (NT / GP_QL) * GP_LF);
    double* Os = Ys + LB_TN;
    double* Vs = Os + LB_TN;                  // the weights of the tile's rows (1 without weights; 0 beyond M and in an empty slot)
    double* Ms = Vs + LB_TN;                  // m of the tile's rows
    double* Hs = Ms + LB_TN;                  // s = sqrt(2 v+)
    double* Ls = Hs + LB_TN;                  // lpd
    double* Bd = Ls + LB_TN;                  // 1.0 where m or v is not finite
    double* Vp = Bd + LB_TN;                  // nb x 32 partial sums of v
    double* F0 = NT == 256 ? As : Fs;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    const double* yk = hasy ? a.y + kk * (size_t)M : nullptr;
    const double* ok_ = a.offset ? a.offset + kk * (size_t)M : nullptr;
    const double* wk = a.w ? a.w + kk * (size_t)M : nullptr;
    double* em = a.eta_mean + kk * (size_t)M;
    double* ev = a.eta_var + kk * (size_t)M;
    double* pm = a.pmean + kk * (size_t)M;
    double* lp = hasy ? a.lpd + kk * (size_t)M : nullptr;
    double tau = 1.0;
    if (FAM == LB_GAUSSIAN && valid) tau = a.tau_dev ? a.tau_dev[k] : a.tau;
    if (t < Q) {
        const double lw = a.gh_logw[t];
        gt[t] = a.gh_t[t];
        gl[t] = lw;
        gw[t] = exp(lw);
    }
    for (int e = t; e < LB_TN * lda; e += 256) As[e] = 0.0;         // the padding columns start at zero
    for (int e = l; e < Dp * Dp; e += NT) {                         // Sigma_k as given, both triangles, zeros beyond D
        const int i = e / Dp, j = e - i * Dp;
        Ss[i * lda + j] = valid && i < D && j < D ? a.cov[kk * DD + (size_t)i * D + j] : 0.0;
    }
    if (l < Dp) xs[l] = valid && l < D ? a.mean[kk * D + l] : 0.0;
    __syncthreads();                          // the zeros are in place before any thread writes the first tile

    const int wv = l >> 6, ln = l & 63, cc = ln & 15, ks = ln >> 4, nblk = 2 * nb;
    // the tile elements e = t + 256 q of this thread as (row, column), stepped without a division: the whole workgroup stages A
    const int row0 = t / D, col0 = t - row0 * D, dr = 256 / D, dc = 256 - dr * D;
    const int en = l / NG, eg = l % NG;       // the m pass: row en of the tile, columns eg, eg + NG, ..
    const int pad = Dp - D;

    double pre[GSP_AQ], ypre = 0.0, opre = 0.0, vpre = 0.0;
    {
        const int tnv = (int)(M < LB_TN ? M : LB_TN), te = tnv * D;
#pragma unroll
        for (int q = 0; q < GSP_AQ; ++q) {
            const int e = t + q * 256;
            pre[q] = e < te ? a.A[e] : 0.0;
        }
        if (valid && l < tnv) {               // (v = 0 in the rows beyond M: they are not selected)
            vpre = wk ? wk[l] : 1.0;
            if (vpre > 0.0) {                 // y and o of a row that is not selected are never read
                if (hasy) ypre = yk[l];
                if (ok_) opre = ok_[l];
            }
        }
    }
    double eacc = 0.0;

    for (long long n0 = 0; n0 < M; n0 += LB_TN) {
        const long long left = M - n0;
        const int tnv = (int)(left < LB_TN ? left : LB_TN);
        {                                     // registers -> LDS: the whole tile, zeros in the rows beyond M
            int r = row0, c = col0;
#pragma unroll
            for (int q = 0; q < GSP_AQ; ++q) {
                if (t + q * 256 < LB_TN * D) As[r * lda + c] = pre[q];
                r += dr;
                c += dc;
                if (c >= D) {
                    c -= D;
                    ++r;
                }
            }
            if (NT == 256 && quad && pad > 0) // the node values of the last tile lay over the padding columns
                for (int e = t; e < LB_TN * pad; e += 256) {
                    const int r2 = e / pad;
                    As[r2 * lda + D + (e - r2 * pad)] = 0.0;
                }
        }
        if (l < LB_TN) {
            Ys[l] = ypre;
            Os[l] = opre;
            Vs[l] = vpre;
        }
        __syncthreads();
        {                                     // the next tile's loads: in flight while this one is consumed
            const long long left2 = left - LB_TN;
            const int tnv2 = left2 < 0 ? 0 : (int)(left2 < LB_TN ? left2 : LB_TN), te2 = tnv2 * D;
            const double* An = a.A + (size_t)(n0 + LB_TN) * D;
#pragma unroll
            for (int q = 0; q < GSP_AQ; ++q) {
                const int e = t + q * 256;
                pre[q] = e < te2 ? An[e] : 0.0;
            }
            ypre = 0.0;
            opre = 0.0;
            vpre = 0.0;
            if (valid && l < tnv2) {
                vpre = wk ? wk[n0 + LB_TN + l] : 1.0;
                if (vpre > 0.0) {
                    if (hasy) ypre = yk[n0 + LB_TN + l];
                    if (ok_) opre = ok_[n0 + LB_TN + l];
                }
            }
        }
        if (valid) {                          // m of row en: NG adjacent lanes take the columns eg + i NG, then a butterfly
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
            if (tt < nblk && valid) {         // (wave-uniform)
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
        // the row stage (gsmvi_glm_predict_stage.h) on the rows with a weight > 0; a slot without a problem has none
        gp_row_stage<NT, FAM, true>(hasy, quad, Q, nb, l, tnv, n0, tau, gt, gl, gw, Vp, Ms, Ys, Vs, Hs, Bd, Ls, F0, em, ev, pm, lp);
        if (valid && l < tnv && !(Vs[l] > 0.0)) {                   // the rows that are not selected
            em[n0 + l] = qnan;
            ev[n0 + l] = qnan;
            pm[n0 + l] = qnan;
            if (hasy) lp[n0 + l] = qnan;
        }
        // elpd: ascending m in one thread.  A row that is not valid adds +0.0 by a select (its Ls is stale; eacc is never -0.0, so
        // the bits are those of skipping it), which keeps the loop free of branches and its LDS loads in flight together
        if (hasy && l == NT - 1) {
#pragma unroll 8
            for (int n = 0; n < LB_TN; ++n) {
                const double v = Vs[n], t = Ls[n];
                eacc += v > 0.0 ? v * t : 0.0;
            }
        }
        __syncthreads();                      // the next tile overwrites the tile region and the per-row arrays
    }
    if (valid && hasy && l == NT - 1) a.elpd[k] = eacc;
}

// dynamic LDS bytes of a launch at D: at most 53.5 KB, below the default limit of 64 KB, so no kernel attribute is needed
static size_t gsp_launch_lds(int D, int* ppw) {
    const int nt = gb_nt(D);
    *ppw = 256 / nt;
    return ((size_t)gsp_wg_doubles(D, nt) + (size_t)*ppw * gsp_slot_doubles(D, nt)) * sizeof(double);
}

extern "C" {

// the model's checks are the per-problem entry's (its "K M D is too large" bounds offset, y, weights and the outputs, and A a
// fortiori; K is bounded by the slot packing, as in the shared-design Laplace entries)
int gsmvi_glm_shared_predict_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t M, int family, const double* A,
                                         const double* offset, const double* y, const double* weights, double noise_prec,
                                         const double* noise_prec_dev, const double* mean, const double* cov, int Q,
                                         const double* gh_t, const double* gh_logw, double* eta_mean, double* eta_var, double* pmean,
                                         double* lpd, double* elpd) {
    const glm_model m = {K, M, D, A, y, offset, nullptr, 0.0, nullptr, noise_prec, noise_prec_dev};
    if (int st = glm_check_model(__func__, m, family, "M", false)) return st;
    GB_BAD(Q < 1 || Q > GP_MAXQ, "Q must be in [1, 64]");
    GB_BAD(!A || !mean || !cov || !gh_t || !gh_logw || !eta_mean || !eta_var || !pmean, "NULL array");
    GB_BAD((y != nullptr) != (lpd != nullptr) || (y != nullptr) != (elpd != nullptr),
           "lpd and elpd are required with y and only with it");
    const size_t nm = (size_t)K * M * 8, nx = (size_t)K * D * 8, nq = (size_t)Q * 8;
    const gb_arr all[] = {{A, (size_t)M * D * 8, "A", GB_RD},       // (one (M, D) matrix here)
                          {y, nm, "y", GB_RD},
                          {offset, nm, "offset", GB_RD},
                          {weights, nm, "weights", GB_RD},
                          {noise_prec_dev, (size_t)K * 8, "noise_prec_dev", GB_RD},
                          {mean, nx, "mean", GB_RD},
                          {cov, nx * D, "cov", GB_RD},
                          {gh_t, nq, "gh_t", GB_RD},
                          {gh_logw, nq, "gh_logw", GB_RD},
                          {eta_mean, nm, "eta_mean", GB_WR},
                          {eta_var, nm, "eta_var", GB_WR},
                          {pmean, nm, "pmean", GB_WR},
                          {lpd, nm, "lpd", GB_WR},
                          {elpd, (size_t)K * 8, "elpd", GB_WR}};
    if (int st = gb_check_overlaps(__func__, all, all + sizeof all / sizeof all[0])) return st;
    GB_BAD(!ctx, "ctx is NULL");
    const gsp_args a = {K, M, D, A, y, offset, weights, noise_prec, noise_prec_dev, mean, cov, gh_t, gh_logw, eta_mean, eta_var,
                        pmean, lpd, elpd, Q};
    int ppw;
    const size_t lds = gsp_launch_lds(D, &ppw);
    const unsigned grid = (unsigned)((K + ppw - 1) / ppw);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    glm_for_family(family, [&](auto fam) {
        if (ppw == 4)
            hipLaunchKernelGGL((k_glm_shared_predict_batched<64, decltype(fam)::value>), dim3(grid), dim3(256), lds, st, a);
        else
            hipLaunchKernelGGL((k_glm_shared_predict_batched<256, decltype(fam)::value>), dim3(grid), dim3(256), lds, st, a);
    });
    // the pair of bits is this kernel's alone (include/gsmvi_hip.h)
    return gb_launched(ctx, GSMVI_PATH_BATCHED_PREDICT | GSMVI_PATH_BATCHED_TARGET, "k_glm_shared_predict_batched");
}

}  // extern "C"
