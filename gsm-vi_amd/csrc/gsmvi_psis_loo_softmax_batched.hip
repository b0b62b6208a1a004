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
//       reference class's exp(-m) last.  No eta is stored and the registers do not depend on C.  Only lanes whose column is a
//       valid observation run the comparisons and exponentials.  The tile's l_si stay in LDS (NI x S doubles).
//       The padding rule: with P % 4 != 0 the k positions 4 j + kq >= P of class c would address x entries of class c + 1 (past
//       column D - 1 at the last class), and there the B operand holds a padded zero: 0 x non-finite = NaN would flag a draw
//       that the definition does not.  The X tile keeps the memory layout and the A operand is MASKED instead: a lane whose k
//       position is >= P feeds 0.0 and loads nothing, so a padded position is 0 x 0 on both sides and no LDS word outside the
//       row's D entries is read.  (A padded layout, Pp columns per class, takes up to 64 x 257 doubles at (65, 1): it would not
//       leave room for one observation at S = 4096.)  A non-finite x_{s, c P + j} needs no flag of its own: it meets a_ij in the
//       dot of class c of every valid row, the product is +-inf or NaN (0 x inf included), and so is the sum: the draw's l_si is
//       NaN for every valid observation of the problem, by the non-finite-eta rule.
//   (2) per observation of the tile: the body of k_psis_loo_batched (gsmvi_psis_loo_batched.hip, its twin: the statements are
//       copied, not shared, so that file's object code stays as it is; change both together): rho_s = logr_s - l_si into the
//       stage's array, ps_stage (gsmvi_psis_stage.h), then the two log-sum-exps through ps_max and ps_sum.
// The tiles of (1) lie over the stage's LDS (dead before the first stage starts).  NI is the largest count, at most PLS_NI_CAP,
// whose l_si fit beside that region in GB_LDS_MAX.  Every sum is a fixed tree and there are no atomics; every thread of a
// workgroup runs the same barriers whatever the verdicts; a workgroup reads only slice k of the inputs and writes only its own
// (k, i) entries.  A label is compared, never used as an index.  Inputs are only read; no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_psis_stage.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

#define PLS_TR 64       // draws per tile of X_k: one 16-row MFMA block per wave
#define PLS_NB 16       // rows of the A_k tile: the MFMA's 16 columns, NI of them in use
#ifndef PLS_NI_CAP
#define PLS_NI_CAP 4    // observations per workgroup at most (fewer observations, more workgroups per CU)
#endif

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
    const double* logr;         // (K, S) lp - log q of the problem-level run
    const double* lw;           // (K, S) its normalised smoothed log weights
    double* loglik;             // (K, N, S) or null
    double* elpd;               // (K, N) each
    double* lpd;
    double* khat;
    double* ess;
    int* info;                  // (K, N) 0; -1 non-finite ratios; -2 tail too short; -3 not a valid row
};

__host__ __device__ inline int pls_pp(int P) { return ((P + 3) >> 2) << 2; }

// doubles of the shared region: the stage's arrays and its S2 indices, or the X tile, the A tile and the 16 labels
__host__ __device__ inline int pls_region_doubles(int C, int P, int S, int S2) {
    const int stage = ps_lds_doubles(S, S2) + S2 / 2, tiles = PLS_TR * (((C - 1) * P) | 1) + PLS_NB * (pls_pp(P) + 1) + PLS_NB;
    return stage > tiles ? stage : tiles;
}

// C >= 2 and 1 <= (C - 1) P <= 64, without forming a product that could overflow
static bool pls_shape_ok(int C, int P) { return C >= 2 && P >= 1 && C - 1 <= GB_MAX_D && P <= GB_MAX_D && (C - 1) * P <= GB_MAX_D; }

static int pls_tile(int C, int P, int S) {
    int S2, M;
    ps_sizes(S, &S2, &M);
    const int fit = (GB_LDS_MAX / 8 - pls_region_doubles(C, P, S, S2)) / S;     // >= 2 at S = 4096
    return fit < PLS_NI_CAP ? fit : PLS_NI_CAP;
}

// eta_c of the lane's four (draw, observation) pairs: the MFMA chain of class c.  px points at the lane's row of the X tile plus
// kq, pb at its row of the A tile plus kq; a k position 4 j + kq >= P feeds 0.0 from the A side and loads nothing.
__device__ __forceinline__ v4d pls_eta(const double* px, const double* pb, int c, int P, int Pp, int kq) {
    const double* pa = px + c * P;
    v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < Pp; j += 4) acc = GSMVI_MFMA_F64(j + kq < P ? pa[j] : 0.0, pb[j], acc);
    return acc;
}

__global__ __launch_bounds__(256) void k_psis_loo_softmax_batched(pls_args a) {
    extern __shared__ double pls_sm[];
    const int l = threadIdx.x, S = a.S, S2 = a.S2, M = a.M, NI = a.NI;
    const int P = a.P, Cm = a.C - 1, D = a.D, Pp = pls_pp(P), lda = Pp + 1, ldx = D | 1;
    const long long N = a.N;
    const size_t k = blockIdx.x / a.ntile;
    const long long i0 = (long long)(blockIdx.x - (unsigned)k * a.ntile) * NI;       // the tile's first observation
    const int ni = (int)(N - i0 < NI ? N - i0 : NI);
    long long nk = N;
    if (a.counts) {
        const long long c = a.counts[k];
        nk = c < 0 ? 0 : (c > N ? N : c);
    }
    const int nv = (int)(nk - i0 < 0 ? 0 : (nk - i0 < ni ? nk - i0 : ni));            // its valid observations: the first nv
    const ps_lds sm = ps_carve(pls_sm, reinterpret_cast<int*>(pls_sm + ps_lds_doubles(S, S2)), S, S2);
    double* Xs = pls_sm;                      // PLS_TR x ldx  a tile of draws          (over the stage's arrays)
    double* As = Xs + PLS_TR * ldx;           // PLS_NB x lda  the tile's rows of A_k, zero-padded
    int* ys = reinterpret_cast<int*>(As + PLS_NB * lda);    // PLS_NB labels (in PLS_NB doubles)
    double* ell = pls_sm + a.U;               // NI x S        l_si of the tile
    const size_t ks = k * (size_t)S, kn = k * (size_t)N + (size_t)i0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL), inf = __builtin_huge_val();

    // ---- (1) l_si of the tile's valid observations ------------------------------------------------------------------------
    if (nv > 0) {                             // (uniform in the workgroup)
        const double* Ak = a.A + kn * P;
        for (int e = l; e < PLS_NB * lda; e += 256) {
            const int r = e / lda, j = e - r * lda;
            As[e] = r < nv && j < P ? Ak[(size_t)r * P + j] : 0.0;
        }
        if (l < PLS_NB) ys[l] = l < nv ? a.labels[kn + l] : 0;
        const double* Xk = a.X + ks * D;
        const int wv = l >> 6, ln = l & 63, cc = ln & 15, kq = ln >> 4;
        for (int t0 = 0; t0 < S; t0 += PLS_TR) {
            __syncthreads();                  // the previous tile's readers are done
            for (int e = l; e < PLS_TR * ldx; e += 256) {
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
                    const v4d acc = pls_eta(px, pb, c, P, Pp, kq);
                    if (live) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            fine[r] = fine[r] && gb_finite(acc[r]);
                            m[r] = fmax(m[r], acc[r]);
                            ey[r] = c == yv ? acc[r] : ey[r];
                        }
                    }
                }
                double z[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
                for (int c = 0; c < Cm; ++c) {                  // sweep 2: the same chain, the sum in class order
                    const v4d acc = pls_eta(px, pb, c, P, Pp, kq);
                    if (live) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) z[r] += exp(acc[r] - m[r]);
                    }
                }
                if (live) {
                    const bool yok = yv >= 0 && yv <= Cm;       // (yv = C - 1: the reference class, eta_y = 0)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int s = t0 + 16 * wv + kq + 4 * r;    // the draw; cc is the observation
                        if (s < S) ell[cc * S + s] = yok && fine[r] ? ey[r] - m[r] - log(z[r] + exp(0.0 - m[r])) : qnan;
                    }
                }
            }
        }
    }
    __syncthreads();                          // l_si is published; the tiles are dead, the stage may take their place

    // ---- (2) per observation: the PSIS stage on rho, then the two log-sum-exps (the twin of k_psis_loo_batched's) -------------
    for (int i = 0; i < ni; ++i) {
        const size_t ki = kn + i;
        double* lk = a.loglik ? a.loglik + ki * S : nullptr;
        if (i >= nv) {                        // not a valid row (uniform in the workgroup: no barrier is skipped by a part of it)
            if (lk)
                for (int s = l; s < S; s += 256) lk[s] = qnan;
            if (l == 0) {
                a.elpd[ki] = qnan;
                a.lpd[ki] = qnan;
                a.khat[ki] = qnan;
                a.ess[ki] = qnan;
                a.info[ki] = -3;
            }
            continue;
        }
        const double* el = ell + i * S;
        for (int s = l; s < S; s += 256) {
            const double e = el[s];
            sm.val[s] = a.logr[ks + s] - e;
            if (lk) lk[s] = e;
        }
        __syncthreads();
        const ps_verdict v = ps_stage(sm, S, S2, M, l, false);
        double m1 = -inf, m2 = -inf;
        for (int s = l; s < S; s += 256) {
            const double e = el[s];
            m1 = fmax(m1, sm.lwu[s] + e);
            m2 = fmax(m2, a.lw[ks + s] + e);
        }
        m1 = ps_max(m1, sm.red, l);
        m2 = ps_max(m2, sm.red, l);
        double s1 = 0.0, s2 = 0.0;
        for (int s = l; s < S; s += 256) {
            const double e = el[s];
            s1 += exp((sm.lwu[s] + e) - m1);
            s2 += exp((a.lw[ks + s] + e) - m2);
        }
        s1 = ps_sum(s1, sm.red, l);
        s2 = ps_sum(s2, sm.red, l);
        if (l == 0) {
            a.elpd[ki] = v.bad ? qnan : m1 + log(s1);
            a.lpd[ki] = v.bad ? qnan : m2 + log(s2);
            a.khat[ki] = v.bad ? qnan : v.khat;
            a.ess[ki] = v.bad ? qnan : v.ess;
            a.info[ki] = v.bad ? -1 : (v.fit ? 0 : -2);
        }
        __syncthreads();                      // the next observation overwrites the stage's arrays
    }
}

hipError_t gsmvi_psis_loo_softmax_batched_prepare() { return gb_allow_lds(k_psis_loo_softmax_batched); }

extern "C" {

int gsmvi_psis_loo_softmax_tile(int C, int P, int64_t S) {
    if (!pls_shape_ok(C, P) || S < PS_MIN_S || S > PS_MAX_S) return 0;
    return pls_tile(C, P, (int)S);
}

int gsmvi_psis_loo_softmax_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int C, int P, int64_t N, int64_t S,
                                       const double* A, const int* labels, const int* counts_dev, const double* X,
                                       const double* logr, const double* lw, double* loglik, double* elpd, double* lpd,
                                       double* khat, double* ess, int* info) {
    GB_BAD(C < 2, "C must be at least 2");
    GB_BAD(!pls_shape_ok(C, P), "P must be at least 1 and D = (C - 1) P in [1, 64]");
    const int D = (C - 1) * P;
    GB_BAD(K < 1 || K > 16777215, "K must be in [1, 2^24 - 1]");
    GB_BAD(N < 1, "N must be at least 1");
    GB_BAD(S < PS_MIN_S || S > PS_MAX_S, "S must be in [5, 4096]");
    GB_BAD(!A || !labels || !X || !logr || !lw || !elpd || !lpd || !khat || !ess || !info, "NULL array");
    GB_BAD(N > (INT64_MAX / 8 / S) / K, "K N S is too large");
    GB_BAD(N > (INT64_MAX / 8 / P) / K, "K N P is too large");
    const int NI = pls_tile(C, P, (int)S);
    const int64_t ntile = (N + NI - 1) / NI;
    GB_BAD(ntile > 16777215 / K,
           "K ceil(N / gsmvi_psis_loo_softmax_tile(C, P, S)) must be at most 2^24 - 1 (one tile per workgroup)");
    const size_t nn = (size_t)K * N * 8, ns = (size_t)K * S * 8;
    if (int st = gb_check_overlaps(__func__, {{A, nn * P, "A", GB_RD}, {labels, (size_t)K * N * 4, "labels", GB_RD},
                                              {counts_dev, (size_t)K * 4, "counts_dev", GB_RD}, {X, ns * D, "X", GB_RD},
                                              {logr, ns, "logr", GB_RD}, {lw, ns, "lw", GB_RD},
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
    a.U = pls_region_doubles(C, P, a.S, a.S2);
    a.ntile = (unsigned)ntile;
    a.A = A; a.labels = labels; a.counts = counts_dev;
    a.X = X; a.logr = logr; a.lw = lw; a.loglik = loglik; a.elpd = elpd; a.lpd = lpd; a.khat = khat; a.ess = ess; a.info = info;
    const size_t lds = ((size_t)a.U + (size_t)NI * a.S) * sizeof(double);      // <= GB_LDS_MAX by the choice of NI
    const unsigned grid = (unsigned)(K * ntile);
    hipLaunchKernelGGL(k_psis_loo_softmax_batched, dim3(grid), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_SOFTMAX, "k_psis_loo_softmax_batched");
}

}  // extern "C"
