// Batched ADVI: K independent full-rank ADVI fits of the same (D, B), D <= 64, B <= 32, one launch per iteration after the
// score ("Batched ADVI").
//
// The reference's baseline (gsmvi/advi.py) maximises the ELBO of q = N(loc, L L^T), L lower triangular, over (loc, scales),
// scales = the D (D + 1) / 2 entries of L in np.tril_indices order (p = i (i + 1) / 2 + j, j <= i; advi.py:23-27,80-83), with
// jax.grad of the loss of advi.py:31-45 and an optax optimiser (:69-73).  For the draws x_b = loc + L z_b and the scores
// g_b = grad lp(x_b) that gradient is closed form,
//   d / d loc  = -sum_b g_b,      d / d L_ij = -sum_b g_bi z_bj  (j <= i),  and -B / L_ii more on the diagonal
// (the loss holds +sum_b log q(x_b), whose -B sum_i log|L_ii| gives the diagonal term; |z|^2 does not depend on the
// parameters), so no autograd runs and the user supplies the score, as for the batched GSM and BaM.  Adam is built in:
//   m <- b1 m + (1 - b1) g,  v <- b2 v + (1 - b2) g^2,  p <- p - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// (torch.optim.Adam at its defaults, optax.adam: eps outside the root).
//   k_advi_batched<NT, GA_INIT> : scales_k = packed lower Cholesky factor of cov_k (gb_chol_lds, transposed on the way out),
//                                 info[k]; with seeds (or forced normals) the first samples and their logq_sum
//   k_advi_batched<NT, GA_STEP> : the gradient, Adam on loc and scales in place (moments in place), then the next samples
//                                 X_k = loc_k + Z_k L_k^T and logq_sum[k] = sum_b (-|z_b|^2 / 2) - B sum_i log|L_ii|
//                                 - B D / 2 log 2 pi of the UPDATED state
//   k_advi_cov_batched<NT>      : cov_k = L_k L_k^T, exactly symmetric (both (i, j) and (j, i) sum the same products in the
//                                 same order)
// Work mapping: the slots of gsmvi_batched.h (gb_nt(D) threads per problem, four problems per 256-thread workgroup for
// D <= 16).  There is no factorisation in a step: the state IS the Cholesky factor.  Per problem a step reads and writes
// three packed triangles and three vectors once; thread l owns the packed entries p = l, l + NT, ... (contiguous across the
// slot), all of them loaded before the first barrier.  G, the z behind it (regenerated from the problem's Philox stream: draw
// call - 1, the fits' layout of B x gb_dz(D) normals) and the new L live in LDS.  A non-finite score is not caught: it makes
// that problem's state NaN from then on, as in the reference.  A slot reads and writes only slice k of every array and every
// slot runs the same barriers, so nothing crosses between problems.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "../../include/gsmvi_hip.h"
#include "../../include/gsmvi_hip_debug.h"   // gsmvi_debug_advi_batched_lds
#include <cmath>
#include <cstdint>

enum { GA_INIT = 0, GA_STEP = 1, GA_COV = 2 };

struct ga_args {
    long long K;
    int D, B;
    const double* G;        // STEP: (K, B, D) scores of the current samples
    const double* mean;     // INIT: (K, D)
    const double* cov;      // INIT: (K, D, D)
    double* loc;            // STEP: (K, D) in / out
    double* scales;         // STEP: (K, P) in / out; INIT: out
    double* m_loc;          // STEP: Adam's moments, in / out
    double* v_loc;
    double* m_s;
    double* v_s;
    double lr;              // the step size of every problem ...
    const double* lr_dev;   // ... or (K) per-problem values on the device (null: `lr`)
    double b1, b2, eps;
    double bc1, bc2s;       // 1 - b1^t, sqrt(1 - b2^t)
    const unsigned long long* seeds;   // (K) the problems' draw keys (null: the normals are given)
    unsigned long long call;           // draw number of the samples written (STEP: the z behind G is draw call - 1)
    const double* Zcur;     // STEP without seeds: (K, B, D) the z behind G
    const double* Znext;    // without seeds: (K, B, D) the z of the samples written
    double* Xout;           // (K, B, D) samples of the new state (null: none)
    double* logq;           // (K) sum_b log q(x_b) of those samples
    int* info;              // INIT: (K) 0, or 1 + the first bad pivot
};

__host__ __device__ inline int ga_tri(int D) { return D * (D + 1) / 2; }
// LDS doubles per problem.  STEP: G (B x D) + z (B x Dz) + the new L (packed) + the new loc (D) + 4 partial sums.
// INIT: cov / its factor (D x D) + z (B x Dz) + mean, pivots (D each) + 4 partial sums.  (64, 32): 6244 and 6276 doubles, 49 KB.
__host__ __device__ inline int ga_lds_doubles(int D, int B, int mode) {
    return mode == GA_COV ? ga_tri(D)
                          : mode == GA_STEP ? B * D + B * gb_dz(D) + ga_tri(D) + D + 4 : D * D + B * gb_dz(D) + 2 * D + 4;
}

// row of packed entry p: the i with i (i + 1) / 2 <= p < (i + 1) (i + 2) / 2  (p <= 2079: the float root is off by one at most)
__device__ __forceinline__ int ga_row(int p) {
    int i = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
    if (i * (i + 1) / 2 > p) --i;
    if ((i + 1) * (i + 2) / 2 <= p) ++i;
    return i;
}

// The z of draw `call` of the slot's problem into Zb (B x Dz), or the given normals Zg (B x D); returns this thread's share of
// sum |z|^2 over the B x D entries that are used (column D of an odd-D draw is dropped).
template <int NT>
__device__ __forceinline__ double ga_fill_z(const ga_args& a, long long k, int l, unsigned long long call, const double* Zg,
                                            double* Zb) {
    const int D = a.D, B = a.B, Dz = gb_dz(D);
    double acc = 0.0;
    if (a.seeds) {
        const unsigned long long seed = a.seeds[k];
        for (int p = l; p < (B * Dz) / 2; p += NT) {
            unsigned w[4];
            philox4x32_10((unsigned)p, 0u, (unsigned)call, (unsigned)(call >> 32), (unsigned)seed, (unsigned)(seed >> 32), w);
            double z0, z1;
            philox_normal_pair(w, z0, z1);
            Zb[2 * p] = z0;
            Zb[2 * p + 1] = z1;
            acc += z0 * z0;                                             // (2 p is never column D: Dz is even)
            if ((2 * p + 1) % Dz < D) acc += z1 * z1;
        }
    } else {
        const double* Zk = Zg + (size_t)k * B * D;
        for (int e = l; e < B * D; e += NT) {
            const int b = e / D, j = e - b * D;
            const double z = Zk[e];
            Zb[b * Dz + j] = z;
            acc += z * z;
        }
    }
    return acc;
}

// The samples of the slot's problem and their log q: X = loc + Z L^T with L given by at(i, j) (j <= i), products first, then
// the mean (gb_fit_tail's order); logq[k] = -acc / 2 - B sum_i log|L_ii| - B D / 2 log 2 pi with acc = the slot's sum of |z|^2
// (summed over the slot by gb_slot_sum of gsmvi_batched.h).  Every thread of the slot calls it (barrier inside for NT > 64).
template <int NT, typename At>
__device__ __forceinline__ void ga_sample(const ga_args& a, bool valid, long long k, int l, double acc, const double* Zb,
                                          const double* loc, double* red, At at) {
    const int D = a.D, B = a.B, Dz = gb_dz(D), BD = B * D;
    if (valid) {
        double* Xk = a.Xout + (size_t)k * BD;
        for (int e = l; e < BD; e += NT) {
            const int b = e / D, i = e - b * D;
            double s = 0.0;
            for (int j = 0; j <= i; ++j) s += Zb[b * Dz + j] * at(i, j);
            Xk[e] = s + loc[i];
        }
    }
    // thread l < D folds -B log|L_ll| into its share, so the D logarithms run side by side and one reduction serves both sums
    double v = -0.5 * acc;
    if (valid && l < D) v -= (double)B * log(fabs(at(l, l)));
    v = gb_slot_sum<NT>(v, l, red);
    if (valid && l == 0) a.logq[k] = v - 0.5 * (double)B * D * 1.8378770664093454836;   // log 2 pi
}

template <int NT, int MODE>
__global__ __launch_bounds__(256) void k_advi_batched(ga_args a) {
    extern __shared__ double ga_sm[];
    constexpr int PPW = 256 / NT;
    constexpr int MAXE = NT == 256 ? (GB_MAX_D * GB_MAX_D) / 256 : (16 * 16) / 64;   // matrix entries per thread (INIT)
    constexpr int MAXP = NT == 256 ? (GB_MAX_D * (GB_MAX_D + 1) / 2 + 255) / 256 : (16 * 17 / 2 + 63) / 64;   // packed entries
    const int D = a.D, B = a.B, Dz = gb_dz(D), P = ga_tri(D), BD = B * D;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;               // a tail slot runs every barrier and nothing else
    double* sm = ga_sm + (size_t)slot * ga_lds_doubles(D, B, MODE);
    const size_t kd = (size_t)(valid ? k : 0) * D, kp = (size_t)(valid ? k : 0) * P, kbd = (size_t)(valid ? k : 0) * BD;

    if (MODE == GA_INIT) {
        double* S = sm;                       // D x D  cov, then its upper factor R = L^T
        double* Zb = S + D * D;               // B x Dz
        double* m = Zb + B * Dz;              // D
        double* pv = m + D;                   // D      pivots
        double* red = pv + D;                 // 4
        if (valid) {
            for (int i = l; i < D; i += NT) m[i] = a.mean[kd + i];
            for (int e = l; e < D * D; e += NT) S[e] = a.cov[(size_t)k * D * D + e];
        }
        __syncthreads();
        const int info = gb_chol_lds<NT, MAXE>(valid, D, l, D, S, pv);
        __syncthreads();
        if (valid) {
            for (int p = l; p < P; p += NT) {
                const int i = ga_row(p), j = p - i * (i + 1) / 2;
                a.scales[kp + p] = S[j * D + i];
            }
            if (l == 0) a.info[k] = info;
        }
        if (!a.Xout) return;                                            // (uniform: no barrier follows)
        const double acc = valid ? ga_fill_z<NT>(a, k, l, 0ull, a.Znext, Zb) : 0.0;
        __syncthreads();
        ga_sample<NT>(a, valid, k, l, acc, Zb, m, red, [&](int i, int j) { return S[j * D + i]; });
        return;
    }

    double* Gm = sm;                          // B x D   the scores
    double* Zb = Gm + BD;                     // B x Dz  the z behind them; later the next z
    double* Ln = Zb + B * Dz;                 // P       the new L, packed
    double* ln = Ln + P;                      // D       the new loc
    double* red = ln + D;                     // 4

    // every global load of the step is issued before the first barrier
    double s[MAXP], ms[MAXP], vs[MAXP];
    double lc = 0.0, ml = 0.0, vl = 0.0, lr = a.lr;
    if (valid) {
#pragma unroll
        for (int q = 0; q < MAXP; ++q) {
            const int p = l + q * NT;
            if (p < P) {
                s[q] = a.scales[kp + p];
                ms[q] = a.m_s[kp + p];
                vs[q] = a.v_s[kp + p];
            }
        }
        if (l < D) {
            lc = a.loc[kd + l];
            ml = a.m_loc[kd + l];
            vl = a.v_loc[kd + l];
        }
        if (a.lr_dev) lr = a.lr_dev[k];
        for (int e = l; e < BD; e += NT) Gm[e] = a.G[kbd + e];
        ga_fill_z<NT>(a, k, l, a.call - 1, a.Zcur, Zb);
    }
    __syncthreads();

    const double step = lr / a.bc1, omb1 = 1.0 - a.b1, omb2 = 1.0 - a.b2;
    if (valid) {
#pragma unroll
        for (int q = 0; q < MAXP; ++q) {                                // d loss / d L_ij, Adam   (advi.py:31-45,69-73)
            const int p = l + q * NT;
            if (p < P) {
                const int i = ga_row(p), j = p - i * (i + 1) / 2;
                double acc = 0.0;
                for (int b = 0; b < B; ++b) acc += Gm[b * D + i] * Zb[b * Dz + j];
                double g = -acc;
                if (i == j) g -= (double)B / s[q];
                const double mn = a.b1 * ms[q] + omb1 * g;
                const double vn = a.b2 * vs[q] + omb2 * (g * g);
                const double sn = s[q] - step * (mn / (sqrt(vn) / a.bc2s + a.eps));
                a.m_s[kp + p] = mn;
                a.v_s[kp + p] = vn;
                a.scales[kp + p] = sn;
                Ln[p] = sn;
            }
        }
        if (l < D) {                                                    // d loss / d loc = -sum_b g_b
            double acc = 0.0;
            for (int b = 0; b < B; ++b) acc += Gm[b * D + l];
            const double g = -acc;
            const double mn = a.b1 * ml + omb1 * g;
            const double vn = a.b2 * vl + omb2 * (g * g);
            const double cn = lc - step * (mn / (sqrt(vn) / a.bc2s + a.eps));
            a.m_loc[kd + l] = mn;
            a.v_loc[kd + l] = vn;
            a.loc[kd + l] = cn;
            ln[l] = cn;
        }
    }
    if (!a.Xout) return;                                                // (uniform: no barrier follows)
    __syncthreads();                                                    // the z behind G is no longer read
    const double acc = valid ? ga_fill_z<NT>(a, k, l, a.call, a.Znext, Zb) : 0.0;
    __syncthreads();
    ga_sample<NT>(a, valid, k, l, acc, Zb, ln, red, [&](int i, int j) { return Ln[i * (i + 1) / 2 + j]; });
}

// cov_k = L_k L_k^T: entry (i, j) sums L_ic L_jc over c = 0 .. min(i, j) in that order, so (j, i) gets the same bits
template <int NT>
__global__ __launch_bounds__(256) void k_advi_cov_batched(long long K, int D, const double* __restrict__ scales,
                                                          double* __restrict__ cov) {
    extern __shared__ double ga_sm[];
    constexpr int PPW = 256 / NT;
    const int P = ga_tri(D), DD = D * D;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < K;
    double* L = ga_sm + (size_t)slot * P;
    if (valid)
        for (int p = l; p < P; p += NT) L[p] = scales[(size_t)k * P + p];
    __syncthreads();
    if (!valid) return;
    for (int e = l; e < DD; e += NT) {
        const int i = e / D, j = e - i * D, n = i < j ? i : j;
        const double* Li = L + i * (i + 1) / 2;
        const double* Lj = L + j * (j + 1) / 2;
        double acc = 0.0;
        for (int c = 0; c <= n; ++c) acc += Li[c] * Lj[c];
        cov[(size_t)k * DD + e] = acc;
    }
}

// dynamic LDS bytes of a launch at (D, B): at most 49 KB, below the default limit, so no kernel attribute is needed
static size_t ga_launch_lds(int D, int B, int mode, int* ppw) {
    *ppw = 256 / gb_nt(D);
    return (size_t)*ppw * ga_lds_doubles(D, B, mode) * sizeof(double);
}

static int ga_launch(gsmvi_ctx* ctx, void* stream, int mode, const ga_args& a, const char* fn) {
    int ppw;
    const size_t lds = ga_launch_lds(a.D, a.B, mode, &ppw);
    const unsigned grid = (unsigned)((a.K + ppw - 1) / ppw);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define GA_GO(NTV, M) hipLaunchKernelGGL((k_advi_batched<NTV, M>), dim3(grid), dim3(256), lds, st, a)
    if (ppw == 4) {
        if (mode == GA_INIT) GA_GO(64, GA_INIT); else GA_GO(64, GA_STEP);
    } else {
        if (mode == GA_INIT) GA_GO(256, GA_INIT); else GA_GO(256, GA_STEP);
    }
#undef GA_GO
    return gb_launched(ctx, GSMVI_PATH_BATCHED_ADVI, fn);
}

extern "C" {

int gsmvi_advi_init_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* mean, const double* cov,
                                double* scales, int* info_dev, const uint64_t* seeds_dev, const double* Z, double* X,
                                double* logq_sum) {
    if (int st = gb_check_shape(__func__, K, D, gb_ppw, B)) return st;
    GB_BAD(!mean || !cov || !scales || !info_dev, "NULL array");
    GB_BAD(seeds_dev && Z, "give seeds_dev or Z, not both");
    GB_BAD((seeds_dev || Z) && (!X || !logq_sum), "samples asked for without X and logq_sum");
    GB_BAD(!seeds_dev && !Z && (X || logq_sum), "X or logq_sum given without seeds_dev or Z");
    const size_t nv = (size_t)K * D * 8, nm = (size_t)K * D * D * 8, nx = (size_t)K * B * D * 8, nk = (size_t)K * 8,
                 ni = (size_t)K * 4, np = (size_t)K * ga_tri(D) * 8;
    if (int st = gb_check_overlaps(__func__, {{mean, nv, "mean", GB_RD}, {cov, nm, "cov", GB_RD}, {scales, np, "scales", GB_WR},
                                              {info_dev, ni, "info_dev", GB_WR}, {seeds_dev, nk, "seeds_dev", GB_RD},
                                              {Z, nx, "Z", GB_RD}, {X, nx, "X", GB_WR}, {logq_sum, nk, "logq_sum", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    ga_args a = {};
    a.K = K; a.D = D; a.B = B; a.mean = mean; a.cov = cov; a.scales = scales; a.info = info_dev;
    a.seeds = reinterpret_cast<const unsigned long long*>(seeds_dev); a.Znext = Z; a.Xout = X; a.logq = logq_sum;
    return ga_launch(ctx, stream, GA_INIT, a, "k_advi_batched (init)");
}

int gsmvi_advi_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* G, double* loc,
                                double* scales, double* m_loc, double* v_loc, double* m_s, double* v_s, int64_t t, double lr,
                                const double* lr_dev, double b1, double b2, double eps, const uint64_t* seeds_dev, uint64_t call,
                                const double* Zcur, const double* Znext, double* Xout, double* logq_sum) {
    if (int st = gb_check_shape(__func__, K, D, gb_ppw, B)) return st;
    GB_BAD(!G || !loc || !scales || !m_loc || !v_loc || !m_s || !v_s, "NULL array");
    GB_BAD(t < 1, "t must be at least 1 (iteration + 1)");
    GB_BAD(!(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0), "b1 and b2 must be in [0, 1)");
    GB_BAD(seeds_dev && (Zcur || Znext), "give seeds_dev or Zcur / Znext, not both");
    GB_BAD(seeds_dev && call < 1, "call must be at least 1 (the z behind G is draw call - 1)");
    GB_BAD(!seeds_dev && !Zcur, "without seeds_dev the z behind G is needed (Zcur)");
    GB_BAD(Xout && !seeds_dev && !Znext, "without seeds_dev the next samples need Znext");
    GB_BAD(!Xout != !logq_sum, "Xout and logq_sum go together");
    const size_t nv = (size_t)K * D * 8, nx = (size_t)K * B * D * 8, nk = (size_t)K * 8, np = (size_t)K * ga_tri(D) * 8;
    if (int st = gb_check_overlaps(__func__, {{G, nx, "G", GB_RD}, {loc, nv, "loc", GB_WR}, {scales, np, "scales", GB_WR},
                                              {m_loc, nv, "m_loc", GB_WR}, {v_loc, nv, "v_loc", GB_WR}, {m_s, np, "m_s", GB_WR},
                                              {v_s, np, "v_s", GB_WR}, {lr_dev, nk, "lr_dev", GB_RD},
                                              {seeds_dev, nk, "seeds_dev", GB_RD}, {Zcur, nx, "Zcur", GB_RD},
                                              {Znext, nx, "Znext", GB_RD}, {Xout, nx, "Xout", GB_WR},
                                              {logq_sum, nk, "logq_sum", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    ga_args a = {};
    a.K = K; a.D = D; a.B = B; a.G = G; a.loc = loc; a.scales = scales; a.m_loc = m_loc; a.v_loc = v_loc; a.m_s = m_s; a.v_s = v_s;
    a.lr = lr; a.lr_dev = lr_dev; a.b1 = b1; a.b2 = b2; a.eps = eps;
    a.bc1 = 1.0 - std::pow(b1, (double)t);
    a.bc2s = std::sqrt(1.0 - std::pow(b2, (double)t));
    a.seeds = reinterpret_cast<const unsigned long long*>(seeds_dev); a.call = call; a.Zcur = Zcur; a.Znext = Znext;
    a.Xout = Xout; a.logq = logq_sum;
    return ga_launch(ctx, stream, GA_STEP, a, "k_advi_batched (step)");
}

int gsmvi_advi_cov_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, const double* scales, double* cov) {
    if (int st = gb_check_shape(__func__, K, D, gb_ppw)) return st;
    GB_BAD(!scales || !cov, "NULL array");
    if (int st = gb_check_overlaps(__func__, {{scales, (size_t)K * ga_tri(D) * 8, "scales", GB_RD},
                                              {cov, (size_t)K * D * D * 8, "cov", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    int ppw;
    const size_t lds = ga_launch_lds(D, 1, GA_COV, &ppw);
    const unsigned grid = (unsigned)((K + ppw - 1) / ppw);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (ppw == 4)
        hipLaunchKernelGGL(k_advi_cov_batched<64>, dim3(grid), dim3(256), lds, st, (long long)K, D, scales, cov);
    else
        hipLaunchKernelGGL(k_advi_cov_batched<256>, dim3(grid), dim3(256), lds, st, (long long)K, D, scales, cov);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_ADVI, "k_advi_cov_batched");
}

// include/gsmvi_hip_debug.h: what a launch at (D, B) requests (exported by the debug library only); mode 0 = init, 1 = step,
// 2 = cov (B plays no part)
int gsmvi_debug_advi_batched_lds(int D, int B, int mode, size_t* bytes, int* problems_per_workgroup) {
    GB_BAD(D < 1 || D > GB_MAX_D || B < 1 || B > GB_MAX_B || mode < 0 || mode > 2 || !bytes || !problems_per_workgroup,
           "bad shape, mode or NULL output");
    *bytes = ga_launch_lds(D, B, mode, problems_per_workgroup);
    return GSMVI_OK;
}

}  // extern "C"
