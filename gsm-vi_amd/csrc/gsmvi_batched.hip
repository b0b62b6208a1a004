// Batched GSM: K independent problems of the same (D, B), D <= 64, B <= 32, each in one launch.
//
// The reference's update is a pure function of (samples, vs, mu0, S0) (gsmvi/gsm_numpy.py:27-55, gsmvi/gsm.py:31-58), so
// its users batch small problems with jax.vmap.  At D <= 64 one problem is a few microseconds of work for ONE workgroup: the
// single-problem entry points leave almost the whole chip idle and are bound by launch overhead.  Here a problem lives in
// the LDS of one workgroup slot from its first read to its last write:
//   k_gsm_batched<NT, GB_UPDATE> : (mu_k, S_k) = gsm_update(X_k, V_k, mu0_k, S0_k)          (gsm_numpy.py:4-55)
//   k_gsm_batched<NT, GB_STEP>   : the same update, the Cholesky test of S'_k (_check_goodness, gsm_numpy.py:121-146),
//                                  accept or revert of (mean, cov, factor) PER PROBLEM, and the next samples
//                                  X = mean + Z R from the problem's own Philox stream (gsmvi_philox.h)
//   k_gsm_batched<NT, GB_INIT>   : the Cholesky factor of the initial covariance and the first samples
// Work mapping: a 256-thread workgroup holds 256 / NT problems, NT threads each (NT = 64, one wave per problem, for D <= 16;
// NT = 256 above).  The algebra is the O(B D^2) form of the single-problem kernels: S0 g_b,
// the per-sample scalars, the mean, then S' = S0 + mean_b (d_b d_b^T - e_b e_b^T) entry by entry (exactly symmetric when S0
// is).  Plain fp64 FMA loops: at D <= 64 a problem's products are 2 B D^2 <= 262k flops, and the launch is bound by the D^2
// bytes it moves and the D-step pivot chain, not by the vector rate (DESIGN.md section 9 says what was measured).
// A workgroup reads and writes only its own problems' slices, so nothing -- a revert, a NaN -- crosses between problems.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "../../include/gsmvi_hip.h"
#include <cstdint>

enum { GB_UPDATE = 0, GB_STEP = 1, GB_INIT = 2 };

// LDS doubles per problem: S (D x D) + d (B x D) + g / z (B x Dz) + S0 g / e (B x D) + mu0, mu, pivots (D each) + 2 B scalars
__host__ __device__ inline int gb_lds_doubles(int D, int B) { return D * D + 2 * B * D + B * gb_dz(D) + 3 * D + 2 * B; }

template <int NT, int MODE>
__global__ __launch_bounds__(256) void k_gsm_batched(gb_args a) {
    extern __shared__ double gb_sm[];
    constexpr int PPW = 256 / NT;
    constexpr int MAXE = NT == 256 ? (GB_MAX_D * GB_MAX_D) / 256 : (16 * 16) / 64;   // matrix entries per thread
    const int D = a.D, B = a.B, Dz = gb_dz(D), DD = D * D, BD = B * D;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;               // a tail slot runs every barrier and nothing else
    double* S = gb_sm + (size_t)slot * gb_lds_doubles(D, B);
    double* Dm = S + DD;                      // B x D   d_b = mu0 - x_b
    double* Gm = Dm + BD;                     // B x Dz  g_b; later the draws z_b
    double* Em = Gm + B * Dz;                 // B x D   S0 g_b; later e_b = d_b + dmu_b
    double* m0 = Em + BD;                     // D       mean in
    double* m1 = m0 + D;                      // D       mean out
    double* pv = m1 + D;                      // D       pivots sqrt(a_cc)
    double* sc = pv + D;                      // 2 B     (gSg - mv) / den, 1 + rho
    const size_t kd = (size_t)(valid ? k : 0) * D, kdd = (size_t)(valid ? k : 0) * DD, kbd = (size_t)(valid ? k : 0) * BD;
    const double* mu_in = MODE == GB_UPDATE ? a.mu0 : a.mu;
    const double* S_in = MODE == GB_UPDATE ? a.S0 : a.S;
    double sreg[MAXE];

    if (valid) {
        for (int i = l; i < D; i += NT) m0[i] = mu_in[kd + i];
        for (int e = l; e < DD; e += NT) S[e] = S_in[kdd + e];          // all of S0 (both triangles)
        if (MODE != GB_INIT) {
            for (int e = l; e < BD; e += NT) {
                const int b = e / D, j = e - b * D;
                Gm[b * Dz + j] = a.V[kbd + e];
                Dm[e] = mu_in[kd + j] - a.X[kbd + e];
            }
        }
    }
    __syncthreads();
    if (MODE != GB_INIT) {
        if (valid) {                                                    // S0 g_b   (gsm_numpy.py:7)
            for (int e = l; e < BD; e += NT) {
                const int b = e / D, i = e - b * D;
                double s = 0.0;
                for (int j = 0; j < D; ++j) s += S[i * D + j] * Gm[b * Dz + j];
                Em[e] = s;
            }
        }
        __syncthreads();
        if (valid && l < B) {                                           // gsm_numpy.py:8-10,15
            double gSg = 0.0, mv = 0.0;
            for (int i = 0; i < D; ++i) {
                gSg += Gm[l * Dz + i] * Em[l * D + i];
                mv += Dm[l * D + i] * Gm[l * Dz + i];
            }
            const double rho = 0.5 * sqrt(1.0 + 4.0 * (gSg + mv * mv)) - 0.5;
            sc[2 * l] = (gSg - mv) / (1.0 + rho + mv);
            sc[2 * l + 1] = 1.0 + rho;
        }
        __syncthreads();
        if (valid) {                                                    // dmu_b, e_b, the new mean (gsm_numpy.py:11-18,50)
            for (int i = l; i < D; i += NT) {
                double acc = 0.0;
                for (int b = 0; b < B; ++b) {
                    const double d = Dm[b * D + i];
                    const double dmu = ((Em[b * D + i] - d) - d * sc[2 * b]) / sc[2 * b + 1];
                    Em[b * D + i] = d + dmu;
                    acc += dmu;
                }
                m1[i] = m0[i] + acc / B;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < MAXE; ++q) {                                // S' = S0 + mean_b (d d^T - e e^T)   (gsm_numpy.py:21-23,51-53)
            const int e = l + q * NT;
            if (valid && e < DD) {
                const int i = e / D, j = e - i * D;
                double acc = 0.0;
                for (int b = 0; b < B; ++b) acc += Dm[b * D + i] * Dm[b * D + j] - Em[b * D + i] * Em[b * D + j];
                sreg[q] = S[e] + acc / B;
            }
        }
        if (MODE == GB_UPDATE) {
            if (valid) {
                for (int i = l; i < D; i += NT) a.mu[kd + i] = m1[i];
#pragma unroll
                for (int q = 0; q < MAXE; ++q) {
                    const int e = l + q * NT;
                    if (e < DD) a.S[kdd + e] = sreg[q];
                }
            }
            return;
        }
#pragma unroll
        for (int q = 0; q < MAXE; ++q) {                                // (each thread overwrites only its own entries)
            const int e = l + q * NT;
            if (valid && e < DD) S[e] = sreg[q];
        }
    } else if (valid) {
        for (int i = l; i < D; i += NT) m1[i] = m0[i];
    }
    __syncthreads();

    gb_fit_tail<NT, MAXE, MODE == GB_INIT>(a, valid, k, l, D, S, sreg, pv, Gm, m0, m1);
}

// G_k = -(X_k - 1 m_k^T) P_k: one thread per output entry (consecutive threads = consecutive columns of P_k: coalesced)
__global__ __launch_bounds__(256) void k_gauss_score_batched(long long total, int D, int B, const double* __restrict__ X,
                                                             const double* __restrict__ m, const double* __restrict__ P,
                                                             double* __restrict__ G) {
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= total) return;
    const long long BD = (long long)B * D;
    const long long k = n / BD;
    const int r = (int)(n - k * BD), b = r / D, j = r - b * D;
    const double* x = X + k * BD + (long long)b * D;
    const double* mk = m + k * D;
    const double* pk = P + k * D * (long long)D;
    double acc = 0.0;
    for (int i = 0; i < D; ++i) acc += (x[i] - mk[i]) * pk[(long long)i * D + j];
    G[n] = -acc;
}

hipError_t gsmvi_batched_prepare() {
    return gb_allow_lds(k_gsm_batched<64, GB_UPDATE>, k_gsm_batched<256, GB_UPDATE>, k_gsm_batched<64, GB_STEP>,
                        k_gsm_batched<256, GB_STEP>, k_gsm_batched<64, GB_INIT>, k_gsm_batched<256, GB_INIT>);
}

static int gb_launch(gsmvi_ctx* ctx, void* stream, int mode, const gb_args& a, const char* fn) {
    const int nt = gb_nt(a.D), ppw = 256 / nt;
    const unsigned grid = (unsigned)((a.K + ppw - 1) / ppw);
    const size_t lds = (size_t)ppw * gb_lds_doubles(a.D, a.B) * sizeof(double);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define GB_GO(NTV, M) hipLaunchKernelGGL((k_gsm_batched<NTV, M>), dim3(grid), dim3(256), lds, st, a)
    if (nt == 64) {
        if (mode == GB_UPDATE) GB_GO(64, GB_UPDATE); else if (mode == GB_STEP) GB_GO(64, GB_STEP); else GB_GO(64, GB_INIT);
    } else {
        if (mode == GB_UPDATE) GB_GO(256, GB_UPDATE); else if (mode == GB_STEP) GB_GO(256, GB_STEP); else GB_GO(256, GB_INIT);
    }
#undef GB_GO
    return gb_launched(ctx, GSMVI_PATH_BATCHED, fn);
}

extern "C" {

int gsmvi_gsm_update_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* X, const double* G,
                                 const double* mu0, const double* S0, double* mu, double* S) {
    if (int st = gb_check_shape(__func__, K, D, gb_ppw, B)) return st;
    GB_BAD(!X || !G || !mu0 || !S0 || !mu || !S, "NULL array");
    const size_t nv = (size_t)K * D * 8, nm = (size_t)K * D * D * 8, nx = (size_t)K * B * D * 8;
    if (int st = gb_check_overlaps(__func__, {{X, nx, "X", GB_RD}, {G, nx, "G", GB_RD}, {mu0, nv, "mu0", GB_RD},
                                              {S0, nm, "S0", GB_RD}, {mu, nv, "mu", GB_WR}, {S, nm, "S", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    gb_args a = {};
    a.K = K; a.D = D; a.B = B; a.X = X; a.V = G; a.mu0 = mu0; a.S0 = S0; a.mu = mu; a.S = S;
    return gb_launch(ctx, stream, GB_UPDATE, a, "k_gsm_batched (update)");
}

int gsmvi_gsm_fit_init_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* mean, const double* cov,
                                   double* R, int* info_dev, const uint64_t* seeds_dev, double* X) {
    if (int st = gb_check_shape(__func__, K, D, gb_ppw, B)) return st;
    GB_BAD(!mean || !cov || !R || !info_dev, "NULL array");
    GB_BAD(seeds_dev && !X, "seeds given without X");
    const size_t nv = (size_t)K * D * 8, nm = (size_t)K * D * D * 8, nx = (size_t)K * B * D * 8, nk = (size_t)K * 8,
                 ni = (size_t)K * 4;
    if (int st = gb_check_overlaps(__func__, {{mean, nv, "mean", GB_RD}, {cov, nm, "cov", GB_RD}, {R, nm, "R", GB_WR},
                                              {info_dev, ni, "info_dev", GB_WR}, {seeds_dev, nk, "seeds_dev", GB_RD},
                                              {X, nx, "X", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    gb_args a = {};
    a.K = K; a.D = D; a.B = B; a.mu = const_cast<double*>(mean); a.S = const_cast<double*>(cov); a.R = R; a.info = info_dev;
    a.seeds = reinterpret_cast<const unsigned long long*>(seeds_dev); a.call = 0; a.Xout = X;
    return gb_launch(ctx, stream, GB_INIT, a, "k_gsm_batched (fit init)");
}

int gsmvi_gsm_fit_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, double* X, const double* G, double* mean,
                                   double* cov, double* R, int* info_dev, int* n_reverts_dev, const uint64_t* seeds_dev,
                                   uint64_t call) {
    if (int st = gb_check_shape(__func__, K, D, gb_ppw, B)) return st;
    GB_BAD(!X || !G || !mean || !cov, "NULL array");
    GB_BAD(seeds_dev && !R, "drawing the next samples needs the sampling factor R");
    const size_t nv = (size_t)K * D * 8, nm = (size_t)K * D * D * 8, nx = (size_t)K * B * D * 8, nk = (size_t)K * 8,
                 ni = (size_t)K * 4;
    if (int st = gb_check_overlaps(__func__, {{X, nx, "X", GB_WR}, {G, nx, "G", GB_RD}, {mean, nv, "mean", GB_WR},
                                              {cov, nm, "cov", GB_WR}, {R, nm, "R", GB_WR}, {info_dev, ni, "info_dev", GB_WR},
                                              {n_reverts_dev, ni, "n_reverts_dev", GB_WR}, {seeds_dev, nk, "seeds_dev", GB_RD}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    gb_args a = {};
    a.K = K; a.D = D; a.B = B; a.X = X; a.V = G; a.mu = mean; a.S = cov; a.R = R; a.info = info_dev; a.n_rev = n_reverts_dev;
    a.seeds = reinterpret_cast<const unsigned long long*>(seeds_dev); a.call = call; a.Xout = seeds_dev ? X : nullptr;
    return gb_launch(ctx, stream, GB_STEP, a, "k_gsm_batched (fit step)");
}

int gsmvi_gaussian_score_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* X, const double* m,
                                     const double* P, double* G) {
    if (int st = gb_check_shape(__func__, K, D, gb_ppw, B)) return st;
    GB_BAD(!X || !m || !P || !G, "NULL array");
    const size_t nv = (size_t)K * D * 8, nm = (size_t)K * D * D * 8, nx = (size_t)K * B * D * 8;
    if (int st = gb_check_overlaps(__func__, {{X, nx, "X", GB_RD}, {m, nv, "m", GB_RD}, {P, nm, "P", GB_RD}, {G, nx, "G", GB_WR}}))
        return st;
    const long long total = (long long)K * B * D;
    GB_BAD(total > 0xFFFFFF00ll, "K B D must be below 2^32 - 256 (one thread per score entry)");
    GB_BAD(!ctx, "ctx is NULL");
    hipLaunchKernelGGL(k_gauss_score_batched, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), total, D, B, X, m, P, G);
    return gb_launched(ctx, GSMVI_PATH_BATCHED, "k_gauss_score_batched");
}

}  // extern "C"
