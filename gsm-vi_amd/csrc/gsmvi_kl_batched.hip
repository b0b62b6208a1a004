// Batched KL monitor: the Gaussian q_k = N(mean_k, cov_k) of K problems of one D, D <= 64, in one launch.
//
// The reference's monitor (gsmvi/monitors.py:83-125) draws batch_size_kl samples of q, evaluates MultivariateNormal.log_prob
// on them (:104-113) and, with reference samples, on those too.  DeviceKLMonitor does that on the GPU for ONE problem: a
// Cholesky launch, a draw, a sample, a whitening launch.  Here every problem of a batched fit in one launch:
//   k_kl_batched<NT, KB_DRAW> : R_k = chol(cov_k) (upper) in LDS; for the rows s = s0 .. s0 + nc - 1 of draw `call`:
//                               z = the rows of gsmvi_randn_f64(seed_k, call, n D) (element s D + j, pair (s D + j) / 2 --
//                               the plain layout, no odd-D padding), x = mean_k + z R_k -> X (K x nc x D), and
//                               logq_sum[k] = sum over the rows of (-|z|^2 / 2 - sum_i log R_ii - D / 2 log 2 pi)
//   k_kl_batched<NT, KB_EVAL> : R_k as above; for the rows y of Y (K x nc x D): w = the solution of R_k^T w = y - mean_k
//                               (forward substitution), logq_sum[k] = the same sum with w in place of z
// Work mapping: the problem of one workgroup slot (gb_nt(D) threads: four problems per 256-thread workgroup for D <= 16) lives
// in LDS: R (D x ld), the mean, the pivots, and a tile of rows (TR x ldy) that the launch walks through, so nc is unbounded
// and the LDS is not.  The row strides are odd (D | 1): the substitution's lanes walk down a column of the tile, and each meets
// a different LDS bank.  The Cholesky is gb_chol_lds (gsmvi_batched.h), the one the batched fit steps test with; the slot sum
// and the log-density sum are gb_slot_sum and gb_logq_sum of gsmvi_batched.h, shared with k_pf_propose.  A draw
// element depends only on (seed, call, element index), and x_sj sums its products in a fixed order, so a call split into
// chunks (s0 > 0) writes the same x bit for bit as the unsplit call.  A pivot that is not > 0 and finite: info[k] = 1 + that
// pivot, logq_sum[k] = NaN and problem k's rows of X are NaN.  A slot reads and writes only its own problem's slices, and
// every slot runs the same barriers (D + 1 per tile in EVAL, 2 per tile in DRAW), so nothing crosses between problems.
// mean and cov are only read: no context workspace, safe between two steps of a running batched fit.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "../../include/gsmvi_hip.h"
#include <cstdint>

enum { KB_DRAW = 0, KB_EVAL = 1 };
#define KB_Q 4     // tile elements per thread: TR = max(1, NT KB_Q / D) rows

struct kb_args {
    long long K, nc, s0;
    int D, ld, ldy, tr;                 // dimension, row strides of R and of the tile, rows per tile
    const double* mean;                 // (K, D)
    const double* cov;                  // (K, D, D)
    const unsigned long long* seeds;    // DRAW: (K) the problems' stream keys
    unsigned long long call;            // DRAW: draw number
    const double* Y;                    // EVAL: (K, nc, D) rows to evaluate
    double* X;                          // DRAW: (K, nc, D) samples
    double* logq;                       // (K) sum over the rows of log q_k
    int* info;                          // (K) 0, or 1 + the first bad pivot
};

__host__ __device__ inline int kb_tile_rows(int D, int NT) { return (NT * KB_Q) / D > 1 ? (NT * KB_Q) / D : 1; }
// LDS doubles per problem: R (D x ld) + mean, pivots (D each) + the row tile (tr x ldy) + 4 partial sums (one per wave)
__host__ __device__ inline int kb_lds_doubles(int D, int ld, int ldy, int tr) { return D * ld + 2 * D + tr * ldy + 4; }

template <int NT, int MODE>
__global__ __launch_bounds__(256) void k_kl_batched(kb_args a) {
    extern __shared__ double kb_sm[];
    constexpr int PPW = 256 / NT;
    constexpr int MAXE = NT == 256 ? (GB_MAX_D * GB_MAX_D) / 256 : (16 * 16) / 64;   // matrix entries per thread
    const int D = a.D, ld = a.ld, ldy = a.ldy, TR = a.tr, DD = D * D;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;               // a tail slot runs every barrier and nothing else
    double* R = kb_sm + (size_t)slot * kb_lds_doubles(D, ld, ldy, TR);
    double* m = R + D * ld;                   // D      mean
    double* pv = m + D;                       // D      pivots R_cc
    double* T = pv + D;                       // TR x ldy  z (DRAW) or y - mean, then w (EVAL)
    double* red = T + TR * ldy;               // 4      per-wave partial sums
    const size_t kd = (size_t)(valid ? k : 0) * D, kdd = (size_t)(valid ? k : 0) * DD;
    const size_t krow = (size_t)(valid ? k : 0) * (size_t)a.nc * D;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    if (valid) {
        for (int i = l; i < D; i += NT) m[i] = a.mean[kd + i];
        for (int e = l; e < DD; e += NT) {
            const int i = e / D, j = e - i * D;
            R[i * ld + j] = a.cov[kdd + e];
        }
    }
    __syncthreads();
    const int info = gb_chol_lds<NT, MAXE>(valid, D, l, ld, R, pv);
    __syncthreads();
    const bool ok = valid && info == 0;

    double acc = 0.0;                         // this thread's share of sum |z|^2 (DRAW) or sum |w|^2 (EVAL)
    for (long long t0 = 0; t0 < a.nc; t0 += TR) {
        const int tr = (int)(a.nc - t0 < TR ? a.nc - t0 : TR), te = tr * D;
        if (MODE == KB_DRAW) {
            if (valid) {                      // the tile's elements n0 .. n0 + te - 1 of the stream: pairs n0 / 2 .. (n0 + te - 1) / 2
                const unsigned long long seed = a.seeds[k], call = a.call;
                const long long n0 = (a.s0 + t0) * D, p0 = n0 >> 1, p1 = (n0 + te - 1) >> 1;
                for (long long p = p0 + l; p <= p1; p += NT) {
                    unsigned w[4];
                    philox4x32_10((unsigned)p, (unsigned)((unsigned long long)p >> 32), (unsigned)call, (unsigned)(call >> 32),
                                  (unsigned)seed, (unsigned)(seed >> 32), w);
                    double z0, z1;
                    philox_normal_pair(w, z0, z1);
                    const long long e0 = 2 * p - n0;
                    if (e0 >= 0) {
                        const int r = (int)e0 / D;
                        T[r * ldy + ((int)e0 - r * D)] = z0;
                        acc += z0 * z0;
                    }
                    if (e0 + 1 < te) {
                        const int r = (int)(e0 + 1) / D;
                        T[r * ldy + ((int)(e0 + 1) - r * D)] = z1;
                        acc += z1 * z1;
                    }
                }
            }
            __syncthreads();
            if (valid) {                      // x = mean + z R   (gb_fit_tail's order: the products, then the mean)
                for (int e = l; e < te; e += NT) {
                    const int r = e / D, j = e - r * D;
                    double s = 0.0;
                    for (int i = 0; i <= j; ++i) s += T[r * ldy + i] * R[i * ld + j];
                    a.X[krow + (size_t)(t0 + r) * D + j] = ok ? s + m[j] : qnan;
                }
            }
            __syncthreads();                  // the next tile overwrites T
        } else {
            if (valid) {
                for (int e = l; e < te; e += NT) {
                    const int r = e / D, j = e - r * D;
                    T[r * ldy + j] = a.Y[krow + (size_t)(t0 + r) * D + j] - m[j];
                }
            }
            __syncthreads();
            // R^T w = y - mean by rows, right-looking: after step c, T[r][c] R_cc^-1 = w_rc and every later column has lost
            // w_rc R_cj -- one pivot per barrier, as the Cholesky
            for (int c = 0; c < D; ++c) {
                if (valid) {
                    const double inv = 1.0 / pv[c];
                    for (int e = l; e < te; e += NT) {
                        const int r = e / D, j = e - r * D;
                        if (j > c) T[r * ldy + j] -= (T[r * ldy + c] * inv) * R[c * ld + j];
                    }
                }
                __syncthreads();
            }
            if (valid) {
                for (int e = l; e < te; e += NT) {
                    const int r = e / D, j = e - r * D;
                    const double w = T[r * ldy + j] * (1.0 / pv[j]);
                    acc += w * w;
                }
            }
            __syncthreads();                  // the next tile overwrites T
        }
    }

    acc = gb_slot_sum<NT>(acc, l, red);
    if (valid && l == 0) {
        a.logq[k] = gb_logq_sum(ok, acc, a.nc, D, pv);
        a.info[k] = info;
    }
}

static int kb_launch(gsmvi_ctx* ctx, void* stream, int mode, kb_args& a, const char* fn) {
    const int nt = gb_nt(a.D), ppw = 256 / nt;
    a.ld = a.D | 1;
    a.ldy = a.D | 1;
    a.tr = kb_tile_rows(a.D, nt);
    const unsigned grid = (unsigned)((a.K + ppw - 1) / ppw);
    const size_t lds = (size_t)ppw * kb_lds_doubles(a.D, a.ld, a.ldy, a.tr) * sizeof(double);   // <= 43 KB (D = 64)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define KB_GO(NTV, M) hipLaunchKernelGGL((k_kl_batched<NTV, M>), dim3(grid), dim3(256), lds, st, a)
    if (nt == 64) {
        if (mode == KB_DRAW) KB_GO(64, KB_DRAW); else KB_GO(64, KB_EVAL);
    } else {
        if (mode == KB_DRAW) KB_GO(256, KB_DRAW); else KB_GO(256, KB_EVAL);
    }
#undef KB_GO
    return gb_launched(ctx, GSMVI_PATH_BATCHED_KL, fn);
}

extern "C" {

int gsmvi_kl_draw_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t nc, int64_t s0, const double* mean,
                              const double* cov, const uint64_t* seeds, uint64_t call, double* X, double* logq_sum, int* info) {
    if (int st = gb_check_shape(__func__, K, D, gb_ppw)) return st;
    GB_BAD(nc < 1, "nc must be at least 1");
    GB_BAD(nc > (INT64_MAX / 8 / D) / K, "K nc D is too large");
    GB_BAD(s0 < 0 || s0 > (INT64_MAX / 2 - nc) / D, "s0 must be >= 0 and (s0 + nc) D below 2^62");
    GB_BAD(!mean || !cov || !seeds || !X || !logq_sum || !info, "NULL array");
    const size_t nv = (size_t)K * D * 8, nm = (size_t)K * D * D * 8, nx = (size_t)K * nc * D * 8, nk = (size_t)K * 8,
                 ni = (size_t)K * 4;
    if (int st = gb_check_overlaps(__func__, {{mean, nv, "mean", GB_RD}, {cov, nm, "cov", GB_RD}, {seeds, nk, "seeds", GB_RD},
                                              {X, nx, "X", GB_WR}, {logq_sum, nk, "logq_sum", GB_WR}, {info, ni, "info", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    kb_args a = {};
    a.K = K; a.D = D; a.nc = nc; a.s0 = s0; a.mean = mean; a.cov = cov;
    a.seeds = reinterpret_cast<const unsigned long long*>(seeds); a.call = call; a.X = X; a.logq = logq_sum; a.info = info;
    return kb_launch(ctx, stream, KB_DRAW, a, "k_kl_batched (draw)");
}

int gsmvi_logq_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t nc, const double* mean, const double* cov,
                           const double* Y, double* logq_sum, int* info) {
    if (int st = gb_check_shape(__func__, K, D, gb_ppw)) return st;
    GB_BAD(nc < 1, "nc must be at least 1");
    GB_BAD(nc > (INT64_MAX / 8 / D) / K, "K nc D is too large");
    GB_BAD(!mean || !cov || !Y || !logq_sum || !info, "NULL array");
    const size_t nv = (size_t)K * D * 8, nm = (size_t)K * D * D * 8, ny = (size_t)K * nc * D * 8, nk = (size_t)K * 8,
                 ni = (size_t)K * 4;
    if (int st = gb_check_overlaps(__func__, {{mean, nv, "mean", GB_RD}, {cov, nm, "cov", GB_RD}, {Y, ny, "Y", GB_RD},
                                              {logq_sum, nk, "logq_sum", GB_WR}, {info, ni, "info", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    kb_args a = {};
    a.K = K; a.D = D; a.nc = nc; a.mean = mean; a.cov = cov; a.Y = Y; a.logq = logq_sum; a.info = info;
    return kb_launch(ctx, stream, KB_EVAL, a, "k_kl_batched (eval)");
}

}  // extern "C"
