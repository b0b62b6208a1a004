// Batched Pathfinder initialiser, single-path form (Zhang, Carpenter, Gelman, Vehtari 2022): every accepted iterate of the
// batched L-BFGS (gsmvi_lbfgs_batched.hip) defines a Gaussian from the pairs held at that moment, a few draws estimate its ELBO,
// and the best one is kept as the start of a fit ("Batched Pathfinder initialiser").  It fills the role of
// gsmvi/initializers.py:5-17 -- a mean and a covariance to start the fit from -- with a start that is chosen by how well it fits.
// Two launches per L-BFGS round, around the caller's lp of the draws:
//   k_pf_propose<NT> : fresh[k] = (nit of the L-BFGS state != seen[k]), seen[k] <- nit.  A fresh problem: gamma = h0 if h0 > 0,
//                      else s.y / y.y of the newest held pair (1 without a pair); Sigma = H after H_0 = gamma I and, over the held
//                      pairs oldest to newest, H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T -- gl_dense_fill and
//                      gl_dense_rounds of gsmvi_lbfgs_state.h, the statements of k_lbfgs_hess_inv_batched with the base gamma
//                      in place of 1; mu = x - Sigma g;
//                      R = chol(Sigma) (upper, gb_chol_lds); the rows s = 0 .. M - 1 of draw `call` = nit of key seeds[k] (element
//                      s D + j, pair (s D + j) / 2: the plain layout of k_kl_batched), X_k row s = mu + z_s R and
//                      logq[k] = sum_s (-|z_s|^2 / 2 - sum_i log R_ii - D / 2 log 2 pi); mu, cov, info written.  A bad pivot, or
//                      a mean that is not finite (a non-finite gradient): NaN rows and a NaN logq.  A problem that is not fresh
//                      (a rejected trial, a frozen problem): X_k rows <- x_k, so that the lp that follows reads defined memory,
//                      logq[k] <- NaN, and nothing else of the problem is written.
//   k_pf_select<NT>  : e = (lpsum[k] - logq[k]) / M for a fresh problem with info 0; elbo_last[k] = e (NaN when not fresh),
//                      npts[k] += fresh[k]; e finite and e > best_elbo[k] (strict: the first maximum wins) -> best_elbo, best_mean,
//                      best_cov, best_it <- e, mu, Sigma, nit; otherwise nothing of the best state is written.
// Work mapping: the slots of gsmvi_batched.h (gb_nt(D) threads per problem, four problems per 256-thread workgroup for D <= 16).
// The matrix lives in LDS with the odd row stride D | 1 (the product u = H y and the substitution walk down a column: every lane
// another bank); the draws are walked in row tiles of k_kl_batched's shape, so M does not bound the LDS: the draw of a tile and
// x = mu + z R are k_kl_batched's statements, restated here (on shared functions this kernel missed the speed bound at every
// D <= 16: DESIGN.md section 9, "One copy of each initialiser stage"), so a change to one belongs in the other; the
// slot sum and the log-density sum are gb_slot_sum and gb_logq_sum of gsmvi_batched.h.  The state's layout and the clamped read
// of its counters are gsmvi_lbfgs_state.h's.  Every slot runs every barrier (3 + 2 x 10 + D + 1, then 2 per tile, then 1 for
// NT = 256), a slot reads and writes only slice k of every array, and every sum runs in an order fixed by (D, M) alone: a
// problem's bits depend neither on K nor on its neighbours.  No scratch, no context workspace.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_lbfgs_state.h"
#include "../../include/gsmvi_hip.h"
#include "../../include/gsmvi_hip_debug.h"   // gsmvi_debug_pathfinder_batched_lds
#include <cmath>
#include <cstdint>

#define PF_Q 4         // tile elements per thread: TR = max(1, NT PF_Q / D) rows (k_kl_batched's tile)
#define PF_MAX_DRAWS 4096

struct pf_args {
    long long K, M;
    int D, ld, ldy, tr;                 // dimension, row strides of the matrix and of the tile, rows per tile
    const double* x;                    // (K, D)     the L-BFGS state: the last accepted point
    const double* g;                    // (K, D)     the gradient of phi = -lp there
    const double* S;                    // (K, 10, D)
    const double* Y;                    // (K, 10, D)
    const double* sc;                   // (K, 24)
    const int* ist;                     // (K, 8)
    const unsigned long long* seeds;    // (K) the problems' stream keys
    int* seen;                          // (K) nit of the last proposal (in / out)
    double h0;                          // > 0: the base gamma; else the newest pair's s.y / y.y
    int* fresh;                         // (K)
    double* mu;                         // (K, D)
    double* cov;                        // (K, D, D)
    double* X;                          // (K, M, D)
    double* logq;                       // (K)
    int* info;                          // (K)
};

__host__ __device__ inline int pf_tile_rows(int D, int NT) { return (NT * PF_Q) / D > 1 ? (NT * PF_Q) / D : 1; }
// LDS doubles per problem: H (D x ld) + S, Y (10 x D each) + u, g, mean, pivots (D each) + s.y (10) + the row tile + 4 partial sums
__host__ __device__ inline int pf_lds_doubles(int D, int ld, int ldy, int tr) {
    return D * ld + 2 * GL_M * D + 4 * D + GL_M + tr * ldy + 4;
}

template <int NT>
__global__ __launch_bounds__(256) void k_pf_propose(pf_args a) {
    extern __shared__ double pf_sm[];
    constexpr int PPW = 256 / NT;
    constexpr int MAXE = NT == 256 ? (GB_MAX_D * GB_MAX_D) / 256 : (16 * 16) / 64;   // matrix entries per thread
    const int D = a.D, ld = a.ld, ldy = a.ldy, TR = a.tr, DD = D * D;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;               // a tail slot runs every barrier and nothing else
    double* H = pf_sm + (size_t)slot * pf_lds_doubles(D, ld, ldy, TR);
    double* Sl = H + D * ld;                  // 10 x D
    double* Yl = Sl + GL_M * D;               // 10 x D
    double* u = Yl + GL_M * D;                // D      H y
    double* gl = u + D;                       // D      gradient
    double* m = gl + D;                       // D      mean
    double* pv = m + D;                       // D      pivots R_cc
    double* lsy = pv + D;                     // 10     s.y of the slots
    double* T = lsy + GL_M;                   // TR x ldy  the draws of a tile
    double* red = T + TR * ldy;               // 4      per-wave partial sums
    const size_t kk = (size_t)(valid ? k : 0), kd = kk * D, kdd = kk * DD;
    const size_t krow = kk * (size_t)a.M * D;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    int np = 0, head = 0, nit = 0;
    bool on = false;                          // valid and fresh: uniform in the slot (every thread reads the same words)
    double xl = 0.0;
    if (valid) {
        nit = a.ist[kk * GL_NIS + GL_NIT];
        gl_load_ring(a.ist + kk * GL_NIS, np, head);
        on = nit != a.seen[kk];               // seen[k] is written by thread 0 after the last barrier of the launch
    }
    if (on) {
        double gamma = a.h0;
        if (!(gamma > 0.0)) {
            const int nw = head == 0 ? GL_M - 1 : head - 1;
            gamma = np > 0 ? a.sc[kk * GL_NSC + GL_SY + nw] / a.sc[kk * GL_NSC + GL_YY + nw] : 1.0;
        }
        gl_dense_fill<NT>(D, l, ld, np, head, gamma, a.S, a.Y, kk, H, Sl, Yl);
        if (l < D) {
            gl[l] = a.g[kd + l];
            xl = a.x[kd + l];
        }
    }
    gl_dense_rounds<NT>(on, D, l, ld, np, head, H, Sl, Yl, u, lsy);
    if (on) {
        for (int e = l; e < DD; e += NT) {
            const int i = e / D, j = e - i * D;
            a.cov[kdd + e] = H[i * ld + j];
        }
        if (l < D) {                                                    // mu = x - Sigma g, the products in the order 0 .. D - 1
            double acc = 0.0;
            for (int j = 0; j < D; ++j) acc += H[l * ld + j] * gl[j];
            const double ml = xl - acc;
            m[l] = ml;
            a.mu[kd + l] = ml;
        }
    }
    __syncthreads();                          // the factorisation overwrites H
    const int info = gb_chol_lds<NT, MAXE>(on, D, l, ld, H, pv);
    __syncthreads();
    bool ok = on && info == 0;
    if (ok)
        for (int j = 0; j < D; ++j) ok = ok && gb_finite(m[j]);         // every thread the same D words

    double acc = 0.0;                         // this thread's share of sum |z|^2
    for (long long t0 = 0; t0 < a.M; t0 += TR) {
        const int tr = (int)(a.M - t0 < TR ? a.M - t0 : TR), te = tr * D;
        if (on) {                             // the tile's elements n0 .. n0 + te - 1 of the stream: pairs n0 / 2 .. (n0 + te - 1) / 2
            const unsigned long long seed = a.seeds[kk], call = (unsigned long long)(long long)nit;
            const long long n0 = t0 * D, p0 = n0 >> 1, p1 = (n0 + te - 1) >> 1;
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
        if (on) {                             // x = mu + z R   (k_kl_batched's order: the products, then the mean)
            for (int e = l; e < te; e += NT) {
                const int r = e / D, j = e - r * D;
                double s = 0.0;
                for (int i = 0; i <= j; ++i) s += T[r * ldy + i] * H[i * ld + j];
                a.X[krow + (size_t)(t0 + r) * D + j] = ok ? s + m[j] : qnan;
            }
        } else if (valid) {                   // not fresh: the rows are the point itself
            for (int e = l; e < te; e += NT) {
                const int r = e / D, j = e - r * D;
                a.X[krow + (size_t)(t0 + r) * D + j] = a.x[kd + j];
            }
        }
        __syncthreads();                      // the next tile overwrites T
    }

    acc = gb_slot_sum<NT>(acc, l, red);
    if (valid && l == 0) {
        if (on) {
            a.logq[kk] = gb_logq_sum(ok, acc, a.M, D, pv);
            a.info[kk] = info;
            a.fresh[kk] = 1;
            a.seen[kk] = nit;
        } else {
            a.logq[kk] = qnan;
            a.fresh[kk] = 0;
        }
    }
}

struct ps_args {
    long long K, M;
    int D;
    const double* lpsum;    // (K) sum of lp over the rows of X_k
    const double* logq;     // (K)
    const int* fresh;       // (K)
    const int* info;        // (K)
    const int* ist;         // (K, 8)
    const double* mu;       // (K, D)
    const double* cov;      // (K, D, D)
    double* elbo_last;      // (K)
    int* npts;              // (K)
    double* best_elbo;      // (K)
    double* best_mean;      // (K, D)
    double* best_cov;       // (K, D, D)
    int* best_it;           // (K)
};

template <int NT>
__global__ __launch_bounds__(256) void k_pf_select(ps_args a) {
    constexpr int PPW = 256 / NT;
    const int D = a.D, DD = D * D;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;
    const size_t kk = (size_t)(valid ? k : 0);
    double e = __longlong_as_double(0x7ff8000000000000LL);
    bool fr = false, take = false;
    if (valid) {
        fr = a.fresh[kk] != 0;
        if (fr && a.info[kk] == 0) e = (a.lpsum[kk] - a.logq[kk]) / (double)a.M;
        take = fr && gb_finite(e) && e > a.best_elbo[kk];
    }
    __syncthreads();                          // every wave of the slot has read best_elbo[k] before thread 0 replaces it
    if (!valid) return;
    if (l == 0) {
        a.elbo_last[kk] = e;
        if (fr) a.npts[kk] += 1;
    }
    if (!take) return;
    if (l == 0) {
        a.best_elbo[kk] = e;
        a.best_it[kk] = a.ist[kk * GL_NIS + GL_NIT];
    }
    for (int i = l; i < D; i += NT) a.best_mean[kk * D + i] = a.mu[kk * D + i];
    for (int i = l; i < DD; i += NT) a.best_cov[kk * DD + i] = a.cov[kk * DD + i];
}

// dynamic LDS bytes of a propose launch at D: at most 53 KB (D = 64), below the default limit, so no kernel attribute is needed
static size_t pf_launch_lds(int D, int* ppw, int* tr) {
    const int nt = gb_nt(D);
    *ppw = 256 / nt;
    *tr = pf_tile_rows(D, nt);
    return (size_t)*ppw * pf_lds_doubles(D, D | 1, D | 1, *tr) * sizeof(double);
}

extern "C" {

int gsmvi_pathfinder_propose_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t M, const double* x,
                                         const double* g, const double* S, const double* Y, const double* sc, const int* ist,
                                         const uint64_t* seeds, int* seen, double h0, int* fresh, double* mu, double* cov,
                                         double* X, double* logq_sum, int* info) {
    if (int st = gb_check_shape(__func__, K, D, gb_ppw)) return st;
    GB_BAD(M < 1 || M > PF_MAX_DRAWS, "M must be in [1, 4096]");
    GB_BAD(M > (INT64_MAX / 8 / D) / K, "K M D is too large");
    GB_BAD(!x || !g || !S || !Y || !sc || !ist || !seeds || !seen || !fresh || !mu || !cov || !X || !logq_sum || !info, "NULL array");
    GB_BAD(!(h0 >= 0.0) || !(h0 < __builtin_huge_val()), "h0 must be 0 (the newest pair's scale) or a positive finite number");
    const size_t nk = (size_t)K * 8, ni = (size_t)K * 4, nv = (size_t)K * D * 8, nm = nv * D, nh = nv * GL_M,
                 nx = (size_t)K * M * D * 8;
    if (int st = gb_check_overlaps(__func__, {{x, nv, "x", GB_RD}, {g, nv, "g", GB_RD}, {S, nh, "S", GB_RD}, {Y, nh, "Y", GB_RD},
                                              {sc, (size_t)K * GL_NSC * 8, "sc", GB_RD}, {ist, (size_t)K * GL_NIS * 4, "ist", GB_RD},
                                              {seeds, nk, "seeds", GB_RD}, {seen, ni, "seen", GB_WR}, {fresh, ni, "fresh", GB_WR},
                                              {mu, nv, "mu", GB_WR}, {cov, nm, "cov", GB_WR}, {X, nx, "X", GB_WR},
                                              {logq_sum, nk, "logq_sum", GB_WR}, {info, ni, "info", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    pf_args a = {};
    a.K = K; a.M = M; a.D = D; a.ld = D | 1; a.ldy = D | 1; a.x = x; a.g = g; a.S = S; a.Y = Y; a.sc = sc; a.ist = ist;
    a.seeds = reinterpret_cast<const unsigned long long*>(seeds); a.seen = seen; a.h0 = h0; a.fresh = fresh; a.mu = mu; a.cov = cov;
    a.X = X; a.logq = logq_sum; a.info = info;
    int ppw;
    const size_t lds = pf_launch_lds(D, &ppw, &a.tr);
    const unsigned grid = (unsigned)((K + ppw - 1) / ppw);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (ppw == 4)
        hipLaunchKernelGGL(k_pf_propose<64>, dim3(grid), dim3(256), lds, st, a);
    else
        hipLaunchKernelGGL(k_pf_propose<256>, dim3(grid), dim3(256), lds, st, a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_PATHFINDER, "k_pf_propose");
}

int gsmvi_pathfinder_select_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t M, const double* lpsum,
                                        const double* logq_sum, const int* fresh, const int* info, const int* ist, const double* mu,
                                        const double* cov, double* elbo_last, int* npts, double* best_elbo, double* best_mean,
                                        double* best_cov, int* best_it) {
    if (int st = gb_check_shape(__func__, K, D, gb_ppw)) return st;
    GB_BAD(M < 1 || M > PF_MAX_DRAWS, "M must be in [1, 4096]");
    GB_BAD(!lpsum || !logq_sum || !fresh || !info || !ist || !mu || !cov || !elbo_last || !npts || !best_elbo || !best_mean ||
               !best_cov || !best_it, "NULL array");
    const size_t nk = (size_t)K * 8, ni = (size_t)K * 4, nv = (size_t)K * D * 8, nm = nv * D;
    if (int st = gb_check_overlaps(__func__, {{lpsum, nk, "lpsum", GB_RD}, {logq_sum, nk, "logq_sum", GB_RD}, {fresh, ni, "fresh", GB_RD},
                                              {info, ni, "info", GB_RD}, {ist, (size_t)K * GL_NIS * 4, "ist", GB_RD}, {mu, nv, "mu", GB_RD},
                                              {cov, nm, "cov", GB_RD}, {elbo_last, nk, "elbo_last", GB_WR}, {npts, ni, "npts", GB_WR},
                                              {best_elbo, nk, "best_elbo", GB_WR}, {best_mean, nv, "best_mean", GB_WR},
                                              {best_cov, nm, "best_cov", GB_WR}, {best_it, ni, "best_it", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    ps_args a = {};
    a.K = K; a.M = M; a.D = D; a.lpsum = lpsum; a.logq = logq_sum; a.fresh = fresh; a.info = info; a.ist = ist; a.mu = mu; a.cov = cov;
    a.elbo_last = elbo_last; a.npts = npts; a.best_elbo = best_elbo; a.best_mean = best_mean; a.best_cov = best_cov; a.best_it = best_it;
    const int ppw = 256 / gb_nt(D);
    const unsigned grid = (unsigned)((K + ppw - 1) / ppw);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (ppw == 4)
        hipLaunchKernelGGL(k_pf_select<64>, dim3(grid), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(k_pf_select<256>, dim3(grid), dim3(256), 0, st, a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_PATHFINDER, "k_pf_select");
}

// include/gsmvi_hip_debug.h: what a propose launch at D requests (exported by the debug library only)
int gsmvi_debug_pathfinder_batched_lds(int D, size_t* bytes, int* problems_per_workgroup, int* tile_rows) {
    GB_BAD(D < 1 || D > GB_MAX_D || !bytes || !problems_per_workgroup || !tile_rows, "bad shape or NULL output");
    *bytes = pf_launch_lds(D, problems_per_workgroup, tile_rows);
    return GSMVI_OK;
}

}  // extern "C"
