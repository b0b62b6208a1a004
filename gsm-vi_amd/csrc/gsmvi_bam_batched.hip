// Batched BaM: K independent problems of the same (D, B), D <= 64, B <= 32, each in one launch.
//
// The reference's BaM update is a pure function of (samples, vs, mu0, S0, reg) (gsmvi/bam.py:31-114), which its users batch
// with jax.vmap.  Here, as in k_gsm_batched (gsmvi_batched.hip), a problem lives in the LDS of one workgroup slot from its
// first read to its last write:
//   k_bam_batched<NT, BB_UPDATE> : (mu_k, S_k) = bam_lowrank_update(X_k, G_k, mu0_k, S0_k, reg_k), symmetrised, + jitter I
//   k_bam_batched<NT, BB_STEP>   : the same update + jitter I, the Cholesky test of S'_k, accept or revert of (mean, cov,
//                                  factor) PER PROBLEM and the next samples (bam.py:189-212; gb_fit_tail, gsmvi_batched.h)
// The fit starts with k_gsm_batched<NT, GB_INIT> (gsmvi_gsm_fit_init_batched_f64): a BaM fit starts exactly like a GSM fit.
//
// Per problem the algebra of the single dense update (gsmvi_bam.hip), with n = B:
//   Qt (n x D) rows  sqrt(reg/B) helmert_k(g), k < B;  sqrt(reg/(1+reg)) gbar            (bam.py:55-59)
//   Vf (n x D) rows  sqrt(reg/B) helmert_k(x), k < B;  sqrt(reg/(1+reg)) (mu0 - xbar)   V = S0 + Vf^T Vf (bam.py:50-53,60)
//   P = Qt S0;  N0 = P Qt^T, M1 = Vf Qt^T;  N = M1^T M1 + sym(N0);  A^T = P + M1^T Vf                 (bam.py:105-107)
//   BB = N + I/2 + (N + I/4)^(1/2) = L L^T   (scaled coupled Newton-Schulz, the recurrence of gsmvi_bam_small.hip)  (:108-109)
//   Z = L^-1 A^T;  S = sym(S0 + Vf^T Vf - Z^T Z);  mu = mu0/(1+reg) + reg/(1+reg) (S gbar + xbar)    (bam.py:110-112)
// Plain fp64 loops: at n <= 32 and D <= 64 the 16 x 16 MFMA fragments of the single-problem kernels would be mostly padding.
// The square root runs each problem's own step count k*: the workgroup runs the largest k* of its slots, and a slot past its
// own k* only waits at the barriers, so its bits never depend on its neighbours.  A non-finite score or a failed chain
// (the scale s not finite, or BB not positive definite) poisons that problem's S' with NaN: UPDATE writes NaN and info = 1,
// STEP reverts it.  Row strides of the D x D and n x n arrays are odd (D | 1, n | 1): a lane walking down a column then
// meets a different LDS bank on every row (knob "bam_batched_pad" = 0 gives the unpadded strides, for A/B runs).
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "../../include/gsmvi_hip.h"
#include "../../include/gsmvi_hip_debug.h"   // gsmvi_debug_bam_batched_lds
#include <cstdint>

#define BB_KMAX 32       // Newton-Schulz steps at most (gsmvi_bam_small.hip BAMS_KMAX): cond(N + I/4) beyond ~1e12 fails
#define BB_SC 40         // per-problem scalars: [0, 32) c_k^2, [32] s, [33] k*, [34] 1 = the chain failed

enum { BB_UPDATE = 0, BB_STEP = 1 };

__host__ __device__ inline int bb_ld(int D) { return D | 1; }
__host__ __device__ inline int bb_ldn(int B) { return B | 1; }
// LDS doubles per problem at row strides (ld, ldn): S (D x ld) + Qt, Vf, P / A^T / Z (n x ld each) + N, M1, Y (2), Z (2), M
// (n x ldn each) + xbar, gbar, mu0, mu, pivots (D each) + BB_SC scalars + the n pivots of BB.  (64, 32) padded: 18184 doubles
// = 145 KB, one problem per workgroup; (10, 2): 254 doubles.
__host__ __device__ inline int bb_lds_doubles(int D, int B, int ld, int ldn) {
    return D * ld + 3 * B * ld + 7 * B * ldn + 5 * D + BB_SC + B;
}
__host__ __device__ inline int bb_lds_doubles(int D, int B) { return bb_lds_doubles(D, B, bb_ld(D), bb_ldn(B)); }
// four problems (one wave each) per workgroup for D <= 16 when they fit in 160 KiB together, else one problem on 256 threads
static inline int bb_nt(int D, int B) { return (D <= 16 && 4 * 8 * bb_lds_doubles(D, B) <= GB_LDS_MAX) ? 64 : 256; }
static inline int bb_ppw(int D, int B) { return 256 / bb_nt(D, B); }

template <int NT, int MODE>
__global__ __launch_bounds__(256) void k_bam_batched(gb_args a) {
    extern __shared__ double bb_sm[];
    constexpr int PPW = 256 / NT;
    constexpr int MAXE = NT == 256 ? (GB_MAX_D * GB_MAX_D) / 256 : (16 * 16) / 64;   // matrix entries per thread
    const int D = a.D, B = a.B, n = B, ld = a.ld, ldn = a.ldn, DD = D * D, BD = B * D, NN = n * n, ND = n * D;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;               // a tail slot runs every barrier and nothing else
    const int per = bb_lds_doubles(D, B, ld, ldn);
    double* S = bb_sm + (size_t)slot * per;   // D x ld  S0; then S'; then its factor (gb_fit_tail)
    double* Qt = S + D * ld;                  // n x ld  raw scores, then Qt; later (with Vf) the draws
    double* Vf = Qt + n * ld;                 // n x ld  raw samples, then Vf
    double* P = Vf + n * ld;                  // n x ld  P, then A^T, then Z
    double* Nm = P + n * ld;                  // n x ldn N
    double* M1 = Nm + n * ldn;                // n x ldn M1
    double* Ys = M1 + n * ldn;                // 2 n x ldn  Newton-Schulz Y (two buffers); N0 before the iteration
    double* Zs = Ys + 2 * n * ldn;            // 2 n x ldn  Newton-Schulz Z
    double* Mm = Zs + 2 * n * ldn;            // n x ldn M = c^2 Z Y; then BB and its factor
    double* xb = Mm + n * ldn;                // D xbar
    double* gbv = xb + D;                     // D gbar
    double* m0 = gbv + D;                     // D mean in
    double* m1 = m0 + D;                      // D mean out
    double* pv = m1 + D;                      // D pivots of the test (gb_fit_tail)
    double* sc = pv + D;                      // BB_SC scalars
    double* pn = sc + BB_SC;                  // n pivots of BB
    const size_t kd = (size_t)(valid ? k : 0) * D, kdd = (size_t)(valid ? k : 0) * DD, kbd = (size_t)(valid ? k : 0) * BD;
    const double* mu_in = MODE == BB_UPDATE ? a.mu0 : a.mu;
    const double* S_in = MODE == BB_UPDATE ? a.S0 : a.S;
    const double reg = valid ? (a.reg_dev ? a.reg_dev[k] : a.reg) : 1.0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    double sreg[MAXE];

    if (valid) {
        for (int i = l; i < D; i += NT) m0[i] = mu_in[kd + i];
        for (int e = l; e < DD; e += NT) {                              // all of S0 (both triangles)
            const int i = e / D, j = e - i * D;
            S[i * ld + j] = S_in[kdd + e];
        }
        for (int e = l; e < BD; e += NT) {
            const int b = e / D, j = e - b * D;
            Vf[b * ld + j] = a.X[kbd + e];
            Qt[b * ld + j] = a.V[kbd + e];
        }
    }
    __syncthreads();
    if (valid) {                                  // means and Helmert rows of the centred samples and scores (bam.py:50-60)
        const double as = sqrt(reg / B), r1s = sqrt(reg / (1.0 + reg));
        for (int i = l; i < D; i += NT) {
            double sx = 0.0, sg = 0.0;
            for (int b = 0; b < B; ++b) {
                sx += Vf[b * ld + i];
                sg += Qt[b * ld + i];
            }
            const double xbar = sx / B, gbar = sg / B;
            double px = Vf[i] - xbar, pg = Qt[i] - gbar;                // prefix sums of the centred values
            for (int h = 1; h < B; ++h) {                               // row h - 1 = (sum_{j<h} c_j - h c_h) / sqrt(h (h + 1))
                const double cx = Vf[h * ld + i] - xbar, cg = Qt[h * ld + i] - gbar;
                const double w = 1.0 / sqrt((double)h * (double)(h + 1));
                Vf[(h - 1) * ld + i] = as * ((px - h * cx) * w);
                Qt[(h - 1) * ld + i] = as * ((pg - h * cg) * w);
                px += cx;
                pg += cg;
            }
            Vf[(n - 1) * ld + i] = r1s * (m0[i] - xbar);
            Qt[(n - 1) * ld + i] = r1s * gbar;
            xb[i] = xbar;
            gbv[i] = gbar;
        }
    }
    __syncthreads();
    if (valid) {                                  // P = Qt S0
        for (int e = l; e < ND; e += NT) {
            const int r = e / D, j = e - r * D;
            double s = 0.0;
            for (int i = 0; i < D; ++i) s += Qt[r * ld + i] * S[i * ld + j];
            P[r * ld + j] = s;
        }
    }
    __syncthreads();
    double* N0 = Ys;
    if (valid) {                                  // N0 = P Qt^T, M1 = Vf Qt^T
        for (int e = l; e < NN; e += NT) {
            const int r = e / n, c = e - r * n;
            double s0 = 0.0, s1 = 0.0;
            for (int i = 0; i < D; ++i) {
                const double q = Qt[c * ld + i];
                s0 += P[r * ld + i] * q;
                s1 += Vf[r * ld + i] * q;
            }
            N0[r * ldn + c] = s0;
            M1[r * ldn + c] = s1;
        }
    }
    __syncthreads();
    if (valid) {                                  // N = M1^T M1 + sym(N0) (exactly symmetric), A^T = P + M1^T Vf in place
        for (int e = l; e < NN; e += NT) {
            const int r = e / n, c = e - r * n;
            double s = 0.0;
            for (int q = 0; q < n; ++q) s += M1[q * ldn + r] * M1[q * ldn + c];
            Nm[r * ldn + c] = s + 0.5 * (N0[r * ldn + c] + N0[c * ldn + r]);
        }
        for (int e = l; e < ND; e += NT) {
            const int r = e / D, j = e - r * D;
            double s = P[r * ld + j];
            for (int q = 0; q < n; ++q) s += M1[q * ldn + r] * Vf[q * ld + j];
            P[r * ld + j] = s;
        }
    }
    __syncthreads();
    // s = trace(N + I/4) >= lambda_max and the scaling recurrence of gsmvi_bam_small.hip (k_bam_ns_step0): the eigenvalues of
    // Z Y start in [1/(4s), 1] and obey mu <- f(c^2 mu), f(x) = x (3 - x)^2 / 4, c^2 = 3 / (1 + sqrt(l) + l) from the bound l
    if (l == 0) {
        int kst = 0, failed = 0;
        double s = 1.0;
        if (valid) {
            double tr = 0.0;
            for (int i = 0; i < n; ++i) tr += Nm[i * ldn + i] + 0.25;
            s = tr;
            const bool s_ok = (s == s) && s > 0.0 && s < 1e300;
            double lb = 0.25 / s;
            if (!(lb > 0.0) || lb > 1.0) lb = 1.0;
            kst = BB_KMAX + 1;
            for (int q = 0; q < BB_KMAX; ++q) {
                const double c2 = (lb < 0.25) ? 3.0 / (1.0 + sqrt(lb) + lb) : 1.0;
                sc[q] = c2;
                const double x = c2 * lb;
                lb = x * (3.0 - x) * (3.0 - x) * 0.25;
                if (lb > 1.0) lb = 1.0;
                if (1.0 - lb < 5e-9 && kst > BB_KMAX) kst = q + 2;
                if (q + 1 >= kst) break;
            }
            failed = (!s_ok || kst > BB_KMAX) ? 1 : 0;    // the bound did not close in BB_KMAX steps (trace beyond ~1e21)
            if (failed) kst = 0;                             // -> no iteration, S' poisoned below: UPDATE NaN + info, STEP revert
        }
        sc[32] = s;
        sc[33] = (double)kst;
        sc[34] = (double)failed;
    }
    __syncthreads();
    int kmax = 0;                                 // the workgroup runs the largest step count of its slots
#pragma unroll
    for (int p = 0; p < PPW; ++p) kmax = max(kmax, (int)bb_sm[(size_t)p * per + (sc + 33 - S)]);
    const int kst = (int)sc[33];
    const double s = sc[32];
    bool bad = sc[34] != 0.0;
    if (valid) {                                  // Y0 = (N + I/4) / s, Z0 = I
        const double sinv = 1.0 / s;
        for (int e = l; e < NN; e += NT) {
            const int r = e / n, c = e - r * n;
            Ys[r * ldn + c] = (Nm[r * ldn + c] + (r == c ? 0.25 : 0.0)) * sinv;
            Zs[r * ldn + c] = r == c ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    // coupled Newton-Schulz in product form (Higham (6.35)): M = c^2 Z Y, T = (3 I - M) / 2, Y <- c Y T, Z <- c T Z
    for (int it = 0; it < kmax; ++it) {
        const bool act = valid && it < kst;       // uniform in the slot
        const double* Y = Ys + (it & 1) * n * ldn;
        const double* Z = Zs + (it & 1) * n * ldn;
        double* Yo = Ys + ((it & 1) ^ 1) * n * ldn;
        double* Zo = Zs + ((it & 1) ^ 1) * n * ldn;
        const double c2 = act ? sc[it] : 1.0, c = sqrt(c2);
        if (act) {
            for (int e = l; e < NN; e += NT) {
                const int r = e / n, j = e - r * n;
                double m = 0.0;
                for (int q = 0; q < n; ++q) m += Z[r * ldn + q] * Y[q * ldn + j];
                Mm[r * ldn + j] = m;
            }
        }
        __syncthreads();
        if (act) {
            for (int e = l; e < NN; e += NT) {
                const int r = e / n, j = e - r * n;
                double sy = 0.0, sz = 0.0;
                for (int q = 0; q < n; ++q) {
                    const double tqj = (q == j ? 1.5 : 0.0) - 0.5 * c2 * Mm[q * ldn + j];
                    const double trq = (r == q ? 1.5 : 0.0) - 0.5 * c2 * Mm[r * ldn + q];
                    sy += Y[r * ldn + q] * tqj;
                    sz += trq * Z[q * ldn + j];
                }
                Yo[r * ldn + j] = c * sy;
                Zo[r * ldn + j] = c * sz;
            }
        }
        __syncthreads();
    }
    if (valid) {                                  // BB = N + I/2 + sqrt(s) sym(Y)  (the iterate k* lives in buffer k* & 1)
        const double* Yf = Ys + (kst & 1) * n * ldn;
        const double rs = sqrt(s);
        for (int e = l; e < NN; e += NT) {
            const int r = e / n, c = e - r * n;
            Mm[r * ldn + c] = Nm[r * ldn + c] + (r == c ? 0.5 : 0.0) + rs * 0.5 * (Yf[r * ldn + c] + Yf[c * ldn + r]);
        }
    }
    __syncthreads();
    // BB = R^T R (upper, in place, one pivot per barrier; L = R^T), n steps for every slot
    int cinfo = 0;
    for (int c = 0; c < n; ++c) {
        const double acc_ = Mm[c * ldn + c];
        if (cinfo == 0 && !(acc_ > 0.0 && acc_ < __builtin_huge_val())) cinfo = c + 1;
        const double piv = sqrt(acc_), inv = 1.0 / piv;
        if (l == 0) pn[c] = piv;
        if (valid) {
            for (int e = l; e < NN; e += NT) {
                const int i = e / n, j = e - i * n;
                if (i > c && j >= i) Mm[i * ldn + j] -= (Mm[c * ldn + i] * inv) * (Mm[c * ldn + j] * inv);
            }
        }
        __syncthreads();
    }
    bad = bad || cinfo != 0;
    if (valid && !bad) {
        for (int e = l; e < NN; e += NT) {
            const int i = e / n, j = e - i * n;
            Mm[i * ldn + j] = j > i ? Mm[i * ldn + j] / pn[i] : (j == i ? pn[i] : 0.0);
        }
    }
    __syncthreads();
    if (valid && !bad) {                          // Z = L^-1 A^T: forward substitution, one column per lane, L[r][q] = R[q][r]
        for (int j = l; j < D; j += NT) {
            for (int r = 0; r < n; ++r) {
                double z = P[r * ld + j];
                for (int q = 0; q < r; ++q) z -= Mm[q * ldn + r] * P[q * ld + j];
                P[r * ld + j] = z / Mm[r * ldn + r];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MAXE; ++q) {              // S' = sym(S0 + Vf^T Vf - Z^T Z): exactly symmetric (bam.py:111, :199)
        const int e = l + q * NT;
        if (valid && e < DD) {
            const int i = e / D, j = e - i * D;
            double v = 0.0, z = 0.0;
            for (int b = 0; b < n; ++b) {
                v += Vf[b * ld + i] * Vf[b * ld + j];
                z += P[b * ld + i] * P[b * ld + j];
            }
            const double sij = (S[i * ld + j] + v) - z, sji = (S[j * ld + i] + v) - z;
            sreg[q] = bad ? qnan : 0.5 * (sij + sji);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MAXE; ++q) {
        const int e = l + q * NT;
        if (valid && e < DD) {
            const int i = e / D, j = e - i * D;
            S[i * ld + j] = sreg[q];
        }
    }
    __syncthreads();
    if (valid) {                                  // mu = mu0 / (1 + reg) + reg / (1 + reg) (S gbar + xbar)   (bam.py:112)
        for (int i = l; i < D; i += NT) {
            double sg = 0.0;
            for (int j = 0; j < D; ++j) sg += S[i * ld + j] * gbv[j];
            m1[i] = bad ? qnan : m0[i] / (1.0 + reg) + reg / (1.0 + reg) * (sg + xb[i]);
        }
    }
#pragma unroll
    for (int q = 0; q < MAXE; ++q) {              // + jitter I (bam.py:198)
        const int e = l + q * NT;
        if (valid && e < DD && e / D == e - (e / D) * D) sreg[q] += a.jitter;
    }
    if (MODE == BB_UPDATE) {
        if (valid) {
            for (int i = l; i < D; i += NT) a.mu[kd + i] = m1[i];
#pragma unroll
            for (int q = 0; q < MAXE; ++q) {
                const int e = l + q * NT;
                if (e < DD) a.S[kdd + e] = sreg[q];
            }
            if (l == 0 && a.info) a.info[k] = bad ? 1 : 0;
        }
        return;
    }
    __syncthreads();                              // every read of S by the mean is done
#pragma unroll
    for (int q = 0; q < MAXE; ++q) {
        const int e = l + q * NT;
        if (valid && e < DD && e / D == e - (e / D) * D) S[(e / D) * (ld + 1)] = sreg[q];
    }
    __syncthreads();
    gb_fit_tail<NT, MAXE, false>(a, valid, k, l, ld, S, sreg, pv, Qt, m0, m1);
}

hipError_t gsmvi_bam_batched_prepare() {
    return gb_allow_lds(k_bam_batched<64, BB_UPDATE>, k_bam_batched<256, BB_UPDATE>, k_bam_batched<64, BB_STEP>,
                        k_bam_batched<256, BB_STEP>);
}

// the dynamic LDS a launch requests per workgroup (and the problems it holds) at the given row strides
static size_t bb_launch_lds(int D, int B, int ld, int ldn, int* ppw) {
    *ppw = bb_ppw(D, B);
    return (size_t)*ppw * bb_lds_doubles(D, B, ld, ldn) * sizeof(double);
}

static int bb_launch(gsmvi_ctx* ctx, void* stream, int mode, gb_args& a, const char* fn) {
    const int nt = bb_nt(a.D, a.B);
    const bool pad = ctx->tune_bam_batched_pad != 0;
    a.ld = pad ? bb_ld(a.D) : a.D;
    a.ldn = pad ? bb_ldn(a.B) : a.B;
    int ppw = 1;
    const size_t lds = bb_launch_lds(a.D, a.B, a.ld, a.ldn, &ppw);
    const unsigned grid = (unsigned)((a.K + ppw - 1) / ppw);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define BB_GO(NTV, M) hipLaunchKernelGGL((k_bam_batched<NTV, M>), dim3(grid), dim3(256), lds, st, a)
    if (nt == 64) {
        if (mode == BB_UPDATE) BB_GO(64, BB_UPDATE); else BB_GO(64, BB_STEP);
    } else {
        if (mode == BB_UPDATE) BB_GO(256, BB_UPDATE); else BB_GO(256, BB_STEP);
    }
#undef BB_GO
    return gb_launched(ctx, GSMVI_PATH_BATCHED_BAM, fn);
}

extern "C" {

int gsmvi_bam_update_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* X, const double* G,
                                 const double* mu0, const double* S0, double reg, const double* reg_dev, double jitter,
                                 double* mu, double* S, int* info_dev) {
    if (int st = gb_check_shape(__func__, K, D, bb_ppw, B)) return st;
    GB_BAD(!X || !G || !mu0 || !S0 || !mu || !S, "NULL array");
    const size_t nv = (size_t)K * D * 8, nm = (size_t)K * D * D * 8, nx = (size_t)K * B * D * 8, nk = (size_t)K * 8,
                 ni = (size_t)K * 4;
    if (int st = gb_check_overlaps(__func__, {{X, nx, "X", GB_RD}, {G, nx, "G", GB_RD}, {mu0, nv, "mu0", GB_RD},
                                              {S0, nm, "S0", GB_RD}, {reg_dev, nk, "reg_dev", GB_RD}, {mu, nv, "mu", GB_WR},
                                              {S, nm, "S", GB_WR}, {info_dev, ni, "info_dev", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    gb_args a = {};
    a.K = K; a.D = D; a.B = B; a.X = X; a.V = G; a.mu0 = mu0; a.S0 = S0; a.mu = mu; a.S = S; a.info = info_dev;
    a.reg = reg; a.reg_dev = reg_dev; a.jitter = jitter;
    return bb_launch(ctx, stream, BB_UPDATE, a, "k_bam_batched (update)");
}

int gsmvi_bam_fit_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* X, const double* G,
                                   double* mean, double* cov, double* R, double reg, const double* reg_dev, double jitter,
                                   int* info_dev, int* n_reverts_dev, const uint64_t* seeds_dev, uint64_t call, double* Xout) {
    if (int st = gb_check_shape(__func__, K, D, bb_ppw, B)) return st;
    GB_BAD(!X || !G || !mean || !cov, "NULL array");
    GB_BAD(seeds_dev && (!R || !Xout), "drawing the next samples needs the sampling factor R and Xout");
    const size_t nv = (size_t)K * D * 8, nm = (size_t)K * D * D * 8, nx = (size_t)K * B * D * 8, nk = (size_t)K * 8,
                 ni = (size_t)K * 4;
    // X counts as written (Xout may be X).  Xout == X exactly is the one overlap allowed: X's entry then stands for both.
    if (int st = gb_check_overlaps(__func__, {{X, nx, "X", GB_WR}, {G, nx, "G", GB_RD}, {mean, nv, "mean", GB_WR},
                                              {cov, nm, "cov", GB_WR}, {R, nm, "R", GB_WR}, {reg_dev, nk, "reg_dev", GB_RD},
                                              {info_dev, ni, "info_dev", GB_WR}, {n_reverts_dev, ni, "n_reverts_dev", GB_WR},
                                              {seeds_dev, nk, "seeds_dev", GB_RD}, {Xout != X ? Xout : nullptr, nx, "Xout", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    gb_args a = {};
    a.K = K; a.D = D; a.B = B; a.X = X; a.V = G; a.mu = mean; a.S = cov; a.R = R; a.info = info_dev; a.n_rev = n_reverts_dev;
    a.seeds = reinterpret_cast<const unsigned long long*>(seeds_dev); a.call = call; a.Xout = seeds_dev ? Xout : nullptr;
    a.reg = reg; a.reg_dev = reg_dev; a.jitter = jitter;
    return bb_launch(ctx, stream, BB_STEP, a, "k_bam_batched (fit step)");
}

// include/gsmvi_hip_debug.h: what a launch at (D, B) requests (exported by the debug library only)
int gsmvi_debug_bam_batched_lds(int D, int B, int pad, size_t* bytes, int* problems_per_workgroup) {
    GB_BAD(D < 1 || D > GB_MAX_D || B < 1 || B > GB_MAX_B || !bytes || !problems_per_workgroup, "bad shape or NULL output");
    *bytes = bb_launch_lds(D, B, pad ? bb_ld(D) : D, pad ? bb_ldn(B) : B, problems_per_workgroup);
    return GSMVI_OK;
}

}  // extern "C"
