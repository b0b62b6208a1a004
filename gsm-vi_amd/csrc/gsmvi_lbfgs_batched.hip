// Batched L-BFGS initialiser: K independent minimisations of phi_k = -lp_k of one D <= 64, one launch per function evaluation
// after the score and lp ("Batched L-BFGS initialiser").
//
// The reference starts its fits from gsmvi/initializers.py:5-17: the L-BFGS-B maximiser of lp as the mean and the optimiser's
// dense inverse-Hessian estimate (scipy.optimize.LbfgsInvHessProduct(S, Y).todense()) as the covariance.  Here plain L-BFGS
// with history 10 and a backtracking (Armijo, c1 = 1e-4, halving) line search, for every problem at once:
//   k_lbfgs_step_batched<NT>     : start != 0: the first evaluation (f, g at x0) -> status 4 (non-finite), 1 (max|g| <= gtol) or
//                                  the steepest-descent start d = -g, t = min(1, 1 / |g|), trial point x + t d.
//                                  start == 0: (ft, gt) at the trial point -> reject (t halved, next trial point; 21 rejections
//                                  = status 3) or accept (s = xt - x, y = gt - g, the pair stored iff s.y > 2.2e-16 y.y, the
//                                  stopping tests, the two-loop recursion for the next direction, t = 1, next trial point).
//   k_lbfgs_hess_inv_batched<NT> : cov_k = H_n, H_0 = I, H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T over the stored
//                                  pairs, oldest to newest, as H - rho (s u^T + u s^T) + (rho^2 y.u + rho) s s^T with u = H y;
//                                  exactly symmetric ((i, j) and (j, i) come from the same products in the same order).
// State (caller-owned, per problem): x, g, d (D each), the ring buffers S, Y (10 x D each), sc (24 doubles: f, t, g.d, a spare,
// s.y of the ten slots, y.y of the ten slots), ist (8 ints: status, nit, nfev, nls, pairs held, next slot to write, two spares)
// and the trial point Xt (D).  The held pairs are the slots head - n .. head - 1 (mod 10), oldest first.
// Work mapping: the slots of gsmvi_batched.h (gb_nt(D) threads per problem, four problems per 256-thread workgroup for
// D <= 16).  All threads of a slot bring the held pairs into LDS; after the one barrier of the launch the slot's first wave
// does the step with component l of every vector in lane l (D <= 64: a vector is one wave wide).  Every dot product is the
// 64-lane butterfly of that wave (gb_wave_sum of gsmvi_batched.h; lanes >= D add zeros): a fixed order that depends on nothing
// but D, and no barrier.  A lane reads and writes only column l of the LDS buffers after the barrier.  A problem that has
// stopped (status != 0) is frozen:
// the launch writes nothing of it.  A slot reads and writes only slice k of every array and every slot runs the same single
// barrier, so nothing crosses between problems.  Only the newest pair's slot of the ring buffers is written.
// The layout of the state and the ring-buffer test are gsmvi_lbfgs_state.h's, shared with gsmvi_pathfinder_batched.hip.  That
// header also holds the clamped read of the counters and the dense recursion as functions, for k_pf_propose; both kernels here
// keep the same statements inline (through the functions the step kernel lost a range proof and the dense estimate missed one
// of six cases of the speed check: DESIGN.md section 9, "One copy of each initialiser stage"), so a change to the header's copy
// belongs here too.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_lbfgs_state.h"
#include "../../include/gsmvi_hip.h"
#include "../../include/gsmvi_hip_debug.h"   // gsmvi_debug_lbfgs_batched_lds
#include <cmath>
#include <cstdint>

enum { GL_STEP = 0, GL_HESS = 1 };

struct gl_args {
    long long K;
    int D, start;
    const double* fv;    // (K)    sign * fv[k] = phi at the trial point
    const double* gv;    // (K, D) sign * gv[k] = its gradient
    double sign;
    double* x;           // (K, D)
    double* g;           // (K, D)
    double* d;           // (K, D)
    double* S;           // (K, 10, D)
    double* Y;           // (K, 10, D)
    double* sc;          // (K, 24)
    int* ist;            // (K, 8)
    double* Xt;          // (K, D) the trial point: read (the accepted point is the trial point as it was written), then written
    int* stopped;        // (1) += the problems that stopped in this launch (may be null)
    int maxiter, maxfun;
    double gtol, ftol;
};

// LDS doubles per problem.  STEP: S, Y (10 x D each) + s.y, y.y (10 each).  HESS: H (D x (D | 1)) + S, Y + u (D) + s.y (10).
__host__ __device__ inline int gl_lds_doubles(int D, int mode) {
    return mode == GL_STEP ? 2 * GL_M * D + 2 * GL_M : D * (D | 1) + 2 * GL_M * D + D + GL_M;
}

template <int NT>
__global__ __launch_bounds__(256) void k_lbfgs_step_batched(gl_args a) {
    extern __shared__ double gl_sm[];
    constexpr int PPW = 256 / NT;
    const int D = a.D;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < a.K;               // a tail slot runs the barrier and nothing else
    const size_t kk = (size_t)(valid ? k : 0), kd = kk * D;
    double* Sl = gl_sm + (size_t)slot * gl_lds_doubles(D, GL_STEP);
    double* Yl = Sl + GL_M * D;
    double* lsy = Yl + GL_M * D;
    double* lyy = lsy + GL_M;
    const int ln = l & 63;
    const bool act = ln < D;                  // this lane holds component ln of the vectors

    int* is = a.ist + kk * GL_NIS;
    double* sc = a.sc + kk * GL_NSC;
    int status = 0, nit = 0, nfev = 0, nls = 0, np = 0, head = 0;
    double f = 0.0, t = 0.0, gd = 0.0;
    if (valid && !a.start) {
        status = is[GL_STATUS]; nit = is[GL_NIT]; nfev = is[GL_NFEV]; nls = is[GL_NLS];
        np = is[GL_NP]; head = is[GL_HEAD];
        np = np < 0 ? 0 : (np > GL_M ? GL_M : np);                      // gl_load_ring's clamp, restated: through the function
        head = ((head % GL_M) + GL_M) % GL_M;                           // the compiler no longer knows np, head >= 0 below
        f = sc[GL_F]; t = sc[GL_T]; gd = sc[GL_GD];
    }
    const bool live = valid && status == 0;
    // every wave of the slot forms the decision from the same numbers: no barrier
    double ft = 0.0, gtl = 0.0;
    if (live) {
        ft = a.sign * a.fv[kk];
        if (act) gtl = a.sign * a.gv[kd + ln];
    }
    const bool fin = gb_finite(ft) && __all(gb_finite(gtl));
    const bool ok = live && !a.start && fin && ft <= f + (1e-4 * t) * gd;
    if (ok) {                                                           // the held pairs are needed for the next direction
        for (int e = l; e < GL_M * D; e += NT) {
            if (gl_held(e / D, head, np)) {
                Sl[e] = a.S[kk * GL_M * D + e];
                Yl[e] = a.Y[kk * GL_M * D + e];
            }
        }
        if (l < GL_M) lsy[l] = sc[GL_SY + l];
        else if (l < 2 * GL_M) lyy[l - GL_M] = sc[GL_YY + l - GL_M];
    }
    __syncthreads();
    if (!live || l >= 64) return;

    double xl = act ? a.x[kd + ln] : 0.0;
    double gl = 0.0, dl = 0.0;
    bool steepest = false, trial = false;

    if (a.start) {
        nfev = 1;
        f = ft;
        gl = gtl;
        const double gmax = gb_wave_max(fabs(gl));
        if (!fin) status = 4;
        else if (gmax <= a.gtol) status = 1;
        else steepest = true;
    } else {
        nfev += 1;
        if (!ok) {
            t = 0.5 * t;
            nls += 1;
            if (nls > 20) status = 3;
            else if (nfev >= a.maxfun) status = 2;
            else {
                dl = act ? a.d[kd + ln] : 0.0;
                if (act) a.Xt[kd + ln] = xl + t * dl;
            }
            if (ln == 0) {
                sc[GL_T] = t;
                is[GL_NLS] = nls; is[GL_NFEV] = nfev; is[GL_STATUS] = status;
                if (status != 0 && a.stopped) atomicAdd(a.stopped, 1);
            }
            return;
        }
        const double xtl = act ? a.Xt[kd + ln] : 0.0;
        const double g0 = act ? a.g[kd + ln] : 0.0;
        const double s = xtl - xl, y = gtl - g0;
        const double fprev = f;
        xl = xtl; f = ft; gl = gtl;
        nit += 1;
        const double sy = gb_wave_sum(s * y), yy = gb_wave_sum(y * y);
        if (sy > 2.2e-16 * yy) {
            if (act) {
                Sl[head * D + ln] = s;
                Yl[head * D + ln] = y;
                a.S[(kk * GL_M + head) * D + ln] = s;
                a.Y[(kk * GL_M + head) * D + ln] = y;
            }
            lsy[head] = sy;                                             // (every lane the same value; each reads its own write)
            lyy[head] = yy;
            if (ln == 0) {
                sc[GL_SY + head] = sy;
                sc[GL_YY + head] = yy;
            }
            head = head + 1 == GL_M ? 0 : head + 1;
            np = np < GL_M ? np + 1 : GL_M;
        }
        const double gmax = gb_wave_max(fabs(gl));
        if (gmax <= a.gtol || (fprev - f) <= a.ftol * fmax(fmax(fabs(fprev), fabs(f)), 1.0)) status = 1;
        else if (nit >= a.maxiter || nfev >= a.maxfun) status = 2;
        else if (np == 0) steepest = true;
        else {                                                          // two-loop recursion: d = -H g
            double al[GL_M];
            double q = gl;
#pragma unroll
            for (int j = 0; j < GL_M; ++j) {                            // newest to oldest
                if (j < np) {
                    const int i = head - 1 - j < 0 ? head - 1 - j + GL_M : head - 1 - j;
                    const double si = act ? Sl[i * D + ln] : 0.0, yi = act ? Yl[i * D + ln] : 0.0;
                    const double alpha = (1.0 / lsy[i]) * gb_wave_sum(si * q);
                    al[j] = alpha;
                    q = q - alpha * yi;
                }
            }
            const int i0 = head == 0 ? GL_M - 1 : head - 1;
            double r = (lsy[i0] / lyy[i0]) * q;
#pragma unroll
            for (int j = GL_M - 1; j >= 0; --j) {                       // oldest to newest
                if (j < np) {
                    const int i = head - 1 - j < 0 ? head - 1 - j + GL_M : head - 1 - j;
                    const double si = act ? Sl[i * D + ln] : 0.0, yi = act ? Yl[i * D + ln] : 0.0;
                    const double beta = (1.0 / lsy[i]) * gb_wave_sum(yi * r);
                    r = r + si * (al[j] - beta);
                }
            }
            dl = -r;
            t = 1.0;
            gd = gb_wave_sum(gl * dl);
            nls = 0;
            trial = true;
            if (!(gd < 0.0)) {                                          // not a descent direction: drop the history
                np = 0;
                head = 0;
                steepest = true;
            }
        }
    }
    if (steepest) {
        dl = -gl;
        const double nrm = sqrt(gb_wave_sum(gl * gl));
        t = fmin(1.0, 1.0 / nrm);
        gd = gb_wave_sum(gl * dl);
        nls = 0;
        trial = true;
    }
    if (act) {
        a.x[kd + ln] = xl;
        a.g[kd + ln] = gl;
        if (trial || a.start) a.d[kd + ln] = dl;
        if (trial) a.Xt[kd + ln] = xl + t * dl;
    }
    if (ln == 0) {
        sc[GL_F] = f;
        if (trial || a.start) {
            sc[GL_T] = t;
            sc[GL_GD] = gd;
        }
        if (a.start) sc[3] = 0.0;
        is[GL_STATUS] = status; is[GL_NIT] = nit; is[GL_NFEV] = nfev; is[GL_NLS] = nls; is[GL_NP] = np; is[GL_HEAD] = head;
        if (a.start) { is[6] = 0; is[7] = 0; }
        if (status != 0 && a.stopped) atomicAdd(a.stopped, 1);
    }
    if (a.start && ln < 2 * GL_M) sc[GL_SY + ln] = 0.0;                 // (GL_YY = GL_SY + 10: the twenty sums)
}

template <int NT>
__global__ __launch_bounds__(256) void k_lbfgs_hess_inv_batched(long long K, int D, const double* __restrict__ S,
                                                                const double* __restrict__ Y, const int* __restrict__ ist,
                                                                double* __restrict__ cov) {
    extern __shared__ double gl_sm[];
    constexpr int PPW = 256 / NT;
    const int ld = D | 1, DD = D * D;
    const int slot = threadIdx.x / NT, l = threadIdx.x % NT;
    const long long k = (long long)blockIdx.x * PPW + slot;
    const bool valid = k < K;
    const size_t kk = (size_t)(valid ? k : 0);
    double* H = gl_sm + (size_t)slot * gl_lds_doubles(D, GL_HESS);
    double* Sl = H + D * ld;
    double* Yl = Sl + GL_M * D;
    double* u = Yl + GL_M * D;
    double* lsy = u + D;
    // from here to the write of cov: the statements of gl_load_ring, gl_dense_fill and gl_dense_rounds (gsmvi_lbfgs_state.h) with
    // the base 1, restated; a change to either copy belongs in the other
    int np = 0, head = 0;
    if (valid) {
        np = ist[kk * GL_NIS + GL_NP];
        head = ist[kk * GL_NIS + GL_HEAD];
        np = np < 0 ? 0 : (np > GL_M ? GL_M : np);
        head = ((head % GL_M) + GL_M) % GL_M;
        for (int e = l; e < GL_M * D; e += NT) {
            const bool h = gl_held(e / D, head, np);
            Sl[e] = h ? S[kk * GL_M * D + e] : 0.0;
            Yl[e] = h ? Y[kk * GL_M * D + e] : 0.0;
        }
        for (int e = l; e < DD; e += NT) {
            const int i = e / D, j = e - i * D;
            H[i * ld + j] = i == j ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    if (valid && l < GL_M) {                                            // s.y of slot l, summed in the order 0 .. D - 1
        double acc = 0.0;
        for (int j = 0; j < D; ++j) acc += Sl[l * D + j] * Yl[l * D + j];
        lsy[l] = acc;
    }
    __syncthreads();
    for (int p = 0; p < GL_M; ++p) {                                    // oldest to newest; every slot runs all ten rounds
        const bool on = valid && p < np;
        int i = head - np + p;
        if (i < 0) i += GL_M;
        const double* s = Sl + i * D;
        const double* y = Yl + i * D;
        if (on && l < D) {                                              // u = H y
            double acc = 0.0;
            for (int j = 0; j < D; ++j) acc += H[l * ld + j] * y[j];
            u[l] = acc;
        }
        __syncthreads();
        if (on) {
            const double rho = 1.0 / lsy[i];
            double yu = 0.0;                                            // every thread the same sum in the same order
            for (int j = 0; j < D; ++j) yu += y[j] * u[j];
            const double c = (rho * rho) * yu + rho;
            for (int e = l; e < DD; e += NT) {
                const int r = e / D, q = e - r * D;
                H[r * ld + q] = (H[r * ld + q] - rho * (s[r] * u[q] + u[r] * s[q])) + c * (s[r] * s[q]);
            }
        }
        __syncthreads();
    }
    if (valid)
        for (int e = l; e < DD; e += NT) {
            const int i = e / D, j = e - i * D;
            cov[kk * DD + e] = H[i * ld + j];
        }
}

// dynamic LDS bytes of a launch at D: at most 44 KB, below the default limit, so no kernel attribute is needed
static size_t gl_launch_lds(int D, int mode, int* ppw) {
    *ppw = 256 / gb_nt(D);
    return (size_t)*ppw * gl_lds_doubles(D, mode) * sizeof(double);
}

extern "C" {

int gsmvi_lbfgs_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int start, const double* fv, const double* gv,
                                 double sign, double* x, double* g, double* d, double* S, double* Y, double* sc, int* ist,
                                 double* Xt, int* stopped_dev, int maxiter, int maxfun, double gtol, double ftol) {
    if (int st = gb_check_shape(__func__, K, D, gb_ppw)) return st;
    GB_BAD(!fv || !gv || !x || !g || !d || !S || !Y || !sc || !ist || !Xt, "NULL array");
    GB_BAD(!(sign == 1.0 || sign == -1.0), "sign must be 1 or -1");
    GB_BAD(maxiter < 1 || maxfun < 2, "maxiter must be at least 1 and maxfun at least 2");
    GB_BAD(!(gtol >= 0.0) || !(ftol >= 0.0), "gtol and ftol must be >= 0");
    const size_t nk = (size_t)K * 8, nv = (size_t)K * D * 8, nh = nv * GL_M, ns = (size_t)K * GL_NSC * 8,
                 ni = (size_t)K * GL_NIS * 4;
    if (int st = gb_check_overlaps(__func__, {{fv, nk, "fv", GB_RD}, {gv, nv, "gv", GB_RD}, {x, nv, "x", GB_WR}, {g, nv, "g", GB_WR},
                                              {d, nv, "d", GB_WR}, {S, nh, "S", GB_WR}, {Y, nh, "Y", GB_WR}, {sc, ns, "sc", GB_WR},
                                              {ist, ni, "ist", GB_WR}, {Xt, nv, "Xt", GB_WR},
                                              {stopped_dev, 4, "stopped_dev", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    gl_args a = {};
    a.K = K; a.D = D; a.start = start != 0; a.fv = fv; a.gv = gv; a.sign = sign; a.x = x; a.g = g; a.d = d; a.S = S; a.Y = Y;
    a.sc = sc; a.ist = ist; a.Xt = Xt; a.stopped = stopped_dev; a.maxiter = maxiter; a.maxfun = maxfun; a.gtol = gtol; a.ftol = ftol;
    int ppw;
    const size_t lds = gl_launch_lds(D, GL_STEP, &ppw);
    const unsigned grid = (unsigned)((K + ppw - 1) / ppw);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (ppw == 4)
        hipLaunchKernelGGL(k_lbfgs_step_batched<64>, dim3(grid), dim3(256), lds, st, a);
    else
        hipLaunchKernelGGL(k_lbfgs_step_batched<256>, dim3(grid), dim3(256), lds, st, a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LBFGS, "k_lbfgs_step_batched");
}

int gsmvi_lbfgs_hess_inv_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, const double* S, const double* Y,
                                     const int* ist, double* cov) {
    if (int st = gb_check_shape(__func__, K, D, gb_ppw)) return st;
    GB_BAD(!S || !Y || !ist || !cov, "NULL array");
    const size_t nh = (size_t)K * GL_M * D * 8;
    if (int st = gb_check_overlaps(__func__, {{S, nh, "S", GB_RD}, {Y, nh, "Y", GB_RD}, {ist, (size_t)K * GL_NIS * 4, "ist", GB_RD},
                                              {cov, (size_t)K * D * D * 8, "cov", GB_WR}}))
        return st;
    GB_BAD(!ctx, "ctx is NULL");
    int ppw;
    const size_t lds = gl_launch_lds(D, GL_HESS, &ppw);
    const unsigned grid = (unsigned)((K + ppw - 1) / ppw);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (ppw == 4)
        hipLaunchKernelGGL(k_lbfgs_hess_inv_batched<64>, dim3(grid), dim3(256), lds, st, (long long)K, D, S, Y, ist, cov);
    else
        hipLaunchKernelGGL(k_lbfgs_hess_inv_batched<256>, dim3(grid), dim3(256), lds, st, (long long)K, D, S, Y, ist, cov);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LBFGS, "k_lbfgs_hess_inv_batched");
}

// include/gsmvi_hip_debug.h: what a launch at D requests (exported by the debug library only); mode 0 = step, 1 = hess_inv
int gsmvi_debug_lbfgs_batched_lds(int D, int mode, size_t* bytes, int* problems_per_workgroup) {
    GB_BAD(D < 1 || D > GB_MAX_D || mode < 0 || mode > 1 || !bytes || !problems_per_workgroup, "bad shape, mode or NULL output");
    *bytes = gl_launch_lds(D, mode, problems_per_workgroup);
    return GSMVI_OK;
}

}  // extern "C"
