// What the five batched Laplace kernels share around their sweep over the data ("The Laplace stage block"):
// lp_io, the state and output fields that end every kernel's argument block; the tail after the sweep -- the layout of the Newton
// state, the in-LDS Cholesky factorisation with the relative pivot rule, the write of H, the inverse R^{-1} R^{-T}, and the accept /
// reject decision, the stopping tests, the two triangular solves and the state update of one Newton round, the state machine
// documented for gsmvi_laplace_step_batched_f64 in include/gsmvi_hip.h; and on the host what the ten entry points check and set
// after their model's checks.  The tail serves gsmvi_softmax_laplace_batched.hip, gsmvi_laplace_shared_batched.hip,
// gsmvi_negbin_laplace_batched.hip (its last-pivot rule stands between lp_chol_lds and lp_step_tail) and
// gsmvi_ordinal_laplace_batched.hip (its retry rule, likewise).  The GLM kernel (gsmvi_laplace_batched.hip) takes lp_chol_lds from
// here and keeps the statements of the rest of the tail inline, and a change to one copy belongs in the other: with its tail from
// this header its listing is not the parent's, and in the A/B against the parent's library with the parent's own copy as the
// noise base it passes 17 of 18 cases and misses one (Hessian at K = 8192, N = 1024, D = 64: +0.45 % against a margin of 0.37 %;
// profiles/batched/laplace_glm_tail_ab_parent.txt), so by the rule of that pass the copy stays.
// The sweep itself (block map, prefetched tile walk, row counts) stays inline in each kernel: as functions those pieces reach the
// tile loop already unrolled, the compiler then lifts the put's eight LDS addresses out of the loop, and 14 of 90 cases of that A/B
// missed and four instantiations took 2 to 6 more VGPRs (profiles/batched/laplace_sweep_ab_parent.txt).
// Every function is for the problem of one workgroup slot: l is the thread's index in the slot (NT threads), Hs the slot's D x D
// matrix in LDS with row stride ldh, and every slot of a workgroup calls the functions that hold a barrier.
#pragma once
#include "gsmvi_batched.h"

#define LP_NSC 4       // doubles per problem in sc
#define LP_NIS 8       // ints per problem in ist
#define LP_PIVOT_REL 1.4210854715202004e-14   // 64 eps
enum { LP_F = 0, LP_T = 1, LP_GD = 2 };
enum { LP_STATUS = 0, LP_NIT = 1, LP_NFEV = 2, LP_NLS = 3 };
enum { LP_HESS = 0, LP_STEP = 1 };

// the state and the outputs of a launch: the last member of every kernel's argument block, after its model's fields
struct lp_io {
    int start;
    // LP_HESS
    const double* X;            // (K, D)
    double* H;                  // (K, D, D) or null
    double* cov;                // (K, D, D) or null
    int* info;                  // (K), with cov
    // LP_STEP: the state
    double* x;                  // (K, D)
    double* g;                  // (K, D)
    double* d;                  // (K, D)
    double* sc;                 // (K, 4)
    int* ist;                   // (K, 8)
    double* Xt;                 // (K, D)
    int* stopped;               // (1) or null
    int maxiter, maxfun;
    double gtol;
};

// the running state of one problem (ist, sc of include/gsmvi_hip.h) in registers
struct lp_run {
    int status, nit, nfev, nls;
    double f, t, gd;
};

// what the round's evaluation says: f and the thread's component of g at the trial point, max |g|, all finite, Armijo holds, and
// whether the factorisation is needed
struct lp_verdict {
    double ft, gtl, gmax;
    bool fin, ok, need;
};

// gb_chol_lds with the relative pivot rule (dg: the diagonal of S before the factorisation): 0, or 1 + the first pivot that is
// not finite or not > 64 eps dg[c].  `on` is uniform in the slot; every slot runs the D barriers.
template <int NT, int MAXE>
__device__ __forceinline__ int lp_chol_lds(bool on, int D, int l, int ld, double* S, double* pv, const double* dg) {
    const int DD = D * D;
    int info = 0;
    for (int c = 0; c < D; ++c) {
        if (on) {
            const double acc_ = S[c * ld + c];
            if (info == 0 && !(acc_ > LP_PIVOT_REL * dg[c] && acc_ < __builtin_huge_val())) info = c + 1;
            const double piv = sqrt(acc_), inv = 1.0 / piv;
            if (l == 0) pv[c] = piv;
#pragma unroll
            for (int q = 0; q < MAXE; ++q) {
                const int e = l + q * NT;
                if (e < DD) {
                    const int i = e / D, j = e - i * D;
                    if (i > c && j >= i) S[i * ld + j] -= (S[c * ld + i] * inv) * (S[c * ld + j] * inv);
                }
            }
        }
        __syncthreads();
    }
    if (on) {
#pragma unroll
        for (int q = 0; q < MAXE; ++q) {
            const int e = l + q * NT;
            if (e < DD) {
                const int i = e / D, j = e - i * D;
                if (j > i) S[i * ld + j] = S[i * ld + j] / pv[i];
                else if (j == i) S[i * ld + j] = pv[i];
            }
        }
    }
    __syncthreads();
    return info;
}

// the state of problem kk at the start of a round (zeros at the first one)
__device__ __forceinline__ void lp_load_state(const lp_io& a, bool valid, const int* is, const double* sc, lp_run& s) {
    s.status = 0; s.nit = 0; s.nfev = 0; s.nls = 0;
    s.f = 0.0; s.t = 0.0; s.gd = 0.0;
    if (valid && !a.start) {
        s.status = is[LP_STATUS]; s.nit = is[LP_NIT]; s.nfev = is[LP_NFEV]; s.nls = is[LP_NLS];
        s.f = sc[LP_F]; s.t = sc[LP_T]; s.gd = sc[LP_GD];
    }
}

// LP_STEP: f = cell[1] and g = gs at the trial point (NaN when `bad`), the Armijo test against the state, and whether a new
// direction will be needed
__device__ __forceinline__ void lp_step_test(const lp_io& a, bool live, bool bad, int D, int ln, const double* gs, const double* cell,
                                             const lp_run& s, lp_verdict& v) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    v.ok = false;
    v.need = false;
    v.ft = bad ? qnan : cell[1];
    v.gtl = ln < D ? (bad ? qnan : gs[ln]) : 0.0;
    v.fin = !bad && gb_finite(v.ft) && __all(gb_finite(v.gtl));
    v.gmax = gb_wave_max(fabs(v.gtl));
    if (live) {
        if (a.start)
            v.need = v.fin && !(v.gmax <= a.gtol);
        else {
            v.ok = v.fin && v.ft <= (s.f + (1e-4 * s.t) * s.gd) + 1e-10 * fmax(1.0, fabs(s.f));
            v.need = v.ok && !(v.gmax <= a.gtol) && !(s.nit + 1 >= a.maxiter || s.nfev + 1 >= a.maxfun);
        }
    }
}

// LP_HESS: H of a live problem from LDS (the upper triangle holds it; NaN when `bad`), then the barrier after which the
// factorisation may overwrite it: entry (i, j), i > j, is read from another thread's cell (j, i)
template <int NT, int MAXE>
__device__ __forceinline__ void lp_write_h(const lp_io& a, bool live, bool bad, size_t kk, int D, int l, int ldh, const double* Hs) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const int DD = D * D;
    if (live && a.H) {
#pragma unroll
        for (int q = 0; q < MAXE; ++q) {
            const int e = l + q * NT;
            if (e < DD) {
                const int i = e / D, j = e - i * D;
                a.H[kk * DD + e] = bad ? qnan : (i <= j ? Hs[i * ldh + j] : Hs[j * ldh + i]);
            }
        }
    }
    __syncthreads();
}

// LP_HESS after the factorisation: cov = R^{-1} R^{-T} (thread j back-substitutes column j of R^{-1} into row j of the free lower
// triangle, then entry (i, j), i <= j, is one dot product, written to (i, j) and (j, i)), or the identity, and info
template <int NT, int MAXE>
__device__ __forceinline__ void lp_inverse_tail(const lp_io& a, bool live, bool bad, bool need, int info, long long k, size_t kk, int D,
                                                int l, int ldh, double* Hs, const double* pv, double* rd) {
    const int DD = D * D;
    if (live && bad) info = 1;
    const bool inv = need && info == 0;
    if (inv && l < D) {                   // column l of R^{-1} into row l of the lower triangle, its diagonal into rd
        const int j = l;
        const double xj = 1.0 / pv[j];
        rd[j] = xj;
        for (int i = j - 1; i >= 0; --i) {
            double s = 0.0;
            for (int c = i + 1; c < j; ++c) s += Hs[i * ldh + c] * Hs[j * ldh + c];
            s += Hs[i * ldh + j] * xj;
            Hs[j * ldh + i] = -s / pv[i];
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int q = 0; q < MAXE; ++q) {
            const int e = l + q * NT;
            if (e < DD) {
                const int i = e / D, j = e - i * D;
                if (i <= j) {
                    double s;
                    if (inv) {
                        s = (i == j ? rd[j] : Hs[j * ldh + i]) * rd[j];
                        for (int c = j + 1; c < D; ++c) s += Hs[c * ldh + i] * Hs[c * ldh + j];
                    } else
                        s = i == j ? 1.0 : 0.0;                     // nothing is known: the identity
                    a.cov[kk * DD + e] = s;
                    a.cov[kk * DD + (size_t)j * D + i] = s;
                }
            }
        }
        if (l == 0) a.info[k] = info;
    }
}

// LP_STEP after the factorisation, for the first wave of a live slot (component l of every vector in lane l < 64): the state
// machine of gsmvi_laplace_step_batched_f64 (include/gsmvi_hip.h), the Newton direction by two triangular solves, the writes
__device__ __forceinline__ void lp_step_tail(const lp_io& a, lp_run s, const lp_verdict& v, int info, size_t kd, int D, int l, int ldh,
                                             const double* Hs, const double* pv, const double* xs, double* sc, int* is) {
    const bool act = l < D;
    double xl = act ? xs[l] : 0.0, gl = v.gtl, dl = 0.0;
    bool newdir = false;
    if (a.start) {
        s.nfev = 1;
        s.nit = 0;
        s.nls = 0;
        s.f = v.ft;
        s.t = 0.0;
        s.gd = 0.0;
        if (!v.fin) s.status = 4;
        else if (v.gmax <= a.gtol) s.status = 1;
        else if (info != 0) s.status = 5;
        else newdir = true;
    } else {
        s.nfev += 1;
        if (!v.ok) {
            s.t = 0.5 * s.t;
            s.nls += 1;
            if (s.nls > 20) s.status = 3;
            else if (s.nfev >= a.maxfun) s.status = 2;
            else if (act) a.Xt[kd + l] = a.x[kd + l] + s.t * a.d[kd + l];
            if (l == 0) {
                sc[LP_T] = s.t;
                is[LP_NLS] = s.nls; is[LP_NFEV] = s.nfev; is[LP_STATUS] = s.status;
                if (s.status != 0 && a.stopped) atomicAdd(a.stopped, 1);
            }
            return;
        }
        s.f = v.ft;
        s.nit += 1;
        if (v.gmax <= a.gtol) s.status = 1;
        else if (s.nit >= a.maxiter || s.nfev >= a.maxfun) s.status = 2;
        else if (info != 0) s.status = 5;
        else newdir = true;
    }
    if (newdir) {                             // d = -H^{-1} g: R^T z = g, R s = z (R upper, R^T R = H)
        double b = gl;
        for (int c = 0; c < D; ++c) {
            const double zc = __shfl(b, c) / pv[c];
            if (l == c) b = zc;
            else if (l > c && act) b -= Hs[c * ldh + l] * zc;
        }
        for (int c = D - 1; c >= 0; --c) {
            const double sc_ = __shfl(b, c) / pv[c];
            if (l == c) b = sc_;
            else if (l < c) b -= Hs[l * ldh + c] * sc_;
        }
        dl = act ? -b : 0.0;
        s.t = 1.0;
        s.gd = gb_wave_sum(gl * dl);
        s.nls = 0;
    }
    if (act) {
        a.x[kd + l] = xl;
        a.g[kd + l] = gl;
        if (newdir || a.start) a.d[kd + l] = dl;
        if (newdir) a.Xt[kd + l] = xl + dl;
    }
    if (l == 0) {
        sc[LP_F] = s.f;
        if (newdir || a.start) {
            sc[LP_T] = s.t;
            sc[LP_GD] = s.gd;
        }
        if (a.start) sc[3] = 0.0;
        is[LP_STATUS] = s.status; is[LP_NIT] = s.nit; is[LP_NFEV] = s.nfev; is[LP_NLS] = s.nls;
        if (a.start) { is[4] = 0; is[5] = 0; is[6] = 0; is[7] = 0; }
        if (s.status != 0 && a.stopped) atomicAdd(a.stopped, 1);
    }
}

// ---- host side: what every entry point checks and sets after its model's checks ---------------------------------------------------
// the Hessian entries' own conditions, in their order (the model's "NULL array" comes before, the overlap table and the context after)
static inline int lp_check_hess(const char* fn, const lp_io& o) {
    if (!o.X) return gb_bad(fn, "NULL array");
    if (!o.H && !o.cov) return gb_bad(fn, "give H or cov (or both)");
    if ((o.cov != nullptr) != (o.info != nullptr)) return gb_bad(fn, "info_dev is required with cov and only with it");
    return GSMVI_OK;
}

// the step entries' own conditions
static inline int lp_check_step(const char* fn, const lp_io& o) {
    if (!o.x || !o.g || !o.d || !o.sc || !o.ist || !o.Xt) return gb_bad(fn, "NULL array");
    if (o.maxiter < 1 || o.maxfun < 2) return gb_bad(fn, "maxiter must be at least 1 and maxfun at least 2");
    if (!(o.gtol >= 0.0)) return gb_bad(fn, "gtol must be >= 0");
    return GSMVI_OK;
}

static inline lp_io lp_hess_io(const double* X, double* H, double* cov, int* info_dev) {
    lp_io o = {};
    o.X = X; o.H = H; o.cov = cov; o.info = info_dev;
    return o;
}

static inline lp_io lp_step_io(int start, double* x, double* g, double* d, double* sc, int* ist, double* Xt, int* stopped_dev,
                               int maxiter, int maxfun, double gtol) {
    lp_io o = {};
    o.start = start != 0; o.x = x; o.g = g; o.d = d; o.sc = sc; o.ist = ist; o.Xt = Xt; o.stopped = stopped_dev;
    o.maxiter = maxiter; o.maxfun = maxfun; o.gtol = gtol;
    return o;
}

// the rows every entry's overlap table ends with, after its model's
#define LP_HESS_ROWS 4
#define LP_STEP_ROWS 7
static inline void lp_hess_rows(gb_arr* rows, int64_t K, int D, const lp_io& o) {
    const size_t nx = (size_t)K * D * 8, nh = nx * D;
    const gb_arr own[LP_HESS_ROWS] = {{o.X, nx, "X", GB_RD}, {o.H, nh, "H", GB_WR}, {o.cov, nh, "cov", GB_WR},
                                      {o.info, (size_t)K * 4, "info_dev", GB_WR}};
    for (int i = 0; i < LP_HESS_ROWS; ++i) rows[i] = own[i];
}

static inline void lp_step_rows(gb_arr* rows, int64_t K, int D, const lp_io& o) {
    const size_t nv = (size_t)K * D * 8;
    const gb_arr own[LP_STEP_ROWS] = {{o.x, nv, "x", GB_WR}, {o.g, nv, "g", GB_WR}, {o.d, nv, "d", GB_WR},
                                      {o.sc, (size_t)K * LP_NSC * 8, "sc", GB_WR}, {o.ist, (size_t)K * LP_NIS * 4, "ist", GB_WR},
                                      {o.Xt, nv, "Xt", GB_WR}, {o.stopped, 4, "stopped_dev", GB_WR}};
    for (int i = 0; i < LP_STEP_ROWS; ++i) rows[i] = own[i];
}

// a launch at D: the problems per workgroup, the grid, and the dynamic LDS in bytes of `slot` doubles per problem and `shared`
// doubles per workgroup: at most 56.0 KB in every kernel, below the default limit of 64 KB, so no kernel attribute is needed
static inline size_t lp_slot_launch(long long K, int D, int slot, int shared, int* ppw, unsigned* grid) {
    *ppw = 256 / gb_nt(D);
    *grid = (unsigned)((K + *ppw - 1) / *ppw);
    return ((size_t)shared + (size_t)*ppw * slot) * sizeof(double);
}
