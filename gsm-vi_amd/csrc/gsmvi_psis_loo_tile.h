// The tile block of the PSIS leave-one-out kernels ("The leave-one-out tile block"): one copy of what
// k_psis_loo_batched<FAM, SHARED> (gsmvi_psis_loo_batched.hip), k_psis_loo_softmax_batched (gsmvi_psis_loo_softmax_batched.hip),
// k_psis_loo_negbin_batched (gsmvi_psis_loo_negbin_batched.hip) and k_psis_loo_ordinal_batched (gsmvi_psis_loo_ordinal_batched.hip)
// share around their link steps, and of what their entry points share around their model checks.
// Work mapping: one 256-thread workgroup per (problem k, tile of NI consecutive observations), k-major.
//   (1) the kernel's own: l_si of the tile (NI x S doubles) into LDS.  The NI rows of A sit in LDS zero-padded to PS_LOO_NB = 16 rows
//       (ps_loo_load_rows); X_k streams through LDS once in tiles of PS_LOO_TR = 64 draws, zero-padded the same way
//       (ps_loo_load_draws); wave w takes the 16 draws 16 w .. 16 w + 15 of the tile on the fp64 MFMA (16 x 16 x 4, ps_loo_lane_of,
//       ps_loo_eta); what happens to eta is the kernel's.
//   (2) per observation of the tile: ps_loo_stage below: rho_s = logr_s - l_si into the PSIS stage's array, ps_stage
//       (gsmvi_psis_stage.h), then the two log-sum-exps -- elpd from the stage's weights, lpd from the problem-level weights lw.
// The tiles of (1) lie over the stage's LDS (they are dead before the first stage starts: the kernel's barrier between (1) and (2)).
// NI is the largest count, at most the kernel's cap, whose l_si fit beside that region in GB_LDS_MAX.  Every sum is a fixed tree or
// chain and there are no atomics.  Every thread of a workgroup runs the same barriers whatever the verdicts: whether a row of the
// tile is valid is uniform in the workgroup, and the helpers with a barrier in them (ps_loo_stage) are called by all of it.  A
// workgroup reads only slice k of the per-problem inputs and writes only its own (k, i) entries.  Inputs are only read; no context
// workspace.
#pragma once
#include "gsmvi_common.h"    // v4d, GSMVI_MFMA_F64
#include "gsmvi_psis_stage.h"
#include <cstdint>
#include <cstdio>

#define PS_LOO_TR 64    // draws per tile of X_k: one 16-row MFMA block per wave
#define PS_LOO_NB 16    // rows of the A_k tile: the MFMA's 16 columns, NI of them in use
// observations per workgroup at most (fewer observations, more workgroups per CU); a diagnostic build changes the cap
// of one kernel, 1 <= n <= 16, with -DPL_NI_CAP=n (k_psis_loo_batched, both forms), -DPLS_NI_CAP=n (k_psis_loo_softmax_batched),
// -DPLN_NI_CAP=n (k_psis_loo_negbin_batched) or -DPLO_NI_CAP=n (k_psis_loo_ordinal_batched)
#ifndef PL_NI_CAP
#define PL_NI_CAP 4
#endif
#ifndef PLS_NI_CAP
#define PLS_NI_CAP 4
#endif
#ifndef PLN_NI_CAP
#define PLN_NI_CAP 4
#endif
#ifndef PLO_NI_CAP
#define PLO_NI_CAP 4
#endif
static_assert(PLN_NI_CAP >= 1 && PLN_NI_CAP <= PS_LOO_NB, "the tile's observations are columns of one 16-column MFMA block");
static_assert(PLO_NI_CAP >= 1 && PLO_NI_CAP <= PS_LOO_NB, "the tile's observations are columns of one 16-column MFMA block");

// doubles of the region the stage shares with a kernel's `tiles` doubles of MFMA tiles: the stage's arrays and its S2 indices, or
// the tiles, whichever is larger
__host__ __device__ inline int ps_loo_region_doubles(int tiles, int S, int S2) {
    const int stage = ps_lds_doubles(S, S2) + S2 / 2;
    return stage > tiles ? stage : tiles;
}

// NI: the largest count, at most `cap`, whose l_si (NI x S doubles) fit beside the region in GB_LDS_MAX (>= 2 at S = 4096)
static inline int ps_loo_tile(int tiles, int S, int cap) {
    int S2, M;
    ps_sizes(S, &S2, &M);
    const int fit = (GB_LDS_MAX / 8 - ps_loo_region_doubles(tiles, S, S2)) / S;
    return fit < cap ? fit : cap;
}

// what stage (2) reads and writes beside the l_si
struct ps_loo_io {
    const double* logr;         // (K, S) lp - log q of the problem-level run
    const double* lw;           // (K, S) its normalised smoothed log weights
    double* loglik;             // (K, N, S) or null
    double* elpd;               // (K, N) each
    double* lpd;
    double* khat;
    double* ess;
    int* info;                  // (K, N) 0; -1 non-finite ratios; -2 tail too short; -3 not a valid row
};

// the part of every kernel's argument block that is not its model: filled by ps_loo_plan
struct ps_loo_args {
    int S, S2, M;               // draws, draws padded to a power of two, the tail size before ties
    int NI, U;                  // observations per tile; doubles of the region the stage and the MFMA tiles share
    unsigned ntile;             // tiles per problem: ceil(N / NI)
    const double* X;            // (K, S, D) the draws of q_k
    ps_loo_io o;                // the ratios and weights of the problem-level run, the outputs
};

// ---- device side: where a workgroup stands, its LDS, the two tile loaders, the lane map and the MFMA chain ---------------------
struct ps_loo_pos {
    size_t k;                   // the problem
    long long i0;               // the tile's first observation
    int ni;                     // its observations: NI, fewer in a problem's last tile
    size_t ks, kn;              // k S; k N + i0
};

__device__ __forceinline__ ps_loo_pos ps_loo_pos_of(const ps_loo_args c, long long N) {
    ps_loo_pos p;
    p.k = blockIdx.x / c.ntile;
    p.i0 = (long long)(blockIdx.x - (unsigned)p.k * c.ntile) * c.NI;
    p.ni = (int)(N - p.i0 < c.NI ? N - p.i0 : c.NI);
    p.ks = p.k * (size_t)c.S;
    p.kn = p.k * (size_t)N + (size_t)p.i0;
    return p;
}

// nv: with nk rows of the problem that count (clamped to 0 .. N), the tile's valid observations are its first nv
__device__ __forceinline__ int ps_loo_valid(long long nk, const ps_loo_pos p) {
    return (int)(nk - p.i0 < 0 ? 0 : (nk - p.i0 < p.ni ? nk - p.i0 : p.ni));
}

struct ps_loo_lds {
    ps_lds sm;                  // the stage's arrays, the S2 indices behind them
    double* tiles;              // the kernel's own use of the region, over the stage's arrays
    double* ell;                // NI x S        l_si of the tile
};

__device__ __forceinline__ ps_loo_lds ps_loo_carve(const ps_loo_args c) {
    extern __shared__ double ps_loo_sm[];
    return {ps_carve(ps_loo_sm, reinterpret_cast<int*>(ps_loo_sm + ps_lds_doubles(c.S, c.S2)), c.S, c.S2), ps_loo_sm, ps_loo_sm + c.U};
}

// PS_LOO_NB rows of stride ld at dst from the rows of stride src_ld at src; 0.0 past `rows` and past `cols` (ld - cols >= 1)
__device__ __forceinline__ void ps_loo_load_rows(double* dst, int ld, const double* src, int src_ld, int rows, int cols, int l) {
    for (int e = l; e < PS_LOO_NB * ld; e += 256) {
        const int r = e / ld, j = e - r * ld;
        dst[e] = r < rows && j < cols ? src[(size_t)r * src_ld + j] : 0.0;
    }
}

// PS_LOO_TR rows of stride ld at dst: the first `cols` entries of the draws t0 .. t0 + 63 of Xk (row stride src_ld); 0.0 past draw
// S - 1 and past `cols`
__device__ __forceinline__ void ps_loo_load_draws(double* dst, int ld, const double* Xk, int src_ld, int cols, int t0, int S, int l) {
    for (int e = l; e < PS_LOO_TR * ld; e += 256) {
        const int r = e / ld, j = e - r * ld;
        dst[e] = t0 + r < S && j < cols ? Xk[(size_t)(t0 + r) * src_ld + j] : 0.0;
    }
}

// Thread l in the MFMA's layout: wave wv takes the draws 16 wv .. 16 wv + 15 of a tile (it has work iff t0 + 16 wv < S, which is
// wave-uniform); the lane feeds row cc of both operand tiles at the k positions 4 j + kq; its accumulator entry r is the pair
// (draw ps_loo_draw(t0, ln, r), observation cc).
struct ps_loo_lane {
    int wv, cc, kq;
};
__device__ __forceinline__ ps_loo_lane ps_loo_lane_of(int l) { return {l >> 6, l & 15, (l & 63) >> 4}; }
__device__ __forceinline__ int ps_loo_draw(int t0, const ps_loo_lane ln, int r) { return t0 + 16 * ln.wv + ln.kq + 4 * r; }

// eta of the lane's four pairs: the A operand x_{s, 4 j + kq} from the draw tile Xs, the B operand a_{i, 4 j + kq} from the row tile
// As, both of row stride ld, kp / 4 steps
__device__ __forceinline__ v4d ps_loo_eta(const double* Xs, const double* As, int ld, int kp, const ps_loo_lane ln) {
    const double* pa = Xs + (16 * ln.wv + ln.cc) * ld + ln.kq;
    const double* pb = As + ln.cc * ld + ln.kq;
    v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < kp; j += 4) acc = GSMVI_MFMA_F64(pa[j], pb[j], acc);
    return acc;
}

// Stage (2), per observation i < ni of the tile: rho_s = logr_s - l_si into the stage's array, ps_stage, then the two
// log-sum-exps -- the maximum by a block reduction, then the sum of exp(. - max) -- elpd from the stage's weights, lpd from the
// problem-level weights lw.  ell: the tile's l_si in LDS (NI x S, published by a barrier before the call); ks = k S, kn = k N + the
// tile's first observation.  w: null -- the first nv rows of the tile are the valid ones -- or the observation weights of the
// tile's ni rows (k_psis_loo_batched<FAM, true>; nv is then not used): row i is valid iff w_i > 0 (not for 0 or NaN), and leaving it
// out removes its whole weighted term, rho_s = logr_s - w_i l_si (w_i = 1: the product is exact, the same bits as without w).
__device__ __forceinline__ void ps_loo_stage(const ps_loo_io a, const ps_lds sm, const double* ell, int ni, int nv, const double* w,
                                             size_t ks, size_t kn, int S, int S2, int M, int l) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL), inf = __builtin_huge_val();
    for (int i = 0; i < ni; ++i) {
        const size_t ki = kn + i;
        double* lk = a.loglik ? a.loglik + ki * S : nullptr;
        const double wi = w ? w[i] : 1.0;
        if (w ? !(wi > 0.0) : i >= nv) {      // not a valid row (uniform in the workgroup: no barrier is skipped by a part of it)
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
            sm.val[s] = w ? a.logr[ks + s] - wi * e : a.logr[ks + s] - e;
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

// ---- host side: what every entry point checks and sets after its model's checks -------------------------------------------------
struct ps_loo_launch {
    ps_loo_args c;
    size_t lds;                 // dynamic LDS in bytes: <= GB_LDS_MAX by the choice of NI
    unsigned grid;              // K ntile
};

// In this order: S; a null among the required arrays (`model_null`: among the model's own); "K N S"; with P > 0 the softmax and
// negbin entries' "K N P" (the GLM entries' model check has bounded K N D); NI and the tiles per problem, whose message names the
// entry's `tile_fn`.  `tiles`: the doubles of the kernel's own use of the shared region; `cap`: its *_NI_CAP.
static inline int ps_loo_plan(const char* fn, int64_t K, int64_t N, int64_t S, int P, bool model_null, const double* X,
                              const ps_loo_io& o, int tiles, int cap, const char* tile_fn, ps_loo_launch* p) {
    if (S < PS_MIN_S || S > PS_MAX_S) return gb_bad(fn, "S must be in [5, 4096]");
    if (model_null || !X || !o.logr || !o.lw || !o.elpd || !o.lpd || !o.khat || !o.ess || !o.info) return gb_bad(fn, "NULL array");
    if (N > (INT64_MAX / 8 / S) / K) return gb_bad(fn, "K N S is too large");
    if (P > 0 && N > (INT64_MAX / 8 / P) / K) return gb_bad(fn, "K N P is too large");
    ps_loo_args& c = p->c;
    c.S = (int)S;
    ps_sizes(c.S, &c.S2, &c.M);
    c.NI = ps_loo_tile(tiles, c.S, cap);
    const int64_t ntile = (N + c.NI - 1) / c.NI;
    if (ntile > 16777215 / K) {
        char msg[128];
        snprintf(msg, sizeof msg, "K ceil(N / %s) must be at most 2^24 - 1 (one tile per workgroup)", tile_fn);
        return gb_bad(fn, msg);
    }
    c.U = ps_loo_region_doubles(tiles, c.S, c.S2);
    c.ntile = (unsigned)ntile;
    c.X = X;
    c.o = o;
    p->lds = ((size_t)c.U + (size_t)c.NI * c.S) * sizeof(double);
    p->grid = (unsigned)(K * ntile);
    return GSMVI_OK;
}

// the rows every entry's overlap table ends with, after its model's: X (K, S, D), the problem-level run's, the outputs
#define PS_LOO_ROWS 9
static inline void ps_loo_overlap_rows(gb_arr* rows, int64_t K, int64_t N, int D, const ps_loo_args& c) {
    const size_t nn = (size_t)K * N * 8, ns = (size_t)K * c.S * 8;
    const gb_arr own[PS_LOO_ROWS] = {{c.X, ns * D, "X", GB_RD},          {c.o.logr, ns, "logr", GB_RD},
                                     {c.o.lw, ns, "lw", GB_RD},          {c.o.loglik, nn * c.S, "loglik", GB_WR},
                                     {c.o.elpd, nn, "elpd", GB_WR},      {c.o.lpd, nn, "lpd", GB_WR},
                                     {c.o.khat, nn, "khat", GB_WR},      {c.o.ess, nn, "ess", GB_WR},
                                     {c.o.info, (size_t)K * N * 4, "info", GB_WR}};
    for (int i = 0; i < PS_LOO_ROWS; ++i) rows[i] = own[i];
}
