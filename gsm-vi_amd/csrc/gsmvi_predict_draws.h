// The draw-predictive block ("The draw-predictive block"): one copy of what k_softmax_predict_batched
// (gsmvi_softmax_predict_batched.hip), k_negbin_predict_batched (gsmvi_negbin_predict_batched.hip) and k_ordinal_predict_batched
// (gsmvi_ordinal_predict_batched.hip) share around their link steps, and of what their entry points share after their model checks.
// Work mapping: one 256-thread workgroup per (problem k, tile of PD_NB = 16 new rows), k-major: all 16 columns of the fp64 MFMA
// (16 x 16 x 4) carry a row.  The tile's rows of A_k sit in LDS zero-padded (ps_loo_load_rows of gsmvi_psis_loo_tile.h); X_k streams
// through LDS once in tiles of PD_TR = 64 draws (ps_loo_load_draws; the softmax kernel keeps its own class-major tile) with the
// tile's lw_s, and where class probabilities are summed w_s = exp(lw_s), beside it (pd_load_weights).  Wave w takes the 16 draws
// 16 w .. 16 w + 15 of the tile and a lane holds four (draw, row) pairs: row cc, draws kq + 4 r (ps_loo_lane_of, ps_loo_eta).  What
// happens between eta and a lane's four log terms or four class terms is the kernel's: its link step.
// The sum orders.  A log-sum-exp over the draws is a (maximum, scaled sum) pair: the lane's four entries (their maximum, then the sum
// in order), the row's four lanes by a butterfly (xor 16, xor 32), then the tile's pair merged into the pair that lane kq = 0 carries
// from tile to tile (pd_fold); at the end the four waves' pairs in wave order, then max + log(sum) (pd_publish, pd_lse).  pd_merge
// forms no inf - inf: a pair whose maximum is -inf contributes 0.  A class probability is a sum: the lane's four terms in order
// (the kernel's), the butterfly, lane kq = 0 adding to the LDS slot of (wave, class, row), which one thread alone updates tile after
// tile (pd_add_slot); at the end ((q0 + q1) + q2) + q3 over the waves (pd_write_classes).  Every sum is a fixed tree or chain and there
// are no atomics.
// The verdicts are flags, not arithmetic.  The problem's weights are refused when they hold a NaN or +inf, or only -inf
// (pd_weights_bad: two block reductions before the first tile); a draw is flagged from its LOADED values (pd_beta_flag,
// pd_pos_normal), the flag carried by thread s < 64 from tile to tile and reduced once at the end (pd_draws_bad); a row is flagged
// by a non-finite eta at a draw s < S (the kernel's test, reduced in pd_publish, read by pd_row_bad).  A refused problem or row
// is written as NaN.
// The barrier rule: every thread of a workgroup runs the same barriers whatever the verdicts.  The helpers with a barrier in them
// (pd_weights_bad, pd_draws_bad) are called by all of it; the early exit of a tile without a valid row (pd_no_rows, then return) is
// uniform in the workgroup and comes before the first barrier.  pd_publish needs a barrier after it before the outputs are read:
// __syncthreads() or the ones in pd_draws_bad.  A workgroup reads only slice k of the inputs and writes only its own (k, i) entries.
#pragma once
#include "gsmvi_batched.h"
#include "gsmvi_psis_loo_tile.h"    // the lane map, the two tile loaders, the MFMA chain; ps_sum and ps_max of gsmvi_psis_stage.h
#include <cstdint>

#define PD_TR PS_LOO_TR     // draws per tile of X_k: one 16-row MFMA block per wave
#define PD_NB PS_LOO_NB     // new rows per workgroup: the MFMA's 16 columns
#define PD_MAX_S 4096

__host__ __device__ inline int pd_pp(int P) { return (P + 3) & ~3; }       // Pp = 4 ceil(P / 4)

// doubles of the end of a kernel's LDS: the accumulator slots of `classes` classes (0: none), the four waves' pairs of `nout`
// log-sum-exps, their row flags, the 8 words of the block reductions
__host__ __device__ inline int pd_tail_doubles(int classes, int nout) {
    return 4 * PD_NB * classes + 2 * nout * 4 * PD_NB + 4 * PD_NB + 8;
}

// ---- device side ----------------------------------------------------------------------------------------------------------------
struct pd_tail {
    double* pac;                // 4 x classes x PD_NB   the accumulator slots: (wave, class, row)
    double* pm;                 // nout x 4 x PD_NB      the waves' pairs: maxima (output, wave, row)
    double* psum;               // nout x 4 x PD_NB                       scaled sums
    int* pbad;                  // 4 x PD_NB             row flags (in 4 x PD_NB doubles)
    double* red;                // 8                     the block reductions
};

__device__ __forceinline__ pd_tail pd_carve_tail(double* at, int classes, int nout) {
    double* pm = at + 4 * PD_NB * classes;
    double* psum = pm + nout * 4 * PD_NB;
    return {at, pm, psum, reinterpret_cast<int*>(psum + nout * 4 * PD_NB), psum + nout * 4 * PD_NB + 4 * PD_NB};
}

// where the workgroup stands: ps_loo_pos with tiles of PD_NB rows (kn = k M + the tile's first row)
__device__ __forceinline__ ps_loo_pos pd_pos_of(unsigned ntile, long long M, int S) {
    ps_loo_pos p;
    p.k = blockIdx.x / ntile;
    p.i0 = (long long)(blockIdx.x - (unsigned)p.k * ntile) * PD_NB;
    p.ni = (int)(M - p.i0 < PD_NB ? M - p.i0 : PD_NB);
    p.ks = p.k * (size_t)S;
    p.kn = p.k * (size_t)M + (size_t)p.i0;
    return p;
}

// nv: the tile's valid rows are its first nv; counts[k] clamped to 0 .. M (null: M)
__device__ __forceinline__ int pd_valid(const int* counts, long long M, const ps_loo_pos p) {
    long long nk = M;
    if (counts) {
        const long long c = counts[p.k];
        nk = c < 0 ? 0 : (c > M ? M : c);
    }
    return ps_loo_valid(nk, p);
}

// a tile without a valid row: NaN to its ni rows of `out` (`width` entries each) and of lpd (or null); nothing is loaded
__device__ __forceinline__ void pd_no_rows(double* out, int width, double* lpd, const ps_loo_pos p, int l) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (int e = l; e < p.ni * width; e += 256) out[p.kn * width + e] = qnan;
    if (lpd && l < p.ni) lpd[p.kn + l] = qnan;
}

// the problem's weights (called by the whole workgroup): a NaN or +inf, or nothing but -inf, refuses every row; null: uniform
__device__ __forceinline__ bool pd_weights_bad(const double* lw, size_t ks, int S, double* red, int l) {
    if (!lw) return false;
    const double inf = __builtin_huge_val();
    double nb = 0.0, vmax = -inf;
    for (int s = l; s < S; s += 256) {
        const double v = lw[ks + s];
        if (!(v < inf)) nb += 1.0;            // NaN or +inf
        vmax = fmax(vmax, v);
    }
    nb = ps_sum(nb, red, l);
    vmax = ps_max(vmax, red, l);
    return nb > 0.0 || vmax == -inf;
}

// thread l < 64: lw_s of draw t0 + l into lws (null lw: the uniform lwu = -log S; past S: -inf) and, with wts, w_s = exp(lw_s)
// (uniform: wu = 1 / S; past S: 0)
__device__ __forceinline__ void pd_load_weights(double* lws, double* wts, const double* lw, size_t ks, int t0, int S, double lwu,
                                                double wu, int l) {
    if (l < PD_TR) {
        const double v = t0 + l < S ? (lw ? lw[ks + t0 + l] : lwu) : -__builtin_huge_val();
        lws[l] = v;
        if (wts) wts[l] = t0 + l < S ? (lw ? exp(v) : wu) : 0.0;
    }
}

// the draw flag's two tests, on loaded values: 0 x beta_sj summed over the draw's row of the operand tile (0.0, or NaN for a
// non-finite beta_sj); a positive normal number
__device__ __forceinline__ double pd_beta_flag(const double* xr, int P) {
    double z = 0.0;
    for (int j = 0; j < P; ++j) z += xr[j] * 0.0;
    return z;
}
__device__ __forceinline__ bool pd_pos_normal(double w) { return w >= 2.2250738585072014e-308 && w < __builtin_huge_val(); }

// the problem's draw flag (called by the whole workgroup; its barriers publish what pd_publish stored): nflag, the thread's count
// of flagged draws (or 1.0 for any), is positive in some thread
__device__ __forceinline__ bool pd_draws_bad(double nflag, double* red, int l) { return ps_sum(nflag, red, l) > 0.0; }

// (m1, s1) + (m2, s2) of two log-sum-exp pairs, into the first: (M, s1 e^(m1 - M) + s2 e^(m2 - M)) with M the larger maximum, whose
// own factor e^0 is exactly 1 and is not computed; a pair whose maximum is -inf contributes 0 (two of them: no inf - inf is formed)
__device__ __forceinline__ void pd_merge(double& m1, double& s1, double m2, double s2) {
    const double mm = fmax(m1, m2);
    const double e = mm == -__builtin_huge_val() ? 0.0 : exp(fmin(m1, m2) - mm);
    s1 = m1 >= m2 ? s1 + s2 * e : s1 * e + s2;
    m1 = mm;
}

// the pair of a lane's four entries (-inf: left out), then of the row's four lanes, merged into the pair (lm, ls) carried from tile
// to tile
__device__ __forceinline__ void pd_fold(double& lm, double& ls, const double (&t)[4], bool live) {
    const double inf = __builtin_huge_val();
    double tm = -inf, ts = 0.0;
    if (live) {
#pragma unroll
        for (int r = 0; r < 4; ++r) tm = fmax(tm, t[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) ts += tm == -inf ? 0.0 : exp(t[r] - tm);
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const double om = __shfl_xor(tm, o), os = __shfl_xor(ts, o);
        pd_merge(tm, ts, om, os);
    }
    pd_merge(lm, ls, tm, ts);                 // (used from lane kq = 0 alone)
}

// after the last tile: a row's flag over its four lanes, then lane kq = 0 stores its wave's NOUT pairs and the flag
template <int NOUT>
__device__ __forceinline__ void pd_publish(const pd_tail sm, const double (&lm)[NOUT], const double (&ls)[NOUT], bool rbad,
                                           const ps_loo_lane ln) {
    int fl = rbad ? 1 : 0;
    fl |= __shfl_xor(fl, 16);
    fl |= __shfl_xor(fl, 32);
    if (ln.kq == 0) {
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            sm.pm[(o * 4 + ln.wv) * PD_NB + ln.cc] = lm[o];
            sm.psum[(o * 4 + ln.wv) * PD_NB + ln.cc] = ls[o];
        }
        sm.pbad[ln.wv * PD_NB + ln.cc] = fl;
    }
}

// row r's flag: its four waves
__device__ __forceinline__ bool pd_row_bad(const int* pbad, int r) {
    return (pbad[r] | pbad[PD_NB + r] | pbad[2 * PD_NB + r] | pbad[3 * PD_NB + r]) != 0;
}

// log-sum-exp o of row r: the four waves' pairs in wave order
__device__ __forceinline__ double pd_lse(const pd_tail sm, int o, int r) {
    const double* qm = sm.pm + o * 4 * PD_NB + r;
    const double* qs = sm.psum + o * 4 * PD_NB + r;
    double mm = qm[0], ss = qs[0];
    for (int w = 1; w < 4; ++w) pd_merge(mm, ss, qm[w * PD_NB], qs[w * PD_NB]);
    return mm + log(ss);
}

// ---- the class accumulators of the softmax and ordinal kernels ------------------------------------------------------------------
__device__ __forceinline__ void pd_zero_slots(double* pac, int C, int l) {
    for (int e = l; e < 4 * PD_NB * C; e += 256) pac[e] = 0.0;
}

// v: the lane's four terms of class c in order; the row's four lanes, then lane kq = 0 adds the sum to its slot
__device__ __forceinline__ void pd_add_slot(double* pac, int C, int c, double v, bool live, const ps_loo_lane ln) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (live && ln.kq == 0) pac[(ln.wv * C + c) * PD_NB + ln.cc] += v;
}

// the tile's outputs, the waves in order: prob (K, M, C); lpd (K, M) or null, NaN also for a label outside 0 .. C - 1 (ys: the
// tile's labels as given: compared, never used as an index).  kbad: the problem is refused
__device__ __forceinline__ void pd_write_classes(double* prob, double* lpd, const pd_tail sm, const int* ys, int C, int nv, bool kbad,
                                                 const ps_loo_pos p, int l) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (int e = l; e < p.ni * C; e += 256) {
        const int r = e / C, c = e - r * C;
        const bool bad = r >= nv || kbad || pd_row_bad(sm.pbad, r);
        const double* q = sm.pac + c * PD_NB + r;
        prob[p.kn * C + e] = bad ? qnan : ((q[0] + q[C * PD_NB]) + q[2 * C * PD_NB]) + q[3 * C * PD_NB];
    }
    if (lpd && l < p.ni) {
        const int yv = ys[l];
        const bool bad = l >= nv || kbad || yv < 0 || yv > C - 1 || pd_row_bad(sm.pbad, l);
        const double v = pd_lse(sm, 0, l);
        lpd[p.kn + l] = bad ? qnan : v;
    }
}

// ---- host side: what every entry point checks and sets after its model's checks -------------------------------------------------
struct pd_launch {
    unsigned ntile;             // tiles per problem: ceil(M / 16)
    unsigned grid;              // K ntile
};

// In this order: S; "K M" (`width`: a bound on the doubles of a row of A and of the output, so that K M width doubles are
// addressable); the tiles; a null among the required arrays (`null_array`); y (or the labels) and lpd given together (`pair` names
// them in the message).  The order is the ordinal entry's; the softmax and negbin entries looked at the arrays before "K M", so of
// two bad arguments at once they may now name the other one.  A single bad argument gives every entry the message it always gave.
static inline int pd_plan(const char* fn, int64_t K, int64_t M, int64_t S, int width, bool null_array, const void* y, const void* lpd,
                          const char* pair, pd_launch* p) {
    if (S < 1 || S > PD_MAX_S) return gb_bad(fn, "S must be in [1, 4096]");
    if (M > (INT64_MAX / 8 / width) / K) return gb_bad(fn, "K M is too large");
    const int64_t ntile = (M + PD_NB - 1) / PD_NB;
    if (ntile > 16777215 / K) return gb_bad(fn, "K ceil(M / 16) must be at most 2^24 - 1 (one tile of 16 rows per workgroup)");
    if (null_array) return gb_bad(fn, "NULL array");
    if ((y != nullptr) != (lpd != nullptr)) return gb_bad(fn, pair);
    p->ntile = (unsigned)ntile;
    p->grid = (unsigned)(K * ntile);
    return GSMVI_OK;
}
