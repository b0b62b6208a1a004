// Batched ordinal PSIS leave-one-out: for K fitted Gaussians q_k over (beta, delta) of K cumulative-logit (proportional odds)
// regressions of one (N, P, C), D = P + C - 1 <= 64, the pointwise leave-one-out log predictive density of every observation from S
// draws of q_k, one launch ("Batched ordinal PSIS-LOO"; the definition is in include/gsmvi_hip.h, above
// gsmvi_psis_loo_ordinal_batched_f64).  The reference has no twin.
//   k_psis_loo_ordinal_batched      (the sibling of k_psis_loo_negbin_batched: a draw carries C - 1 cutpoint parameters behind beta)
// The work mapping, the LDS, the loaders, the MFMA chain and stage (2) are the tile block's (gsmvi_psis_loo_tile.h), with
// NI = gsmvi_psis_loo_ordinal_tile(P, C, S) and the first nv rows of a tile valid (counts, clamped to 0 .. N).
//   (1) l_si of the tile, per tile of PS_LOO_TR = 64 draws, in three steps between barriers:
//       (a) the tile of X_k into LDS: 64 rows of Pp = 4 ceil(P / 4) columns (row stride Pp + 1).  Only the columns j < P of a draw
//           are copied; the C - 1 delta columns never enter the operand, and every padded position (j >= P, rows past S) holds
//           0.0.  The NI rows of A_k sit beside it zero-padded to 16 rows of the same Pp columns, loaded once.  The deltas go
//           from X_k straight into the per-draw table T (64 rows of C - 1, row stride (C - 1) | 1), entry e = l, l + 256, ... of
//           the tile's 64 (C - 1): delta_0 as it is, w_j = e^{delta_j} for j >= 1 -- the exponentials of a draw are spread over
//           the whole workgroup (at C = 64 each thread takes about sixteen of the 64 x 62).
//       (b) eta = X_tile A_tile^T, Pp / 4 steps; a lane whose column is a valid observation leaves eta_si in the cell of l_si.
//           Meanwhile thread s < 64 walks row s of T once: the flag -- from the LOADED values: a non-finite beta_sj or delta_0
//           (0 x value summed), or a w_j, j >= 1, that is not a positive normal number (which a non-finite delta_j gives too),
//           whatever the labels of the tile: the score kernel's row flag; not from the product, in which delta does not take
//           part -- and the cutpoints cut_0 = delta_0, cut_j = cut_{j-1} + w_j as one chain in ascending j (k_ordinal_batched's
//           prologue: the same bits), each written over the w_j it has just consumed: ONE table, which keeps the kernel's use of
//           the shared region at or below 5736 doubles, so that two workgroups fit a CU at S = 1024 for every (P, C) as they do
//           for the negative binomial sibling (with w and the cutpoints side by side, 8808 doubles at C = 64, only one fits,
//           and stage (2), which lives on latency hiding, takes twice as long).
//       (c) the link, re-mapped so that every lane works: entry e = l, l + 256, ... of the tile's nv x 64 (observation, draw)
//           pairs -- one per thread at NI <= 4 -- reads eta_si + o_i, forms the gap of an interior label again as w_{y_i} =
//           e^{delta_{y_i}} from X_k (the same exp of the same double as in (a): the same bits; the row is in cache) and takes
//           its gap term from ord_gap of it (only the pairs of the tile are evaluated: at most NI classes per draw, not C - 2),
//           runs ord_link<false, true> (gsmvi_ordinal_link.h, unchanged: t is bit for bit the score launch's at the same eta and
//           cutpoints) and stores l_si = t, or NaN for a flagged draw.  No constant is added: the probability is normalised.
//       The labels, clamped to 0 .. C - 1, and o_i go into LDS once per workgroup.  Strides: the rows of T are read by 64 lanes
//       at one column each, in (b) and in (c), so their stride is odd.
#include "gsmvi_common.h"
#include "gsmvi_ctx.h"
#include "gsmvi_batched.h"
#include "gsmvi_ordinal_link.h"
#include "gsmvi_psis_loo_tile.h"
#include "../../include/gsmvi_hip.h"
#include <cmath>
#include <cstdint>

struct plo_args {
    long long N;
    int P, C;                   // columns of A, classes (D = P + C - 1)
    const double* A;            // (K, N, P)
    const int* y;               // (K, N) labels
    const double* offset;       // (K, N) added to eta, or null
    const int* counts;          // (K) valid rows, clamped to 0 .. N (null: N)
    ps_loo_args c;              // (X (K, S, P + C - 1): beta, then delta)
};

__host__ __device__ inline int plo_pp(int P) { return (P + 3) & ~3; }
__host__ __device__ inline int plo_ldc(int C) { return (C - 1) | 1; }

// doubles of the kernel's own use of the shared region: the X tile and the A tile (80 rows of Pp + 1), the table of w, then of the
// cutpoints (64 rows of (C - 1) | 1), the 16 offsets, the 16 labels (8 doubles), the 64 draw flags and one cell per thread for
// the gap term.  The most is 5736, at (P, C) = (61, 4) and (62, 3)
static inline int plo_tiles_doubles(int P, int C) {
    return (PS_LOO_TR + PS_LOO_NB) * (plo_pp(P) + 1) + PS_LOO_TR * plo_ldc(C) + PS_LOO_NB + PS_LOO_NB / 2 + PS_LOO_TR + 256;
}

__global__ __launch_bounds__(256) void k_psis_loo_ordinal_batched(plo_args a) {
    const int l = threadIdx.x, S = a.c.S;
    const int P = a.P, C = a.C, lc = C - 1, D = P + lc, Pp = plo_pp(P), lda = Pp + 1, ldc = plo_ldc(C);
    const ps_loo_pos p = ps_loo_pos_of(a.c, a.N);
    long long nk = a.N;                       // the rows that count
    if (a.counts) {
        const long long c = a.counts[p.k];
        nk = c < 0 ? 0 : (c > a.N ? a.N : c);
    }
    const int nv = ps_loo_valid(nk, p);
    const ps_loo_lds lds = ps_loo_carve(a.c);
    double* Xs = lds.tiles;                   // 64 x lda      the beta part of a tile of draws   (over the stage's arrays)
    double* As = Xs + PS_LOO_TR * lda;        // 16 x lda      the tile's rows of A_k, zero-padded
    double* Ct = As + PS_LOO_NB * lda;        // 64 x ldc      delta_0 and w_j = e^{delta_j} of the tile's draws, then their cutpoints
    double* os = Ct + PS_LOO_TR * ldc;        // 16            offset_i
    int* ys = reinterpret_cast<int*>(os + PS_LOO_NB);           // 16 labels, clamped to 0 .. C - 1 (in 8 doubles)
    double* fs = os + PS_LOO_NB + PS_LOO_NB / 2;                // 64            1.0 or 0.0 (a flagged draw)
    double* gs = fs + PS_LOO_TR;              // 256           the gap term of the thread's pair
    double* ell = lds.ell;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    // ---- (1) l_si of the tile's valid observations ------------------------------------------------------------------------
    if (nv > 0) {                             // (uniform in the workgroup)
        ps_loo_load_rows(As, lda, a.A + p.kn * P, P, nv, P, l);
        if (l < PS_LOO_NB) {
            const int yv = l < nv ? a.y[p.kn + l] : 0;
            ys[l] = yv < 0 ? 0 : (yv > lc ? lc : yv);
            os[l] = a.offset && l < nv ? a.offset[p.kn + l] : 0.0;
        }
        const double* Xk = a.c.X + p.ks * D;
        const ps_loo_lane ln = ps_loo_lane_of(l);
        for (int t0 = 0; t0 < S; t0 += PS_LOO_TR) {
            __syncthreads();                  // the previous tile's readers are done
            ps_loo_load_draws(Xs, lda, Xk, D, P, t0, S, l);                        // (a)
            for (int e = l; e < PS_LOO_TR * lc; e += 256) {
                const int r = e / lc, j = e - r * lc;
                const double d = t0 + r < S ? Xk[(size_t)(t0 + r) * D + P + j] : 0.0;
                Ct[r * ldc + j] = j == 0 ? d : exp(d);                             // (a NaN delta gives a NaN w: flagged)
            }
            __syncthreads();
            if (l < PS_LOO_TR) {                                                   // (b) the per-draw values ...
                const double* xr = Xs + l * lda;
                double* cr = Ct + l * ldc;
                double z = 0.0;
                for (int j = 0; j < P; ++j) z += xr[j] * 0.0;                      // (NaN for a non-finite beta_sj)
                double cut = cr[0];
                z += cut * 0.0;
                bool okw = true;
                for (int j = 1; j < lc; ++j) {
                    const double w = cr[j];
                    okw = okw && w >= 2.2250738585072014e-308 && w < __builtin_huge_val();
                    cut += w;
                    cr[j] = cut;                                                   // (over the w_j just read)
                }
                fs[l] = okw && z == 0.0 ? 1.0 : 0.0;
            }
            if (t0 + 16 * ln.wv < S) {        // ... and eta (wave-uniform)
                const v4d acc = ps_loo_eta(Xs, As, lda, Pp, ln);
                if (ln.cc < nv) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int s = ps_loo_draw(t0, ln, r);
                        if (s < S) ell[ln.cc * S + s] = acc[r];
                    }
                }
            }
            __syncthreads();
            for (int e = l; e < nv * PS_LOO_TR; e += 256) {                        // (c)
                const int i = e >> 6, q = e & 63, s = t0 + q;
                if (s < S) {
                    const int yv = ys[i];
                    double lm = 0.0, qe = 0.0;
                    if (yv >= 1 && yv <= C - 2) ord_gap(exp(Xk[(size_t)s * D + P + yv]), lm, qe);       // w of (a), again
                    gs[l] = lm;               // the link reads lm[y]: the thread's own cell stands at index y of its table
                    double re = 0.0, ulo = 0.0, uhi = 0.0, t = 0.0;
                    ord_link<false, true>(ell[i * S + s] + os[i], yv, C, Ct + q * ldc, gs + l - yv, nullptr, re, ulo, uhi, t);
                    ell[i * S + s] = fs[q] != 0.0 ? t : qnan;
                }
            }
        }
    }
    __syncthreads();                          // l_si is published; the tiles are dead, the stage may take their place

    ps_loo_stage(a.c.o, lds.sm, ell, p.ni, nv, nullptr, p.ks, p.kn, S, a.c.S2, a.c.M, l);     // (2)
}

hipError_t gsmvi_psis_loo_ordinal_batched_prepare() { return gb_allow_lds(k_psis_loo_ordinal_batched); }

extern "C" {

int gsmvi_psis_loo_ordinal_tile(int P, int C, int64_t S) {
    if (C < 2 || C > GB_MAX_D || P < 1 || P > GB_MAX_D - (C - 1) || S < PS_MIN_S || S > PS_MAX_S) return 0;
    return ps_loo_tile(plo_tiles_doubles(P, C), (int)S, PLO_NI_CAP);
}

int gsmvi_psis_loo_ordinal_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int C, int64_t N, int64_t S, const double* A,
                                       const int* y, const double* offset, const int* counts_dev, const double* X,
                                       const double* logr, const double* lw, double* loglik, double* elpd, double* lpd,
                                       double* khat, double* ess, int* info) {
    GB_BAD(C < 2 || C > GB_MAX_D, "C must be in [2, 64]");
    GB_BAD(P < 1 || P > GB_MAX_D - (C - 1), "P must be in [1, 65 - C] (D = P + C - 1 <= 64)");
    GB_BAD(K < 1 || K > 16777215, "K must be in [1, 2^24 - 1]");
    GB_BAD(N < 1, "N must be at least 1");
    ps_loo_launch p = {};
    if (int st = ps_loo_plan(__func__, K, N, S, P, !A || !y, X, {logr, lw, loglik, elpd, lpd, khat, ess, info},
                             plo_tiles_doubles(P, C), PLO_NI_CAP, "gsmvi_psis_loo_ordinal_tile(P, C, S)", &p))
        return st;
    const size_t nn = (size_t)K * N;
    gb_arr all[4 + PS_LOO_ROWS] = {{A, nn * P * 8, "A", GB_RD},
                                   {y, nn * 4, "y", GB_RD},
                                   {offset, nn * 8, "offset", GB_RD},
                                   {counts_dev, (size_t)K * 4, "counts_dev", GB_RD}};
    ps_loo_overlap_rows(all + 4, K, N, P + C - 1, p.c);
    if (int st = gb_check_overlaps(__func__, all, all + 4 + PS_LOO_ROWS)) return st;
    GB_BAD(!ctx, "ctx is NULL");
    const plo_args a = {N, P, C, A, y, offset, counts_dev, p.c};
    hipLaunchKernelGGL(k_psis_loo_ordinal_batched, dim3(p.grid), dim3(256), p.lds, reinterpret_cast<hipStream_t>(stream), a);
    return gb_launched(ctx, GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_TARGET, "k_psis_loo_ordinal_batched");
}

}  // extern "C"
