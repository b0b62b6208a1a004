// The row stage of the two GLM predictive kernels: from v of a tile's rows to their eta_mean, eta_var,
// pmean and lpd.  One copy for k_glm_predict_batched (gsmvi_glm_predict_batched.hip: a design per problem, rows n < n_k) and
// k_glm_shared_predict_batched (gsmvi_glm_shared_predict_batched.hip: one design, rows selected by weights), so the closed forms,
// the Gauss-Hermite log-sum-exp and every sum order of a row exist once and the two launches give the same bits for the same row.
#pragma once
#include "gsmvi_batched.h"
#include "gsmvi_glm_link.h"

#define GP_MAXQ 64     // quadrature nodes at most
#define GP_LF 65       // row stride of the node values in LDS
#define GP_QL 8        // lanes per row in the quadrature

// Called by all NT threads of a slot after the barrier that publishes Ms (m of the tile's rows) and Vp (nb x 32 block sums of v);
// every slot of a workgroup calls it in the same iteration: its barriers are the workgroup's (quad, hasy and Q are uniform in the
// launch).  Row n of the tile is worked on iff n < tnv and (SEL) Vs[n] > 0; any other row is left alone: nothing of it is read but
// Vs[n], nothing is written.  Thread n forms v (ascending block order), v+, s = sqrt(2 v+), the NaN flag and the closed forms;
// then the quadrature: NT / 8 rows at a time, 8 adjacent lanes per row, lane g the nodes g, g + 8, .., the node values in F0
// ((NT / 8) x GP_LF doubles, which may lie over the tile: it is dead after the first barrier here), the maximum a butterfly, the
// sum over q in ascending q in one lane.  Leaves lpd of the rows in Ls (with y) for the caller's ordered elpd sum, which needs
// no further barrier.  gt, gl, gw: the nodes, the logarithms of the weights, the weights.
template <int NT, int FAM, bool SEL>
__device__ __forceinline__ void gp_row_stage(const bool hasy, const bool quad, const int Q, const int nb, const int l, const int tnv,
                                             const long long n0, const double tau, const double* gt, const double* gl,
                                             const double* gw, const double* Vp, const double* Ms, const double* Ys, const double* Vs,
                                             double* Hs, double* Bd, double* Ls, double* F0, double* em, double* ev, double* pm,
                                             double* lp) {
    constexpr int RG = NT / GP_QL, NGRP = LB_TN / RG;
    const int rr = l / GP_QL, g = l % GP_QL;  // the quadrature: row rr of the group, nodes g, g + 8, ..
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    if (l < tnv && (!SEL || Vs[l] > 0.0)) {   // row l: v, the NaN rule, the closed forms
        const int n = l;
        double v = 0.0;
        for (int jb = 0; jb < nb; ++jb) v += Vp[jb * LB_TN + n];
        const double m = Ms[n];
        const bool bad = !(gb_finite(m) && gb_finite(v));
        const double vp = v > 0.0 ? v : 0.0;
        Hs[n] = sqrt(2.0 * vp);
        Bd[n] = bad ? 1.0 : 0.0;
        em[n0 + n] = bad ? qnan : m;
        ev[n0 + n] = bad ? qnan : v;
        if (FAM == LB_GAUSSIAN) pm[n0 + n] = bad ? qnan : m;
        if (FAM == LB_PROBIT) pm[n0 + n] = bad ? qnan : 0.5 * erfc(-(m / sqrt(1.0 + vp)) * 0.70710678118654752440);
        if (FAM == LB_POISSON) pm[n0 + n] = bad ? qnan : exp(m + 0.5 * vp);
        if (FAM == LB_GAUSSIAN && hasy) {
            const double var = vp + 1.0 / tau, d = Ys[n] - m;
            const double t = -0.5 * log(6.28318530717958647692 * var) - (d * d) / (2.0 * var);
            const double out = bad ? qnan : t;
            lp[n0 + n] = out;
            Ls[n] = out;
        }
    }
    __syncthreads();                          // m, s and the flags are published; the tile is free
    if (quad) {
#pragma unroll 1
        for (int grp = 0; grp < NGRP; ++grp) {
            const int n = grp * RG + rr;
            const bool on = n < tnv && (!SEL || Vs[n] > 0.0);
            double* F = F0 + rr * GP_LF;
            double m = 0.0, s = 0.0, yv = 0.0;
            bool bad = false;
            if (on) {
                m = Ms[n];
                s = Hs[n];
                bad = Bd[n] != 0.0;
                if (hasy) yv = Ys[n];
            }
            if (FAM == LB_LOGISTIC) {         // pmean: sigma(eta_q) = -r(eta_q, y = 0) of the link
                if (on)
                    for (int q = g; q < Q; q += GP_QL) {
                        double r = 0.0, t = 0.0;
                        lb_link<FAM, true, false>(m + s * gt[q], 0.0, 1.0, r, t);
                        F[q] = gw[q] * -r;
                    }
                __syncthreads();
                if (on && g == 0) {
                    double sum = 0.0;
                    for (int q = 0; q < Q; ++q) sum += F[q];
                    pm[n0 + n] = bad ? qnan : sum / 1.77245385090551602730;
                }
                __syncthreads();
            }
            if (hasy) {                       // lpd: the maximum first, then the sum in ascending q
                double mx = -__builtin_huge_val();
                if (on)
                    for (int q = g; q < Q; q += GP_QL) {
                        double r = 0.0, t = 0.0;
                        lb_link<FAM, false, true>(m + s * gt[q], yv, 1.0, r, t);
                        const double f = gl[q] + t;
                        F[q] = f;
                        mx = fmax(mx, f);
                    }
#pragma unroll
                for (int o = GP_QL / 2; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
                if (on)
                    for (int q = g; q < Q; q += GP_QL) F[q] = exp(F[q] - mx);
                __syncthreads();
                if (on && g == 0) {
                    double sum = 0.0;
                    for (int q = 0; q < Q; ++q) sum += F[q];
                    double t = (mx + log(sum)) - 0.57236494292470008707;
                    if (FAM == LB_POISSON) t -= lgamma(yv + 1.0);
                    const double out = bad ? qnan : t;
                    lp[n0 + n] = out;
                    Ls[n] = out;
                }
                __syncthreads();
            }
        }
    }
}
