// The links of the batched GLM kernels (gsmvi_logistic_batched.hip: score and density; gsmvi_laplace_batched.hip: Hessian and
// Newton step; gsmvi_glm_predict_batched.hip: the predictive): r = dt / d eta and t of family FAM
// (lb_link), and the weight w = -dr / d eta (lb_weight).  What surrounds the kernels is in gsmvi_glm_model.h.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/gsmvi_hip.h"

enum { LB_G = 1, LB_LP = 2 };
enum { LB_LOGISTIC = GSMVI_GLM_LOGISTIC, LB_POISSON = GSMVI_GLM_POISSON, LB_PROBIT = GSMVI_GLM_PROBIT,
       LB_GAUSSIAN = GSMVI_GLM_GAUSSIAN };
#define LB_TN 32   // rows of A_k per tile
#define LB_PROBIT_S0 4.0   // lb_weight<LB_PROBIT>: the tail side is the continued fraction from |eta| = 4 on
#define LB_PROBIT_CF 40    // ... at this depth

// The link of family FAM at eta = h, label y (tau: the gaussian noise precision): r = d t / d eta and t, each evaluated only
// when wanted.  Returns false when the row of X must be flagged (poisson: e^eta is not finite); what r and t then hold reaches
// no output, the flag replaces every output of the row.
template <int FAM, bool HAS_G, bool HAS_LP>
__device__ __forceinline__ bool lb_link(double h, double y, double tau, double& r, double& t) {
    if constexpr (FAM == LB_LOGISTIC) {
        const double e = exp(-fabs(h)), d = 1.0 + e;
        if (HAS_G) r = y - (h >= 0.0 ? 1.0 / d : e / d);
        if (HAS_LP) t = y * h - ((h > 0.0 ? h : 0.0) + log1p(e));
        return true;
    } else if constexpr (FAM == LB_POISSON) {
        const double m = exp(h);
        if (HAS_G) r = y - m;
        if (HAS_LP) t = y * h - m;
        return m < __builtin_huge_val();                   // (false for a NaN too)
    } else if constexpr (FAM == LB_PROBIT) {
        // s = |eta|, u = erfcx(s / sqrt 2), e = exp(-s^2 / 2), q = u e / 2 = Phi(-s).  Tail side: log Phi(-s) = log(u / 2) - s^2 / 2,
        // phi / Phi(-s) = sqrt(2 / pi) / u.  Central side: log Phi(s) = log1p(-q), phi / Phi(s) = e / sqrt(2 pi) / (1 - q).
        const double s = fabs(h), u = erfcx(s * 0.70710678118654752440), hs = 0.5 * (s * s), e = exp(-hs), q = 0.5 * (u * e);
        const double rt = 0.79788456080286535588 / u, rc = e * 0.39894228040143267794 / (1.0 - q);
        double lt = 0.0, lc = 0.0;
        if (HAS_LP) {
            // From |eta| = 1.34e154 on s^2 overflows; held at the largest finite number, a tail label of weight exactly 0 gives
            // the -0 it gives at every other eta, not the NaN of 0 * inf.  (A maximum and not a select on y: the 256-thread
            // density kernel of k_logistic_batched has no register to spare.  A NaN eta still reaches t through lc.)  The
            // consequence for a tail label of weight > 0 there: t is (1 - y) times -1.8e308, finite, where log Phi(-s) itself
            // is below the float64 range from 1.9e154 on and the earlier form gave -inf.  Nothing may take lp = -inf as the
            // sign of such an eta.
            lt = fmax(log(0.5 * u) - hs, -1.7976931348623157e308);
            lc = log1p(-q);
        }
        if (h >= 0.0) {                                    // Phi(eta) is the central side
            if (HAS_G) r = y * rc - (1.0 - y) * rt;
            if (HAS_LP) t = y * lc + (1.0 - y) * lt;
        } else {
            if (HAS_G) r = y * rt - (1.0 - y) * rc;
            if (HAS_LP) t = y * lt + (1.0 - y) * lc;
        }
        return true;
    } else {
        const double d = y - h;
        if (HAS_G) r = tau * d;
        if (HAS_LP) t = -0.5 * (tau * (d * d));
        return true;
    }
}

// The weight w = -dr / d eta of family FAM at eta = h: the negative Hessian of lp is sum_n w_n a_n a_n^T + lam I.  All four
// families are log-concave, so w >= 0 up to rounding.  Returns false when the row must be flagged (poisson: e^eta not finite).
//   logistic  sigma (1 - sigma) = e / (1 + e)^2, e = exp(-|eta|)
//   poisson   e^eta
//   probit    y wp + (1 - y) wm with wp = hp (hp + eta), wm = hm (hm - eta), hp = phi / Phi(eta), hm = phi / Phi(-eta): the two
//             values lb_link forms from erfcx.  With s = |eta| one of the two is the central side, h (h + s), a sum of positive
//             terms; the other is the tail side (wp at eta < 0, wm at eta > 0), h (h - s) with h ~ s + 1 / s: the subtraction
//             cancels, and what is left has the relative error of erfcx times about s^2 (by 1e8 it was the whole value).  So
//             from s = LB_PROBIT_S0 on the tail side comes without a subtraction, from Laplace's continued fraction of the
//             Mills ratio, h = s + K, K = 1 / (s + 2 / (s + 3 / (s + ..))): with z = 1 / s^2 and g = s K = 1 / (1 + 2 z / (1 + 3 z /
//             (1 + ..))), h (h - s) = g (1 + z g).  g is the convergent of depth LB_PROBIT_CF as ONE ratio of its forward
//             recurrence (all terms positive, z <= 1 / 16: no overflow, one division); its truncation error at s = 4 is 0.05 eps
//             and falls with s.  Below S0 the subtraction stays, with erfcx's error times at most 17 ("The
//             links element by element", has the measured figures).  Both sides are finite for every finite eta and
//             0 <= w <= 1, so a label weight of exactly 0 never meets an infinity.
//   gaussian  tau
template <int FAM>
__device__ __forceinline__ bool lb_weight(double h, double y, double tau, double& w) {
    if constexpr (FAM == LB_LOGISTIC) {
        const double e = exp(-fabs(h)), d = 1.0 + e;
        w = e / (d * d);
        return true;
    } else if constexpr (FAM == LB_POISSON) {
        w = exp(h);
        return w < __builtin_huge_val();
    } else if constexpr (FAM == LB_PROBIT) {
        const double s = fabs(h), u = erfcx(s * 0.70710678118654752440), hs = 0.5 * (s * s), e = exp(-hs), q = 0.5 * (u * e);
        const double rt = 0.79788456080286535588 / u, rc = e * 0.39894228040143267794 / (1.0 - q);
        const double wc = rc * (rc + s);                   // the central side
        double wt;                                         // the tail side
        if (s >= LB_PROBIT_S0) {
            const double x = 1.0 / s, z = x * x;
            double a0 = 0.0, a1 = 1.0, b0 = 1.0, b1 = 1.0;  // numerator and denominator of the convergents of g
#pragma unroll
            for (int k = 2; k <= LB_PROBIT_CF; ++k) {
                const double c = k * z, a2 = fma(c, a0, a1), b2 = fma(c, b0, b1);
                a0 = a1;
                a1 = a2;
                b0 = b1;
                b1 = b2;
            }
            const double g = a1 / b1;
            wt = g * fma(z, g, 1.0);
        } else
            wt = rt * (rt - s);
        w = h >= 0.0 ? y * wc + (1.0 - y) * wt : y * wt + (1.0 - y) * wc;
        return true;
    } else {
        w = tau;
        return true;
    }
}
