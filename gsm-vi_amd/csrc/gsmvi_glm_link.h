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
            lt = log(0.5 * u) - hs;
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
//   probit    y hp (hp + eta) + (1 - y) hm (hm - eta) with hp = phi / Phi(eta), hm = phi / Phi(-eta): the two values lb_link forms
//             from erfcx.  On the tail side (hp at eta < 0, hm at eta > 0) h -+ eta cancels: h ~ |eta| + 1 / |eta|, so the factor
//             is ~ 1 / |eta| from two terms of size |eta| and the relative error of w grows like eps eta^2 (1e-14 at |eta| = 8).
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
        const double hp = h >= 0.0 ? rc : rt, hm = h >= 0.0 ? rt : rc;
        w = y * (hp * (hp + h)) + (1.0 - y) * (hm * (hm - h));
        return true;
    } else {
        w = tau;
        return true;
    }
}
