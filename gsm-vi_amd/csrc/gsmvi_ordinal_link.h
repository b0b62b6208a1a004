// The link of the batched ordinal (cumulative logit, proportional odds) target (gsmvi_ordinal_batched.hip; DESIGN.md section 9,
// "Batched ordinal target"): with the ordered cutpoints cut_0 = delta_0, cut_j = cut_{j-1} + e^{delta_j}, the label y in
// 0 .. C - 1 and the linear predictor eta,
//   P(y = c) = sigma(cut_c - eta) - sigma(cut_{c-1} - eta),   cut_{-1} = -inf, cut_{C-1} = +inf
// Write a = cut_{y-1} - eta (y >= 1), b = cut_y - eta (y <= C - 2) and, for an interior class 1 <= y <= C - 2, w = e^{delta_y} = b - a:
// the gap itself, never a difference of two rounded cutpoints.  sigma(b) - sigma(a) = sigma(b) sigma(-a) (1 - e^{-w}) gives
//   t    = -[y <= C-2] softplus(-b) - [y >= 1] softplus(a) + [interior] log1mexp(w)
//   u_lo = dt / d cut_{y-1} = -sigma(a) - [interior] / expm1(w)          (y >= 1, else 0)
//   u_hi = dt / d cut_y     =  sigma(-b) + [interior] / expm1(w)         (y <= C-2, else 0)
//   r_eta = dt / d eta      =  sigma(a) - sigma(-b)
// No two probabilities are subtracted anywhere.  log1mexp(w) = log(1 - e^{-w}) and 1 / expm1(w) depend on the row of X alone, so
// the kernel's prologue evaluates them once per (row of X, class) with ord_gap and the link only reads them.  softplus and sigma are
// the overflow-safe forms of the logistic link: e^{+|z|} is never formed.
#pragma once
#include <hip/hip_runtime.h>

// The gap terms of w = e^{delta_j} > 0: lm = log(1 - e^{-w}), the proper log1mexp (log(-expm1(-w)) below log 2, log1p(-e^{-w}) above),
// and qe = 1 / expm1(w) (0 where expm1 overflows; at most 4.5e307 for a normal w)
__device__ __forceinline__ void ord_gap(double w, double& lm, double& qe) {
    lm = w < 0.6931471805599453 ? log(-expm1(-w)) : log1p(-exp(-w));
    qe = 1.0 / expm1(w);
}

// softplus(z) and sigma(z) from one exponential
template <bool HAS_G, bool HAS_LP>
__device__ __forceinline__ void ord_sps(double z, double& sp, double& sg) {
    const double e = exp(-fabs(z));
    if (HAS_LP) sp = (z > 0.0 ? z : 0.0) + log1p(e);
    if (HAS_G) {
        const double q = 1.0 + e;
        sg = z >= 0.0 ? 1.0 / q : e / q;
    }
}

// The link at eta = h for the label y in 0 .. C - 1 (the caller clamps it) of a row of X whose prologue left cut (C - 1 cutpoints),
// lm and qe (ord_gap of e^{delta_j}, j = 1 .. C - 2; entry 0 is not read): re = r_eta, ulo, uhi when HAS_G, t when HAS_LP.
template <bool HAS_G, bool HAS_LP>
__device__ __forceinline__ void ord_link(double h, int y, int C, const double* cut, const double* lm, const double* qe, double& re,
                                         double& ulo, double& uhi, double& t) {
    const bool lo = y >= 1, hi = y <= C - 2, in = lo && hi;
    double spa = 0.0, sga = 0.0, spb = 0.0, sgb = 0.0;         // softplus(a), sigma(a); softplus(-b), sigma(-b)
    if (lo) ord_sps<HAS_G, HAS_LP>(cut[y - 1] - h, spa, sga);
    if (hi) ord_sps<HAS_G, HAS_LP>(-(cut[y] - h), spb, sgb);
    if (HAS_LP) t = (-spb - spa) + (in ? lm[y] : 0.0);
    if (HAS_G) {
        const double q = in ? qe[y] : 0.0;
        ulo = lo ? -sga - q : 0.0;
        uhi = hi ? sgb + q : 0.0;
        re = sga - sgb;
    }
}
