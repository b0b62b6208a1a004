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

// The curvature (gsmvi_ordinal_laplace_batched.hip).  In the gap coordinates gamma = (delta_0, w_1 .. w_{C-2}) both a and b are
// linear, a = gamma_0 + sum_{1 <= i < y} gamma_i - eta and b = a + gamma_y, and with fa = sigma(a) sigma(-a) (0 for y = 0),
// fb = sigma(b) sigma(-b) (0 for y = C - 1), z_a = (-a_n; 1 on gamma_0 .. gamma_{y-1}), z_b = (-a_n; 1 on gamma_0 .. gamma_y),
//   -grad^2 t = fa z_a z_a^T + fb z_b z_b^T + [interior] q_y (1 + q_y) e_y e_y^T,      q_y = 1 / expm1(w_y),
// a sum of positive semi-definite terms: no two probabilities are subtracted and no q^2 terms cancel (the derivative of
// (u_lo, u_hi) in the cutpoints has +-q^2 entries that cancel against each other for a narrow gap: H is never built from that form).
// The gap term depends on the class alone and is added per class by the kernel's epilogue.

// softplus(z), sigma(z) and sigma(z) sigma(-z) from one exponential (sp only when HAS_LP); sg and sp are ord_sps's, bit for bit
template <bool HAS_LP>
__device__ __forceinline__ void ord_spsf(double z, double& sp, double& sg, double& f) {
    const double e = exp(-fabs(z));
    if (HAS_LP) sp = (z > 0.0 ? z : 0.0) + log1p(e);
    const double q = 1.0 + e, big = 1.0 / q, small = e / q;
    sg = z >= 0.0 ? big : small;
    f = big * small;
}

// ord_link with the curvature weights: re = r_eta and t (when HAS_LP) as ord_link gives them, sb = sigma(-b) (0 for y = C - 1),
// fab = fa + fb and fb
template <bool HAS_LP>
__device__ __forceinline__ void ord_link_curv(double h, int y, int C, const double* cut, const double* lm, double& re, double& sb,
                                              double& fab, double& fb, double& t) {
    const bool lo = y >= 1, hi = y <= C - 2;
    double spa = 0.0, sga = 0.0, fa = 0.0, spb = 0.0, sgb = 0.0, fbv = 0.0;
    if (lo) ord_spsf<HAS_LP>(cut[y - 1] - h, spa, sga, fa);
    if (hi) ord_spsf<HAS_LP>(-(cut[y] - h), spb, sgb, fbv);
    if (HAS_LP) t = (-spb - spa) + (lo && hi ? lm[y] : 0.0);
    re = sga - sgb;
    sb = sgb;
    fab = fa + fbv;
    fb = fbv;
}
