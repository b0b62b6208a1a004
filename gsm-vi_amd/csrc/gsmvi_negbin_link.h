// The link of the batched negative binomial target (gsmvi_negbin_batched.hip; DESIGN.md section 9, "Batched negative binomial
// target"): with r = e^theta the size, d = eta - theta and the two difference functions
//   dlg(y, r) = lgamma(y + r) - lgamma(r)          dps(y, r) = psi(y + r) - psi(r)
// the per-observation density and its two derivatives are
//   t       = dlg - r softplus(d) - y softplus(-d)
//   r_eta   = y sigma(-d) - r sigma(d)
//   r_theta = r (dps - softplus(d)) - r_eta
// Neither difference is formed from two library calls (lgamma(1e13) is 3e14: its rounding alone is 0.03, the difference is of
// order y log r; and the device library has no digamma).  Both come from Stirling's series as a difference: for z >= 10
//   lgamma(z) = (z - 1/2) log z - z + log(2 pi) / 2 + S(z)         psi(z) = log z - 1 / (2 z) + P(z)
//   dlg = (z - 1/2) log1p(y / z) + y (log(z + y) - 1) + [S(z + y) - S(z)]
//   dps = log1p(y / z) + y / (2 z (z + y)) + [P(z + y) - P(z)]
// with S and P the seven-term tails (the first term left out is 3e-17 and 5e-17 at z = 10).  For r < NB_SHIFT_BELOW the
// recurrences lgamma(r) = lgamma(r + 10) - sum_j log(r + j), psi(r) = psi(r + 10) - sum_j 1 / (r + j), j = 0 .. 9, applied to both
// arguments leave z = r + 10 and the two sums of positive terms
//   sl = sum_j log1p(y / (r + j))  (subtracted from dlg)       sp = sum_j y / ((r + j)(r + j + y))  (added to dps)
// The term j = 0 of sp is (y / (r + y)) / r (r (r + y) may underflow), and of sl it is log y - theta where y / r overflows.
// softplus and sigma are the overflow-safe forms of the logistic link: e^eta is never formed.
//
// The curvature (gsmvi_negbin_laplace_batched.hip): the row's 2 x 2 block of the negative Hessian in (eta, theta), with
// dtg(y, r) = psi'(y + r) - psi'(r) <= 0,
//   w_ee = -d r_eta / d eta     = (y + r) sigma(d) sigma(-d)                                       (>= 0)
//   w_et = -d r_eta / d theta   = -sigma(d) r_eta
//   w_tt = -d r_theta / d theta = -[ r (dps - softplus(d)) + r^2 dtg + r sigma(d) - sigma(d) r_eta ]    (any sign)
// dtg is the same kind of difference: psi'(z) = 1 / z + 1 / (2 z^2) + T(z), T the nine-term tail (the first term left out is 5e-19
// at z = 10, and its slope in y 1e-16 of dtg's: seven terms would leave 50 eps of dtg at r = 10, small y), so for z >= 10
//   dtg = -y / (z (z + y)) - y (2 z + y) / (2 z^2 (z + y)^2) + [T(z + y) - T(z)]
// and for r < NB_SHIFT_BELOW the recurrence psi'(r) = psi'(r + 10) + sum_j 1 / (r + j)^2 adds the terms
//   -y (2 a + y) / (a^2 (a + y)^2) = -q_j (2 a + y) / (a (a + y)),   a = r + j,   q_j = y / (a (a + y)) the term of sp.
// Only r^2 dtg is needed.  It is r (r [..]) with the term j = 0 kept apart as -(y / (r + y)) (1 + r / (r + y)): r^2 is never
// formed (it underflows below r = 1e-154) and is not cancelled against the 1 / r^2 of that term.
#pragma once
#include <hip/hip_runtime.h>

#define NB_SHIFT_BELOW 10.0   // r below it: ten steps of the recurrence, z = r + 10
#define NB_SHIFT 10

// S(z) = sum_{k=1..7} B_2k / (2k (2k - 1) z^(2k - 1)), z >= 10
__device__ __forceinline__ double nb_lgamma_tail(double z) {
    const double x = 1.0 / z, w = x * x;
    double p = 1.0 / 156.0;
    p = p * w + -691.0 / 360360.0;
    p = p * w + 1.0 / 1188.0;
    p = p * w + -1.0 / 1680.0;
    p = p * w + 1.0 / 1260.0;
    p = p * w + -1.0 / 360.0;
    p = p * w + 1.0 / 12.0;
    return p * x;
}

// P(z) = -sum_{k=1..7} B_2k / (2k z^(2k)), z >= 10
__device__ __forceinline__ double nb_digamma_tail(double z) {
    const double x = 1.0 / z, w = x * x;
    double p = -1.0 / 12.0;
    p = p * w + 691.0 / 32760.0;
    p = p * w + -1.0 / 132.0;
    p = p * w + 1.0 / 240.0;
    p = p * w + -1.0 / 252.0;
    p = p * w + 1.0 / 120.0;
    p = p * w + -1.0 / 12.0;
    return p * w;
}

// T(z) = sum_{k=1..9} B_2k / z^(2k + 1), z >= 10
__device__ __forceinline__ double nb_trigamma_tail(double z) {
    const double x = 1.0 / z, w = x * x;
    double p = 43867.0 / 798.0;
    p = p * w + -3617.0 / 510.0;
    p = p * w + 7.0 / 6.0;
    p = p * w + -691.0 / 2730.0;
    p = p * w + 5.0 / 66.0;
    p = p * w + -1.0 / 30.0;
    p = p * w + 1.0 / 42.0;
    p = p * w + -1.0 / 30.0;
    p = p * w + 1.0 / 6.0;
    return (p * w) * x;
}

// The link at eta = h, log size theta, r = e^theta (a positive normal number: anything else is the caller's row flag, and what
// comes out then reaches no output), response y >= 0: re = r_eta and rt = r_theta when HAS_G, t when HAS_LP, and with HAS_W (which
// needs HAS_G) the curvature wee, wet, wtt.  Without HAS_W every operation is the one the score kernel has always run.
template <bool HAS_G, bool HAS_LP, bool HAS_W>
__device__ __forceinline__ void nb_link_core(double h, double theta, double r, double y, double& re, double& rt, double& t,
                                             double& wee, double& wet, double& wtt) {
    static_assert(HAS_G || !HAS_W, "the curvature is formed from r_eta and dps");
    const double d = h - theta, e = exp(-fabs(d)), q = 1.0 + e, l1 = log1p(e);
    const double spd = (d > 0.0 ? d : 0.0) + l1;               // softplus(d)
    double z = r, sl = 0.0, sp = 0.0, st = 0.0, tg0 = 0.0;     // st: the terms j >= 1 of dtg; tg0: r^2 times its term j = 0
    if (r < NB_SHIFT_BELOW) {
        if (HAS_LP) {
            const double u = y / r;
            sl = u < 1e300 ? log1p(u) : log(y) - theta;
        }
        if (HAS_G) sp = (y / (r + y)) / r;
        if (HAS_W) {
            const double ry = r + y;
            tg0 = -((y / ry) * (1.0 + r / ry));
        }
#pragma unroll 1
        for (int j = 1; j < NB_SHIFT; ++j) {
            const double a = r + (double)j;
            if (HAS_LP) sl += log1p(y / a);
            if (HAS_G) {
                const double m = a * (a + y), qj = y / m;
                sp += qj;
                if (HAS_W) st -= qj * ((a + (a + y)) / m);
            }
        }
        z = r + (double)NB_SHIFT;
    }
    const double zy = z + y, lu = log1p(y / z);
    if (HAS_LP) {
        const double spn = (d < 0.0 ? -d : 0.0) + l1;          // softplus(-d)
        const double dlg = ((z - 0.5) * lu + y * (log(zy) - 1.0)) + (nb_lgamma_tail(zy) - nb_lgamma_tail(z)) - sl;
        t = dlg - r * spd - y * spn;
    }
    if (HAS_G) {
        const double sg = d >= 0.0 ? 1.0 / q : e / q, sn = d >= 0.0 ? e / q : 1.0 / q;     // sigma(d), sigma(-d)
        const double dps = lu + y / (2.0 * z * zy) + (nb_digamma_tail(zy) - nb_digamma_tail(z)) + sp;
        re = y * sn - r * sg;
        rt = r * (dps - spd) - re;
        if (HAS_W) {
            const double x1 = -((y / zy) / z);                                   // 1 / (z + y) - 1 / z
            const double x2 = x1 * ((0.5 * (z / zy + 1.0)) / z);                  // 1 / (2 (z + y)^2) - 1 / (2 z^2)
            const double dtz = ((x1 + x2) + (nb_trigamma_tail(zy) - nb_trigamma_tail(z))) + st;
            const double r2dtg = r * (r * dtz) + tg0, sre = sg * re;
            wee = ((y + r) * sg) * sn;
            wet = -sre;
            wtt = -(((r * (dps - spd) + r2dtg) + r * sg) - sre);
        }
    }
}

template <bool HAS_G, bool HAS_LP>
__device__ __forceinline__ void nb_link(double h, double theta, double r, double y, double& re, double& rt, double& t) {
    double wee, wet, wtt;
    nb_link_core<HAS_G, HAS_LP, false>(h, theta, r, y, re, rt, t, wee, wet, wtt);
}

// the link with the curvature: r_eta, r_theta, the three weights, and t when HAS_LP
template <bool HAS_LP>
__device__ __forceinline__ void nb_link_curv(double h, double theta, double r, double y, double& re, double& rt, double& t,
                                             double& wee, double& wet, double& wtt) {
    nb_link_core<true, HAS_LP, true>(h, theta, r, y, re, rt, t, wee, wet, wtt);
}
