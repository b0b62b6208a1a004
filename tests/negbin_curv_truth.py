"""The element-wise truth of the curvature of the negative binomial link (csrc/gsmvi_negbin_link.h: w_ee, w_et, w_tt, the row's
2 x 2 block of the negative Hessian in (eta, theta)), independent of the kernel's forms, on the grid of tests/negbin_link_truth.py
and with its metric ("Negative binomial Laplace initialiser").  Test-only.

``values`` evaluates, with mpmath's digamma and polygamma, at the float64 inputs (eta, theta, y), r = e^theta, d = eta - theta,
sigma = sigma(d), r_eta = y sigma(-d) - r sigma, dps = psi(y + r) - psi(r), dtg = psi'(y + r) - psi'(r):

    w_ee = (y + r) sigma sigma(-d)
    w_et = -sigma r_eta
    w_tt = -[ r (dps - softplus(d)) + r^2 dtg + r sigma - sigma r_eta ]

to 60 and to 120 digits (plus guard digits), which must agree to 1e-40 of the scale below, or it raises.

The metric is negbin_link_truth's: the error of a computed f in {w_ee, w_et, w_tt} is measured in units of

    eps (|f| + |eta df/d eta| + |theta df/d theta| + a_f) + 2^-1070

a_f: the sum of the magnitudes of the terms as written above, with dps and dtg as primitives: a_ee = (y + r) sigma sigma(-d),
a_et = sigma (y sigma(-d) + r sigma), a_tt = r |dps| + r softplus(d) + r^2 |dtg| + r sigma + a_et.  The derivatives of f are third
derivatives of the density: they come from ``mp.diff`` of ``negbin_link_truth.written``, not from a formula of this module.  The
committed table (tests/golden/negbin_curv_truth.npz) holds per grid point the value, the float64 remainder and the scale (all
float64: w_ee is of order e^-700 at d = 700, below the float32 range), so that the GPU test needs no mpmath."""
import os

import numpy as np

import negbin_link_truth as lt
from negbin_link_truth import EPS, FLOOR, grid, split, ratio, load_table as _load     # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "negbin_curv_truth.npz")
QUANTITIES = ("wee", "wet", "wtt")
NAMES = QUANTITIES + tuple("scale_" + q for q in QUANTITIES)
# The worst ratio of the float64 restatement (negbin_laplace_ref.curv: numpy's exp, log, log1p) over the whole grid, rounded up:
# asserted in tests/test_negbin_laplace_cpu.py, printed there, DESIGN.md section 9
C_CPU = {"wee": 1.1, "wet": 0.9, "wtt": 1.3}
C_FLOOR, C_DEVICE = lt.C_FLOOR, lt.C_DEVICE     # the GPU bound: max(16, 4 C_CPU); never from the device's own figures


def c_gpu(quantity):
    return max(C_FLOOR, C_DEVICE * C_CPU[quantity])


def _at(eta, theta, y, dps):
    """(wee, wet, wtt, a_ee, a_et, a_tt) at working precision dps + 40 guard digits"""
    import mpmath as mp
    with mp.workdps(dps + 40):
        h, th, yy, one = mp.mpf(float(eta)), mp.mpf(float(theta)), mp.mpf(float(y)), mp.mpf(1)
        r, d = mp.exp(th), h - th
        sg, sn = one / (one + mp.exp(-d)), one / (one + mp.exp(d))                 # sigma(d), sigma(-d)
        spd = -mp.log(sn)                                                          # softplus(d)
        dpsi = mp.digamma(yy + r) - mp.digamma(r)
        dtri = mp.polygamma(1, yy + r) - mp.polygamma(1, r)
        re = yy * sn - r * sg
        wee = (yy + r) * sg * sn
        wet = -sg * re
        wtt = -(r * (dpsi - spd) + r * r * dtri + r * sg - sg * re)
        a_et = sg * (yy * sn + r * sg)
        return wee, wet, wtt, wee, a_et, r * abs(dpsi) + r * spd + r * r * abs(dtri) + r * sg + a_et


def _third(eta, theta, y, dps=30):
    """the four third derivatives of the written density, by mp.diff: (t_eee, t_eet, t_ett, t_ttt).  mp.diff resolves a derivative
    relative to the size of the function, and the derivatives in eta fall like e^-|d| beside it: |d| / log 10 more digits."""
    import mpmath as mp
    with mp.workdps(dps + 40 + int(abs(float(eta) - float(theta)) / 2.302585)):
        h, th = mp.mpf(float(eta)), mp.mpf(float(theta))
        f = lambda a, b: lt.written(a, b, y)                         # noqa: E731
        return tuple(mp.diff(f, (h, th), n) for n in ((3, 0), (2, 1), (1, 2), (0, 3)))


def values(eta, theta, y):
    """{"wee", "wet", "wtt", "scale_wee", "scale_wet", "scale_wtt"} as mpf: the values computed to 60 and to 120 digits, which
    must agree to 1e-40 of the quantity's scale (raises ArithmeticError otherwise); the 120-digit values are returned"""
    import mpmath as mp
    lo, hi = _at(eta, theta, y, 60), _at(eta, theta, y, 120)
    eee, eet, ett, ttt = _third(eta, theta, y)
    with mp.workdps(170):
        ah, at = abs(mp.mpf(float(eta))), abs(mp.mpf(float(theta)))
        der = (ah * abs(eee) + at * abs(eet), ah * abs(eet) + at * abs(ett), ah * abs(ett) + at * abs(ttt))
        scales = [abs(hi[i]) + der[i] + hi[3 + i] for i in range(3)]
        for i, name in enumerate(QUANTITIES):
            if abs(lo[i] - hi[i]) > mp.mpf(10) ** -40 * scales[i]:
                raise ArithmeticError(f"{name} at eta = {eta!r}, theta = {theta!r}, y = {y!r}: 60 and 120 digits disagree")
    return dict(zip(NAMES, list(hi[:3]) + scales))


def build_table():
    """the arrays of tests/golden/negbin_curv_truth.npz, from mpmath"""
    eta, theta, y = grid()
    tab = {q: np.zeros((2, len(eta))) for q in QUANTITIES}
    tab.update({"scale_" + q: np.zeros(len(eta)) for q in QUANTITIES})
    for i, (h, th, yy) in enumerate(zip(eta, theta, y)):
        v = values(h, th, yy)
        for q in QUANTITIES:
            tab[q][:, i] = split(v[q])
            tab["scale_" + q][i] = np.nextafter(float(v["scale_" + q]), 0.0)        # (rounded down: it never flatters)
    return tab


def write_table(path=GOLDEN):
    np.savez(path, **build_table())


def load_table(path=GOLDEN):
    return _load(path)


if __name__ == "__main__":
    write_table()
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
