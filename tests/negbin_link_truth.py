"""The element-wise truth of the negative binomial link (csrc/gsmvi_negbin_link.h: t, r_eta = dt / d eta, r_theta = dt / d theta),
independent of the kernel's forms, and the metric it is held to ("Batched negative binomial target").
Test-only, in the style of tests/glm_link_truth.py.

``values`` evaluates, with mpmath's loggamma, digamma and polygamma, at the float64 inputs (eta, theta, y), r = e^theta, d = eta - theta:

    t       = dlg - r softplus(d) - y softplus(-d)                 dlg = lgamma(y + r) - lgamma(r)
    r_eta   = y sigma(-d) - r sigma(d)
    r_theta = r (dps - softplus(d)) - r_eta                        dps = psi(y + r) - psi(r)

to 60 and to 120 digits (plus guard digits: lgamma(1e13) is 3e14), which must agree to 1e-40 of the scale below, or it raises.

``grid`` is the single source of points: theta in [-30, 30] (fixed points, both sides of the shift threshold log 10 among them, and
seeded points in [-5, 8]) x d in D_VALUES x y in Y_VALUES, eta = d + theta rounded to float64.  The committed table
(tests/golden/negbin_link_truth.npz) holds per grid point the value and the float64 remainder of the three quantities (float64) and
their scales (float32: a scale needs no more), so that the GPU test needs no mpmath.

The metric: the error of a computed f in {t, r_eta, r_theta} is measured in units of

    eps (|f| + |eta df/d eta| + |theta df/d theta| + a_f) + 2^-1070

|eta df/d eta| + |theta df/d theta|: what the inputs being rounded numbers costs; a_f: the sum of the magnitudes of the terms of
the written definition, with dlg and dps as primitives: a_t = |dlg| + r softplus(d) + y softplus(-d), a_r_eta = y sigma(-d) +
r sigma(d), a_r_theta = r |dps| + r softplus(d) + y sigma(-d) + r sigma(d).  Taking dlg and dps as primitives is deliberate: a
scale built from |lgamma(y + r)| + |lgamma(r)| would admit the naive difference of two library calls.  ``ratio`` returns
err / (eps scale) with the subnormal floor taken off first."""
import os

import numpy as np

EPS = 2.0 ** -52
FLOOR = 2.0 ** -1070
LOG10 = 2.302585092994046                       # log 10: r = e^theta crosses NB_SHIFT_BELOW = 10 here
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "negbin_link_truth.npz")
D_VALUES = (-40.0, -5.0, -1.0, 0.0, 0.5, 3.0, 20.0, 700.0)
Y_VALUES = (0.0, 1.0, 2.0, 7.0, 0.3, 1e3, 1e6)
QUANTITIES = ("t", "re", "rt")
BEYOND = (1e160, 1e300)                         # |eta| outside the grid: no NaN, the sign of r_eta, inf only where the truth overflows
# The worst ratio of the float64 restatement (negbin_batched_ref.link: numpy's exp, log, log1p) over the whole grid, rounded up:
# asserted in tests/test_negbin_batched_cpu.py, printed there, DESIGN.md section 9
C_CPU = {"t": 1.8, "re": 0.6, "rt": 1.5}
C_FLOOR, C_DEVICE = 16.0, 4.0                   # the GPU bound: max(16, 4 C_CPU); never from the device's own figures


def c_gpu(quantity):
    return max(C_FLOOR, C_DEVICE * C_CPU[quantity])


def thetas():
    fixed = [-30.0, -20.0, -10.0, -5.0, -1.0, -1e-3, 0.0, 0.5, 1.0, 2.0, 2.3025, np.nextafter(LOG10, 0.0) - 1e-14, LOG10 + 1e-14,
             2.31, 3.0, 5.0, 8.0, 12.0, 20.0, 30.0]
    seeded = np.random.RandomState(20261020).uniform(-5.0, 8.0, 12)
    return np.concatenate([np.array(fixed, dtype=np.float64), seeded])


def grid():
    """(eta, theta, y) of every grid point, float64, theta-major then d then y"""
    th, d, y = np.meshgrid(thetas(), np.array(D_VALUES), np.array(Y_VALUES), indexing="ij")
    return (d + th).ravel(), th.ravel().copy(), y.ravel().copy()


# ---- mpmath ---------------------------------------------------------------------------------------------------------------
def written(eta, theta, y):
    """t of the density as written, literally, as a function of mpf eta, theta (for mp.diff)"""
    import mpmath as mp
    y = mp.mpf(float(y))
    r, d = mp.exp(theta), eta - theta
    return mp.loggamma(y + r) - mp.loggamma(r) - r * mp.log(1 + mp.exp(d)) - y * mp.log(1 + mp.exp(-d))


def _at(eta, theta, y, dps):
    """(t, re, rt, scale_t, scale_re, scale_rt) at working precision dps + 40 guard digits"""
    import mpmath as mp
    with mp.workdps(dps + 40):
        h, th, yy, one = mp.mpf(float(eta)), mp.mpf(float(theta)), mp.mpf(float(y)), mp.mpf(1)
        r, d = mp.exp(th), h - th
        sg, sn = one / (one + mp.exp(-d)), one / (one + mp.exp(d))                 # sigma(d), sigma(-d)
        spd, spn = -mp.log(sn), -mp.log(sg)                                        # softplus(d), softplus(-d)
        dlg = mp.loggamma(yy + r) - mp.loggamma(r)
        dpsi = mp.digamma(yy + r) - mp.digamma(r)
        dtri = mp.polygamma(1, yy + r) - mp.polygamma(1, r)
        s = sg * sn
        t = dlg - r * spd - yy * spn
        re = yy * sn - r * sg
        rt = r * (dpsi - spd) - re
        re_e = -(yy + r) * s                                                       # d r_eta / d eta
        re_t = (yy + r) * s - r * sg                                               # d r_eta / d theta = d r_theta / d eta
        rt_t = r * (dpsi - spd) + r * r * dtri + r * sg - re_t                     # d r_theta / d theta
        a_t = abs(dlg) + r * spd + yy * spn
        a_re = yy * sn + r * sg
        a_rt = r * abs(dpsi) + r * spd + a_re
        ah, at = abs(h), abs(th)
        return (t, re, rt, abs(t) + ah * abs(re) + at * abs(rt) + a_t, abs(re) + ah * abs(re_e) + at * abs(re_t) + a_re,
                abs(rt) + ah * abs(re_t) + at * abs(rt_t) + a_rt)


NAMES = ("t", "re", "rt", "scale_t", "scale_re", "scale_rt")


def values(eta, theta, y):
    """{"t", "re", "rt", "scale_t", "scale_re", "scale_rt"} as mpf: computed to 60 and to 120 digits, which must agree to 1e-40 of
    the quantity's scale (raises ArithmeticError otherwise); the 120-digit values are returned"""
    import mpmath as mp
    lo, hi = _at(eta, theta, y, 60), _at(eta, theta, y, 120)
    with mp.workdps(170):
        for i, (name, a, b) in enumerate(zip(NAMES, lo, hi)):
            # (relative to the quantity's scale: r_eta is an exact 0 where y = e^eta, e.g. at eta = 0, y = 1)
            if abs(a - b) > mp.mpf(10) ** -40 * hi[3 + i % 3]:
                raise ArithmeticError(f"{name} at eta = {eta!r}, theta = {theta!r}, y = {y!r}: 60 and 120 digits disagree: {a} {b}")
    return dict(zip(NAMES, hi))


def split(v):
    """an mpf as (float64 nearest, float64 remainder); an overflow stays +-inf with remainder 0"""
    import mpmath as mp
    with mp.workdps(170):
        hi = float(v)
        return hi, (float(v - mp.mpf(hi)) if np.isfinite(hi) else 0.0)


def build_table():
    """the arrays of tests/golden/negbin_link_truth.npz, from mpmath"""
    eta, theta, y = grid()
    tab = {q: np.zeros((2, len(eta))) for q in QUANTITIES}
    tab.update({"scale_" + q: np.zeros(len(eta), dtype=np.float32) for q in QUANTITIES})
    for i, (h, th, yy) in enumerate(zip(eta, theta, y)):
        v = values(h, th, yy)
        for q in QUANTITIES:
            tab[q][:, i] = split(v[q])
            # (rounded down, so that the float32 scale never flatters: at most 6e-8 below the true one)
            tab["scale_" + q][i] = np.nextafter(np.float32(float(v["scale_" + q])), np.float32(0.0))
    tab["thetas"] = thetas()
    # beyond the grid: float64 roundings of t, r_eta, r_theta (an overflow: +-inf) per (eta, theta, y); at 400 digits, since
    # d = eta - theta itself takes 300 digits there, and with no remainder to hold there is nothing for a second precision to check
    far = []
    for s in BEYOND:
        for h in (s, -s):
            for th in (-3.0, 1.0, 6.0):
                for yy in (0.0, 1.0, 7.0, 1e6):
                    v = dict(zip(NAMES, _at(h, th, yy, 400)))
                    far.append([h, th, yy] + [split(v[q])[0] for q in QUANTITIES])
    tab["beyond"] = np.array(far, dtype=np.float64)
    return tab


def write_table(path=GOLDEN):
    np.savez(path, **build_table())


def load_table(path=GOLDEN):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def ratio(got, tab, quantity):
    """|got - truth| / (eps scale) element-wise over the grid, the subnormal floor 2^-1070 taken off the error first; a NaN or a
    wrong infinity gives inf"""
    hi, lo = tab[quantity]
    sc = tab["scale_" + quantity].astype(np.float64)
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        err = np.where(np.isinf(hi) & (got == hi), 0.0, np.abs((got - hi) - lo))
        out = np.where(err <= FLOOR, 0.0, (err - FLOOR) / (EPS * sc))
    return np.where(np.isnan(got) | np.isnan(out), np.inf, out)


if __name__ == "__main__":
    write_table()
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
