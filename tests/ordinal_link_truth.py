"""The element-wise truth of the ordinal (cumulative logit) link (csrc/gsmvi_ordinal_link.h) for C = 3 classes, independent of the
kernel's forms, and the metric it is held to ("Batched ordinal target").  Test-only, in the style of
tests/negbin_link_truth.py.

``values`` evaluates with mpmath, at the float64 inputs (eta, delta_0, delta_1) and the label y in {0, 1, 2}, the density as it is
written, cut_0 = delta_0, cut_1 = delta_0 + e^{delta_1}, cut_{-1} = -inf, cut_2 = +inf:

    t = log( sigma(cut_y - eta) - sigma(cut_{y-1} - eta) )

and its partial derivatives dt / d eta, dt / d delta_0, dt / d delta_1 (``re``, ``d0``, ``d1``: what one observation adds to the
components P - 1 + ... of the score at P = 1, A = 1, beta = 0), from sigma' = sigma(x) sigma(-x) and the quotient rule on that
difference: no product identity, no log1mexp, no expm1.  The difference is taken as sigma(b) - sigma(a) or, where a > 0, as the equal
sigma(-a) - sigma(-b) (1 - sigma(x) is sigma(-x)): at e^{delta_1} = 1e304 the top class has sigma(a) = 1 - e^{-1e304}, which no
working precision holds.  Everything runs to 60 and to 120 digits plus 700 guard digits (at eta - delta_0 = 700, delta_1 = -700 the
difference is 1e-608 of its terms), which must agree to 1e-40 of the scale below, or it raises.

``grid`` is the single source of points: y in {0, 1, 2} x delta_0 in D0_VALUES x (eta - delta_0) in H_VALUES x delta_1 in
``delta1s()`` (both sides of log log 2, where log1mexp changes its form, among them), eta = (eta - delta_0) + delta_0 rounded to
float64.  The committed table (tests/golden/ordinal_link_truth.npz) holds per grid point the value and the float64 remainder of the
four quantities (float64) and their scales (a float32 mantissa and an int16 exponent: a scale needs no more), so that the GPU test needs no mpmath.

The metric: the error of a computed f in {t, re, d0, d1} is measured in units of

    eps (|f| + |eta df/d eta| + |delta_0 df/d delta_0| + |delta_1 df/d delta_1| + a_f) + 2^-1070

the three products: what the inputs being rounded numbers costs; a_f: the sum of the magnitudes of the terms of the forms of
csrc/gsmvi_ordinal_link.h, with L = log1mexp(w) and Q = 1 / expm1(w) of the gap w = e^{delta_1} as primitives (an interior class;
0 otherwise):  a_t = softplus(-b) + softplus(a) + |L|,  a_re = sigma(a) + sigma(-b),  a_d0 = sigma(a) + sigma(-b) + 2 Q,
a_d1 = w ([y = 2] sigma(a) + [y = 1] (sigma(-b) + Q)), a term of a class without an a or a b being 0.  Taking L and Q as primitives
is deliberate: a scale built from sigma(b) and sigma(a) separately would admit the naive difference of two probabilities.  ``ratio``
returns err / (eps scale) with the subnormal floor taken off first."""
import os

import numpy as np

EPS = 2.0 ** -52
FLOOR = 2.0 ** -1070
LOGLOG2 = -0.36651292058166435                  # log log 2: w = e^{delta_1} crosses log 2 here
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ordinal_link_truth.npz")
H_VALUES = (-700.0, -40.0, -5.0, -1.0, 0.0, 0.5, 3.0, 20.0, 700.0)
D0_VALUES = (0.0, 30.0, -30.0, 1.25)
QUANTITIES = ("t", "re", "d0", "d1")
BEYOND = (1e160, 1e300)                         # |eta| outside the grid: no NaN, the sign of r_eta, inf only where the truth overflows
GUARD = 700
# The worst ratio of the float64 restatement (ordinal_batched_ref.link3: numpy's exp, expm1, log, log1p) over the whole grid, rounded
# up: asserted in tests/test_ordinal_batched_cpu.py, printed there, DESIGN.md section 9
C_CPU = {"t": 0.5, "re": 0.4, "d0": 0.4, "d1": 0.6}
C_FLOOR, C_DEVICE = 16.0, 4.0                   # the GPU bound: max(16, 4 C_CPU); never from the device's own figures


def c_gpu(quantity):
    return max(C_FLOOR, C_DEVICE * C_CPU[quantity])


def delta1s():
    return np.array([-700.0, -30.0, -10.0, -1.0, np.nextafter(LOGLOG2, -1.0) - 1e-14, LOGLOG2 + 1e-14, 0.0, 1.0, 3.0, 6.5, 700.0],
                    dtype=np.float64)


def grid():
    """(eta, delta_0, delta_1, y) of every grid point, y-major, then delta_0, then eta - delta_0, then delta_1"""
    y, d0, h, d1 = np.meshgrid(np.arange(3), np.array(D0_VALUES), np.array(H_VALUES), delta1s(), indexing="ij")
    return (h + d0).ravel(), d0.ravel().copy(), d1.ravel().copy(), y.ravel().astype(np.int64)


# ---- mpmath ---------------------------------------------------------------------------------------------------------------
def written(eta, delta, y):
    """t of the density as written, literally, for any C: delta a list of C - 1 mpf, eta an mpf (for mp.diff)"""
    import mpmath as mp
    cuts = [delta[0]]
    for d in delta[1:]:
        cuts.append(cuts[-1] + mp.exp(d))
    sig = lambda x: 1 / (1 + mp.exp(-x))                                           # noqa: E731
    hi = sig(cuts[y] - eta) if y <= len(cuts) - 1 else mp.mpf(1)
    lo = sig(cuts[y - 1] - eta) if y >= 1 else mp.mpf(0)
    return mp.log(hi - lo)


def _at(eta, d0, d1, y, dps):
    """(t, re, d0, d1, scale_t, scale_re, scale_d0, scale_d1) at working precision dps + GUARD digits"""
    import mpmath as mp
    with mp.workdps(dps + GUARD):
        h, c0, dl, one, zero = mp.mpf(float(eta)), mp.mpf(float(d0)), mp.mpf(float(d1)), mp.mpf(1), mp.mpf(0)
        w = mp.exp(dl)
        sig = lambda x: one / (one + mp.exp(-x))                                   # noqa: E731
        lo, hi = y >= 1, y <= 1
        a = ((c0 if y == 1 else c0 + w) - h) if lo else None
        b = ((c0 if y == 0 else c0 + w) - h) if hi else None
        # the difference of the two probabilities, on the side where neither is a rounded 1
        if not lo:
            p = sig(b)
        elif not hi:
            p = sig(-a)
        else:
            p = sig(-a) - sig(-b) if a > 0 else sig(b) - sig(a)
        s1 = lambda x: sig(x) * sig(-x)                                            # noqa: E731  sigma'
        s2 = lambda x: s1(x) * (sig(-x) - sig(x))                                  # noqa: E731  sigma''
        ta = -s1(a) / p if lo else zero
        tb = s1(b) / p if hi else zero
        taa = -s2(a) / p - ta * ta if lo else zero
        tbb = s2(b) / p - tb * tb if hi else zero
        tab = s1(a) * s1(b) / (p * p) if lo and hi else zero
        # a and b as functions of (eta, delta_0, delta_1): gradients ja, jb, and the one second derivative d2 cut_1 / d delta_1^2 = w
        ja = [-one, one, w if y == 2 else zero] if lo else [zero] * 3
        jb = [-one, one, w if y == 1 else zero] if hi else [zero] * 3
        t = mp.log(p)
        g = [ta * ja[i] + tb * jb[i] for i in range(3)]
        H = [[taa * ja[i] * ja[j] + tbb * jb[i] * jb[j] + tab * (ja[i] * jb[j] + jb[i] * ja[j]) for j in range(3)] for i in range(3)]
        H[2][2] += (ta if y == 2 else zero) * w + (tb if y == 1 else zero) * w
        x = [abs(h), abs(c0), abs(dl)]
        # the terms of the forms
        inner = lo and hi
        L = abs(mp.log(one - mp.exp(-w))) if inner else zero
        Q = one / mp.expm1(w) if inner else zero
        sga, sgb = (sig(a) if lo else zero), (sig(-b) if hi else zero)
        spa = -mp.log(sig(-a)) if lo else zero                                     # softplus(a)
        spb = -mp.log(sig(b)) if hi else zero                                      # softplus(-b)
        a_f = [spb + spa + L, sga + sgb, sga + sgb + 2 * Q, w * (sga if y == 2 else (sgb + Q if y == 1 else zero))]
        f = [t] + g
        dfs = [g] + H
        scales = [abs(f[i]) + sum(x[j] * abs(dfs[i][j]) for j in range(3)) + a_f[i] for i in range(4)]
        return tuple(f) + tuple(scales)


NAMES = QUANTITIES + tuple("scale_" + q for q in QUANTITIES)


def values(eta, d0, d1, y):
    """{"t", "re", "d0", "d1", "scale_..."} as mpf: computed to 60 and to 120 digits (plus the guard), which must agree to 1e-40
    of the quantity's scale (raises ArithmeticError otherwise); the 120-digit values are returned"""
    import mpmath as mp
    lo, hi = _at(eta, d0, d1, y, 60), _at(eta, d0, d1, y, 120)
    with mp.workdps(170 + GUARD):
        for i, (name, a, b) in enumerate(zip(NAMES, lo, hi)):
            if abs(a - b) > mp.mpf(10) ** -40 * hi[4 + i % 4]:
                raise ArithmeticError(f"{name} at eta = {eta!r}, delta = ({d0!r}, {d1!r}), y = {y}: 60 and 120 digits disagree: {a} {b}")
    return dict(zip(NAMES, hi))


def split(v):
    """an mpf as (float64 nearest, float64 remainder); an overflow stays +-inf with remainder 0"""
    import mpmath as mp
    with mp.workdps(170 + GUARD):
        hi = float(v)
        return hi, (float(v - mp.mpf(hi)) if np.isfinite(hi) else 0.0)


def pack_scale(v):
    """a scale as (float32 mantissa in [0.5, 1), int16 binary exponent): the scales run from 1e-300 to 1e307, outside float32's
    range.  The mantissa is rounded down, so that the stored scale never flatters: at most 1.2e-7 below the true one."""
    m, e = np.frexp(min(float(v), 1.7e308))
    return np.nextafter(np.float32(m), np.float32(0.0)), np.int16(e)


def unpack_scale(tab, quantity):
    return np.ldexp(tab["scale_" + quantity].astype(np.float64), tab["scexp_" + quantity].astype(np.int64))


def beyond_points():
    """(eta, delta_0, delta_1, y) beyond the grid: |eta| = 1e160 and 1e300"""
    return [(h, c0, d1, y) for s in BEYOND for h in (s, -s) for c0 in (-30.0,) for d1 in (-3.0, 1.0, 6.0) for y in (0, 1, 2)]


def build_table():
    """the arrays of tests/golden/ordinal_link_truth.npz, from mpmath"""
    eta, d0, d1, y = grid()
    tab = {q: np.zeros((2, len(eta))) for q in QUANTITIES}
    tab.update({"scale_" + q: np.zeros(len(eta), dtype=np.float32) for q in QUANTITIES})
    tab.update({"scexp_" + q: np.zeros(len(eta), dtype=np.int16) for q in QUANTITIES})
    for i in range(len(eta)):
        v = values(eta[i], d0[i], d1[i], int(y[i]))
        for q in QUANTITIES:
            tab[q][:, i] = split(v[q])
            tab["scale_" + q][i], tab["scexp_" + q][i] = pack_scale(v["scale_" + q])
    tab["delta1s"] = delta1s()
    # beyond the grid: float64 roundings of the four quantities (an overflow: +-inf) per point; at 400 digits plus the guard, since
    # cut - eta itself takes 300 digits there, and with no remainder to hold there is nothing for a second precision to check
    far = []
    for h, c0, dl, yy in beyond_points():
        v = dict(zip(NAMES, _at(h, c0, dl, yy, 400)))
        far.append([h, c0, dl, yy] + [split(v[q])[0] for q in QUANTITIES])
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
    sc = unpack_scale(tab, quantity)
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        err = np.where(np.isinf(hi) & (got == hi), 0.0, np.abs((got - hi) - lo))
        out = np.where(err <= FLOOR, 0.0, (err - FLOOR) / (EPS * sc))
    return np.where(np.isnan(got) | np.isnan(out), np.inf, out)


if __name__ == "__main__":
    write_table()
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
