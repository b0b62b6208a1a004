"""The element-wise truth of the curvature of the ordinal (cumulative logit) link (csrc/gsmvi_ordinal_link.h, the forms of
csrc/gsmvi_ordinal_laplace_batched.hip) for C = 3 classes, independent of the kernel's forms, and the metric it is held to
("Ordinal Laplace initialiser").  Test-only, in the style of tests/ordinal_link_truth.py, whose grid it uses.

``values`` evaluates with mpmath, at the float64 inputs (eta, delta_0, delta_1) and the label y in {0, 1, 2}, the six entries of the
negative Hessian of the density as it is written, t = log(sigma(cut_y - eta) - sigma(cut_{y-1} - eta)), in (eta, delta_0, delta_1):

    hee, he0, he1, h00, h01, h11 = -d2 t / d(eta, delta_0, delta_1)^2        (upper triangle, row-major)

from sigma' = sigma(x) sigma(-x), sigma'' and the quotient rule on that difference of probabilities (taken on the side where
neither is a rounded 1, as in ordinal_link_truth): no gap coordinates, no expm1, no sum of positive semi-definite terms.  They are
what one observation gives as H of gsmvi_ordinal_hessian_batched_f64 at N = 1, P = 1, A = 1, beta = 0, the offset eta, no priors.
Everything runs to 60 and to 120 digits plus GUARD guard digits, which must agree to 1e-40 of the scale below, or
it raises.  The committed table (tests/golden/ordinal_curv_truth.npz) holds per grid point the value and the float64 remainder of
the six quantities and their scales (a float32 mantissa and an int16 exponent), so that the GPU test needs no mpmath.

The metric is ordinal_link_truth's: the error of a computed f is measured in units of

    eps (|f| + |eta df/d eta| + |delta_0 df/d delta_0| + |delta_1 df/d delta_1| + a_f) + 2^-1070

(the three derivatives by mpmath's numerical differentiation of the analytic second derivatives, at the lower precision: a scale
needs few digits) with a_f the sum of the magnitudes of the terms of the kernel's forms, Q = 1 / expm1(w) of the gap w = e^{delta_1}
as a primitive (an interior class; 0 otherwise), fa = sigma(a) sigma(-a), fb = sigma(b) sigma(-b), e_1 = fa (y = 2), fb (y = 1), 0:
    a_hee = a_he0 = a_h00 = fa + fb,     a_he1 = a_h01 = w e_1,
    a_h11 = w^2 e_1 + [y = 1] (w Q)(w + w Q) + w ([y = 2] sigma(a) + [y = 1] (sigma(-b) + Q))
A point whose truth overflows float64 is held to the same infinity (``ratio``)."""
import os

import numpy as np

from ordinal_link_truth import grid, pack_scale, unpack_scale, ratio, load_table as _load, EPS, FLOOR   # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ordinal_curv_truth.npz")
# guard digits: at eta - delta_0 = -700, delta_1 = -700 the difference of the two probabilities is 1e-608 of its terms and the second
# derivatives square that ratio: terms of 1e608 leave a value of 1e-304
GUARD = 1400
QUANTITIES = ("hee", "he0", "he1", "h00", "h01", "h11")
INDEX = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))        # of H (3 x 3) at P = 1, C = 3
# The worst ratio of the float64 restatement (ordinal_laplace_ref.evaluate: numpy's exp, expm1, log1p) over the whole grid, rounded
# up: asserted in tests/test_ordinal_laplace_cpu.py, printed there, DESIGN.md section 9
C_CPU = {"hee": 0.6, "he0": 0.6, "he1": 0.6, "h00": 0.6, "h01": 0.6, "h11": 0.7}
C_FLOOR, C_DEVICE = 16.0, 4.0                   # the GPU bound: max(16, 4 C_CPU); never from the device's own figures


def c_gpu(quantity):
    return max(C_FLOOR, C_DEVICE * C_CPU[quantity])


def _hess(h, c0, dl, y):
    """the six entries of -grad^2 t in (eta, delta_0, delta_1) and the a_f of each, at the current working precision (mpf in)"""
    import mpmath as mp
    one, zero = mp.mpf(1), mp.mpf(0)
    w = mp.exp(dl)
    sig = lambda x: one / (one + mp.exp(-x))                                   # noqa: E731
    lo, hi = y >= 1, y <= 1
    a = ((c0 if y == 1 else c0 + w) - h) if lo else None
    b = ((c0 if y == 0 else c0 + w) - h) if hi else None
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
    ja = [-one, one, w if y == 2 else zero] if lo else [zero] * 3
    jb = [-one, one, w if y == 1 else zero] if hi else [zero] * 3
    H = [[taa * ja[i] * ja[j] + tbb * jb[i] * jb[j] + tab * (ja[i] * jb[j] + jb[i] * ja[j]) for j in range(3)] for i in range(3)]
    H[2][2] += (ta if y == 2 else zero) * w + (tb if y == 1 else zero) * w
    f = [-H[i][j] for i, j in INDEX]
    fa, fb = (s1(a) if lo else zero), (s1(b) if hi else zero)
    Q = one / mp.expm1(w) if lo and hi else zero
    e1 = fa if y == 2 else (fb if y == 1 else zero)
    sga, sgb = (sig(a) if lo else zero), (sig(-b) if hi else zero)
    a11 = w * w * e1 + (w * Q) * (w + w * Q) + w * (sga if y == 2 else (sgb + Q if y == 1 else zero))
    return f, [fa + fb, fa + fb, w * e1, fa + fb, w * e1, a11]


def _at(eta, d0, d1, y, dps, scales):
    import mpmath as mp
    with mp.workdps(dps + GUARD):
        x = [mp.mpf(float(eta)), mp.mpf(float(d0)), mp.mpf(float(d1))]
        f, a_f = _hess(x[0], x[1], x[2], y)
        if not scales:
            return f, None
        sc = []
        for i in range(6):
            cond = mp.mpf(0)
            for j in range(3):
                if x[j] != 0:
                    cond += abs(x[j]) * abs(mp.diff(lambda v, i=i, j=j: _hess(*[v if m == j else x[m] for m in range(3)], y)[0][i], x[j]))
            sc.append(abs(f[i]) + cond + a_f[i])
        return f, sc


def values(eta, d0, d1, y):
    """{"hee", .., "scale_hee", ..} as mpf: the six entries computed to 60 and to 120 digits (plus the guard), which must agree to
    1e-40 of the quantity's scale (raises ArithmeticError otherwise); the 120-digit values are returned"""
    import mpmath as mp
    (lo, sc), (hi, _) = _at(eta, d0, d1, y, 60, True), _at(eta, d0, d1, y, 120, False)
    with mp.workdps(170 + GUARD):
        for name, a, b, s in zip(QUANTITIES, lo, hi, sc):
            if abs(a - b) > mp.mpf(10) ** -40 * s:
                raise ArithmeticError(f"{name} at eta = {eta!r}, delta = ({d0!r}, {d1!r}), y = {y}: 60 and 120 digits disagree: {a} {b}")
    out = dict(zip(QUANTITIES, hi))
    out.update({"scale_" + q: s for q, s in zip(QUANTITIES, sc)})
    return out


def split(v):
    """an mpf as (float64 nearest, float64 remainder); an overflow stays +-inf with remainder 0"""
    import mpmath as mp
    with mp.workdps(170 + GUARD):
        hi = float(v)
        return hi, (float(v - mp.mpf(hi)) if np.isfinite(hi) else 0.0)


def _point(args):
    """one grid point as plain floats: [(value, remainder, scale mantissa, scale exponent) per quantity]"""
    v = values(*args)
    return [split(v[q]) + pack_scale(v["scale_" + q]) for q in QUANTITIES]


def build_table(processes=1):
    """the arrays of tests/golden/ordinal_curv_truth.npz, from mpmath (``processes`` > 1: the grid points in a process pool)"""
    eta, d0, d1, y = grid()
    pts = [(float(eta[i]), float(d0[i]), float(d1[i]), int(y[i])) for i in range(len(eta))]
    if processes > 1:
        import multiprocessing
        with multiprocessing.Pool(processes) as pool:
            rows = pool.map(_point, pts, chunksize=8)
    else:
        rows = [_point(p) for p in pts]
    tab = {q: np.zeros((2, len(eta))) for q in QUANTITIES}
    tab.update({"scale_" + q: np.zeros(len(eta), dtype=np.float32) for q in QUANTITIES})
    tab.update({"scexp_" + q: np.zeros(len(eta), dtype=np.int16) for q in QUANTITIES})
    for i, row in enumerate(rows):
        for q, (hi, lo, m, e) in zip(QUANTITIES, row):
            tab[q][:, i] = hi, lo
            tab["scale_" + q][i], tab["scexp_" + q][i] = m, e
    return tab


def write_table(path=GOLDEN, processes=1):
    np.savez_compressed(path, **build_table(processes))


def load_table(path=GOLDEN):
    return _load(path)


def problems():
    """the truth grid as one problem per point: A (K, 1, 1) = 1, labels (K, 1), offset (K, 1) = eta, X (K, 3) = (0, d0, d1)"""
    eta, d0, d1, y = grid()
    K = len(eta)
    return np.ones((K, 1, 1)), y.astype(np.int32)[:, None], eta[:, None], np.stack([np.zeros(K), d0, d1], axis=1)


def entries(H):
    """{quantity: (K,)} from H (K, 3, 3)"""
    return {q: H[:, i, j] for q, (i, j) in zip(QUANTITIES, INDEX)}


if __name__ == "__main__":
    import sys
    write_table(processes=int(sys.argv[1]) if len(sys.argv) > 1 else 1)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
