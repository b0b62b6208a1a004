"""The element-wise truth of the GLM links (csrc/gsmvi_glm_link.h: t, r = dt / d eta, w = -dr / d eta), independent of the
kernel's forms, and the metric the links are held to ("The links element by element").  Test-only.

``values`` evaluates, with mpmath, the densities as include/gsmvi_hip.h writes them

    logistic  t = y eta - log(1 + e^eta)        poisson   t = y eta - e^eta
    probit    t = y log Phi(eta) + (1 - y) log Phi(-eta)        gaussian  t = -tau (y - eta)^2 / 2

and their derivatives in closed form.  The Bernoulli families are evaluated as the sum over the two labels that the written
density is for y in [0, 1], t = y log p(eta) + (1 - y) log p(-eta) with p = sigma or Phi from exp, log1p and erfc: no term of it
cancels (``written`` is the literal formula; tests/test_glm_link_truth_cpu.py holds the two together, and mp.diff of ``written``
to the closed-form derivatives, at moderate points).  No erfcx appears anywhere.  Every value is computed to 60 and to 120
digits (plus the guard digits the probit tail needs, ``_guard``) and the two must agree to 1e-40, or ``values`` raises.

``etas`` is the single source of points.  The committed table (tests/golden/glm_link_truth.npz) is what a machine without
mpmath needs to rebuild the truth of every grid row to 2^-106: t, r, w are affine in the label of a Bernoulli family and
f(-eta, y) = +-f(eta, 1 - y), so the table holds them at (|eta|, y = 1) and (|eta|, y = 0) as a float64 and its float64
remainder, w' as one float64, e^eta for the poisson family, and ``rows`` combines them in exact rational arithmetic; the gaussian
family is rational in its float64 inputs and needs no table.  Beside them: Phi(+-|eta|) (the probit mean), the float64 roundings
at the points beyond the grid, and the weights of the large-eta Hessian.  (The full grid, (eta, y, tau) by three quantities by value,
remainder and scale, is 700 KB; this form is 80 KB.)

The metric: the error of a computed f in {t, r, w} at (eta, y) is measured in units of

    eps (|f| + |eta f'(eta)| + a_f) + 2^-1070 / c

|eta f'|: what eta being a rounded number costs; a_f: the sum of the magnitudes of the terms the written definition adds
(logistic t: |y eta| + softplus, r: |y| + sigma; poisson t: |y eta| + e^eta, r: |y| + e^eta; probit t and r: the magnitudes of
the two label terms; a_w = 0; gaussian: 0, since y - eta is one subtraction of two given numbers); 2^-1070 covers subnormal
results.  ``ratio`` returns err / (eps scale) with the subnormal floor taken off first."""
import os
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
FLOOR = 2.0 ** -1070
SWITCH = 4.0                                    # LB_PROBIT_S0 of csrc/gsmvi_glm_link.h
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glm_link_truth.npz")
FAMILIES = ("logistic", "poisson", "probit", "gaussian")
LABELS = {"logistic": (0.0, 1.0, 0.3), "probit": (0.0, 1.0, 0.3), "poisson": (0.0, 1.0, 7.0, 1e6)}
TAUS = (0.5, 1.0, 3.0)
POISSON_MAX = 709.78                            # above it the flag rule applies
BEYOND = (1e160, 1e170, 1e300)                  # outside the table: no NaN, the sign of r, inf only where the truth overflows
HESS_SHAPE, HESS_SCALE, HESS_SEED = (5, 33, 16), 100.0, 49      # the large-eta Hessian: max|eta| in [1e4, 1e5]
FAR = 1e155                                     # probit: the asymptotic series of the tail instead of mpmath's erfc beyond it
# The worst ratio of the float64 restatements (glm_batched_ref.link, laplace_batched_ref.weights: numpy's exp, log, log1p and
# scipy's erfcx) over the whole grid, rounded up: asserted in tests/test_glm_link_truth_cpu.py, printed there, DESIGN.md section 9
C_CPU = {("logistic", "t"): 0.5, ("logistic", "r"): 0.5, ("logistic", "w"): 0.9, ("poisson", "t"): 0.5, ("poisson", "r"): 0.3,
         ("poisson", "w"): 0.6, ("probit", "t"): 3.0, ("probit", "r"): 2.9, ("probit", "w"): 24.0, ("gaussian", "t"): 1.0,
         ("gaussian", "r"): 0.5, ("gaussian", "w"): 0.0}
C_FLOOR, C_DEVICE = 16.0, 4.0                   # the GPU bound: max(16, 4 C_CPU); never from the device's own figures


def c_gpu(family, quantity):
    return max(C_FLOOR, C_DEVICE * C_CPU[family, quantity])


def magnitudes():
    fixed = [0.0, 5e-324, 1e-300, 1e-17, 1e-8, 1e-3, 0.5, 1.0, 2.0, 3.0, 5.0, np.nextafter(SWITCH, 0.0), SWITCH,
             np.nextafter(SWITCH, np.inf), 12.0, 20.0, 26.5, 37.5, 38.6, 40.0, 100.0, 700.0, 709.78, 745.0, 800.0, 1e4, 1e6, 1e8, 1e100,
             1e150]
    seeded = 10.0 ** np.random.RandomState(20261020).uniform(-3.0, 8.0, 200)
    return np.concatenate([np.array(fixed, dtype=np.float64), seeded])


def etas():
    """the grid: every magnitude with both signs (so 0 and -0)"""
    m = magnitudes()
    return np.concatenate([m, -m])


def gaussian_labels(eta):
    """y of the gaussian family at eta: 0, eta (1 + 1e-12), eta + 1, -eta"""
    return np.stack([np.zeros_like(eta), eta * (1.0 + 1e-12), eta + 1.0, -eta])


def hessian_problem():
    """the probit problems of the large-eta Hessian test: make_inputs at HESS_SHAPE with scale HESS_SCALE and seed HESS_SEED,
    the points x_k = X[k, 0]; returns (inputs, eta (K, N) rounded from np.longdouble, y (K, N), valid (K, N) by counts)"""
    import glm_batched_ref as gref
    inp = gref.make_inputs("probit", *HESS_SHAPE, 1, scale=HESS_SCALE, seed=HESS_SEED)
    A, y, o, counts = inp[:4]
    L = np.longdouble
    eta = (np.einsum("knd,kd->kn", A.astype(L), inp[6][:, 0, :].astype(L)) + o.astype(L)).astype(np.float64)
    return inp, eta, y, np.arange(A.shape[1])[None, :] < counts[:, None]


def hessian_truth(tab):
    """H_k = sum_n w_n a_n a_n^T + lam_k I of hessian_problem() with the table's weights, accumulated in np.longdouble"""
    inp, eta, y, valid = hessian_problem()
    assert np.array_equal(eta, tab["hessian_eta"])
    L = np.longdouble
    A, lam = inp[0].astype(L), inp[4]
    w = (tab["hessian_w"][..., 0].astype(L) + tab["hessian_w"][..., 1].astype(L)) * valid
    H = np.einsum("kn,kni,knj->kij", w, A, A) + lam.astype(L)[:, None, None] * np.eye(A.shape[2], dtype=L)
    return H


# ---- mpmath ---------------------------------------------------------------------------------------------------------------
def _guard(family, eta):
    """guard digits: on the probit tail h - |eta| ~ 1 / |eta| loses 2 log10|eta| digits, w = h (h - |eta|) ~ 1 - 1 / eta^2
    four, and w' ~ 2 / |eta|^3, from h ~ |eta| times w - 1, eight"""
    s = abs(float(eta))
    return 15 + (int(8 * np.log10(s)) + 1 if family == "probit" and s > 1.0 else 0)


def _at(family, eta, y, tau, dps):
    """(t, r, w, w', a_t, a_r) at working precision dps + guard"""
    import mpmath as mp
    with mp.workdps(dps + _guard(family, eta)):
        h, yy, one = mp.mpf(float(eta)), mp.mpf(float(y)), mp.mpf(1)
        if family == "logistic":
            sp, sm = one / (one + mp.exp(-h)), one / (one + mp.exp(h))             # sigma(eta), sigma(-eta)
            lp, lm = -mp.log1p(mp.exp(-h)), -mp.log1p(mp.exp(h))                  # their logarithms
            out = (yy * lp + (one - yy) * lm, yy * sm - (one - yy) * sp, sp * sm, sp * sm * (sm - sp),
                   abs(yy * h) - lm, abs(yy) + sp)
        elif family == "poisson":
            e = mp.exp(h)
            out = (yy * h - e, yy - e, e, e, abs(yy * h) + e, abs(yy) + e)
        elif family == "probit":
            rt2 = mp.sqrt(2)
            phi = mp.exp(-h * h / 2) / mp.sqrt(2 * mp.pi)
            if abs(h) <= FAR:
                cp, cm = mp.erfc(-h / rt2) / 2, mp.erfc(h / rt2) / 2               # Phi(eta), Phi(-eta)
            else:
                # mpmath's erfc does not take such an argument: Phi(-s) = phi(s) / s (1 - 1 / s^2 + 3 / s^4 - 15 / s^6 + ..), whose
                # error is below the first term left out, (2 n - 1)!! / s^(2 n) with n = 12: below 1e-1800
                s, term, ser = abs(h), one, one
                for n in range(1, 12):
                    term = -term * (2 * n - 1) / (s * s)
                    ser += term
                tail = phi / s * ser
                cp, cm = (one - tail, tail) if h > 0 else (tail, one - tail)
            lp = mp.log1p(-cm) if h >= 0 else mp.log(cp)
            lm = mp.log1p(-cp) if h < 0 else mp.log(cm)
            hp, hm = phi / cp, phi / cm
            wp, wm = hp * (hp + h), hm * (hm - h)
            dwp = -wp * (hp + h) + hp * (one - wp)                                  # hp' = -wp, hm' = wm
            dwm = wm * (hm - h) + hm * (wm - one)
            out = (yy * lp + (one - yy) * lm, yy * hp - (one - yy) * hm, yy * wp + (one - yy) * wm, yy * dwp + (one - yy) * dwm,
                   abs(yy * lp) + abs((one - yy) * lm), abs(yy * hp) + abs((one - yy) * hm))
        elif family == "gaussian":
            tt, d = mp.mpf(float(tau)), yy - h
            out = (-tt * d * d / 2, tt * d, tt, mp.mpf(0), mp.mpf(0), mp.mpf(0))
        else:
            raise ValueError(family)
        return out


def values(family, eta, y, tau=1.0):
    """{"t", "r", "w", "dw", "a_t", "a_r"} as mpf at (eta, y, tau): computed to 60 and to 120 digits, which must agree to
    1e-40 relative (raises ArithmeticError otherwise); the 120-digit values are returned"""
    import mpmath as mp
    lo, hi = _at(family, eta, y, tau, 60), _at(family, eta, y, tau, 120)
    with mp.workdps(150):
        for name, a, b in zip(("t", "r", "w", "dw", "a_t", "a_r"), lo, hi):
            if abs(a - b) > mp.mpf(10) ** -40 * abs(b):
                raise ArithmeticError(f"{family} {name} at eta = {eta!r}, y = {y!r}: 60 and 120 digits disagree: {a} {b}")
    return dict(zip(("t", "r", "w", "dw", "a_t", "a_r"), hi))


def cdf(eta):
    """Phi(eta) as an mpf, to 60 and to 120 digits, which must agree to 1e-40"""
    import mpmath as mp
    out = []
    for dps in (60, 120):
        with mp.workdps(dps + _guard("probit", eta)):             # (exp(-eta^2 / 2) needs 2 log10|eta| digits of them)
            h = mp.mpf(float(eta))
            out.append(mp.erfc(-h / mp.sqrt(2)) / 2 if h < 0 else 1 - mp.erfc(h / mp.sqrt(2)) / 2)
    if abs(out[0] - out[1]) > mp.mpf(10) ** -40 * abs(out[1]):
        raise ArithmeticError(f"Phi at eta = {eta!r}: 60 and 120 digits disagree")
    return out[1]


def written(family, eta, y, tau=1.0):
    """t of the density as written, literally, as a function of an mpf eta (for mp.diff and the comparison with ``values``)"""
    import mpmath as mp
    y, tau = mp.mpf(float(y)), mp.mpf(float(tau))
    if family == "logistic":
        return y * eta - mp.log(1 + mp.exp(eta))
    if family == "poisson":
        return y * eta - mp.exp(eta)
    if family == "probit":
        return y * mp.log(mp.ncdf(eta)) + (1 - y) * mp.log(mp.ncdf(-eta))
    if family == "gaussian":
        return -tau * (y - eta) ** 2 / 2
    raise ValueError(family)


def split(v):
    """an mpf or a Fraction as (float64 nearest, float64 remainder); an overflow stays +-inf with remainder 0"""
    if isinstance(v, Fraction):
        try:
            hi = float(v)
        except OverflowError:
            return (np.inf if v > 0 else -np.inf), 0.0
        return hi, float(v - Fraction(hi))
    import mpmath as mp
    with mp.workdps(150):
        hi = float(v)
        return hi, (float(v - mp.mpf(hi)) if np.isfinite(hi) else 0.0)


def scales(f, eta, a_t=0.0, a_r=0.0):
    """the three scales |f| + |eta f'| + a_f from t, r, w, dw (t' = r, r' = -w), in the arithmetic of the arguments"""
    e = abs(eta)
    return abs(f["t"]) + e * abs(f["r"]) + a_t, abs(f["r"]) + e * abs(f["w"]) + a_r, abs(f["w"]) + e * abs(f["dw"])


def build_table():
    """the arrays of tests/golden/glm_link_truth.npz, from mpmath"""
    m = magnitudes()
    tab = {"magnitudes": m, "switch": np.array([SWITCH])}
    for family in ("logistic", "probit"):
        b = np.zeros((2, 7, len(m)))                                                # label 1, label 0; t r w (hi, lo), w'
        for i, s in enumerate(m):
            for j, y in enumerate((1.0, 0.0)):
                v = values(family, s, y)
                for q, name in enumerate("trw"):
                    b[j, 2 * q, i], b[j, 2 * q + 1, i] = split(v[name])
                b[j, 6, i] = float(v["dw"])
        tab[family] = b
    # Phi(|eta|) and Phi(-|eta|), value and remainder: the probit family's mean (the predictive's pmean)
    tab["probit_cdf"] = np.array([[split(cdf(h)) for h in m], [split(cdf(-h)) for h in m]])
    e = etas()
    e = e[e <= POISSON_MAX]
    tab["poisson_eta"] = e
    tab["poisson_exp"] = np.array([split(values("poisson", h, 0.0)["w"]) for h in e]).T.copy()
    # beyond the table: float64 roundings of t, r, w (an overflow: +-inf) and the sign of r, per (family, eta, y)
    far = []
    for fi, family in enumerate(FAMILIES):
        for s in BEYOND:
            for h in (s, -s):
                if family == "poisson" and h > POISSON_MAX:
                    continue
                ys = gaussian_labels(np.array([h]))[:, 0] if family == "gaussian" else LABELS[family]
                for y in ys:
                    v = values(family, h, y, 1.0)
                    far.append([fi, h, y] + [split(v[name])[0] for name in "trw"] + [float((v["r"] > 0) - (v["r"] < 0))])
    tab["beyond"] = np.array(far, dtype=np.float64)
    # the realistic-shape Hessian: the probit weights at the float64 eta of hessian_problem(), value and remainder
    eta, y = hessian_problem()[1:3]
    tab["hessian_eta"] = eta
    tab["hessian_w"] = np.array([[split(values("probit", h, yy)["w"]) for h, yy in zip(er, yr)] for er, yr in zip(eta, y)])
    return tab


def write_table(path=GOLDEN):
    np.savez(path, **build_table())


def load_table(path=GOLDEN):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


# ---- without mpmath: the grid's rows from the table, in exact rational arithmetic ----------------------------------------------
def _frac(hi, lo):
    return Fraction(float(hi)) + Fraction(float(lo))


def rows(tab, family):
    """every grid row of ``family`` as a dict of float64 arrays: eta, y, tau, t, t_lo, r, r_lo, w, w_lo (value and remainder)
    and scale_t, scale_r, scale_w; eta-major within each label (and each tau, gaussian)"""
    out = {k: [] for k in ("eta", "y", "tau", "t", "t_lo", "r", "r_lo", "w", "w_lo", "scale_t", "scale_r", "scale_w")}

    def put(eta, y, tau, f, a_t, a_r):
        st, sr, sw = scales(f, Fraction(float(eta)), a_t, a_r)
        for name, v in (("t", f["t"]), ("r", f["r"]), ("w", f["w"])):
            out[name], out[name + "_lo"] = out[name] + [split(v)[0]], out[name + "_lo"] + [split(v)[1]]
        for name, v in (("eta", eta), ("y", y), ("tau", tau), ("scale_t", split(st)[0]), ("scale_r", split(sr)[0]),
                        ("scale_w", split(sw)[0])):                     # (poisson near 709.78: |eta e^eta| overflows, scale = inf)
            out[name].append(float(v))

    if family in ("logistic", "probit"):
        m, b = tab["magnitudes"], tab[family]
        for y in LABELS[family]:
            yf = Fraction(y)
            for sign in (1.0, -1.0):
                for i, s in enumerate(m):
                    # f(eta, 1), f(eta, 0) at eta = sign s: f(-s, 1) = f(s, 0) for t, w; r and w' change sign with it
                    j1, j0, sg = (0, 1, 1) if sign > 0 else (1, 0, -1)
                    one = {"t": _frac(b[j1, 0, i], b[j1, 1, i]), "r": sg * _frac(b[j1, 2, i], b[j1, 3, i]),
                           "w": _frac(b[j1, 4, i], b[j1, 5, i]), "dw": sg * Fraction(float(b[j1, 6, i]))}
                    zero = {"t": _frac(b[j0, 0, i], b[j0, 1, i]), "r": sg * _frac(b[j0, 2, i], b[j0, 3, i]),
                            "w": _frac(b[j0, 4, i], b[j0, 5, i]), "dw": sg * Fraction(float(b[j0, 6, i]))}
                    f = {k: yf * one[k] + (1 - yf) * zero[k] for k in one}
                    eta = sign * s
                    if family == "logistic":                            # softplus(eta) = -t(eta, 0), sigma(eta) = -r(eta, 0)
                        a_t, a_r = abs(yf * Fraction(float(eta))) - zero["t"], abs(yf) - zero["r"]
                    else:
                        a_t = abs(yf * one["t"]) + abs((1 - yf) * zero["t"])
                        a_r = abs(yf * one["r"]) + abs((1 - yf) * zero["r"])
                    put(eta, y, 1.0, f, a_t, a_r)
    elif family == "poisson":
        for y in LABELS[family]:
            yf = Fraction(y)
            for eta, hi, lo in zip(tab["poisson_eta"], *tab["poisson_exp"]):
                e, h = _frac(hi, lo), Fraction(float(eta))
                put(eta, y, 1.0, {"t": yf * h - e, "r": yf - e, "w": e, "dw": e}, abs(yf * h) + e, abs(yf) + e)
    elif family == "gaussian":
        e = etas()
        for tau in TAUS:
            for ys in gaussian_labels(e):
                for eta, y in zip(e, ys):
                    d, tf = Fraction(float(y)) - Fraction(float(eta)), Fraction(tau)
                    put(eta, y, tau, {"t": -tf * d * d / 2, "r": tf * d, "w": tf, "dw": Fraction(0)}, 0, 0)
    else:
        raise ValueError(family)
    return {k: np.array(v, dtype=np.float64) for k, v in out.items()}


def ratio(got, row, quantity):
    """|got - truth| / (eps scale) element-wise over the rows of ``rows``, the subnormal floor 2^-1070 taken off the error first;
    a NaN or a wrong infinity gives inf"""
    hi, lo, sc = row[quantity], row[quantity + "_lo"], row["scale_" + quantity]
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        err = np.where(np.isinf(hi) & (got == hi), 0.0, np.abs((got - hi) - lo))
        out = np.where(err <= FLOOR, 0.0, (err - FLOOR) / (EPS * sc))
    return np.where(np.isnan(got) | np.isnan(out), np.inf, out)


if __name__ == "__main__":
    write_table()
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
