"""The element-wise truth of the multinomial logit link (csrc/gsmvi_softmax_model.h: m, z, log z, p and 1 - p of the four softmax
kernels), independent of the kernels' forms, the single source of points, the layouts that turn the public entry points into
link probes, and the metric the link is held to ("The softmax block element by element").  Test-only; the
counterpart of glm_link_truth.py.

``values`` evaluates, with mpmath, for a vector eta of C entries whose last is fixed at 0 (the reference class)

    lse = log sum_c e^eta_c,    p_c = e^eta_c / sum,    q_c = sum_{c' != c} p_c'     (1 - p_c AS A SUM, never 1 - p)

so that no term cancels: the maximum m is taken out, the non-maximal e^(eta_c - m) are summed (``rest``; the first class that
attains m counts as the maximal term, exactly 1), lse = m + log1p(rest), and q_c is the sum of the other terms over 1 + rest,
from prefix and suffix sums.  Every value is computed to 60 and to 120 digits (plus the guard digits eta_c - m and e^(eta_c - m)
need at a large |eta|) and the two must agree to 1e-40 relative, or ``values`` raises.  (log(1 + rest) at a fixed 80 digits is
wrong at eta = -700: the trap this module exists to keep out.)

Everything else is affine or bilinear in these and the label y:

    t = eta_y - lse,    r_c = [y = c] - p_c  with  r_y = q_y,    w_cc = p_c q_c,    w_cc' = -p_c p_c'  (c != c')

The committed table (tests/golden/softmax_link_truth.npz) holds lse, p and q per vector, each as a float64 and its float64
remainder; ``rows`` rebuilds t, r and w from them in exact rational arithmetic (t in Fractions; r is a copy of -p or q; a product
of two table entries is a product of two integers over 2^2148), so a machine without mpmath has every value to 2^-106.

The metric is the project's: the error of a computed f is measured in units of

    eps (|f| + sum_c |eta_c df/deta_c| + a_f) + 2^-1070

with a_t = |eta_y| + |lse|, a_r = [y = c] + p_c, a_p = a_w = 0: the magnitudes of the terms the written definition adds.  There
is no "+1 for the rounding of z" in a_t: z rounds to 1 exactly where the reference class wins by more than 1 / eps, and the
definition's t = -log(1 + rest) is then -rest, not 0; the logistic link is held without that term too.  The scales are sums of
non-negative float64 terms (no subtraction: sum_{j != c} |eta_j| p_j comes from prefix and suffix sums), so they carry a relative
error of a few eps, which a bound of 16 units does not see.  ``ratio`` returns err / (eps scale) with the floor taken off first."""
import functools
import os
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
FLOOR = 2.0 ** -1070
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "softmax_link_truth.npz")
# (C, P): one, two and eight classes per lane of the Laplace kernel; the four-problem and the 256-thread packings; P % 4 != 0 for
# the padded MFMA chain; D = 64
SHAPES = ((2, 1), (3, 1), (3, 3), (9, 3), (17, 1), (65, 1))
MAGNITUDES = (0.0, 5e-324, 1e-300, 1e-17, 1e-3, 0.5, 1.0, 3.0, 12.0, 20.0, 36.0, 37.5, 40.0, 100.0, 700.0, 709.78, 745.0, 800.0,
              1e4, 1e8, 1e150)
# The magnitudes kept at C = 65.  None lies in the band 708.4 < h < 745.2 where e^-h is a subnormal number: there a float64 e^-h
# carries up to half a subnormal ulp, 64 equal terms carry it 64 times, and any float64 sum of them can be 2^-1069 from the truth,
# past the metric's floor of 2^-1070 (16 subnormal ulps: sums of up to 32 such terms) by the number format alone.  The band is
# covered at C <= 17, where at most 16 such terms meet.
DOZEN = (0.0, 1e-17, 1e-3, 1.0, 12.0, 36.0, 37.5, 40.0, 700.0, 800.0, 1e4, 1e150)
DELTAS = (1e-3, 1.0, 40.0)
SEEDED, SEED = 100, 20261020
FILLER = (1.0, -2.0)                            # x entries that meet the zero features of a P = 3 row
# beyond the table's grid (P = 1): no NaN, the signs of r, p exactly 0 or 1 where the truth rounds to that
BEYOND = {2: ((1e160,), (-1e160,), (1e300,), (-1e300,)),
          3: ((1e160, -1e300), (-1e160, -1e300), (1e300, 1e300), (1e160, 1e300), (-1e300, 1e160), (-1e300, 0.0))}
BEYOND_A = 1e150                                # eta = BEYOND_A x there, so that |x|^2 stays finite (lam |x|^2 / 2 is formed with lam = 0)
REAL_SHAPE, REAL_SEED, REAL_TOP = (5, 33, 5, 4), 77, -37.5      # the realistic shape: every valid eta <= REAL_TOP, every label C - 1
# The worst ratio of the float64 restatements (softmax_batched_ref, softmax_laplace_ref, psis_loo_softmax_ref,
# softmax_predict_ref: the kernels' forms with numpy's exp, log and division, fed the layouts below) over every table point of every shape, rounded up:
# asserted in tests/test_softmax_link_truth_cpu.py, printed there, DESIGN.md section 9.  (probe, quantity); "rq": the Laplace
# residual at the label's class against q_y with a_r = 0
# (p and the score's r = [y = c] - e / s at C = 65: s is a sum of 65 terms in class order, 7 eps at the worst point)
C_CPU = {("score", "t"): 1.0, ("score", "r"): 3.5, ("hessian", "w"): 2.4, ("laplace", "t"): 0.6, ("laplace", "r"): 0.6,
         ("laplace", "rq"): 0.8, ("loo", "t"): 1.0, ("predict", "p"): 7.0, ("predict", "t"): 1.0}
C_FLOOR, C_DEVICE = 16.0, 4.0                   # the GPU bound: max(16, 4 C_CPU); never from the device's own figures


def c_gpu(probe, quantity):
    return max(C_FLOOR, C_DEVICE * C_CPU[probe, quantity])


# ---- the points ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vectors(C):
    """the free entries (V, C - 1) of the table's vectors at C classes, duplicates (bit for bit) dropped: per magnitude h one
    class at +-h and the rest 0 (the first and the last free class), all at -h (the reference class wins), all at +h (every free
    class ties for the maximum), one at h and the rest at h - delta; then SEEDED vectors with entries +-10^U(-3, 3).  At C = 65
    only the structured families, at a dozen magnitudes"""
    Cm = C - 1
    out = []
    for h in (DOZEN if C == 65 else MAGNITUDES):
        for sign in (1.0, -1.0):
            for c in (0, Cm - 1):
                v = np.zeros(Cm)
                v[c] = sign * h
                out.append(v)
        out.append(np.full(Cm, -h))
        out.append(np.full(Cm, h))
        for d in DELTAS:
            v = np.full(Cm, h - d)
            v[Cm // 2] = h
            out.append(v)
    if C != 65:
        rs = np.random.RandomState(SEED + C)
        for _ in range(SEEDED):
            out.append(np.where(rs.random_sample(Cm) < 0.5, -1.0, 1.0) * 10.0 ** rs.uniform(-3.0, 3.0, Cm))
    seen, keep = set(), []
    for v in out:
        if v.tobytes() not in seen:
            seen.add(v.tobytes())
            keep.append(v)
    return np.array(keep, dtype=np.float64).reshape(len(keep), Cm)


def real_problem():
    """the realistic shape: softmax_batched_ref.make_inputs at REAL_SHAPE with |A|, X = -|X| scaled so that the largest valid eta
    is REAL_TOP, and every label the reference class.  Returns A, y, counts, X (K, 1, D) and eta (K N, C - 1), the dots rounded
    from np.longdouble (the rows past a problem's count keep their eta: they are left out of the sums by ``counts``)"""
    import softmax_batched_ref as sref
    K, N, C, P = REAL_SHAPE
    A, y, counts, _, X = sref.make_inputs(K, N, C, P, 1, seed=REAL_SEED)
    A, X = np.abs(A), -np.abs(X)
    L = np.longdouble

    def dots(X):
        return np.einsum("knp,kcp->knc", A.astype(L), X[:, 0].reshape(K, C - 1, P).astype(L)).astype(np.float64)

    valid = np.arange(N)[None, :] < counts[:, None]
    X = X * (REAL_TOP * 1.0001 / dots(X)[valid].max())
    eta = dots(X)
    assert eta[valid].max() <= REAL_TOP and eta[valid].max() > 1.01 * REAL_TOP
    return A, np.full_like(y, C - 1), counts, X, eta.reshape(K * N, C - 1)


def sets():
    """name -> the free entries (V, C - 1) of every set of the table: one per C of SHAPES, "b2" and "b3" beyond the grid, "real" """
    out = {str(C): vectors(C) for C in sorted({c for c, _ in SHAPES})}
    out.update({f"b{C}": np.array(v, dtype=np.float64) for C, v in BEYOND.items()})
    out["real"] = real_problem()[4]
    return out


# ---- mpmath -----------------------------------------------------------------------------------------------------------------
def _at(free, dps):
    """(lse, [p_c], [q_c]) at working precision dps + guard: eta_c - m is formed from two float64, and e^x has the relative error
    |x| times that of x, so log10 of the largest |eta| is added to the digits"""
    import mpmath as mp
    big = max([abs(float(v)) for v in free] + [1.0])
    with mp.workdps(dps + 15 + int(np.log10(big)) + 1):
        one = mp.mpf(1)
        h = [mp.mpf(float(v)) for v in free] + [mp.mpf(0)]
        m = max(h)
        cs = h.index(m)                                                 # the first class that attains the maximum: its term is 1
        e = [one if c == cs else mp.exp(v - m) for c, v in enumerate(h)]
        o = [v for c, v in enumerate(e) if c != cs]                     # the other terms, in class order
        pre, suf = [mp.mpf(0)], [mp.mpf(0)]
        for v in o:
            pre.append(pre[-1] + v)
        for v in reversed(o):
            suf.append(suf[-1] + v)
        rest = pre[-1]
        s = one + rest
        q, i = [], 0
        for c in range(len(h)):
            if c == cs:
                q.append(rest / s)
            else:
                q.append((one + (pre[i] + suf[len(o) - 1 - i])) / s)    # 1 (the maximal term) + the others but e_c: a sum
                i += 1
        return m + mp.log1p(rest), [v / s for v in e], q


def values(free):
    """{"lse": mpf, "p": [mpf] * C, "q": [mpf] * C} of the vector whose free entries are ``free``: computed to 60 and to 120
    digits, which must agree to 1e-40 relative (raises ArithmeticError otherwise); the 120-digit values are returned"""
    import mpmath as mp
    lo, hi = _at(free, 60), _at(free, 120)
    with mp.workdps(150):
        flat = lambda v: [v[0]] + list(v[1]) + list(v[2])              # noqa: E731
        for a, b in zip(flat(lo), flat(hi)):
            if abs(a - b) > mp.mpf(10) ** -40 * abs(b):
                raise ArithmeticError(f"softmax truth at eta = {list(free)!r}: 60 and 120 digits disagree: {a} {b}")
    return {"lse": hi[0], "p": hi[1], "q": hi[2]}


def written(h, y):
    """t of the density as written, literally, as a function of the list h of C - 1 mpf (for mp.diff)"""
    import mpmath as mp
    full = list(h) + [mp.mpf(0)]
    return full[y] - mp.log(mp.fsum(mp.exp(v) for v in full))


def split(v):
    """an mpf or a Fraction as (float64 nearest, float64 remainder)"""
    if isinstance(v, Fraction):
        hi = float(v)
        return hi, float(v - Fraction(hi))
    import mpmath as mp
    with mp.workdps(400):
        hi = float(v)
        return hi, float(v - mp.mpf(hi))


def build_table():
    """the arrays of tests/golden/softmax_link_truth.npz, from mpmath: per set ``name`` eta_name (V, C - 1), lse_name (V, 2),
    p_name and q_name (V, C, 2); [..., 0] the float64 value, [..., 1] its remainder"""
    tab = {}
    for name, free in sets().items():
        V, C = free.shape[0], free.shape[1] + 1
        lse, p, q = np.zeros((V, 2)), np.zeros((V, C, 2)), np.zeros((V, C, 2))
        for i, f in enumerate(free):
            v = values(f)
            lse[i] = split(v["lse"])
            p[i] = [split(x) for x in v["p"]]
            q[i] = [split(x) for x in v["q"]]
        tab["eta_" + name], tab["lse_" + name], tab["p_" + name], tab["q_" + name] = free, lse, p, q
    return tab


def write_table(path=GOLDEN):
    np.savez_compressed(path, **build_table())


def load_table(path=GOLDEN):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


# ---- without mpmath: t, r, w and the scales from the table ------------------------------------------------------------------------
_E = 1074                                       # a float64 is an integer over 2^1074


def _int(x):
    a, b = float(x).as_integer_ratio()
    return a * ((1 << _E) // b)


def _split_int(n, e):
    """the integer n over 2^e as (float64 nearest, float64 remainder)"""
    d = 1 << e
    hi = n / d
    a, b = hi.as_integer_ratio()
    return hi, (n - a * (d // b)) / d


def rows(tab, name, w=False):
    """the set ``name`` of the table as a dict of float64 arrays, V vectors of C classes:
      eta (V, C) with the reference class's 0;   lse, p, q and their remainders lse_lo, p_lo, q_lo;   scale_p (V, C)
      t, t_lo, scale_t (V, C): indexed [vector, label]
      r, r_lo, scale_r, scale_rq (V, C, C - 1): indexed [vector, label, class]; scale_rq is scale_r without a_r = [y = c] + p_c:
        what a residual formed as q_y (a sum over the other classes) at the label's class is held to
      with ``w``: w, w_lo, scale_w (V, C - 1, C - 1)"""
    free, lse, p, q = (tab[k + "_" + name] for k in ("eta", "lse", "p", "q"))
    V, C = free.shape[0], free.shape[1] + 1
    Cm = C - 1
    eta = np.concatenate([free, np.zeros((V, 1))], axis=1)
    out = {"eta": eta, "lse": lse[:, 0], "lse_lo": lse[:, 1], "p": p[..., 0], "p_lo": p[..., 1], "q": q[..., 0], "q_lo": q[..., 1]}
    ph, qh, ae = p[..., 0], q[..., 0], np.abs(eta)
    # D_c = sum_j |eta_j| |delta_cj - p_j| = sum_{j != c} |eta_j| p_j + |eta_c| q_c, the first sum from prefix and suffix sums
    a = ae * ph
    pre = np.concatenate([np.zeros((V, 1)), np.cumsum(a, axis=1)[:, :-1]], axis=1)
    suf = np.concatenate([np.cumsum(a[:, ::-1], axis=1)[:, ::-1][:, 1:], np.zeros((V, 1))], axis=1)
    Dc = pre + suf + ae * qh
    out["scale_p"] = ph + ph * Dc                                      # dp_c / deta_j = p_c (delta_cj - p_j)
    t, tlo = np.zeros((V, C)), np.zeros((V, C))
    for i in range(V):
        ls = Fraction(float(lse[i, 0])) + Fraction(float(lse[i, 1]))
        for y in range(C):
            t[i, y], tlo[i, y] = split(Fraction(float(eta[i, y])) - ls)
    out["t"], out["t_lo"] = t, tlo
    out["scale_t"] = np.abs(t) + Dc + ae + np.abs(lse[:, :1])           # dt / deta_j = r_j = delta_yj - p_j
    hot = np.eye(C, dtype=bool)[None, :, :Cm]                           # [label, class]
    out["r"] = np.where(hot, qh[:, None, :Cm], -ph[:, None, :Cm])
    out["r_lo"] = np.where(hot, q[:, None, :Cm, 1], -p[:, None, :Cm, 1])
    out["a_r"] = hot + ph[:, None, :Cm]
    out["scale_rq"] = np.abs(out["r"]) + (ph * Dc)[:, None, :Cm]                    # dr_c / deta_j = -w_cj
    out["scale_r"] = out["scale_rq"] + out["a_r"]
    if not w:
        return out
    wh, wlo = np.zeros((V, Cm, Cm)), np.zeros((V, Cm, Cm))
    for i in range(V):
        pi = [_int(p[i, c, 0]) + _int(p[i, c, 1]) for c in range(Cm)]
        qi = [_int(q[i, c, 0]) + _int(q[i, c, 1]) for c in range(Cm)]
        for c in range(Cm):
            wh[i, c, c], wlo[i, c, c] = _split_int(pi[c] * qi[c], 2 * _E)
            for c2 in range(c + 1, Cm):
                hi, lo = _split_int(pi[c] * pi[c2], 2 * _E)
                wh[i, c, c2] = wh[i, c2, c] = -hi
                wlo[i, c, c2] = wlo[i, c2, c] = -lo
    out["w"], out["w_lo"] = wh, wlo
    # w_cc = p_c q_c: d / deta_j = (q_c - p_c) p_c (delta_cj - p_j).  w_cc' = -p_c p_c': d / deta_j = -p_c p_c' (delta_cj + delta_c'j
    # - 2 p_j): sum_j |eta_j| |..| = 2 sum_{j != c, c'} |eta_j| p_j + |eta_c| |q_c - p_c| + |eta_c'| |q_c' - p_c'|, the sum without
    # two classes from the prefix, the run between them and the suffix
    gap = np.abs(qh - ph)
    mid = np.cumsum(a[:, None, :] * (np.arange(C)[None, None, :] > np.arange(C)[None, :, None]), axis=2)     # [v, c, k]: sum_{c < j <= k}
    mid = np.concatenate([np.zeros((V, C, 1)), mid[:, :, :-1]], axis=2)                                       # [v, c, c']: sum_{c < j < c'}
    ex2 = pre[:, :, None] + mid + suf[:, None, :]
    ex2 = np.triu(ex2, 1) + np.swapaxes(np.triu(ex2, 1), 1, 2)
    off = np.abs(wh) * (1.0 + 2.0 * ex2[:, :Cm, :Cm] + (ae * gap)[:, :Cm, None] + (ae * gap)[:, None, :Cm])
    diag = (ph * qh + ph * gap * Dc)[:, :Cm]
    eye = np.eye(Cm, dtype=bool)[None]
    out["scale_w"] = np.where(eye, diag[:, :, None], off)
    return out


def ratio(got, row, quantity, scale=None):
    """|got - truth| / (eps scale) element-wise, the subnormal floor 2^-1070 taken off the error first; a NaN gives inf"""
    hi, lo = row[quantity], row[quantity + "_lo"]
    sc = row["scale_" + quantity] if scale is None else scale
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        err = np.abs((got - hi) - lo)
        out = np.where(err <= FLOOR, 0.0, (err - FLOOR) / (EPS * sc))
    return np.where(np.isnan(got) | np.isnan(out), np.inf, out)


# ---- the layouts: with these inputs and prior_prec = 0 the outputs of the public entry points ARE the link values -------------------
def points(free, P, alpha):
    """the rows of X (V, D) at which the row a = (alpha, 0, ..) has eta = free: x[c P] = free_c / alpha (exact for alpha a power of two),
    the entries that meet a zero feature FILLER"""
    V, Cm = free.shape
    X = np.empty((V, Cm, P))
    X[:, :, 0] = free / alpha
    for j in range(1, P):
        X[:, :, j] = FILLER[(j - 1) % len(FILLER)]
    return X.reshape(V, Cm * P)


def feature_row(P, alpha):
    a = np.zeros(P)
    a[0] = alpha
    return a


def layout_score(free, P, alpha):
    """softmax_batched: one problem per label, N = 1, the vectors as the rows of X: A (C, 1, P), labels (C, 1), X (C, V, D);
    lp[y, v] = t, G[y, v, c P] = alpha r_c"""
    C = free.shape[1] + 1
    X = points(free, P, alpha)
    return (np.tile(feature_row(P, alpha), (C, 1, 1)), np.arange(C, dtype=np.int32)[:, None], np.tile(X[None], (C, 1, 1)))


def layout_point(free, P, alpha):
    """softmax_hessian_batched: one problem per vector, N = 1 (the label does not enter H): A (V, 1, P), labels (V, 1), X (V, D);
    H[v, c P, c' P] = alpha^2 w_cc'"""
    V = free.shape[0]
    return np.tile(feature_row(P, alpha), (V, 1, 1)), np.zeros((V, 1), dtype=np.int32), points(free, P, alpha)


def layout_step(free, P, alpha):
    """softmax_laplace_step_batched(start=True): one problem per (vector, label), vector-major, N = 1: A (V C, 1, P), labels
    (V C, 1), x0 (V C, D); f = -t, g[c P] = -alpha r_c"""
    V, C = free.shape[0], free.shape[1] + 1
    return (np.tile(feature_row(P, alpha), (V * C, 1, 1)), np.tile(np.arange(C, dtype=np.int32), V)[:, None],
            np.repeat(points(free, P, alpha), C, axis=0))


def layout_rows(free, P, alpha, per_problem):
    """the leave-one-out and the predictive: N = C rows a = (alpha, 0, ..), label n on row n.  ``per_problem`` false: one problem,
    the vectors as its draws (repeated to at least 5): A (1, C, P), labels (1, C), X (1, S, D); true: one problem per vector with
    one draw: A (V, C, P), labels (V, C), X (V, 1, D)"""
    V, C = free.shape[0], free.shape[1] + 1
    X = points(free, P, alpha)
    K = V if per_problem else 1
    A = np.tile(feature_row(P, alpha), (K, C, 1))
    y = np.tile(np.arange(C, dtype=np.int32), (K, 1))
    if per_problem:
        return A, y, X[:, None, :].copy()
    reps = -(-5 // V)
    return A, y, np.tile(X, (reps, 1))[None].copy()


if __name__ == "__main__":
    write_table()
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
