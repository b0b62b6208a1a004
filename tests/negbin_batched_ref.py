"""Numpy restatements of the batched negative binomial target (gsmvi_negbin_batched_f64, csrc/gsmvi_negbin_batched.hip and
csrc/gsmvi_negbin_link.h), the generator of its test inputs and a stand-in engine for the host logic of
BatchedNegBinomialTarget.  Test-only.  For problem k with design matrix A_k (N, P), responses y_k >= 0, offsets o_k, n_k valid
rows, at x = (beta, theta), r = exp(theta), d = eta - theta:

    t = dlg(y, r) - r softplus(d) - y softplus(-d),   r_eta = y sigma(-d) - r sigma(d),   r_theta = r (dps(y, r) - softplus(d)) - r_eta
    lp_k(x) = sum_n t_n - lam_k |beta|^2 / 2 - kap_k (theta - m_k)^2 / 2
    grad lp_k(x) = (sum_n r_eta,n a_n - lam_k beta,  sum_n r_theta,n - kap_k (theta - m_k))

``link`` is the float64 restatement: the kernel's forms operation by operation (the shifted Stirling differences of dlg = lgamma(y +
r) - lgamma(r) and dps = psi(y + r) - psi(r)); ``score_and_lp`` sums the observations in ascending order as the kernel does.
``link_ld`` / ``score_and_lp_ld`` are the same model in np.longdouble with the differences shifted to z >= 40, where the seven-term
tails leave less than 1e-20: the reference of the GPU test."""
import numpy as np
import torch

SHIFT_BELOW, SHIFT = 10.0, 10                    # NB_SHIFT_BELOW, NB_SHIFT of csrc/gsmvi_negbin_link.h
R_MIN = 2.2250738585072014e-308                  # the smallest positive normal number
LG = (1.0 / 156.0, -691.0 / 360360.0, 1.0 / 1188.0, -1.0 / 1680.0, 1.0 / 1260.0, -1.0 / 360.0, 1.0 / 12.0)
PS = (-1.0 / 12.0, 691.0 / 32760.0, -1.0 / 132.0, 1.0 / 240.0, -1.0 / 252.0, 1.0 / 120.0, -1.0 / 12.0)


def _tails(z, L=np.float64):
    """S(z), P(z): the seven-term Stirling tails of lgamma and psi, Horner in 1 / z^2 as the kernel"""
    x = L(1.0) / z
    w = x * x
    if L is np.float64:
        cs, cp = LG, PS
    else:
        cs = [L(1) / 156, L(-691) / 360360, L(1) / 1188, L(-1) / 1680, L(1) / 1260, L(-1) / 360, L(1) / 12]
        cp = [L(-1) / 12, L(691) / 32760, L(-1) / 132, L(1) / 240, L(-1) / 252, L(1) / 120, L(-1) / 12]
    s, p = cs[0], cp[0]
    for a, b in zip(cs[1:], cp[1:]):
        s, p = s * w + a, p * w + b
    return s * x, p * w


def link(eta, theta, y, r=None):
    """(r_eta, r_theta, t) in float64, the kernel's forms; eta, theta, y broadcast; r = exp(theta) unless given"""
    with np.errstate(all="ignore"):
        eta, theta, y = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (eta, theta, y)))
        r = np.exp(theta) if r is None else np.broadcast_to(np.asarray(r, dtype=np.float64), eta.shape)
        d = eta - theta
        e = np.exp(-np.abs(d))
        q, l1 = 1.0 + e, np.log1p(e)
        spd, spn = np.where(d > 0.0, d, 0.0) + l1, np.where(d < 0.0, -d, 0.0) + l1
        small = r < SHIFT_BELOW
        u = y / r
        sl = np.where(u < 1e300, np.log1p(u), np.log(y) - theta)
        sp = (y / (r + y)) / r
        for j in range(1, SHIFT):
            a = r + float(j)
            sl = sl + np.log1p(y / a)
            sp = sp + y / (a * (a + y))
        sl, sp = np.where(small, sl, 0.0), np.where(small, sp, 0.0)
        z = np.where(small, r + float(SHIFT), r)
        zy, lu = z + y, np.log1p(y / z)
        (s1, p1), (s0, p0) = _tails(zy), _tails(z)
        dlg = ((z - 0.5) * lu + y * (np.log(zy) - 1.0)) + (s1 - s0) - sl
        t = dlg - r * spd - y * spn
        sg, sn = np.where(d >= 0.0, 1.0 / q, e / q), np.where(d >= 0.0, e / q, 1.0 / q)
        dps = lu + y / (2.0 * z * zy) + (p1 - p0) + sp
        re = y * sn - r * sg
        rt = r * (dps - spd) - re
    return re, rt, t


def link_ld(eta, theta, y, zmin=40.0):
    """(r_eta, r_theta, t) in np.longdouble: the same model, the differences shifted until z >= zmin (tails below 1e-20)"""
    L = np.longdouble
    with np.errstate(all="ignore"):
        eta, theta, y = np.broadcast_arrays(*(np.asarray(v, dtype=L) for v in (eta, theta, y)))
        r = np.exp(theta)
        d = eta - theta
        e = np.exp(-np.abs(d))
        q, l1 = 1 + e, np.log1p(e)
        spd, spn = np.where(d > 0, d, L(0)) + l1, np.where(d < 0, -d, L(0)) + l1
        sl, sp = np.zeros(r.shape, dtype=L), np.zeros(r.shape, dtype=L)
        for j in range(int(zmin)):
            a = r + j
            on = r < zmin
            sl = sl + np.where(on, np.log1p(y / a), L(0))
            sp = sp + np.where(on, (y / (a + y)) / a, L(0))
        z = np.where(r < zmin, r + int(zmin), r)
        zy, lu = z + y, np.log1p(y / z)
        (s1, p1), (s0, p0) = _tails(zy, L), _tails(z, L)
        dlg = ((z - L(0.5)) * lu + y * (np.log(zy) - 1)) + (s1 - s0) - sl
        t = dlg - r * spd - y * spn
        sg, sn = np.where(d >= 0, 1 / q, e / q), np.where(d >= 0, e / q, 1 / q)
        dps = lu + y / (2 * z * zy) + (p1 - p0) + sp
        re = y * sn - r * sg
        rt = r * (dps - spd) - re
    return re, rt, t


def _score_and_lp(A, y, offset, counts, lam, tm, tk, X, L, fn):
    A, y, X = np.asarray(A, dtype=L), np.asarray(y, dtype=L), np.asarray(X, dtype=L)
    K, N, P = A.shape
    lam, tm, tk = (np.broadcast_to(np.asarray(v, dtype=L), (K,)) for v in (lam, tm, tk))
    G, lp = np.empty(X.shape, dtype=L), np.empty(X.shape[:2], dtype=L)
    for k in range(K):
        n = N if counts is None else int(min(max(int(counts[k]), 0), N))
        Ak, yk, beta, theta = A[k, :n], y[k, :n], X[k, :, :P], X[k, :, P]
        with np.errstate(all="ignore"):
            eta = np.zeros((X.shape[1], n), dtype=L)
            for j in range(P):                                          # the kernel's chain over the columns
                eta = eta + beta[:, j, None] * Ak[None, :, j]
            if offset is not None:
                eta = eta + np.asarray(offset, dtype=L)[k, None, :n]
            re, rt, t = fn(eta, theta[:, None], yk[None, :])
            g, gt, s = np.zeros(beta.shape, dtype=L), np.zeros(theta.shape, dtype=L), np.zeros(theta.shape, dtype=L)
            for i in range(n):                                          # ascending n, one chain per output
                g, gt, s = g + re[:, i, None] * Ak[None, i, :], gt + rt[:, i], s + t[:, i]
            dm = theta - tm[k]
            G[k, :, :P] = g - lam[k] * beta
            G[k, :, P] = gt - tk[k] * dm
            bb = np.zeros(theta.shape, dtype=L)
            for j in range(P):
                bb = bb + beta[:, j] * beta[:, j]
            lp[k] = s - L(0.5) * lam[k] * bb - L(0.5) * tk[k] * (dm * dm)
            rr = np.exp(X[k, :, P].astype(np.float64))
        bad = ~np.isfinite(X[k].astype(np.float64)).all(1) | ~((rr >= R_MIN) & (rr < np.inf))
        G[k, bad] = np.nan
        lp[k, bad] = np.nan
    return G, lp


def score_and_lp(A, y, offset, counts, lam, tm, tk, X):
    """A (K, N, P), y (K, N), offset (K, N) or None, counts (K,) or None, lam, tm, tk a number or (K,), X (K, rows, P + 1) ->
    G (K, rows, P + 1), lp (K, rows) in float64: the kernel's forms, sums in its order, and its row flag"""
    return _score_and_lp(A, y, offset, counts, lam, tm, tk, X, np.float64, link)


def score_and_lp_ld(A, y, offset, counts, lam, tm, tk, X):
    """the same in np.longdouble (rounded to float64 by the caller): the GPU test's reference"""
    return _score_and_lp(A, y, offset, counts, lam, tm, tk, X, np.longdouble, link_ld)


def make_inputs(K, N, P, rows, seed=None, theta_lo=-1.0, theta_hi=4.0, poison=True):
    """The inputs of the tests: RandomState(N + P) (or ``seed``); A = N(0, 1) / sqrt(P), offsets 0.3 N(0, 1), beta* ~ N(0, 1),
    log r* ~ U(0, 3) and y negative binomial at mu = exp(A beta* + offset) (capped at e^10) with size r*; counts = N for problem
    0, 0 for problem 1 (when K > 1) and max(1, N - 1 - 3 k) after it; lam = 0 for problem 0 and 0.1 + U(0, 1) after it; the prior of
    theta m ~ N(1, 1), kap = U(0, 2) with kap = 0 for problem 0; X = (N(0, 1), U(theta_lo, theta_hi)): the rows' r = e^theta lie
    on both sides of the shift threshold 10 = e^2.30.  ``poison``: the rows beyond counts hold NaN (A), -1 and NaN (y) and inf
    (offset).  Returns A, y, offset, counts (int32), lam, tm, tk, X."""
    rs = np.random.RandomState(N + P if seed is None else seed)
    A = rs.standard_normal((K, N, P)) / np.sqrt(P)
    offset = 0.3 * rs.standard_normal((K, N))
    beta = rs.standard_normal((K, P))
    size = np.exp(rs.uniform(0.0, 3.0, K))
    mu = np.exp(np.minimum(np.einsum("knp,kp->kn", A, beta) + offset, 10.0))
    y = rs.poisson(rs.gamma(size[:, None], mu / size[:, None])).astype(np.float64)
    counts = np.array([N if k == 0 else 0 if k == 1 else max(1, N - 1 - 3 * k) for k in range(K)], dtype=np.int32)
    lam = 0.1 + rs.random_sample(K)
    lam[0] = 0.0
    tm = 1.0 + rs.standard_normal(K)
    tk = 2.0 * rs.random_sample(K)
    tk[0] = 0.0
    X = np.concatenate([rs.standard_normal((K, rows, P)), rs.uniform(theta_lo, theta_hi, (K, rows, 1))], axis=2)
    if poison:
        for k in range(K):
            A[k, counts[k]:] = np.nan
            y[k, counts[k]:] = [-1.0, np.nan][k % 2]
            offset[k, counts[k]:] = np.inf
    return A, y, offset, counts, lam, tm, tk, X


class RestatementEngine:
    """the engine calls BatchedNegBinomialTarget makes, on numpy and the float64 restatement; ``calls`` records every one"""
    name = "restatement-negbin(test-only)"

    def __init__(self):
        self.calls = []

    def asarray(self, x):
        self.calls.append("asarray")
        return np.array(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)

    def to_numpy(self, a):
        return np.asarray(a)

    def batched_counts(self, values):
        self.calls.append("batched_counts")
        return np.asarray(values, dtype=np.int32).reshape(-1)

    def batched_regs(self, values):
        self.calls.append("batched_regs")
        return np.asarray(values, dtype=np.float64).reshape(-1)

    def negbin_batched(self, X, A, y, offset=None, counts=None, prior_prec=1.0, log_size_mean=0.0, log_size_prec=1.0, out=None,
                       lp_out=None, want="g"):
        self.calls.append(("negbin", want, out is not None))
        self.last = dict(A=A, y=y, offset=offset, counts=counts, prior_prec=prior_prec, log_size_mean=log_size_mean,
                         log_size_prec=log_size_prec)
        assert A.dtype == np.float64 and y.dtype == np.float64 and (counts is None or counts.dtype == np.int32)
        assert offset is None or offset.dtype == np.float64
        G, lp = score_and_lp(A, y, offset, counts, prior_prec, log_size_mean, log_size_prec, X)
        if out is not None:
            out[...] = G
            G = out
        return G if want == "g" else lp if want == "lp" else (G, lp)
