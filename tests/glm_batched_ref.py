"""Numpy restatement of the batched GLM targets (gsmvi_glm_batched_f64, csrc/gsmvi_logistic_batched.hip), the generator of
their test inputs and a stand-in engine for the host logic of BatchedGLMTarget.  Test-only.  For problem k with design matrix
A_k (N, D), responses y_k, offsets o_k, n_k valid rows, prior precision lam_k and (gaussian) noise precision tau_k:

    eta = A_k[:n_k] x + o_k[:n_k],   lp_k(x) = sum_n t(eta_n, y_n) - lam_k |x|^2 / 2,   grad lp_k(x) = sum_n r(eta_n, y_n) a_n - lam_k x

with the link (r, t) of ``link`` below in the kernel's forms, and the kernel's two NaN rules: a row of X with a non-finite entry,
and (poisson) a row for which some valid exp(eta) is not finite, get NaN outputs.  It is pinned to torch autograd of the written
densities in tests/test_glm_batched_cpu.py."""
import numpy as np
import torch
from scipy.special import erfcx

import logistic_batched_ref as lref

FAMILIES = ("logistic", "poisson", "probit", "gaussian")


def link(family, eta, y, tau=1.0):
    """r = dt / d eta, t, and the mask of the entries that flag their row (poisson: exp(eta) not finite; r = t = 0 there)"""
    none = np.zeros(eta.shape, dtype=bool)
    if family == "logistic":
        sig, sp = lref.sigmoid_softplus(eta)
        return y - sig, y * eta - sp, none
    if family == "poisson":
        m = np.exp(eta)
        bad = ~(m < np.inf)                                         # (a NaN too)
        return np.where(bad, 0.0, y - m), np.where(bad, 0.0, y * eta - m), bad
    if family == "probit":
        # s = |eta|, u = erfcx(s / sqrt 2), e = exp(-s^2 / 2), q = u e / 2 = Phi(-s); tail side: log Phi(-s) = log(u / 2) - s^2 / 2,
        # phi / Phi(-s) = sqrt(2 / pi) / u; central side: log Phi(s) = log1p(-q), phi / Phi(s) = e / sqrt(2 pi) / (1 - q)
        s = np.abs(eta)
        u, hs = erfcx(s * 0.70710678118654752440), 0.5 * (s * s)
        e = np.exp(-hs)
        q = 0.5 * (u * e)
        rt, rc = 0.79788456080286535588 / u, e * 0.39894228040143267794 / (1.0 - q)
        # (lt held at the largest finite number: from |eta| = 1.34e154 on s^2 overflows, and 0 * inf would be a NaN)
        lt, lc = np.fmax(np.log(0.5 * u) - hs, -1.7976931348623157e308), np.log1p(-q)
        pos = eta >= 0.0
        r = np.where(pos, y * rc - (1.0 - y) * rt, y * rt - (1.0 - y) * rc)
        t = np.where(pos, y * lc + (1.0 - y) * lt, y * lt + (1.0 - y) * lc)
        return r, t, none
    if family == "gaussian":
        d = y - eta
        return tau * d, -0.5 * (tau * (d * d)), none
    raise ValueError(family)


def score_and_lp(family, A, y, offset, counts, lam, tau, X):
    """A (K, N, D), y (K, N), offset (K, N) or None, counts (K,) or None, lam and tau a number or (K,), X (K, rows, D) ->
    G (K, rows, D), lp (K, rows); a per-problem loop with both NaN rules of the kernel."""
    A, y, X = np.asarray(A, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(X, dtype=np.float64)
    K, N, D = A.shape
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (K,))
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (K,))
    G, lp = np.empty_like(X), np.empty(X.shape[:2])
    for k in range(K):
        n = N if counts is None else int(min(max(int(counts[k]), 0), N))
        Ak, yk = A[k, :n], y[k, :n]
        with np.errstate(all="ignore"):
            eta = X[k] @ Ak.T                                           # (rows, n)
            if offset is not None:
                eta = eta + np.asarray(offset, dtype=np.float64)[k, None, :n]
            r, t, flag = link(family, eta, yk[None, :], tau[k])
            G[k] = r @ Ak - lam[k] * X[k]
            lp[k] = t.sum(1) - 0.5 * lam[k] * (X[k] * X[k]).sum(1)
        bad = ~np.isfinite(X[k]).all(1) | flag.any(1)
        G[k, bad] = np.nan
        lp[k, bad] = np.nan
    return G, lp


def make_inputs(family, K, N, D, rows, scale=1.0, seed=None):
    """The inputs of the tests: RandomState(N + D) (or ``seed``); A = scale N(0, 1) / sqrt(D), offsets 0.3 N(0, 1), theta* ~
    N(0, 1) and y drawn from the family at eta* = A theta* + offset (poisson: the rate capped at e^20; gaussian: noise of
    precision tau), counts = N for problem 0 and max(1, N - 1 - 3 k) after it, lam = 0 for problem 0 and 0.1 + U(0, 1) after it,
    tau = 0.5 + U(0, 1) for the gaussian family and 1.0 otherwise, X = scale N(0, 1) (poisson: scale capped at 2, so that
    exp(eta) stays finite).  Returns A, y, offset, counts (int32), lam, tau, X."""
    rs = np.random.RandomState(N + D if seed is None else seed)
    A = scale * rs.standard_normal((K, N, D)) / np.sqrt(D)
    offset = 0.3 * rs.standard_normal((K, N))
    theta = rs.standard_normal((K, D))
    eta = np.einsum("knd,kd->kn", A, theta) + offset
    u = rs.random_sample((K, N))
    tau = 0.5 + rs.random_sample(K) if family == "gaussian" else 1.0
    if family == "logistic":
        y = (u < lref.sigmoid_softplus(eta)[0]).astype(np.float64)
    elif family == "probit":
        y = (u < torch.special.ndtr(torch.tensor(eta)).numpy()).astype(np.float64)
    elif family == "poisson":
        y = rs.poisson(np.exp(np.minimum(eta, 20.0))).astype(np.float64)
    else:
        y = eta + rs.standard_normal((K, N)) / np.sqrt(tau)[:, None]
    counts = np.array([N if k == 0 else max(1, N - 1 - 3 * k) for k in range(K)], dtype=np.int32)
    lam = 0.1 + rs.random_sample(K)
    lam[0] = 0.0
    X = (min(scale, 2.0) if family == "poisson" else scale) * rs.standard_normal((K, rows, D))
    return A, y, offset, counts, lam, tau, X


class RestatementEngine:
    """the engine calls BatchedGLMTarget makes, on numpy and the restatement; ``calls`` records every one"""
    name = "restatement-glm(test-only)"

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

    def glm_batched(self, X, A, y, family, offset=None, counts=None, prior_prec=1.0, noise_prec=1.0, out=None, lp_out=None,
                    want="g"):
        self.calls.append(("glm", family, want, out is not None))
        assert A.dtype == np.float64 and y.dtype == np.float64 and (counts is None or counts.dtype == np.int32)
        assert offset is None or offset.dtype == np.float64
        G, lp = score_and_lp(family, A, y, offset, counts, prior_prec, noise_prec, X)
        if out is not None:
            out[...] = G
            G = out
        return G if want == "g" else lp if want == "lp" else (G, lp)
