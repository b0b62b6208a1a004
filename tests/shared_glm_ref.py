"""Numpy restatement of the shared-design GLM target (gsmvi_glm_shared_batched_f64, csrc/gsmvi_glm_shared_batched.hip), the
generator of its test inputs and a stand-in engine for the host logic of SharedDesignGLMTarget.  Test-only.  All K problems have
the rows a_n of ONE design matrix A (N, D); problem k has responses y_k, offsets o_k, observation weights w_k >= 0, prior
precision lam_k and (gaussian) noise precision tau_k:

    eta = A x + o_k,   lp_k(x) = sum_n w_kn t(eta_n, y_kn) - lam_k |x|^2 / 2,   grad lp_k(x) = sum_n w_kn r(eta_n, y_kn) a_n - lam_k x

with the link (r, t) of glm_batched_ref.link.  An observation with a weight that is not > 0 is removed by selection (its y, offset
and eta are never looked at), as the kernel removes it; the sums over the selected observations are formed as
glm_batched_ref.score_and_lp forms them over its valid rows, so that weights = None is that function on the K-fold replicated
design bit for bit.  The kernel's two NaN rules: a row of X with a non-finite entry, and (poisson) a row for which exp(eta) is not
finite at a selected observation, get NaN outputs."""
import numpy as np
import torch

import glm_batched_ref as gref
import logistic_batched_ref as lref

FAMILIES = gref.FAMILIES


def score_and_lp(family, A, y, offset, weights, lam, tau, X):
    """A (N, D), y (K, N), offset and weights (K, N) or None, lam and tau a number or (K,), X (K, rows, D) -> G (K, rows, D),
    lp (K, rows); float64, a per-problem loop"""
    A, y, X = np.asarray(A, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(X, dtype=np.float64)
    (N, D), K = A.shape, y.shape[0]
    assert y.shape == (K, N) and X.shape[0] == K and X.shape[2] == D
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (K,))
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (K,))
    G, lp = np.empty_like(X), np.empty(X.shape[:2])
    for k in range(K):
        if weights is None:
            Ak, yk, ok, wk = A, y[k], None if offset is None else np.asarray(offset, dtype=np.float64)[k], None
        else:
            w = np.asarray(weights, dtype=np.float64)[k]
            with np.errstate(invalid="ignore"):
                sel = np.flatnonzero(w > 0.0)
            Ak, yk, wk = A[sel], y[k, sel], w[sel]
            ok = None if offset is None else np.asarray(offset, dtype=np.float64)[k, sel]
        with np.errstate(all="ignore"):
            eta = X[k] @ Ak.T                                           # (rows, selected)
            if ok is not None:
                eta = eta + ok[None, :]
            r, t, flag = gref.link(family, eta, yk[None, :], tau[k])
            if wk is not None:
                r, t = wk[None, :] * r, wk[None, :] * t
            G[k] = r @ Ak - lam[k] * X[k]
            lp[k] = t.sum(1) - 0.5 * lam[k] * (X[k] * X[k]).sum(1)
        bad = ~np.isfinite(X[k]).all(1) | flag.any(1)
        G[k, bad] = np.nan
        lp[k, bad] = np.nan
    return G, lp


def make_inputs(family, K, N, D, rows, scale=1.0, seed=None, zero_frac=0.25, poison=False):
    """The inputs of the tests: RandomState(N + D) (or ``seed``); A (N, D) = scale N(0, 1) / sqrt(D), offsets 0.3 N(0, 1),
    theta*_k ~ N(0, 1) and y_k drawn from the family at eta* = A theta*_k + offset_k (poisson: the rate capped at e^20;
    gaussian: noise of precision tau_k), weights U(0, 2) with a fraction ``zero_frac`` of exact zeros (``poison``: y = NaN and
    offset = inf there), lam = 0 for problem 0 and 0.1 + U(0, 1) after it, tau = 0.5 + U(0, 1) for the gaussian family and 1.0
    otherwise, X = scale N(0, 1) (poisson: scale capped at 2, so that exp(eta) stays finite).  Returns A, y, offset, weights,
    lam, tau, X."""
    rs = np.random.RandomState(N + D if seed is None else seed)
    A = scale * rs.standard_normal((N, D)) / np.sqrt(D)
    offset = 0.3 * rs.standard_normal((K, N))
    theta = rs.standard_normal((K, D))
    eta = theta @ A.T + offset
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
    weights = 2.0 * rs.random_sample((K, N))
    weights[rs.random_sample((K, N)) < zero_frac] = 0.0
    if poison:
        y[weights == 0.0] = np.nan
        offset[weights == 0.0] = np.inf
    lam = 0.1 + rs.random_sample(K)
    lam[0] = 0.0
    X = (min(scale, 2.0) if family == "poisson" else scale) * rs.standard_normal((K, rows, D))
    return A, y, offset, weights, lam, tau, X


def replicate(A, K):
    """the K-fold copy (K, N, D) of the design that the per-problem entry point needs"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(A)[None], (K,) + np.asarray(A).shape))


class RestatementEngine(gref.RestatementEngine):
    """the engine calls SharedDesignGLMTarget makes, on numpy and the restatement; ``calls`` records every one and ``last`` holds
    the arrays of the last launch as they were passed"""
    name = "restatement-shared-glm(test-only)"

    def glm_shared_batched(self, X, A, y, family, offset=None, weights=None, prior_prec=1.0, noise_prec=1.0, out=None,
                           lp_out=None, want="g"):
        self.calls.append(("glm_shared", family, want, out is not None))
        self.last = dict(A=A, y=y, offset=offset, weights=weights, prior_prec=prior_prec, noise_prec=noise_prec)
        assert A.dtype == np.float64 and y.dtype == np.float64
        assert (offset is None or offset.dtype == np.float64) and (weights is None or weights.dtype == np.float64)
        G, lp = score_and_lp(family, A, y, offset, weights, prior_prec, noise_prec, X)
        if out is not None:
            out[...] = G
            G = out
        return G if want == "g" else lp if want == "lp" else (G, lp)
