"""Numpy restatement of the batched GLM posterior predictive (gsmvi_glm_predict_batched_f64, csrc/gsmvi_glm_predict_batched.hip),
the generator of its test problems and a stand-in engine for the host logic of ``predict``.  Test-only.  For row n < n_k of
problem k under q_k = N(mu_k, Sigma_k), in numpy ``longdouble`` with the Gauss-Hermite table rounded to double:

    m = a_n . mu_k + o_kn,   v = a_n^T Sigma_k a_n,   v+ = max(v, 0),   s = sqrt(2 v+),   eta_q = m + s t_q
    eta_mean = m,  eta_var = v
    gaussian   pmean = m                                     lpd = -log(2 pi (v+ + 1 / tau)) / 2 - (y - m)^2 / (2 (v+ + 1 / tau))
    probit     pmean = Phi(m / sqrt(1 + v+))                 lpd = LSE_q(logw_q + t(eta_q, y)) - log(pi) / 2
    poisson    pmean = exp(m + v+ / 2)                       lpd = LSE_q(logw_q + y eta_q - e^eta_q) - log(pi) / 2 - lgamma(y + 1)
    logistic   pmean = sum_q exp(logw_q) sigma(eta_q) / sqrt(pi)   lpd = LSE_q(logw_q + t(eta_q, y)) - log(pi) / 2

LSE takes the maximum first and sums exp(. - max) in ascending q; elpd[k] sums lpd[k, :n_k] in row order.  Phi, erfcx and lgamma
come from scipy.special (in double: scipy has no wider forms); everything else is carried in longdouble.  Rows n >= n_k are NaN,
as is a row whose m or v is not finite.  It is pinned to closed forms and to brute-force quadrature in tests/test_glm_predict_cpu.py."""
import functools

import numpy as np
from scipy import special

import glm_batched_ref as gref

FAMILIES = gref.FAMILIES
LD = np.longdouble
# (D, M, K) of the GPU parity test: every D at which the padding, the packing or the MFMA block count changes, every M around the
# 32-row tile and the prefetch tail, K not a multiple of the four slots
SHAPES = ((1, 31, 3), (2, 1, 1), (15, 33, 7), (16, 65, 3), (17, 32, 7), (31, 1, 3), (32, 33, 1), (33, 65, 7), (48, 31, 3),
          (63, 32, 1), (64, 65, 7), (10, 32, 7), (16, 31, 1), (64, 33, 3), (5, 65, 7), (17, 31, 3))


def gh_table(Q):
    """the nodes and the logarithms of the weights of the Q-point rule, rounded to double: what the kernel is handed"""
    t, w = np.polynomial.hermite.hermgauss(int(Q))
    return np.asarray(t, dtype=np.float64), np.log(np.asarray(w, dtype=np.float64))


def _t(family, eta, y):
    """t(eta, y) of the family in longdouble (probit: the erfcx forms of glm_batched_ref.link, in double)"""
    if family == "logistic":
        return y * eta - (np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta))))
    if family == "poisson":
        return y * eta - np.exp(eta)
    if family == "probit":
        return gref.link("probit", np.asarray(eta, dtype=np.float64), np.asarray(y, dtype=np.float64))[1].astype(LD)
    raise ValueError(family)


def _sigmoid(eta):
    e = np.exp(-np.abs(eta))
    return np.where(eta >= 0, 1 / (1 + e), e / (1 + e))


def _ordered_sum(x):
    """sum over the last axis in ascending index (np.sum is pairwise)"""
    s = np.zeros(x.shape[:-1], dtype=x.dtype)
    for q in range(x.shape[-1]):
        s = s + x[..., q]
    return s


def rows(family, m, v, y=None, tau=1.0, Q=32):
    """the table for rows given by their (m, v): pmean and (with y) lpd, longdouble in, longdouble out"""
    m, v = np.asarray(m, dtype=LD), np.asarray(v, dtype=LD)
    t, lw = (x.astype(LD) for x in gh_table(Q))
    vp = np.maximum(v, 0)
    eta = m[..., None] + np.sqrt(2 * vp)[..., None] * t
    pi = 4 * np.arctan(LD(1))
    with np.errstate(all="ignore"):
        if family == "gaussian":
            pmean = m.copy()
        elif family == "probit":
            pmean = special.ndtr(np.asarray(m / np.sqrt(1 + vp), dtype=np.float64)).astype(LD)
        elif family == "poisson":
            pmean = np.exp(m + vp / 2)
        else:
            pmean = _ordered_sum(np.exp(lw) * _sigmoid(eta)) / np.sqrt(pi)
        lpd = None
        if y is not None:
            y = np.asarray(y, dtype=LD)
            if family == "gaussian":
                var = vp + 1 / LD(tau)
                lpd = -np.log(2 * pi * var) / 2 - (y - m) ** 2 / (2 * var)
            else:
                f = lw + _t(family, eta, y[..., None])
                mx = f.max(-1)
                lpd = mx + np.log(_ordered_sum(np.exp(f - mx[..., None]))) - np.log(pi) / 2
                if family == "poisson":
                    lpd = lpd - special.gammaln(np.asarray(y, dtype=np.float64) + 1.0).astype(LD)
    return pmean, lpd


def predict(family, A, offset, y, counts, tau, mean, cov, Q=32):
    """A (K, M, D), offset and y (K, M) or None, counts (K,) or None, tau a number or (K,), mean (K, D), cov (K, D, D) -> a dict of
    float64 arrays eta_mean, eta_var, mean, lpd (K, M), elpd (K,) (the last two None without y) and ``scale_var`` (K, M) =
    sum_ij |a_i| |Sigma_ij| |a_j|, what the rounding error of eta_var is proportional to"""
    A, mean, cov = (np.asarray(x, dtype=np.float64) for x in (A, mean, cov))
    K, M, D = A.shape
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (K,))
    out = {k: np.full((K, M), np.nan) for k in ("eta_mean", "eta_var", "mean", "scale_var")}
    out["lpd"] = np.full((K, M), np.nan) if y is not None else None
    out["elpd"] = np.zeros(K) if y is not None else None
    for k in range(K):
        n = M if counts is None else int(min(max(int(counts[k]), 0), M))
        Ak, mu, S = A[k, :n].astype(LD), mean[k].astype(LD), cov[k].astype(LD)
        with np.errstate(all="ignore"):
            m = Ak @ mu
            if offset is not None:
                m = m + np.asarray(offset, dtype=np.float64)[k, :n].astype(LD)
            v = np.einsum("ni,ij,nj->n", Ak, S, Ak)
            pmean, lpd = rows(family, m, v, None if y is None else np.asarray(y, dtype=np.float64)[k, :n], tau[k], Q)
            bad = ~(np.isfinite(m) & np.isfinite(v))
            out["scale_var"][k, :n] = np.einsum("ni,ij,nj->n", np.abs(Ak), np.abs(S), np.abs(Ak))
        for name, val in (("eta_mean", m), ("eta_var", v), ("mean", pmean)) + ((("lpd", lpd),) if y is not None else ()):
            out[name][k, :n] = np.where(bad, np.nan, val).astype(np.float64)
        if y is not None:
            with np.errstate(all="ignore"):
                out["elpd"][k] = np.float64(_ordered_sum(np.where(bad, np.nan, lpd).astype(LD)[None, :])[0]) if n else 0.0
    return out


def make_problem(family, K, M, D, seed=None):
    """The problems of the tests: RandomState(1000 + 7 M + D) (or ``seed``); A = N(0, 1) / sqrt(D), offsets 0.3 N(0, 1), the
    posterior mean 0.5 N(0, 1), its covariance G G^T / (4 D) scaled down, where needed, so that a^T Sigma a <= 0.9 on every row
    (the band in which the quadrature at Q = 32 is accurate), y drawn from the family at a theta* + o with theta* ~ N(mean, I / 4)
    (poisson: the rate capped at e^10; gaussian: noise of precision tau), tau = 0.5 + U(0, 1) per problem for the gaussian
    family and 1.0 otherwise, counts cycling through M, 0, a mid value, M, 1, ... (K = 1: M).  Returns a dict."""
    rs = np.random.RandomState(1000 + 7 * M + D if seed is None else seed)
    A = rs.standard_normal((K, M, D)) / np.sqrt(D)
    offset = 0.3 * rs.standard_normal((K, M))
    mean = 0.5 * rs.standard_normal((K, D))
    G = rs.standard_normal((K, D, D))
    cov = G @ np.swapaxes(G, 1, 2) / (4.0 * D)
    vmax = np.einsum("kni,kij,knj->kn", A, cov, A).max(1)
    cov = cov * np.minimum(1.0, 0.9 / vmax)[:, None, None]
    theta = mean + 0.5 * rs.standard_normal((K, D))
    eta = np.einsum("knd,kd->kn", A, theta) + offset
    u = rs.random_sample((K, M))
    tau = 0.5 + rs.random_sample(K) if family == "gaussian" else 1.0
    if family == "logistic":
        y = (u < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    elif family == "probit":
        y = (u < special.ndtr(eta)).astype(np.float64)
    elif family == "poisson":
        y = rs.poisson(np.exp(np.minimum(eta, 10.0))).astype(np.float64)
    else:
        y = eta + rs.standard_normal((K, M)) / np.sqrt(tau)[:, None]
    cyc = [M, 0, max(1, M // 2), M, 1, max(1, M - 1), max(1, M // 3)]
    counts = np.array([cyc[k % len(cyc)] for k in range(K)], dtype=np.int32)
    return {"family": family, "A": A, "offset": offset, "y": y, "counts": counts, "tau": tau, "mean": mean, "cov": cov}


@functools.lru_cache(maxsize=None)
def reference(family, shape, with_offset, Q=32):
    """(problem, restatement with y) at ``shape`` = (D, M, K): computed once and shared (do not modify)"""
    D, M, K = shape
    p = make_problem(family, K, M, D)
    r = predict(family, p["A"], p["offset"] if with_offset else None, p["y"], p["counts"], p["tau"], p["mean"], p["cov"], Q)
    return p, r


E2E = dict(K=8, N=96, D=5, held=32, seed=5)          # the end-to-end problem of the CPU and the GPU test


def e2e_problem():
    """K = 8 logistic problems at (N, D) = (96, 5), prior precision 1, the last 32 rows held out: ((A, y, lam) to fit, (A, y) held
    out).  make_inputs at scale 2 and a seed at which the property of the end-to-end test holds on the restatement alone
    (tests/test_glm_predict_cpu.py checks that)."""
    A, y, _, _, _, _, _ = gref.make_inputs("logistic", E2E["K"], E2E["N"], E2E["D"], 1, scale=2.0, seed=E2E["seed"])
    n = E2E["N"] - E2E["held"]
    return (A[:, :n], y[:, :n], np.full(E2E["K"], 1.0)), (A[:, n:], y[:, n:])


class StandInEngine(gref.RestatementEngine):
    """the engine calls of ``predict`` on numpy and the restatement"""
    name = "restatement-predict(test-only)"

    def glm_predict_batched(self, mean, cov, A, family, offset=None, y=None, counts=None, noise_prec=1.0, nodes=32):
        self.calls.append(("predict", family, y is not None, offset is not None, counts is not None, nodes))
        assert A.dtype == np.float64 and mean.dtype == np.float64 and cov.dtype == np.float64
        assert counts is None or counts.dtype == np.int32
        r = predict(family, A, offset, y, counts, noise_prec, mean, cov, nodes)
        return r["eta_mean"], r["eta_var"], r["mean"], r["lpd"], r["elpd"]


def check_bad_arguments(lib):
    """the entry point through the C ABI with a NULL context: every bad argument returns GSMVI_ERR_BAD_ARG (1) with its own
    message, so nothing can have been enqueued; valid calls end at the context"""
    import ctypes as C
    buf = (C.c_double * 16384)()
    p = C.cast(buf, C.c_void_p).value
    a = lambda n: p + 8 * 512 * n                                   # noqa: E731  thirty-two disjoint 4 KB arrays
    err = lambda: (lib.gsmvi_last_error() or b"").decode()           # noqa: E731
    name = "gsmvi_glm_predict_batched_f64"

    def call(K=2, D=4, M=5, family=1, A=a(0), offset=a(1), y=a(2), counts=a(3), tau=1.0, tau_dev=None, mean=a(4), cov=a(5), Q=32,
             gh_t=a(6), gh_logw=a(7), eta_mean=a(8), eta_var=a(9), pmean=a(10), lpd=a(11), elpd=a(12)):
        return lib.gsmvi_glm_predict_batched_f64(None, None, K, D, M, family, A, offset, y, counts, tau, tau_dev, mean, cov, Q, gh_t,
                                                 gh_logw, eta_mean, eta_var, pmean, lpd, elpd)

    assert call(D=0) == 1 and "D must be" in err() and name in err()
    assert call(D=65) == 1 and "D must be" in err()
    assert call(K=0) == 1 and "K must be" in err()
    assert call(M=0) == 1 and "M must be" in err()
    assert call(K=2 ** 20, M=2 ** 40) == 1 and "too large" in err()
    for fam in (-1, 4):
        assert call(family=fam) == 1 and "family" in err(), fam
    assert call(Q=0) == 1 and "Q must be" in err()
    assert call(Q=65) == 1 and "Q must be" in err()
    for arr in ("A", "mean", "cov", "gh_t", "gh_logw", "eta_mean", "eta_var", "pmean"):
        assert call(**{arr: None}) == 1 and "NULL array" in err(), arr
    assert call(y=None) == 1 and "required with y" in err()                      # lpd and elpd without y
    assert call(y=None, elpd=None) == 1 and "required with y" in err()           # lpd without y
    assert call(y=None, lpd=None) == 1 and "required with y" in err()            # elpd without y
    assert call(lpd=None) == 1 and "required with y" in err()                    # y without lpd
    assert call(elpd=None) == 1 and "required with y" in err()
    assert call(tau=2.0) == 1 and "noise_prec" in err()
    assert call(tau_dev=a(13)) == 1 and "noise_prec" in err()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(family=3, tau=bad) == 1 and "noise_prec" in err(), bad
    for w in ("eta_mean", "eta_var", "pmean", "lpd", "elpd"):
        for arr, where in (("A", a(0)), ("offset", a(1)), ("y", a(2)), ("counts_dev", a(3)), ("mean", a(4)), ("cov", a(5)),
                           ("gh_t", a(6)), ("gh_logw", a(7))):
            assert call(**{w: where}) == 1 and f"{w} overlaps {arr}" in err(), (w, arr)
    assert call(eta_var=a(8)) == 1 and "eta_var overlaps eta_mean" in err()
    assert call(family=3, tau_dev=a(13), pmean=a(13)) == 1 and "pmean overlaps noise_prec_dev" in err()
    assert call(eta_mean=a(4) + 8 * (2 * 4 - 1)) == 1 and "eta_mean overlaps mean" in err()     # the last element of mean
    assert call(eta_mean=a(4) + 8 * 2 * 4) == 1 and "ctx is NULL" in err()                      # adjacent is not overlapping
    for fam in (0, 1, 2, 3):
        assert call(family=fam) == 1 and "ctx is NULL" in err(), fam
        assert call(family=fam, y=None, lpd=None, elpd=None, offset=None, counts=None) == 1 and "ctx is NULL" in err(), fam
    assert call(family=3, tau=2.5) == 1 and "ctx is NULL" in err()
    assert call(family=3, tau=-1.0, tau_dev=a(13)) == 1 and "ctx is NULL" in err()              # the scalar is unused with K values
    assert call(Q=1) == 1 and "ctx is NULL" in err()
    assert call(Q=64) == 1 and "ctx is NULL" in err()
    assert call(y=a(0), offset=a(0), counts=a(0), mean=a(0), cov=a(0)) == 1 and "ctx is NULL" in err()   # read-only arrays may overlap
