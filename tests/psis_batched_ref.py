"""Numpy restatement of the batched Pareto-smoothed importance diagnostic (gsmvi_psis_batched_f64 and
gsmvi_psis_weights_batched_f64, csrc/gsmvi_psis_batched.hip), in np.longdouble (``dtype=np.float64`` is the switch that measures
the float64 noise floor of the same arithmetic).  Written from the definition in include/gsmvi_hip.h and nothing else:

  (a) logq_s = -|w_s|^2 / 2 - sum_i log R_ii - D / 2 log 2 pi with R the upper Cholesky factor of cov_k (right-looking
      elimination; a pivot that is not > 0 and finite: info = 1 + that pivot, every output NaN) and R^T w_s = x_s - mean_k;
      logr_s = lp_s - logq_s
  (b) the PSIS stage on logr: ``psis_weights`` below, step by step (Vehtari, Simpson, Gelman, Yao, Gabry, JMLR 2024; the tail
      fit of Zhang & Stephens 2009 with the weakly informative prior: ``gpd_fit``)
  (c) w_s = exp(lw_s), d_s = x_s - mean_k: mean_is = mean_k + sum w_s d_s, cov_is = sum w_s d_s d_s^T - (sum w d)(sum w d)^T

The order of the sort is (value, index) -- numpy's stable argsort -- so tied entries get the same smoothed values as on the
device.  The float64 run of (b) rounds as the device does wherever the order of the operations is fixed by the definition; the
sums are numpy's (pairwise), the device's are a fixed tree: the bar of the GPU tests is 1000 times the float64-to-longdouble
gap of this file (tests/test_psis_batched_cpu.py measures it).  The stand-in engine at the end serves the host-logic tests."""
import ctypes as C

import numpy as np

from engines import OracleBatchedEngine
from oracle import gsm_oracle as orc

LD = np.longdouble
MIN_S, MAX_S, MAX_D = 5, 4096, 64
PATH_BIT = 0x200000


def tail_size(S):
    """M = ceil(min(S / 5, 3 sqrt(S)))"""
    return int(np.ceil(min(S / 5.0, 3.0 * np.sqrt(float(S)))))


def threshold(S):
    return min(1.0 - 1.0 / np.log10(S), 0.7)


def gpd_fit(x, dtype=LD):
    """(khat, sigma) of the generalised Pareto fit to the ascending exceedances x (n > 4 of them): step 5 of the definition"""
    x = np.asarray(x, dtype=dtype)
    n = x.shape[0]
    m = 30 + int(np.floor(np.sqrt(n)))
    j = np.arange(1, m + 1, dtype=dtype)
    one, half = dtype(1), dtype(0.5)
    with np.errstate(all="ignore"):
        b = (one - np.sqrt(dtype(m) / (j - half))) / (dtype(3) * x[(n + 2) // 4 - 1]) + one / x[n - 1]
        kap = np.log1p(-b[:, None] * x[None, :]).sum(1) / dtype(n)
        L = dtype(n) * (np.log(-b / kap) - kap - one)
        om = one / np.exp(L[None, :] - L[:, None]).sum(1)
        om = np.where(om < dtype(10 * np.finfo(np.float64).eps), dtype(0), om)
        om = om / om.sum()
        bb = (om * b).sum()
        kappa = np.log1p(-bb * x).sum() / dtype(n)
        sigma = -kappa / bb
        khat = (dtype(n) * kappa + dtype(5)) / dtype(n + 10)
    return khat, sigma


def psis_weights(logr, dtype=LD):
    """One problem: dict(lw (S,), khat, ess, log_z, info, n) from logr (S,), steps 1-8 of the definition"""
    logr = np.asarray(logr, dtype=np.float64).astype(dtype)
    S = logr.shape[0]
    assert MIN_S <= S <= MAX_S
    nan = dtype(np.nan)
    mx = logr.max() if not np.isnan(logr).any() else nan
    if np.isnan(logr).any() or np.isposinf(logr).any() or np.isneginf(mx):
        return dict(lw=np.full(S, nan), khat=nan, ess=nan, log_z=nan, info=-1, n=0)
    with np.errstate(all="ignore"):
        lw = logr - mx
        M = tail_size(S)
        order = np.argsort(lw, kind="stable")
        srt = lw[order]
        cutoff = max(srt[S - M - 1], np.log(dtype(np.finfo(np.float64).tiny)))
        n = int((srt > cutoff).sum())
        info, khat = 0, dtype(np.inf)
        if n <= 4:
            info = -2
        else:
            ec = np.exp(cutoff)
            khat, sigma = gpd_fit(np.exp(srt[S - n:]) - ec, dtype)
            if np.isfinite(khat):
                p = (np.arange(n, dtype=dtype) + dtype(0.5)) / dtype(n)
                q = -sigma * np.log1p(-p) if khat == 0 else sigma * np.expm1(-khat * np.log1p(-p)) / khat
                srt = srt.copy()
                srt[S - n:] = np.log(q + ec)
        srt = np.where(srt > 0, dtype(0), srt)
        lse = np.log(np.exp(srt).sum())
        out = np.empty(S, dtype=dtype)
        out[order] = srt - lse
        ess = dtype(1) / np.exp(dtype(2) * out).sum()
        log_z = lse + mx - np.log(dtype(S))
    return dict(lw=out, khat=khat, ess=ess, log_z=log_z, info=info, n=n)


def chol_upper(cov, dtype=LD):
    """(R, info): right-looking upper Cholesky of the upper triangle of cov; info = 1 + the first pivot not > 0 and finite"""
    A = np.array(cov, dtype=np.float64).astype(dtype)
    D = A.shape[0]
    R = np.zeros((D, D), dtype=dtype)
    with np.errstate(all="ignore"):
        for c in range(D):
            if not (A[c, c] > 0 and np.isfinite(A[c, c])):
                return None, c + 1
            R[c, c] = np.sqrt(A[c, c])
            R[c, c + 1:] = A[c, c + 1:] / R[c, c]
            for i in range(c + 1, D):
                A[i, i:] -= R[c, i] * R[c, i:]
    return R, 0


def log_ratios(mean, cov, X, lp, dtype=LD):
    """(logr (S,), info): stage (a) of one problem"""
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    S, D = X.shape
    R, info = chol_upper(cov, dtype)
    if info:
        return np.full(S, dtype(np.nan)), info
    d = X - np.asarray(mean, dtype=np.float64).astype(dtype)[None, :]
    w = np.zeros_like(d)
    for j in range(D):                                   # R^T w = d by forward substitution
        w[:, j] = (d[:, j] - w[:, :j] @ R[:j, j]) / R[j, j]
    log2pi = np.log(dtype(8) * np.arctan(dtype(1)))      # (pi to the precision of dtype)
    logq = -(w * w).sum(1) / dtype(2) - np.log(np.diag(R)).sum() - dtype(D) * log2pi / dtype(2)
    with np.errstate(all="ignore"):
        return np.asarray(lp, dtype=np.float64).astype(dtype) - logq, 0


def moments(mean, X, lw, dtype=LD):
    """(mean_is, cov_is): stage (c) of one problem"""
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    mean = np.asarray(mean, dtype=np.float64).astype(dtype)
    with np.errstate(all="ignore"):
        w = np.exp(np.asarray(lw).astype(dtype))
        d = X - mean[None, :]
        m1 = (w[:, None] * d).sum(0)
        C2 = np.einsum("s,si,sj->ij", w, d, d) - np.outer(m1, m1)
    return mean + m1, C2


def weights_batched(logr, dtype=LD):
    """dict of (K, ...) arrays from logr (K, S)"""
    logr = np.asarray(logr, dtype=np.float64)
    rs = [psis_weights(row, dtype) for row in logr]
    return dict(lw=np.stack([r["lw"] for r in rs]), khat=np.array([r["khat"] for r in rs], dtype=dtype),
                ess=np.array([r["ess"] for r in rs], dtype=dtype), log_z=np.array([r["log_z"] for r in rs], dtype=dtype),
                info=np.array([r["info"] for r in rs], dtype=np.int64), n=np.array([r["n"] for r in rs]))


def fused_batched(mean, cov, X, lp, with_moments=True, dtype=LD, logr=None):
    """The fused entry on K problems.  ``logr`` (K, S) given: stages (b) and (c) run on it (the device's own ratios) in place
    of stage (a)'s -- a problem whose covariance fails its Cholesky test is still all NaN, with its pivot code."""
    mean, cov, X, lp = (np.asarray(a, dtype=np.float64) for a in (mean, cov, X, lp))
    K, S, D = X.shape
    lr = np.empty((K, S), dtype=dtype)
    pivot = np.zeros(K, dtype=np.int64)
    for k in range(K):
        lr[k], pivot[k] = log_ratios(mean[k], cov[k], X[k], lp[k], dtype)
    # stage (b) reads float64 ratios, as the device's does
    src = lr.astype(np.float64) if logr is None else np.where(pivot[:, None] != 0, np.nan, np.asarray(logr, dtype=np.float64))
    out = weights_batched(src, dtype)
    out["logr"] = lr
    out["info"] = np.where(pivot != 0, pivot, out["info"])
    if with_moments:
        mi, ci = np.empty((K, D), dtype=dtype), np.empty((K, D, D), dtype=dtype)
        for k in range(K):
            mi[k], ci[k] = moments(mean[k], X[k], out["lw"][k], dtype)
        out["mean_is"], out["cov_is"] = mi, ci
    return out


def rel_gap(a, b, floor_lw=None):
    """max |a - b| / max(1, |b|) over the entries where both are finite; entries that are not must agree exactly (NaN with
    NaN, an infinity with the same one).  ``floor_lw``: entries of b below it are left out (lw below -700)."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    assert a.shape == b.shape, (a.shape, b.shape)
    fin = np.isfinite(a) & np.isfinite(b)
    rest = ~fin
    assert np.array_equal(np.isnan(a[rest]), np.isnan(b[rest])) and np.array_equal(a[rest][~np.isnan(a[rest])], b[rest][~np.isnan(b[rest])]), \
        "non-finite entries differ"
    if floor_lw is not None:
        fin &= b >= floor_lw
    if not fin.any():
        return 0.0
    return float((np.abs(a[fin] - b[fin]) / np.maximum(1, np.abs(b[fin]))).max())


# ---- the inputs of the GPU tests (tests/test_gpu_psis_batched.py) and of the noise-floor measurement -----------------------
WEIGHT_S = (5, 20, 25, 33, 64, 100, 257, 1000, 4096)
WEIGHT_K = (1, 3, 9)
FUSED_D = (1, 2, 15, 16, 17, 33, 64)
FUSED_S = (33, 257)
FUSED_K = (1, 5)


def gaussian_ratio_rows(rs, S, D, s):
    """log N(x; 0, s I) - log N(x; 0, I) at S draws x of N(0, I_D): the true tail shape is 1 - 1 / s"""
    x = rs.standard_normal((S, D))
    r2 = (x * x).sum(1)
    return -0.5 * r2 / s - 0.5 * D * np.log(s) + 0.5 * r2


def weight_inputs(kind, K, S, seed=0):
    """logr (K, S) of one of the five kinds of the weights-entry tests"""
    rs = np.random.default_rng([seed, K, S, sum(map(ord, kind))])
    if kind == "gaussian":
        scales = (0.5, 1.25, 4.0)
        return np.stack([gaussian_ratio_rows(rs, S, 1 + (k % 4), scales[k % 3]) for k in range(K)])
    if kind == "pareto":                                     # log of Pareto draws of shape 0.9: u^-0.9
        return -0.9 * np.log(rs.uniform(size=(K, S))) + rs.normal(size=(K, 1)) * 50.0
    if kind == "ties":                                       # blocks of exactly tied values, ties across the cutoff included
        out = np.empty((K, S))
        for k in range(K):
            levels = np.sort(rs.normal(size=max(2, S // (3 + k))))
            v = levels[rs.integers(0, levels.shape[0], size=S)]
            M = tail_size(S)
            top = np.argsort(v, kind="stable")
            v[top[S - M - 1 - min(2, S - M - 1):S - M + 1 + (k % 2)]] = v[top[S - M - 1]]      # a tie that straddles S - M - 1
            out[k] = v
        return out
    if kind == "nan":                                        # one problem with a NaN (or +inf) among healthy neighbours
        out = weight_inputs("gaussian", K, S, seed + 1)
        out[K // 2, S // 3] = np.nan if K != 3 else np.inf
        return out
    if kind == "neginf":
        out = weight_inputs("pareto", K, S, seed + 2)
        out[0, ::3] = -np.inf
        if K > 1:
            out[K - 1, :] = -np.inf                          # every row: info = -1
            out[K - 1, 0] = -np.inf
        return out
    raise ValueError(kind)


WEIGHT_KINDS = ("gaussian", "pareto", "ties", "nan", "neginf")


def fused_inputs(target, K, D, S, seed=0):
    """dict(mean, cov, X, lp, and what builds the target) of one fused-entry case: X are draws of q_k, lp_k the rows' values of
    a Gaussian target (``gauss``: mean mt, covariance ct) or a small logistic GLM (``glm``: A (K, 8, D), y, unit prior)"""
    rs = np.random.default_rng([seed, K, D, S, sum(map(ord, target))])
    mean = rs.normal(size=(K, D)) * 0.3
    A = rs.normal(size=(K, D, D)) / np.sqrt(D)
    cov = 0.6 * np.eye(D)[None] + 0.4 * A @ np.swapaxes(A, 1, 2)
    cov = 0.5 * (cov + np.swapaxes(cov, 1, 2))
    L = np.linalg.cholesky(cov)
    X = mean[:, None, :] + np.einsum("ksj,kij->ksi", rs.normal(size=(K, S, D)), L)
    p = dict(mean=mean, cov=cov, X=X)
    if target == "gauss":
        p["mt"] = mean + 0.1 * rs.normal(size=(K, D))
        Bm = rs.normal(size=(K, D, D)) / np.sqrt(D)
        ct = 0.8 * (0.6 * np.eye(D)[None] + 0.4 * Bm @ np.swapaxes(Bm, 1, 2))
        p["ct"] = 0.5 * (ct + np.swapaxes(ct, 1, 2))
        P = np.linalg.inv(p["ct"])
        r = X - p["mt"][:, None, :]
        p["lp"] = -0.5 * np.einsum("ksi,kij,ksj->ks", r, P, r)
    else:
        p["A"] = rs.normal(size=(K, 8, D)) / np.sqrt(D)
        p["y"] = (rs.uniform(size=(K, 8)) < 0.5).astype(np.float64)
        eta = np.einsum("knd,ksd->ksn", p["A"], X)
        p["lp"] = (p["y"][:, None, :] * eta - np.logaddexp(0.0, eta)).sum(2) - 0.5 * (X * X).sum(2)
    return p


# ---- the stand-in engine of the host-logic tests ---------------------------------------------------------------------------
class StandInEngine(OracleBatchedEngine):
    """tests/engines.py's OracleBatchedEngine with the draw launch of the KL monitor and the two PSIS launches restated (this
    file, float64 out).  ``calls`` records every engine call; the launches as tuples."""
    name = "oracle-batched-psis(test-only)"

    def kl_draw_batched(self, mean, cov, seeds, call, s0, nc, out=None, info=None):
        self._rec(("draw", tuple(int(s) for s in seeds), int(call), int(s0), int(nc)))
        K, D = mean.shape
        X, logq, inf = np.empty((K, nc, D)), np.empty(K), np.zeros(K, dtype=np.int64)
        for k in range(K):
            R, inf[k] = chol_upper(cov[k], np.float64)
            if inf[k]:
                X[k], logq[k] = np.nan, np.nan
                continue
            Z = orc.philox_randn(int(seeds[k]), call, (s0 + nc) * D)[s0 * D:].reshape(nc, D)
            X[k] = mean[k][None, :] + Z @ R
            logq[k] = -0.5 * np.sum(Z * Z) - nc * (np.sum(np.log(np.diag(R))) + 0.5 * D * np.log(2 * np.pi))
        return X, logq, inf

    def psis_weights_batched(self, logr):
        self._rec(("psis_weights", tuple(logr.shape)))
        r = weights_batched(logr)
        return tuple(np.asarray(r[n], dtype=np.float64) for n in ("lw", "khat", "ess", "log_z")) + (r["info"],)

    def psis_batched(self, mean, cov, X, lp, moments=True):
        self._rec(("psis", tuple(X.shape), bool(moments)))
        r = fused_batched(mean, cov, X, lp, with_moments=moments)
        f = lambda n: np.asarray(r[n], dtype=np.float64) if n in r else None       # noqa: E731
        return f("logr"), f("lw"), f("khat"), f("ess"), f("log_z"), f("mean_is"), f("cov_is"), r["info"]


# ---- the C ABI's argument checks (NULL context) ------------------------------------------------------------------------------
def check_bad_arguments(lib):
    err = lambda: (lib.gsmvi_last_error() or b"").decode()          # noqa: E731
    buf = (C.c_double * 16384)()
    p = C.cast(buf, C.c_void_p).value
    at = lambda i: p + 8 * 1024 * i                                   # noqa: E731  (slots of 8 KB: K = 2, D = 4, S = 8 fit)
    W = dict(logr=at(0), lw=at(1), khat=at(2), ess=at(3), log_z=at(4), info=at(5))
    F = dict(mean=at(6), cov=at(7), X=at(8), lp=at(9), logr=at(0), lw=at(1), khat=at(2), ess=at(3), log_z=at(4),
             mean_is=at(10), cov_is=at(11), info=at(5))

    def weights(K=2, S=8, **kw):
        a = dict(W, **kw)
        return lib.gsmvi_psis_weights_batched_f64(None, None, K, S, a["logr"], a["lw"], a["khat"], a["ess"], a["log_z"], a["info"])

    def fused(K=2, D=4, S=8, **kw):
        a = dict(F, **kw)
        return lib.gsmvi_psis_batched_f64(None, None, K, D, S, a["mean"], a["cov"], a["X"], a["lp"], a["logr"], a["lw"],
                                          a["khat"], a["ess"], a["log_z"], a["mean_is"], a["cov_is"], a["info"])

    for f, names in ((weights, W), (fused, F)):
        assert f(S=4) == 1 and "S must be" in err()
        assert f(S=4097) == 1 and "S must be" in err()
        assert f(K=0) == 1 and "K must be" in err()
        assert f(K=2 ** 24) == 1 and "K must be" in err()
        for name in names:
            if name not in ("mean_is", "cov_is"):
                assert f(**{name: None}) == 1 and "NULL array" in err(), name
        assert f(lw=names["logr"] + 8) == 1 and "overlap" in err()           # an output over an input (weights) / an output
        assert f(khat=names["lw"]) == 1 and "overlap" in err()
        assert f(info=names["ess"] + 4) == 1 and "overlap" in err()
        assert f() == 1 and "ctx is NULL" in err()
    assert weights(lw=W["logr"]) == 1 and "lw overlaps logr" in err()
    assert fused(D=65) == 1 and "D must be" in err()
    assert fused(D=0) == 1 and "D must be" in err()
    assert fused(logr=F["lp"]) == 1 and "overlap" in err()
    assert fused(lw=F["X"] + 16) == 1 and "overlap" in err()
    assert fused(mean_is=F["mean"]) == 1 and "overlap" in err()
    assert fused(cov_is=None) == 1 and "mean_is and cov_is" in err()
    assert fused(mean_is=None) == 1 and "mean_is and cov_is" in err()
    assert fused(mean_is=None, cov_is=None) == 1 and "ctx is NULL" in err()
    assert fused(lp=F["X"]) == 1 and "ctx is NULL" in err()                  # read-only arrays may overlap
