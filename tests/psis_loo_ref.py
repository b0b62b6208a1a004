"""Numpy restatement of the batched PSIS leave-one-out (gsmvi_psis_loo_batched_f64, csrc/gsmvi_psis_loo_batched.hip) in
np.longdouble (``dtype=np.float64`` is the switch that measures the float64 noise floor of the same arithmetic), the generator
of its test inputs, the closed-form leave-one-out density of the conjugate Gaussian model it is pinned to, and a stand-in engine
for the host logic of ``psis_loo_batched``.  Test-only.  Written from the definition in include/gsmvi_hip.h: for problem k, draws
x_s of q_k and row i < n_k

    eta_si = a_i . x_s + offset_i
    l_si   = t(eta_si, y_i)  [- lgamma(y_i + 1) poisson]  [+ log(tau_k / 2 pi) / 2 gaussian],  NaN where the link flags the draw
    rho_si = logr_s - l_si   (one float64 subtraction)
    (w_.i, khat, ess, info) = the PSIS stage on rho_.i: psis_batched_ref.psis_weights, steps 1-8
    elpd_i = log sum_s exp(w_si + l_si),   lpd_i = log sum_s exp(lw_s + l_si)     (max first, then the sum of exp(. - max))

rows i >= n_k: NaN and info = -3; info = -1: the four outputs NaN.  scipy.special supplies erfcx and lgamma in double."""
import ctypes as C
import functools

import numpy as np
from scipy import special

import glm_batched_ref as gref
import glm_predict_ref as pref_glm
import psis_batched_ref as pref

LD = np.longdouble
PATH_BIT = 0x400000
FAMILIES = gref.FAMILIES
FAMILY_CODE = {"logistic": 0, "poisson": 1, "probit": 2, "gaussian": 3}
NI_CAP = 4
LDS_MAX_DOUBLES = 160 * 1024 // 8

# The bar of elpd, lpd, khat and ess on the GPU, relative to max(1, |value|): 1000 times the float64 noise floor of this restatement.
# NOISE_FLOOR is the largest gap between its float64 and longdouble runs over every case of CASES (both fed the same float64
# l_si, logr and lw; rows whose verdict differs between the two precisions left out), measured by
# tests/test_psis_loo_cpu.py::test_float64_noise_floor_of_the_restatement_on_the_gpu_inputs: 1.42e-14, at ess; khat 3.7e-15, elpd
# 9.0e-16, lpd 2.9e-16; no row of the 230 changes its verdict.  (l_si itself: 1.4e-15 between the two precisions.)
NOISE_FLOOR = 1.5e-14
BAR = 1000 * NOISE_FLOOR
LOGLIK_BAR = 1e-11                  # the project's single-launch bar, for l_si against the longdouble restatement

# The Monte-Carlo gap of elpd_i against the closed-form leave-one-out density of the conjugate Gaussian model, q the exact
# posterior, S = 4096, lam = tau = 1, seeds 0 .. 4 of gaussian_exact_problem (float64 run of this restatement): the largest
# |elpd_i - closed form| over the rows and seeds at each (N, D), and the bound of the test, twice that for the draw-to-draw spread.
# (The largest pointwise khat of these runs: 0.91, 0.65, 0.61; sum p_loo / D between 0.45 and 1.21; the problem-level khat below
# -0.17.  With q widened 1.5 times the largest pointwise khat is 0.28, 0.21, 0.35.)
GAUSS_SHAPES = ((20, 3), (40, 5), (64, 10))
GAUSS_SEEDS = (0, 1, 2, 3, 4)
GAUSS_S = 4096
GAUSS_GAP = {(20, 3): 0.0815, (40, 5): 0.0699, (64, 10): 0.0584}
GAUSS_BOUND = {k: 2.0 * v for k, v in GAUSS_GAP.items()}


def loo_tile(D, S):
    """NI of gsmvi_psis_loo_tile(D, S) from the header's formula"""
    if not (1 <= D <= 64 and 5 <= S <= 4096):
        return 0
    S2 = 8
    while S2 < S:
        S2 *= 2
    stage = S2 + S + 508 + S2 // 2
    tiles = 80 * (16 * ((D + 15) // 16) + 1) + 48
    return min(NI_CAP, (LDS_MAX_DOUBLES - max(stage, tiles)) // S)


def valid_rows(counts, K, N):
    return np.full(K, N) if counts is None else np.clip(np.asarray(counts, dtype=np.int64), 0, N)


def loglik(family, A, y, offset, counts, tau, X, dtype=LD):
    """l_si as (K, N, S) of ``dtype``; NaN for rows i >= n_k and for flagged draws"""
    A, y, X = (np.asarray(a, dtype=np.float64) for a in (A, y, X))
    K, N, D = A.shape
    S = X.shape[1]
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (K,))
    nk = valid_rows(counts, K, N)
    out = np.full((K, N, S), np.nan, dtype=dtype)
    pi = dtype(4) * np.arctan(dtype(1))
    for k in range(K):
        n = int(nk[k])
        if n == 0:
            continue
        with np.errstate(all="ignore"):
            eta = A[k, :n].astype(dtype) @ X[k].astype(dtype).T                      # (n, S)
            if offset is not None:
                eta = eta + np.asarray(offset, dtype=np.float64)[k, :n, None].astype(dtype)
            yk = y[k, :n, None].astype(dtype)
            if family == "gaussian":
                d = yk - eta
                ell = -(dtype(tau[k]) * (d * d)) / dtype(2) + np.log(dtype(tau[k]) / (dtype(2) * pi)) / dtype(2)
            elif family == "probit":
                ell = gref.link("probit", np.asarray(eta, dtype=np.float64), y[k, :n, None])[1].astype(dtype)
            else:
                ell = pref_glm._t(family, eta, yk)
                if family == "poisson":
                    ell = ell - special.gammaln(y[k, :n, None] + 1.0).astype(dtype)
                    ell = np.where(np.exp(np.asarray(eta, dtype=np.float64)) < np.inf, ell, dtype(np.nan))
        out[k, :n] = ell
    return out


def lse(v, dtype=LD):
    """log sum exp of the last axis: the maximum first, then the sum of exp(. - max)"""
    v = np.asarray(v).astype(dtype)
    with np.errstate(all="ignore"):
        mx = v.max(-1)
        return mx + np.log(np.exp(v - mx[..., None]).sum(-1))


def loo_rows(ell, logr, lw, n, dtype=LD):
    """one problem: ell (N, S) float64 l_si, logr and lw (S,), n valid rows -> dict of elpd, lpd, khat, ess (N,) of ``dtype`` and
    info (N,)"""
    ell, logr, lw = (np.asarray(a, dtype=np.float64) for a in (ell, logr, lw))
    N = ell.shape[0]
    nan = dtype(np.nan)
    out = {name: np.full(N, nan, dtype=dtype) for name in ("elpd", "lpd", "khat", "ess")}
    out["info"] = np.full(N, -3, dtype=np.int64)
    for i in range(n):
        with np.errstate(all="ignore"):
            rho = logr - ell[i]                                                  # float64, as on the device
        r = pref.psis_weights(rho, dtype)
        out["info"][i] = r["info"]
        if r["info"] == -1:
            continue
        out["khat"][i], out["ess"][i] = r["khat"], r["ess"]
        out["elpd"][i] = lse(np.asarray(r["lw"], dtype=dtype) + ell[i].astype(dtype), dtype)
        out["lpd"][i] = lse(lw.astype(dtype) + ell[i].astype(dtype), dtype)
    return out


def loo_batched(ell, logr, lw, counts=None, dtype=LD):
    """K problems: ell (K, N, S), logr and lw (K, S) -> dict of (K, N) arrays"""
    ell = np.asarray(ell, dtype=np.float64)
    K, N, _ = ell.shape
    nk = valid_rows(counts, K, N)
    rs = [loo_rows(ell[k], logr[k], lw[k], int(nk[k]), dtype) for k in range(K)]
    return {name: np.stack([r[name] for r in rs]) for name in ("elpd", "lpd", "khat", "ess", "info")}


def summaries(r, counts, S):
    """the per-problem fields of LOOBatchedResult from the pointwise ones, in float64"""
    e, lp, kh = (np.asarray(r[n], dtype=np.float64) for n in ("elpd", "lpd", "khat"))
    info = np.asarray(r["info"])
    K, N = e.shape
    nk = valid_rows(counts, K, N)
    mask = np.arange(N)[None, :] < nk[:, None]
    thr = pref.threshold(S)
    with np.errstate(all="ignore"):
        elpd_loo = np.where(mask, e, 0.0).sum(1)
        p_loo = np.where(mask, lp - e, 0.0).sum(1)
        dev = np.where(mask, e - (elpd_loo / nk)[:, None], 0.0)
        se = np.where(nk >= 2, np.sqrt(nk * ((dev * dev).sum(1) / (nk - 1.0))), np.nan)
        n_bad = (mask & ((info != 0) | (kh >= thr))).sum(1)
    return dict(elpd_loo=elpd_loo, p_loo=p_loo, se=se, n_bad=n_bad)


# ---- the conjugate Gaussian model: the closed-form leave-one-out density ---------------------------------------------------------
def gaussian_exact_problem(N, D, seed, lam=1.0, tau=1.0):
    """A (N, D) = N(0, 1) / sqrt(D), theta* ~ N(0, I), y = A theta* + noise of precision tau; the exact posterior (mean, cov)"""
    rs = np.random.default_rng([seed, N, D])
    A = rs.standard_normal((N, D)) / np.sqrt(D)
    y = A @ rs.standard_normal(D) + rs.standard_normal(N) / np.sqrt(tau)
    P = lam * np.eye(D) + tau * A.T @ A
    cov = np.linalg.inv(P)
    cov = 0.5 * (cov + cov.T)
    return dict(A=A, y=y, lam=lam, tau=tau, mean=cov @ (tau * A.T @ y), cov=cov, P=P, rs=rs)


def gaussian_exact_loo(p):
    """log N(y_i | a_i . m_-i, 1 / tau + a_i^T Sigma_-i a_i) with (m_-i, Sigma_-i) the posterior without row i"""
    A, y, tau = p["A"], p["y"], p["tau"]
    out = np.empty(A.shape[0])
    b = tau * A.T @ y
    for i in range(A.shape[0]):
        Si = np.linalg.inv(p["P"] - tau * np.outer(A[i], A[i]))
        mi = Si @ (b - tau * A[i] * y[i])
        var = 1.0 / tau + A[i] @ Si @ A[i]
        out[i] = -0.5 * np.log(2 * np.pi * var) - 0.5 * (y[i] - A[i] @ mi) ** 2 / var
    return out


def gaussian_restatement_run(p, S, widen=1.0, dtype=np.float64):
    """the restatement on S draws of q = N(mean, widen^2 cov) of the problem: (loo dict of (N,) arrays, problem-level khat)"""
    A, y = p["A"], p["y"]
    cov = widen * widen * p["cov"]
    X = p["mean"][None, :] + p["rs"].standard_normal((S, A.shape[1])) @ np.linalg.cholesky(cov).T
    _, lp = gref.score_and_lp("gaussian", A[None], y[None], None, None, p["lam"], p["tau"], X[None])
    logr, info = pref.log_ratios(p["mean"], cov, X, lp[0], np.float64)
    assert info == 0
    top = pref.psis_weights(np.asarray(logr, dtype=np.float64), dtype)
    ell = loglik("gaussian", A[None], y[None], None, None, p["tau"], X[None], np.float64)[0]
    r = loo_rows(ell, np.asarray(logr, dtype=np.float64), np.asarray(top["lw"], dtype=np.float64), A.shape[0], dtype)
    return r, float(top["khat"])


# ---- the inputs of the GPU tests (tests/test_gpu_psis_loo.py) and of the noise-floor measurement -------------------------------------
# (family, with offset, D, S, N as a function of NI = loo_tile(D, S), K): every value of each axis at least once, the N edges at
# D = 10 and D = 64.  K = 3 runs with counts = (0, a partial value, N), K = 1 without counts.
N_OF = {"1": lambda ni: 1, "NI-1": lambda ni: max(1, ni - 1), "NI": lambda ni: ni, "NI+1": lambda ni: ni + 1,
        "2NI+3": lambda ni: 2 * ni + 3}
CASES = (
    ("logistic", False, 1, 5, "1", 1),
    ("logistic", True, 2, 33, "NI-1", 3),
    ("poisson", True, 15, 257, "NI", 3),
    ("poisson", False, 16, 33, "NI+1", 1),
    ("probit", False, 17, 257, "2NI+3", 3),
    ("probit", True, 33, 33, "NI+1", 1),
    ("gaussian", True, 64, 257, "2NI+3", 3),
    ("gaussian", False, 16, 5, "NI", 3),
) + tuple(("logistic", bool(j % 2), 10, 33, n, 3) for j, n in enumerate(N_OF)) \
  + tuple(("poisson", bool(j % 2), 64, 33, n, 1 + 2 * (j % 2)) for j, n in enumerate(N_OF)) + (
    ("logistic", True, 10, 1024, "NI+1", 1),
    ("gaussian", False, 64, 4096, "NI+1", 1),
)


def case_id(c):
    return f"{c[0]}-{'off' if c[1] else 'nooff'}-D{c[2]}-S{c[3]}-N{c[4]}-K{c[5]}"


@functools.lru_cache(maxsize=None)
def make_case(case):
    """The inputs of one case (computed once and shared: do not modify): the model (A, y, offset, counts, tau), S draws X of a
    Gaussian q_k near the posterior, and the problem-level logr and lw of psis_batched_ref on them, all float64."""
    family, with_offset, D, S, nspec, K = case
    N = N_OF[nspec](loo_tile(D, S))
    rs = np.random.default_rng([D, S, N, K, FAMILY_CODE[family]])
    A = rs.standard_normal((K, N, D)) / np.sqrt(D)
    offset = 0.3 * rs.standard_normal((K, N)) if with_offset else None
    theta = 0.7 * rs.standard_normal((K, D))
    eta = np.einsum("knd,kd->kn", A, theta) + (offset if with_offset else 0.0)
    tau = 0.5 + rs.uniform(size=K) if family == "gaussian" else 1.0
    if family == "logistic":
        y = (rs.uniform(size=(K, N)) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    elif family == "probit":
        y = (rs.uniform(size=(K, N)) < special.ndtr(eta)).astype(np.float64)
    elif family == "poisson":
        y = rs.poisson(np.exp(np.minimum(eta, 5.0))).astype(np.float64)
    else:
        y = eta + rs.standard_normal((K, N)) / np.sqrt(tau)[:, None]
    counts = np.array([0, max(1, N // 2), N], dtype=np.int32) if K == 3 else None
    mean = 0.8 * theta + 0.1 * rs.standard_normal((K, D))
    G = rs.standard_normal((K, D, D)) / np.sqrt(D)
    cov = np.linalg.inv(np.eye(D)[None] + 0.25 * np.swapaxes(A, 1, 2) @ A + 0.1 * G @ np.swapaxes(G, 1, 2))
    cov = 0.5 * (cov + np.swapaxes(cov, 1, 2))
    X = mean[:, None, :] + np.einsum("ksj,kij->ksi", rs.standard_normal((K, S, D)), np.linalg.cholesky(cov))
    _, lp = gref.score_and_lp(family, A, y, offset, counts, 1.0, tau, X)
    logr, lw = np.empty((K, S)), np.empty((K, S))
    for k in range(K):
        lr, info = pref.log_ratios(mean[k], cov[k], X[k], lp[k], np.float64)
        assert info == 0
        logr[k] = lr
        lw[k] = np.asarray(pref.psis_weights(logr[k], np.float64)["lw"], dtype=np.float64)
    return dict(family=family, K=K, N=N, D=D, S=S, A=A, y=y, offset=offset, counts=counts, tau=tau, mean=mean, cov=cov, X=X,
                logr=logr, lw=lw)


def rel_gap(a, b, keep=None):
    """psis_batched_ref.rel_gap over the entries selected by ``keep`` (a boolean array, None: all)"""
    a, b = np.asarray(a), np.asarray(b)
    if keep is not None:
        a, b = a[keep], b[keep]
    return pref.rel_gap(a, b)


# ---- the stand-in engine of the host-logic tests -----------------------------------------------------------------------------------
class StandInEngine(pref.StandInEngine):
    """psis_batched_ref's stand-in engine with what BatchedGLMTarget asks of an engine (glm_batched_ref's restatement) and the
    leave-one-out launch restated (this file, float64 out).  ``calls`` records the launches as tuples."""
    name = "oracle-batched-loo(test-only)"

    def to_numpy(self, a):
        return np.asarray(a)

    def batched_counts(self, values):
        return np.asarray(values, dtype=np.int32).reshape(-1)

    def batched_regs(self, values):
        return np.asarray(values, dtype=np.float64).reshape(-1)

    def glm_batched(self, X, A, y, family, offset=None, counts=None, prior_prec=1.0, noise_prec=1.0, out=None, lp_out=None, want="g"):
        self._rec(("glm", family, want))
        G, lp = gref.score_and_lp(family, A, y, offset, counts, prior_prec, noise_prec, X)
        return G if want == "g" else lp if want == "lp" else (G, lp)

    def psis_loo_batched(self, X, logr, lw, A, y, family, offset=None, counts=None, noise_prec=1.0, pointwise_loglik=False):
        self._rec(("loo", family, tuple(X.shape), tuple(A.shape), offset is not None, counts is not None, bool(pointwise_loglik)))
        ell = np.asarray(loglik(family, A, y, offset, counts, noise_prec, X), dtype=np.float64)
        r = loo_batched(ell, np.asarray(logr), np.asarray(lw), counts)
        f = lambda n: np.asarray(r[n], dtype=np.float64)                         # noqa: E731
        return f("elpd"), f("lpd"), f("khat"), f("ess"), r["info"], (ell if pointwise_loglik else None)


# ---- the C ABI's argument checks (NULL context) ------------------------------------------------------------------------------------
def check_bad_arguments(lib):
    """the entry point through the C ABI with a NULL context: every bad argument returns GSMVI_ERR_BAD_ARG (1) with its own
    message, so nothing can have been enqueued; valid calls end at the context"""
    err = lambda: (lib.gsmvi_last_error() or b"").decode()          # noqa: E731
    buf = (C.c_double * 32768)()
    p = C.cast(buf, C.c_void_p).value
    at = lambda i: p + 8 * 1024 * i                                   # noqa: E731  (slots of 8 KB: K = 2, N = 5, D = 4, S = 8 fit)
    name = "gsmvi_psis_loo_batched_f64"
    names = dict(A=at(0), y=at(1), offset=at(2), counts=at(3), tau_dev=None, X=at(4), logr=at(5), lw=at(6), loglik=at(7), elpd=at(8),
                 lpd=at(9), khat=at(10), ess=at(11), info=at(12))

    def call(family=1, K=2, N=5, D=4, S=8, tau=1.0, **kw):
        a = dict(names, **kw)
        return lib.gsmvi_psis_loo_batched_f64(None, None, family, K, N, D, S, a["A"], a["y"], a["offset"], a["counts"], tau,
                                              a["tau_dev"], a["X"], a["logr"], a["lw"], a["loglik"], a["elpd"], a["lpd"], a["khat"],
                                              a["ess"], a["info"])

    assert call(D=0) == 1 and "D must be" in err() and name in err()
    assert call(D=65) == 1 and "D must be" in err()
    assert call(K=0) == 1 and "K must be" in err()
    assert call(N=0) == 1 and "N must be" in err()
    assert call(S=4) == 1 and "S must be" in err()
    assert call(S=4097) == 1 and "S must be" in err()
    assert call(K=2 ** 20, N=2 ** 40) == 1 and "too large" in err()
    assert call(K=2 ** 20, N=2 ** 30, S=4096) == 1 and "too large" in err()
    assert call(K=2 ** 22, N=64) == 1 and "2^24 - 1" in err()                      # K ceil(N / NI) tiles
    assert call(K=2 ** 25) == 1 and ("2^24 - 1" in err() or "K must be" in err())
    for fam in (-1, 4):
        assert call(family=fam) == 1 and "family" in err(), fam
    for arr in ("A", "y", "X", "logr", "lw", "elpd", "lpd", "khat", "ess", "info"):
        assert call(**{arr: None}) == 1 and "NULL array" in err(), arr
    assert call(tau=2.0) == 1 and "noise_prec" in err()
    assert call(tau_dev=at(13)) == 1 and "noise_prec" in err()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(family=3, tau=bad) == 1 and "noise_prec" in err(), bad
    for w in ("loglik", "elpd", "lpd", "khat", "ess", "info"):
        for arr, key in (("A", "A"), ("y", "y"), ("offset", "offset"), ("counts_dev", "counts"), ("X", "X"), ("logr", "logr"),
                         ("lw", "lw")):
            assert call(**{w: names[key]}) == 1 and f"{w} overlaps {arr}" in err(), (w, arr)
    assert call(lpd=names["elpd"]) == 1 and "lpd overlaps elpd" in err()
    assert call(info=names["ess"] + 4) == 1 and "info overlaps ess" in err()
    assert call(khat=names["loglik"] + 8 * (2 * 5 * 8 - 1)) == 1 and "khat overlaps loglik" in err()     # the last element
    assert call(khat=names["loglik"] + 8 * 2 * 5 * 8) == 1 and "ctx is NULL" in err()                    # adjacent is not overlapping
    assert call(family=3, tau_dev=at(13), ess=at(13)) == 1 and "ess overlaps noise_prec_dev" in err()
    for fam in (0, 1, 2, 3):
        assert call(family=fam) == 1 and "ctx is NULL" in err(), fam
        assert call(family=fam, offset=None, counts=None, loglik=None) == 1 and "ctx is NULL" in err(), fam
    assert call(family=3, tau=2.5) == 1 and "ctx is NULL" in err()
    assert call(S=5) == 1 and "ctx is NULL" in err()
    assert call(S=16, D=8) == 1 and "ctx is NULL" in err()
    assert call(y=names["A"], offset=names["A"], X=names["A"], logr=names["A"], lw=names["A"]) == 1 and "ctx is NULL" in err()
