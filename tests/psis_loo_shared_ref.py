"""Numpy restatement of the shared-design PSIS leave-one-out (gsmvi_psis_loo_shared_batched_f64,
csrc/gsmvi_psis_loo_batched.hip, SHARED) in np.longdouble (``dtype=np.float64`` measures the float64 noise floor of the same
arithmetic), the generator of its test inputs, the closed-form leave-row-out density of the weighted conjugate Gaussian model, and
a stand-in engine for the host logic of ``psis_loo_shared_batched``.  Test-only.  Built on psis_loo_ref (the pointwise likelihood,
the log-sum-exps), psis_batched_ref (the PSIS stage) and shared_glm_ref (the weighted density).  From the definition in
include/gsmvi_hip.h: all K problems have the rows a_i of ONE A (N, D); for problem k with weights v_ki and a row with v_ki > 0

    eta_si = a_i . x_s + o_ki
    l_si   = the log density of ONE unit observation (psis_loo_ref.loglik: unweighted, normalised)
    rho_si = logr_s - v_ki l_si   (float64: one product, one subtraction; weights None: logr_s - l_si)
    (w_.i, khat, ess, info) = psis_batched_ref.psis_weights(rho_.i)
    elpd_i = log sum_s exp(w_si + l_si),   lpd_i = log sum_s exp(lw_s + l_si)

a row with v_ki not > 0 (0 or NaN): NaN and info = -3, whatever y and the offset hold there.  The per-problem sums over the n_k
valid rows: c_i = v_ki elpd_i, elpd_loo = sum c_i, p_loo = sum v_ki (lpd_i - elpd_i), se = sqrt(n_k var(c_i))."""
import ctypes as C
import functools

import numpy as np

import psis_batched_ref as pref
import psis_loo_ref as lref
import shared_glm_ref as sref

LD = np.longdouble
PATH_BITS = 0x400000 | 0x20000        # batched_loo | batched_target (checked against HipEngine.PATH_BITS by the CPU test)
FAMILY_CODE = lref.FAMILY_CODE
WEIGHT_VALUES = (0.0, 0.5, 1.0, 2.5)
LAM = 1.0                             # the prior precision of the cases' weighted density

# The bar of elpd, lpd, khat and ess on the GPU, relative to max(1, |value|): 1000 times the float64 noise floor of this restatement.
# NOISE_FLOOR is the largest gap between its float64 and longdouble runs over every case of CASES (both fed the same float64
# l_si, logr and lw; NO row left out: the two precisions agree on every verdict), measured by
# tests/test_psis_loo_shared_cpu.py::test_float64_noise_floor_of_the_restatement_on_the_gpu_inputs: 1.42e-14, at ess; khat 5.1e-15,
# elpd 1.3e-15, lpd 4.3e-16, over the 130 valid rows (122 x info 0, 8 x info -2; 100 rows are not valid).  (l_si itself: 1.6e-15
# between the two precisions.)
NOISE_FLOOR = 1.5e-14
BAR = 1000 * NOISE_FLOOR
LOGLIK_BAR = lref.LOGLIK_BAR

CASES = lref.CASES
case_id = lref.case_id
loo_tile = lref.loo_tile
lse = lref.lse
rel_gap = lref.rel_gap


def valid_mask(weights, K, N):
    """(K, N) bool: v > 0 (False for 0 and NaN); every row for None"""
    if weights is None:
        return np.ones((K, N), dtype=bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(weights, dtype=np.float64) > 0.0


def loglik(family, A, y, offset, weights, tau, X, dtype=LD):
    """l_si as (K, N, S) of ``dtype``: psis_loo_ref.loglik on the replicated design, with y and the offset of the rows that are not
    valid never looked at (they are replaced by 0 before the link and their rows are NaN)"""
    A, y = np.asarray(A, dtype=np.float64), np.asarray(y, dtype=np.float64)
    K, N = y.shape
    ok = valid_mask(weights, K, N)
    y0 = np.where(ok, y, 0.0)
    o0 = None if offset is None else np.where(ok, np.asarray(offset, dtype=np.float64), 0.0)
    out = lref.loglik(family, sref.replicate(A, K), y0, o0, None, tau, X, dtype)
    out[~ok] = dtype(np.nan)
    return out


def loo_rows(ell, logr, lw, v, dtype=LD):
    """one problem: ell (N, S) float64 l_si, logr and lw (S,), v (N,) weights or None -> dict of elpd, lpd, khat, ess (N,) of
    ``dtype`` and info (N,)"""
    ell, logr, lw = (np.asarray(a, dtype=np.float64) for a in (ell, logr, lw))
    N = ell.shape[0]
    nan = dtype(np.nan)
    out = {name: np.full(N, nan, dtype=dtype) for name in ("elpd", "lpd", "khat", "ess")}
    out["info"] = np.full(N, -3, dtype=np.int64)
    ok = valid_mask(None if v is None else np.asarray(v)[None], 1, N)[0]
    for i in np.flatnonzero(ok):
        with np.errstate(all="ignore"):
            rho = logr - ell[i] if v is None else logr - np.float64(v[i]) * ell[i]      # float64, as on the device
        r = pref.psis_weights(rho, dtype)
        out["info"][i] = r["info"]
        if r["info"] == -1:
            continue
        out["khat"][i], out["ess"][i] = r["khat"], r["ess"]
        out["elpd"][i] = lse(np.asarray(r["lw"], dtype=dtype) + ell[i].astype(dtype), dtype)
        out["lpd"][i] = lse(lw.astype(dtype) + ell[i].astype(dtype), dtype)
    return out


def loo_batched(ell, logr, lw, weights=None, dtype=LD):
    """K problems: ell (K, N, S), logr and lw (K, S), weights (K, N) or None -> dict of (K, N) arrays"""
    ell = np.asarray(ell, dtype=np.float64)
    K = ell.shape[0]
    rs = [loo_rows(ell[k], logr[k], lw[k], None if weights is None else np.asarray(weights)[k], dtype) for k in range(K)]
    return {name: np.stack([r[name] for r in rs]) for name in ("elpd", "lpd", "khat", "ess", "info")}


def summaries(r, weights, S):
    """the per-problem fields of LOOBatchedResult from the pointwise ones, in float64, weighted"""
    e, lp, kh = (np.asarray(r[n], dtype=np.float64) for n in ("elpd", "lpd", "khat"))
    info = np.asarray(r["info"])
    K, N = e.shape
    mask = valid_mask(weights, K, N)
    v = np.ones((K, N)) if weights is None else np.asarray(weights, dtype=np.float64)
    nk = mask.sum(1)
    thr = pref.threshold(S)
    with np.errstate(all="ignore"):
        c = v * e
        elpd_loo = np.where(mask, c, 0.0).sum(1)
        p_loo = np.where(mask, v * (lp - e), 0.0).sum(1)
        dev = np.where(mask, c - (elpd_loo / nk)[:, None], 0.0)
        se = np.where(nk >= 2, np.sqrt(nk * ((dev * dev).sum(1) / (nk - 1.0))), np.nan)
        n_bad = (mask & ((info != 0) | (kh >= thr))).sum(1)
    return dict(elpd_loo=elpd_loo, p_loo=p_loo, se=se, n_bad=n_bad)


# ---- the inputs of the GPU tests (tests/test_gpu_psis_loo_shared.py) and of the noise-floor measurement ---------------------------
@functools.lru_cache(maxsize=None)
def make_case(case):
    """The inputs of one case of psis_loo_ref.CASES on ONE design (computed once and shared: do not modify): A = A[0] of
    psis_loo_ref.make_case(case), its y, offset, tau, draws X and (mean, cov).  K = 1: weights None.  K = 3: weights drawn from
    WEIGHT_VALUES, problem 0 all zero, weights[1, 0] = 2.5, and (N >= 3) row 0 of problem 2 valid with a row of weight 0 behind it,
    so that the valid rows are no prefix; NaN in y and +inf in the offset at every weight-0 row of problems 1 and 2 and at every
    other row of problem 0.  logr and lw from the WEIGHTED shared density (lam = LAM) by psis_batched_ref."""
    b = lref.make_case(case)
    family, K, N, D, S = b["family"], b["K"], b["N"], b["D"], b["S"]
    A = np.ascontiguousarray(b["A"][0])
    y = b["y"].copy()
    offset = None if b["offset"] is None else b["offset"].copy()
    weights = None
    if K == 3:
        rs = np.random.default_rng([7, D, S, N, FAMILY_CODE[family]])
        weights = rs.choice(np.array(WEIGHT_VALUES), size=(K, N))
        weights[0] = 0.0
        weights[1, 0] = 2.5
        if N >= 3:
            weights[2, 0], weights[2, 1], weights[2, N - 1] = 1.0, 0.0, 0.5
        dead = weights == 0.0
        dead[0, 1::2] = False
        y[dead] = np.nan
        if offset is not None:
            offset[dead] = np.inf
    X, mean, cov = b["X"], b["mean"], b["cov"]
    _, lp = sref.score_and_lp(family, A, y, offset, weights, LAM, b["tau"], X)
    logr, lw = np.empty((K, S)), np.empty((K, S))
    for k in range(K):
        lr, info = pref.log_ratios(mean[k], cov[k], X[k], lp[k], np.float64)
        assert info == 0
        logr[k] = lr
        lw[k] = np.asarray(pref.psis_weights(logr[k], np.float64)["lw"], dtype=np.float64)
    return dict(family=family, K=K, N=N, D=D, S=S, A=A, y=y, offset=offset, weights=weights, tau=b["tau"], mean=mean, cov=cov, X=X,
                logr=logr, lw=lw)


# ---- the weighted conjugate Gaussian model: the closed-form leave-row-out density ---------------------------------------------------
# The Monte-Carlo gap of elpd_i against the closed-form density of ONE unit observation at row i under the posterior without row
# i's whole weighted term, q the exact weighted posterior, S = 4096, lam = tau = 1, weights from WEIGHT_VALUES, seeds 0 .. 4 (float64
# run of this restatement): the largest |elpd_i - closed form| over the valid rows and seeds at each (N, D), and the bound of the
# test, twice that for the draw-to-draw spread (as psis_loo_ref.GAUSS_BOUND).  Removing a row of weight 2.5 moves the posterior
# further than removing a unit row, so the gaps are larger than psis_loo_ref.GAUSS_GAP's (the largest pointwise khat of these runs:
# 0.99, 0.85).
GAUSS_SHAPES = ((20, 3), (40, 5))
GAUSS_SEEDS = (0, 1, 2, 3, 4)
GAUSS_S = 4096
GAUSS_GAP = {(20, 3): 0.0882, (40, 5): 0.1808}
GAUSS_BOUND = {k: 2.0 * v for k, v in GAUSS_GAP.items()}


def gaussian_exact_problem(N, D, seed, lam=1.0, tau=1.0):
    """psis_loo_ref.gaussian_exact_problem's A and y with weights from WEIGHT_VALUES (at least two of each value) and the exact
    WEIGHTED posterior: precision lam I + tau A^T diag(v) A"""
    rs = np.random.default_rng([seed, N, D, 1])
    A = rs.standard_normal((N, D)) / np.sqrt(D)
    y = A @ rs.standard_normal(D) + rs.standard_normal(N) / np.sqrt(tau)
    v = rs.permutation(np.resize(np.array(WEIGHT_VALUES), N))
    P = lam * np.eye(D) + tau * (A.T * v) @ A
    cov = np.linalg.inv(P)
    cov = 0.5 * (cov + cov.T)
    return dict(A=A, y=y, v=v, lam=lam, tau=tau, mean=cov @ (tau * A.T @ (v * y)), cov=cov, P=P, rs=rs)


def gaussian_exact_loo(p):
    """log N(y_i | a_i . m_-i, 1 / tau + a_i^T Sigma_-i a_i) with (m_-i, Sigma_-i) the posterior without the WHOLE weighted term of
    row i, for the rows with v_i > 0 (NaN elsewhere): the density of one unit observation"""
    A, y, v, tau = p["A"], p["y"], p["v"], p["tau"]
    out = np.full(A.shape[0], np.nan)
    b = tau * A.T @ (v * y)
    for i in np.flatnonzero(v > 0):
        Si = np.linalg.inv(p["P"] - tau * v[i] * np.outer(A[i], A[i]))
        mi = Si @ (b - tau * v[i] * A[i] * y[i])
        var = 1.0 / tau + A[i] @ Si @ A[i]
        out[i] = -0.5 * np.log(2 * np.pi * var) - 0.5 * (y[i] - A[i] @ mi) ** 2 / var
    return out


def gaussian_restatement_run(p, S, dtype=np.float64):
    """the restatement on S draws of the exact weighted posterior: (loo dict of (N,) arrays, problem-level khat)"""
    A, y, v = p["A"], p["y"], p["v"]
    X = p["mean"][None, :] + p["rs"].standard_normal((S, A.shape[1])) @ np.linalg.cholesky(p["cov"]).T
    _, lp = sref.score_and_lp("gaussian", A, y[None], None, v[None], p["lam"], p["tau"], X[None])
    logr, info = pref.log_ratios(p["mean"], p["cov"], X, lp[0], np.float64)
    assert info == 0
    top = pref.psis_weights(np.asarray(logr, dtype=np.float64), dtype)
    ell = loglik("gaussian", A, y[None], None, v[None], p["tau"], X[None], np.float64)[0]
    r = loo_rows(ell, np.asarray(logr, dtype=np.float64), np.asarray(top["lw"], dtype=np.float64), v, dtype)
    return r, float(top["khat"])


# ---- the stand-in engine of the host-logic tests -----------------------------------------------------------------------------------
class StandInEngine(lref.StandInEngine):
    """psis_loo_ref's stand-in engine with what SharedDesignGLMTarget asks of an engine (shared_glm_ref's restatement) and the
    shared-design leave-one-out launch restated (this file, float64 out).  ``calls`` records the launches as tuples."""
    name = "oracle-batched-loo-shared(test-only)"

    def glm_shared_batched(self, X, A, y, family, offset=None, weights=None, prior_prec=1.0, noise_prec=1.0, out=None,
                           lp_out=None, want="g"):
        self._rec(("glm_shared", family, want))
        G, lp = sref.score_and_lp(family, A, y, offset, weights, prior_prec, noise_prec, X)
        return G if want == "g" else lp if want == "lp" else (G, lp)

    def psis_loo_shared_batched(self, X, logr, lw, A, y, family, offset=None, weights=None, noise_prec=1.0, pointwise_loglik=False):
        self._rec(("loo_shared", family, tuple(X.shape), tuple(A.shape), offset is not None, weights is not None,
                   bool(pointwise_loglik)))
        ell = np.asarray(loglik(family, A, y, offset, weights, noise_prec, X), dtype=np.float64)
        r = loo_batched(ell, np.asarray(logr), np.asarray(lw), weights)
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
    name = "gsmvi_psis_loo_shared_batched_f64"
    names = dict(A=at(0), y=at(1), offset=at(2), weights=at(3), tau_dev=None, X=at(4), logr=at(5), lw=at(6), loglik=at(7),
                 elpd=at(8), lpd=at(9), khat=at(10), ess=at(11), info=at(12))

    def call(family=1, K=2, N=5, D=4, S=8, tau=1.0, **kw):
        a = dict(names, **kw)
        return lib.gsmvi_psis_loo_shared_batched_f64(None, None, family, K, N, D, S, a["A"], a["y"], a["offset"], a["weights"], tau,
                                                     a["tau_dev"], a["X"], a["logr"], a["lw"], a["loglik"], a["elpd"], a["lpd"],
                                                     a["khat"], a["ess"], a["info"])

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
        for arr in ("A", "y", "offset", "weights", "X", "logr", "lw"):
            assert call(**{w: names[arr]}) == 1 and f"{w} overlaps {arr}" in err(), (w, arr)
    assert call(lpd=names["elpd"]) == 1 and "lpd overlaps elpd" in err()
    assert call(info=names["ess"] + 4) == 1 and "info overlaps ess" in err()
    assert call(khat=names["loglik"] + 8 * (2 * 5 * 8 - 1)) == 1 and "khat overlaps loglik" in err()     # the last element
    assert call(khat=names["loglik"] + 8 * 2 * 5 * 8) == 1 and "ctx is NULL" in err()                    # adjacent is not overlapping
    # A is ONE (N, D) matrix: N D doubles, not K N D
    assert call(elpd=names["A"] + 8 * (5 * 4 - 1)) == 1 and "elpd overlaps A" in err()
    assert call(elpd=names["A"] + 8 * 5 * 4) == 1 and "ctx is NULL" in err()
    assert call(family=3, tau_dev=at(13), ess=at(13)) == 1 and "ess overlaps noise_prec_dev" in err()
    for fam in (0, 1, 2, 3):
        assert call(family=fam) == 1 and "ctx is NULL" in err(), fam
        assert call(family=fam, offset=None, weights=None, loglik=None) == 1 and "ctx is NULL" in err(), fam
    assert call(family=3, tau=2.5) == 1 and "ctx is NULL" in err()
    assert call(S=5) == 1 and "ctx is NULL" in err()
    assert call(S=16, D=8) == 1 and "ctx is NULL" in err()
    assert call(y=names["A"], offset=names["A"], weights=names["A"], X=names["A"], logr=names["A"], lw=names["A"]) == 1 \
        and "ctx is NULL" in err()
