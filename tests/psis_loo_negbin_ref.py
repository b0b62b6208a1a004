"""Numpy restatement of the batched negative binomial PSIS leave-one-out (gsmvi_psis_loo_negbin_batched_f64,
csrc/gsmvi_psis_loo_negbin_batched.hip) in np.longdouble (``dtype=np.float64`` measures the float64 noise floor of the same
arithmetic), the generator of its test inputs, the leave-one-out density by quadrature that it is pinned to, and a stand-in engine
for the host logic of ``psis_loo_negbin_batched``.  Test-only.  Written from the definition in include/gsmvi_hip.h: for problem k,
draws x_s = (beta_s, theta_s) of q_k and a valid row i < n_k

    eta_si = a_i . beta_s + o_i
    l_si   = t(eta_si, theta_s, y_i) - lgamma(y_i + 1)

with t of negbin_batched_ref (``link_ld`` in longdouble, ``link`` -- the kernel's forms -- in float64).  NaN for a draw with a
non-finite entry, theta included, or whose e^theta is not a positive normal number.  From there the text is the GLM
leave-one-out's, so the stage and the log-sum-exps are psis_loo_ref's ``loo_batched`` and ``summaries`` on the l_si block: there is
no second copy."""
import ctypes as C_
import functools

import numpy as np
from scipy import special

import negbin_batched_ref as nref
import psis_batched_ref as pref
import psis_loo_ref as lref
from psis_loo_ref import LD, N_OF, loo_batched, loo_rows, rel_gap, summaries, valid_rows      # noqa: F401

PATH_BITS = 0x400000 | 0x20000              # GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_TARGET: the pair names the launch
NI_CAP = 4
LDS_MAX_DOUBLES = 160 * 1024 // 8

# The bar of elpd, lpd, khat and ess on the GPU, relative to max(1, |value|): 1000 times the float64 noise floor of the restatement.
# NOISE_FLOOR is the largest gap between its float64 and longdouble runs over every case of CASES (both fed the same float64 l_si,
# logr and lw), measured by tests/test_psis_loo_negbin_cpu.py::test_float64_noise_floor_of_the_restatement_on_the_gpu_inputs:
# 2.77e-14, at ess (the S = 4096 case); khat 5.5e-15, elpd 2.7e-15, lpd 3.4e-16; none of the 109 valid rows changes its verdict
# between the two precisions (every case at seed 0 of SEEDS).  (l_si itself: 2.7e-15 between the two precisions.)
NOISE_FLOOR = 2.8e-14
BAR = 1000 * NOISE_FLOOR
LOGLIK_BAR = 1e-11                  # the project's single-launch bar, for l_si against the longdouble restatement

# The Monte-Carlo gap of elpd_i against the leave-one-out density by 2-D quadrature of the posterior without row i: P = 1 (D = 2:
# beta and theta), N = 12, proper priors (lam = 1; theta ~ N(1.5, 1)), q the Laplace Gaussian, S = 4096, seeds 0 .. 4 (float64 run
# of the restatement): the largest |elpd_i - quadrature| over the rows and seeds, and the bound of the test, twice that for the
# draw-to-draw spread.  (Per seed 0.015, 0.012, 0.032, 0.204, 0.021: seed 3 holds a count of 17 among counts of 0 .. 2, whose
# leave-one-out ratios have the largest pointwise khat of these runs, 0.87; the problem-level khat is at most 0.66.)
QUAD_SHAPE = dict(N=12, lam=1.0, tm=1.5, tk=1.0)
QUAD_SEEDS = (0, 1, 2, 3, 4)
QUAD_S = 4096
QUAD_GAP = 0.2039
QUAD_BOUND = 2.0 * QUAD_GAP


def loo_tile(P, S):
    """NI of gsmvi_psis_loo_negbin_tile(P, S) from the header's formula"""
    if not (1 <= P <= 63 and 5 <= S <= 4096):
        return 0
    S2 = 8
    while S2 < S:
        S2 *= 2
    stage = S2 + S + 508 + S2 // 2
    tiles = 80 * (4 * ((P + 3) // 4) + 1) + 240
    return min(NI_CAP, (LDS_MAX_DOUBLES - max(stage, tiles)) // S)


def draw_flag(Xk):
    """the kernel's draw flag of the rows of Xk (S, D): a non-finite entry, or e^theta not a positive normal number"""
    Xk = np.asarray(Xk, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.exp(Xk[:, -1])
    return ~np.isfinite(Xk).all(axis=1) | ~((r >= nref.R_MIN) & (r < np.inf))


def loglik_negbin(A, y, offset, counts, X, dtype=LD):
    """l_si as (K, N, S) of ``dtype``; NaN for rows i >= n_k and for flagged draws"""
    A, y, X = (np.asarray(a, dtype=np.float64) for a in (A, y, X))
    K, N, P = A.shape
    S, D = X.shape[1], X.shape[2]
    assert D == P + 1
    fn = nref.link_ld if dtype is LD else nref.link
    nk = valid_rows(counts, K, N)
    out = np.full((K, N, S), np.nan, dtype=dtype)
    for k in range(K):
        n = int(nk[k])
        if n == 0:
            continue
        with np.errstate(all="ignore"):
            eta = A[k, :n].astype(dtype) @ X[k, :, :P].astype(dtype).T                    # (n, S)
            if offset is not None:
                eta = eta + np.asarray(offset, dtype=np.float64)[k, :n, None].astype(dtype)
            t = fn(eta, X[k, None, :, P].astype(dtype), y[k, :n, None].astype(dtype))[2]
            ell = np.asarray(t, dtype=dtype) - special.gammaln(y[k, :n, None] + 1.0).astype(dtype)
        out[k, :n] = np.where(draw_flag(X[k])[None, :], dtype(np.nan), ell)
    return out


# ---- the inputs of the GPU tests (tests/test_gpu_psis_loo_negbin.py) and of the noise-floor measurement -----------------------------
# (P, with offset, S, N as a function of NI = loo_tile(P, S), K): every value of each axis at least once, the N edges at P = 9 and
# P = 63.  K = 3 runs with counts = (0, a partial value, N), K = 1 without counts.
CASES = (
    (1, False, 5, "1", 1),              # the smallest of everything
    (3, True, 33, "NI-1", 3),           # P % 4 = 3
    (4, False, 257, "NI", 3),           # P % 4 = 0, a partial last draw tile
    (15, True, 257, "2NI+3", 3),
    (16, False, 33, "NI+1", 1),
    (17, True, 257, "NI+1", 3),         # P % 4 = 1
) + tuple((9, bool(j % 2), 33, n, 3) for j, n in enumerate(N_OF)) \
  + tuple((63, bool(j % 2), 33, n, 1 + 2 * (j % 2)) for j, n in enumerate(N_OF)) + (
    (9, True, 1024, "NI+1", 1),
    (63, False, 4096, "NI+1", 1),       # NI below the cap
)
# the seed of each case's generator: 0 unless the draws of seed 0 lay on one side of the r = 10 branch of the link, or a valid
# row's verdict differed between float64 and longdouble there
SEEDS = {}


def case_id(c):
    return f"P{c[0]}-{'off' if c[1] else 'nooff'}-S{c[2]}-N{c[3]}-K{c[4]}"


def draw_counts(rs, A, offset, beta, size):
    """y (K, N) negative binomial at mu = exp(A beta + offset) (capped at e^10) with size (K,): a gamma mixture of Poissons"""
    eta = np.einsum("knp,kp->kn", A, beta) + (offset if offset is not None else 0.0)
    mu = np.exp(np.minimum(eta, 10.0))
    return rs.poisson(rs.gamma(size[:, None], mu / size[:, None])).astype(np.float64)


THETA_PRIOR = (1.5, 1.0)            # the prior N(mean, 1 / precision) of theta in make_case's lp


@functools.lru_cache(maxsize=None)
def make_case(case):
    """The inputs of one case (computed once and shared: do not modify): the model (A, y, offset, counts), S draws X of a Gaussian
    q_k near the posterior in beta whose theta is spread over about [-1, 4] (mean 1.5, standard deviation 1.25: both sides of the
    r = 10 branch of the link, theta = 2.30, occur in every case -- asserted), and the problem-level logr and lw of
    psis_batched_ref on the negative binomial lp (unit prior of beta, THETA_PRIOR), all float64."""
    P, with_offset, S, nspec, K = case
    D = P + 1
    N = N_OF[nspec](loo_tile(P, S))
    rs = np.random.default_rng([P, S, N, K, SEEDS.get(case, 0)])
    A = rs.standard_normal((K, N, P)) / np.sqrt(P)
    offset = 0.3 * rs.standard_normal((K, N)) if with_offset else None
    beta = 0.7 * rs.standard_normal((K, P))
    size = np.exp(rs.uniform(0.0, 3.0, K))
    y = draw_counts(rs, A, offset, beta, size)
    counts = np.array([0, max(1, N // 2), N], dtype=np.int32) if K == 3 else None
    mean = np.concatenate([0.8 * beta + 0.1 * rs.standard_normal((K, P)), np.full((K, 1), 1.5)], axis=1)
    G = rs.standard_normal((K, D, D)) / np.sqrt(D)
    H = np.zeros((K, D, D))
    H[:, :P, :P] = np.swapaxes(A, 1, 2) @ A
    cov = np.linalg.inv(np.eye(D)[None] + 0.25 * H + 0.1 * G @ np.swapaxes(G, 1, 2))
    sc = np.ones((K, D))
    sc[:, P] = 1.25 / np.sqrt(cov[:, P, P])                                   # the spread of theta
    cov = sc[:, :, None] * cov * sc[:, None, :]
    cov = 0.5 * (cov + np.swapaxes(cov, 1, 2))
    X = mean[:, None, :] + np.einsum("ksj,kij->ksi", rs.standard_normal((K, S, D)), np.linalg.cholesky(cov))
    r = np.exp(X[:, :, P])
    assert (r < nref.SHIFT_BELOW).any() and (r >= nref.SHIFT_BELOW).any(), case    # both branches of the link
    _, lp = nref.score_and_lp(A, y, offset, counts, 1.0, THETA_PRIOR[0], THETA_PRIOR[1], X)
    logr, lw = np.empty((K, S)), np.empty((K, S))
    for k in range(K):
        lr, info = pref.log_ratios(mean[k], cov[k], X[k], lp[k], np.float64)
        assert info == 0
        logr[k] = lr
        lw[k] = np.asarray(pref.psis_weights(logr[k], np.float64)["lw"], dtype=np.float64)
    return dict(P=P, K=K, N=N, D=D, S=S, A=A, y=y, offset=offset, counts=counts, mean=mean, cov=cov, X=X, logr=logr, lw=lw)


# ---- the statistical check with an exact answer: D = 2, the posterior without row i by grid quadrature ---------------------------
def quad_lp(p, X):
    """(ell (N, rows), log prior (rows,)) of the problem at the rows of X (rows, 2), float64"""
    ell = np.asarray(loglik_negbin(p["A"], p["y"], None, None, X[None], np.float64), dtype=np.float64)[0]
    prior = -0.5 * p["lam"] * X[:, 0] ** 2 - 0.5 * p["tk"] * (X[:, 1] - p["tm"]) ** 2
    return ell, prior


def quad_problem(seed, N=12, lam=1.0, tm=1.5, tk=1.0):
    """P = 1: A (1, N, 1), counts from the model at beta* ~ N(0, 1), log r* ~ U(0, 3), and the Laplace Gaussian in (beta, theta)
    (mode by Newton rounds on the restatement's score with a finite-difference Hessian, inverse Hessian)"""
    rs = np.random.default_rng([seed, N, 77])
    A = rs.standard_normal((1, N, 1))
    beta = rs.standard_normal((1, 1))
    y = draw_counts(rs, A, None, beta, np.exp(rs.uniform(0.0, 3.0, 1)))
    score = lambda x: nref.score_and_lp(A, y, None, None, lam, tm, tk, x[None, None, :])[0][0, 0]      # noqa: E731
    x, h = np.array([0.0, tm]), 1e-5
    for _ in range(100):
        g = score(x)
        H = -np.stack([(score(x + h * e) - score(x - h * e)) / (2 * h) for e in np.eye(2)])
        H = 0.5 * (H + H.T)
        step = np.linalg.solve(H, g)
        x = x + step
        if np.abs(step).max() < 1e-10:
            break
    cov = np.linalg.inv(H)
    return dict(A=A, y=y, lam=lam, tm=tm, tk=tk, mean=x, cov=0.5 * (cov + cov.T), rs=rs)


def quad_exact_loo(p, half=8.0, n=321):
    """log of  int p(y_i | x) exp(lp_-i(x)) dx / int exp(lp_-i(x)) dx  for every row i, on an n x n grid of [-half, half] x
    [tm - half, tm + half] in (beta, theta): eight prior standard deviations each way, where the priors alone are e^-32 of their
    peak (the integrands are smooth: n = 641 moves the result by less than 3e-15)"""
    t = np.linspace(-half, half, n)
    X = np.stack(np.meshgrid(t, p["tm"] + t, indexing="ij"), axis=-1).reshape(n * n, 2)
    ell, prior = quad_lp(p, X)
    total = ell.sum(0) + prior
    out = np.empty(ell.shape[0])
    for i in range(ell.shape[0]):
        rest = total - ell[i]
        out[i] = float(lref.lse(rest + ell[i], np.float64) - lref.lse(rest, np.float64))
    return out


def quad_restatement_run(p, S, dtype=np.float64):
    """the restatement on S draws of the problem's Laplace Gaussian: (loo dict of (N,) arrays, problem-level khat)"""
    A, y = p["A"], p["y"]
    X = p["mean"][None, :] + p["rs"].standard_normal((S, 2)) @ np.linalg.cholesky(p["cov"]).T
    _, lp = nref.score_and_lp(A, y, None, None, p["lam"], p["tm"], p["tk"], X[None])
    logr, info = pref.log_ratios(p["mean"], p["cov"], X, lp[0], np.float64)
    assert info == 0
    top = pref.psis_weights(np.asarray(logr, dtype=np.float64), dtype)
    ell = np.asarray(loglik_negbin(A, y, None, None, X[None], np.float64), dtype=np.float64)[0]
    r = loo_rows(ell, np.asarray(logr, dtype=np.float64), np.asarray(top["lw"], dtype=np.float64), A.shape[1], dtype)
    return r, float(top["khat"])


# ---- the stand-in engine of the host-logic tests -----------------------------------------------------------------------------------
class StandInEngine(lref.StandInEngine):
    """psis_loo_ref's stand-in engine with what BatchedNegBinomialTarget asks of an engine (negbin_batched_ref's restatement) and
    the negative binomial leave-one-out launch restated (this file, float64 out).  ``calls`` records the launches as tuples."""
    name = "oracle-batched-loo-negbin(test-only)"

    def negbin_batched(self, X, A, y, offset=None, counts=None, prior_prec=1.0, log_size_mean=0.0, log_size_prec=1.0, out=None,
                       lp_out=None, want="g"):
        self._rec(("negbin", want))
        G, lp = nref.score_and_lp(A, y, offset, counts, prior_prec, log_size_mean, log_size_prec, X)
        return G if want == "g" else lp if want == "lp" else (G, lp)

    def psis_loo_negbin_batched(self, X, logr, lw, A, y, offset=None, counts=None, pointwise_loglik=False):
        self._rec(("loo_negbin", tuple(X.shape), tuple(A.shape), offset is not None, counts is not None, bool(pointwise_loglik)))
        ell = np.asarray(loglik_negbin(A, y, offset, counts, X), dtype=np.float64)
        r = loo_batched(ell, np.asarray(logr), np.asarray(lw), counts)
        f = lambda n: np.asarray(r[n], dtype=np.float64)                         # noqa: E731
        return f("elpd"), f("lpd"), f("khat"), f("ess"), r["info"], (ell if pointwise_loglik else None)


# ---- the C ABI's argument checks (NULL context) ------------------------------------------------------------------------------------
def check_bad_arguments(lib):
    """the entry point through the C ABI with a NULL context: every bad argument returns GSMVI_ERR_BAD_ARG (1) with its own
    message, so nothing can have been enqueued; valid calls end at the context"""
    err = lambda: (lib.gsmvi_last_error() or b"").decode()          # noqa: E731
    buf = (C_.c_double * 32768)()
    p = C_.cast(buf, C_.c_void_p).value
    at = lambda i: p + 8 * 1024 * i                                   # noqa: E731  (slots of 8 KB: K = 2, N = 5, D = 4, S = 8 fit)
    name = "gsmvi_psis_loo_negbin_batched_f64"
    names = dict(A=at(0), y=at(1), offset=at(2), counts=at(3), X=at(4), logr=at(5), lw=at(6), loglik=at(7), elpd=at(8), lpd=at(9),
                 khat=at(10), ess=at(11), info=at(12))

    def call(K=2, P=3, N=5, S=8, **kw):
        a = dict(names, **kw)
        return lib.gsmvi_psis_loo_negbin_batched_f64(None, None, K, P, N, S, a["A"], a["y"], a["offset"], a["counts"], a["X"],
                                                     a["logr"], a["lw"], a["loglik"], a["elpd"], a["lpd"], a["khat"], a["ess"],
                                                     a["info"])

    assert call(P=0) == 1 and "P must be" in err() and name in err()
    assert call(P=64) == 1 and "P must be" in err()                               # D = 65
    assert call(P=-1) == 1 and "P must be" in err()
    assert call(K=0) == 1 and "K must be" in err()
    assert call(N=0) == 1 and "N must be" in err()
    assert call(S=4) == 1 and "S must be" in err()
    assert call(S=4097) == 1 and "S must be" in err()
    assert call(K=2 ** 20, N=2 ** 40) == 1 and "too large" in err()
    assert call(K=2 ** 20, N=2 ** 30, S=4096) == 1 and "too large" in err()
    assert call(K=2 ** 22, N=64) == 1 and "2^24 - 1" in err()                      # K ceil(N / NI) tiles
    ni = loo_tile(3, 8)
    assert call(K=2 ** 12, N=ni * 2 ** 12) == 1 and "2^24 - 1" in err()            # 2^24 tiles: one too many
    far = {n: (j + 1) << 40 for j, n in enumerate(names)}                          # (never dereferenced: far enough apart not to overlap)
    assert call(K=2 ** 12 - 1, N=ni * 2 ** 12, **far) == 1 and "ctx is NULL" in err()     # (2^12 - 1) 2^12 tiles fit
    assert call(K=2 ** 12 - 1, N=ni * 2 ** 12 + ni, **far) == 1 and "ctx is NULL" in err()  # 2^24 - 1 tiles exactly
    assert call(K=2 ** 12 - 1, N=ni * 2 ** 12 + ni + 1, **far) == 1 and "2^24 - 1" in err()
    assert call(K=2 ** 25) == 1 and ("2^24 - 1" in err() or "K must be" in err())
    for arr in ("A", "y", "X", "logr", "lw", "elpd", "lpd", "khat", "ess", "info"):
        assert call(**{arr: None}) == 1 and "NULL array" in err(), arr
    for w in ("loglik", "elpd", "lpd", "khat", "ess", "info"):
        for arr, key in (("A", "A"), ("y", "y"), ("offset", "offset"), ("counts_dev", "counts"), ("X", "X"), ("logr", "logr"),
                         ("lw", "lw")):
            assert call(**{w: names[key]}) == 1 and f"{w} overlaps {arr}" in err(), (w, arr)
    assert call(lpd=names["elpd"]) == 1 and "lpd overlaps elpd" in err()
    assert call(info=names["ess"] + 4) == 1 and "info overlaps ess" in err()
    assert call(khat=names["loglik"] + 8 * (2 * 5 * 8 - 1)) == 1 and "khat overlaps loglik" in err()     # the last element
    assert call(khat=names["loglik"] + 8 * 2 * 5 * 8) == 1 and "ctx is NULL" in err()                    # adjacent is not overlapping
    assert call() == 1 and "ctx is NULL" in err()
    assert call(offset=None, counts=None, loglik=None) == 1 and "ctx is NULL" in err()
    assert call(S=5) == 1 and "ctx is NULL" in err()
    assert call(P=63, S=16, N=1, K=1) == 1 and "ctx is NULL" in err()
    assert call(P=1, S=16) == 1 and "ctx is NULL" in err()
    assert call(y=names["A"], offset=names["A"], X=names["A"], logr=names["A"], lw=names["A"]) == 1 and "ctx is NULL" in err()
