"""Numpy restatement of the batched ordinal PSIS leave-one-out (gsmvi_psis_loo_ordinal_batched_f64,
csrc/gsmvi_psis_loo_ordinal_batched.hip) in np.longdouble (``dtype=np.float64`` measures the float64 noise floor of the same
arithmetic), the generator of its test inputs, the leave-one-out density by quadrature that it is pinned to, and a stand-in engine
for the host logic of ``psis_loo_ordinal_batched``.  Test-only.  Written from the definition in include/gsmvi_hip.h: for problem k,
draws x_s = (beta_s, delta_s) of q_k and a valid row i < n_k

    cut_s0 = delta_s0,   cut_sj = cut_s,j-1 + exp(delta_sj)
    eta_si = a_i . beta_s + o_i
    l_si   = t(eta_si, cut_s, exp(delta_s), y_i) = log P(y_i | eta_si, cut_s)

with t of ordinal_batched_ref (``cutpoints``, ``gap`` and ``link``, in longdouble or float64: there is no second copy of the
link).  NaN for a draw with a non-finite entry, or in which some exp(delta_j), j >= 1, is not a positive normal number.  From there
the text is the GLM leave-one-out's, so the stage and the log-sum-exps are psis_loo_ref's ``loo_batched`` and ``summaries`` on the
l_si block."""
import ctypes as C_
import functools

import numpy as np

import ordinal_batched_ref as oref
import psis_batched_ref as pref
import psis_loo_ref as lref
from psis_loo_ref import LD, N_OF, loo_batched, loo_rows, rel_gap, summaries, valid_rows      # noqa: F401

PATH_BITS = 0x400000 | 0x20000              # GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_TARGET
NI_CAP = 4
LDS_MAX_DOUBLES = 160 * 1024 // 8
LOG2 = oref.LOG2

# The bar of elpd, lpd, khat and ess on the GPU, relative to max(1, |value|): 1000 times the float64 noise floor of the restatement.
# NOISE_FLOOR is the largest gap between its float64 and longdouble runs over every case of CASES (both fed the same float64 l_si,
# logr and lw), measured by tests/test_psis_loo_ordinal_cpu.py::test_float64_noise_floor_of_the_restatement_on_the_gpu_inputs:
# 1.68e-14, at ess (the S = 4096 case); khat 9.3e-15, elpd 3.6e-15, lpd 3.5e-16; none of the 143 valid rows changes its verdict
# between the two precisions at the seeds of SEEDS.  (l_si itself: 7.9e-16 between the two precisions.)
NOISE_FLOOR = 1.7e-14
BAR = 1000 * NOISE_FLOOR
LOGLIK_BAR = 1e-11                  # the project's single-launch bar, for l_si against the longdouble restatement

# The Monte-Carlo gap of elpd_i against the leave-one-out density by 3-D quadrature of the posterior without row i: P = 1, C = 3
# (D = 3: beta, delta_0, delta_1), N = 12, unit priors, q the Laplace Gaussian, S = 4096, seeds 0 .. 4 (float64 run of the
# restatement): the largest |elpd_i - quadrature| over the rows and seeds, and the bound of the test, twice that for the
# draw-to-draw spread.  (Per seed 0.016, 0.037, 0.020, 0.032, 0.012; the largest pointwise khat of these runs is 0.79, the
# problem-level khat at most 0.55.)
QUAD_SHAPE = dict(N=12, lam=1.0, kap=1.0)
QUAD_SEEDS = (0, 1, 2, 3, 4)
QUAD_S = 4096
QUAD_GAP = 0.0370
QUAD_BOUND = 2.0 * QUAD_GAP


def tiles_doubles(P, C):
    """the kernel's own use of the shared region: the X and A tiles (80 rows of 4 ceil(P / 4) + 1), one table of e^delta, then of
    the cutpoints, of 64 draws (rows of (C - 1) | 1), 16 offsets, 16 labels (8 doubles), 64 flags and one cell per thread"""
    return 80 * (4 * ((P + 3) // 4) + 1) + 64 * ((C - 1) | 1) + 344


def loo_tile(P, C, S):
    """NI of gsmvi_psis_loo_ordinal_tile(P, C, S) from the header's formula"""
    if not (2 <= C <= 64 and 1 <= P <= 65 - C and 5 <= S <= 4096):
        return 0
    S2 = 8
    while S2 < S:
        S2 *= 2
    stage = S2 + S + 508 + S2 // 2
    return min(NI_CAP, (LDS_MAX_DOUBLES - max(stage, tiles_doubles(P, C))) // S)


def draw_flag(Xk, P):
    """the kernel's draw flag of the rows of Xk (S, D): a non-finite entry, or some e^{delta_j}, j >= 1, not a positive normal
    number"""
    Xk = np.asarray(Xk, dtype=np.float64)
    with np.errstate(all="ignore"):
        w = np.exp(Xk[:, P + 1:])
    return ~np.isfinite(Xk).all(axis=1) | ~((w >= oref.W_MIN) & (w < np.inf)).all(axis=1)


def loglik_ordinal(A, y, offset, counts, X, C, dtype=LD):
    """l_si as (K, N, S) of ``dtype``; NaN for rows i >= n_k and for flagged draws"""
    A, X = (np.asarray(a, dtype=np.float64) for a in (A, X))
    y = np.asarray(y)
    K, N, P = A.shape
    S, D = X.shape[1], X.shape[2]
    assert D == P + C - 1
    nk = valid_rows(counts, K, N)
    out = np.full((K, N, S), np.nan, dtype=dtype)
    for k in range(K):
        n = int(nk[k])
        if n == 0:
            continue
        yk = np.clip(y[k, :n].astype(np.int64), 0, C - 1)                        # (the kernel clamps a label as it stages it)
        with np.errstate(all="ignore"):
            eta = X[k, :, :P].astype(dtype) @ A[k, :n].astype(dtype).T               # (S, n)
            if offset is not None:
                eta = eta + np.asarray(offset, dtype=np.float64)[k, None, :n].astype(dtype)
            cut, w = oref.cutpoints(X[k, :, P:], dtype)
            lm, qe = oref.gap(w)
            t = oref.link(eta, yk, cut, lm, qe)[3]                                   # (S, n)
        out[k, :n] = np.where(draw_flag(X[k], P)[None, :], dtype(np.nan), np.asarray(t, dtype=dtype).T)
    return out


# ---- the inputs of the GPU tests (tests/test_gpu_psis_loo_ordinal.py) and of the noise-floor measurement ----------------------------
# (P, C, with offset, S, N as a function of NI = loo_tile(P, C, S), K): every value of each axis at least once, the N edges at
# (P, C) = (9, 3) and (1, 64).  K = 3 runs with counts = (0, a partial value, N), K = 1 without counts.
CASES = (
    (1, 2, False, 5, "1", 1),               # the smallest of everything: no interior class
    (3, 3, True, 33, "NI-1", 3),            # P % 4 = 3, one interior class
    (4, 5, False, 257, "NI", 3),            # P % 4 = 0, a partial last draw tile
    (9, 16, True, 257, "2NI+3", 3),
    (17, 2, True, 257, "NI+1", 3),          # P % 4 = 1; C = 2 against the logistic launch
    (3, 2, False, 33, "NI+1", 3),           # P % 4 = 3 at C = 2: delta_0 right behind beta, where the padded positions would read
    (6, 5, True, 33, "2NI+3", 3),           # P % 4 = 2; the rows that sum to the score launch
    (60, 5, True, 33, "2NI+3", 3),          # D = 64 with P large
) + tuple((9, 3, bool(j % 2), 33, n, 3) for j, n in enumerate(N_OF)) \
  + tuple((1, 64, bool(j % 2), 33, n, 1 + 2 * (j % 2)) for j, n in enumerate(N_OF)) + (
    (9, 5, True, 1024, "NI+1", 1),
    (1, 64, False, 4096, "NI+1", 1),        # NI below the cap
)
# the seed of each case's generator: 0 unless the labels of seed 0 missed a class that make_case asks for (0, C - 1 and an interior
# one among the valid rows of every problem with at least three), the draws of seed 0 lay on one side of the w = log 2 branch of
# ord_gap, or a valid row's verdict differed between float64 and longdouble there
SEEDS = {(3, 3, True, 33, "NI-1", 3): 1, (4, 5, False, 257, "NI", 3): 2, (9, 16, True, 257, "2NI+3", 3): 2,
         (6, 5, True, 33, "2NI+3", 3): 1, (60, 5, True, 33, "2NI+3", 3): 2, (9, 3, True, 33, "NI+1", 3): 1,
         (1, 64, True, 33, "NI+1", 3): 3, (1, 64, False, 4096, "NI+1", 1): 13}


def case_id(c):
    return f"P{c[0]}-C{c[1]}-{'off' if c[2] else 'nooff'}-S{c[3]}-N{c[4]}-K{c[5]}"


def planted_cutpoints(C):
    """the cutpoints the labels are drawn at: C - 1 of them evenly over [-1.2, 1.2] (C = 2: 0), so that the first and the last
    class each hold about a quarter of the rows whatever C is"""
    return np.zeros(1) if C == 2 else np.linspace(-1.2, 1.2, C - 1)


def draw_labels(rs, A, offset, beta, C):
    """y (K, N) int32 from the cumulative-logit model at the planted cutpoints"""
    eta = np.einsum("knp,kp->kn", A, beta) + (offset if offset is not None else 0.0)
    cdf = 1.0 / (1.0 + np.exp(-(planted_cutpoints(C)[None, None, :] - eta[:, :, None])))      # P(y <= j)
    return (rs.uniform(size=eta.shape)[:, :, None] > cdf).sum(2).astype(np.int32)


def case_model(case, seed):
    """(rs, N, A, offset, beta, y, counts) of a case at a seed: the part of make_case that the labels depend on"""
    P, C, with_offset, S, nspec, K = case
    N = N_OF[nspec](loo_tile(P, C, S))
    rs = np.random.default_rng([P, C, S, N, K, seed])
    A = rs.standard_normal((K, N, P)) / np.sqrt(P)
    offset = 0.3 * rs.standard_normal((K, N)) if with_offset else None
    beta = 0.7 * rs.standard_normal((K, P))
    y = draw_labels(rs, A, offset, beta, C)
    counts = np.array([0, max(1, N // 2), N], dtype=np.int32) if K == 3 else None
    return rs, N, A, offset, beta, y, counts


def labels_cover(y, counts, C):
    """every problem with at least three valid rows holds a label 0, a label C - 1 and, for C >= 3, an interior one among them"""
    K, N = y.shape
    for k, n in enumerate(valid_rows(counts, K, N)):
        v = y[k, :int(n)]
        if n >= 3 and not ((v == 0).any() and (v == C - 1).any() and (C == 2 or ((v > 0) & (v < C - 1)).any())):
            return False
    return True


@functools.lru_cache(maxsize=None)
def make_case(case):
    """The inputs of one case (computed once and shared: do not modify): the model (A, y, offset, counts) with labels drawn from
    it, S draws X of a Gaussian q_k near the posterior in beta and delta_0 whose delta_j, j >= 1, are spread about log log 2 with
    standard deviation 0.6 (w = e^{delta_j} on both sides of log 2, the branch of ord_gap, occurs in every case with C >= 3 --
    asserted), and the problem-level logr and lw of psis_batched_ref on the ordinal lp (unit priors), all float64."""
    P, C, with_offset, S, nspec, K = case
    D = P + C - 1
    rs, N, A, offset, beta, y, counts = case_model(case, SEEDS.get(case, 0))
    assert labels_cover(y, counts, C), case
    mean = np.concatenate([0.8 * beta + 0.1 * rs.standard_normal((K, P)),
                           planted_cutpoints(C)[0] + 0.1 * rs.standard_normal((K, 1)),
                           np.full((K, C - 2), np.log(LOG2))], axis=1)
    G = rs.standard_normal((K, D, D)) / np.sqrt(D)
    H = np.zeros((K, D, D))
    H[:, :P, :P] = np.swapaxes(A, 1, 2) @ A
    cov = np.linalg.inv(np.eye(D)[None] + 0.25 * H + 0.1 * G @ np.swapaxes(G, 1, 2))
    sc = np.ones((K, D))
    sc[:, P + 1:] = 0.6 / np.sqrt(np.diagonal(cov, axis1=1, axis2=2)[:, P + 1:])       # the spread of delta_j, j >= 1
    cov = sc[:, :, None] * cov * sc[:, None, :]
    cov = 0.5 * (cov + np.swapaxes(cov, 1, 2))
    X = mean[:, None, :] + np.einsum("ksj,kij->ksi", rs.standard_normal((K, S, D)), np.linalg.cholesky(cov))
    if C >= 3:
        w = np.exp(X[:, :, P + 1:])
        assert (w < LOG2).any() and (w >= LOG2).any(), case                           # both branches of ord_gap
    _, lp = oref.score_and_lp(A, y, offset, counts, 1.0, 1.0, X, C)
    logr, lw = np.empty((K, S)), np.empty((K, S))
    for k in range(K):
        lr, info = pref.log_ratios(mean[k], cov[k], X[k], lp[k], np.float64)
        assert info == 0
        logr[k] = lr
        lw[k] = np.asarray(pref.psis_weights(logr[k], np.float64)["lw"], dtype=np.float64)
    return dict(P=P, C=C, K=K, N=N, D=D, S=S, A=A, y=y, offset=offset, counts=counts, mean=mean, cov=cov, X=X, logr=logr, lw=lw)


# ---- the statistical check with an exact answer: D = 3, the posterior without row i by grid quadrature ---------------------------
def quad_lp(p, X):
    """(ell (N, rows), log prior (rows,)) of the problem at the rows of X (rows, 3), float64"""
    ell = np.asarray(loglik_ordinal(p["A"], p["y"], None, None, X[None], 3, np.float64), dtype=np.float64)[0]
    prior = -0.5 * p["lam"] * X[:, 0] ** 2 - 0.5 * p["kap"] * (X[:, 1] ** 2 + X[:, 2] ** 2)
    return ell, prior


def quad_problem(seed, N=12, lam=1.0, kap=1.0):
    """P = 1, C = 3: A (1, N, 1), labels from the model at beta* ~ N(0, 1) and the planted cutpoints, and the Laplace Gaussian in
    (beta, delta_0, delta_1) (mode by Newton rounds on the restatement's score with a finite-difference Hessian, inverse Hessian)"""
    rs = np.random.default_rng([seed, N, 79])
    A = rs.standard_normal((1, N, 1))
    y = draw_labels(rs, A, None, rs.standard_normal((1, 1)), 3)
    score = lambda x: oref.score_and_lp(A, y, None, None, lam, kap, x[None, None, :], 3)[0][0, 0]      # noqa: E731
    x, h = np.zeros(3), 1e-5
    for _ in range(100):
        g = score(x)
        H = -np.stack([(score(x + h * e) - score(x - h * e)) / (2 * h) for e in np.eye(3)])
        H = 0.5 * (H + H.T)
        step = np.linalg.solve(H, g)
        x = x + step
        if np.abs(step).max() < 1e-10:
            break
    cov = np.linalg.inv(H)
    return dict(A=A, y=y, lam=lam, kap=kap, mean=x, cov=0.5 * (cov + cov.T), rs=rs)


def quad_exact_loo(p, half=6.0, n=65):
    """log of  int p(y_i | x) exp(lp_-i(x)) dx / int exp(lp_-i(x)) dx  for every row i, on an n x n x n grid of [-half, half]^3 in
    (beta, delta_0, delta_1): six prior standard deviations each way, where the priors alone are e^-18 of their peak (the
    integrands are smooth: n = 97 moves the result by 2.2e-11, and n = 129 on [-8, 8]^3 by 4e-11)"""
    t = np.linspace(-half, half, n)
    X = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(n ** 3, 3)
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
    X = p["mean"][None, :] + p["rs"].standard_normal((S, 3)) @ np.linalg.cholesky(p["cov"]).T
    _, lp = oref.score_and_lp(A, y, None, None, p["lam"], p["kap"], X[None], 3)
    logr, info = pref.log_ratios(p["mean"], p["cov"], X, lp[0], np.float64)
    assert info == 0
    top = pref.psis_weights(np.asarray(logr, dtype=np.float64), dtype)
    ell = np.asarray(loglik_ordinal(A, y, None, None, X[None], 3, np.float64), dtype=np.float64)[0]
    r = loo_rows(ell, np.asarray(logr, dtype=np.float64), np.asarray(top["lw"], dtype=np.float64), A.shape[1], dtype)
    return r, float(top["khat"])


# ---- the stand-in engine of the host-logic tests -----------------------------------------------------------------------------------
class StandInEngine(lref.StandInEngine):
    """psis_loo_ref's stand-in engine with what BatchedOrdinalTarget asks of an engine (ordinal_batched_ref's restatement) and the
    ordinal leave-one-out launch restated (this file, float64 out).  ``calls`` records the launches as tuples."""
    name = "oracle-batched-loo-ordinal(test-only)"

    def batched_labels(self, values):
        return np.ascontiguousarray(values, dtype=np.int32)

    def ordinal_batched(self, X, A, y, C, offset=None, counts=None, prior_prec=1.0, cut_prec=1.0, out=None, lp_out=None, want="g"):
        self._rec(("ordinal", want))
        G, lp = oref.score_and_lp(A, y, offset, counts, prior_prec, cut_prec, X, C)
        return G if want == "g" else lp if want == "lp" else (G, lp)

    def psis_loo_ordinal_batched(self, X, logr, lw, A, y, C, offset=None, counts=None, pointwise_loglik=False):
        self._rec(("loo_ordinal", tuple(X.shape), tuple(A.shape), int(C), offset is not None, counts is not None,
                   bool(pointwise_loglik)))
        ell = np.asarray(loglik_ordinal(A, y, offset, counts, X, C), dtype=np.float64)
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
    at = lambda i: p + 8 * 1024 * i                                   # noqa: E731  (slots of 8 KB: K = 2, N = 5, D = 5, S = 8 fit)
    name = "gsmvi_psis_loo_ordinal_batched_f64"
    names = dict(A=at(0), y=at(1), offset=at(2), counts=at(3), X=at(4), logr=at(5), lw=at(6), loglik=at(7), elpd=at(8), lpd=at(9),
                 khat=at(10), ess=at(11), info=at(12))

    def call(K=2, P=3, C=3, N=5, S=8, **kw):
        a = dict(names, **kw)
        return lib.gsmvi_psis_loo_ordinal_batched_f64(None, None, K, P, C, N, S, a["A"], a["y"], a["offset"], a["counts"], a["X"],
                                                      a["logr"], a["lw"], a["loglik"], a["elpd"], a["lpd"], a["khat"], a["ess"],
                                                      a["info"])

    for C in (1, 0, -1, 65):
        assert call(C=C) == 1 and "C must be in [2, 64]" in err() and name in err(), C
    assert call(C=1, P=0) == 1 and "C must be" in err()                           # C is looked at first
    for P, C in ((0, 3), (-1, 3), (63, 3), (64, 2), (2, 64), (33, 33)):           # D = 65
        assert call(P=P, C=C) == 1 and "P must be in [1, 65 - C]" in err(), (P, C)
    assert call(K=0) == 1 and "K must be" in err()
    assert call(K=2 ** 24) == 1 and "K must be" in err()
    assert call(N=0) == 1 and "N must be" in err()
    assert call(K=0, N=0, S=0) == 1 and "K must be" in err()                      # K before N before S
    assert call(N=0, S=0) == 1 and "N must be" in err()
    assert call(S=4) == 1 and "S must be" in err()
    assert call(S=4097) == 1 and "S must be" in err()
    assert call(S=4, A=None) == 1 and "S must be" in err()                        # S before the NULL arrays
    assert call(K=2 ** 20, N=2 ** 40) == 1 and "K N S is too large" in err()
    assert call(K=2 ** 20, N=2 ** 37, P=62, S=5) == 1 and "K N P is too large" in err()
    assert call(K=2 ** 22, N=64) == 1 and "2^24 - 1" in err() and "gsmvi_psis_loo_ordinal_tile(P, C, S)" in err()
    ni = loo_tile(3, 3, 8)
    assert call(K=2 ** 12, N=ni * 2 ** 12) == 1 and "2^24 - 1" in err()            # 2^24 tiles: one too many
    far = {n: (j + 1) << 40 for j, n in enumerate(names)}                          # (never dereferenced: far enough apart not to overlap)
    assert call(K=2 ** 12 - 1, N=ni * 2 ** 12, **far) == 1 and "ctx is NULL" in err()     # (2^12 - 1) 2^12 tiles fit
    assert call(K=2 ** 12 - 1, N=ni * 2 ** 12 + ni, **far) == 1 and "ctx is NULL" in err()  # 2^24 - 1 tiles exactly
    assert call(K=2 ** 12 - 1, N=ni * 2 ** 12 + ni + 1, **far) == 1 and "2^24 - 1" in err()
    for arr in ("A", "y", "X", "logr", "lw", "elpd", "lpd", "khat", "ess", "info"):
        assert call(**{arr: None}) == 1 and "NULL array" in err(), arr
    for w in ("loglik", "elpd", "lpd", "khat", "ess", "info"):
        for arr, key in (("A", "A"), ("y", "y"), ("offset", "offset"), ("counts_dev", "counts"), ("X", "X"), ("logr", "logr"),
                         ("lw", "lw")):
            assert call(**{w: names[key]}) == 1 and f"{w} overlaps {arr}" in err(), (w, arr)
    assert call(lpd=names["elpd"]) == 1 and "lpd overlaps elpd" in err()
    assert call(info=names["ess"] + 4) == 1 and "info overlaps ess" in err()
    assert call(elpd=names["y"] + 4 * (2 * 5 - 1)) == 1 and "elpd overlaps y" in err()                   # y is K N ints: its last one
    assert call(elpd=names["y"] + 4 * 2 * 5) == 1 and "ctx is NULL" in err()                             # adjacent is not overlapping
    assert call(khat=names["loglik"] + 8 * (2 * 5 * 8 - 1)) == 1 and "khat overlaps loglik" in err()     # the last element
    assert call(khat=names["loglik"] + 8 * 2 * 5 * 8) == 1 and "ctx is NULL" in err()
    assert call(khat=names["X"] + 8 * (2 * 8 * 5 - 1)) == 1 and "khat overlaps X" in err()               # X is K S (P + C - 1)
    assert call(khat=names["X"] + 8 * 2 * 8 * 5) == 1 and "ctx is NULL" in err()
    assert call() == 1 and "ctx is NULL" in err()
    assert call(offset=None, counts=None, loglik=None) == 1 and "ctx is NULL" in err()
    assert call(S=5) == 1 and "ctx is NULL" in err()
    assert call(P=1, C=64, S=16, N=1, K=1) == 1 and "ctx is NULL" in err()
    assert call(P=63, C=2, S=16, N=1, K=1) == 1 and "ctx is NULL" in err()
    assert call(y=names["A"], offset=names["A"], X=names["A"], logr=names["A"], lw=names["A"]) == 1 and "ctx is NULL" in err()
