"""Numpy restatement of the batched softmax PSIS leave-one-out (gsmvi_psis_loo_softmax_batched_f64,
csrc/gsmvi_psis_loo_softmax_batched.hip) in np.longdouble (``dtype=np.float64`` measures the float64 noise floor of the same
arithmetic), the generator of its test inputs, the leave-one-out density by quadrature that it is pinned to, and a stand-in engine
for the host logic of ``psis_loo_softmax_batched``.  Test-only.  Written from the definition in include/gsmvi_hip.h: for problem
k, draws x_s of q_k (class-major: x_s[c P + j] = W_cj) and a valid row i < n_k

    eta_sic = a_i . x_s[c P .. c P + P - 1]  (c < C - 1),   eta_si,C-1 = 0
    m_si    = max_c eta_sic,   z_si = sum_{c = 0 .. C-1} exp(eta_sic - m_si)   (class order, the reference class last)
    l_si    = eta_si,y_i - m_si - log z_si

with z = 1 + rest and log z = log1p(rest) in the kernels' forms (softmax_batched_ref's ``s_minus_one`` and ``log_s``).

NaN where a dot product is not finite, where x_s has a non-finite entry, and where y_i is outside 0 .. C - 1 (compared, never an
index).  From there the text is the GLM leave-one-out's, so the stage and the log-sum-exps are psis_loo_ref's ``loo_batched`` and
``summaries`` on the l_si block: there is no second copy."""
import ctypes as C_
import functools

import numpy as np

import psis_batched_ref as pref
import psis_loo_ref as lref
import softmax_batched_ref as sref
from psis_loo_ref import LD, N_OF, loo_batched, loo_rows, rel_gap, summaries, valid_rows      # noqa: F401

PATH_BITS = 0x400000 | 0x1000000            # GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_SOFTMAX: the pair names the launch
NI_CAP = 4
LDS_MAX_DOUBLES = 160 * 1024 // 8

# The bar of elpd, lpd, khat and ess on the GPU, relative to max(1, |value|): 1000 times the float64 noise floor of the restatement.
# NOISE_FLOOR is the largest gap between its float64 and longdouble runs over every case of CASES (both fed the same float64 l_si,
# logr and lw), measured by tests/test_psis_loo_softmax_cpu.py::test_float64_noise_floor_of_the_restatement_on_the_gpu_inputs:
# 1.05e-14, at ess; khat 6.3e-15, elpd 1.4e-15, lpd 3.7e-16; no row of the 126 changes its verdict between the two precisions
# (every case at seed 0 of SEEDS).  (l_si itself: 5.0e-16 between the two precisions.)
NOISE_FLOOR = 1.1e-14
BAR = 1000 * NOISE_FLOOR
LOGLIK_BAR = 1e-11                  # the project's single-launch bar, for l_si against the longdouble restatement

# The Monte-Carlo gap of elpd_i against the leave-one-out density by 2-D quadrature of the posterior without row i: C = 3, P = 1
# (D = 2), N = 12, lam = 1, q the Laplace Gaussian, S = 4096, seeds 0 .. 4 (float64 run of the restatement): the largest
# |elpd_i - quadrature| over the rows and seeds, and the bound of the test, twice that for the draw-to-draw spread.  (The largest
# pointwise khat of these runs: 0.79; the problem-level khat at most 0.55: at N = 12 the Laplace Gaussian is not the posterior.)
QUAD_SHAPE = dict(C=3, P=1, N=12, lam=1.0)
QUAD_SEEDS = (0, 1, 2, 3, 4)
QUAD_S = 4096
QUAD_GAP = 0.0561
QUAD_BOUND = 2.0 * QUAD_GAP


def loo_tile(C, P, S):
    """NI of gsmvi_psis_loo_softmax_tile(C, P, S) from the header's formula"""
    if not (C >= 2 and P >= 1 and (C - 1) * P <= 64 and 5 <= S <= 4096):
        return 0
    S2 = 8
    while S2 < S:
        S2 *= 2
    stage = S2 + S + 508 + S2 // 2
    tiles = 64 * (((C - 1) * P) | 1) + 16 * (4 * ((P + 3) // 4) + 1) + 16
    return min(NI_CAP, (LDS_MAX_DOUBLES - max(stage, tiles)) // S)


def loglik_softmax(A, labels, C, counts, X, dtype=LD):
    """l_si as (K, N, S) of ``dtype``; NaN for rows i >= n_k and by the three rules of the definition"""
    A, X = np.asarray(A, dtype=np.float64), np.asarray(X, dtype=np.float64)
    y = np.asarray(labels).astype(np.int64)
    K, N, P = A.shape
    S, D = X.shape[1], X.shape[2]
    assert D == (C - 1) * P
    nk = valid_rows(counts, K, N)
    out = np.full((K, N, S), np.nan, dtype=dtype)
    for k in range(K):
        n = int(nk[k])
        if n == 0:
            continue
        W = X[k].astype(dtype).reshape(S, C - 1, P)
        with np.errstate(all="ignore"):
            dots = np.einsum("np,scp->nsc", A[k, :n].astype(dtype), W)                  # (n, S, C - 1)
            eta = np.concatenate([dots, np.zeros((n, S, 1), dtype=dtype)], axis=2)
            m = eta.max(axis=2)
            rest = sref.s_minus_one(np.exp(eta - m[:, :, None]))                         # class order; the reference class last
            etay = np.zeros((n, S), dtype=dtype)
            for c in range(C):                                                          # a label is compared, never an index
                etay = np.where((y[k, :n] == c)[:, None], eta[:, :, c], etay)
            ell = etay - m - sref.log_s(rest, 1 + rest)                                 # log z, z = 1 + rest
        bad = ~np.isfinite(dots).all(axis=2) | ~np.isfinite(X[k]).all(axis=1)[None, :]
        bad |= ((y[k, :n] < 0) | (y[k, :n] > C - 1))[:, None]
        out[k, :n] = np.where(bad, dtype(np.nan), ell)
    return out


# ---- the inputs of the GPU tests (tests/test_gpu_psis_loo_softmax.py) and of the noise-floor measurement ---------------------------
# (C, P, S, N as a function of NI = loo_tile(C, P, S), K).  K = 3 runs with counts = (0, a partial value, N), K = 1 without counts.
CASES = (
    (2, 1, 5, "1", 1),              # the smallest of everything
    (3, 3, 33, "NI-1", 3),
    (3, 5, 257, "2NI+3", 3),        # P % 4 = 1, a partial last draw tile
    (4, 7, 33, "NI", 3),            # P % 4 = 3
    (5, 4, 64, "NI+1", 3),          # exactly one draw tile
    (9, 8, 65, "NI+1", 1),
    (2, 64, 33, "NI+1", 1),         # D = 64, one class
    (33, 2, 33, "2NI+3", 3),        # D = 64, P % 4 = 2: the last class's k-step would read past D
    (65, 1, 33, "NI+1", 1),         # D = 64, the most classes
    (17, 4, 4096, "NI+1", 1),       # NI below the cap
    (3, 5, 1024, "NI+1", 1),
)
# the seed of each case's generator: 0 unless a row's verdict differed between float64 and longdouble there (none did)
SEEDS = {}


def case_id(c):
    return f"C{c[0]}-P{c[1]}-S{c[2]}-N{c[3]}-K{c[4]}"


def draw_labels(rs, A, W):
    """labels (K, N) int32 drawn from the model at W (K, C - 1, P)"""
    K, N, _ = A.shape
    eta = np.concatenate([np.einsum("knp,kcp->knc", A, W), np.zeros((K, N, 1))], axis=2)
    p = np.exp(eta - eta.max(axis=2, keepdims=True))
    cdf = np.cumsum(p / p.sum(axis=2, keepdims=True), axis=2)
    return np.minimum((rs.uniform(size=(K, N, 1)) > cdf).sum(axis=2), eta.shape[2] - 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def make_case(case):
    """The inputs of one case (computed once and shared: do not modify): the model (A, y, counts), S draws X of a Gaussian q_k near
    the posterior, and the problem-level logr and lw of psis_batched_ref on the softmax lp (unit prior), all float64."""
    Cc, P, S, nspec, K = case
    D = (Cc - 1) * P
    N = N_OF[nspec](loo_tile(Cc, P, S))
    rs = np.random.default_rng([Cc, P, S, N, K, SEEDS.get(case, 0)])
    A = rs.standard_normal((K, N, P)) / np.sqrt(P)
    W = 0.7 * rs.standard_normal((K, Cc - 1, P))
    y = draw_labels(rs, A, W)
    counts = np.array([0, max(1, N // 2), N], dtype=np.int32) if K == 3 else None
    theta = W.reshape(K, D)
    mean = 0.8 * theta + 0.1 * rs.standard_normal((K, D))
    G = rs.standard_normal((K, D, D)) / np.sqrt(D)
    AtA = np.swapaxes(A, 1, 2) @ A
    H = np.stack([np.kron(np.eye(Cc - 1), AtA[k]) for k in range(K)])
    cov = np.linalg.inv(np.eye(D)[None] + 0.25 * H + 0.1 * G @ np.swapaxes(G, 1, 2))
    cov = 0.5 * (cov + np.swapaxes(cov, 1, 2))
    X = mean[:, None, :] + np.einsum("ksj,kij->ksi", rs.standard_normal((K, S, D)), np.linalg.cholesky(cov))
    _, lp = sref.score_and_lp(A, y, Cc, counts, 1.0, X)
    logr, lw = np.empty((K, S)), np.empty((K, S))
    for k in range(K):
        lr, info = pref.log_ratios(mean[k], cov[k], X[k], lp[k], np.float64)
        assert info == 0
        logr[k] = lr
        lw[k] = np.asarray(pref.psis_weights(logr[k], np.float64)["lw"], dtype=np.float64)
    return dict(C=Cc, P=P, K=K, N=N, D=D, S=S, A=A, y=y, counts=counts, mean=mean, cov=cov, X=X, logr=logr, lw=lw)


# ---- the statistical check with an exact answer: D = 2, the posterior without row i by grid quadrature ---------------------------
def quad_problem(seed, C=3, P=1, N=12, lam=1.0):
    """A (N, P), labels from the model at W* ~ N(0, I), and the Laplace Gaussian (mode by Newton rounds, inverse Hessian)"""
    rs = np.random.default_rng([seed, C, P, N])
    A = rs.standard_normal((1, N, P))
    y = draw_labels(rs, A, rs.standard_normal((1, C - 1, P)))
    D = (C - 1) * P
    x = np.zeros(D)
    for _ in range(50):
        eta = np.concatenate([A[0] @ x.reshape(C - 1, P).T, np.zeros((N, 1))], axis=1)
        p = np.exp(eta - eta.max(1, keepdims=True))
        p = (p / p.sum(1, keepdims=True))[:, :C - 1]
        hot = (y[0][:, None] == np.arange(C - 1)[None, :]).astype(np.float64)
        g = np.einsum("nc,np->cp", hot - p, A[0]).reshape(D) - lam * x
        Wt = np.einsum("nc,cd->ncd", p, np.eye(C - 1)) - np.einsum("nc,nd->ncd", p, p)
        H = np.einsum("ncd,np,nq->cpdq", Wt, A[0], A[0]).reshape(D, D) + lam * np.eye(D)
        step = np.linalg.solve(H, g)
        x = x + step
        if np.abs(step).max() < 1e-14:
            break
    cov = np.linalg.inv(H)
    return dict(A=A, y=y, C=C, P=P, lam=lam, mean=x, cov=0.5 * (cov + cov.T), rs=rs)


def quad_exact_loo(p, half=9.0, n=361):
    """log of  int p(y_i | x) exp(lp_-i(x)) dx / int exp(lp_-i(x)) dx  for every row i, on an n x n grid of [-half, half]^2 (the
    integrands are smooth and below e^-30 of their peak at the edge: the sum is exact to rounding; n = 721 moves it by < 1e-14)"""
    assert (p["C"] - 1) * p["P"] == 2
    t = np.linspace(-half, half, n)
    X = np.stack(np.meshgrid(t, t, indexing="ij"), axis=-1).reshape(1, n * n, 2)
    ell = np.asarray(loglik_softmax(p["A"], p["y"], p["C"], None, X, np.float64), dtype=np.float64)[0]     # (N, n n)
    total = ell.sum(0) - 0.5 * p["lam"] * (X[0] * X[0]).sum(1)
    out = np.empty(ell.shape[0])
    for i in range(ell.shape[0]):
        rest = total - ell[i]
        out[i] = float(lref.lse(rest + ell[i], np.float64) - lref.lse(rest, np.float64))
    return out


def quad_restatement_run(p, S, dtype=np.float64):
    """the restatement on S draws of the problem's Laplace Gaussian: (loo dict of (N,) arrays, problem-level khat)"""
    A, y, Cc = p["A"], p["y"], p["C"]
    X = p["mean"][None, :] + p["rs"].standard_normal((S, p["mean"].shape[0])) @ np.linalg.cholesky(p["cov"]).T
    _, lp = sref.score_and_lp(A, y, Cc, None, p["lam"], X[None])
    logr, info = pref.log_ratios(p["mean"], p["cov"], X, lp[0], np.float64)
    assert info == 0
    top = pref.psis_weights(np.asarray(logr, dtype=np.float64), dtype)
    ell = np.asarray(loglik_softmax(A, y, Cc, None, X[None], np.float64), dtype=np.float64)[0]
    r = loo_rows(ell, np.asarray(logr, dtype=np.float64), np.asarray(top["lw"], dtype=np.float64), A.shape[1], dtype)
    return r, float(top["khat"])


# ---- the stand-in engine of the host-logic tests -----------------------------------------------------------------------------------
class StandInEngine(lref.StandInEngine):
    """psis_loo_ref's stand-in engine with what BatchedSoftmaxTarget asks of an engine (softmax_batched_ref's restatement) and the
    softmax leave-one-out launch restated (this file, float64 out).  ``calls`` records the launches as tuples."""
    name = "oracle-batched-loo-softmax(test-only)"

    def batched_labels(self, values):
        return np.ascontiguousarray(values, dtype=np.int32)

    def softmax_batched(self, X, A, labels, num_classes, counts=None, prior_prec=1.0, out=None, lp_out=None, want="g"):
        self._rec(("softmax", num_classes, want))
        G, lp = sref.score_and_lp(A, labels, num_classes, counts, prior_prec, X)
        return G if want == "g" else lp if want == "lp" else (G, lp)

    def psis_loo_softmax_batched(self, X, logr, lw, A, labels, num_classes, counts=None, pointwise_loglik=False):
        self._rec(("loo_softmax", num_classes, tuple(X.shape), tuple(A.shape), counts is not None, bool(pointwise_loglik)))
        ell = np.asarray(loglik_softmax(A, labels, num_classes, counts, X), dtype=np.float64)
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
    name = "gsmvi_psis_loo_softmax_batched_f64"
    names = dict(A=at(0), labels=at(1), counts=at(3), X=at(4), logr=at(5), lw=at(6), loglik=at(7), elpd=at(8), lpd=at(9),
                 khat=at(10), ess=at(11), info=at(12))

    def call(K=2, C=3, P=2, N=5, S=8, **kw):
        a = dict(names, **kw)
        return lib.gsmvi_psis_loo_softmax_batched_f64(None, None, K, C, P, N, S, a["A"], a["labels"], a["counts"], a["X"], a["logr"],
                                                      a["lw"], a["loglik"], a["elpd"], a["lpd"], a["khat"], a["ess"], a["info"])

    assert call(C=1) == 1 and "C must be" in err() and name in err()
    assert call(C=0) == 1 and "C must be" in err()
    assert call(P=0) == 1 and "P must be" in err()
    assert call(C=66, P=1) == 1 and "D = (C - 1) P" in err()                      # (C - 1) P = 65
    assert call(C=6, P=13) == 1 and "D = (C - 1) P" in err()                      # 65 again
    assert call(C=2, P=65) == 1 and "D = (C - 1) P" in err()
    assert call(C=2 ** 17, P=2 ** 17) == 1 and "D = (C - 1) P" in err()           # the product would overflow an int
    assert call(K=0) == 1 and "K must be" in err()
    assert call(N=0) == 1 and "N must be" in err()
    assert call(S=4) == 1 and "S must be" in err()
    assert call(S=4097) == 1 and "S must be" in err()
    assert call(K=2 ** 20, N=2 ** 40) == 1 and "too large" in err()
    assert call(K=2 ** 20, N=2 ** 30, S=4096) == 1 and "too large" in err()
    assert call(K=2 ** 22, N=64) == 1 and "2^24 - 1" in err()                      # K ceil(N / NI) tiles
    ni = loo_tile(3, 2, 8)
    assert call(K=2 ** 12, N=ni * 2 ** 12) == 1 and "2^24 - 1" in err()            # 2^24 tiles: one too many
    far = {n: (j + 1) << 40 for j, n in enumerate(names)}                          # (never dereferenced: far enough apart not to overlap)
    assert call(K=2 ** 12 - 1, N=ni * 2 ** 12, **far) == 1 and "ctx is NULL" in err()     # (2^12 - 1) 2^12 tiles fit
    assert call(K=2 ** 12 - 1, N=ni * 2 ** 12 + ni, **far) == 1 and "ctx is NULL" in err()  # 2^24 - 1 tiles exactly
    assert call(K=2 ** 12 - 1, N=ni * 2 ** 12 + ni + 1, **far) == 1 and "2^24 - 1" in err()
    assert call(K=2 ** 25) == 1 and ("2^24 - 1" in err() or "K must be" in err())
    for arr in ("A", "labels", "X", "logr", "lw", "elpd", "lpd", "khat", "ess", "info"):
        assert call(**{arr: None}) == 1 and "NULL array" in err(), arr
    for w in ("loglik", "elpd", "lpd", "khat", "ess", "info"):
        for arr, key in (("A", "A"), ("labels", "labels"), ("counts_dev", "counts"), ("X", "X"), ("logr", "logr"), ("lw", "lw")):
            assert call(**{w: names[key]}) == 1 and f"{w} overlaps {arr}" in err(), (w, arr)
    assert call(lpd=names["elpd"]) == 1 and "lpd overlaps elpd" in err()
    assert call(info=names["ess"] + 4) == 1 and "info overlaps ess" in err()
    assert call(khat=names["loglik"] + 8 * (2 * 5 * 8 - 1)) == 1 and "khat overlaps loglik" in err()     # the last element
    assert call(khat=names["loglik"] + 8 * 2 * 5 * 8) == 1 and "ctx is NULL" in err()                    # adjacent is not overlapping
    assert call() == 1 and "ctx is NULL" in err()
    assert call(counts=None, loglik=None) == 1 and "ctx is NULL" in err()
    assert call(S=5) == 1 and "ctx is NULL" in err()
    assert call(C=65, P=1, S=16) == 1 and "ctx is NULL" in err()
    assert call(C=2, P=64, S=16) == 1 and "ctx is NULL" in err()
    assert call(labels=names["A"], X=names["A"], logr=names["A"], lw=names["A"]) == 1 and "ctx is NULL" in err()
