"""Numpy restatement of the batched ordinal posterior predictive (gsmvi_ordinal_predict_batched_f64,
csrc/gsmvi_ordinal_predict_batched.hip) in np.longdouble (``dtype=np.float64`` measures the float64 noise floor of the same
arithmetic), the generator of its test inputs, the expectation by tensor Gauss-Hermite quadrature that it is pinned to, and a
stand-in engine for the host logic of ``predict_ordinal_batched``.  Test-only.  Written from the definition in include/gsmvi_hip.h:
for problem k, draws x_s = (beta_s, delta_s) of q_k, normalised log weights lw_s (None: lw_s = -log S, w_s = 1 / S) and a valid row
i < n_k

    cut_s0 = delta_s0,   cut_sj = cut_s,j-1 + w_sj,   w_sj = exp(delta_sj)
    eta_si = a_i . beta_s + o_i,   z_sij = cut_sj - eta_si
    p_si0  = sigma(z_si0),   p_si,C-1 = sigma(-z_si,C-2),   p_sic = sigma(z_sic) sigma(-z_si,c-1) (-expm1(-w_sc))   (0 < c < C - 1)
    prob[k, i, c] = sum_s w_s p_sic,   w_s = exp(lw_s)
    l_si   = t(eta_si, cut_s, w_s, y_i) = log P(y_i | eta_si, cut_s)
    lpd[k, i]     = log sum_s exp(lw_s + l_si)

NaN: every valid row of a problem with a flagged draw (psis_loo_ordinal_ref's ``draw_flag``) or whose lw holds a NaN or +inf, or
only -inf; a row with a draw whose eta is not finite; the lpd of a row whose label is outside 0 .. C - 1; rows i >= n_k.  The
cutpoints are ordinal_batched_ref's ``cutpoints`` and l_si is psis_loo_ordinal_ref's ``loglik_ordinal`` (ordinal_batched_ref's
``gap`` and ``link``): there is no second copy of the link.

The float64 noise floor of this arithmetic, measured by tests/test_ordinal_predict_cpu.py::test_float64_noise_floor_of_the_
restatement (float64 against longdouble over CASES, relative to max(1, |value|)): prob 4.4e-16, lpd 7.0e-16; |sum_c prob - 1| is
at most 8.9e-16 in float64 and 6.0e-16 in longdouble (the weights exp(lw_s) of a float64 lw do not sum to 1 exactly; 2.2e-19 with
uniform weights).  BAR = 1e-11 is more than 10000 times the prob and lpd floors, and the GPU test's 1e-13 on the row sums is more
than 100 times theirs."""
import ctypes as C_
import functools

import numpy as np

import ordinal_batched_ref as oref
import psis_loo_ordinal_ref as lo
import psis_loo_ref as lref
import softmax_predict_ref as spref
from psis_loo_ordinal_ref import draw_flag, loglik_ordinal      # noqa: F401
from psis_loo_ref import LD, lse, valid_rows                      # noqa: F401
from softmax_predict_ref import rel_gap                           # noqa: F401

PATH_BITS = 0x100000 | 0x20000              # GSMVI_PATH_BATCHED_PREDICT | GSMVI_PATH_BATCHED_TARGET
BAR = spref.BAR                             # 1e-11: the project's single-launch bar, relative to max(1, |value|)
ROWSUM_BAR = 1e-13                          # |sum_c prob - 1| on the GPU: the bound of tests/test_gpu_softmax_predict.py
LDS_MAX = 160 * 1024
LOG2 = oref.LOG2

# The Monte-Carlo check: |prob - E_q[p_c]| <= 5 x 0.5 / sqrt(S): a probability lies in [0, 1], so its standard deviation over the
# draws is at most 0.5 and the standard error of the mean of S independent draws at most 0.5 / sqrt(S); five of them.
QUAD_S = 4096
QUAD_SEEDS = (0, 1, 2, 3, 4)
QUAD_BOUND = 5 * 0.5 / np.sqrt(QUAD_S)


def lds_bytes(P, C):
    """gsmvi_ordinal_predict_lds_bytes(P, C) from the header's formula"""
    if not (2 <= C <= 64 and 1 <= P <= 65 - C):
        return 0
    return 8 * (80 * (4 * ((P + 3) // 4) + 1) + 128 * ((C - 1) | 1) + 64 * C + 616)


def class_probs(eta, cut, w):
    """p (S, n, C) from eta (S, n), the draws' cutpoints cut (S, C - 1) and gaps w (S, C - 1; column 0 is not used), in their
    precision: the product form, sigma(z) and sigma(-z) from one exp(-|z|); no two probabilities are subtracted"""
    S, n = eta.shape
    lc = cut.shape[1]
    with np.errstate(all="ignore"):
        z = cut[:, None, :] - eta[:, :, None]
        e = np.exp(-np.abs(z))
        q = 1 + e
        big, small = 1 / q, e / q
        sp, sn = np.where(z >= 0, big, small), np.where(z >= 0, small, big)
        g = -np.expm1(-w)
        p = np.empty((S, n, lc + 1), dtype=eta.dtype)
        p[:, :, 0] = sp[:, :, 0]
        p[:, :, 1:lc] = (sp[:, :, 1:] * sn[:, :, :-1]) * g[:, None, 1:]
        p[:, :, lc] = sn[:, :, lc - 1]
    return p


def predict(A, y, offset, counts, X, lw, C, dtype=LD):
    """(prob (K, M, C), lpd (K, M) or None without labels) of ``dtype``"""
    A, X = np.asarray(A, dtype=np.float64), np.asarray(X, dtype=np.float64)
    K, M, P = A.shape
    S, D = X.shape[1], X.shape[2]
    assert D == P + C - 1
    nk = valid_rows(counts, K, M)
    nan = dtype(np.nan)
    prob = np.full((K, M, C), nan, dtype=dtype)
    lpd = None if y is None else np.full((K, M), nan, dtype=dtype)
    ell = None if y is None else loglik_ordinal(A, y, offset, counts, X, C, dtype)            # (K, M, S); NaN by its rules
    for k in range(K):
        n = int(nk[k])
        if n == 0 or draw_flag(X[k], P).any():
            continue                                                                  # the problem's valid rows stay NaN
        with np.errstate(all="ignore"):
            if lw is None:
                lwk = np.full(S, -np.log(dtype(S)), dtype=dtype)
                w = np.full(S, dtype(1) / dtype(S), dtype=dtype)
            else:
                l64 = np.asarray(lw, dtype=np.float64)[k]
                if np.isnan(l64).any() or (l64 == np.inf).any() or (l64 == -np.inf).all():
                    continue
                lwk = l64.astype(dtype)
                w = np.exp(lwk)
            eta = X[k, :, :P].astype(dtype) @ A[k, :n].astype(dtype).T                # (S, n)
            if offset is not None:
                eta = eta + np.asarray(offset, dtype=np.float64)[k, None, :n].astype(dtype)
            cut, gapw = oref.cutpoints(X[k, :, P:], dtype)
            p = class_probs(eta, cut, gapw)
            pr = np.einsum("s,snc->nc", w, p)
            bad = ~np.isfinite(eta).all(axis=0)                                       # (n,) rows
            prob[k, :n] = np.where(bad[:, None], nan, pr)
            if y is not None:
                yk = np.asarray(y)[k, :n]
                out = lse(lwk[None, :] + ell[k, :n], dtype)
                lpd[k, :n] = np.where(bad | (yk < 0) | (yk > C - 1), nan, out)
    return prob, lpd


# ---- the inputs of the GPU tests (tests/test_gpu_ordinal_predict.py) and of the noise-floor measurement ---------------------------
# (P, C, with offset, S, M, K, weighted).  K = 3 runs with counts = (0, M - 5 clipped to >= 1, M); K = 1 without counts.  weighted:
# lw random normalised log weights, else None (uniform).  S over {5, 63, 64, 65, 257} around the tile of 64 draws, M over
# {1, 15, 16, 17, 33} around the tile of 16 rows.
CASES = (
    (1, 2, False, 5, 1, 1, False),          # the smallest of everything: no interior class
    (3, 3, True, 63, 15, 3, True),          # P % 4 = 3, one interior class
    (5, 4, False, 257, 33, 3, True),        # P % 4 = 1, five draw tiles the last one partial, three row tiles
    (4, 5, True, 64, 16, 3, False),         # exactly one draw tile and one row tile
    (3, 2, False, 65, 17, 1, True),         # C = 2: delta_0 right behind beta, where a padded position would read
    (1, 64, True, 63, 17, 3, True),         # D = 64, the most classes: the largest LDS request (above 64 KB)
    (63, 2, False, 65, 33, 1, False),       # D = 64, the widest P
    (60, 5, True, 64, 17, 1, True),
    (6, 5, True, 5, 33, 3, True),           # P % 4 = 2, one wave at work
)
# the seed of each case's generator: 0 unless the labels of seed 0 missed a class that make_case asks for (0, C - 1 and an interior
# one among the valid rows of every problem with at least three) or the draws of seed 0 lay on one side of the w = log 2 branch of
# ord_gap (the rule of psis_loo_ordinal_ref.SEEDS).  Seed 0 serves every case of CASES as they stand.
SEEDS = {}


def case_id(c):
    return f"P{c[0]}-C{c[1]}-{'off' if c[2] else 'nooff'}-S{c[3]}-M{c[4]}-K{c[5]}-{'w' if c[6] else 'u'}"


def partial_count(M):
    """a count of valid rows that ends inside a tile of 16 rows (1 for M = 1)"""
    return max(1, M - 5)


def case_model(case, seed):
    """(rs, A, offset, beta, y, counts) of a case at a seed: the part of make_case that the labels depend on"""
    P, C, with_offset, S, M, K, weighted = case
    rs = np.random.default_rng([P, C, S, M, K, int(weighted), seed])
    A = rs.standard_normal((K, M, P)) / np.sqrt(P)
    offset = 0.3 * rs.standard_normal((K, M)) if with_offset else None
    beta = 0.7 * rs.standard_normal((K, P))
    y = lo.draw_labels(rs, A, offset, beta, C)
    counts = np.array([0, partial_count(M), M], dtype=np.int32) if K == 3 else None
    return rs, A, offset, beta, y, counts


def draws_cover(X, P, C):
    """w = e^{delta_j}, j >= 1, falls on both sides of log 2, the branch of ord_gap (C >= 3)"""
    w = np.exp(X[:, :, P + 1:])
    return C < 3 or bool((w < LOG2).any() and (w >= LOG2).any())


@functools.lru_cache(maxsize=None)
def make_case(case):
    """The inputs of one case (computed once and shared: do not modify), all float64 / int32: new rows A, labels y drawn from the
    model at the planted cutpoints of psis_loo_ordinal_ref, offset, counts, S draws X of a Gaussian near the model in beta and
    delta_0 whose delta_j, j >= 1, are spread about log log 2 with standard deviation 0.6 (psis_loo_ordinal_ref.make_case's rule:
    w on both sides of the ord_gap branch, asserted for C >= 3), and the log weights lw (or None)"""
    P, C, with_offset, S, M, K, weighted = case
    D = P + C - 1
    rs, A, offset, beta, y, counts = case_model(case, SEEDS.get(case, 0))
    assert lo.labels_cover(y, counts, C), case
    mean = np.concatenate([0.8 * beta + 0.1 * rs.standard_normal((K, P)),
                           lo.planted_cutpoints(C)[0] + 0.1 * rs.standard_normal((K, 1)),
                           np.full((K, C - 2), np.log(LOG2))], axis=1)
    sd = np.concatenate([np.full(P + 1, 0.3), np.full(C - 2, 0.6)])
    X = mean[:, None, :] + sd[None, None, :] * rs.standard_normal((K, S, D))
    assert draws_cover(X, P, C), case
    lw = None
    if weighted:
        raw = 1.5 * rs.standard_normal((K, S))
        lw = raw - np.asarray(lse(raw, np.float64), dtype=np.float64)[:, None]
    return dict(P=P, C=C, K=K, M=M, D=D, S=S, A=A, y=y, offset=offset, counts=counts, X=X, lw=lw)


@functools.lru_cache(maxsize=None)
def expected(case):
    """(prob, lpd) of the longdouble restatement on a case's inputs (computed once and shared: do not modify)"""
    p = make_case(case)
    return predict(p["A"], p["y"], p["offset"], p["counts"], p["X"], p["lw"], p["C"])


# ---- the statistical check with an exact answer: P = 1, C = 3 (D = 3), E_q[p_c] by tensor Gauss-Hermite quadrature ----------------
def quad_problem(seed, M=8):
    """a Gaussian q = N(mean, cov) over (beta, delta_0, delta_1) and M rows a_i (P = 1)"""
    rs = np.random.default_rng([seed, 3, 1, M, 83])
    mean = np.array([rs.standard_normal(), -0.6 + 0.3 * rs.standard_normal(), np.log(1.2) + 0.2 * rs.standard_normal()])
    G = rs.standard_normal((3, 3))
    cov = 0.1 * (G @ G.T) + 0.1 * np.eye(3)
    A = 1.5 * rs.standard_normal((1, M, 1))
    return dict(mean=mean, cov=cov, A=A, rs=rs)


def quad_exact(p, Q=48):
    """E_q[P(y = c | a_i beta, cutpoints)] for every row, (M, 3), by the Q x Q x Q tensor Gauss-Hermite rule (the integrand is
    smooth and bounded; the test compares two orders)"""
    t, w = np.polynomial.hermite.hermgauss(Q)
    L = np.linalg.cholesky(p["cov"])
    T = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3)
    wt = (w[:, None, None] * w[None, :, None] * w[None, None, :]).reshape(-1) / np.pi ** 1.5
    Xq = p["mean"][None, :] + np.sqrt(2.0) * T @ L.T                                      # (Q^3, 3)
    eta = Xq[:, :1] @ p["A"][0].T                                                         # (Q^3, M)
    cut, gapw = oref.cutpoints(Xq[:, 1:], np.float64)
    return np.einsum("s,snc->nc", wt, class_probs(eta, cut, gapw))


def quad_draws(p, S):
    return (p["mean"][None, :] + p["rs"].standard_normal((S, 3)) @ np.linalg.cholesky(p["cov"]).T)[None]


# ---- the stand-in engine of the host-logic tests -----------------------------------------------------------------------------------
class StandInEngine(lo.StandInEngine):
    """psis_loo_ordinal_ref's stand-in engine with the predictive launch restated (this file, float64 out).  ``calls`` records the
    launches as tuples."""
    name = "oracle-batched-ordinal-predict(test-only)"

    def ordinal_predict_batched(self, X, lw, A, C, y=None, offset=None, counts=None):
        self._rec(("predict_ordinal", int(C), tuple(X.shape), tuple(A.shape), lw is not None, y is not None, offset is not None,
                   counts is not None))
        prob, lpd = predict(A, y, offset, counts, X, lw, int(C))
        return np.asarray(prob, dtype=np.float64), None if lpd is None else np.asarray(lpd, dtype=np.float64)


# ---- the C ABI's argument checks (NULL context) ------------------------------------------------------------------------------------
def check_bad_arguments(lib):
    """the entry point through the C ABI with a NULL context: every bad argument returns GSMVI_ERR_BAD_ARG (1) with its own
    message, so nothing can have been enqueued; valid calls end at the context"""
    err = lambda: (lib.gsmvi_last_error() or b"").decode()          # noqa: E731
    buf = (C_.c_double * 16384)()
    p = C_.cast(buf, C_.c_void_p).value
    at = lambda i: p + 8 * 1024 * i                                   # noqa: E731  (slots of 8 KB: K = 2, M = 5, D = 5, S = 8 fit)
    name = "gsmvi_ordinal_predict_batched_f64"
    names = dict(A=at(0), y=at(1), offset=at(2), counts=at(3), X=at(4), lw=at(5), prob=at(6), lpd=at(7))

    def call(K=2, P=3, C=3, M=5, S=8, **kw):
        a = dict(names, **kw)
        return lib.gsmvi_ordinal_predict_batched_f64(None, None, K, P, C, M, S, a["A"], a["y"], a["offset"], a["counts"], a["X"],
                                                     a["lw"], a["prob"], a["lpd"])

    for C in (1, 0, -1, 65):
        assert call(C=C) == 1 and "C must be in [2, 64]" in err() and name in err(), C
    assert call(C=1, P=0) == 1 and "C must be" in err()                           # C is looked at first
    for P, C in ((0, 3), (-1, 3), (63, 3), (64, 2), (2, 64), (33, 33)):           # D = 65
        assert call(P=P, C=C) == 1 and "P must be in [1, 65 - C]" in err(), (P, C)
    assert call(P=0, K=0) == 1 and "P must be" in err()                           # P before K
    assert call(K=0) == 1 and "K must be in [1, 2^24 - 1]" in err()
    assert call(K=2 ** 24) == 1 and "K must be in [1, 2^24 - 1]" in err()
    assert call(M=0) == 1 and "M must be at least 1" in err()
    assert call(K=0, M=0, S=0) == 1 and "K must be" in err()                      # K before M before S
    assert call(M=0, S=0) == 1 and "M must be" in err()
    assert call(S=0) == 1 and "S must be in [1, 4096]" in err()
    assert call(S=4097) == 1 and "S must be in [1, 4096]" in err()
    assert call(S=0, A=None) == 1 and "S must be" in err()                        # S before the NULL arrays
    assert call(K=2 ** 20, M=2 ** 40) == 1 and "K M is too large" in err()
    assert call(K=2 ** 20, M=2 ** 40, A=None) == 1 and "K M is too large" in err()
    assert call(K=2 ** 22, M=64) == 1 and "2^24 - 1" in err() and "ceil(M / 16)" in err()      # 2^24 tiles: one too many
    far = {n: (j + 1) << 44 for j, n in enumerate(names)}                          # (never dereferenced: far enough apart not to overlap)
    assert call(K=2 ** 12 - 1, M=16 * 2 ** 12 + 16, **far) == 1 and "ctx is NULL" in err()    # 2^24 - 1 tiles exactly
    assert call(K=2 ** 12 - 1, M=16 * 2 ** 12 + 17, **far) == 1 and "2^24 - 1" in err()
    for arr in ("A", "X", "prob"):
        assert call(**{arr: None}) == 1 and "NULL array" in err(), arr
    assert call(y=None) == 1 and "labels and lpd are given together or not at all" in err()      # the pairing: both or neither
    assert call(lpd=None) == 1 and "labels and lpd are given together or not at all" in err()
    assert call(y=None, lpd=None) == 1 and "ctx is NULL" in err()
    for w in ("prob", "lpd"):
        for arr, key in (("A", "A"), ("y", "y"), ("offset", "offset"), ("counts_dev", "counts"), ("X", "X"), ("lw", "lw")):
            assert call(**{w: names[key]}) == 1 and f"{w} overlaps {arr}" in err(), (w, arr)
    assert call(lpd=names["prob"]) == 1 and "lpd overlaps prob" in err()
    assert call(lpd=names["prob"] + 8 * (2 * 5 * 3 - 1)) == 1 and "lpd overlaps prob" in err()     # the last element
    assert call(lpd=names["prob"] + 8 * 2 * 5 * 3) == 1 and "ctx is NULL" in err()                 # adjacent is not overlapping
    assert call(prob=names["y"] + 4 * (2 * 5 - 1)) == 1 and "prob overlaps y" in err()             # y is K M ints: its last one
    assert call(prob=names["y"] + 4 * 2 * 5) == 1 and "ctx is NULL" in err()
    assert call(prob=names["X"] + 8 * (2 * 8 * 5 - 1)) == 1 and "prob overlaps X" in err()         # X is K S (P + C - 1)
    assert call(prob=names["X"] + 8 * 2 * 8 * 5) == 1 and "ctx is NULL" in err()
    assert call() == 1 and "ctx is NULL" in err()
    assert call(offset=None, counts=None, lw=None) == 1 and "ctx is NULL" in err()
    assert call(S=1) == 1 and "ctx is NULL" in err()
    assert call(S=4096, **far) == 1 and "ctx is NULL" in err()
    assert call(P=1, C=64, S=16, M=1, K=1) == 1 and "ctx is NULL" in err()
    assert call(P=63, C=2, S=16, M=1, K=1) == 1 and "ctx is NULL" in err()
    assert call(y=names["A"], offset=names["A"], X=names["A"], lw=names["A"]) == 1 and "ctx is NULL" in err()    # read arrays may alias
