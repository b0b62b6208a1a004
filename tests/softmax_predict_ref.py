"""Numpy restatement of the batched softmax posterior predictive (gsmvi_softmax_predict_batched_f64,
csrc/gsmvi_softmax_predict_batched.hip) in np.longdouble, the generator of its test inputs, the expectation by tensor Gauss-Hermite
quadrature that it is pinned to, and a stand-in engine for the host logic of ``predict_softmax_batched``.  Test-only.  Written from
the definition in include/gsmvi_hip.h: for problem k, draws x_s of q_k (class-major: x_s[c P + j] = W_cj), normalised log weights
lw_s (None: lw_s = -log S, w_s = 1 / S) and a valid row i < n_k

    eta_sic = a_i . x_s[c P .. c P + P - 1]  (c < C - 1),   eta_si,C-1 = 0
    m_si    = max_c eta_sic,   z_si = sum_{c = 0 .. C-1} exp(eta_sic - m_si)   (class order, the reference class last)
    p_sic   = exp(eta_sic - m_si) / z_si
    prob[k, i, c] = sum_s w_s p_sic,   w_s = exp(lw_s)
    l_si    = eta_si,y_i - m_si - log z_si
    lpd[k, i]     = log sum_s exp(lw_s + l_si)

NaN: a row with a draw whose eta is not finite (a non-finite entry of a_i or x_s); every valid row of a problem whose lw holds a NaN
or +inf, or only -inf; the lpd of a row whose label is outside 0 .. C - 1; rows i >= n_k.  l_si is psis_loo_softmax_ref's
``loglik_softmax``: there is no second copy."""
import ctypes as C_
import functools

import numpy as np

import psis_loo_ref as lref
import psis_loo_softmax_ref as sref
import softmax_batched_ref as bref
from psis_loo_ref import LD, valid_rows      # noqa: F401
from psis_loo_softmax_ref import draw_labels, loglik_softmax      # noqa: F401

PATH_BITS = 0x100000 | 0x1000000            # GSMVI_PATH_BATCHED_PREDICT | GSMVI_PATH_BATCHED_SOFTMAX: the pair names the launch
BAR = 1e-11                                 # the project's single-launch bar (psis_loo_softmax_ref.LOGLIK_BAR), relative to max(1, |value|)
LDS_MAX = 160 * 1024

# The Monte-Carlo check: |prob - E_q[softmax]| <= 5 x 0.5 / sqrt(S): a probability lies in [0, 1], so its standard deviation over
# the draws is at most 0.5 and the standard error of the mean of S independent draws at most 0.5 / sqrt(S); five of them.
QUAD_S = 4096
QUAD_SEEDS = (0, 1, 2, 3, 4)
QUAD_BOUND = 5 * 0.5 / np.sqrt(QUAD_S)


def lds_bytes(C, P):
    """gsmvi_softmax_predict_lds_bytes(C, P) from the header's formula"""
    if not (C >= 2 and P >= 1 and (C - 1) * P <= 64):
        return 0
    return 8 * (64 * (((C - 1) * P) | 1) + 16 * (4 * ((P + 3) // 4) + 1) + 64 * C + 344)


def rel_gap(got, want):
    """largest |got - want| / max(1, |want|) over the entries; NaN and infinities must sit at the same places with the same sign"""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs"
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), "infinities differ"
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(LD(1), np.abs(want[fin]))))


def predict(A, labels, C, counts, X, lw, dtype=LD):
    """(prob (K, M, C), lpd (K, M) or None without labels) of ``dtype``"""
    A, X = np.asarray(A, dtype=np.float64), np.asarray(X, dtype=np.float64)
    K, M, P = A.shape
    S, D = X.shape[1], X.shape[2]
    assert D == (C - 1) * P
    nk = valid_rows(counts, K, M)
    nan = dtype(np.nan)
    prob = np.full((K, M, C), nan, dtype=dtype)
    lpd = None if labels is None else np.full((K, M), nan, dtype=dtype)
    ell = None if labels is None else loglik_softmax(A, labels, C, counts, X, dtype)          # (K, M, S); NaN by its rules
    for k in range(K):
        n = int(nk[k])
        if n == 0:
            continue
        with np.errstate(all="ignore"):
            if lw is None:
                lwk = np.full(S, -np.log(dtype(S)), dtype=dtype)
                w = np.full(S, dtype(1) / dtype(S), dtype=dtype)
            else:
                l64 = np.asarray(lw, dtype=np.float64)[k]
                if np.isnan(l64).any() or (l64 == np.inf).any() or (l64 == -np.inf).all():
                    continue                                                              # the problem's valid rows stay NaN
                lwk = l64.astype(dtype)
                w = np.exp(lwk)
            W = X[k].astype(dtype).reshape(S, C - 1, P)
            dots = np.einsum("np,scp->nsc", A[k, :n].astype(dtype), W)                    # (n, S, C - 1)
            eta = np.concatenate([dots, np.zeros((n, S, 1), dtype=dtype)], axis=2)
            m = eta.max(axis=2)
            e = np.exp(eta - m[:, :, None])
            z = 1 + bref.s_minus_one(e)                                                   # class order; the reference class last
            p = e / z[:, :, None]
            pr = np.einsum("s,nsc->nc", w, p)
            bad = (~np.isfinite(dots).all(axis=2) | ~np.isfinite(X[k]).all(axis=1)[None, :]).any(axis=1)      # (n,) rows
            prob[k, :n] = np.where(bad[:, None], nan, pr)
            if labels is not None:
                t = lwk[None, :] + ell[k, :n]
                out = lref.lse(t, dtype)
                lpd[k, :n] = np.where(bad | np.isnan(ell[k, :n]).any(axis=1), nan, out)
    return prob, lpd


# ---- the inputs of the GPU tests (tests/test_gpu_softmax_predict.py) ------------------------------------------------------------------
# (C, P, S, M, K, weighted).  K = 3 runs with counts = (0, a partial tile, M); K = 1 without counts.  weighted: lw random normalised
# log weights, else None (uniform).  (C, P) over {(2,1), (3,3), (3,5), (5,4), (9,8), (65,1), (2,64)}, S over {5, 63, 64, 65, 257}
# around the tile of 64 draws, M over {1, 15, 16, 17, 33} around the tile of 16 rows.
CASES = (
    (2, 1, 5, 1, 1, False),             # the smallest of everything
    (3, 3, 63, 15, 3, True),            # P % 4 = 3
    (3, 5, 257, 33, 3, True),           # P % 4 = 1, five draw tiles the last one partial, three row tiles
    (5, 4, 64, 16, 3, False),           # exactly one draw tile and one row tile
    (9, 8, 65, 17, 1, True),
    (65, 1, 63, 17, 3, True),           # D = 64, the most classes: the largest LDS request (above 64 KB)
    (2, 64, 65, 33, 1, False),          # D = 64, one class
    (3, 5, 64, 17, 1, True),
    (5, 4, 5, 33, 3, True),             # one wave at work
)


def case_id(c):
    return f"C{c[0]}-P{c[1]}-S{c[2]}-M{c[3]}-K{c[4]}-{'w' if c[5] else 'u'}"


def partial_count(M):
    """a count of valid rows that ends inside a tile of 16 rows (1 for M = 1)"""
    return max(1, M - 5)


@functools.lru_cache(maxsize=None)
def make_case(case):
    """The inputs of one case (computed once and shared: do not modify), all float64 / int32: new rows A, labels y drawn from the
    model, counts, S draws X of a Gaussian near the model's coefficients and the log weights lw (or None)"""
    Cc, P, S, M, K, weighted = case
    D = (Cc - 1) * P
    rs = np.random.default_rng([Cc, P, S, M, K, int(weighted)])
    A = rs.standard_normal((K, M, P)) / np.sqrt(P)
    W = 1.5 * rs.standard_normal((K, Cc - 1, P))
    y = draw_labels(rs, A, W)
    counts = np.array([0, partial_count(M), M], dtype=np.int32) if K == 3 else None
    X = W.reshape(K, 1, D) + 0.5 * rs.standard_normal((K, S, D))
    lw = None
    if weighted:
        raw = 1.5 * rs.standard_normal((K, S))
        lw = raw - np.asarray(lref.lse(raw, np.float64), dtype=np.float64)[:, None]
    return dict(C=Cc, P=P, K=K, M=M, D=D, S=S, A=A, y=y, counts=counts, X=X, lw=lw)


# ---- the statistical check with an exact answer: C = 3, P = 1 (D = 2), E_q[softmax] by tensor Gauss-Hermite quadrature ---------------
def quad_problem(seed, M=8):
    """a Gaussian q = N(mean, cov) over the two coefficients and M rows a_i (P = 1)"""
    rs = np.random.default_rng([seed, 3, 1, M])
    mean = rs.standard_normal(2)
    G = rs.standard_normal((2, 2))
    cov = 0.3 * (G @ G.T) + 0.2 * np.eye(2)
    A = 1.5 * rs.standard_normal((1, M, 1))
    return dict(mean=mean, cov=cov, A=A, rs=rs)


def quad_exact(p, Q=96):
    """E_q[softmax(a_i x_0, a_i x_1, 0)] for every row, (M, 3), by the Q x Q tensor Gauss-Hermite rule (the integrand is smooth and
    bounded: Q = 64 and Q = 96 agree within 1e-5, four hundred times below the bound of the test)"""
    t, w = np.polynomial.hermite.hermgauss(Q)
    L = np.linalg.cholesky(p["cov"])
    T = np.stack(np.meshgrid(t, t, indexing="ij"), axis=-1).reshape(-1, 2)
    wt = (w[:, None] * w[None, :]).reshape(-1) / np.pi
    Xq = p["mean"][None, :] + np.sqrt(2.0) * T @ L.T                                      # (Q Q, 2)
    eta = np.concatenate([p["A"][0][:, None, :] * Xq[None, :, :], np.zeros((p["A"].shape[1], Xq.shape[0], 1))], axis=2)
    sm = np.exp(eta - eta.max(2, keepdims=True))
    sm = sm / sm.sum(2, keepdims=True)
    return np.einsum("s,nsc->nc", wt, sm)


def quad_draws(p, S):
    return (p["mean"][None, :] + p["rs"].standard_normal((S, 2)) @ np.linalg.cholesky(p["cov"]).T)[None]


# ---- the stand-in engine of the host-logic tests -----------------------------------------------------------------------------------
class StandInEngine(sref.StandInEngine):
    """psis_loo_softmax_ref's stand-in engine with the predictive launch restated (this file, float64 out).  ``calls`` records the
    launches as tuples."""
    name = "oracle-batched-softmax-predict(test-only)"

    def softmax_predict_batched(self, X, lw, A, num_classes, labels=None, counts=None):
        self._rec(("predict_softmax", num_classes, tuple(X.shape), tuple(A.shape), lw is not None, labels is not None,
                   counts is not None))
        prob, lpd = predict(A, labels, num_classes, counts, X, lw)
        return np.asarray(prob, dtype=np.float64), None if lpd is None else np.asarray(lpd, dtype=np.float64)


# ---- the C ABI's argument checks (NULL context) ------------------------------------------------------------------------------------
def check_bad_arguments(lib):
    """the entry point through the C ABI with a NULL context: every bad argument returns GSMVI_ERR_BAD_ARG (1) with its own
    message, so nothing can have been enqueued; valid calls end at the context"""
    err = lambda: (lib.gsmvi_last_error() or b"").decode()          # noqa: E731
    buf = (C_.c_double * 16384)()
    p = C_.cast(buf, C_.c_void_p).value
    at = lambda i: p + 8 * 1024 * i                                   # noqa: E731  (slots of 8 KB: K = 2, M = 5, D = 4, S = 8 fit)
    name = "gsmvi_softmax_predict_batched_f64"
    names = dict(A=at(0), labels=at(1), counts=at(2), X=at(3), lw=at(4), prob=at(5), lpd=at(6))

    def call(K=2, C=3, P=2, M=5, S=8, **kw):
        a = dict(names, **kw)
        return lib.gsmvi_softmax_predict_batched_f64(None, None, K, C, P, M, S, a["A"], a["labels"], a["counts"], a["X"], a["lw"],
                                                     a["prob"], a["lpd"])

    assert call(C=1) == 1 and "C must be" in err() and name in err()
    assert call(C=0) == 1 and "C must be" in err()
    assert call(P=0) == 1 and "P must be" in err()
    assert call(C=66, P=1) == 1 and "D = (C - 1) P" in err()                      # (C - 1) P = 65
    assert call(C=6, P=13) == 1 and "D = (C - 1) P" in err()                      # 65 again
    assert call(C=2, P=65) == 1 and "D = (C - 1) P" in err()
    assert call(C=2 ** 17, P=2 ** 17) == 1 and "D = (C - 1) P" in err()           # the product would overflow an int
    assert call(K=0) == 1 and "K must be" in err()
    assert call(K=2 ** 24) == 1 and "K must be" in err()
    assert call(M=0) == 1 and "M must be" in err()
    assert call(S=0) == 1 and "S must be" in err()
    assert call(S=4097) == 1 and "S must be" in err()
    assert call(K=2 ** 20, M=2 ** 40) == 1 and "too large" in err()
    assert call(K=2 ** 22, M=64) == 1 and "2^24 - 1" in err()                      # K ceil(M / 16) = 2^24 tiles: one too many
    far = {n: (j + 1) << 44 for j, n in enumerate(names)}                          # (never dereferenced: far enough apart not to overlap)
    assert call(K=2 ** 12 - 1, M=16 * 2 ** 12 + 16, **far) == 1 and "ctx is NULL" in err()    # 2^24 - 1 tiles exactly
    assert call(K=2 ** 12 - 1, M=16 * 2 ** 12 + 17, **far) == 1 and "2^24 - 1" in err()
    for arr in ("A", "X", "prob"):
        assert call(**{arr: None}) == 1 and "NULL array" in err(), arr
    assert call(labels=None) == 1 and "labels and lpd" in err()                    # the pairing: both or neither
    assert call(lpd=None) == 1 and "labels and lpd" in err()
    assert call(labels=None, lpd=None) == 1 and "ctx is NULL" in err()
    for w in ("prob", "lpd"):
        for arr, key in (("A", "A"), ("labels", "labels"), ("counts_dev", "counts"), ("X", "X"), ("lw", "lw")):
            assert call(**{w: names[key]}) == 1 and f"{w} overlaps {arr}" in err(), (w, arr)
    assert call(lpd=names["prob"]) == 1 and "lpd overlaps prob" in err()
    assert call(lpd=names["prob"] + 8 * (2 * 5 * 3 - 1)) == 1 and "lpd overlaps prob" in err()     # the last element
    assert call(lpd=names["prob"] + 8 * 2 * 5 * 3) == 1 and "ctx is NULL" in err()                 # adjacent is not overlapping
    assert call() == 1 and "ctx is NULL" in err()
    assert call(counts=None, lw=None) == 1 and "ctx is NULL" in err()
    assert call(S=1) == 1 and "ctx is NULL" in err()
    assert call(S=4096, **far) == 1 and "ctx is NULL" in err()
    assert call(C=65, P=1, S=16, **far) == 1 and "ctx is NULL" in err()
    assert call(C=2, P=64, S=16, **far) == 1 and "ctx is NULL" in err()
    assert call(labels=names["A"], X=names["A"], lw=names["A"]) == 1 and "ctx is NULL" in err()    # read arrays may alias
