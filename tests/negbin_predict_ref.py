"""Numpy restatement of the batched negative binomial posterior predictive (gsmvi_negbin_predict_batched_f64,
csrc/gsmvi_negbin_predict_batched.hip) in np.longdouble, the generator of its test inputs, the log predictive density by 2-D
quadrature that it is pinned to, and a stand-in engine for the host logic of ``predict_negbin_batched``.  Test-only.  Written from
the definition in include/gsmvi_hip.h: for problem k, draws x_s = (beta_s, theta_s) of q_k, normalised log weights lw_s (None:
lw_s = -log S) and a valid row i < n_k

    eta_si = a_i . beta_s + o_i
    lmom[k, i, 0] = log sum_s exp(lw_s + eta_si)
    lmom[k, i, 1] = log sum_s exp(lw_s + 2 eta_si)
    lmom[k, i, 2] = log sum_s exp(lw_s + 2 eta_si - theta_s)
    l_si   = t(eta_si, theta_s, y_i) - lgamma(y_i + 1)
    lpd[k, i]     = log sum_s exp(lw_s + l_si)

NaN: every valid row of a problem with a flagged draw (a non-finite entry, theta included, or e^theta not a positive normal number)
or whose lw holds a NaN or +inf, or only -inf; a row with a draw whose eta is not finite; rows i >= n_k.  l_si and the draw flag are
psis_loo_negbin_ref's ``loglik_negbin`` and ``draw_flag``: there is no second copy."""
import ctypes as C_
import functools

import numpy as np

import psis_loo_negbin_ref as nref
import psis_loo_ref as lref
from psis_loo_negbin_ref import draw_counts, draw_flag, loglik_negbin      # noqa: F401
from psis_loo_ref import LD, valid_rows      # noqa: F401
from softmax_predict_ref import partial_count, rel_gap      # noqa: F401  (relative to max(1, |value|); the NaN patterns compared inside)

PATH_BITS = 0x100000 | 0x20000              # GSMVI_PATH_BATCHED_PREDICT | GSMVI_PATH_BATCHED_TARGET: the pair names the launch
BAR = 1e-11                                 # the project's single-launch bar, relative to max(1, |value|)
LOG_DBL_MAX = 709.782712893384              # e^x overflows float64 above it

# The Monte-Carlo gap of lpd against log int p(y | a beta + o, theta) q(beta, theta) d beta d theta by tensor Gauss-Hermite
# quadrature: P = 1 (D = 2), q the Laplace Gaussian of psis_loo_negbin_ref.quad_problem, M = 12 new rows, S = 4096 uniform draws,
# seeds 0 .. 4 (float64 run of the restatement): the largest |lpd - quadrature| over the rows and seeds, measured by
# tests/test_negbin_predict_cpu.py::test_lpd_is_the_predictive_density_by_quadrature (per seed 0.0057, 0.0177, 0.0077, 0.0110,
# 0.0038), and the bound of the test, twice that for the draw-to-draw spread.
QUAD_SEEDS = (0, 1, 2, 3, 4)
QUAD_S = 4096
QUAD_M = 12
QUAD_GAP = 0.0177
QUAD_BOUND = 2.0 * QUAD_GAP


def lds_bytes(P):
    """the dynamic LDS of the launch from the header's formula"""
    return 8 * (80 * (4 * ((P + 3) // 4) + 1) + 824)


def predict(A, y, offset, counts, X, lw, dtype=LD):
    """(lmom (K, M, 3), lpd (K, M) or None without y) of ``dtype``"""
    A, X = np.asarray(A, dtype=np.float64), np.asarray(X, dtype=np.float64)
    K, M, P = A.shape
    S, D = X.shape[1], X.shape[2]
    assert D == P + 1
    nk = valid_rows(counts, K, M)
    nan = dtype(np.nan)
    lmom = np.full((K, M, 3), nan, dtype=dtype)
    lpd = None if y is None else np.full((K, M), nan, dtype=dtype)
    ell = None if y is None else loglik_negbin(A, y, offset, counts, X, dtype)               # (K, M, S); NaN for flagged draws
    for k in range(K):
        n = int(nk[k])
        if n == 0 or draw_flag(X[k]).any():
            continue                                                                      # the problem's valid rows stay NaN
        with np.errstate(all="ignore"):
            if lw is None:
                lwk = np.full(S, -np.log(dtype(S)), dtype=dtype)
            else:
                l64 = np.asarray(lw, dtype=np.float64)[k]
                if np.isnan(l64).any() or (l64 == np.inf).any() or (l64 == -np.inf).all():
                    continue
                lwk = l64.astype(dtype)
            eta = A[k, :n].astype(dtype) @ X[k, :, :P].astype(dtype).T                        # (n, S)
            if offset is not None:
                eta = eta + np.asarray(offset, dtype=np.float64)[k, :n, None].astype(dtype)
            theta = X[k, None, :, P].astype(dtype)
            bad = ~np.isfinite(eta).all(axis=1)                                               # (n,) rows
            terms = [lwk[None, :] + eta, lwk[None, :] + 2 * eta, lwk[None, :] + (2 * eta - theta)]
            if y is not None:
                terms.append(lwk[None, :] + ell[k, :n])
            out = [np.where(bad, nan, lref.lse(np.where(bad[:, None], dtype(0), t), dtype)) for t in terms]
            lmom[k, :n] = np.stack(out[:3], axis=1)
            if y is not None:
                lpd[k, :n] = out[3]
    return lmom, lpd


def variance(lmom):
    """(mean, var) of the predictive count from the log moments, in their dtype: e^l0 and e^l0 + e^l2 + e^l1 - e^(2 l0)"""
    with np.errstate(all="ignore"):
        m1, m2, m2r = np.exp(lmom[..., 0]), np.exp(lmom[..., 1]), np.exp(lmom[..., 2])
        return m1, m1 + m2r + m2 - m1 * m1


# ---- the inputs of the GPU tests (tests/test_gpu_negbin_predict.py) ---------------------------------------------------------------
# (P, with offset, S, M, K, weighted).  K = 3 runs with counts = (M, a partial tile, 0); K = 1 without counts.  weighted: lw random
# normalised log weights, else None (uniform).  P over {1, 3, 4, 5, 8, 16, 63} (P % 4 = 0 .. 3, the largest), S over {5, 63, 64,
# 65, 257} around the tile of 64 draws, M over {1, 15, 16, 17, 33} around the tile of 16 rows.
CASES = (
    (1, False, 5, 1, 1, False),             # the smallest of everything
    (3, True, 63, 15, 3, True),             # P % 4 = 3
    (5, True, 257, 33, 3, True),            # P % 4 = 1, five draw tiles the last one partial, three row tiles
    (4, False, 64, 16, 3, False),           # exactly one draw tile and one row tile
    (8, True, 65, 17, 1, True),
    (63, True, 63, 17, 3, True),            # D = 64: the largest LDS request
    (16, False, 64, 17, 1, True),
    (4, True, 5, 33, 3, True),              # one wave at work
)


def case_id(c):
    return f"P{c[0]}-{'off' if c[1] else 'nooff'}-S{c[2]}-M{c[3]}-K{c[4]}-{'w' if c[5] else 'u'}"


@functools.lru_cache(maxsize=None)
def make_case(case):
    """The inputs of one case (computed once and shared: do not modify), all float64 / int32: new rows A, counts y drawn from the
    model, offset, counts, S draws X of a Gaussian near the model's coefficients whose theta is uniform on [-2, 4] (draws 0 and 1
    of every problem at 3.5 and 0.5: both sides of the r = 10 branch of the link) and the log weights lw (or None).  |eta| stays
    below 6 and the restatement is finite on every valid row (asserted)."""
    P, with_offset, S, M, K, weighted = case
    D = P + 1
    rs = np.random.default_rng([P, int(with_offset), S, M, K, int(weighted)])
    A = rs.standard_normal((K, M, P)) / np.sqrt(P)
    offset = 0.3 * rs.standard_normal((K, M)) if with_offset else None
    beta = 0.7 * rs.standard_normal((K, P))
    y = draw_counts(rs, A, offset, beta, np.exp(rs.uniform(0.0, 3.0, K)))
    counts = np.array([M, partial_count(M), 0], dtype=np.int32) if K == 3 else None
    X = np.concatenate([beta[:, None, :] + 0.3 * rs.standard_normal((K, S, P)), rs.uniform(-2.0, 4.0, (K, S, 1))], axis=2)
    X[:, 0, P], X[:, 1, P] = 3.5, 0.5
    lw = None
    if weighted:
        raw = 1.5 * rs.standard_normal((K, S))
        lw = raw - np.asarray(lref.lse(raw, np.float64), dtype=np.float64)[:, None]
    eta = np.einsum("kmp,ksp->kms", A, X[:, :, :P]) + (offset[:, :, None] if with_offset else 0.0)
    assert np.abs(eta).max() < 6.0 and X[:, :, P].min() >= -2.0 and X[:, :, P].max() <= 4.0, case
    p = dict(P=P, K=K, M=M, D=D, S=S, A=A, y=y, offset=offset, counts=counts, X=X, lw=lw)
    lmom, lpd = predict(A, y, offset, counts, X, lw)
    live = np.arange(M)[None, :] < valid_rows(counts, K, M)[:, None]
    assert np.isfinite(lmom[live].astype(np.float64)).all() and np.isfinite(lpd[live].astype(np.float64)).all(), case
    assert np.isnan(lmom[~live]).all() and np.isnan(lpd[~live]).all(), case
    p["want"] = (lmom, lpd)                                                   # the longdouble restatement of the case
    return p


# ---- the statistical check with an exact answer: P = 1 (D = 2), the predictive density by tensor Gauss-Hermite quadrature ---------
def quad_problem(seed, M=QUAD_M):
    """psis_loo_negbin_ref.quad_problem's fitted Gaussian q = N(mean, cov) over (beta, theta) and M new rows (a_i, y_i) drawn from
    the model at the mean of q"""
    p = nref.quad_problem(seed, **nref.QUAD_SHAPE)
    rs = np.random.default_rng([seed, M, 78])
    A = rs.standard_normal((1, M, 1))
    y = draw_counts(rs, A, None, p["mean"][None, :1], np.exp(p["mean"][1:]))
    return dict(mean=p["mean"], cov=p["cov"], A=A, y=y, rs=rs)


def quad_exact(p, Q=96):
    """(lmom0, lpd) (M,) each: log E_q[e^eta] and log E_q[p(y_i | a_i beta, theta)] by the Q x Q tensor Gauss-Hermite rule (the
    integrand is smooth: Q = 64 and Q = 96 agree within 1e-12)"""
    t, w = np.polynomial.hermite.hermgauss(Q)
    L = np.linalg.cholesky(p["cov"])
    T = np.stack(np.meshgrid(t, t, indexing="ij"), axis=-1).reshape(-1, 2)
    lwt = np.log((w[:, None] * w[None, :]).reshape(-1) / np.pi)
    Xq = p["mean"][None, :] + np.sqrt(2.0) * T @ L.T                                      # (Q Q, 2)
    ell = np.asarray(loglik_negbin(p["A"], p["y"], None, None, Xq[None], np.float64), dtype=np.float64)[0]      # (M, Q Q)
    eta = p["A"][0] * Xq[None, :, 0]
    return (np.asarray(lref.lse(lwt[None, :] + eta, np.float64), dtype=np.float64),
            np.asarray(lref.lse(lwt[None, :] + ell, np.float64), dtype=np.float64))


def quad_draws(p, S):
    return (p["mean"][None, :] + p["rs"].standard_normal((S, 2)) @ np.linalg.cholesky(p["cov"]).T)[None]


# ---- the stand-in engine of the host-logic tests -----------------------------------------------------------------------------------
class StandInEngine(nref.StandInEngine):
    """psis_loo_negbin_ref's stand-in engine with the predictive launch restated (this file, float64 out).  ``calls`` records the
    launches as tuples."""
    name = "oracle-batched-negbin-predict(test-only)"

    def negbin_predict_batched(self, X, lw, A_new, y=None, offset=None, counts=None):
        self._rec(("predict_negbin", tuple(X.shape), tuple(A_new.shape), lw is not None, y is not None, offset is not None,
                   counts is not None))
        lmom, lpd = predict(A_new, y, offset, counts, X, lw)
        return np.asarray(lmom, dtype=np.float64), None if lpd is None else np.asarray(lpd, dtype=np.float64)


# ---- the C ABI's argument checks (NULL context) ------------------------------------------------------------------------------------
def check_bad_arguments(lib):
    """the entry point through the C ABI with a NULL context: every bad argument returns GSMVI_ERR_BAD_ARG (1) with its own
    message, so nothing can have been enqueued; valid calls end at the context"""
    err = lambda: (lib.gsmvi_last_error() or b"").decode()          # noqa: E731
    buf = (C_.c_double * 16384)()
    p = C_.cast(buf, C_.c_void_p).value
    at = lambda i: p + 8 * 1024 * i                                   # noqa: E731  (slots of 8 KB: K = 2, M = 5, D = 4, S = 8 fit)
    name = "gsmvi_negbin_predict_batched_f64"
    names = dict(A=at(0), y=at(1), offset=at(2), counts=at(3), X=at(4), lw=at(5), lmom=at(6), lpd=at(7))

    def call(K=2, P=3, M=5, S=8, **kw):
        a = dict(names, **kw)
        return lib.gsmvi_negbin_predict_batched_f64(None, None, K, P, M, S, a["A"], a["y"], a["offset"], a["counts"], a["X"],
                                                    a["lw"], a["lmom"], a["lpd"])

    assert call(P=0) == 1 and "P must be" in err() and name in err()
    assert call(P=64) == 1 and "P must be" in err()                               # D = 65
    assert call(P=-1) == 1 and "P must be" in err()
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
    for arr in ("A", "X", "lmom"):
        assert call(**{arr: None}) == 1 and "NULL array" in err(), arr
    assert call(y=None) == 1 and "y and lpd" in err()                              # the pairing: both or neither
    assert call(lpd=None) == 1 and "y and lpd" in err()
    assert call(y=None, lpd=None) == 1 and "ctx is NULL" in err()
    for w in ("lmom", "lpd"):
        for arr, key in (("A", "A"), ("y", "y"), ("offset", "offset"), ("counts_dev", "counts"), ("X", "X"), ("lw", "lw")):
            assert call(**{w: names[key]}) == 1 and f"{w} overlaps {arr}" in err(), (w, arr)
    assert call(lpd=names["lmom"]) == 1 and "lpd overlaps lmom" in err()
    assert call(lpd=names["lmom"] + 8 * (2 * 5 * 3 - 1)) == 1 and "lpd overlaps lmom" in err()     # the last element
    assert call(lpd=names["lmom"] + 8 * 2 * 5 * 3) == 1 and "ctx is NULL" in err()                 # adjacent is not overlapping
    assert call() == 1 and "ctx is NULL" in err()
    assert call(offset=None, counts=None, lw=None) == 1 and "ctx is NULL" in err()
    assert call(S=1) == 1 and "ctx is NULL" in err()
    assert call(S=4096, **far) == 1 and "ctx is NULL" in err()
    assert call(P=63, S=16, **far) == 1 and "ctx is NULL" in err()
    assert call(P=1, S=16) == 1 and "ctx is NULL" in err()
    assert call(y=names["A"], offset=names["A"], X=names["A"], lw=names["A"]) == 1 and "ctx is NULL" in err()    # read arrays may alias
