"""Numpy restatement of the shared-design GLM posterior predictive (gsmvi_glm_shared_predict_batched_f64,
csrc/gsmvi_glm_shared_predict_batched.hip) in np.longdouble, the generator of its test problems, the weight pattern of every test
that takes weights, the conjugate Gaussian K-fold problem with its independent route through two marginal likelihoods, a stand-in
engine for the host logic of ``predict_shared_batched`` and the argument checks of the C ABI.  Test-only.  Built on
glm_predict_ref.rows (the table of the four families) and psis_loo_shared_ref.valid_mask (the selection rule).  From the
definition in include/gsmvi_hip.h: all K problems have the rows a_m of ONE A (M, D); row m of problem k is valid iff weights is
None or v_km > 0, and for a valid row under q_k = N(mu_k, Sigma_k)

    m = a_m . mu_k + o_km,   v = a_m^T Sigma_k a_m,   (pmean, lpd) = glm_predict_ref.rows(family, m, v, y_km, tau_k, Q)
    eta_mean = m,  eta_var = v;  all four NaN where m or v is not finite

a row that is not valid: NaN in all four, whatever y and the offset hold there.  elpd[k] = sum over the valid rows of v_km lpd[k, m]
in ascending m (v = 1 without weights), 0 without a valid row.  lpd is the density of ONE unit observation, not weighted."""
import ctypes as C
import functools

import numpy as np
from scipy import special, stats

import glm_predict_ref as gp
import psis_loo_shared_ref as plref

FAMILIES = gp.FAMILIES
LD = np.longdouble
PATH_BITS = 0x100000 | 0x20000        # batched_predict | batched_target (checked against HipEngine.PATH_BITS by the CPU test)
FAMILY_CODE = plref.FAMILY_CODE
NAMES = ("eta_mean", "eta_var", "mean", "lpd", "elpd")
# (D, M, K) of the GPU tests.  D in {1, 5, 16}: four slots per workgroup, Dp = 16; D in {17, 33, 64}: one slot, Dp = 32, 48, 64;
# M in {1, 31, 32, 33, 65}: the tile edge, and three tiles with the prefetch; K in {1, 3, 4, 5, 7}: partly filled workgroups
SHAPES = ((1, 31, 3), (5, 65, 7), (16, 33, 4), (16, 65, 5), (17, 32, 7), (33, 65, 3), (64, 33, 5), (64, 65, 1), (5, 1, 4),
          (17, 31, 1), (33, 1, 7), (1, 32, 5))

valid_mask = plref.valid_mask


def predict(family, A, offset, y, weights, tau, mean, cov, Q=32):
    """A (M, D), offset, y and weights (K, M) or None, tau a number or (K,), mean (K, D), cov (K, D, D) -> a dict of float64 arrays
    eta_mean, eta_var, mean, lpd (K, M), elpd (K,) (the last two None without y) and ``scale_var`` (K, M) = sum_ij |a_i| |Sigma_ij|
    |a_j| and ``scale_elpd`` (K,) = sum v |lpd|, what the rounding errors of eta_var and elpd are proportional to.  y and offset
    are looked at in the valid rows only."""
    A, mean, cov = (np.asarray(x, dtype=np.float64) for x in (A, mean, cov))
    M, D = A.shape
    K = mean.shape[0]
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (K,))
    ok = valid_mask(weights, K, M)
    out = {k: np.full((K, M), np.nan) for k in ("eta_mean", "eta_var", "mean", "scale_var")}
    out["lpd"] = np.full((K, M), np.nan) if y is not None else None
    out["elpd"] = np.zeros(K) if y is not None else None
    out["scale_elpd"] = np.zeros(K) if y is not None else None
    for k in range(K):
        idx = np.flatnonzero(ok[k])
        Ak, mu, S = A[idx].astype(LD), mean[k].astype(LD), cov[k].astype(LD)
        with np.errstate(all="ignore"):
            m = Ak @ mu
            if offset is not None:
                m = m + np.asarray(offset, dtype=np.float64)[k, idx].astype(LD)
            v = np.einsum("ni,ij,nj->n", Ak, S, Ak)
            pmean, lpd = gp.rows(family, m, v, None if y is None else np.asarray(y, dtype=np.float64)[k, idx], tau[k], Q)
            bad = ~(np.isfinite(m) & np.isfinite(v))
            out["scale_var"][k, idx] = np.einsum("ni,ij,nj->n", np.abs(Ak), np.abs(S), np.abs(Ak))
        for name, val in (("eta_mean", m), ("eta_var", v), ("mean", pmean)) + ((("lpd", lpd),) if y is not None else ()):
            out[name][k, idx] = np.where(bad, np.nan, val).astype(np.float64)
        if y is not None and idx.size:
            with np.errstate(all="ignore"):
                terms = np.where(bad, np.nan, lpd).astype(LD)
                if weights is not None:
                    terms = np.asarray(weights, dtype=np.float64)[k, idx].astype(LD) * terms
                out["elpd"][k] = np.float64(gp._ordered_sum(terms[None, :])[0])
                out["scale_elpd"][k] = np.float64(np.abs(terms).sum())
    return out


def make_problem(family, K, M, D, seed=None):
    """The problems of the tests on ONE A: RandomState(2000 + 7 M + D) (or ``seed``); A (M, D) = N(0, 1) / sqrt(D), offsets 0.3
    N(0, 1), the posterior means 0.5 N(0, 1), the covariances G G^T / (4 D) scaled down, where needed, so that a^T Sigma_k a <= 0.9
    on every row of every problem (the band the existing predict tests keep: the quadrature at Q = 32 is accurate there), y drawn
    from the family at a theta*_k + o with theta*_k ~ N(mean_k, I / 4) (poisson: the rate capped at e^10; gaussian: noise of
    precision tau_k), tau = 0.5 + U(0, 1) per problem for the gaussian family and 1.0 otherwise.  Returns a dict."""
    rs = np.random.RandomState(2000 + 7 * M + D if seed is None else seed)
    A = rs.standard_normal((M, D)) / np.sqrt(D)
    offset = 0.3 * rs.standard_normal((K, M))
    mean = 0.5 * rs.standard_normal((K, D))
    G = rs.standard_normal((K, D, D))
    cov = G @ np.swapaxes(G, 1, 2) / (4.0 * D)
    vmax = np.einsum("ni,kij,nj->kn", A, cov, A).max(1)
    cov = cov * np.minimum(1.0, 0.9 / vmax)[:, None, None]
    theta = mean + 0.5 * rs.standard_normal((K, D))
    eta = theta @ A.T + offset
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
    return {"family": family, "A": A, "offset": offset, "y": y, "tau": tau, "mean": mean, "cov": cov}


def weight_pattern(K, M, seed=0):
    """the weights of every test that takes weights: U(0, 2) with a quarter of the entries (K M // 4 of them, at random places)
    exactly 0, problem 1 all zero (K > 1), rows 0 .. 31 of problem 2 all zero (K > 2 and M > 32: one slot's tile has no valid row
    while its neighbours' do)"""
    rs = np.random.default_rng([11, K, M, seed])
    w = rs.uniform(0.0, 2.0, size=(K, M))
    w.flat[rs.permutation(K * M)[:(K * M) // 4]] = 0.0
    if K > 1:
        w[1] = 0.0
    if K > 2 and M > 32:
        w[2, :32] = 0.0
    return w


def plant(y, offset, weights):
    """copies of y and offset with NaN and +inf wherever the weight is 0: what a kernel that reads them there would show"""
    y, offset = np.array(y, dtype=np.float64), np.array(offset, dtype=np.float64)
    y[weights == 0.0] = np.nan
    offset[weights == 0.0] = np.inf
    return y, offset


@functools.lru_cache(maxsize=None)
def reference(family, shape, with_offset, with_weights, Q=32):
    """(problem, restatement with y) at ``shape`` = (D, M, K): computed once and shared (do not modify).  With weights the problem
    carries ``weights`` and its y and offset are planted (NaN, +inf) where the weight is 0."""
    D, M, K = shape
    p = make_problem(family, K, M, D)
    p["weights"] = None
    if with_weights:
        p["weights"] = weight_pattern(K, M)
        p["y"], p["offset"] = plant(p["y"], p["offset"], p["weights"])
    r = predict(family, p["A"], p["offset"] if with_offset else None, p["y"], p["weights"], p["tau"], p["mean"], p["cov"], Q)
    return p, r


def rel(got, want, scale=None):
    """max |got - want| / max(1, |want|) (or / scale) over the entries where want is finite; 0 for none"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ok = np.isfinite(want)
    if not ok.any():
        return 0.0
    den = np.maximum(1.0, np.abs(want[ok])) if scale is None else np.asarray(scale, dtype=np.float64)[ok]
    with np.errstate(invalid="ignore"):
        e = np.abs(got[ok] - want[ok]) / den
    return float(np.where(np.isnan(e), np.inf, e).max())


# ---- K-fold cross-validation on the conjugate Gaussian model -------------------------------------------------------------------------
KFOLD = dict(N=24, D=5, F=4, pairs=((0.5, 2.0), (1.0, 1.0), (4.0, 0.5)), seeds=(0, 1, 2, 3, 4))


def kfold_gaussian_problem(N, D, F, lam, tau, seed):
    """y = A x* + noise of precision tau under the prior x ~ N(0, I / lam); F folds by a random permutation.  Returns A (N, D),
    y (N,), the fold masks (F, N) as 0 / 1 floats, and the closed-form posterior of every fold's training rows: mean (F, D),
    cov (F, D, D) (precision lam I + tau A_tr^T A_tr)"""
    rs = np.random.default_rng([seed, N, D, F])
    A = rs.standard_normal((N, D)) / np.sqrt(D)
    y = A @ (rs.standard_normal(D) / np.sqrt(lam)) + rs.standard_normal(N) / np.sqrt(tau)
    fold = rs.permutation(N) % F
    mask = (fold[None, :] == np.arange(F)[:, None]).astype(np.float64)
    mean, cov = np.empty((F, D)), np.empty((F, D, D))
    for f in range(F):
        tr = mask[f] == 0.0
        P = lam * np.eye(D) + tau * A[tr].T @ A[tr]
        S = np.linalg.inv(P)
        cov[f] = 0.5 * (S + S.T)
        mean[f] = cov[f] @ (tau * A[tr].T @ y[tr])
    return A, y, mask, mean, cov


def kfold_gaussian_heldout(A, y, mask, lam, tau):
    """log p(y_train, y_m) - log p(y_train) for every held-out row m of every fold (NaN elsewhere), from the two marginal
    likelihoods y_S ~ N(0, I / tau + A_S A_S^T / lam): a route that never forms a posterior"""
    F, N = mask.shape
    out = np.full((F, N), np.nan)

    def logp(rows):
        As = A[rows]
        return stats.multivariate_normal.logpdf(y[rows], mean=np.zeros(len(rows)), cov=np.eye(len(rows)) / tau + As @ As.T / lam)

    for f in range(F):
        tr = np.flatnonzero(mask[f] == 0.0)
        base = logp(tr)
        for m in np.flatnonzero(mask[f] > 0.0):
            out[f, m] = logp(np.append(tr, m)) - base
    return out


# ---- the stand-in engine of the host-logic tests -----------------------------------------------------------------------------------
class StandInEngine(plref.StandInEngine):
    """psis_loo_shared_ref's stand-in engine (what SharedDesignGLMTarget asks of an engine) with the shared-design predictive
    restated (this file, float64 out).  ``calls`` records the launches as tuples."""
    name = "restatement-shared-predict(test-only)"

    def glm_shared_predict_batched(self, mean, cov, A, family, offset=None, y=None, weights=None, noise_prec=1.0, nodes=32):
        self._rec(("shared_predict", family, tuple(A.shape), y is not None, offset is not None, weights is not None, nodes))
        assert A.dtype == np.float64 and mean.dtype == np.float64 and cov.dtype == np.float64 and A.ndim == 2
        r = predict(family, A, offset, y, weights, noise_prec, mean, cov, nodes)
        return r["eta_mean"], r["eta_var"], r["mean"], r["lpd"], r["elpd"]


# ---- the C ABI's argument checks (NULL context) ------------------------------------------------------------------------------------
def check_bad_arguments(lib):
    """the entry point through the C ABI with a NULL context: every bad argument returns GSMVI_ERR_BAD_ARG (1) with its own
    message, so nothing can have been enqueued; valid calls end at the context"""
    buf = (C.c_double * 16384)()
    p = C.cast(buf, C.c_void_p).value
    a = lambda n: p + 8 * 512 * n                                   # noqa: E731  thirty-two disjoint 4 KB arrays
    err = lambda: (lib.gsmvi_last_error() or b"").decode()           # noqa: E731
    name = "gsmvi_glm_shared_predict_batched_f64"
    names = dict(A=a(0), offset=a(1), y=a(2), weights=a(3), tau_dev=None, mean=a(4), cov=a(5), gh_t=a(6), gh_logw=a(7),
                 eta_mean=a(8), eta_var=a(9), pmean=a(10), lpd=a(11), elpd=a(12))

    def call(K=2, D=4, M=5, family=1, tau=1.0, Q=32, **kw):
        v = dict(names, **kw)
        return lib.gsmvi_glm_shared_predict_batched_f64(None, None, K, D, M, family, v["A"], v["offset"], v["y"], v["weights"], tau,
                                                        v["tau_dev"], v["mean"], v["cov"], Q, v["gh_t"], v["gh_logw"], v["eta_mean"],
                                                        v["eta_var"], v["pmean"], v["lpd"], v["elpd"])

    assert call(D=0) == 1 and "D must be" in err() and name in err()
    assert call(D=65) == 1 and "D must be" in err()
    assert call(K=0) == 1 and "K must be" in err()
    assert call(M=0) == 1 and "M must be" in err()
    assert call(K=2 ** 20, M=2 ** 40) == 1 and "too large" in err()
    assert call(K=2 ** 40) == 1 and "K must be" in err()                          # the launch bound of the shared entries
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
        for arr in ("A", "offset", "y", "weights", "mean", "cov", "gh_t", "gh_logw"):
            assert call(**{w: names[arr]}) == 1 and f"{w} overlaps {arr}" in err(), (w, arr)
    assert call(eta_var=a(8)) == 1 and "eta_var overlaps eta_mean" in err()
    assert call(family=3, tau_dev=a(13), pmean=a(13)) == 1 and "pmean overlaps noise_prec_dev" in err()
    assert call(eta_mean=a(4) + 8 * (2 * 4 - 1)) == 1 and "eta_mean overlaps mean" in err()     # the last element of mean
    assert call(eta_mean=a(4) + 8 * 2 * 4) == 1 and "ctx is NULL" in err()                      # adjacent is not overlapping
    # A is ONE (M, D) matrix: M D doubles, not K M D
    assert call(elpd=a(0) + 8 * (5 * 4 - 1)) == 1 and "elpd overlaps A" in err()
    assert call(elpd=a(0) + 8 * 5 * 4) == 1 and "ctx is NULL" in err()
    assert call(elpd=a(3) + 8 * (2 * 5 - 1)) == 1 and "elpd overlaps weights" in err()          # weights are K M doubles
    for fam in (0, 1, 2, 3):
        assert call(family=fam) == 1 and "ctx is NULL" in err(), fam
        assert call(family=fam, y=None, lpd=None, elpd=None, offset=None, weights=None) == 1 and "ctx is NULL" in err(), fam
    assert call(family=3, tau=2.5) == 1 and "ctx is NULL" in err()
    assert call(family=3, tau=-1.0, tau_dev=a(13)) == 1 and "ctx is NULL" in err()              # the scalar is unused with K values
    assert call(Q=1) == 1 and "ctx is NULL" in err()
    assert call(Q=64) == 1 and "ctx is NULL" in err()
    assert call(y=a(0), offset=a(0), weights=a(0), mean=a(0), cov=a(0)) == 1 and "ctx is NULL" in err()   # read-only arrays may overlap
