"""The batched negative binomial posterior predictive without a GPU: the C ABI declaration, binding and argument checks through the
built library; the host logic of ``predict_negbin_batched`` on a stand-in engine; the properties of the restatement
(tests/negbin_predict_ref.py): one-hot weights give the score launch's lp, log E[mu] against its closed form, the Poisson limit, lpd
against a 2-D quadrature, the NaN rules."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from scipy import special

import glm_batched_ref as gref
import negbin_batched_ref as bref
import negbin_predict_ref as ref
import psis_loo_ref as lref
from gsmvi_amd import predict_negbin_batched      # noqa: F401  (the feature: without it nothing here can pass)
from gsmvi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsmvi_negbin_predict_batched_f64"


# ---- 1. declaration, binding, argument checks --------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr)
    for mp in ("exports.map", "exports_debug.map"):
        assert re.search(r"^\s*" + NAME + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), mp
    assert NAME in _lib.exported_symbols() and NAME in built
    res, args = _lib._SIGS[NAME]
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert res is C.c_int and len(args) == len(params) == 14
    for p, a in zip(params, args):
        want = C.c_int64 if p.startswith("int64_t") else C.c_int if p.startswith("int ") else \
            C.c_double if p.startswith("double ") else C.c_void_p
        assert a is want, (p, a)
    assert NAME in hdr.split("#ifndef GSMVI_HIP_H")[0]                         # the mapping list
    block = hdr[:hdr.index("int " + NAME)].rsplit("/*", 1)[1]                  # the definition is written above the entry point
    for line in ("eta_si = a_i . beta_s + o_i,   theta_s = x_s[P],   r_s = e^theta_s",
                 "lmom[k, i, 0] = log sum_s exp(lw_s + eta_si)",
                 "lmom[k, i, 1] = log sum_s exp(lw_s + 2 eta_si)",
                 "lmom[k, i, 2] = log sum_s exp(lw_s + 2 eta_si - theta_s)",
                 "l_si   = t(eta_si, theta_s, y_i) - lgamma(y_i + 1)",
                 "lpd[k, i]     = log sum_s exp(lw_s + l_si)",
                 "INCLUDED",
                 "8 (80 (4 ceil(P / 4) + 1) + 824) bytes",
                 "GSMVI_PATH_BATCHED_PREDICT |",
                 "GSMVI_PATH_BATCHED_TARGET: after a reset exactly that pair identifies this launch"):
        assert line in block, line
    assert ref.lds_bytes(63) == 48192 < 64 * 1024                              # no kernel attribute is needed
    # no new path bit, the word is not widened, the ABI version stays
    assert len(re.findall(r"#define\s+GSMVI_PATH_\w+\s+0x[0-9a-fA-F]+u", hdr)) == 32
    assert re.search(r"#define\s+GSMVI_ABI_VERSION\s+1\b", hdr) and _lib.load_library().gsmvi_abi_version() == 1
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_predict"] | HipEngine.PATH_BITS["batched_target"] == ref.PATH_BITS
    assert callable(HipEngine.negbin_predict_batched)
    import gsmvi_amd
    assert gsmvi_amd.predict_negbin_batched is not None and "predict_negbin_batched" in gsmvi_amd.__doc__
    assert dataclasses.is_dataclass(gsmvi_amd.NegBinPrediction) and "709.78" in gsmvi_amd.NegBinPrediction.__doc__
    assert "predict_negbin_batched" in gsmvi_amd.BatchedNegBinomialTarget.__doc__
    assert [f.name for f in dataclasses.fields(gsmvi_amd.NegBinPrediction)] == \
        ["mean", "var", "log_moments", "lpd", "elpd", "psis", "num_draws", "nlaunch"]


def test_abi_checks_arguments_before_the_context():
    ref.check_bad_arguments(_lib.load_library())


def test_the_cases_are_the_table():
    assert ref.CASES == ((1, False, 5, 1, 1, False), (3, True, 63, 15, 3, True), (5, True, 257, 33, 3, True),
                         (4, False, 64, 16, 3, False), (8, True, 65, 17, 1, True), (63, True, 63, 17, 3, True),
                         (16, False, 64, 17, 1, True), (4, True, 5, 33, 3, True))
    assert ref.BAR == 1e-11
    for case in ref.CASES:
        p = ref.make_case(case)                                               # (asserts the ranges and the finiteness itself)
        if p["K"] == 3:
            M = p["M"]
            assert p["counts"].tolist() == [M, ref.partial_count(M), 0] and (p["counts"][1] % 16 != 0 or M == 1)
        r = np.exp(p["X"][:, :, -1])
        assert (r < 10.0).any(1).all() and (r >= 10.0).any(1).all()           # both branches of the link in every problem


# ---- 2. host logic on the stand-in engine ------------------------------------------------------------------------------------------
def _fitted(K=3, N=12, P=3, M=7, seed=3):
    import gsmvi_amd
    rs = np.random.default_rng(seed)
    A = rs.standard_normal((K, N + M, P)) / np.sqrt(P)
    offset = 0.3 * rs.standard_normal((K, N + M))
    y = ref.draw_counts(rs, A, offset, rs.standard_normal((K, P)), np.exp(rs.uniform(0.0, 3.0, K)))
    eng = ref.StandInEngine()
    tgt = gsmvi_amd.BatchedNegBinomialTarget(A[:, :N], y[:, :N], 1.0, offset=offset[:, :N], log_size_mean=1.5,
                                             log_size_precision=1.0, engine=eng)
    D = P + 1
    mean = np.concatenate([0.3 * rs.standard_normal((K, P)), np.full((K, 1), 1.5)], axis=1)
    G = rs.standard_normal((K, D, D))
    cov = np.linalg.inv(np.eye(D)[None] + 0.3 * G @ np.swapaxes(G, 1, 2))
    return tgt, eng, mean, 0.5 * (cov + np.swapaxes(cov, 1, 2)), A[:, N:], y[:, N:], offset[:, N:]


def _launches(eng):
    return [c for c in eng.calls if isinstance(c, tuple)]


def test_uniform_mode_draws_once_makes_no_lp_call_and_summarises_under_counts():
    import gsmvi_amd
    tgt, eng, mean, cov, A_new, y_new, o_new = _fitted()
    K, M, D, S = 3, 7, 4, 40
    keys = [5, 6, 7]
    cnt = np.array([7, 0, 4])
    m0, c0 = mean.copy(), cov.copy()
    eng.calls.clear()
    r = gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A_new, keys, offset=o_new, y=y_new, counts=cnt, num_draws=S, call=2)
    assert isinstance(r, gsmvi_amd.NegBinPrediction) and r.nlaunch == 2 and r.num_draws == S and r.psis is None
    assert np.array_equal(mean, m0) and np.array_equal(cov, c0)
    seeds = tuple((k % 2 ** 32) ^ 0x5DEECE66D for k in keys)
    assert _launches(eng) == [("draw", seeds, 2, 0, S), ("predict_negbin", (K, S, D), (K, M, 3), False, True, True, True)]
    # the draws are psis_batched's for the same keys and call
    top = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, call=2, moments=False, engine=ref.StandInEngine())
    lmom, lpd = ref.predict(A_new, y_new, o_new, cnt, top.samples, None)
    assert isinstance(r.mean, np.ndarray) and r.log_moments.shape == (K, M, 3) and r.mean.shape == r.var.shape == r.lpd.shape == (K, M)
    assert r.elpd.shape == (K,)
    assert np.array_equal(r.log_moments, np.asarray(lmom, dtype=np.float64), equal_nan=True)
    assert np.array_equal(r.lpd, np.asarray(lpd, dtype=np.float64), equal_nan=True)
    mask = np.arange(M)[None, :] < cnt[:, None]
    for a in (r.mean, r.var, r.lpd, r.log_moments):
        assert np.isfinite(a[mask]).all() and np.isnan(a[~mask]).all()
    # mean and var are composed from the log moments; the variance is wider than the mean
    wm, wv = ref.variance(np.asarray(lmom, dtype=np.float64))
    assert np.array_equal(r.mean[mask], wm[mask]) and np.allclose(r.var[mask], wv[mask], rtol=1e-12, atol=0)
    assert (r.var[mask] > r.mean[mask]).all()
    # elpd: the sum over the valid rows, 0 for a problem without one
    want = np.array([r.lpd[k, :cnt[k]].sum() for k in range(K)])
    assert np.allclose(r.elpd, want, rtol=1e-14, atol=0) and r.elpd[1] == 0.0 and (r.elpd[[0, 2]] < 0).all()
    # without y: no lpd, no elpd, the same moments; without counts and offset every row counts
    eng.calls.clear()
    bare = gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A_new, keys, offset=o_new, counts=cnt, num_draws=S, call=2)
    assert bare.lpd is None and bare.elpd is None and _launches(eng)[-1] == ("predict_negbin", (K, S, D), (K, M, 3), False, False, True, True)
    assert np.array_equal(bare.log_moments, r.log_moments, equal_nan=True)
    eng.calls.clear()
    full = gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A_new, keys, num_draws=S, call=2)
    assert _launches(eng)[-1] == ("predict_negbin", (K, S, D), (K, M, 3), False, False, False, False) and np.isfinite(full.mean).all()
    # the target gained no method
    assert not any(hasattr(tgt, name) for name in ("neg_hessian", "predict", "loo", "family"))


def test_psis_mode_weights_the_draws_and_psis_is_reused():
    import gsmvi_amd
    tgt, eng, mean, cov, A_new, y_new, o_new = _fitted()
    K, M, D, S = 3, 7, 4, 40
    keys = [5, 6, 7]
    eng.calls.clear()
    r = gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A_new, keys, o_new, y_new, num_draws=S, weights="psis")
    seeds = tuple((k % 2 ** 32) ^ 0x5DEECE66D for k in keys)
    assert _launches(eng) == [("draw", seeds, 0, 0, S), ("negbin", "lp"), ("psis", (K, S, D), False),
                              ("predict_negbin", (K, S, D), (K, M, 3), True, True, True, False)]
    assert r.nlaunch == 3 and isinstance(r.psis, gsmvi_amd.PSISBatchedResult) and r.psis.khat.shape == (K,) and r.psis.mean is None
    lmom, lpd = ref.predict(A_new, y_new, o_new, None, r.psis.samples, r.psis.log_weights)
    assert np.array_equal(r.log_moments, np.asarray(lmom, dtype=np.float64)) and np.array_equal(r.lpd, np.asarray(lpd, dtype=np.float64))
    uni = gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A_new, keys, o_new, y_new, num_draws=S)
    assert not np.array_equal(uni.log_moments, r.log_moments) and uni.psis is None
    # psis= with "psis": one launch, the same numbers; with "uniform": its samples only
    names = ("mean", "var", "log_moments", "lpd", "elpd")
    eng.calls.clear()
    again = gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A_new, keys, o_new, y_new, psis=r.psis, weights="psis", num_draws=7)
    assert [c[0] for c in _launches(eng)] == ["predict_negbin"] and again.nlaunch == 1 and again.num_draws == S
    assert again.psis is r.psis
    for n in names:
        assert np.array_equal(getattr(again, n), getattr(r, n)), n
    eng.calls.clear()
    plain = gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A_new, keys, o_new, y_new, psis=r.psis)
    assert _launches(eng) == [("predict_negbin", (K, S, D), (K, M, 3), False, True, True, False)] and plain.nlaunch == 1
    for n in names:
        assert np.array_equal(getattr(plain, n), getattr(uni, n)), n
    # a problem whose problem-level run failed comes out NaN
    broken = dataclasses.replace(r.psis, log_weights=np.where(np.arange(K)[:, None] == 1, np.nan, r.psis.log_weights))
    b = gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A_new, keys, o_new, y_new, psis=broken, weights="psis")
    assert all(np.isnan(getattr(b, n)[1]).all() for n in names)
    assert np.array_equal(b.mean[[0, 2]], r.mean[[0, 2]]) and np.array_equal(b.elpd[[0, 2]], r.elpd[[0, 2]])
    # torch out
    t = gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A_new, keys, o_new, y_new, psis=r.psis, as_torch=True)
    assert isinstance(t.var, torch.Tensor) and isinstance(t.elpd, torch.Tensor)
    assert np.array_equal(np.asarray(t.var), plain.var) and np.array_equal(np.asarray(t.elpd), plain.elpd)


def test_type_and_argument_errors_come_before_any_engine_call():
    import gsmvi_amd
    tgt, eng, mean, cov, A_new, y_new, o_new = _fitted()
    Ag, yg, offset, _, _, tau, _ = gref.make_inputs("poisson", 3, 12, 4, 1, seed=3)
    glm = gsmvi_amd.BatchedGLMTarget(Ag, yg, "poisson", 1.0, offset=offset, noise_precision=tau, engine=lref.StandInEngine())
    eng.calls.clear()
    for bad in (glm, tgt.lp, None):
        with pytest.raises(TypeError, match="BatchedNegBinomialTarget"):
            gsmvi_amd.predict_negbin_batched(bad, mean, cov, A_new, [1, 2, 3])
    pr = lambda *a, **kw: gsmvi_amd.predict_negbin_batched(tgt, *a, **kw)     # noqa: E731
    keys = [1, 2, 3]
    with pytest.raises(ValueError, match="predict_negbin_batched: A_new"):
        pr(mean, cov, A_new[:, :, :1], keys)
    with pytest.raises(ValueError, match="A_new"):
        pr(mean, cov, A_new[:2], keys)
    with pytest.raises(ValueError, match="A_new"):
        pr(mean, cov, A_new[0], keys)
    with pytest.raises(ValueError, match="predict_negbin_batched: mean must be"):
        pr(mean[:, :3], cov, A_new, keys)
    with pytest.raises(ValueError, match="cov must be"):
        pr(mean, cov[:, :3], A_new, keys)
    with pytest.raises(ValueError, match=r"predict_negbin_batched: offset: expected shape \(K, M\)"):
        pr(mean, cov, A_new, keys, offset=o_new[:, :3])
    bad_o = o_new.copy()
    bad_o[1, 2] = np.inf
    with pytest.raises(ValueError, match=r"offset: non-finite values .* problems \[1\]"):
        pr(mean, cov, A_new, keys, offset=bad_o)
    with pytest.raises(ValueError, match="predict_negbin_batched: y: expected shape"):
        pr(mean, cov, A_new, keys, y=y_new[:, :3])
    for v in (-1.0, np.nan, np.inf):
        bad_y = y_new.copy()
        bad_y[2, 1] = v
        with pytest.raises(ValueError, match=r"y: values negative or non-finite .* problems \[2\]"):
            pr(mean, cov, A_new, keys, y=bad_y)
    assert not _launches(eng)
    ok = pr(mean, cov, A_new, keys, y=bad_y, offset=bad_o, counts=np.array([7, 2, 1]), num_draws=8)      # beyond counts: ignored
    half = y_new + 0.5                                                        # non-integers are allowed, as in the target
    assert ok.lpd.shape == (3, 7) and np.isfinite(pr(mean, cov, A_new, keys, y=half, num_draws=8).lpd).all()
    eng.calls.clear()
    with pytest.raises(ValueError, match=r"predict_negbin_batched: counts: values outside 0 \.\. M = 7"):
        pr(mean, cov, A_new, keys, counts=np.array([1, 8, 2]))
    with pytest.raises(ValueError, match="counts: expected 3 integers"):
        pr(mean, cov, A_new, keys, counts=np.array([1.0, 2.0, 2.0]))
    with pytest.raises(ValueError, match="keys"):
        pr(mean, cov, A_new, [1, 2])
    for S in (4, 4097, 0, 10.5):
        with pytest.raises(ValueError, match="num_draws"):
            pr(mean, cov, A_new, keys, num_draws=S)
    for w in ("PSIS", None, "importance", 1):
        with pytest.raises(ValueError, match="weights"):
            pr(mean, cov, A_new, keys, weights=w)
    with pytest.raises(ValueError, match="PSISBatchedResult"):
        pr(mean, cov, A_new, keys, psis=dict(samples=None))
    w = gsmvi_amd.psis_weights_batched(np.zeros((3, 8)), engine=ref.StandInEngine())
    with pytest.raises(ValueError, match="samples"):                           # the weights entry keeps no draws
        pr(mean, cov, A_new, keys, psis=w)
    assert not _launches(eng)
    good = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=8, moments=False, engine=ref.StandInEngine())
    eng.calls.clear()                                                          # (tgt.lp went through the target's engine)
    with pytest.raises(ValueError, match=r"psis.samples must be"):
        pr(mean, cov, A_new, keys, psis=dataclasses.replace(good, samples=good.samples[:, :, :3]))
    with pytest.raises(ValueError, match="log_ratios and psis.log_weights"):
        pr(mean, cov, A_new, keys, psis=dataclasses.replace(good, log_weights=good.log_weights[:, :5]), weights="psis")
    assert not _launches(eng)

    class Device(ref.StandInEngine):                                           # an engine that works on device tensors
        device = torch.device("cpu")
    with pytest.raises(ValueError, match="samples, log_ratios, log_weights"):  # host copies: as_torch=False results
        gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A_new, keys, psis=good, engine=Device())


# ---- 3. properties of the restatement ------------------------------------------------------------------------------------------
def test_one_hot_weights_give_the_score_launchs_lp():
    """lw one-hot on draw s*, the new rows the training rows, flat priors (lam = kap = 0): sum_i (lpd_i + lgamma(y_i + 1)) is
    negbin_batched_ref's lp at x_s*, within 1e-12 relative"""
    for case in (ref.CASES[1], ref.CASES[2], ref.CASES[4]):
        p = ref.make_case(case)
        K, S, M = p["K"], p["S"], p["M"]
        nk = ref.valid_rows(p["counts"], K, M)
        _, lp = bref.score_and_lp_ld(p["A"], p["y"], p["offset"], p["counts"], 0.0, 0.0, 0.0, p["X"])
        for star in (0, 1, S - 1):
            lw = np.full((K, S), -np.inf)
            lw[:, star] = 0.0
            _, lpd = ref.predict(p["A"], p["y"], p["offset"], p["counts"], p["X"], lw)
            for k in range(K):
                n = int(nk[k])
                if n == 0:
                    continue
                got = (lpd[k, :n] + special.gammaln(p["y"][k, :n] + 1.0).astype(ref.LD)).sum()
                assert abs(got - lp[k, star]) <= 1e-12 * max(1.0, abs(float(lp[k, star]))), (case, star, k)


def test_log_mean_is_the_closed_form():
    """uniform weights, S = 4096 draws of q, seeds 0 .. 4: lmom0 against log E[e^eta] = a . m_beta + o + v / 2, v = a^T Sigma_bb a:
    within 5 standard errors of the mean of S independent e^(eta - its mean), se = sqrt((e^v - 1) / S), relative to E: the log's
    error to first order; v <= 0.5, so 5 se <= 0.063"""
    P, M, S = 3, 8, 4096
    worst = 0.0
    for seed in range(5):
        rs = np.random.default_rng([seed, P, M, 41])
        A = rs.standard_normal((1, M, P)) / np.sqrt(P)
        o = 0.3 * rs.standard_normal((1, M))
        mean = np.concatenate([0.5 * rs.standard_normal(P), [1.5]])
        G = rs.standard_normal((P + 1, P + 1))
        cov = 0.03 * (G @ G.T) + 0.03 * np.eye(P + 1)
        v = np.einsum("mp,pq,mq->m", A[0], cov[:P, :P], A[0])
        assert v.max() <= 0.5
        X = (mean[None, :] + rs.standard_normal((S, P + 1)) @ np.linalg.cholesky(cov).T)[None]
        lmom, _ = ref.predict(A, None, o, None, X, None, np.float64)
        exact = A[0] @ mean[:P] + o[0] + 0.5 * v
        ratio = np.abs(lmom[0, :, 0] - exact) / (5.0 * np.sqrt(np.expm1(v) / S))
        worst = max(worst, float(ratio.max()))
    print(f"largest |lmom0 - closed form| in units of the bound: {worst:.3f}")
    assert worst <= 1.0


def test_large_size_is_the_poisson_predictive():
    """theta_s = 35 in every draw (r = 1.6e15): lpd against the log-mean-exp of the Poisson log pmf at the same eta, within 1e-9;
    and lmom2 = lmom1 - 35: the overdispersion part of the variance is gone"""
    rs = np.random.default_rng(35)
    K, M, P, S = 2, 9, 4, 64
    A = rs.standard_normal((K, M, P)) / np.sqrt(P)
    offset = 0.3 * rs.standard_normal((K, M))
    beta = 1.5 * rs.standard_normal((K, S, P))
    eta = np.einsum("kmp,ksp->kms", A, beta) + offset[:, :, None]
    y = rs.poisson(np.exp(eta[:, :, 0])).astype(np.float64)
    X = np.concatenate([beta, np.full((K, S, 1), 35.0)], axis=2)
    counts = np.array([M, 5])
    raw = rs.standard_normal((K, S))
    lw = raw - np.asarray(lref.lse(raw, np.float64), dtype=np.float64)[:, None]
    for w in (None, lw):
        lmom, lpd = ref.predict(A, y, offset, counts, X, w)
        po = lref.loglik("poisson", A, y, offset, counts, 1.0, beta, ref.LD)               # (K, M, S)
        lwk = np.full((K, 1, S), -np.log(ref.LD(S))) if w is None else w[:, None, :].astype(ref.LD)
        want = lref.lse(lwk + po)
        g = ref.rel_gap(lpd, want)
        print(f"theta = 35 against the poisson predictive: {g:.2e}")
        assert g <= 1e-9
        live = np.arange(M)[None, :] < counts[:, None]
        assert np.abs(lmom[live][:, 2] - (lmom[live][:, 1] - 35)).max() <= 1e-15


def test_lpd_is_the_predictive_density_by_quadrature():
    """P = 1 (D = 2: beta and theta), q the Laplace Gaussian of psis_loo_negbin_ref.quad_problem, 12 new rows, seeds 0 .. 4: lpd of
    the restatement on S = 4096 uniform draws of q against log int p(y_i | a_i beta, theta) q(beta, theta) by tensor Gauss-Hermite
    quadrature: a Monte-Carlo gap, bounded by twice the largest measured over the rows and seeds (negbin_predict_ref.QUAD_GAP)"""
    gap, gap0 = [], []
    for seed in ref.QUAD_SEEDS:
        p = ref.quad_problem(seed)
        e0, el = ref.quad_exact(p)
        f0, fl = ref.quad_exact(p, Q=64)
        assert max(np.abs(e0 - f0).max(), np.abs(el - fl).max()) <= 1e-12 and (el < 0).all()
        lmom, lpd = ref.predict(p["A"], p["y"], None, None, ref.quad_draws(p, ref.QUAD_S), None, np.float64)
        gap.append(float(np.abs(lpd[0] - el).max()))
        gap0.append(float(np.abs(lmom[0, :, 0] - e0).max()))
    print(f"lpd gap {max(gap):.4f} (per seed {np.array2string(np.array(gap), precision=4)}), lmom0 gap {max(gap0):.4f}")
    assert abs(max(gap) - ref.QUAD_GAP) <= 0.02 * ref.QUAD_GAP                  # the recorded gap is the measured one
    assert ref.QUAD_BOUND == 2.0 * ref.QUAD_GAP and max(gap) <= ref.QUAD_BOUND


def test_restatement_nan_rules():
    """the rules of the header: a flagged draw (a non-finite beta or theta entry, e^theta not a positive normal number) -> every
    valid row of its problem, whatever its weight; a non-finite a or o entry -> its row; a NaN or +inf in lw, or only -inf -> the
    problem; a lone -inf is weight 0; rows beyond counts are NaN and never read"""
    p = ref.make_case(ref.CASES[2])                                           # P = 5, K = 3, counts (M, partial, 0), weighted
    K, M, S, P = p["K"], p["M"], p["S"], p["P"]
    args = lambda **kw: [dict(p, **kw)[n] for n in ("A", "y", "offset", "counts", "X", "lw")]      # noqa: E731
    clean = p["want"]
    same = lambda g, c: np.array_equal(g, c, equal_nan=True)                  # noqa: E731
    for j, v in ((0, np.inf), (P - 1, np.nan), (P, np.nan), (P, 710.0), (P, -746.0), (P, -np.inf)):
        X = p["X"].copy()
        X[0, 7, j] = v
        lw = p["lw"].copy()
        lw[0, 7] = -np.inf                                                    # weight 0 does not hide the draw
        got = ref.predict(*args(X=X, lw=lw))
        assert np.isnan(got[0][0]).all() and np.isnan(got[1][0]).all(), (j, v)
        assert all(same(g[1:], c[1:]) for g, c in zip(got, clean))
    for v in (709.0, -708.0):                                                 # e^theta is still a positive normal number
        X = p["X"].copy()
        X[0, 7, P] = v
        got = ref.predict(*args(X=X))
        assert np.isfinite(got[0][0].astype(np.float64)).all() and np.isfinite(got[1][0].astype(np.float64)).all()
    A, o = p["A"].copy(), p["offset"].copy()
    A[0, 3, 1] = np.nan
    o[0, 5] = np.inf
    A[1, M - 1, 0] = np.nan                                                   # beyond counts[1]: never read
    got = ref.predict(*args(A=A, offset=o))
    assert np.isnan(got[0][0, [3, 5]]).all() and np.isnan(got[1][0, [3, 5]]).all()
    keep = ~np.isin(np.arange(M), (3, 5))
    assert same(got[0][0, keep], clean[0][0, keep]) and same(got[1][0, keep], clean[1][0, keep])
    assert all(same(g[1:], c[1:]) for g, c in zip(got, clean))
    for v in (np.nan, np.inf):
        lw = p["lw"].copy()
        lw[1, 5] = v
        got = ref.predict(*args(lw=lw))
        assert np.isnan(got[0][1]).all() and np.isnan(got[1][1]).all() and same(got[0][0], clean[0][0])
    lw = p["lw"].copy()
    lw[1, :] = -np.inf
    lw[0, 5] = -np.inf                                                        # a lone -inf: weight 0
    got = ref.predict(*args(lw=lw))
    assert np.isnan(got[0][1]).all() and np.isfinite(got[0][0].astype(np.float64)).all() and np.isfinite(got[1][0].astype(np.float64)).all()
    keep = np.arange(S) != 5
    sub = ref.predict(p["A"][:1], p["y"][:1], p["offset"][:1], None, p["X"][:1, keep], p["lw"][:1, keep])
    assert np.abs(got[0][0] - sub[0][0]).max() <= 1e-15 and np.abs(got[1][0] - sub[1][0]).max() <= 1e-15
    assert p["counts"][2] == 0 and np.isnan(clean[0][2]).all() and np.isnan(clean[1][2]).all()
    bare, none = ref.predict(p["A"], None, p["offset"], p["counts"], p["X"], p["lw"])
    assert none is None and same(bare, clean[0])


def test_log_moments_do_not_overflow_at_large_predictors():
    """eta near 1000 at every draw: the log moments are about 1000 and 2000 where e^eta is inf, and a count of 3 at eta near -800
    keeps a finite lpd (about 3 x -800) where the log of a linear-space sum is -inf"""
    A = np.array([[[1.0]]])
    th = np.full((1, 8, 1), 1.0)
    X = np.concatenate([1000.0 + 0.1 * np.arange(8.0).reshape(1, 8, 1), th], axis=2)
    lmom, _ = ref.predict(A, None, None, None, X, None)
    assert 1000.0 < float(lmom[0, 0, 0]) < 1001.0 and 2000.0 < float(lmom[0, 0, 1]) < 2002.0 and 1999.0 < float(lmom[0, 0, 2]) < 2001.0
    m, v = ref.variance(np.asarray(lmom, dtype=np.float64))
    assert m[0, 0] == np.inf and float(lmom[0, 0, 0]) > ref.LOG_DBL_MAX
    X = np.concatenate([-800.0 + 0.1 * np.arange(8.0).reshape(1, 8, 1), th], axis=2)
    _, lpd = ref.predict(A, np.array([[3.0]]), None, None, X, None)
    assert -2410.0 < float(lpd[0, 0]) < -2390.0
