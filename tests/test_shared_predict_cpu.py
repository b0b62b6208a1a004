"""The shared-design GLM posterior predictive without a GPU: the restatement (tests/shared_predict_ref.py) against
glm_predict_ref where the weights say nothing new, K-fold cross-validation on the conjugate Gaussian model against an independent
route through two marginal likelihoods, the surface (header, export maps, bindings, docstrings), the argument checks of the C ABI
on the loaded library without a context, and the host logic of ``predict_shared_batched`` on a stand-in engine."""
import os
import re

import numpy as np
import pytest

import glm_batched_ref as gref
import glm_predict_ref as gp
import shared_glm_ref as sref
import shared_predict_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("eta_mean", "eta_var", "mean", "lpd", "elpd", "scale_var")


# ---- 1. the restatement where the weights say nothing new ---------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_without_weights_the_restatement_is_glm_predict_ref_on_the_replicated_rows(family):
    """weights None: glm_predict_ref.predict on np.broadcast_to(A, (K, M, D)), every field exactly; all-one weights too; a 0 / 1
    prefix mask equals its ``counts``.  The restatement directly, and ``predict_shared_batched`` on the stand-in engine."""
    import gsmvi_amd
    K, M, D = 5, 37, 6
    p = ref.make_problem(family, K, M, D)
    rep = np.broadcast_to(p["A"], (K, M, D))
    tgt = gsmvi_amd.SharedDesignGLMTarget(p["A"], p["y"], family, offset=p["offset"], noise_precision=p["tau"],
                                          engine=ref.StandInEngine())
    public = lambda off, w: gsmvi_amd.predict_shared_batched(tgt, p["mean"], p["cov"], p["A"], offset=off, y=p["y"],   # noqa: E731
                                                             weights=w)
    for off in (p["offset"], None):
        want = gp.predict(family, rep, off, p["y"], None, p["tau"], p["mean"], p["cov"])
        for w in (None, np.ones((K, M))):
            got = ref.predict(family, p["A"], off, p["y"], w, p["tau"], p["mean"], p["cov"])
            for n in FIELDS:
                assert np.array_equal(got[n], want[n], equal_nan=True), (n, w is None)
            r = public(off, w)
            assert all(np.array_equal(getattr(r, n), want[n], equal_nan=True) for n in ref.NAMES), w is None
        noy = ref.predict(family, p["A"], off, None, None, p["tau"], p["mean"], p["cov"])
        assert noy["lpd"] is None and noy["elpd"] is None
        assert all(np.array_equal(noy[n], want[n]) for n in ("eta_mean", "eta_var", "mean"))
        counts = np.array([M, 0, 1, 32, M - 1], dtype=np.int32)
        mask = (np.arange(M)[None, :] < counts[:, None]).astype(np.float64)
        want = gp.predict(family, rep, off, p["y"], counts, p["tau"], p["mean"], p["cov"])
        got = ref.predict(family, p["A"], off, p["y"], mask, p["tau"], p["mean"], p["cov"])
        for n in FIELDS:
            assert np.array_equal(got[n], want[n], equal_nan=True), n
        assert got["elpd"][1] == 0.0
        r = public(off, mask)
        assert all(np.array_equal(getattr(r, n), want[n], equal_nan=True) for n in ref.NAMES)


def test_the_weight_pattern_and_the_rows_that_are_not_valid():
    """the pattern of the GPU tests: a quarter of the entries exactly 0, problem 1 all zero, rows 0 .. 31 of problem 2 zero; the
    restatement never looks at y or the offset there, the rows are NaN, elpd is the ordered weighted sum and 0 for problem 1"""
    import gsmvi_amd
    K, M, D = 4, 65, 5
    w = ref.weight_pattern(K, M)
    assert (w >= 0).all() and (w < 2).all() and (w == 0).sum() >= (K * M) // 4
    assert (w[1] == 0).all() and (w[2, :32] == 0).all() and (w[2, 32:] > 0).any() and (w[3, :32] > 0).any()
    assert set(ref.SHAPES) and {s[0] for s in ref.SHAPES} == {1, 5, 16, 17, 33, 64}
    assert {s[1] for s in ref.SHAPES} == {1, 31, 32, 33, 65} and {s[2] for s in ref.SHAPES} == {1, 3, 4, 5, 7}
    assert any(s[0] <= 16 and s[1] > 32 and s[2] > 2 for s in ref.SHAPES) and any(s[0] > 16 and s[1] > 32 and s[2] > 2 for s in ref.SHAPES)
    for family in ref.FAMILIES:
        p = ref.make_problem(family, K, M, D)
        v = np.einsum("ni,kij,nj->kn", p["A"], p["cov"], p["A"])
        assert v.max() <= 0.9 * (1 + 1e-12)                                     # the band of the existing predict tests
        clean = ref.predict(family, p["A"], p["offset"], p["y"], w, p["tau"], p["mean"], p["cov"])
        y, o = ref.plant(p["y"], p["offset"], w)
        assert np.isnan(y[w == 0]).all() and np.isinf(o[w == 0]).all()
        got = ref.predict(family, p["A"], o, y, w, p["tau"], p["mean"], p["cov"])
        for n in FIELDS:
            assert np.array_equal(got[n], clean[n], equal_nan=True), n
        # the public function accepts the planted y and offset under the zero weights and returns the same numbers
        tgt = gsmvi_amd.SharedDesignGLMTarget(p["A"], p["y"], family, noise_precision=p["tau"], engine=ref.StandInEngine())
        r = gsmvi_amd.predict_shared_batched(tgt, p["mean"], p["cov"], tgt.A, offset=o, y=y, weights=w)
        assert all(np.array_equal(getattr(r, n), clean[n], equal_nan=True) for n in ref.NAMES)
        for n in ("eta_mean", "eta_var", "mean", "lpd"):
            assert np.isnan(got[n][w == 0]).all() and np.isfinite(got[n][w > 0]).all(), n
        assert got["elpd"][1] == 0.0
        for k in range(K):
            s = np.longdouble(0)
            for m in np.flatnonzero(w[k] > 0):
                s = s + np.longdouble(w[k, m]) * np.longdouble(got["lpd"][k, m])
            assert abs(got["elpd"][k] - float(s)) <= 1e-13 * max(1.0, got["scale_elpd"][k]), k
        # the unweighted rows are those of the unweighted call: lpd is the density of one unit observation
        plain = ref.predict(family, p["A"], p["offset"], p["y"], None, p["tau"], p["mean"], p["cov"])
        assert np.array_equal(got["lpd"][w > 0], plain["lpd"][w > 0])


# ---- 2. K-fold cross-validation on the conjugate Gaussian model ----------------------------------------------------------------------
def test_kfold_heldout_density_of_the_conjugate_gaussian_model():
    """(N, D, F) = (24, 5, 4), three (lam, tau) pairs, five seeds: with the closed-form posterior of every fold's training rows the
    restatement's lpd on the held-out rows is log p(y_train, y_m) - log p(y_train) from the two marginal likelihoods
    (scipy.stats.multivariate_normal), 1e-11 relative to max(1, |value|) (measured for exactly these inputs: 1.8e-14); elpd is the
    weighted ordered sum"""
    import gsmvi_amd
    c = ref.KFOLD
    worst = 0.0
    for lam, tau in c["pairs"]:
        for seed in c["seeds"]:
            A, y, mask, mean, cov = ref.kfold_gaussian_problem(c["N"], c["D"], c["F"], lam, tau, seed)
            assert (mask.sum(0) == 1.0).all() and (mask.sum(1) == c["N"] // c["F"]).all()
            Y = np.broadcast_to(y, mask.shape)
            got = ref.predict("gaussian", A, None, Y, mask, tau, mean, cov)
            want = ref.kfold_gaussian_heldout(A, y, mask, lam, tau)
            # the same through the public function: the fold's target carries the training weights, the call the fold masks
            tgt = gsmvi_amd.SharedDesignGLMTarget(A, Y, "gaussian", lam, weights=1.0 - mask, noise_precision=tau,
                                                  engine=ref.StandInEngine())
            r = gsmvi_amd.predict_shared_batched(tgt, mean, cov, tgt.A, y=Y, weights=mask)
            assert np.array_equal(r.lpd, got["lpd"], equal_nan=True) and np.array_equal(r.elpd, got["elpd"])
            worst = max(worst, ref.rel(r.lpd, want))
            assert np.array_equal(np.isnan(got["lpd"]), mask == 0.0) and np.array_equal(np.isnan(want), mask == 0.0)
            worst = max(worst, ref.rel(got["lpd"], want))
            for f in range(c["F"]):
                s = np.longdouble(0)
                for m in np.flatnonzero(mask[f] > 0):
                    s = s + np.longdouble(got["lpd"][f, m])
                assert abs(got["elpd"][f] - float(s)) <= 1e-14 * max(1.0, abs(float(s)))
            # a weight other than 1 scales the row's term of elpd and leaves lpd alone
            w2 = 0.5 * mask
            half = ref.predict("gaussian", A, None, Y, w2, tau, mean, cov)
            assert np.array_equal(half["lpd"], got["lpd"], equal_nan=True)
            assert np.allclose(half["elpd"], 0.5 * got["elpd"], rtol=1e-14, atol=0)
    print(f"K-fold held-out density against the marginal likelihoods: worst {worst:.2e}")
    assert worst <= 1e-11, worst


# ---- 3. the surface -------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_exported_and_documented():
    from gsmvi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    name = "gsmvi_glm_shared_predict_batched_f64"
    assert re.search(r"int\s+" + name + r"\(gsmvi_ctx\*", hdr)
    for m in ("exports.map", "exports_debug.map"):
        assert f"    {name};" in open(os.path.join(ROOT, "gsm-vi_amd", "csrc", m)).read(), m
    assert name in _lib._SIGS and hasattr(_lib.load_library(), name)
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_predict"] | HipEngine.PATH_BITS["batched_target"] == ref.PATH_BITS
    assert callable(HipEngine.glm_shared_predict_batched)
    import gsmvi_amd
    assert callable(gsmvi_amd.predict_shared_batched) and gsmvi_amd.predict_shared_batched is gsmvi_amd.targets.predict_shared_batched
    assert "predict_shared_batched" in gsmvi_amd.__doc__ and "predict_shared_batched" in gsmvi_amd.SharedDesignGLMTarget.__doc__
    assert "stays absent" not in gsmvi_amd.SharedDesignGLMTarget.__doc__
    assert not hasattr(gsmvi_amd.SharedDesignGLMTarget, "predict")              # a function, not a method
    # the row stage both predict kernels run: the link is called, not restated, and both kernels include that one copy
    csrc = os.path.join(ROOT, "gsm-vi_amd", "csrc")
    stage = open(os.path.join(csrc, "gsmvi_glm_predict_stage.h")).read()
    assert "lb_link<" in stage and "erfcx" not in stage and "log1p" not in stage
    for f in ("gsmvi_glm_predict_batched.hip", "gsmvi_glm_shared_predict_batched.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "gsmvi_glm_predict_stage.h"' in src and "gp_row_stage<NT, FAM," in src, f
        assert "erfcx" not in src and "log1p" not in src, f


def test_abi_checks_arguments_before_the_context():
    from gsmvi_amd import _lib
    ref.check_bad_arguments(_lib.load_library())


# ---- 4. host logic on the stand-in engine ------------------------------------------------------------------------------------------
def _fitted(family="poisson", K=4, N=12, D=3, seed=5):
    import gsmvi_amd
    A, y, offset, w, lam, tau, _ = sref.make_inputs(family, K, N, D, 1, seed=seed, poison=True)
    y, offset = np.where(np.isfinite(y), y, 0.0), np.where(np.isfinite(offset), offset, 0.0)
    eng = ref.StandInEngine()
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, family, lam + 0.5, offset=offset, noise_precision=tau, engine=eng)
    rs = np.random.default_rng(seed)
    mean = 0.3 * rs.standard_normal((K, D))
    G = rs.standard_normal((K, D, D))
    cov = np.linalg.inv(np.eye(D)[None] + 0.3 * G @ np.swapaxes(G, 1, 2))
    return tgt, eng, mean, 0.5 * (cov + np.swapaxes(cov, 1, 2)), A, y, offset, tau


@pytest.mark.parametrize("family", ("poisson", "gaussian"))
def test_predict_shared_batched_protocol(family):
    import gsmvi_amd
    tgt, eng, mean, cov, A, y, offset, tau = _fitted(family)
    K, N, D = tgt.K, tgt.N, tgt.D
    w = ref.weight_pattern(K, N)
    w[0, 0] = 0.0
    yp, op = ref.plant(y, offset, w)                                            # y = NaN, offset = +inf under every zero weight
    m0, c0 = mean.copy(), cov.copy()
    eng.calls.clear()
    r = gsmvi_amd.predict_shared_batched(tgt, mean, cov, tgt.A, offset=op, y=yp, weights=w)
    assert [c for c in eng.calls if isinstance(c, tuple)] == [("shared_predict", family, (N, D), True, True, True, 32)]
    assert np.array_equal(mean, m0) and np.array_equal(cov, c0)
    assert isinstance(r, gsmvi_amd.GLMPrediction) and all(isinstance(getattr(r, n), np.ndarray) for n in ref.NAMES)
    want = ref.predict(family, A, op, yp, w, tau, mean, cov)
    assert all(np.array_equal(getattr(r, n), want[n], equal_nan=True) for n in ref.NAMES)
    assert np.isnan(r.lpd[w == 0]).all() and np.isfinite(r.lpd[w > 0]).all() and r.elpd[1] == 0.0
    # new rows, no y, no offset, no weights, another Q
    An = A[:5] + 0.1
    eng.calls.clear()
    r2 = gsmvi_amd.predict_shared_batched(tgt, mean, cov, An, nodes=16)
    assert [c for c in eng.calls if isinstance(c, tuple)] == [("shared_predict", family, (5, D), False, False, False, 16)]
    assert r2.lpd is None and r2.elpd is None and r2.mean.shape == (K, 5) and np.isfinite(r2.mean).all()
    # without weights: BatchedGLMTarget.predict on the replicated rows, every field
    rep = gsmvi_amd.BatchedGLMTarget(sref.replicate(A, K), y, family, 1.0, offset=offset, noise_precision=tau,
                                     engine=gp.StandInEngine())
    a = rep.predict(mean, cov, sref.replicate(A, K), offset=offset, y=y)
    b = gsmvi_amd.predict_shared_batched(tgt, mean, cov, A, offset=offset, y=y)
    assert all(np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True) for n in ref.NAMES)
    # an engine of the caller's
    other = ref.StandInEngine()
    gsmvi_amd.predict_shared_batched(tgt, mean, cov, A, engine=other)
    assert [c[0] for c in other.calls if isinstance(c, tuple)] == ["shared_predict"]


def test_type_and_argument_errors_come_before_any_engine_call():
    import gsmvi_amd
    tgt, eng, mean, cov, A, y, offset, tau = _fitted()
    K, N, D = tgt.K, tgt.N, tgt.D
    Ag, yg, og, _, _, tg, _ = gref.make_inputs("poisson", 4, 12, 3, 1, seed=3)
    glm = gsmvi_amd.BatchedGLMTarget(Ag, yg, "poisson", 1.0, offset=og, noise_precision=tg, engine=gp.StandInEngine())
    eng.calls.clear()
    for bad in (glm, tgt.lp, None):
        with pytest.raises(TypeError, match=r"predict_shared_batched: target must be a SharedDesignGLMTarget.*BatchedGLMTarget\.predict"):
            gsmvi_amd.predict_shared_batched(bad, mean, cov, A)
    ps = lambda *a, **kw: gsmvi_amd.predict_shared_batched(tgt, *a, **kw)     # noqa: E731
    w = np.ones((K, N))
    w[2, 3] = 0.0
    ybad = y.copy()
    ybad[2, 3] = np.nan
    assert np.isfinite(ps(mean, cov, A, y=ybad, weights=w).elpd).all()          # y = NaN under a zero weight is accepted
    with pytest.raises(ValueError, match=r"^y: .*problems \[2\]"):
        ps(mean, cov, A, y=ybad)                                                # ... and refused under a positive one
    with pytest.raises(ValueError, match=r"^y: .*problems \[2\]"):
        ps(mean, cov, A, y=ybad, weights=2.0 * np.ones((K, N)))
    obad = offset.copy()
    obad[1, 0] = np.inf
    with pytest.raises(ValueError, match=r"^offset: non-finite.*problems \[1\]"):
        ps(mean, cov, A, offset=obad)
    w0 = np.ones((K, N))
    w0[1, 0] = 0.0
    assert np.isfinite(ps(mean, cov, A, offset=obad, weights=w0).mean[1, 1:]).all()
    for wbad in (-w, np.where(w == 0, np.nan, w), np.full((K, N), np.inf)):
        with pytest.raises(ValueError, match="^weights: negative or non-finite"):
            ps(mean, cov, A, weights=wbad)
    with pytest.raises(ValueError, match=r"^weights: expected shape \(K, M\)"):
        ps(mean, cov, A, weights=w[:, :-1])
    with pytest.raises(ValueError, match=r"^weights: expected shape \(K, M\)"):
        ps(mean, cov, A, weights=w[0])
    with pytest.raises(ValueError, match=r"^weights: expected shape \(K, N\)"):      # the constructor's message is unchanged
        gsmvi_amd.SharedDesignGLMTarget(A, y, "poisson", weights=w[:, :-1], engine=eng)
    for nodes in (65, 0, 2.0, True):
        with pytest.raises(ValueError, match="^nodes:"):
            ps(mean, cov, A, nodes=nodes)
    with pytest.raises(ValueError, match="^A_new:"):
        ps(mean, cov, sref.replicate(A, K))
    with pytest.raises(ValueError, match="^A_new:"):
        ps(mean, cov, A[:, :2])
    with pytest.raises(ValueError, match="^mean:"):
        ps(mean[:2], cov, A)
    with pytest.raises(ValueError, match="^cov:"):
        ps(mean, cov[:, :2], A)
    with pytest.raises(ValueError, match=r"^y: expected shape \(K, M\)"):
        ps(mean, cov, A, y=y[:, :-1])
    with pytest.raises(ValueError, match=r"^offset: expected shape \(K, M\)"):
        ps(mean, cov, A, offset=offset[:, :-1])
    launched = [c for c in eng.calls if isinstance(c, tuple)]
    assert [c[0] for c in launched] == ["shared_predict", "shared_predict"]     # the two accepted calls and nothing else
