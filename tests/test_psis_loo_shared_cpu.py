"""The shared-design PSIS leave-one-out without a GPU: the float64 noise floor of the restatement (tests/psis_loo_shared_ref.py) on
the GPU tests' inputs, its equality with psis_loo_ref where the weights say nothing new, the weighted conjugate Gaussian model
against its closed form, the host logic of ``psis_loo_shared_batched`` on a stand-in engine, and the argument checks of the C ABI
on the loaded library without a context."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import glm_batched_ref as gref
import psis_batched_ref as pref
import psis_loo_ref as lref
import psis_loo_shared_ref as ref
import shared_glm_ref as sref

NAMES = ("elpd", "lpd", "khat", "ess")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the noise floor and the cases ----------------------------------------------------------------------------------------------
def test_float64_noise_floor_of_the_restatement_on_the_gpu_inputs():
    """the restatement in float64 against itself in longdouble on every case of the GPU tests (both fed the float64 l_si),
    relative to max(1, |value|), NO row left out: the two precisions agree on every verdict (122 x info 0, 8 x info -2, 100 rows
    not valid); measured 1.42e-14 at the most (ess); l_si itself differs by 1.6e-15.  The GPU bar is 1000 times the recorded
    floor."""
    worst, verdicts = {}, {}
    for c in ref.CASES:
        p = ref.make_case(c)
        args = (p["family"], p["A"], p["y"], p["offset"], p["weights"], p["tau"], p["X"])
        ell = np.asarray(ref.loglik(*args, np.float64), dtype=np.float64)
        worst["loglik"] = max(worst.get("loglik", 0.0), pref.rel_gap(ell, ref.loglik(*args)))
        a = ref.loo_batched(ell, p["logr"], p["lw"], p["weights"], np.float64)
        b = ref.loo_batched(ell, p["logr"], p["lw"], p["weights"])
        assert np.array_equal(a["info"], b["info"]), ref.case_id(c)             # a flip: change the seed, do not exclude the row
        assert np.array_equal(b["info"] != -3, ref.valid_mask(p["weights"], p["K"], p["N"]))
        for v in np.unique(b["info"]):
            verdicts[int(v)] = verdicts.get(int(v), 0) + int((b["info"] == v).sum())
        for n in NAMES:
            worst[n] = max(worst.get(n, 0.0), ref.rel_gap(a[n], b[n]))
    print("float64 against longdouble:", {n: f"{g:.2e}" for n, g in worst.items()}, "; verdicts", verdicts)
    assert set(verdicts) == {0, -2, -3} and verdicts[0] > 100 and verdicts[-2] >= 1
    assert worst.pop("loglik") <= 1e-13
    floor = max(worst.values())
    assert floor <= ref.NOISE_FLOOR <= 2.0 * floor                            # the recorded floor is the measured one, rounded up
    assert ref.BAR == 1000 * ref.NOISE_FLOOR and ref.BAR < 1e-8 and ref.LOGLIK_BAR == 1e-11


def test_the_cases_are_those_of_the_glm_launch_on_one_design():
    assert ref.CASES is lref.CASES
    seen = set()
    for c in ref.CASES:
        p, b = ref.make_case(c), lref.make_case(c)
        assert p["A"].shape == (p["N"], p["D"]) and np.array_equal(p["A"], b["A"][0]) and p["X"] is b["X"]
        w = p["weights"]
        if p["K"] == 1:
            assert w is None
            continue
        assert set(np.unique(w)) <= set(ref.WEIGHT_VALUES) and (w[0] == 0).all() and (w == 2.5).any()
        seen |= set(np.unique(w))
        dead = w == 0
        assert np.isnan(p["y"][dead]).any() and (p["offset"] is None or np.isposinf(p["offset"][dead]).any())
        assert np.isfinite(p["y"][~dead]).all() and np.isfinite(p["logr"]).all()
        if p["N"] >= 3:                                                         # the valid rows are no prefix
            assert w[2, 0] > 0 and w[2, 1] == 0 and w[2, -1] > 0
    assert seen == set(ref.WEIGHT_VALUES)


# ---- 2. where the weights say nothing new: psis_loo_ref exactly ---------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in lref.CASES if c[3] <= 257], ids=lref.case_id)
def test_no_weights_unit_weights_and_a_prefix_mask_are_the_glm_restatement(case):
    """weights None and all ones against psis_loo_ref.loo_batched on the replicated design, and a prefix 0 / 1 mask against its
    ``counts``: every pointwise output and every summary, bit for bit"""
    b = lref.make_case(case)
    K, N, S = b["K"], b["N"], b["S"]
    A = b["A"][0]
    Ar = sref.replicate(A, K)
    counts = b["counts"]
    ell_glm = np.asarray(lref.loglik(b["family"], Ar, b["y"], b["offset"], None, b["tau"], b["X"], np.float64), dtype=np.float64)
    want = lref.loo_batched(ell_glm, b["logr"], b["lw"], None, np.float64)
    for w in (None, np.ones((K, N))):
        ell = np.asarray(ref.loglik(b["family"], A, b["y"], b["offset"], w, b["tau"], b["X"], np.float64), dtype=np.float64)
        assert np.array_equal(ell, ell_glm)
        got = ref.loo_batched(ell, b["logr"], b["lw"], w, np.float64)
        assert all(np.array_equal(got[n], want[n], equal_nan=True) for n in NAMES + ("info",))
        s, t = ref.summaries(got, w, S), lref.summaries(want, None, S)
        assert all(np.array_equal(s[n], t[n], equal_nan=True) for n in s)
    nk = lref.valid_rows(counts, K, N)
    w = (np.arange(N)[None, :] < nk[:, None]).astype(np.float64)
    ell_c = np.asarray(lref.loglik(b["family"], Ar, b["y"], b["offset"], counts, b["tau"], b["X"], np.float64), dtype=np.float64)
    ell = np.asarray(ref.loglik(b["family"], A, b["y"], b["offset"], w, b["tau"], b["X"], np.float64), dtype=np.float64)
    # (numpy's matrix product on the first n_k rows need not round as the one on all N rows does: the l_si agree to the last bits
    # and have the same NaN rows; the stages are then compared on the same l_si)
    assert np.array_equal(np.isnan(ell), np.isnan(ell_c)) and pref.rel_gap(ell, ell_c) <= 1e-14
    got, want = ref.loo_batched(ell, b["logr"], b["lw"], w, np.float64), lref.loo_batched(ell, b["logr"], b["lw"], counts, np.float64)
    assert all(np.array_equal(got[n], want[n], equal_nan=True) for n in NAMES + ("info",))
    s, t = ref.summaries(got, w, S), lref.summaries(want, counts, S)
    assert all(np.array_equal(s[n], t[n], equal_nan=True) for n in s)


# ---- 3. a statistical check with an exact answer -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.GAUSS_SHAPES, ids=lambda s: f"N{s[0]}-D{s[1]}")
def test_elpd_is_the_leave_row_out_density_of_the_weighted_gaussian_model(shape):
    """conjugate Gaussian model with weights from {0, 0.5, 1, 2.5}, q the exact weighted posterior, S = 4096, seeds 0 .. 4: elpd_i
    of the float64 restatement against the closed-form density of one unit observation at row i under the posterior without row
    i's whole weighted term: a Monte-Carlo gap, bounded by twice the recorded largest one"""
    N, D = shape
    gap, khat = [], []
    for seed in ref.GAUSS_SEEDS:
        p = ref.gaussian_exact_problem(N, D, seed)
        ok = p["v"] > 0
        assert set(np.unique(p["v"])) == set(ref.WEIGHT_VALUES)
        r, _ = ref.gaussian_restatement_run(p, ref.GAUSS_S)      # (q is exact: the problem-level ratios are constant to rounding)
        assert (r["info"][ok] == 0).all() and (r["info"][~ok] == -3).all()
        exact = ref.gaussian_exact_loo(p)
        gap.append(np.abs(np.asarray(r["elpd"], dtype=np.float64)[ok] - exact[ok]).max())
        khat.append(float(np.max(np.asarray(r["khat"], dtype=np.float64)[ok])))
        p_loo = float((p["v"][ok] * np.asarray(r["lpd"] - r["elpd"], dtype=np.float64)[ok]).sum())
        assert 0.0 < p_loo < 2.0 * D
    print(f"(N, D) = {shape}: gap {max(gap):.4f} (per seed {np.array2string(np.array(gap), precision=4)}), largest pointwise khat "
          f"{max(khat):.2f}")
    assert abs(max(gap) - ref.GAUSS_GAP[shape]) <= 0.02 * ref.GAUSS_GAP[shape]  # the recorded gap is the measured one
    assert ref.GAUSS_BOUND[shape] == 2.0 * ref.GAUSS_GAP[shape] and max(gap) <= ref.GAUSS_BOUND[shape]


# ---- 4. the surface -------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_exported_and_documented():
    from gsmvi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    name = "gsmvi_psis_loo_shared_batched_f64"
    assert re.search(r"int\s+" + name + r"\(gsmvi_ctx\*", hdr)
    for m in ("exports.map", "exports_debug.map"):
        assert f"    {name};" in open(os.path.join(ROOT, "gsm-vi_amd", "csrc", m)).read(), m
    assert name in _lib._SIGS and hasattr(_lib.load_library(), name)
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_loo"] | HipEngine.PATH_BITS["batched_target"] == ref.PATH_BITS
    assert callable(HipEngine.psis_loo_shared_batched)
    import gsmvi_amd
    assert "psis_loo_shared_batched" in gsmvi_amd.__doc__ and "psis_loo_shared_batched" in gsmvi_amd.SharedDesignGLMTarget.__doc__
    assert "c_i = v_ki" in gsmvi_amd.LOOBatchedResult.__doc__                   # the result's docstring states the weighted sums
    assert not any(hasattr(gsmvi_amd.SharedDesignGLMTarget, n) for n in ("loo", "predict", "neg_hessian"))


def test_abi_checks_arguments_before_the_context():
    from gsmvi_amd import _lib
    ref.check_bad_arguments(_lib.load_library())


# ---- 5. host logic on the stand-in engine ------------------------------------------------------------------------------------------
def _fitted(family="poisson", K=4, N=12, D=3, seed=5, weights=True):
    import gsmvi_amd
    A, y, offset, w, lam, tau, _ = sref.make_inputs(family, K, N, D, 1, seed=seed, poison=True)
    w[1] = 0.0                                                                  # n_k = 0
    w[2] = 0.0
    w[2, 4] = 1.5                                                               # n_k = 1
    y[w == 0], offset[w == 0] = np.nan, np.inf
    if not weights:
        w = None
        y, offset = np.where(np.isfinite(y), y, 0.0), np.where(np.isfinite(offset), offset, 0.0)
    eng = ref.StandInEngine()
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, family, lam + 0.5, offset=offset, weights=w, noise_precision=tau, engine=eng)
    rs = np.random.default_rng(seed)
    mean = 0.3 * rs.standard_normal((K, D))
    G = rs.standard_normal((K, D, D))
    cov = np.linalg.inv(np.eye(D)[None] + 0.3 * G @ np.swapaxes(G, 1, 2))
    return tgt, eng, mean, 0.5 * (cov + np.swapaxes(cov, 1, 2)), A, y, offset, w, tau


def test_psis_loo_shared_batched_protocol_and_weighted_summaries():
    import gsmvi_amd
    tgt, eng, mean, cov, A, y, offset, w, tau = _fitted()
    K, N, D, S = 4, 12, 3, 40
    keys = [5, 6, 7, 8]
    m0, c0 = mean.copy(), cov.copy()
    eng.calls.clear()
    r = gsmvi_amd.psis_loo_shared_batched(tgt, mean, cov, keys, num_draws=S, call=2, pointwise_loglik=True)
    assert isinstance(r, gsmvi_amd.LOOBatchedResult) and r.nlaunch == 3 and r.threshold == pref.threshold(S)
    assert np.array_equal(mean, m0) and np.array_equal(cov, c0)
    launches = [c for c in eng.calls if isinstance(c, tuple)]
    seeds = tuple((k % 2 ** 32) ^ 0x5DEECE66D for k in keys)
    assert launches == [("draw", seeds, 2, 0, S), ("glm_shared", "poisson", "lp"), ("psis", (K, S, D), False),
                        ("loo_shared", "poisson", (K, S, D), (N, D), True, True, True)]
    top = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, call=2, moments=False, engine=ref.StandInEngine())
    assert np.array_equal(r.psis.khat, top.khat) and np.array_equal(r.psis.samples, top.samples)
    ell = np.asarray(ref.loglik("poisson", A, y, offset, w, tau, top.samples), dtype=np.float64)
    want = ref.loo_batched(ell, top.log_ratios, top.log_weights, w)
    assert np.array_equal(r.loglik, ell, equal_nan=True) and r.loglik.shape == (K, N, S)
    for got, n in ((r.elpd_i, "elpd"), (r.lpd_i, "lpd"), (r.khat, "khat"), (r.ess, "ess")):
        assert isinstance(got, np.ndarray) and np.array_equal(got, np.asarray(want[n], dtype=np.float64), equal_nan=True), n
    assert np.array_equal(r.info, want["info"]) and r.info.dtype == np.int64
    assert np.array_equal(r.info == -3, ~(w > 0)) and (r.info[w > 0] != -1).all()
    # the per-problem summaries are the weighted ones, over the rows of weight > 0
    s = ref.summaries(want, w, S)
    for n in ("elpd_loo", "p_loo", "se"):
        assert np.allclose(getattr(r, n), s[n], rtol=1e-13, atol=0, equal_nan=True), n
    ok = w[0] > 0
    c = w[0, ok] * r.elpd_i[0, ok]
    assert np.isclose(r.elpd_loo[0], c.sum(), rtol=1e-13) and np.isclose(r.se[0], np.sqrt(ok.sum() * c.var(ddof=1)), rtol=1e-12)
    assert np.isclose(r.p_loo[0], (w[0, ok] * (r.lpd_i[0, ok] - r.elpd_i[0, ok])).sum(), rtol=1e-11)
    assert not np.isclose(r.elpd_loo[0], r.elpd_i[0, ok].sum(), rtol=1e-3)    # (the weights matter)
    assert r.elpd_loo[1] == 0.0 and r.p_loo[1] == 0.0 and np.isnan(r.se[1]) and r.n_bad[1] == 0       # n_k = 0
    assert r.elpd_loo[2] == 1.5 * r.elpd_i[2, 4] and np.isnan(r.se[2])                                  # n_k = 1
    assert np.array_equal(r.n_bad, s["n_bad"])
    assert np.array_equal(r.ok, np.asarray(r.psis.ok) & (r.n_bad == 0)) and r.ok.dtype == bool
    # psis= reuses the draws: one launch, the same numbers; no pointwise block unless asked for
    eng.calls.clear()
    again = gsmvi_amd.psis_loo_shared_batched(tgt, mean, cov, keys, psis=r.psis)
    assert [c[0] for c in eng.calls if isinstance(c, tuple)] == ["loo_shared"] and again.nlaunch == 1 and again.loglik is None
    for n in ("elpd_loo", "p_loo", "se", "elpd_i", "lpd_i", "khat", "ess", "info", "n_bad", "ok"):
        assert np.array_equal(getattr(again, n), getattr(r, n), equal_nan=True), n
    assert not any(hasattr(tgt, name) for name in ("neg_hessian", "predict", "loo", "counts"))


@pytest.mark.parametrize("family", ("logistic", "gaussian"))
def test_without_weights_the_result_is_psis_loo_batched_on_the_replicated_target(family):
    """weights None, and 0 / 1 weights forming a prefix against ``counts``: every field of the result equals psis_loo_batched's on
    the K-fold replicated BatchedGLMTarget with the same ``psis=``, bit for bit (both on stand-in engines)"""
    import gsmvi_amd
    tgt, eng, mean, cov, A, y, offset, _, tau = _fitted(family, weights=False)
    K, N = tgt.K, tgt.N
    keys = [1, 2, 3, 4]
    r = gsmvi_amd.psis_loo_shared_batched(tgt, mean, cov, keys, num_draws=33)
    lam = np.asarray(tgt.prior_precision)
    rep = gsmvi_amd.BatchedGLMTarget(sref.replicate(A, K), y, family, lam, offset=offset, noise_precision=tau,
                                     engine=lref.StandInEngine())
    q = gsmvi_amd.psis_loo_batched(rep, mean, cov, keys, psis=r.psis)
    fields = ("elpd_loo", "p_loo", "se", "elpd_i", "lpd_i", "khat", "ess", "info", "n_bad", "ok")
    for n in fields:
        assert np.array_equal(getattr(q, n), getattr(r, n), equal_nan=True), n
    counts = np.array([N, 0, 1, 7])
    w = (np.arange(N)[None, :] < counts[:, None]).astype(np.float64)
    tw = gsmvi_amd.SharedDesignGLMTarget(A, y, family, lam, offset=offset, weights=w, noise_precision=tau, engine=ref.StandInEngine())
    tc = gsmvi_amd.BatchedGLMTarget(sref.replicate(A, K), y, family, lam, offset=offset, counts=counts, noise_precision=tau,
                                    engine=lref.StandInEngine())
    rw = gsmvi_amd.psis_loo_shared_batched(tw, mean, cov, keys, num_draws=33)
    rc = gsmvi_amd.psis_loo_batched(tc, mean, cov, keys, psis=rw.psis)
    for n in fields:
        assert np.array_equal(getattr(rc, n), getattr(rw, n), equal_nan=True), n
    assert np.isnan(rw.se[1]) and np.isnan(rw.se[2]) and np.isfinite(rw.se[[0, 3]]).all()


def test_type_and_argument_errors_come_before_any_engine_call():
    import gsmvi_amd
    tgt, eng, mean, cov, A, y, offset, w, tau = _fitted()
    keys = [1, 2, 3, 4]
    Ag, yg, og, _, _, tg, _ = gref.make_inputs("poisson", 4, 12, 3, 1, seed=3)
    glm = gsmvi_amd.BatchedGLMTarget(Ag, yg, "poisson", 1.0, offset=og, noise_precision=tg, engine=lref.StandInEngine())
    logit = gsmvi_amd.BatchedLogisticTarget(Ag, (yg > 0).astype(np.float64), 1.0, engine=lref.StandInEngine())
    gauss = gsmvi_amd.BatchedGaussianTarget(np.zeros((4, 3)), cov=np.stack([np.eye(3)] * 4), engine=lref.StandInEngine())
    eng.calls.clear()
    for bad in (glm, logit, gauss, tgt.lp, gsmvi_amd.psis_batched, None):
        with pytest.raises(TypeError, match="psis_loo_shared_batched: target must be a SharedDesignGLMTarget"):
            gsmvi_amd.psis_loo_shared_batched(bad, mean, cov, keys)
    # psis_loo_batched still refuses the shared class, and now names the function that takes it
    with pytest.raises(TypeError, match=r"BatchedGLMTarget.*SharedDesignGLMTarget.*psis_loo_shared_batched"):
        gsmvi_amd.psis_loo_batched(tgt, mean, cov, keys)
    with pytest.raises(TypeError, match="BatchedGLMTarget") as ei:
        gsmvi_amd.psis_loo_batched(gauss, mean, cov, keys)
    assert "psis_loo_shared_batched" not in str(ei.value)
    loo = lambda *a, **kw: gsmvi_amd.psis_loo_shared_batched(tgt, *a, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="psis_loo_shared_batched: mean must be"):
        loo(mean[:, :2], cov, keys)
    with pytest.raises(ValueError, match="mean must be"):
        loo(mean[:2], cov, keys)
    with pytest.raises(ValueError, match="cov must be"):
        loo(mean, cov[:, :2], keys)
    with pytest.raises(ValueError, match="keys"):
        loo(mean, cov, [1, 2])
    for S in (4, 4097, 0, 10.5):
        with pytest.raises(ValueError, match="num_draws"):
            loo(mean, cov, keys, num_draws=S)
    with pytest.raises(ValueError, match="PSISBatchedResult"):
        loo(mean, cov, keys, psis=dict(samples=None))
    wts = gsmvi_amd.psis_weights_batched(np.zeros((4, 8)), engine=ref.StandInEngine())
    with pytest.raises(ValueError, match="samples"):                           # the weights entry keeps no draws
        loo(mean, cov, keys, psis=wts)
    assert not any(isinstance(c, tuple) for c in eng.calls)
    good = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=8, moments=False, engine=ref.StandInEngine())
    eng.calls.clear()                                                          # (tgt.lp went through the target's engine)
    with pytest.raises(ValueError, match="log_weights"):
        loo(mean, cov, keys, psis=dataclasses.replace(good, log_weights=None))
    with pytest.raises(ValueError, match=r"psis.samples must be"):
        loo(mean, cov, keys, psis=dataclasses.replace(good, samples=good.samples[:, :, :2]))
    with pytest.raises(ValueError, match="log_ratios and psis.log_weights"):
        loo(mean, cov, keys, psis=dataclasses.replace(good, log_ratios=good.log_ratios[:, :5]))
    assert not any(isinstance(c, tuple) for c in eng.calls)

    class Device(ref.StandInEngine):                                           # an engine that works on device tensors
        device = torch.device("cpu")
    with pytest.raises(ValueError, match="samples, log_ratios, log_weights"):  # host copies: as_torch=False results
        gsmvi_amd.psis_loo_shared_batched(tgt, mean, cov, keys, psis=good, engine=Device())
