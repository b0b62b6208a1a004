"""The batched softmax posterior predictive without a GPU: the C ABI declarations, bindings and argument checks through the built
library; the LDS bound over every legal (C, P); the host logic of ``predict_softmax_batched`` on a stand-in engine; the properties of
the restatement (tests/softmax_predict_ref.py): rows of prob sum to one, two classes are the weighted mean of the sigmoid, the NaN
rules, and the Monte-Carlo mean against E_q[softmax] by tensor Gauss-Hermite quadrature."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import glm_batched_ref as gref
import psis_loo_ref as lref
import softmax_predict_ref as ref
from gsmvi_amd import predict_softmax_batched      # noqa: F401  (the feature: without it nothing here can pass)
from gsmvi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsmvi_softmax_predict_batched_f64"
LDSFN = "gsmvi_softmax_predict_lds_bytes"


# ---- 1. declaration, binding, argument checks, the LDS bound -----------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name, nargs in ((NAME, 14), (LDSFN, 2)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        for mp in ("exports.map", "exports_debug.map"):
            assert re.search(r"^\s*" + name + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), (mp, name)
        assert name in _lib.exported_symbols() and name in built, name
        res, args = _lib._SIGS[name]
        decl = re.search(r"int\s+" + name + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert res is C.c_int and len(args) == len(params) == nargs
        for p, a in zip(params, args):
            want = C.c_int64 if p.startswith("int64_t") else C.c_int if p.startswith("int ") else \
                C.c_double if p.startswith("double ") else C.c_void_p
            assert a is want, (p, a)
    assert NAME in hdr.split("#ifndef GSMVI_HIP_H")[0] and LDSFN in hdr.split("#ifndef GSMVI_HIP_H")[0]      # the mapping list
    block = hdr[:hdr.index("int " + LDSFN)].rsplit("/*", 1)[1]                 # the definition is written above the entry point
    for line in ("eta_sic = a_i . x_s[c P .. c P + P - 1]  (c < C - 1),   eta_si,C-1 = 0",
                 "m_si    = max_c eta_sic   (all C values, the 0 included)",
                 "z_si    = sum_{c = 0 .. C-1} exp(eta_sic - m_si)   (class order, the reference class last)",
                 "p_sic   = exp(eta_sic - m_si) / z_si",
                 "prob[k, i, c] = sum_s w_s p_sic,   w_s = exp(lw_s)",
                 "l_si    = eta_si,y_i - m_si - log z_si",
                 "lpd[k, i]     = log sum_s exp(lw_s + l_si)",
                 "GSMVI_PATH_BATCHED_PREDICT |",
                 "GSMVI_PATH_BATCHED_SOFTMAX: after a reset exactly that pair identifies this launch"):
        assert line in block, line
    # no new path bit, the word is not widened, the ABI version stays
    assert len(re.findall(r"#define\s+GSMVI_PATH_\w+\s+0x[0-9a-fA-F]+u", hdr)) == 32
    assert re.search(r"#define\s+GSMVI_ABI_VERSION\s+1\b", hdr) and _lib.load_library().gsmvi_abi_version() == 1
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_predict"] | HipEngine.PATH_BITS["batched_softmax"] == ref.PATH_BITS
    assert callable(HipEngine.softmax_predict_lds_bytes) and callable(HipEngine.softmax_predict_batched)
    import gsmvi_amd
    assert gsmvi_amd.predict_softmax_batched is not None and "predict_softmax_batched" in gsmvi_amd.__doc__
    assert dataclasses.is_dataclass(gsmvi_amd.SoftmaxPrediction)
    assert "predict_softmax_batched" in gsmvi_amd.BatchedSoftmaxTarget.__doc__


def test_abi_checks_arguments_before_the_context():
    ref.check_bad_arguments(_lib.load_library())


def test_lds_bytes_stay_inside_the_workgroup_limit():
    """every (C, P) with D = (C - 1) P <= 64: the library's value is the header's formula, positive and at most 160 KB; the largest
    is (65, 1), above 64 KB (hence the kernel attribute); 0 outside the bounds"""
    lib = _lib.load_library()
    worst, n = (0, None), 0
    for Cc in range(2, 66):
        for P in range(1, 65):
            if (Cc - 1) * P > 64:
                assert lib.gsmvi_softmax_predict_lds_bytes(Cc, P) == 0 == ref.lds_bytes(Cc, P), (Cc, P)
                continue
            b = lib.gsmvi_softmax_predict_lds_bytes(Cc, P)
            assert b == ref.lds_bytes(Cc, P) and 0 < b <= ref.LDS_MAX and b % 8 == 0, (Cc, P, b)
            worst = max(worst, (b, (Cc, P)))
            n += 1
    assert n == sum(64 // d for d in range(1, 65)) and worst == (69952, (65, 1)) and worst[0] > 64 * 1024
    for Cc, P in ((1, 1), (0, 4), (2, 0), (2, 65), (66, 1), (6, 13), (-1, 3), (3, -1), (2 ** 17, 2 ** 17)):
        assert lib.gsmvi_softmax_predict_lds_bytes(Cc, P) == 0 == ref.lds_bytes(Cc, P), (Cc, P)


# ---- 2. host logic on the stand-in engine ------------------------------------------------------------------------------------------
def _fitted(K=3, N=12, Cc=3, P=2, M=7, seed=3):
    import gsmvi_amd
    rs = np.random.default_rng(seed)
    A = rs.standard_normal((K, N, P))
    W = rs.standard_normal((K, Cc - 1, P))
    y = ref.draw_labels(rs, A, W)
    eng = ref.StandInEngine()
    tgt = gsmvi_amd.BatchedSoftmaxTarget(A, y, Cc, 1.0, engine=eng)
    D = (Cc - 1) * P
    mean = W.reshape(K, D) + 0.1 * rs.standard_normal((K, D))
    G = rs.standard_normal((K, D, D))
    cov = np.linalg.inv(np.eye(D)[None] + 0.3 * G @ np.swapaxes(G, 1, 2))
    A_new = rs.standard_normal((K, M, P))
    y_new = ref.draw_labels(rs, A_new, W)
    return tgt, eng, mean, 0.5 * (cov + np.swapaxes(cov, 1, 2)), A_new, y_new


def _launches(eng):
    return [c for c in eng.calls if isinstance(c, tuple)]


def test_uniform_mode_draws_once_makes_no_lp_call_and_summarises_under_counts():
    import gsmvi_amd
    tgt, eng, mean, cov, A_new, y_new = _fitted()
    K, M, D, S, Cc = 3, 7, 4, 40, 3
    keys = [5, 6, 7]
    cnt = np.array([7, 0, 4])
    m0, c0 = mean.copy(), cov.copy()
    eng.calls.clear()
    r = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, y=y_new, counts=cnt, num_draws=S, call=2)
    assert isinstance(r, gsmvi_amd.SoftmaxPrediction) and r.nlaunch == 2 and r.num_draws == S and r.psis is None
    assert np.array_equal(mean, m0) and np.array_equal(cov, c0)
    seeds = tuple((k % 2 ** 32) ^ 0x5DEECE66D for k in keys)
    assert _launches(eng) == [("draw", seeds, 2, 0, S), ("predict_softmax", Cc, (K, S, D), (K, M, 2), False, True, True)]
    # the draws are psis_batched's for the same keys and call
    top = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, call=2, moments=False, engine=ref.StandInEngine())
    prob, lpd = ref.predict(A_new, y_new, Cc, cnt, top.samples, None)
    assert isinstance(r.prob, np.ndarray) and r.prob.shape == (K, M, Cc) and r.lpd.shape == (K, M) and r.elpd.shape == (K,)
    assert np.array_equal(r.prob, np.asarray(prob, dtype=np.float64), equal_nan=True)
    assert np.array_equal(r.lpd, np.asarray(lpd, dtype=np.float64), equal_nan=True)
    mask = np.arange(M)[None, :] < cnt[:, None]
    assert np.isfinite(r.prob[mask]).all() and np.isnan(r.prob[~mask]).all() and np.isnan(r.lpd[~mask]).all()
    # label: the first maximum, -1 where the row is NaN; elpd: the sum over the valid rows, 0 for a problem without one
    assert r.label.dtype == np.int64 and np.array_equal(r.label[mask], np.argmax(r.prob[mask], axis=1)) and (r.label[~mask] == -1).all()
    want = np.array([r.lpd[k, :cnt[k]].sum() for k in range(K)])
    assert np.allclose(r.elpd, want, rtol=1e-14, atol=0) and r.elpd[1] == 0.0 and (r.elpd[[0, 2]] < 0).all()
    # without y: no lpd, no elpd; without counts every row counts
    eng.calls.clear()
    bare = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, num_draws=S, call=2)
    assert bare.lpd is None and bare.elpd is None and _launches(eng)[-1] == ("predict_softmax", Cc, (K, S, D), (K, M, 2), False, False, False)
    assert np.array_equal(bare.prob[mask], r.prob[mask]) and np.isfinite(bare.prob).all() and (bare.label >= 0).all()
    assert np.abs(bare.prob.sum(2) - 1.0).max() <= 1e-14
    # a tie goes to the first maximum
    tie = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, np.zeros_like(A_new), keys, num_draws=S)
    assert np.array_equal(tie.prob[..., 0], tie.prob[..., 1]) and np.array_equal(tie.prob[..., 0], tie.prob[..., 2])
    assert (tie.label == 0).all()


def test_psis_mode_weights_the_draws_and_psis_is_reused():
    import gsmvi_amd
    tgt, eng, mean, cov, A_new, y_new = _fitted()
    K, M, D, S, Cc = 3, 7, 4, 40, 3
    keys = [5, 6, 7]
    eng.calls.clear()
    r = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, y=y_new, num_draws=S, weights="psis")
    seeds = tuple((k % 2 ** 32) ^ 0x5DEECE66D for k in keys)
    assert _launches(eng) == [("draw", seeds, 0, 0, S), ("softmax", Cc, "lp"), ("psis", (K, S, D), False),
                              ("predict_softmax", Cc, (K, S, D), (K, M, 2), True, True, False)]
    assert r.nlaunch == 3 and isinstance(r.psis, gsmvi_amd.PSISBatchedResult) and r.psis.khat.shape == (K,) and r.psis.mean is None
    prob, lpd = ref.predict(A_new, y_new, Cc, None, r.psis.samples, r.psis.log_weights)
    assert np.array_equal(r.prob, np.asarray(prob, dtype=np.float64)) and np.array_equal(r.lpd, np.asarray(lpd, dtype=np.float64))
    uni = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, y=y_new, num_draws=S)
    assert not np.array_equal(uni.prob, r.prob) and uni.psis is None
    # psis= with "psis": one launch, the same numbers; with "uniform": its samples only
    eng.calls.clear()
    again = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, y=y_new, psis=r.psis, weights="psis", num_draws=7)
    assert [c[0] for c in _launches(eng)] == ["predict_softmax"] and again.nlaunch == 1 and again.num_draws == S
    assert again.psis is r.psis
    for n in ("prob", "label", "lpd", "elpd"):
        assert np.array_equal(getattr(again, n), getattr(r, n)), n
    eng.calls.clear()
    plain = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, y=y_new, psis=r.psis)
    assert _launches(eng) == [("predict_softmax", Cc, (K, S, D), (K, M, 2), False, True, False)] and plain.nlaunch == 1
    for n in ("prob", "label", "lpd", "elpd"):
        assert np.array_equal(getattr(plain, n), getattr(uni, n)), n
    # a problem whose problem-level run failed comes out NaN
    broken = dataclasses.replace(r.psis, log_weights=np.where(np.arange(K)[:, None] == 1, np.nan, r.psis.log_weights))
    b = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, y=y_new, psis=broken, weights="psis")
    assert np.isnan(b.prob[1]).all() and np.isnan(b.lpd[1]).all() and (b.label[1] == -1).all() and np.isnan(b.elpd[1])
    assert np.array_equal(b.prob[[0, 2]], r.prob[[0, 2]]) and np.array_equal(b.elpd[[0, 2]], r.elpd[[0, 2]])
    # torch out
    t = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, y=y_new, psis=r.psis, as_torch=True)
    assert isinstance(t.label, torch.Tensor) and t.label.dtype == torch.int64 and isinstance(t.elpd, torch.Tensor)
    assert np.array_equal(np.asarray(t.label), plain.label) and np.array_equal(np.asarray(t.elpd), plain.elpd)


def test_type_and_argument_errors_come_before_any_engine_call():
    import gsmvi_amd
    tgt, eng, mean, cov, A_new, y_new = _fitted()
    Ag, yg, offset, _, _, tau, _ = gref.make_inputs("logistic", 3, 12, 4, 1, seed=3)
    glm = gsmvi_amd.BatchedGLMTarget(Ag, yg, "logistic", 1.0, offset=offset, noise_precision=tau, engine=lref.StandInEngine())
    eng.calls.clear()
    for bad in (glm, tgt.lp, None):
        with pytest.raises(TypeError, match="BatchedSoftmaxTarget"):
            gsmvi_amd.predict_softmax_batched(bad, mean, cov, A_new, [1, 2, 3])
    with pytest.raises(TypeError, match="predict"):                            # the method keeps its refusal and names the function
        tgt.predict(mean, cov, A_new)
    with pytest.raises(TypeError, match="predict_softmax_batched"):
        tgt.predict(mean, cov, A_new)
    pr = lambda *a, **kw: gsmvi_amd.predict_softmax_batched(tgt, *a, **kw)    # noqa: E731
    keys = [1, 2, 3]
    with pytest.raises(ValueError, match="predict_softmax_batched: A_new"):
        pr(mean, cov, A_new[:, :, :1], keys)
    with pytest.raises(ValueError, match="A_new"):
        pr(mean, cov, A_new[:2], keys)
    with pytest.raises(ValueError, match="A_new"):
        pr(mean, cov, A_new[0], keys)
    with pytest.raises(ValueError, match="mean must be"):
        pr(mean[:, :3], cov, A_new, keys)
    with pytest.raises(ValueError, match="cov must be"):
        pr(mean, cov[:, :3], A_new, keys)
    with pytest.raises(ValueError, match="y: expected shape"):
        pr(mean, cov, A_new, keys, y=y_new[:, :3])
    bad_y = y_new.copy()
    bad_y[2, 1] = 3
    with pytest.raises(ValueError, match=r"y: labels .* problems \[2\]"):
        pr(mean, cov, A_new, keys, y=bad_y)
    assert pr(mean, cov, A_new, keys, y=bad_y, counts=np.array([7, 7, 1]), num_draws=8).lpd.shape == (3, 7)     # beyond counts: ignored
    eng.calls.clear()
    with pytest.raises(ValueError, match="y: expected integer labels"):
        pr(mean, cov, A_new, keys, y=y_new.astype(bool))
    with pytest.raises(ValueError, match=r"counts: values outside 0 \.\. M = 7"):
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
        gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, psis=good, engine=Device())


# ---- 3. properties of the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_rows_of_prob_sum_to_one(case):
    """the valid rows of prob sum to 1 within 1e-14 (longdouble restatement; the weights are normalised to float64 rounding), every
    probability lies in [0, 1], lpd <= 0; rows i >= n_k are NaN"""
    p = ref.make_case(case)
    prob, lpd = ref.predict(p["A"], p["y"], p["C"], p["counts"], p["X"], p["lw"])
    nk = ref.valid_rows(p["counts"], p["K"], p["M"])
    mask = np.arange(p["M"])[None, :] < nk[:, None]
    assert np.abs(prob[mask].sum(1) - 1).max() <= 1e-14 if mask.any() else True
    assert (prob[mask] >= 0).all() and (prob[mask] <= 1).all() and (lpd[mask] <= 0).all() and np.isfinite(lpd[mask].astype(np.float64)).all()
    assert np.isnan(prob[~mask]).all() and np.isnan(lpd[~mask]).all()
    bare, none = ref.predict(p["A"], None, p["C"], p["counts"], p["X"], p["lw"])
    assert none is None and np.array_equal(bare, prob, equal_nan=True)


def test_two_classes_are_the_weighted_mean_of_the_sigmoid():
    """C = 2: prob[..., 0] = sum_s w_s sigmoid(a_i . x_s) and lpd = log sum_s w_s sigmoid(+-eta), within 1e-14"""
    for case in (ref.CASES[0], ref.CASES[6], (2, 3, 33, 5, 1, True)):
        p = ref.make_case(case)
        assert p["C"] == 2 and p["counts"] is None
        prob, lpd = ref.predict(p["A"], p["y"], 2, None, p["X"], p["lw"])
        eta = np.einsum("kmp,ksp->kms", p["A"].astype(ref.LD), p["X"].astype(ref.LD))
        sig = 1 / (1 + np.exp(-eta))
        w = np.full((p["K"], p["S"]), 1 / ref.LD(p["S"])) if p["lw"] is None else np.exp(p["lw"].astype(ref.LD))
        want = np.einsum("ks,kms->km", w, sig)
        assert np.abs(prob[..., 0] - want).max() <= 1e-14 and np.abs(prob[..., 1] - (w.sum(1)[:, None] - want)).max() <= 1e-14
        lik = np.where((p["y"] == 0)[:, :, None], sig, 1 - sig)
        assert np.abs(lpd - np.log(np.einsum("ks,kms->km", w, lik))).max() <= 1e-13


def test_restatement_nan_rules():
    """the rules of the header: a non-finite x entry -> every valid row of its problem; a non-finite a entry -> its row; a NaN or
    +inf in lw, or only -inf -> the problem; a lone -inf is weight 0; a label out of range -> that row's lpd alone"""
    p = ref.make_case(ref.CASES[2])                                           # (3, 5), K = 3, counts (0, partial, M), weighted
    K, M, S = p["K"], p["M"], p["S"]
    args = lambda **kw: [dict(p, **kw)[n] for n in ("A", "y", "C", "counts", "X", "lw")]      # noqa: E731
    clean = ref.predict(*args())
    nk = ref.valid_rows(p["counts"], K, M)
    X = p["X"].copy()
    X[2, 7, 9] = np.inf
    got = ref.predict(*args(X=X))
    assert np.isnan(got[0][2]).all() and np.isnan(got[1][2]).all()
    assert all(np.array_equal(g[:2], c[:2], equal_nan=True) for g, c in zip(got, clean))
    A = p["A"].copy()
    A[2, 3, 1] = np.nan
    A[1, M - 1, 0] = np.nan                                                   # beyond counts[1]: never read
    got = ref.predict(*args(A=A))
    assert np.isnan(got[0][2, 3]).all() and np.isnan(got[1][2, 3])
    keep = np.arange(M) != 3
    assert np.array_equal(got[0][2, keep], clean[0][2, keep]) and np.array_equal(got[1][2, keep], clean[1][2, keep])
    assert all(np.array_equal(g[:2], c[:2], equal_nan=True) for g, c in zip(got, clean))
    for v in (np.nan, np.inf):
        lw = p["lw"].copy()
        lw[1, 5] = v
        got = ref.predict(*args(lw=lw))
        assert np.isnan(got[0][1]).all() and np.isnan(got[1][1]).all() and np.array_equal(got[0][2], clean[0][2])
    lw = p["lw"].copy()
    lw[1, :] = -np.inf
    lw[2, 5] = -np.inf                                                        # a lone -inf: weight 0
    got = ref.predict(*args(lw=lw))
    assert np.isnan(got[0][1]).all() and np.isfinite(got[0][2].astype(np.float64)).all() and np.isfinite(got[1][2].astype(np.float64)).all()
    keep = np.arange(S) != 5
    sub = ref.predict(p["A"][2:], p["y"][2:], 3, None, p["X"][2:, keep], p["lw"][2:, keep])
    assert np.abs(got[0][2] - sub[0][0]).max() <= 1e-17 and np.abs(got[1][2] - sub[1][0]).max() <= 1e-15
    y = p["y"].copy()
    y[2, 0], y[2, 4] = 3, -1
    got = ref.predict(*args(y=y))
    assert np.isnan(got[1][2, [0, 4]]).all() and np.array_equal(got[0], clean[0], equal_nan=True)
    keep = ~np.isin(np.arange(M), (0, 4))
    assert np.array_equal(got[1][2, keep], clean[1][2, keep])
    assert nk[0] == 0 and np.isnan(clean[0][0]).all()


def test_lpd_does_not_underflow_at_large_predictors():
    """the true class at eta near -800 for every draw: lpd stays finite (about -800) where the log of a linear-space sum is -inf"""
    A = np.array([[[1.0]]])
    X = -800.0 + 0.1 * np.arange(8.0).reshape(1, 8, 1)
    prob, lpd = ref.predict(A, np.array([[0]], dtype=np.int32), 2, None, X, None)
    assert -801.0 < float(lpd[0, 0]) < -799.0 and float(np.float64(prob[0, 0, 0])) == 0.0 and float(np.float64(prob[0, 0, 1])) == 1.0
    with np.errstate(divide="ignore"):
        assert np.log(np.exp(X[0, :, 0]).sum() / 8.0) == -np.inf


def test_prob_is_the_expectation_by_quadrature():
    """C = 3, P = 1 (D = 2), S = 4096, seeds 0 .. 4: the restatement on S draws of q against E_q[softmax] by tensor Gauss-Hermite
    quadrature: every probability within 5 x 0.5 / sqrt(S) = 0.039, five times the largest possible Monte-Carlo standard error"""
    assert ref.QUAD_BOUND == 5 * 0.5 / 64.0 and abs(ref.QUAD_BOUND - 0.039) < 1e-4
    worst = []
    for seed in ref.QUAD_SEEDS:
        p = ref.quad_problem(seed)
        exact = ref.quad_exact(p)
        assert np.abs(exact.sum(1) - 1.0).max() <= 1e-12 and np.abs(exact - ref.quad_exact(p, Q=64)).max() <= 1e-4
        X = ref.quad_draws(p, ref.QUAD_S)
        prob, _ = ref.predict(p["A"], None, 3, None, X, None, np.float64)
        worst.append(float(np.abs(prob[0] - exact).max()))
    print("largest |prob - quadrature| per seed:", np.array2string(np.array(worst), precision=4))
    assert max(worst) <= ref.QUAD_BOUND
