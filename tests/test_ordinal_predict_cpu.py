"""The batched ordinal posterior predictive without a GPU: the C ABI declarations, bindings and argument checks through the built
library; the LDS bound over every legal (P, C); the host logic of ``predict_ordinal_batched`` on a stand-in engine; the properties of
the restatement (tests/ordinal_predict_ref.py): its float64 noise floor, rows of prob that sum to one, the product form against
exp(t) of the link, the NaN rules, large linear predictors, and the Monte-Carlo mean against E_q[p_c] by tensor Gauss-Hermite
quadrature."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import glm_batched_ref as gref
import ordinal_batched_ref as oref
import ordinal_predict_ref as ref
import psis_loo_ordinal_ref as lo
import psis_loo_ref as lref
from gsmvi_amd import predict_ordinal_batched      # noqa: F401  (the feature: without it nothing here can pass)
from gsmvi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsmvi_ordinal_predict_batched_f64"
LDSFN = "gsmvi_ordinal_predict_lds_bytes"


# ---- 1. declaration, binding, argument checks, the LDS bound -----------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name, nargs in ((NAME, 15), (LDSFN, 2)):
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
    # the arguments in the order of the issue: the model's are gsmvi_psis_loo_ordinal_batched_f64's
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
    assert [p.split()[-1].lstrip("*") for p in decl.split(",")] == ["ctx", "stream", "K", "P", "C", "M", "S", "A", "y", "offset",
                                                                      "counts_dev", "X", "lw", "prob", "lpd"]
    assert NAME in hdr.split("#ifndef GSMVI_HIP_H")[0] and LDSFN in hdr.split("#ifndef GSMVI_HIP_H")[0]      # the mapping list
    block = hdr[:hdr.index("int " + LDSFN)].rsplit("/*", 1)[1]                 # the definition is written above the entry point
    for line in ("cut_s0 = delta_s0,  cut_sj = cut_s,j-1 + w_sj,  w_sj = exp(delta_sj)",
                 "eta_si = a_i . beta_s + o_i",
                 "z_sij  = cut_sj - eta_si",
                 "p_si0  = sigma(z_si0),   p_si,C-1 = sigma(-z_si,C-2),   p_sic = sigma(z_sic) sigma(-z_si,c-1) (-expm1(-w_sc))",
                 "prob[k, i, c] = sum_s w_s p_sic,   w_s = exp(lw_s)",
                 "lpd[k, i]     = log sum_s exp(lw_s + l_si)",
                 "The reference has no twin",
                 "No two probabilities are subtracted",
                 "8 (80 (4 ceil(P / 4) +",
                 "GSMVI_PATH_BATCHED_PREDICT |",
                 "GSMVI_PATH_BATCHED_TARGET (no bit of its own"):
        assert line in block, line
    # no new path bit, the word is not widened, the ABI version stays; the kernel is named at both bits of its pair
    assert len(re.findall(r"#define\s+GSMVI_PATH_\w+\s+0x[0-9a-fA-F]+u", hdr)) == 32
    assert re.search(r"#define\s+GSMVI_ABI_VERSION\s+1\b", hdr) and _lib.load_library().gsmvi_abi_version() == 1
    for bit in ("GSMVI_PATH_BATCHED_PREDICT", "GSMVI_PATH_BATCHED_TARGET"):
        assert "k_ordinal_predict_batched" in re.search(r"#define\s+" + bit + r"\s.*", hdr).group(0), bit
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_predict"] | HipEngine.PATH_BITS["batched_target"] == ref.PATH_BITS
    assert callable(HipEngine.ordinal_predict_lds_bytes) and callable(HipEngine.ordinal_predict_batched)


def test_public_names_and_docstrings():
    import gsmvi_amd
    import gsmvi_amd.targets as targets
    assert gsmvi_amd.predict_ordinal_batched is targets.predict_ordinal_batched and "predict_ordinal_batched" in gsmvi_amd.__doc__
    assert dataclasses.is_dataclass(gsmvi_amd.OrdinalPrediction) and "OrdinalPrediction" in gsmvi_amd.__doc__
    assert [f.name for f in dataclasses.fields(gsmvi_amd.OrdinalPrediction)] == ["prob", "label", "median", "lpd", "elpd", "psis",
                                                                                 "num_draws", "nlaunch"]
    doc = " ".join(gsmvi_amd.BatchedOrdinalTarget.__doc__.split())
    assert "predict_ordinal_batched" in doc and "OrdinalPrediction" in doc
    # the two sentences that earlier tests look for survive as quoted history
    assert "Only the posterior predictive is missing now" in doc
    assert "A Hessian and Laplace start and a posterior predictive do not exist yet" in doc
    assert "predict_ordinal_batched" in targets.__doc__ and "none exists yet for this family" not in " ".join(targets.__doc__.split())
    assert not hasattr(gsmvi_amd.BatchedOrdinalTarget, "predict")                # a free function: the class gets no method
    fdoc = " ".join(gsmvi_amd.predict_ordinal_batched.__doc__.split())
    assert "gsmvi_ordinal_predict_batched_f64" in fdoc and "psis_batched" in fdoc and "no two probabilities are subtracted" in fdoc


def test_abi_checks_arguments_before_the_context():
    ref.check_bad_arguments(_lib.load_library())


def test_lds_bytes_stay_inside_the_workgroup_limit():
    """every (P, C) with D = P + C - 1 <= 64: the library's value is the header's formula, positive and at most 160 KB; the largest
    is (1, 64), above 64 KB (hence the kernel attribute) and far below the limit; 0 outside the bounds"""
    lib = _lib.load_library()
    worst, n = (0, None), 0
    for Cc in range(2, 65):
        for P in range(1, 70):
            if P > 65 - Cc:
                assert lib.gsmvi_ordinal_predict_lds_bytes(P, Cc) == 0 == ref.lds_bytes(P, Cc), (P, Cc)
                continue
            b = lib.gsmvi_ordinal_predict_lds_bytes(P, Cc)
            assert b == ref.lds_bytes(P, Cc) and 0 < b <= ref.LDS_MAX and b % 8 == 0, (P, Cc, b)
            worst = max(worst, (b, (P, Cc)))
            n += 1
    assert n == sum(65 - c for c in range(2, 65)) and worst == (105408, (1, 64)) and 64 * 1024 < worst[0] < 112 * 1024
    for P, Cc in ((1, 1), (4, 0), (0, 2), (64, 2), (63, 3), (2, 64), (1, 65), (33, 33), (3, -1), (-1, 3), (2 ** 17, 2 ** 17)):
        assert lib.gsmvi_ordinal_predict_lds_bytes(P, Cc) == 0 == ref.lds_bytes(P, Cc), (P, Cc)


# ---- 2. host logic on the stand-in engine ------------------------------------------------------------------------------------------
def _fitted(K=3, N=12, P=3, Cc=4, M=7, seed=3):
    import gsmvi_amd
    rs = np.random.default_rng(seed)
    A = rs.standard_normal((K, N, P)) / np.sqrt(P)
    offset = 0.3 * rs.standard_normal((K, N))
    beta = rs.standard_normal((K, P))
    y = lo.draw_labels(rs, A, offset, beta, Cc)
    eng = ref.StandInEngine()
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, Cc, 1.0, 1.0, offset=offset, engine=eng)
    D = P + Cc - 1
    mean = np.concatenate([beta + 0.1 * rs.standard_normal((K, P)), np.full((K, 1), -1.0), np.full((K, Cc - 2), -0.2)], axis=1)
    G = rs.standard_normal((K, D, D))
    cov = np.linalg.inv(np.eye(D)[None] + 0.3 * G @ np.swapaxes(G, 1, 2))
    A_new = rs.standard_normal((K, M, P)) / np.sqrt(P)
    o_new = 0.3 * rs.standard_normal((K, M))
    y_new = lo.draw_labels(rs, A_new, o_new, beta, Cc)
    return tgt, eng, mean, 0.5 * (cov + np.swapaxes(cov, 1, 2)), A_new, o_new, y_new


def _launches(eng):
    return [c for c in eng.calls if isinstance(c, tuple)]


def _median(prob):
    """the smallest c whose cumulative probability reaches 0.5, row by row in plain Python"""
    out = np.empty(prob.shape[:-1], dtype=np.int64)
    for idx in np.ndindex(*out.shape):
        acc, out[idx] = 0.0, prob.shape[-1] - 1
        for c, v in enumerate(np.cumsum(prob[idx])):
            if v >= 0.5:
                out[idx] = c
                break
    return out


def test_uniform_mode_draws_once_makes_no_lp_call_and_summarises_under_counts():
    import gsmvi_amd
    tgt, eng, mean, cov, A_new, o_new, y_new = _fitted()
    K, M, D, S, Cc, P = 3, 7, 6, 40, 4, 3
    keys = [5, 6, 7]
    cnt = np.array([7, 0, 4])
    m0, c0 = mean.copy(), cov.copy()
    eng.calls.clear()
    r = gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, offset=o_new, y=y_new, counts=cnt, num_draws=S, call=2)
    assert isinstance(r, gsmvi_amd.OrdinalPrediction) and r.nlaunch == 2 and r.num_draws == S and r.psis is None
    assert np.array_equal(mean, m0) and np.array_equal(cov, c0)
    seeds = tuple((k % 2 ** 32) ^ 0x5DEECE66D for k in keys)
    assert _launches(eng) == [("draw", seeds, 2, 0, S), ("predict_ordinal", Cc, (K, S, D), (K, M, P), False, True, True, True)]
    # the draws are psis_batched's for the same keys and call
    top = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, call=2, moments=False, engine=ref.StandInEngine())
    prob, lpd = ref.predict(A_new, y_new, o_new, cnt, top.samples, None, Cc)
    assert isinstance(r.prob, np.ndarray) and r.prob.shape == (K, M, Cc) and r.lpd.shape == (K, M) and r.elpd.shape == (K,)
    assert np.array_equal(r.prob, np.asarray(prob, dtype=np.float64), equal_nan=True)
    assert np.array_equal(r.lpd, np.asarray(lpd, dtype=np.float64), equal_nan=True)
    mask = np.arange(M)[None, :] < cnt[:, None]
    assert np.isfinite(r.prob[mask]).all() and np.isnan(r.prob[~mask]).all() and np.isnan(r.lpd[~mask]).all()
    # label: the first maximum; median: the smallest class whose cumulative probability reaches 0.5; both -1 where the row is NaN
    assert r.label.dtype == np.int64 and np.array_equal(r.label[mask], np.argmax(r.prob[mask], axis=1)) and (r.label[~mask] == -1).all()
    assert r.median.dtype == np.int64 and np.array_equal(r.median[mask], _median(r.prob[mask])) and (r.median[~mask] == -1).all()
    assert r.median[mask].min() >= 0 and r.median[mask].max() <= Cc - 1
    # elpd: the sum over the valid rows, 0 for a problem without one
    want = np.array([r.lpd[k, :cnt[k]].sum() for k in range(K)])
    assert np.allclose(r.elpd, want, rtol=1e-14, atol=0) and r.elpd[1] == 0.0 and (r.elpd[[0, 2]] < 0).all()
    # without y: no lpd, no elpd; without counts every row counts; without offset it is not passed
    eng.calls.clear()
    bare = gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, offset=o_new, num_draws=S, call=2)
    assert bare.lpd is None and bare.elpd is None
    assert _launches(eng)[-1] == ("predict_ordinal", Cc, (K, S, D), (K, M, P), False, False, True, False)
    assert np.array_equal(bare.prob[mask], r.prob[mask]) and np.isfinite(bare.prob).all() and (bare.label >= 0).all()
    assert np.abs(bare.prob.sum(2) - 1.0).max() <= 1e-14
    eng.calls.clear()
    gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, None, y_new, num_draws=S)      # positional: offset, then y
    assert _launches(eng)[-1] == ("predict_ordinal", Cc, (K, S, D), (K, M, P), False, True, False, False)
    # a median that differs from the mode: probabilities (0.4, 0.15, 0.45) have mode 2 and median 1
    pt = torch.tensor([[[0.4, 0.15, 0.45], [0.5, 0.1, 0.4], [0.2, 0.2, 0.6]]])
    assert _median(pt.numpy()).tolist() == [[1, 0, 2]] and ((torch.cumsum(pt, 2) < 0.5).sum(2)).tolist() == [[1, 0, 2]]


def test_psis_mode_weights_the_draws_and_psis_is_reused():
    import gsmvi_amd
    tgt, eng, mean, cov, A_new, o_new, y_new = _fitted()
    K, M, D, S, Cc, P = 3, 7, 6, 40, 4, 3
    keys = [5, 6, 7]
    eng.calls.clear()
    r = gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, o_new, y_new, num_draws=S, weights="psis")
    seeds = tuple((k % 2 ** 32) ^ 0x5DEECE66D for k in keys)
    assert _launches(eng) == [("draw", seeds, 0, 0, S), ("ordinal", "lp"), ("psis", (K, S, D), False),
                              ("predict_ordinal", Cc, (K, S, D), (K, M, P), True, True, True, False)]
    assert r.nlaunch == 3 and isinstance(r.psis, gsmvi_amd.PSISBatchedResult) and r.psis.khat.shape == (K,) and r.psis.mean is None
    prob, lpd = ref.predict(A_new, y_new, o_new, None, r.psis.samples, r.psis.log_weights, Cc)
    assert np.array_equal(r.prob, np.asarray(prob, dtype=np.float64)) and np.array_equal(r.lpd, np.asarray(lpd, dtype=np.float64))
    uni = gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, o_new, y_new, num_draws=S)
    assert not np.array_equal(uni.prob, r.prob) and uni.psis is None and uni.nlaunch == 2
    # psis= with "psis": one launch, the same numbers; with "uniform": its samples only
    eng.calls.clear()
    again = gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, o_new, y_new, psis=r.psis, weights="psis", num_draws=7)
    assert [c[0] for c in _launches(eng)] == ["predict_ordinal"] and again.nlaunch == 1 and again.num_draws == S
    assert again.psis is r.psis
    for n in ("prob", "label", "median", "lpd", "elpd"):
        assert np.array_equal(getattr(again, n), getattr(r, n)), n
    eng.calls.clear()
    plain = gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, o_new, y_new, psis=r.psis)
    assert _launches(eng) == [("predict_ordinal", Cc, (K, S, D), (K, M, P), False, True, True, False)] and plain.nlaunch == 1
    for n in ("prob", "label", "median", "lpd", "elpd"):
        assert np.array_equal(getattr(plain, n), getattr(uni, n)), n
    # a problem whose problem-level run failed comes out NaN
    broken = dataclasses.replace(r.psis, log_weights=np.where(np.arange(K)[:, None] == 1, np.nan, r.psis.log_weights))
    b = gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, o_new, y_new, psis=broken, weights="psis")
    assert np.isnan(b.prob[1]).all() and np.isnan(b.lpd[1]).all() and (b.label[1] == -1).all() and (b.median[1] == -1).all()
    assert np.isnan(b.elpd[1])
    assert np.array_equal(b.prob[[0, 2]], r.prob[[0, 2]]) and np.array_equal(b.elpd[[0, 2]], r.elpd[[0, 2]])
    # torch out
    t = gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, o_new, y_new, psis=r.psis, as_torch=True)
    assert isinstance(t.label, torch.Tensor) and t.label.dtype == torch.int64 and isinstance(t.elpd, torch.Tensor)
    assert isinstance(t.median, torch.Tensor) and t.median.dtype == torch.int64
    assert np.array_equal(np.asarray(t.label), plain.label) and np.array_equal(np.asarray(t.median), plain.median)
    assert np.array_equal(np.asarray(t.elpd), plain.elpd)


def test_type_and_argument_errors_come_before_any_engine_call():
    import gsmvi_amd
    tgt, eng, mean, cov, A_new, o_new, y_new = _fitted()
    Ag, yg, offset, _, _, tau, _ = gref.make_inputs("logistic", 3, 12, 4, 1, seed=3)
    glm = gsmvi_amd.BatchedGLMTarget(Ag, yg, "logistic", 1.0, offset=offset, noise_precision=tau, engine=lref.StandInEngine())
    eng.calls.clear()
    for bad in (glm, tgt.lp, None):
        with pytest.raises(TypeError, match="predict_ordinal_batched: target must be a BatchedOrdinalTarget"):
            gsmvi_amd.predict_ordinal_batched(bad, mean, cov, A_new, [1, 2, 3])
    # the other families' predictives refuse this target, in their own words; the class has no method
    for fn in (gsmvi_amd.predict_softmax_batched, gsmvi_amd.predict_negbin_batched, gsmvi_amd.predict_shared_batched):
        with pytest.raises(TypeError, match=fn.__name__):
            fn(tgt, mean, cov, A_new, [1, 2, 3])
    assert not hasattr(tgt, "predict")
    pr = lambda *a, **kw: gsmvi_amd.predict_ordinal_batched(tgt, *a, **kw)    # noqa: E731
    keys = [1, 2, 3]
    with pytest.raises(ValueError, match="predict_ordinal_batched: A_new"):
        pr(mean, cov, A_new[:, :, :1], keys)
    with pytest.raises(ValueError, match="A_new"):
        pr(mean, cov, A_new[:2], keys)
    with pytest.raises(ValueError, match="A_new"):
        pr(mean, cov, A_new[0], keys)
    with pytest.raises(ValueError, match="predict_ordinal_batched: mean must be"):
        pr(mean[:, :3], cov, A_new, keys)
    with pytest.raises(ValueError, match="predict_ordinal_batched: cov must be"):
        pr(mean, cov[:, :3], A_new, keys)
    with pytest.raises(ValueError, match=r"predict_ordinal_batched: offset: expected shape \(K, M\)"):
        pr(mean, cov, A_new, keys, offset=o_new[:, :3])
    bad_o = o_new.copy()
    bad_o[1, 2] = np.inf
    with pytest.raises(ValueError, match="predict_ordinal_batched: offset"):
        pr(mean, cov, A_new, keys, offset=bad_o)
    with pytest.raises(ValueError, match="predict_ordinal_batched: y: expected shape"):
        pr(mean, cov, A_new, keys, y=y_new[:, :3])
    bad_y = y_new.copy()
    bad_y[2, 1] = 4
    with pytest.raises(ValueError, match=r"predict_ordinal_batched: y: labels .* problems \[2\]"):
        pr(mean, cov, A_new, keys, y=bad_y)
    assert pr(mean, cov, A_new, keys, y=bad_y, counts=np.array([7, 7, 1]), num_draws=8).lpd.shape == (3, 7)     # beyond counts: ignored
    eng.calls.clear()
    with pytest.raises(ValueError, match="y: expected integer labels"):
        pr(mean, cov, A_new, keys, y=y_new.astype(bool))
    with pytest.raises(ValueError, match=r"predict_ordinal_batched: counts: values outside 0 \.\. M = 7"):
        pr(mean, cov, A_new, keys, counts=np.array([1, 8, 2]))
    with pytest.raises(ValueError, match="counts: expected 3 integers"):
        pr(mean, cov, A_new, keys, counts=np.array([1.0, 2.0, 2.0]))
    with pytest.raises(ValueError, match="predict_ordinal_batched: 2 keys"):
        pr(mean, cov, A_new, [1, 2])
    for S in (4, 4097, 0, 10.5):
        with pytest.raises(ValueError, match="predict_ordinal_batched: num_draws"):
            pr(mean, cov, A_new, keys, num_draws=S)
    for w in ("PSIS", None, "importance", 1):
        with pytest.raises(ValueError, match="predict_ordinal_batched: weights"):
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
        gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, psis=good, engine=Device())


# ---- 3. properties of the restatement ------------------------------------------------------------------------------------------
def test_cases_are_the_issue_s_and_cover_what_they_claim():
    assert [c[:6] + ("w" if c[6] else "u",) for c in ref.CASES] == [
        (1, 2, False, 5, 1, 1, "u"), (3, 3, True, 63, 15, 3, "w"), (5, 4, False, 257, 33, 3, "w"), (4, 5, True, 64, 16, 3, "u"),
        (3, 2, False, 65, 17, 1, "w"), (1, 64, True, 63, 17, 3, "w"), (63, 2, False, 65, 33, 1, "u"), (60, 5, True, 64, 17, 1, "w"),
        (6, 5, True, 5, 33, 3, "w")]
    for case in ref.CASES:
        p = ref.make_case(case)
        assert lo.labels_cover(p["y"], p["counts"], p["C"]) and ref.draws_cover(p["X"], p["P"], p["C"]), case
        assert (p["lw"] is not None) == case[6] and (p["offset"] is not None) == case[2]
        if p["K"] == 3:
            assert p["counts"].tolist() == [0, max(1, p["M"] - 5), p["M"]]
        if p["lw"] is not None:
            assert np.abs(np.asarray(ref.lse(p["lw"], np.float64)) - 0.0).max() <= 1e-14      # normalised


def test_float64_noise_floor_of_the_restatement():
    """the restatement in float64 against longdouble over CASES: the floor that BAR and the row-sum bound of the GPU tests are
    measured against (the figures stand in the docstring of tests/ordinal_predict_ref.py)"""
    gp = gl = gs = gsl = 0.0
    for case in ref.CASES:
        p = ref.make_case(case)
        want = ref.expected(case)
        got = ref.predict(p["A"], p["y"], p["offset"], p["counts"], p["X"], p["lw"], p["C"], np.float64)
        gp, gl = max(gp, ref.rel_gap(got[0], want[0])), max(gl, ref.rel_gap(got[1], want[1]))
        live = np.isfinite(got[0]).all(2)
        if live.any():
            gs = max(gs, float(np.abs(got[0][live].sum(1) - 1).max()))
            gsl = max(gsl, float(np.abs(want[0][live].sum(1) - 1).max()))
    print(f"float64 noise floor over CASES: prob {gp:.2e} lpd {gl:.2e} |sum_c prob - 1| {gs:.2e} (longdouble {gsl:.2e})")
    assert ref.BAR == 1e-11 and ref.BAR >= 100 * max(gp, gl)                   # the bar is at least 100 floors wide
    assert ref.ROWSUM_BAR == 1e-13 and ref.ROWSUM_BAR >= 100 * gs


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_rows_of_prob_sum_to_one_and_equal_exp_of_the_link(case):
    """the valid rows of prob sum to 1 within 1e-15 (longdouble restatement; the weights are normalised to float64 rounding), every
    probability lies in [0, 1], lpd <= 0; rows i >= n_k are NaN; per draw the product form equals exp(t) of the link within 1e-18"""
    p = ref.make_case(case)
    prob, lpd = ref.expected(case)
    K, M, P, Cc = p["K"], p["M"], p["P"], p["C"]
    nk = ref.valid_rows(p["counts"], K, M)
    mask = np.arange(M)[None, :] < nk[:, None]
    assert np.abs(prob[mask].sum(1) - 1).max() <= 1e-15
    assert (prob[mask] >= 0).all() and (prob[mask] <= 1).all() and (lpd[mask] <= 0).all() and np.isfinite(lpd[mask].astype(np.float64)).all()
    assert np.isnan(prob[~mask]).all() and np.isnan(lpd[~mask]).all()
    bare, none = ref.predict(p["A"], None, p["offset"], p["counts"], p["X"], p["lw"], Cc)
    assert none is None and np.array_equal(bare, prob, equal_nan=True)
    k = K - 1                                                                  # every row of the last problem is valid
    LD = ref.LD
    eta = p["X"][k, :, :P].astype(LD) @ p["A"][k].astype(LD).T + (0 if p["offset"] is None else p["offset"][k][None, :].astype(LD))
    cut, w = oref.cutpoints(p["X"][k, :, P:], LD)
    pr = ref.class_probs(eta, cut, w)                                          # (S, M, C)
    for c in range(Cc):
        ell = ref.loglik_ordinal(p["A"][k:], np.full((1, M), c, dtype=np.int32), None if p["offset"] is None else p["offset"][k:],
                                 None, p["X"][k:], Cc)[0]                      # (M, S)
        assert np.abs(pr[:, :, c] - np.exp(ell).T).max() <= 1e-18, c


def test_restatement_nan_rules():
    """the rules of the header: a flagged draw (a non-finite x entry, an e^{delta_j} that is not a positive normal number) -> every
    valid row of its problem, whatever its weight; a non-finite a entry or offset -> its row; a NaN or +inf in lw, or only -inf ->
    the problem; a lone -inf is weight 0; a label out of range -> that row's lpd alone"""
    case = ref.CASES[1]                                                       # (3, 3), K = 3, counts (0, partial, M), weighted, offset
    p = ref.make_case(case)
    K, M, S, P, Cc = p["K"], p["M"], p["S"], p["P"], p["C"]
    args = lambda **kw: [dict(p, **kw)[n] for n in ("A", "y", "offset", "counts", "X", "lw", "C")]      # noqa: E731
    clean = ref.expected(case)
    for col, v in ((1, np.inf), (P, np.nan), (P + 1, 800.0), (P + 1, -800.0)):
        X = p["X"].copy()
        X[2, 7, col] = v
        lw = p["lw"].copy()
        lw[2, 7] = -np.inf                                                    # the flag counts whatever the draw's weight is
        got = ref.predict(*args(X=X, lw=lw))
        assert np.isnan(got[0][2]).all() and np.isnan(got[1][2]).all(), (col, v)
        assert all(np.array_equal(g[:2], c[:2], equal_nan=True) for g, c in zip(got, clean))
    A, o = p["A"].copy(), p["offset"].copy()
    A[2, 3, 1] = np.nan
    o[2, 5] = -np.inf
    A[1, M - 1, 0] = np.nan                                                   # beyond counts[1]: never read
    got = ref.predict(*args(A=A, offset=o))
    assert np.isnan(got[0][2, [3, 5]]).all() and np.isnan(got[1][2, [3, 5]]).all()
    keep = ~np.isin(np.arange(M), (3, 5))
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
    sub = ref.predict(p["A"][2:], p["y"][2:], p["offset"][2:], None, p["X"][2:, keep], p["lw"][2:, keep], Cc)
    assert np.abs(got[0][2] - sub[0][0]).max() <= 1e-17 and np.abs(got[1][2] - sub[1][0]).max() <= 1e-15
    y = p["y"].copy()
    y[2, 0], y[2, 4] = Cc, -1
    got = ref.predict(*args(y=y))
    assert np.isnan(got[1][2, [0, 4]]).all() and np.array_equal(got[0], clean[0], equal_nan=True)
    keep = ~np.isin(np.arange(M), (0, 4))
    assert np.array_equal(got[1][2, keep], clean[1][2, keep])
    assert np.isnan(clean[0][0]).all()                                        # counts[0] = 0


def test_large_predictors_stay_finite_with_exact_zeros_and_ones():
    """|eta| around 1000: the float64 product form is finite, holds exact 0 and 1 entries and sums to 1; the lpd of the least
    likely class stays finite (about -1000) where the log of a linear-space sum is -inf"""
    A = np.array([[[1.0], [-1.0], [0.0]]])
    X = np.concatenate([1000.0 + 0.1 * np.arange(8.0).reshape(1, 8, 1), np.zeros((1, 8, 1)), np.full((1, 8, 1), np.log(0.5))], axis=2)
    y = np.array([[0, 2, 1]], dtype=np.int32)                                 # the least likely class of rows 0 and 1
    prob, lpd = ref.predict(A, y, None, None, X, None, 3, np.float64)
    assert np.isfinite(prob).all() and np.isfinite(lpd).all()
    assert prob[0, 0].tolist() == [0.0, 0.0, 1.0] and prob[0, 1].tolist() == [1.0, 0.0, 0.0] and abs(prob[0, 2].sum() - 1) <= 1e-15
    assert -1001.0 < lpd[0, 0] < -999.0 and -1001.0 < lpd[0, 1] < -999.0 and lpd[0, 2] > -3.0
    with np.errstate(divide="ignore"):
        assert np.log(prob[0, 0, 0]) == -np.inf


def test_prob_is_the_expectation_by_quadrature():
    """P = 1, C = 3 (D = 3), S = 4096, seeds 0 .. 4: the restatement on S draws of q against E_q[p_c] by tensor Gauss-Hermite
    quadrature: every probability within 5 x 0.5 / sqrt(S) = 0.039, five times the largest possible Monte-Carlo standard error"""
    assert ref.QUAD_BOUND == 5 * 0.5 / 64.0 and abs(ref.QUAD_BOUND - 0.039) < 1e-4
    worst, conv = [], []
    for seed in ref.QUAD_SEEDS:
        p = ref.quad_problem(seed)
        exact = ref.quad_exact(p)
        conv.append(float(np.abs(exact - ref.quad_exact(p, Q=32)).max()))
        assert np.abs(exact.sum(1) - 1.0).max() <= 1e-12 and conv[-1] <= 1e-4      # two orders agree 400 times below the bound
        X = ref.quad_draws(p, ref.QUAD_S)
        prob, _ = ref.predict(p["A"], None, None, None, X, None, 3, np.float64)
        worst.append(float(np.abs(prob[0] - exact).max()))
    print("largest |prob - quadrature| per seed:", np.array2string(np.array(worst), precision=4),
          "quadrature orders 32 / 48 differ by", np.array2string(np.array(conv), precision=2))
    assert max(worst) <= ref.QUAD_BOUND
