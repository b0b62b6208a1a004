"""The batched ordinal PSIS leave-one-out without a GPU: the float64 noise floor of the restatement (tests/psis_loo_ordinal_ref.py)
on the GPU tests' inputs (the bar of tests/test_gpu_psis_loo_ordinal.py is 1000 times it); the table of cases; the tile helper and
the grid bound; the C ABI declarations and the argument checks; the host logic of ``psis_loo_ordinal_batched`` on a stand-in
engine; the C = 2 case as logistic regression and the rows' sum as the score restatement's lp; elpd_i against the leave-one-out
density by 3-D quadrature."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import glm_batched_ref as gref
import ordinal_batched_ref as oref
import psis_batched_ref as pref
import psis_loo_negbin_ref as nref
import psis_loo_ordinal_ref as ref
import psis_loo_ref as lref
import psis_loo_softmax_ref as sref
from gsmvi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsmvi_psis_loo_ordinal_batched_f64"
TILE = "gsmvi_psis_loo_ordinal_tile"


# ---- 1. the noise floor that sets the GPU tests' bar -------------------------------------------------------------------------------
def test_float64_noise_floor_of_the_restatement_on_the_gpu_inputs():
    """the restatement in float64 against itself in longdouble on every case of the GPU tests (both fed the same float64 l_si, logr
    and lw), relative to max(1, |value|): measured 1.68e-14 at the most (ess); l_si itself differs by 7.9e-16.  No valid row of any
    case changes its verdict between the two precisions (a case whose row did would get another seed in ref.SEEDS, never an
    exclusion).  The GPU bar is 1000 times the recorded floor."""
    worst, rows = {}, 0
    for c in ref.CASES:
        p = ref.make_case(c)
        args = (p["A"], p["y"], p["offset"], p["counts"], p["X"], p["C"])
        ell = np.asarray(ref.loglik_ordinal(*args, np.float64), dtype=np.float64)
        worst["loglik"] = max(worst.get("loglik", 0.0), pref.rel_gap(ell, ref.loglik_ordinal(*args)))
        a = ref.loo_batched(ell, p["logr"], p["lw"], p["counts"], np.float64)
        b = ref.loo_batched(ell, p["logr"], p["lw"], p["counts"])
        assert np.array_equal(a["info"], b["info"]), ref.case_id(c)          # no row is left out: none changes its verdict
        rows += int((a["info"] != -3).sum())
        for n in ("elpd", "lpd", "khat", "ess"):
            worst[n] = max(worst.get(n, 0.0), ref.rel_gap(a[n], b[n]))
    print("float64 against longdouble:", {n: f"{g:.2e}" for n, g in worst.items()}, f"over {rows} valid rows")
    assert worst.pop("loglik") <= 1e-13                                       # (far inside the single-launch bar of 1e-11)
    floor = max(worst.values())
    assert floor <= ref.NOISE_FLOOR <= 2.0 * floor                            # the recorded floor is the measured one, rounded up
    assert ref.BAR == 1000 * ref.NOISE_FLOOR and ref.BAR < 1e-8 and ref.LOGLIK_BAR == 1e-11


def test_the_cases_are_the_table():
    P_, C_, S_ = ({c[i] for c in ref.CASES} for i in (0, 1, 3))
    assert {1, 3, 4, 6, 9, 17, 60} == P_ and {2, 3, 5, 16, 64} == C_ and S_ == {5, 33, 257, 1024, 4096}
    assert {P % 4 for P in P_} == {0, 1, 2, 3} and (60, 5) in {c[:2] for c in ref.CASES}
    for P, Cc in ((9, 3), (1, 64)):                                           # the N edges at a small and at the widest C
        assert {c[4] for c in ref.CASES if c[:2] == (P, Cc) and c[3] == 33} == set(ref.N_OF)
    assert {c[2] for c in ref.CASES} == {False, True} and {c[5] for c in ref.CASES} == {1, 3}
    assert ref.CASES[-2] == (9, 5, True, 1024, "NI+1", 1) and ref.CASES[-1] == (1, 64, False, 4096, "NI+1", 1)
    assert ref.loo_tile(1, 64, 4096) == 2 < ref.NI_CAP and ref.make_case(ref.CASES[-1])["N"] == 3
    assert len(set(ref.CASES)) == len(ref.CASES) and set(ref.SEEDS) <= set(ref.CASES)
    for c in ref.CASES:
        p = ref.make_case(c)
        P, Cc, K, N = p["P"], p["C"], p["K"], p["N"]
        if c[5] == 3:
            assert list(p["counts"]) == [0, max(1, N // 2), N]
        else:
            assert p["counts"] is None
        assert (p["offset"] is not None) == c[2] and p["X"].shape == (K, c[3], P + Cc - 1)
        assert p["y"].dtype == np.int32 and p["y"].min() >= 0 and p["y"].max() <= Cc - 1
        assert ref.labels_cover(p["y"], p["counts"], Cc)                      # 0, C - 1 and an interior label where 3 rows count
        if Cc >= 3:
            w = np.exp(p["X"][:, :, P + 1:])
            assert (w < ref.LOG2).any() and (w >= ref.LOG2).any()             # both branches of ord_gap in every case


# ---- 2. the restatement's flag and counts -------------------------------------------------------------------------------------------
def test_restatement_nan_rules_and_counts():
    """a non-finite entry of a draw and an e^{delta_j}, j >= 1, that is not a positive normal number give NaN in that draw,
    whether or not a row carries the label j; nothing else does (delta_0 is a location: any finite value); rows i >= n_k are NaN;
    l_si is the log of a probability"""
    p = ref.make_case(next(c for c in ref.CASES if c[:2] == (9, 16)))         # offset, K = 3, counts (0, partial, N)
    K, N, S, P, Cc = p["K"], p["N"], p["S"], p["P"], p["C"]
    args = lambda X: (p["A"], p["y"], p["offset"], p["counts"], X, Cc, np.float64)      # noqa: E731
    clean = ref.loglik_ordinal(*args(p["X"]))
    nk = ref.valid_rows(p["counts"], K, N)
    mask = np.arange(N)[None, :] < nk[:, None]
    assert np.isfinite(clean[mask]).all() and np.isnan(clean[~mask]).all() and (clean[mask] < 0).all()
    unused = next(j for j in range(1, Cc - 1) if not (p["y"][2] == j).any())  # an interior class without a row in problem 2
    X = p["X"].copy()
    X[2, 7, 0], X[2, 8, P], X[2, 9, P + unused], X[2, 10, P + 1], X[2, 11, P - 1], X[2, 12, P] = np.inf, np.nan, 720.0, -720.0, -np.inf, 1e6
    bad = ref.loglik_ordinal(*args(X))
    hit = np.zeros(S, dtype=bool)
    hit[7:12] = True
    assert np.isnan(bad[2][:, hit]).all() and np.isfinite(bad[2][:, 12]).all()
    keep = ~hit & (np.arange(S) != 12)
    assert np.array_equal(bad[:, :, keep], clean[:, :, keep], equal_nan=True)
    # e^709 is a normal number (8.2e307), e^-709 is not (1.2e-308 is below the smallest, 2.2e-308); e^710 overflows
    rows = np.array([[0.0, 0.0, d] for d in (709.0, -709.0, 710.0, -710.0, 708.0, -708.0)])
    assert list(ref.draw_flag(rows, 1)) == [False, True, True, True, False, False]
    assert not ref.draw_flag(np.array([[0.0, 1e300]]), 1).any()               # C = 2: delta_0 alone, never limited


# ---- 3. the tile helper and the grid bound ------------------------------------------------------------------------------------------
def test_tile_helper_matches_its_formula_and_the_header_bounds():
    lib = _lib.load_library()
    worst = 0
    for Cc in range(2, 65):
        for P in sorted({1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 65 - Cc - 1, 65 - Cc}):
            if not 1 <= P <= 65 - Cc:
                continue
            tiles = ref.tiles_doubles(P, Cc)
            worst = max(worst, tiles)
            for S in (5, 8, 9, 33, 64, 257, 1024, 1025, 2048, 2049, 3000, 4095, 4096):
                ni = lib.gsmvi_psis_loo_ordinal_tile(P, Cc, S)
                assert ni == ref.loo_tile(P, Cc, S) and 1 <= ni <= ref.NI_CAP, (P, Cc, S)
                S2 = 1 << max(3, (S - 1).bit_length())
                region = max(S2 + S + 508 + S2 // 2, tiles)
                assert region + ni * S <= ref.LDS_MAX_DOUBLES                 # the 160 KB rule
                assert ni == ref.NI_CAP or region + (ni + 1) * S > ref.LDS_MAX_DOUBLES
                if S <= 2048:
                    assert ni == 4, (P, Cc, S)                                # the negbin tile's values
            assert lib.gsmvi_psis_loo_ordinal_tile(P, Cc, 4096) == 2, (P, Cc)
    assert worst == ref.tiles_doubles(61, 4) == 5736 and ref.tiles_doubles(1, 64) == 4776        # under 6144: (6144 + 4 x 1024)
    # doubles are half of the 160 KB, so two workgroups share a CU at S = 1024; far under the 12288 that S = 4096 leaves
    for P, Cc, S in ((0, 3, 8), (-1, 3, 8), (3, 1, 8), (3, 0, 8), (3, 65, 8), (64, 2, 8), (2, 64, 8), (63, 3, 8), (3, 3, 4),
                     (3, 3, 4097), (2 ** 30, 3, 8), (3, 2 ** 30, 8)):
        assert lib.gsmvi_psis_loo_ordinal_tile(P, Cc, S) == 0 == ref.loo_tile(P, Cc, S), (P, Cc, S)
    # K ceil(N / NI) at the 2^24 - 1 edge, in the arithmetic of the entry point
    ni = ref.loo_tile(3, 3, 8)
    K = 2 ** 12 - 1
    assert K * -(-(ni * 2 ** 12 + ni) // ni) == 2 ** 24 - 1 and K * -(-(ni * 2 ** 12 + ni + 1) // ni) > 2 ** 24 - 1


def test_abi_checks_arguments_before_the_context():
    ref.check_bad_arguments(_lib.load_library())


def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    libs = {mp: {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True,
                                                         text=True).stdout.splitlines() if ln.strip()}
            for mp, path in (("exports.map", _lib.library_path()),
                             ("exports_debug.map", os.path.join(os.path.dirname(_lib.library_path()), "libgsmvi_hip_debug.so")))}
    for name, nargs in ((NAME, 20), (TILE, 3)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        for mp, built in libs.items():                                        # the product map and the debug map, and what was built
            assert re.search(r"^\s*" + name + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), (mp, name)
            assert name in built, (mp, name)
        assert name in _lib.exported_symbols(), name
        res, args = _lib._SIGS[name]
        decl = re.search(r"int\s+" + name + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert res is C.c_int and len(args) == len(params) == nargs
        for p, a in zip(params, args):
            want = C.c_int64 if p.startswith("int64_t") else C.c_int if p.startswith("int ") else \
                C.c_double if p.startswith("double ") else C.c_void_p
            assert a is want, (p, a)
    assert NAME in hdr.split("#ifndef GSMVI_HIP_H")[0]
    block = hdr[:hdr.index("int " + TILE)].rsplit("/*", 1)[1]                  # the definition is written above the entry point
    for line in ("eta_si = a_i . beta_s + o_i",
                 "cut_s0 = delta_s0,   cut_sj = cut_s,j-1 + e^{delta_sj}",
                 "l_si   = t(eta_si, cut_s, e^{delta_s}, y_i) = log P(y_i | eta_si, cut_s)",
                 "no constant is added",
                 "rho_si = logr_s - l_si (one subtraction)",
                 "elpd[k, i] = log sum_s exp(w_si + l_si)",
                 "lpd[k, i]  = log sum_s exp(lw_s + l_si)",
                 "tiles = 80 (4 ceil(P / 4) + 1) + 64 ((C - 1) | 1) +",
                 "GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_TARGET"):
        assert line in block, line
    # no new path bit, the word is not widened, the ABI version stays
    assert len(re.findall(r"#define\s+GSMVI_PATH_\w+\s+0x[0-9a-fA-F]+u", hdr)) == 32
    assert re.search(r"#define\s+GSMVI_ABI_VERSION\s+1\b", hdr) and _lib.load_library().gsmvi_abi_version() == 1
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_loo"] | HipEngine.PATH_BITS["batched_target"] == ref.PATH_BITS
    assert callable(HipEngine.psis_loo_ordinal_tile) and callable(HipEngine.psis_loo_ordinal_batched)
    import gsmvi_amd
    assert gsmvi_amd.psis_loo_ordinal_batched is not None and "psis_loo_ordinal_batched" in gsmvi_amd.__doc__
    doc = " ".join(gsmvi_amd.BatchedOrdinalTarget.__doc__.split())
    assert "psis_loo_ordinal_batched" in doc and "leave-one-out and a posterior predictive do not exist" not in doc
    assert "A Hessian and Laplace start and a posterior predictive do not exist yet" in doc       # still true
    import gsmvi_amd.targets as targets
    assert "psis_loo_ordinal_batched" in targets.__doc__
    assert "psis_loo_softmax_batched" in gsmvi_amd.psis_loo_ordinal_batched.__doc__          # the docstring names the shared scale


# ---- 4. host logic on the stand-in engine ------------------------------------------------------------------------------------------
def _fitted(K=3, N=12, P=3, Cc=4, counts=(12, 0, 7), seed=3):
    import gsmvi_amd
    rs = np.random.default_rng(seed)
    A = rs.standard_normal((K, N, P)) / np.sqrt(P)
    offset = 0.3 * rs.standard_normal((K, N))
    y = ref.draw_labels(rs, A, offset, rs.standard_normal((K, P)), Cc)
    eng = ref.StandInEngine()
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, Cc, 1.0, 1.0, counts=None if counts is None else np.array(counts), offset=offset,
                                         engine=eng)
    D = P + Cc - 1
    mean = np.concatenate([0.3 * rs.standard_normal((K, P)), np.full((K, 1), -1.0), np.full((K, Cc - 2), -0.2)], axis=1)
    G = rs.standard_normal((K, D, D))
    cov = np.linalg.inv(np.eye(D)[None] + 0.3 * G @ np.swapaxes(G, 1, 2))
    return tgt, eng, mean, 0.5 * (cov + np.swapaxes(cov, 1, 2)), A, y, offset


def test_psis_loo_ordinal_batched_protocol_and_summaries():
    import gsmvi_amd
    tgt, eng, mean, cov, A, y, offset = _fitted()
    K, N, D, S, Cc = 3, 12, 6, 40, 4
    keys = [5, 6, 7]
    m0, c0 = mean.copy(), cov.copy()
    eng.calls.clear()
    r = gsmvi_amd.psis_loo_ordinal_batched(tgt, mean, cov, keys, num_draws=S, call=2, pointwise_loglik=True)
    assert isinstance(r, gsmvi_amd.LOOBatchedResult) and r.nlaunch == 3 and r.threshold == pref.threshold(S)
    assert np.array_equal(mean, m0) and np.array_equal(cov, c0)
    launches = [c for c in eng.calls if isinstance(c, tuple)]
    seeds = tuple((k % 2 ** 32) ^ 0x5DEECE66D for k in keys)
    assert launches == [("draw", seeds, 2, 0, S), ("ordinal", "lp"), ("psis", (K, S, D), False),
                        ("loo_ordinal", (K, S, D), (K, N, 3), Cc, True, True, True)]
    top = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, call=2, moments=False, engine=ref.StandInEngine())
    assert np.array_equal(r.psis.khat, top.khat) and np.array_equal(r.psis.samples, top.samples)
    cnt = np.array([12, 0, 7])
    ell = np.asarray(ref.loglik_ordinal(A, y, offset, cnt, top.samples, Cc), dtype=np.float64)
    want = ref.loo_batched(ell, top.log_ratios, top.log_weights, cnt)
    assert np.array_equal(r.loglik, ell, equal_nan=True) and r.loglik.shape == (K, N, S)
    for got, n in ((r.elpd_i, "elpd"), (r.lpd_i, "lpd"), (r.khat, "khat"), (r.ess, "ess")):
        assert isinstance(got, np.ndarray) and np.array_equal(got, np.asarray(want[n], dtype=np.float64), equal_nan=True), n
    assert np.array_equal(r.info, want["info"]) and r.info.dtype == np.int64
    assert (r.info[0] != -3).all() and (r.info[1] == -3).all() and (r.info[2, 7:] == -3).all()
    # the per-problem summaries are psis_loo_ref.summaries, under counts
    s = ref.summaries(want, cnt, S)
    for n in ("elpd_loo", "p_loo", "se"):
        assert np.allclose(getattr(r, n), s[n], rtol=1e-13, atol=0, equal_nan=True), n
    assert r.elpd_loo[1] == 0.0 and np.isnan(r.se[1]) and r.n_bad[1] == 0
    assert np.array_equal(r.n_bad, s["n_bad"])
    assert np.array_equal(r.ok, np.asarray(r.psis.ok) & (r.n_bad == 0)) and r.ok.dtype == bool
    # psis= reuses the draws: one launch, the same numbers; no pointwise block unless asked for
    eng.calls.clear()
    again = gsmvi_amd.psis_loo_ordinal_batched(tgt, mean, cov, keys, psis=r.psis)
    assert [c[0] for c in eng.calls if isinstance(c, tuple)] == ["loo_ordinal"] and again.nlaunch == 1 and again.loglik is None
    for n in ("elpd_loo", "p_loo", "se", "elpd_i", "lpd_i", "khat", "ess", "info", "n_bad", "ok"):
        assert np.array_equal(getattr(again, n), getattr(r, n), equal_nan=True), n
    # the target gained no method
    assert not any(hasattr(tgt, name) for name in ("neg_hessian", "predict", "loo", "family"))


def test_type_and_argument_errors_come_before_any_engine_call():
    import dataclasses
    import gsmvi_amd
    tgt, eng, mean, cov, _, _, _ = _fitted()
    Ag, yg, offset, _, _, tau, _ = gref.make_inputs("poisson", 3, 12, 6, 1, seed=3)
    glm = gsmvi_amd.BatchedGLMTarget(Ag, yg, "poisson", 1.0, offset=offset, noise_precision=tau, engine=lref.StandInEngine())
    logit = gsmvi_amd.BatchedLogisticTarget(Ag, (yg > 0).astype(np.float64), 1.0, engine=lref.StandInEngine())
    rs = np.random.default_rng(0)
    As = rs.standard_normal((3, 12, 3))
    soft = gsmvi_amd.BatchedSoftmaxTarget(As, sref.draw_labels(rs, As, rs.standard_normal((3, 2, 3))), 3, 1.0, engine=sref.StandInEngine())
    negbin = gsmvi_amd.BatchedNegBinomialTarget(Ag[:, :, :5], np.floor(np.abs(yg)), 1.0, engine=nref.StandInEngine())
    gauss = gsmvi_amd.BatchedGaussianTarget(np.zeros((3, 6)), cov=np.stack([np.eye(6)] * 3), engine=lref.StandInEngine())
    eng.calls.clear()
    for bad in (glm, logit, soft, negbin, gauss, tgt.lp, gsmvi_amd.psis_batched, None):
        with pytest.raises(TypeError, match="psis_loo_ordinal_batched: target must be a BatchedOrdinalTarget"):
            gsmvi_amd.psis_loo_ordinal_batched(bad, mean, cov, [1, 2, 3])
    # the existing leave-one-out functions keep their refusals of this target
    with pytest.raises(TypeError, match="BatchedGLMTarget"):
        gsmvi_amd.psis_loo_batched(tgt, mean, cov, [1, 2, 3])
    with pytest.raises(TypeError, match="BatchedSoftmaxTarget"):
        gsmvi_amd.psis_loo_softmax_batched(tgt, mean, cov, [1, 2, 3])
    with pytest.raises(TypeError, match="BatchedNegBinomialTarget"):
        gsmvi_amd.psis_loo_negbin_batched(tgt, mean, cov, [1, 2, 3])
    with pytest.raises(TypeError, match="SharedDesignGLMTarget"):
        gsmvi_amd.psis_loo_shared_batched(tgt, mean, cov, [1, 2, 3])
    loo = lambda *a, **kw: gsmvi_amd.psis_loo_ordinal_batched(tgt, *a, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="psis_loo_ordinal_batched: mean must be"):
        loo(mean[:, :3], cov, [1, 2, 3])
    with pytest.raises(ValueError, match="mean must be"):
        loo(mean[:2], cov, [1, 2, 3])
    with pytest.raises(ValueError, match="cov must be"):
        loo(mean, cov[:, :3], [1, 2, 3])
    with pytest.raises(ValueError, match="keys"):
        loo(mean, cov, [1, 2])
    for S in (4, 4097, 0, 10.5):
        with pytest.raises(ValueError, match="num_draws"):
            loo(mean, cov, [1, 2, 3], num_draws=S)
    with pytest.raises(ValueError, match="PSISBatchedResult"):
        loo(mean, cov, [1, 2, 3], psis=dict(samples=None))
    w = gsmvi_amd.psis_weights_batched(np.zeros((3, 8)), engine=ref.StandInEngine())
    with pytest.raises(ValueError, match="samples"):                           # the weights entry keeps no draws
        loo(mean, cov, [1, 2, 3], psis=w)
    assert not any(isinstance(c, tuple) for c in eng.calls)
    good = gsmvi_amd.psis_batched(tgt.lp, mean, cov, [1, 2, 3], num_draws=8, moments=False, engine=ref.StandInEngine())
    eng.calls.clear()                                                          # (tgt.lp went through the target's engine)
    with pytest.raises(ValueError, match="log_weights"):
        loo(mean, cov, [1, 2, 3], psis=dataclasses.replace(good, log_weights=None))
    with pytest.raises(ValueError, match=r"psis.samples must be"):
        loo(mean, cov, [1, 2, 3], psis=dataclasses.replace(good, samples=good.samples[:, :, :3]))
    with pytest.raises(ValueError, match="log_ratios and psis.log_weights"):
        loo(mean, cov, [1, 2, 3], psis=dataclasses.replace(good, log_ratios=good.log_ratios[:, :5]))
    assert not any(isinstance(c, tuple) for c in eng.calls)

    class Device(ref.StandInEngine):                                           # an engine that works on device tensors
        device = torch.device("cpu")
    with pytest.raises(ValueError, match="samples, log_ratios, log_weights"):  # host copies: as_torch=False results
        gsmvi_amd.psis_loo_ordinal_batched(tgt, mean, cov, [1, 2, 3], psis=good, engine=Device())


# ---- 5. properties of the restatement ----------------------------------------------------------------------------------------------
def test_two_classes_are_logistic_regression_on_the_design_with_a_minus_one_column():
    """C = 2: P(y = 1) = sigmoid(eta - cut_0), so l_si is psis_loo_ref.loglik("logistic", ...) on the design [A, -1] at the same
    draws (delta_0 is the coefficient of the last column), to the float64 noise floor of l_si (1e-13, the bound of test 1)"""
    p = ref.make_case(next(c for c in ref.CASES if c[:2] == (17, 2)))
    A1 = np.concatenate([p["A"], -np.ones((p["K"], p["N"], 1))], axis=2)
    for dtype in (np.float64, ref.LD):
        od = ref.loglik_ordinal(p["A"], p["y"], p["offset"], p["counts"], p["X"], 2, dtype)
        lg = lref.loglik("logistic", A1, p["y"].astype(np.float64), p["offset"], p["counts"], 1.0, p["X"], dtype)
        g = pref.rel_gap(od, lg)
        print(f"{dtype.__name__}: C = 2 against logistic on [A, -1] {g:.2e}")
        assert g <= 1e-13, (dtype, g)


@pytest.mark.parametrize("case", [c for c in ref.CASES if c[4] == "2NI+3" and c[1] in (5, 16)], ids=ref.case_id)
def test_rows_sum_to_the_score_restatement_lp(case):
    """for each draw sum_{i < n_k} l_si - lam |beta|^2 / 2 - kap |delta|^2 / 2 is ordinal_batched_ref.score_and_lp_ld's lp, within
    1e-15 of sum |l_si| + 1 in longdouble (the same terms in another order)"""
    p = ref.make_case(case)
    K, N, P, Cc = p["K"], p["N"], p["P"], p["C"]
    lam, kap = 0.7, 0.4
    _, lp = oref.score_and_lp_ld(p["A"], p["y"], p["offset"], p["counts"], lam, kap, p["X"], Cc)
    ell = ref.loglik_ordinal(p["A"], p["y"], p["offset"], p["counts"], p["X"], Cc)
    nk = ref.valid_rows(p["counts"], K, N)
    worst = 0.0
    for k in range(K):
        n = int(nk[k])
        beta, delta = p["X"][k, :, :P].astype(ref.LD), p["X"][k, :, P:].astype(ref.LD)
        total = ell[k, :n].sum(0) - ref.LD(lam) * (beta * beta).sum(1) / 2 - ref.LD(kap) * (delta * delta).sum(1) / 2
        scale = np.abs(ell[k, :n]).sum(0) + 1
        worst = max(worst, float(np.max(np.abs(total - lp[k]) / scale)))
    print(f"{ref.case_id(case)}: sum of l_si against the score restatement's lp {worst:.1e} of sum |l_si| + 1")
    assert worst <= 1e-15


# ---- 6. a statistical check with an exact answer -----------------------------------------------------------------------------------
def test_elpd_is_the_leave_one_out_density_by_quadrature():
    """P = 1, C = 3 (D = 3: beta, delta_0, delta_1), N = 12, unit priors, seeds 0 .. 4: elpd_i of the restatement on S = 4096 draws
    of the Laplace Gaussian against log int p(y_i | x) p(x | y_-i) dx by 3-D grid quadrature: a Monte-Carlo gap, bounded by twice
    the largest measured over the rows and seeds (psis_loo_ordinal_ref.QUAD_GAP: 0.037, at seed 1); 0 < sum p_loo < 2 D"""
    gap, khat, top = [], [], []
    for seed in ref.QUAD_SEEDS:
        p = ref.quad_problem(seed, **ref.QUAD_SHAPE)
        r, t = ref.quad_restatement_run(p, ref.QUAD_S)
        assert (r["info"] == 0).all()
        exact = ref.quad_exact_loo(p)
        assert (exact < 0).all()
        gap.append(np.abs(np.asarray(r["elpd"], dtype=np.float64) - exact).max())
        khat.append(float(np.max(r["khat"])))
        top.append(t)
        assert 0.0 < float((r["lpd"] - r["elpd"]).sum()) < 6.0
    print(f"gap {max(gap):.4f} (per seed {np.array2string(np.array(gap), precision=4)}), largest pointwise khat {max(khat):.2f}, "
          f"problem-level khat <= {max(top):.2f}")
    assert abs(max(gap) - ref.QUAD_GAP) <= 0.02 * ref.QUAD_GAP                  # the recorded gap is the measured one
    assert ref.QUAD_BOUND == 2.0 * ref.QUAD_GAP and max(gap) <= ref.QUAD_BOUND
