"""The batched PSIS leave-one-out without a GPU: the restatement (tests/psis_loo_ref.py) pinned to the closed-form leave-one-out
density of the conjugate Gaussian model; its float64 noise floor on the GPU tests' inputs (the bar of tests/test_gpu_psis_loo.py is
1000 times it); the host logic of ``psis_loo_batched`` on a stand-in engine; the tile helper, the C ABI declarations and the
argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import glm_batched_ref as gref
import psis_batched_ref as pref
import psis_loo_ref as ref
from gsmvi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsmvi_psis_loo_batched_f64"


# ---- 1. the Gaussian family with q the exact posterior -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def gaussian_runs():
    """per (N, D): the largest |elpd_i - closed form|, the largest pointwise khat, sum p_loo and the problem-level khat over
    the seeds, and the largest pointwise khat with q widened 1.5 times"""
    out = {}
    for N, D in ref.GAUSS_SHAPES:
        gap, khat, ploo, top, wide = [], [], [], [], []
        for seed in ref.GAUSS_SEEDS:
            p = ref.gaussian_exact_problem(N, D, seed)
            r, t = ref.gaussian_restatement_run(p, ref.GAUSS_S)
            assert (r["info"] == 0).all()
            gap.append(np.abs(np.asarray(r["elpd"], dtype=np.float64) - ref.gaussian_exact_loo(p)).max())
            khat.append(float(np.max(r["khat"])))
            ploo.append(float((r["lpd"] - r["elpd"]).sum()))
            top.append(t)
            w, _ = ref.gaussian_restatement_run(ref.gaussian_exact_problem(N, D, seed), ref.GAUSS_S, widen=1.5)
            wide.append(float(np.max(w["khat"])))
        out[N, D] = dict(gap=max(gap), khat=max(khat), ploo=ploo, top=max(top), wide=max(wide))
    return out


@pytest.mark.parametrize("shape", ref.GAUSS_SHAPES)
def test_exact_gaussian_posterior_gives_the_closed_form_loo_density(gaussian_runs, shape):
    """elpd_i against log N(y_i | a_i . m_-i, 1 / tau + a_i^T Sigma_-i a_i): a Monte-Carlo gap, bounded by twice the largest
    measured over the seeds (psis_loo_ref.GAUSS_GAP: 0.082, 0.070, 0.058); 0 < sum p_loo < 2 D; the problem-level khat is below 0
    (q is the target); with q widened 1.5 times every pointwise khat is below 0.7 (measured at most 0.35)"""
    g = gaussian_runs[shape]
    D = shape[1]
    print(f"(N, D) = {shape}: gap {g['gap']:.4f}, largest khat {g['khat']:.2f}, sum p_loo / D {min(g['ploo']) / D:.2f} .. "
          f"{max(g['ploo']) / D:.2f}, problem-level khat <= {g['top']:.2f}, widened: khat <= {g['wide']:.2f}")
    assert abs(g["gap"] - ref.GAUSS_GAP[shape]) <= 0.02 * ref.GAUSS_GAP[shape]       # the recorded gap is the measured one
    assert ref.GAUSS_BOUND[shape] == 2.0 * ref.GAUSS_GAP[shape] and g["gap"] <= ref.GAUSS_BOUND[shape]
    assert all(0.0 < s < 2.0 * D for s in g["ploo"])
    assert g["top"] < 0.0
    assert g["wide"] < 0.7


# ---- 2. the noise floor that sets the GPU tests' bar ---------------------------------------------------------------------------
def test_float64_noise_floor_of_the_restatement_on_the_gpu_inputs():
    """the restatement in float64 against itself in longdouble on every case of the GPU tests (both fed the float64 l_si),
    relative to max(1, |value|), rows whose verdict differs left out (at most 1 % of them): measured 1.42e-14 at the most (ess);
    l_si itself differs by 1.4e-15.  The GPU bar is 1000 times the recorded floor."""
    worst, rows, differ = {}, 0, 0
    for c in ref.CASES:
        p = ref.make_case(c)
        args = (p["family"], p["A"], p["y"], p["offset"], p["counts"], p["tau"], p["X"])
        ell = np.asarray(ref.loglik(*args, np.float64), dtype=np.float64)
        worst["loglik"] = max(worst.get("loglik", 0.0), pref.rel_gap(ell, ref.loglik(*args)))
        a = ref.loo_batched(ell, p["logr"], p["lw"], p["counts"], np.float64)
        b = ref.loo_batched(ell, p["logr"], p["lw"], p["counts"])
        same = a["info"] == b["info"]
        rows += same.size
        differ += int((~same).sum())
        for n in ("elpd", "lpd", "khat", "ess"):
            worst[n] = max(worst.get(n, 0.0), ref.rel_gap(a[n], b[n], same))
    print("float64 against longdouble:", {n: f"{g:.2e}" for n, g in worst.items()}, f"; verdict differs in {differ} of {rows} rows")
    assert differ <= 0.01 * rows
    assert worst.pop("loglik") <= 1e-13                                       # (far inside the single-launch bar of 1e-11)
    floor = max(worst.values())
    assert floor <= ref.NOISE_FLOOR <= 2.0 * floor                            # the recorded floor is the measured one, rounded up
    assert ref.BAR == 1000 * ref.NOISE_FLOOR and ref.BAR < 1e-8 and ref.LOGLIK_BAR == 1e-11


def test_the_cases_cover_every_axis_value():
    fams, offs, Ds, Ss, Ns, Ks = (set(c[i] for c in ref.CASES) for i in range(6))
    assert fams == set(ref.FAMILIES) and offs == {False, True} and Ks == {1, 3}
    assert Ds >= {1, 2, 15, 16, 17, 33, 64} and Ss == {5, 33, 257, 1024, 4096} and Ns == set(ref.N_OF)
    for fam in ref.FAMILIES:
        assert {c[1] for c in ref.CASES if c[0] == fam} == {False, True}, fam
    for D in (10, 64):                                                        # the N edges at two values of D
        assert {c[4] for c in ref.CASES if c[2] == D and c[3] == 33} == set(ref.N_OF)
    p = ref.make_case(ref.CASES[2])
    assert list(p["counts"]) == [0, max(1, p["N"] // 2), p["N"]]
    assert ref.make_case(ref.CASES[-1])["N"] == 3 and ref.loo_tile(64, 4096) == 2


# ---- 3. the outcomes of the definition -----------------------------------------------------------------------------------------
def test_verdicts_touch_only_their_own_row():
    p = ref.make_case(("poisson", True, 10, 33, "2NI+3", 3))
    ell = np.asarray(ref.loglik(p["family"], p["A"], p["y"], p["offset"], None, p["tau"], p["X"]), dtype=np.float64)
    clean = ref.loo_batched(ell, p["logr"], p["lw"])
    dirty_ell, logr = ell.copy(), p["logr"].copy()
    dirty_ell[0, 2, 5] = np.nan                                               # a flagged draw of one row
    logr[1, 3] = np.nan                                                       # a failed problem-level run
    r = ref.loo_batched(dirty_ell, logr, p["lw"])
    assert r["info"][0, 2] == -1 and (r["info"][1] == -1).all()
    for n in ("elpd", "lpd", "khat", "ess"):
        assert np.isnan(r[n][0, 2]) and np.isnan(r[n][1]).all()
        keep = np.ones(r[n].shape, dtype=bool)
        keep[0, 2] = keep[1] = False
        assert np.array_equal(r[n][keep], clean[n][keep]), n
    assert np.array_equal(r["info"][2], clean["info"][2])
    # a row beyond the count: NaN and -3
    short = ref.loo_batched(ell, p["logr"], p["lw"], np.array([11, 4, 0]))
    assert (short["info"][1, 4:] == -3).all() and (short["info"][2] == -3).all() and np.isnan(short["elpd"][1, 4:]).all()
    assert np.array_equal(short["elpd"][1, :4], clean["elpd"][1, :4])
    # fewer than five distinct ratios: -2, khat = +inf, plain self-normalised weights: elpd is the harmonic form
    flat = ref.loo_rows(np.full((1, 33), -1.25), np.full(33, 0.5), np.full(33, -np.log(33.0)), 1)
    assert flat["info"][0] == -2 and np.isposinf(flat["khat"][0]) and abs(float(flat["elpd"][0]) + 1.25) < 1e-15


# ---- 4. host logic on the stand-in engine --------------------------------------------------------------------------------------
def _fitted(K=3, N=12, D=4, family="logistic", counts=(12, 0, 7), seed=3):
    import gsmvi_amd
    A, y, offset, _, _, tau, _ = gref.make_inputs(family, K, N, D, 1, seed=seed)
    eng = ref.StandInEngine()
    tgt = gsmvi_amd.BatchedGLMTarget(A, y, family, 1.0, counts=None if counts is None else np.array(counts), offset=offset,
                                     noise_precision=tau, engine=eng)
    rs = np.random.RandomState(seed)
    mean = 0.3 * rs.standard_normal((K, D))
    G = rs.standard_normal((K, D, D))
    cov = np.linalg.inv(np.eye(D)[None] + 0.25 * np.swapaxes(A, 1, 2) @ A + 0.05 * G @ np.swapaxes(G, 1, 2))
    return tgt, eng, mean, 0.5 * (cov + np.swapaxes(cov, 1, 2))


def test_psis_loo_batched_protocol_and_summaries():
    import gsmvi_amd
    tgt, eng, mean, cov = _fitted()
    K, N, D, S = 3, 12, 4, 40
    keys = [5, 6, 7]
    m0, c0 = mean.copy(), cov.copy()
    r = gsmvi_amd.psis_loo_batched(tgt, mean, cov, keys, num_draws=S, call=2, pointwise_loglik=True)
    assert isinstance(r, gsmvi_amd.LOOBatchedResult) and r.nlaunch == 3 and r.threshold == pref.threshold(S)
    assert np.array_equal(mean, m0) and np.array_equal(cov, c0)
    launches = [c for c in eng.calls if isinstance(c, tuple)]
    seeds = tuple((k % 2 ** 32) ^ 0x5DEECE66D for k in keys)
    assert launches == [("draw", seeds, 2, 0, S), ("glm", "logistic", "lp"), ("psis", (K, S, D), False),
                        ("loo", "logistic", (K, S, D), (K, N, D), True, True, True)]
    # the problem-level run is psis_batched's, and the pointwise outputs are the restatement on its draws
    top = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, call=2, moments=False, engine=ref.StandInEngine())
    assert np.array_equal(r.psis.khat, top.khat) and np.array_equal(r.psis.samples, top.samples)
    cnt = np.array([12, 0, 7])
    ell = np.asarray(ref.loglik("logistic", tgt.A, tgt.y, tgt.offset, cnt, 1.0, top.samples), dtype=np.float64)
    want = ref.loo_batched(ell, top.log_ratios, top.log_weights, cnt)
    assert np.array_equal(r.loglik, ell, equal_nan=True) and r.loglik.shape == (K, N, S)
    for got, n in ((r.elpd_i, "elpd"), (r.lpd_i, "lpd"), (r.khat, "khat"), (r.ess, "ess")):
        assert isinstance(got, np.ndarray) and np.array_equal(got, np.asarray(want[n], dtype=np.float64), equal_nan=True), n
    assert np.array_equal(r.info, want["info"]) and r.info.dtype == np.int64
    assert (r.info[0] != -3).all() and (r.info[1] == -3).all() and (r.info[2, 7:] == -3).all()
    # the per-problem summaries under the mask of the counts
    s = ref.summaries(want, cnt, S)
    for n in ("elpd_loo", "p_loo", "se"):
        assert np.allclose(getattr(r, n), s[n], rtol=1e-13, atol=0, equal_nan=True), n
    assert r.elpd_loo[1] == 0.0 and np.isnan(r.se[1]) and r.n_bad[1] == 0
    assert abs(r.elpd_loo[2] - r.elpd_i[2, :7].sum()) < 1e-12 and abs(r.p_loo[0] - (r.lpd_i[0] - r.elpd_i[0]).sum()) < 1e-12
    assert abs(r.se[0] - np.sqrt(12 * np.var(r.elpd_i[0], ddof=1))) < 1e-12
    assert np.array_equal(r.n_bad, s["n_bad"])
    assert np.array_equal(r.ok, np.asarray(r.psis.ok) & (r.n_bad == 0)) and r.ok.dtype == bool
    # psis= reuses the draws: one launch, the same numbers; no pointwise block unless asked for
    eng.calls.clear()
    again = gsmvi_amd.psis_loo_batched(tgt, mean, cov, keys, psis=r.psis)
    assert [c[0] for c in eng.calls if isinstance(c, tuple)] == ["loo"] and again.nlaunch == 1 and again.loglik is None
    for n in ("elpd_loo", "p_loo", "se", "elpd_i", "lpd_i", "khat", "ess", "info", "n_bad", "ok"):
        assert np.array_equal(getattr(again, n), getattr(r, n), equal_nan=True), n
    # the method of the target forwards
    via = tgt.loo(mean, cov, keys, num_draws=S, call=2)
    assert np.array_equal(via.elpd_i, r.elpd_i, equal_nan=True) and via.nlaunch == 3


def test_argument_errors_come_before_any_engine_call():
    import dataclasses
    import torch
    import gsmvi_amd
    tgt, eng, mean, cov = _fitted()
    eng.calls.clear()
    loo = lambda *a, **kw: gsmvi_amd.psis_loo_batched(tgt, *a, **kw)          # noqa: E731
    for bad in (object(), gsmvi_amd.psis_batched, None):
        with pytest.raises(TypeError, match="BatchedGLMTarget"):
            gsmvi_amd.psis_loo_batched(bad, mean, cov, [1, 2, 3])
    with pytest.raises(ValueError, match="mean must be"):
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
        gsmvi_amd.psis_loo_batched(tgt, mean, cov, [1, 2, 3], psis=good, engine=Device())


# ---- 5. the tile helper and the C ABI ------------------------------------------------------------------------------------------
def test_tile_helper_matches_its_formula():
    lib = _lib.load_library()
    for D in (1, 64):
        for S in (5, 1024, 1025, 4096):
            assert lib.gsmvi_psis_loo_tile(D, S) == ref.loo_tile(D, S) >= 1, (D, S)
    assert ref.loo_tile(64, 4096) == 2 and ref.loo_tile(1, 4096) == 2 and ref.loo_tile(64, 1024) == ref.NI_CAP == ref.loo_tile(1, 5)
    for D in (1, 10, 16, 17, 33, 64):
        for S in (5, 8, 9, 33, 257, 2048, 2049, 3000, 4095):
            assert lib.gsmvi_psis_loo_tile(D, S) == ref.loo_tile(D, S) >= 1, (D, S)
    for D, S in ((0, 8), (65, 8), (4, 4), (4, 4097)):
        assert lib.gsmvi_psis_loo_tile(D, S) == 0 == ref.loo_tile(D, S)


def test_loo_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name, nargs in ((NAME, 22), ("gsmvi_psis_loo_tile", 2)):
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
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_LOO\s+0x400000u", hdr)
    mask = re.search(r"#define\s+GSMVI_PATH_GENERIC_MASK\s+\(([^)]*)\)", hdr).group(1)
    assert "0x400000" not in mask and "#define GSMVI_ABI_VERSION 1" in hdr
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_loo"] == ref.PATH_BIT == 0x400000 and not HipEngine.PATH_GENERIC_MASK & 0x400000
    assert len(set(HipEngine.PATH_BITS.values())) == len(HipEngine.PATH_BITS)
    assert _lib.load_library().gsmvi_abi_version() == 1
    import gsmvi_amd
    for name in ("psis_loo_batched", "LOOBatchedResult"):
        assert getattr(gsmvi_amd, name) is not None and name in gsmvi_amd.__doc__
    assert gsmvi_amd.BatchedLogisticTarget.loo is gsmvi_amd.BatchedGLMTarget.loo


def test_abi_checks_arguments_before_the_context():
    ref.check_bad_arguments(_lib.load_library())
