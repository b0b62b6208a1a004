"""The batched GLM posterior predictive without a GPU: the longdouble restatement (tests/glm_predict_ref.py) pinned to closed
forms and to brute-force quadrature, in two bands of the predictor's variance; the band of the GPU tests' problems; the end-to-end
property of the GPU test on the restatement alone; the C ABI declaration and argument checks of gsmvi_glm_predict_batched_f64;
and the host logic of ``predict`` on a stand-in engine."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from scipy import integrate, special, stats

import glm_batched_ref as gref
import glm_predict_ref as ref
import laplace_batched_ref as lref
from gsmvi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsmvi_glm_predict_batched_f64"
BANDS = {"v <= 1": (0.0, 1.0), "1 < v <= 4": (1.0, 4.0)}


def _band(name, n, seed=0):
    lo, hi = BANDS[name]
    rs = np.random.RandomState(seed)
    return rs.uniform(-3.0, 3.0, n), rs.uniform(lo, hi, n)


# ---- 1. the restatement against closed forms ---------------------------------------------------------------------------------
def test_restatement_matches_the_closed_forms():
    """gaussian lpd and mean (scipy.stats.norm), probit and poisson means (a 200-node quadrature of the inverse link: they are
    closed-form in the restatement), 1e-13 relative to max(1, |value|); measured <= 2e-15"""
    for band in BANDS:
        m, v = _band(band, 2000)
        rs = np.random.RandomState(1)
        y, tau = m + rs.standard_normal(m.shape), 0.7
        pm, lpd = ref.rows("gaussian", m, v, y, tau=tau)
        want = stats.norm.logpdf(y, loc=m, scale=np.sqrt(v + 1.0 / tau))
        e = float((np.abs(lpd - want) / np.maximum(1.0, np.abs(want))).max())
        assert np.array_equal(np.asarray(pm, dtype=np.float64), m) and e <= 1e-13, (band, e)
        t, w = np.polynomial.hermite.hermgauss(200)
        eta = m[:, None] + np.sqrt(2.0 * v)[:, None] * t
        for fam, inv in (("probit", special.ndtr), ("poisson", np.exp)):
            pm, _ = ref.rows(fam, m, v)
            want = (w * inv(eta)).sum(1) / np.sqrt(np.pi)
            e2 = float((np.abs(pm - want) / np.maximum(1.0, np.abs(want))).max())
            print(f"{band}: gaussian lpd {e:.1e}, {fam} mean {e2:.1e}")
            assert e2 <= 1e-13, (band, fam, e2)


@pytest.mark.parametrize("band,bound", [("v <= 1", 1e-12), ("1 < v <= 4", 1e-5)])
def test_probit_lpd_is_log_phi_within_the_band(band, bound):
    """log Phi(+-m / sqrt(1 + v)) for y in {0, 1} at Q = 32: measured 2.6e-15 for v <= 1 and 6.9e-7 for 1 < v <= 4"""
    m, v = _band(band, 4000)
    worst = 0.0
    for yv in (0.0, 1.0):
        _, lpd = ref.rows("probit", m, v, np.full(m.shape, yv))
        z = m / np.sqrt(1.0 + v)
        worst = max(worst, float(np.abs(lpd - special.log_ndtr(z if yv else -z)).max()))
    print(f"probit lpd, {band}: worst error {worst:.2e}")
    assert worst <= bound


# ---- 2. the restatement against brute-force quadrature ---------------------------------------------------------------------
# measured at Q = 32 (this file, printed below); the bounds are ten times the measured worst
LOGISTIC_BOUNDS = {"v <= 1": (1e-12, 2.5e-12), "1 < v <= 4": (1.3e-6, 3.8e-6)}      # (mean, lpd); measured 9.5e-14, 2.5e-13; 1.3e-7, 3.8e-7
POISSON_BOUNDS = {"v <= 1": 1.5e-3, "1 < v <= 4": 0.45}                           # lpd, y in {0, 1, 3}; measured 1.5e-4, 4.5e-2


@pytest.mark.parametrize("band", list(BANDS))
def test_logistic_quadrature_against_200_nodes(band):
    m, v = _band(band, 4000)
    bm, bl = LOGISTIC_BOUNDS[band]
    em = el = 0.0
    for yv in (0.0, 1.0, 0.3):
        y = np.full(m.shape, yv)
        p32, l32 = ref.rows("logistic", m, v, y, Q=32)
        p200, l200 = ref.rows("logistic", m, v, y, Q=200)
        em, el = max(em, float(np.abs(p32 - p200).max())), max(el, float(np.abs(l32 - l200).max()))
    print(f"logistic, {band}: mean {em:.2e}, lpd {el:.2e} against 200 nodes")
    assert em <= bm and el <= bl


@pytest.mark.parametrize("band", list(BANDS))
def test_poisson_lpd_against_adaptive_quadrature(band):
    """the poisson integrand e^(y eta - e^eta) is no polynomial times a Gaussian for long: at Q = 32 the lpd is off by 1.5e-4
    for v <= 1 and by 4.5e-2 for 1 < v <= 4 (y <= 3, m in [-3, 3]); the error grows with y (1e-2 at y = 10, v = 1)"""
    lo, hi = BANDS[band]
    worst = 0.0
    for m in np.linspace(-3.0, 3.0, 7):
        for v in np.linspace(max(lo, 0.05) if lo == 0.0 else lo + 0.25, hi, 4):
            for yv in (0.0, 1.0, 3.0):
                f = lambda e: np.exp(yv * e - np.exp(e) - special.gammaln(yv + 1.0) - (e - m) ** 2 / (2 * v)) / np.sqrt(2 * np.pi * v)  # noqa: E731
                val, _ = integrate.quad(f, m - 12 * np.sqrt(v), m + 12 * np.sqrt(v), epsabs=0, epsrel=1e-12, limit=400)
                l32 = float(ref.rows("poisson", [m], [v], [yv], Q=32)[1][0])
                worst = max(worst, abs(l32 - np.log(val)))
    print(f"poisson lpd, {band}: worst error {worst:.2e} against adaptive quadrature")
    assert worst <= POISSON_BOUNDS[band]


# ---- 3. the problems of the GPU tests ----------------------------------------------------------------------------------------
def test_gpu_problems_stay_in_the_accurate_band_and_counts_cover_zero_mid_and_all():
    seen = set()
    for family in ref.FAMILIES:
        for shape in ref.SHAPES:
            for off in (True, False):
                p, r = ref.reference(family, shape, off)
                D, M, K = shape
                live = np.arange(M)[None, :] < p["counts"][:, None]
                assert (r["eta_var"][live] <= 1.0).all() and (r["eta_var"][live] >= 0.0).all(), (family, shape)
                assert np.isfinite(r["lpd"][live]).all() and np.isnan(r["lpd"][~live]).all()
                assert np.isfinite(r["elpd"]).all()
                seen |= {"zero" if c == 0 else "all" if c == M else "mid" for c in p["counts"]}
    assert seen == {"zero", "mid", "all"}
    assert {s[0] for s in ref.SHAPES} >= {1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64}
    assert {s[1] for s in ref.SHAPES} >= {1, 31, 32, 33, 65} and {s[2] for s in ref.SHAPES} == {1, 3, 7}


def test_end_to_end_property_holds_on_the_restatement_alone():
    """the Laplace Gaussian scores a higher held-out elpd than the same mean with 25 times the covariance, on every problem"""
    (A, y, lam), (An, yn) = ref.e2e_problem()
    K, _, D = A.shape
    mean, cov = np.empty((K, D)), np.empty((K, D, D))
    for k in range(K):
        p = lref.problem("logistic", A, y, None, None, lam, 1.0, k)
        s = lref.run(p, np.zeros(D))
        assert s["status"] == 1
        mean[k] = s["x"]
        cov[k], info = lref.inverse(lref.evaluate(p, s["x"])[2])
        assert info == 0
    a = ref.predict("logistic", An, None, yn, None, 1.0, mean, cov)
    b = ref.predict("logistic", An, None, yn, None, 1.0, mean, 25.0 * cov)
    print("elpd(laplace) - elpd(25 cov):", np.array2string(a["elpd"] - b["elpd"], precision=3))
    assert (a["eta_var"] <= 4.0).all()                               # (measured 1.9: the quadrature's 4e-7 band)
    assert (a["elpd"] > b["elpd"] + 0.5).all()                       # (measured 0.84 at the least: far above any rounding)


def test_restatement_nan_rules_and_counts():
    for family in ref.FAMILIES:
        p = ref.make_problem(family, 3, 9, 4)
        base = ref.predict(family, p["A"], p["offset"], p["y"], p["counts"], p["tau"], p["mean"], p["cov"])
        A2, y2, o2 = p["A"].copy(), p["y"].copy(), p["offset"].copy()
        for k in range(3):
            A2[k, p["counts"][k]:] = np.nan
            y2[k, p["counts"][k]:] = np.nan
            o2[k, p["counts"][k]:] = np.nan
        again = ref.predict(family, A2, o2, y2, p["counts"], p["tau"], p["mean"], p["cov"])
        for name in ("eta_mean", "eta_var", "mean", "lpd", "elpd"):
            assert np.array_equal(base[name], again[name], equal_nan=True), (family, name)
        assert base["elpd"][1] == 0.0 and np.isnan(base["lpd"][1]).all()             # counts[1] = 0
        m2 = p["mean"].copy()
        m2[2, 1] = np.nan
        c = ref.predict(family, p["A"], p["offset"], p["y"], p["counts"], p["tau"], m2, p["cov"])
        assert np.isnan(c["elpd"][2]) and all(np.isnan(c[n][2]).all() for n in ("eta_mean", "eta_var", "mean", "lpd"))
        assert all(np.array_equal(c[n][:2], base[n][:2], equal_nan=True) for n in ("eta_mean", "eta_var", "mean", "lpd", "elpd"))
        neg = ref.predict(family, p["A"], p["offset"], p["y"], p["counts"], p["tau"], p["mean"], -p["cov"])
        zero = ref.predict(family, p["A"], p["offset"], p["y"], p["counts"], p["tau"], p["mean"], 0.0 * p["cov"])
        live = np.arange(9)[None, :] < p["counts"][:, None]
        assert (neg["eta_var"][live] < 0.0).all() and (zero["eta_var"][live] == 0.0).all()
        assert np.array_equal(neg["mean"], zero["mean"], equal_nan=True) and np.array_equal(neg["lpd"], zero["lpd"], equal_nan=True)


# ---- 4. the C ABI --------------------------------------------------------------------------------------------------------------
def test_predict_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr)
    for mp in ("exports.map", "exports_debug.map"):
        assert re.search(r"^\s*" + NAME + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), mp
    assert NAME in _lib.exported_symbols() and NAME in built
    head = hdr.split("#ifndef GSMVI_HIP_H")[0]
    assert NAME in head
    block = hdr[:hdr.index("int " + NAME)].rsplit("/*", 1)[1]
    assert "example_gsm.py:34-35" in block and "GSMVI_PATH_BATCHED_PREDICT" in block
    res, args = _lib._SIGS[NAME]
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert res is C.c_int and len(args) == len(params) == 22
    for p, a in zip(params, args):
        want = C.c_double if p.startswith("double ") else C.c_int64 if p.startswith("int64_t") else \
            C.c_int if p.startswith("int ") else C.c_void_p
        assert a is want, (p, a)
    assert params[4] == "int64_t M" and params[5] == "int family" and params[14] == "int Q"
    from gsmvi_amd.engine import HipEngine
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_PREDICT\s+0x100000u", hdr)
    assert HipEngine.PATH_BITS["batched_predict"] == 0x100000 and not HipEngine.PATH_GENERIC_MASK & 0x100000
    assert len(set(HipEngine.PATH_BITS.values())) == len(HipEngine.PATH_BITS)
    assert _lib.load_library().gsmvi_abi_version() == 1
    import gsmvi_amd
    assert gsmvi_amd.GLMPrediction is not None and "GLMPrediction" in gsmvi_amd.__doc__
    src = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_glm_predict_batched.hip")).read()
    assert "lb_link<" in src and "erfcx" not in src and "log1p" not in src           # the link is called, not restated


def test_abi_checks_arguments_before_the_context():
    ref.check_bad_arguments(_lib.load_library())


def test_engine_table_is_hermgauss_rounded_to_double():
    from gsmvi_amd.engine import HipEngine
    for Q in (1, 7, 32, 64):
        t, lw = HipEngine.gauss_hermite(Q)
        t2, lw2 = ref.gh_table(Q)
        assert t.dtype == lw.dtype == np.float64 and np.array_equal(t, t2) and np.array_equal(lw, lw2)
        assert np.isfinite(lw).all() and abs(np.exp(lw).sum() - np.sqrt(np.pi)) < 1e-14


# ---- 5. host logic of predict --------------------------------------------------------------------------------------------------
def _targets(family, p, eng, with_offset=False):
    from gsmvi_amd import BatchedGLMTarget, BatchedLogisticTarget
    tau = p["tau"]
    out = [BatchedGLMTarget(p["A"], p["y"], family, 1.0, offset=p["offset"] if with_offset else None, noise_precision=tau, engine=eng)]
    if family == "logistic":
        out.append(BatchedLogisticTarget(p["A"], p["y"], 1.0, engine=eng))
    return out


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_predict_validates_on_the_host_before_the_engine_is_touched(family):
    eng = ref.StandInEngine()
    K, M, D = 3, 9, 4
    p = ref.make_problem(family, K, M, D)
    train = ref.make_problem(family, K, 12, D, seed=5)
    train["tau"] = p["tau"]
    for tgt in _targets(family, train, eng, with_offset=True):
        base = dict(mean=p["mean"], cov=p["cov"], A_new=p["A"], offset=p["offset"], y=p["y"], counts=p["counts"], nodes=32)

        def bad(match, **kw):
            args = dict(base)
            for k, v in kw.items():
                args[k] = v(args[k]) if callable(v) else v
            eng.calls.clear()
            with pytest.raises(ValueError, match=match):
                tgt.predict(**args)
            assert eng.calls == [], (match, kw)

        def put(k, n, v):
            def f(arr):
                arr = np.array(arr, dtype=np.float64)
                arr[k, n] = v
                return arr
            return f

        for q in (0, 65, -1, 32.0, None, True):
            bad("^nodes:", nodes=q)
        bad("^A_new:", A_new=lambda A: A[:2])
        bad("^A_new:", A_new=lambda A: A[:, :, :3])
        bad("^A_new:", A_new=lambda A: A[0])
        bad("^A_new:", A_new=lambda A: A[:, :0])
        bad("^mean:", mean=lambda m: m[:2])
        bad("^mean:", mean=lambda m: m[:, :3])
        bad("^cov:", cov=lambda c: c[:, :, :3])
        bad("^cov:", cov=lambda c: c[0])
        bad("^y:", y=lambda y: y[:, :8])
        for badc in ([9, 10, 1], [-1, 2, 3], [1, 2], [1.5, 2.0, 3.0]):
            bad("^counts:", counts=badc)
        bad(r"^counts: values outside 0 \.\. M = 9 for problems \[1\]", counts=[9, 10, 1])
        values = {"logistic": (-0.01, 1.01, np.nan), "probit": (-0.01, np.inf), "poisson": (-0.5, np.nan, np.inf),
                  "gaussian": (np.nan, -np.inf)}[family]
        for v in values:
            bad(r"^y: .*\[2\]", y=put(2, 0, v))                         # counts = (9, 0, 4): row 0 of problem 2 counts
        bad("^offset:", offset=lambda o: o[:, :8])
        bad(r"^offset: expected shape \(K, M\)", offset=lambda o: o.T)
        for v in (np.nan, np.inf):
            bad(r"^offset: .*\[2\]", offset=put(2, 3, v))
        # the message of y is the constructor's own for the class
        with pytest.raises(ValueError) as ei:
            tgt.predict(**dict(base, y=put(2, 0, np.nan)(p["y"])))
        assert ("(family" in str(ei.value)) == (type(tgt).__name__ == "BatchedGLMTarget")
        # beyond the valid rows anything goes; a row of problem 1 (counts 0) too
        y2, o2 = p["y"].copy(), p["offset"].copy()
        y2[1, :] = np.nan
        o2[2, 4:] = np.inf
        eng.calls.clear()
        r = tgt.predict(p["mean"], p["cov"], p["A"], offset=o2, y=y2, counts=p["counts"])
        assert [c for c in eng.calls if isinstance(c, tuple)] == [("predict", family, True, True, True, 32)]
        want = ref.predict(family, p["A"], p["offset"], p["y"], p["counts"], p["tau"], p["mean"], p["cov"])
        for name in ("eta_mean", "eta_var", "mean", "lpd", "elpd"):
            assert np.array_equal(getattr(r, name), want[name], equal_nan=True), name


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_predict_protocol_on_the_stand_in_engine(family):
    import gsmvi_amd
    eng = ref.StandInEngine()
    p = ref.make_problem(family, 3, 9, 4)
    train = ref.make_problem(family, 3, 12, 4, seed=5)
    train["tau"] = p["tau"]
    for tgt in _targets(family, train, eng, with_offset=True):
        # a target built with an offset does not require one here; without y there is no lpd
        eng.calls.clear()
        r = tgt.predict(p["mean"], p["cov"], p["A"], nodes=16)
        assert isinstance(r, gsmvi_amd.GLMPrediction) and r.lpd is None and r.elpd is None
        assert [c for c in eng.calls if isinstance(c, tuple)] == [("predict", family, False, False, False, 16)]
        want = ref.predict(family, p["A"], None, None, None, p["tau"], p["mean"], p["cov"], Q=16)
        assert all(isinstance(getattr(r, n), np.ndarray) for n in ("eta_mean", "eta_var", "mean"))
        assert np.array_equal(r.eta_mean, want["eta_mean"]) and np.array_equal(r.eta_var, want["eta_var"])
        assert np.array_equal(r.mean, want["mean"])
        # tensors and float32 data in; lists as counts
        r2 = tgt.predict(torch.tensor(p["mean"]), torch.tensor(p["cov"]), torch.tensor(p["A"], dtype=torch.float32),
                         y=torch.tensor(p["y"]), counts=[int(c) for c in p["counts"]])
        w2 = ref.predict(family, p["A"].astype(np.float32), None, p["y"], p["counts"], p["tau"], p["mean"], p["cov"])
        assert np.array_equal(np.asarray(r2.lpd), w2["lpd"], equal_nan=True) and np.array_equal(np.asarray(r2.elpd), w2["elpd"])
    # the constructors still validate as before, through the shared checks
    with pytest.raises(ValueError, match=r"^counts: values outside 0 \.\. N = 12 for problems \[0\]"):
        gsmvi_amd.BatchedGLMTarget(train["A"], train["y"], family, counts=[13, 1, 1], engine=eng)
    with pytest.raises(ValueError, match=r"^offset: expected shape \(K, N\) = \(3, 12\)"):
        gsmvi_amd.BatchedGLMTarget(train["A"], train["y"], family, offset=train["offset"][:, :5], engine=eng)
