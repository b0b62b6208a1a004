"""The batched softmax PSIS leave-one-out without a GPU: the restatement of l_si (tests/psis_loo_softmax_ref.py) against a direct
torch evaluation and, at two classes, against the logistic family of psis_loo_ref; its float64 noise floor on the GPU tests' inputs
(the bar of tests/test_gpu_psis_loo_softmax.py is 1000 times it); the tile helper and the grid bound; the host logic of
``psis_loo_softmax_batched`` on a stand-in engine; elpd_i against the leave-one-out density by 2-D quadrature; the C ABI
declarations and the argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import glm_batched_ref as gref
import psis_batched_ref as pref
import psis_loo_ref as lref
import psis_loo_softmax_ref as ref
from gsmvi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsmvi_psis_loo_softmax_batched_f64"
TILE = "gsmvi_psis_loo_softmax_tile"


# ---- 1. the restatement of l_si ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in ref.CASES if c[2] <= 257], ids=ref.case_id)
def test_restatement_is_the_direct_evaluation(case):
    """float64 l_si against torch's log_softmax of the linear predictors with the zero column appended, picked at the label:
    within 1e-12 relative to max(1, |value|)"""
    p = ref.make_case(case)
    got = np.asarray(ref.loglik_softmax(p["A"], p["y"], p["C"], p["counts"], p["X"], np.float64), dtype=np.float64)
    K, N, S, Cc, P = p["K"], p["N"], p["S"], p["C"], p["P"]
    A, X = torch.as_tensor(p["A"]), torch.as_tensor(p["X"])
    eta = torch.einsum("knp,kscp->knsc", A, X.reshape(K, S, Cc - 1, P))
    eta = torch.cat([eta, torch.zeros(K, N, S, 1, dtype=eta.dtype)], dim=3)
    idx = torch.as_tensor(p["y"]).long()[:, :, None, None].expand(K, N, S, 1)
    want = torch.log_softmax(eta, dim=3).gather(3, idx)[..., 0].numpy()
    nk = ref.valid_rows(p["counts"], K, N)
    want = np.where((np.arange(N)[None, :] < nk[:, None])[:, :, None], want, np.nan)
    assert pref.rel_gap(got, want) <= 1e-12


def test_two_classes_are_the_logistic_family():
    """C = 2, P = D: l_si of the softmax restatement against psis_loo_ref.loglik("logistic", ...) with y = [label == 0]: 1e-13"""
    for case in (ref.CASES[0], ref.CASES[6]):
        p = ref.make_case(case)
        assert p["C"] == 2
        y = (p["y"] == 0).astype(np.float64)
        for dtype in (np.float64, ref.LD):
            a = ref.loglik_softmax(p["A"], p["y"], 2, p["counts"], p["X"], dtype)
            b = lref.loglik("logistic", p["A"], y, None, p["counts"], 1.0, p["X"], dtype)
            assert pref.rel_gap(a, b) <= 1e-13, (case, dtype)


def test_restatement_nan_rules_and_counts():
    """a non-finite entry of x_s, a dot product that is not finite and a label outside 0 .. C - 1 give NaN, nothing else does; rows
    i >= n_k are NaN"""
    p = ref.make_case(ref.CASES[2])                                           # (3, 5): K = 3, counts (0, partial, N)
    K, N, S = p["K"], p["N"], p["S"]
    clean = ref.loglik_softmax(p["A"], p["y"], 3, p["counts"], p["X"], np.float64)
    nk = ref.valid_rows(p["counts"], K, N)
    mask = np.arange(N)[None, :] < nk[:, None]
    assert np.isfinite(clean[mask]).all() and np.isnan(clean[~mask]).all() and (clean[mask] < 0).all()
    X = p["X"].copy()
    X[2, 7, 9] = np.inf                                                       # the last column of the last class of one draw
    X[2, 8, 0] = np.nan
    bad = ref.loglik_softmax(p["A"], p["y"], 3, p["counts"], X, np.float64)
    assert np.isnan(bad[2, :, 7]).all() and np.isnan(bad[2, :, 8]).all()
    keep = np.ones(S, dtype=bool)
    keep[[7, 8]] = False
    assert np.array_equal(bad[:, :, keep], clean[:, :, keep], equal_nan=True)
    A = p["A"].copy()
    A[2, 1, 2] = np.inf                                                       # a row of A: its dot products are not finite
    bad = ref.loglik_softmax(A, p["y"], 3, p["counts"], p["X"], np.float64)
    assert np.isnan(bad[2, 1]).all() and np.array_equal(np.delete(bad[2], 1, 0), np.delete(clean[2], 1, 0))
    y = p["y"].copy()
    y[2, 0], y[2, 3] = 3, -1
    bad = ref.loglik_softmax(p["A"], y, 3, p["counts"], p["X"], np.float64)
    assert np.isnan(bad[2, 0]).all() and np.isnan(bad[2, 3]).all() and np.array_equal(bad[2, 1:3], clean[2, 1:3])
    # the reference class: eta_y = 0
    y = np.full_like(p["y"], 2)
    ell = ref.loglik_softmax(p["A"], y, 3, None, p["X"], np.float64)
    dots = np.einsum("knp,kscp->knsc", p["A"], p["X"].reshape(K, S, 2, 5))
    assert np.allclose(ell, -np.log1p(np.exp(dots).sum(3)), rtol=1e-13, atol=0)


# ---- 2. the noise floor that sets the GPU tests' bar -------------------------------------------------------------------------------
def test_float64_noise_floor_of_the_restatement_on_the_gpu_inputs():
    """the restatement in float64 against itself in longdouble on every case of the GPU tests (both fed the same float64 l_si, logr
    and lw), relative to max(1, |value|): measured 1.05e-14 at the most (ess); l_si itself differs by 5.0e-16.  No row of any case
    changes its verdict between the two precisions (a case whose row did would get another seed in ref.SEEDS, never an
    exclusion).  The GPU bar is 1000 times the recorded floor."""
    worst, rows = {}, 0
    for c in ref.CASES:
        p = ref.make_case(c)
        args = (p["A"], p["y"], p["C"], p["counts"], p["X"])
        ell = np.asarray(ref.loglik_softmax(*args, np.float64), dtype=np.float64)
        worst["loglik"] = max(worst.get("loglik", 0.0), pref.rel_gap(ell, ref.loglik_softmax(*args)))
        a = ref.loo_batched(ell, p["logr"], p["lw"], p["counts"], np.float64)
        b = ref.loo_batched(ell, p["logr"], p["lw"], p["counts"])
        assert np.array_equal(a["info"], b["info"]), ref.case_id(c)
        rows += a["info"].size
        for n in ("elpd", "lpd", "khat", "ess"):
            worst[n] = max(worst.get(n, 0.0), ref.rel_gap(a[n], b[n]))
    print("float64 against longdouble:", {n: f"{g:.2e}" for n, g in worst.items()}, f"over {rows} rows")
    assert worst.pop("loglik") <= 1e-13                                       # (far inside the single-launch bar of 1e-11)
    floor = max(worst.values())
    assert floor <= ref.NOISE_FLOOR <= 2.0 * floor                            # the recorded floor is the measured one, rounded up
    assert ref.BAR == 1000 * ref.NOISE_FLOOR and ref.BAR < 1e-8 and ref.LOGLIK_BAR == 1e-11


def test_the_cases_are_the_table():
    assert [c[:3] for c in ref.CASES] == [(2, 1, 5), (3, 3, 33), (3, 5, 257), (4, 7, 33), (5, 4, 64), (9, 8, 65), (2, 64, 33),
                                          (33, 2, 33), (65, 1, 33), (17, 4, 4096), (3, 5, 1024)]
    assert [c[3:] for c in ref.CASES] == [("1", 1), ("NI-1", 3), ("2NI+3", 3), ("NI", 3), ("NI+1", 3), ("NI+1", 1), ("NI+1", 1),
                                          ("2NI+3", 3), ("NI+1", 1), ("NI+1", 1), ("NI+1", 1)]
    assert {c[1] % 4 for c in ref.CASES} == {0, 1, 2, 3} and sum((c[0] - 1) * c[1] == 64 for c in ref.CASES) == 5
    p = ref.make_case(ref.CASES[2])
    assert list(p["counts"]) == [0, max(1, p["N"] // 2), p["N"]] and p["N"] == 11 and p["y"].dtype == np.int32
    assert ref.make_case(ref.CASES[-2])["N"] == 3 and ref.loo_tile(17, 4, 4096) == 2 < ref.NI_CAP
    assert all(ref.make_case(c)["counts"] is None for c in ref.CASES if c[4] == 1)
    assert all(0 <= ref.make_case(c)["y"].min() and ref.make_case(c)["y"].max() <= c[0] - 1 for c in ref.CASES)


# ---- 3. the tile helper and the grid bound ------------------------------------------------------------------------------------------
def test_tile_helper_matches_its_formula_and_the_header_bounds():
    lib = _lib.load_library()
    for Cc, P in sorted({(c[0], c[1]) for c in ref.CASES} | {(2, 16), (2, 17), (3, 32), (5, 16), (17, 1), (18, 1), (2, 63)}):
        for S in (5, 8, 9, 33, 64, 257, 1024, 1025, 2048, 2049, 3000, 4095, 4096):
            ni = lib.gsmvi_psis_loo_softmax_tile(Cc, P, S)
            assert ni == ref.loo_tile(Cc, P, S) and 1 <= ni <= ref.NI_CAP, (Cc, P, S)
            S2 = 1 << max(3, (S - 1).bit_length())
            region = max(S2 + S + 508 + S2 // 2, 64 * (((Cc - 1) * P) | 1) + 16 * (4 * ((P + 3) // 4) + 1) + 16)
            assert region + ni * S <= ref.LDS_MAX_DOUBLES                     # the 160 KB rule
            assert ni == ref.NI_CAP or region + (ni + 1) * S > ref.LDS_MAX_DOUBLES
    assert ref.loo_tile(3, 5, 1024) == ref.loo_tile(65, 1, 1024) == ref.NI_CAP
    assert ref.loo_tile(65, 1, 4096) == ref.loo_tile(2, 1, 4096) == 2
    for Cc, P, S in ((1, 1, 8), (0, 4, 8), (2, 0, 8), (2, 65, 8), (66, 1, 8), (6, 13, 8), (3, 2, 4), (3, 2, 4097), (2 ** 17, 2 ** 17, 8)):
        assert lib.gsmvi_psis_loo_softmax_tile(Cc, P, S) == 0 == ref.loo_tile(Cc, P, S), (Cc, P, S)
    # K ceil(N / NI) at the 2^24 - 1 edge, in the arithmetic of the entry point
    ni = ref.loo_tile(3, 2, 8)
    K = 2 ** 12 - 1
    assert K * -(-(ni * 2 ** 12 + ni) // ni) == 2 ** 24 - 1 and K * -(-(ni * 2 ** 12 + ni + 1) // ni) > 2 ** 24 - 1


def test_abi_checks_arguments_before_the_context():
    ref.check_bad_arguments(_lib.load_library())


def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name, nargs in ((NAME, 19), (TILE, 3)):
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
    assert NAME in hdr.split("#ifndef GSMVI_HIP_H")[0]
    block = hdr[:hdr.index("int " + TILE)].rsplit("/*", 1)[1]                  # the definition is written above the entry point
    for line in ("eta_sic = a_i . x_s[c P .. c P + P - 1]  (c < C - 1),   eta_si,C-1 = 0",
                 "m_si    = max_c eta_sic   (all C values, the 0 included)",
                 "z_si    = sum_{c = 0 .. C-1} exp(eta_sic - m_si)   (class order, the reference class last)",
                 "l_si    = eta_si,y_i - m_si - log z_si",
                 "rho_si = logr_s - l_si (one subtraction)",
                 "elpd[k, i] = log sum_s exp(w_si + l_si)",
                 "lpd[k, i]  = log sum_s exp(lw_s + l_si)",
                 "tiles = 64 (D | 1) + 16 (4 ceil(P / 4) + 1) + 16",
                 "GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_SOFTMAX"):
        assert line in block, line
    # no new path bit, the word is not widened, the ABI version stays
    assert len(re.findall(r"#define\s+GSMVI_PATH_\w+\s+0x[0-9a-fA-F]+u", hdr)) == 32
    assert re.search(r"#define\s+GSMVI_ABI_VERSION\s+1\b", hdr) and _lib.load_library().gsmvi_abi_version() == 1
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_loo"] | HipEngine.PATH_BITS["batched_softmax"] == ref.PATH_BITS
    assert callable(HipEngine.psis_loo_softmax_tile) and callable(HipEngine.psis_loo_softmax_batched)
    import gsmvi_amd
    assert gsmvi_amd.psis_loo_softmax_batched is not None and "psis_loo_softmax_batched" in gsmvi_amd.__doc__
    assert "psis_loo_softmax_batched" in gsmvi_amd.BatchedSoftmaxTarget.__doc__


# ---- 4. host logic on the stand-in engine ------------------------------------------------------------------------------------------
def _fitted(K=3, N=12, Cc=3, P=2, counts=(12, 0, 7), seed=3):
    import gsmvi_amd
    rs = np.random.default_rng(seed)
    A = rs.standard_normal((K, N, P))
    y = ref.draw_labels(rs, A, rs.standard_normal((K, Cc - 1, P)))
    eng = ref.StandInEngine()
    tgt = gsmvi_amd.BatchedSoftmaxTarget(A, y, Cc, 1.0, counts=None if counts is None else np.array(counts), engine=eng)
    D = (Cc - 1) * P
    mean = 0.3 * rs.standard_normal((K, D))
    G = rs.standard_normal((K, D, D))
    cov = np.linalg.inv(np.eye(D)[None] + 0.3 * G @ np.swapaxes(G, 1, 2))
    return tgt, eng, mean, 0.5 * (cov + np.swapaxes(cov, 1, 2)), A, y


def test_psis_loo_softmax_batched_protocol_and_summaries():
    import gsmvi_amd
    tgt, eng, mean, cov, A, y = _fitted()
    K, N, D, S = 3, 12, 4, 40
    keys = [5, 6, 7]
    m0, c0 = mean.copy(), cov.copy()
    eng.calls.clear()
    r = gsmvi_amd.psis_loo_softmax_batched(tgt, mean, cov, keys, num_draws=S, call=2, pointwise_loglik=True)
    assert isinstance(r, gsmvi_amd.LOOBatchedResult) and r.nlaunch == 3 and r.threshold == pref.threshold(S)
    assert np.array_equal(mean, m0) and np.array_equal(cov, c0)
    launches = [c for c in eng.calls if isinstance(c, tuple)]
    seeds = tuple((k % 2 ** 32) ^ 0x5DEECE66D for k in keys)
    assert launches == [("draw", seeds, 2, 0, S), ("softmax", 3, "lp"), ("psis", (K, S, D), False),
                        ("loo_softmax", 3, (K, S, D), (K, N, 2), True, True)]
    top = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, call=2, moments=False, engine=ref.StandInEngine())
    assert np.array_equal(r.psis.khat, top.khat) and np.array_equal(r.psis.samples, top.samples)
    cnt = np.array([12, 0, 7])
    ell = np.asarray(ref.loglik_softmax(A, y, 3, cnt, top.samples), dtype=np.float64)
    want = ref.loo_batched(ell, top.log_ratios, top.log_weights, cnt)
    assert np.array_equal(r.loglik, ell, equal_nan=True) and r.loglik.shape == (K, N, S)
    for got, n in ((r.elpd_i, "elpd"), (r.lpd_i, "lpd"), (r.khat, "khat"), (r.ess, "ess")):
        assert isinstance(got, np.ndarray) and np.array_equal(got, np.asarray(want[n], dtype=np.float64), equal_nan=True), n
    assert np.array_equal(r.info, want["info"]) and r.info.dtype == np.int64
    assert (r.info[0] != -3).all() and (r.info[1] == -3).all() and (r.info[2, 7:] == -3).all()
    # the per-problem summaries are psis_loo_ref.summaries
    s = ref.summaries(want, cnt, S)
    for n in ("elpd_loo", "p_loo", "se"):
        assert np.allclose(getattr(r, n), s[n], rtol=1e-13, atol=0, equal_nan=True), n
    assert r.elpd_loo[1] == 0.0 and np.isnan(r.se[1]) and r.n_bad[1] == 0
    assert np.array_equal(r.n_bad, s["n_bad"])
    assert np.array_equal(r.ok, np.asarray(r.psis.ok) & (r.n_bad == 0)) and r.ok.dtype == bool
    # psis= reuses the draws: one launch, the same numbers; no pointwise block unless asked for
    eng.calls.clear()
    again = gsmvi_amd.psis_loo_softmax_batched(tgt, mean, cov, keys, psis=r.psis)
    assert [c[0] for c in eng.calls if isinstance(c, tuple)] == ["loo_softmax"] and again.nlaunch == 1 and again.loglik is None
    for n in ("elpd_loo", "p_loo", "se", "elpd_i", "lpd_i", "khat", "ess", "info", "n_bad", "ok"):
        assert np.array_equal(getattr(again, n), getattr(r, n), equal_nan=True), n


def test_type_and_argument_errors_come_before_any_engine_call():
    import dataclasses
    import gsmvi_amd
    tgt, eng, mean, cov, _, _ = _fitted()
    Ag, yg, offset, _, _, tau, _ = gref.make_inputs("logistic", 3, 12, 4, 1, seed=3)
    glm = gsmvi_amd.BatchedGLMTarget(Ag, yg, "logistic", 1.0, offset=offset, noise_precision=tau, engine=lref.StandInEngine())
    gauss = gsmvi_amd.BatchedGaussianTarget(np.zeros((3, 4)), cov=np.stack([np.eye(4)] * 3), engine=lref.StandInEngine())
    eng.calls.clear()
    for bad in (glm, gauss, tgt.lp, gsmvi_amd.psis_batched, None):
        with pytest.raises(TypeError, match="BatchedSoftmaxTarget"):
            gsmvi_amd.psis_loo_softmax_batched(bad, mean, cov, [1, 2, 3])
    # the GLM function and the target's methods keep their refusals
    with pytest.raises(TypeError, match="BatchedGLMTarget"):
        gsmvi_amd.psis_loo_batched(tgt, mean, cov, [1, 2, 3])
    with pytest.raises(TypeError, match="BatchedGLMTarget"):
        tgt.loo(mean, cov, [1, 2, 3])
    with pytest.raises(TypeError, match="predict"):
        tgt.predict(mean, cov)
    loo = lambda *a, **kw: gsmvi_amd.psis_loo_softmax_batched(tgt, *a, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="psis_loo_softmax_batched: mean must be"):
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
        gsmvi_amd.psis_loo_softmax_batched(tgt, mean, cov, [1, 2, 3], psis=good, engine=Device())


# ---- 5. a statistical check with an exact answer -----------------------------------------------------------------------------------
def test_elpd_is_the_leave_one_out_density_by_quadrature():
    """C = 3, P = 1 (D = 2), N = 12, lam = 1, seeds 0 .. 4: elpd_i of the restatement on S = 4096 draws of the Laplace Gaussian
    against log int p(y_i | x) p(x | y_-i) dx by 2-D grid quadrature: a Monte-Carlo gap, bounded by twice the largest measured
    over the rows and seeds (psis_loo_softmax_ref.QUAD_GAP: 0.056); 0 < sum p_loo < 2 D"""
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
        assert 0.0 < float((r["lpd"] - r["elpd"]).sum()) < 4.0
    print(f"gap {max(gap):.4f} (per seed {np.array2string(np.array(gap), precision=4)}), largest pointwise khat {max(khat):.2f}, "
          f"problem-level khat <= {max(top):.2f}")
    assert abs(max(gap) - ref.QUAD_GAP) <= 0.02 * ref.QUAD_GAP                  # the recorded gap is the measured one
    assert ref.QUAD_BOUND == 2.0 * ref.QUAD_GAP and max(gap) <= ref.QUAD_BOUND
