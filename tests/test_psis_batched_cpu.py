"""The batched Pareto-smoothed importance diagnostic without a GPU: the longdouble restatement (tests/psis_batched_ref.py) pinned
to exact generalised-Pareto quantiles, to Gaussian ratios of known tail shape and to every outcome of the definition; the
float64 noise floor of the restatement on the GPU tests' inputs (the bar of tests/test_gpu_psis_batched.py is 1000 times it);
the host logic of ``psis_batched`` / ``psis_weights_batched`` on a stand-in engine; the C ABI declarations and argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import psis_batched_ref as ref
from gsmvi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gsmvi_psis_weights_batched_f64", "gsmvi_psis_batched_f64"]


# ---- 1. the tail fit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-0.3, 0.1, 0.5, 0.9])
def test_tail_fit_recovers_the_shape_of_exact_quantiles(k):
    """n = 200 exact generalised-Pareto quantiles, sigma = 1: khat within 0.06 of k (measured 0.053, 0.028, 0.002, 0.024: the
    weakly informative prior pulls towards 0.5)"""
    n = 200
    p = (np.arange(n) + 0.5) / n
    khat, sigma = ref.gpd_fit(np.expm1(-k * np.log1p(-p)) / k)
    print(f"k = {k}: khat - k = {float(khat) - k:+.4f}, sigma = {float(sigma):.4f}")
    assert abs(float(khat) - k) <= 0.06
    k64, s64 = ref.gpd_fit(np.expm1(-k * np.log1p(-p)) / k, np.float64)
    assert abs(float(k64) - float(khat)) < 1e-12 and abs(float(s64) - float(sigma)) < 1e-12


# ---- 2. Gaussian ratios of known shape ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gaussian_runs():
    """(khat, log_z) of 20 repeats per (D, s): q = N(0, I_D) against N(0, s I_D), S = 4096; the true shape is 1 - 1 / s"""
    out = {}
    for D in (1, 4):
        for s in (0.5, 1.25, 4.0):
            rs = np.random.default_rng(0)
            rr = [ref.psis_weights(ref.gaussian_ratio_rows(rs, 4096, D, s)) for _ in range(20)]
            out[D, s] = (np.array([float(r["khat"]) for r in rr]), np.array([float(r["log_z"]) for r in rr]))
    return out


@pytest.mark.parametrize("D", [1, 4])
def test_gaussian_ratios_of_known_tail_shape(gaussian_runs, D):
    """measured: maxima -0.27 (s = 0.5) and 0.38 (s = 1.25); medians 0.66 - 0.80 (s = 4) against 0.20 - 0.24 (s = 1.25);
    |log_z| <= 0.03"""
    k05, z05 = gaussian_runs[D, 0.5]
    k125, z125 = gaussian_runs[D, 1.25]
    k4, _ = gaussian_runs[D, 4.0]
    print(f"D = {D}: max khat {k05.max():.2f} (s = 0.5), {k125.max():.2f} (s = 1.25); medians {np.median(k4):.2f} (s = 4), "
          f"{np.median(k125):.2f} (s = 1.25); |log_z| <= {max(np.abs(z05).max(), np.abs(z125).max()):.3f}")
    assert (k05 < 0.0).all()
    assert (k125 < 0.7).all()
    assert np.median(k4) - np.median(k125) >= 0.3
    assert (np.abs(z05) <= 0.1).all() and (np.abs(z125) <= 0.1).all()


# ---- 3. the outcomes of the definition ---------------------------------------------------------------------------------------
def test_short_tail_gives_infinite_khat_and_plain_weights():
    """S = 20: M = 4, so n = 4 <= 4: khat = +inf, info = -2, no smoothing -- the weights are the plain self-normalised ones"""
    rs = np.random.default_rng(1)
    logr = rs.normal(size=20)
    r = ref.psis_weights(logr)
    assert ref.tail_size(20) == 4 and r["n"] == 4 and r["info"] == -2 and np.isposinf(r["khat"])
    want = logr - np.logaddexp.reduce(logr)
    assert np.abs(np.asarray(r["lw"], dtype=np.float64) - want).max() < 1e-14
    same = ref.psis_weights(np.full(20, 3.5))                            # all tied: the tail is empty
    assert same["n"] == 0 and same["info"] == -2
    assert np.abs(np.asarray(same["lw"], dtype=np.float64) + np.log(20.0)).max() < 1e-15
    assert abs(float(same["ess"]) - 20.0) < 1e-12 and abs(float(same["log_z"]) - 3.5) < 1e-15


def test_a_tie_across_the_cutoff_shortens_the_tail():
    S = 100
    M = ref.tail_size(S)
    assert M == 20
    base = np.arange(S, dtype=np.float64) / S
    assert ref.psis_weights(base)["n"] == M
    tied = base.copy()
    tied[S - M:S - M + 3] = tied[S - M - 1]                               # three of the top M tie with the cutoff
    r = ref.psis_weights(tied)
    assert r["n"] == M - 3 and r["info"] == 0
    # the tied entries are left as they are (no smoothing), in index order
    lw = np.asarray(r["lw"], dtype=np.float64)
    assert np.ptp(lw[S - M - 1:S - M + 3]) == 0.0


def test_a_nan_row_flags_its_own_problem_only():
    rs = np.random.default_rng(2)
    logr = rs.normal(size=(4, 64))
    clean = ref.weights_batched(logr)
    for bad_value, row in ((np.nan, 1), (np.inf, 2)):
        dirty = logr.copy()
        dirty[row, 7] = bad_value
        r = ref.weights_batched(dirty)
        assert r["info"][row] == -1 and np.isnan(r["lw"][row]).all()
        assert all(np.isnan(r[n][row]) for n in ("khat", "ess", "log_z"))
        rest = [k for k in range(4) if k != row]
        for n in ("lw", "khat", "ess", "log_z", "info"):
            assert np.array_equal(r[n][rest], clean[n][rest]), n
    allneg = ref.psis_weights(np.full(30, -np.inf))
    assert allneg["info"] == -1 and np.isnan(allneg["lw"]).all()


@pytest.mark.parametrize("S", [5, 20, 33, 257, 1000])
def test_weights_are_normalised_and_ess_is_in_range(S):
    rs = np.random.default_rng(S)
    logr = -0.9 * np.log(rs.uniform(size=S))
    logr[::4] = -np.inf                                                   # outside the support: weight 0
    r = ref.psis_weights(logr)
    lw = np.asarray(r["lw"])
    assert np.isneginf(lw[::4]).all() and np.isfinite(np.delete(lw, np.s_[::4])).all()
    assert abs(float(np.exp(lw).sum()) - 1.0) < 1e-15
    assert 1.0 <= float(r["ess"]) <= S
    assert r["info"] in (0, -2) and (lw <= 0).all()
    # the order of the weights is the order of the ratios (smoothing keeps ranks)
    fin = np.isfinite(logr)
    assert np.array_equal(np.argsort(logr[fin], kind="stable"), np.argsort(np.asarray(lw[fin], dtype=np.float64), kind="stable"))


def test_moments_of_equal_weights_are_the_sample_moments():
    rs = np.random.default_rng(3)
    X = rs.normal(size=(50, 3)) + 2.0
    mean = np.array([1.0, 2.0, 3.0])
    m, c = ref.moments(mean, X, np.full(50, -np.log(50.0)))
    assert np.abs(np.asarray(m, dtype=np.float64) - X.mean(0)).max() < 1e-14
    assert np.abs(np.asarray(c, dtype=np.float64) - np.cov(X.T, bias=True)).max() < 1e-14


# ---- 4. the noise floor that sets the GPU tests' bar -------------------------------------------------------------------------
def test_float64_noise_floor_of_the_restatement_on_the_gpu_inputs():
    """the restatement in float64 against itself in longdouble on every input of the GPU tests, relative to max(1, |value|), lw
    entries below -700 left out: measured 1.2e-13 at the most (khat); the GPU tests' bar is 1000 times the recorded floor and
    must stay tighter than 1e-8"""
    import test_gpu_psis_batched as gpu
    worst = {}

    def upd(name, g):
        worst[name] = max(worst.get(name, 0.0), g)

    for kind in ref.WEIGHT_KINDS:
        for S in ref.WEIGHT_S:
            for K in ref.WEIGHT_K:
                lr = ref.weight_inputs(kind, K, S)
                a, b = ref.weights_batched(lr, np.float64), ref.weights_batched(lr)
                assert np.array_equal(a["info"], b["info"])
                for n in ("khat", "ess", "log_z"):
                    upd(n, ref.rel_gap(a[n], b[n]))
                upd("lw", ref.rel_gap(a["lw"], b["lw"], floor_lw=-700))
    for tgt in ("gauss", "glm"):
        for D in ref.FUSED_D:
            for S, K in ((S, K) for S in ref.FUSED_S for K in ref.FUSED_K):
                p = ref.fused_inputs(tgt, K, D, S)
                b0 = ref.fused_batched(p["mean"], p["cov"], p["X"], p["lp"])
                a0 = ref.fused_batched(p["mean"], p["cov"], p["X"], p["lp"], dtype=np.float64)
                upd("logr", ref.rel_gap(a0["logr"], b0["logr"]))
                lr64 = np.asarray(a0["logr"], dtype=np.float64)
                a = ref.fused_batched(p["mean"], p["cov"], p["X"], p["lp"], dtype=np.float64, logr=lr64)
                b = ref.fused_batched(p["mean"], p["cov"], p["X"], p["lp"], logr=lr64)
                for n in ("khat", "ess", "log_z", "mean_is", "cov_is"):
                    upd(n, ref.rel_gap(a[n], b[n]))
                upd("lw", ref.rel_gap(a["lw"], b["lw"], floor_lw=-700))
    print("float64 against longdouble:", {n: f"{g:.2e}" for n, g in worst.items()})
    floor = max(g for n, g in worst.items() if n != "logr")
    assert worst["logr"] <= 1e-13                                         # (far inside the single-launch bar of 1e-11)
    assert floor <= gpu.NOISE_FLOOR and gpu.NOISE_FLOOR <= 2.0 * floor    # the recorded floor is the measured one, rounded up
    assert gpu.BAR == 1000 * gpu.NOISE_FLOOR and gpu.BAR < 1e-8


# ---- 5. host logic on the stand-in engine ------------------------------------------------------------------------------------
def _state(K, D, seed=0):
    rs = np.random.RandomState(seed)
    mean = rs.standard_normal((K, D))
    A = rs.standard_normal((K, D, D))
    return mean, A @ np.swapaxes(A, 1, 2) + D * np.eye(D)


def _gauss_rows(ms, covs):
    Ps = np.linalg.inv(covs)

    def lp(X):
        r = np.asarray(X) - ms[:, None, :]
        return -0.5 * np.einsum("ksi,kij,ksj->ks", r, Ps, r)
    return lp


def test_psis_batched_protocol_seed_rule_and_call():
    import gsmvi_amd
    from oracle import gsm_oracle as orc
    K, D, S = 3, 4, 40
    mean, cov = _state(K, D)
    lp = _gauss_rows(*_state(K, D, seed=1))
    keys = [7, 2 ** 40 + 3, 12345]
    seeds = tuple((k % 2 ** 32) ^ 0x5DEECE66D for k in keys)
    for call in (0, 5):
        eng = ref.StandInEngine()
        m0, c0 = mean.copy(), cov.copy()
        r = gsmvi_amd.psis_batched(lp, mean, cov, keys, num_draws=S, call=call, engine=eng)
        assert isinstance(r, gsmvi_amd.PSISBatchedResult) and r.nlaunch == 2
        launches = [c for c in eng.calls if isinstance(c, tuple)]
        assert launches == [("draw", seeds, call, 0, S), ("psis", (K, S, D), True)]
        assert np.array_equal(mean, m0) and np.array_equal(cov, c0)                  # only read
        X = np.stack([mean[k] + orc.philox_randn(seeds[k], call, S * D).reshape(S, D) @ np.linalg.cholesky(cov[k]).T
                      for k in range(K)])
        assert np.abs(r.samples - X).max() < 1e-12
        want = ref.fused_batched(mean, cov, r.samples, lp(r.samples))
        for got, name in ((r.khat, "khat"), (r.ess, "ess"), (r.log_z, "log_z"), (r.log_weights, "lw"), (r.log_ratios, "logr"),
                          (r.mean, "mean_is"), (r.cov, "cov_is")):
            assert isinstance(got, np.ndarray) and np.array_equal(got, np.asarray(want[name], dtype=np.float64)), name
        assert r.threshold == min(1 - 1 / np.log10(S), 0.7) and np.array_equal(r.info, want["info"])
        assert np.array_equal(r.ok, (r.info == 0) & (r.khat < r.threshold)) and r.ok.dtype == bool
    # keys equal modulo 2^32 draw the same rows; range / array keys are accepted
    a = gsmvi_amd.psis_batched(lp, mean, cov, [k + 2 ** 32 for k in keys], num_draws=S, call=5, engine=ref.StandInEngine())
    assert np.array_equal(a.samples, r.samples)
    b = gsmvi_amd.psis_batched(lp, mean, cov, np.array(keys), num_draws=S, call=5, moments=False, engine=ref.StandInEngine())
    assert b.mean is None and b.cov is None and np.array_equal(b.khat, r.khat)


def test_psis_batched_lp_gets_the_device_block_first_and_sums_are_refused():
    import gsmvi_amd
    K, D, S = 2, 3, 12
    mean, cov = _state(K, D)
    rows = _gauss_rows(*_state(K, D, seed=1))
    seen = []

    def picky(X):                                    # refuses the first block it is handed, as a host-only log-density would
        seen.append(type(X))
        if len(seen) == 1:
            raise TypeError("numpy only")
        return rows(X)
    r = gsmvi_amd.psis_batched(picky, mean, cov, [1, 2], num_draws=S, engine=ref.StandInEngine())
    assert len(seen) == 2 and r.info.shape == (K,)
    eng = ref.StandInEngine()
    with pytest.raises(ValueError, match="lp_rows"):
        gsmvi_amd.psis_batched(lambda X: rows(X).sum(1), mean, cov, [1, 2], num_draws=S, engine=eng)
    assert not any(isinstance(c, tuple) and c[0] == "psis" for c in eng.calls)
    with pytest.raises(ValueError, match=r"expected \(2, 12\)"):
        gsmvi_amd.psis_batched(lambda X: rows(X)[:, :5], mean, cov, [1, 2], num_draws=S, engine=eng)


def test_shape_and_bound_errors_come_before_any_engine_call():
    import gsmvi_amd
    eng = ref.StandInEngine()
    mean, cov = _state(2, 4)
    lp = lambda X: np.zeros(X.shape[:2])                        # noqa: E731
    pb = lambda *a, **kw: gsmvi_amd.psis_batched(lp, *a, engine=eng, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="D = 65"):
        pb(np.zeros((2, 65)), np.zeros((2, 65, 65)), [1, 2])
    with pytest.raises(ValueError, match="D = 0"):
        pb(np.zeros((2, 0)), np.zeros((2, 0, 0)), [1, 2])
    with pytest.raises(ValueError, match="mean must be"):
        pb(np.zeros(4), cov, [1, 2])
    with pytest.raises(ValueError, match="keys"):
        pb(mean, cov, [1, 2, 3])
    with pytest.raises(ValueError, match="cov"):
        pb(mean, cov[:, :3], [1, 2])
    for S in (4, 4097, 0, 10.5):
        with pytest.raises(ValueError, match="num_draws"):
            pb(mean, cov, [1, 2], num_draws=S)
    for shape in ((2, 4), (2, 4097), (8,), (2, 8, 3), (0, 8)):
        with pytest.raises(ValueError, match="psis_weights_batched"):
            gsmvi_amd.psis_weights_batched(np.zeros(shape), engine=eng)
    assert eng.calls == []


def test_psis_weights_batched_protocol():
    import gsmvi_amd
    eng = ref.StandInEngine()
    logr = ref.weight_inputs("nan", 3, 64)
    r = gsmvi_amd.psis_weights_batched(logr, engine=eng)
    assert [c for c in eng.calls if isinstance(c, tuple)] == [("psis_weights", (3, 64))] and r.nlaunch == 1
    want = ref.weights_batched(logr)
    assert r.samples is None and r.mean is None and r.cov is None
    assert np.array_equal(r.log_ratios, logr, equal_nan=True)
    assert np.array_equal(r.khat, np.asarray(want["khat"], dtype=np.float64), equal_nan=True)
    assert np.array_equal(r.info, want["info"]) and (r.info == -1).sum() == 1 and not r.ok[r.info != 0].any()
    assert not r.ok[np.isnan(r.khat)].any() and r.threshold == min(1 - 1 / np.log10(64), 0.7)


def test_gaussian_target_lp_rows_sums_to_lp():
    import torch
    from gsmvi_amd import BatchedGaussianTarget

    class Eng:
        def asarray(self, x):
            return torch.as_tensor(np.asarray(x, dtype=np.float64))
    ms, covs = _state(3, 4)
    tgt = BatchedGaussianTarget(ms, cov=covs, engine=Eng())
    X = np.random.RandomState(0).standard_normal((3, 7, 4))
    rows = tgt.lp_rows(X)
    assert tuple(rows.shape) == (3, 7)
    assert torch.allclose(rows.sum(1), tgt.lp(X), rtol=0, atol=1e-12)
    assert np.abs(rows.numpy() - _gauss_rows(ms, covs)(X)).max() < 1e-12


# ---- 6. the C ABI ------------------------------------------------------------------------------------------------------------
def test_psis_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name, nargs in zip(NEW, (10, 17)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        for mp in ("exports.map", "exports_debug.map"):
            assert re.search(r"^\s*" + name + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), (mp, name)
        assert name in _lib.exported_symbols() and name in built, name
        res, args = _lib._SIGS[name]
        decl = re.search(r"int\s+" + name + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert res is C.c_int and len(args) == len(params) == nargs
        for p, a in zip(params, args):
            want = C.c_int64 if p.startswith("int64_t") else C.c_int if p.startswith("int ") else C.c_void_p
            assert a is want, (p, a)
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_PSIS\s+0x200000u", hdr)
    mask = re.search(r"#define\s+GSMVI_PATH_GENERIC_MASK\s+\(([^)]*)\)", hdr).group(1)
    assert "0x200000" not in mask and "#define GSMVI_ABI_VERSION 1" in hdr
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_psis"] == ref.PATH_BIT == 0x200000 and not HipEngine.PATH_GENERIC_MASK & 0x200000
    assert len(set(HipEngine.PATH_BITS.values())) == len(HipEngine.PATH_BITS)
    assert _lib.load_library().gsmvi_abi_version() == 1
    import gsmvi_amd
    for name in ("psis_batched", "psis_weights_batched", "PSISBatchedResult"):
        assert getattr(gsmvi_amd, name) is not None and name in gsmvi_amd.__doc__


def test_abi_checks_arguments_before_the_context():
    ref.check_bad_arguments(_lib.load_library())
