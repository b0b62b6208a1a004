"""The batched Pareto-smoothed importance diagnostic on the GPU (csrc/gsmvi_psis_batched.hip): both entry points against the
longdouble restatement (tests/psis_batched_ref.py) at every S, D and K at which the kernel takes another path (S below, at and
above a power of two, one and several strides of 256 rows, D on both sides of the 16 / 17 switch of the moments, odd strides,
several workgroups), the order of tied ratios, the three verdicts among healthy neighbours, run-to-run bits, the path bit, and
``psis_batched`` end to end on Gaussian targets of known tail shape."""
import numpy as np
import pytest
import torch

import psis_batched_ref as ref

pytestmark = pytest.mark.gpu

# The bar of the PSIS outputs (khat, ess, log_z, lw, mean_is, cov_is), relative to max(1, |value|), lw entries below -700 left out.
# NOISE_FLOOR: the largest gap between the restatement in float64 and in longdouble over the inputs of this file, measured on the
# CPU by tests/test_psis_batched_cpu.py::test_float64_noise_floor_of_the_restatement_on_the_gpu_inputs (1.16e-13, at khat: the
# tail fit amplifies a rounding of the exceedances about 500 times; every other output stays below 5e-14).  The device's exp, log
# and log1p differ from numpy's by a few ulp and the same arithmetic amplifies them: the bar is 1000 times the floor.
NOISE_FLOOR = 1.2e-13
BAR = 1000 * NOISE_FLOOR            # 1.2e-10
LOGR_BAR = 1e-11                    # the project's single-launch bar, for the log ratios of the fused entry
W_NAMES = ("lw", "khat", "ess", "log_z")


def _engine():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _weights(logr):
    eng = _engine()
    out = eng.psis_weights_batched(eng.asarray(logr))
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in zip(W_NAMES + ("info",), out)}


def _fused(p, lp, moments=True):
    eng = _engine()
    out = eng.psis_batched(eng.asarray(p["mean"]), eng.asarray(p["cov"]), eng.asarray(p["X"]), eng.asarray(lp), moments=moments)
    torch.cuda.synchronize()
    names = ("logr", "lw", "khat", "ess", "log_z", "mean_is", "cov_is", "info")
    return {n: (t.cpu().numpy() if t is not None else None) for n, t in zip(names, out)}


def _gaps(got, want, names):
    return {n: ref.rel_gap(got[n], want[n], floor_lw=-700 if n == "lw" else None) for n in names}


# ---- 1. the weights entry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", ref.WEIGHT_S)
def test_weights_entry_matches_the_restatement(S):
    """every output against the longdouble restatement on the same ratios: Gaussian ratios, heavy tails, blocks of ties (ties
    across the cutoff included; lw is compared entry by entry, so tied entries must be smoothed in the same order), a NaN or
    +inf among healthy neighbours, -inf rows and a problem of -inf alone"""
    worst = {n: 0.0 for n in W_NAMES}
    for kind in ref.WEIGHT_KINDS:
        for K in ref.WEIGHT_K:
            logr = ref.weight_inputs(kind, K, S)
            want = ref.weights_batched(logr)
            got = _weights(logr)
            assert np.array_equal(got["info"], want["info"]), (kind, K, got["info"], want["info"])
            for n, g in _gaps(got, want, W_NAMES).items():
                worst[n] = max(worst[n], g)
            if kind == "nan":
                assert (want["info"] == -1).sum() == 1 and np.isnan(got["lw"][want["info"] == -1]).all()
            if kind == "neginf":
                assert np.isneginf(got["lw"][0, ::3]).all() and (want["info"][-1] == -1 or K == 1)
            live = want["info"] != -1
            assert not live.any() or np.abs(np.exp(got["lw"][live]).sum(1) - 1.0).max() < 1e-12
    print(f"S={S}: worst " + ", ".join(f"{n} {e:.1e}" for n, e in worst.items()))
    for n, e in worst.items():
        assert e <= BAR, (n, e)


def test_short_tail_and_tied_inputs_take_their_verdicts():
    got = _weights(np.stack([np.random.default_rng(1).normal(size=20), np.full(20, 3.5)]))
    assert list(got["info"]) == [-2, -2] and np.isposinf(got["khat"]).all()
    assert np.abs(got["lw"][1] + np.log(20.0)).max() < 1e-15 and abs(got["ess"][1] - 20.0) < 1e-12


# ---- 2. the fused entry ------------------------------------------------------------------------------------------------------
def _target_lp(target, p):
    """the (K, S) values of the target at p["X"], from the product's own targets on the device"""
    from gsmvi_amd import BatchedGaussianTarget, BatchedGLMTarget
    eng = _engine()
    if target == "gauss":
        lp = BatchedGaussianTarget(p["mt"], cov=p["ct"], engine=eng).lp_rows(eng.asarray(p["X"]))
    else:
        lp = BatchedGLMTarget(p["A"], p["y"], "logistic", 1.0, engine=eng).lp(eng.asarray(p["X"]))
    lp = lp.cpu().numpy()
    assert lp.shape == p["lp"].shape and ref.rel_gap(lp, p["lp"]) < 1e-9
    return lp


@pytest.mark.parametrize("D", ref.FUSED_D)
@pytest.mark.parametrize("target", ["gauss", "glm"])
def test_fused_entry_matches_the_restatement(target, D):
    """logr against the restatement's at 1e-11; every other output against the restatement fed the device's own logr (a rounding
    of a ratio cannot then move a row across the cutoff) at the bar above; moments=False gives no moments and the same bits"""
    worst = {n: 0.0 for n in ("logr",) + W_NAMES + ("mean_is", "cov_is")}
    for S in ref.FUSED_S:
        for K in ref.FUSED_K:
            p = ref.fused_inputs(target, K, D, S)
            lp = _target_lp(target, p)
            got = _fused(p, lp)
            first = ref.fused_batched(p["mean"], p["cov"], p["X"], lp, with_moments=False)
            worst["logr"] = max(worst["logr"], ref.rel_gap(got["logr"], first["logr"]))
            want = ref.fused_batched(p["mean"], p["cov"], p["X"], lp, logr=got["logr"])
            assert np.array_equal(got["info"], want["info"]) and (got["info"] == 0).all()
            for n, g in _gaps(got, want, W_NAMES + ("mean_is", "cov_is")).items():
                worst[n] = max(worst[n], g)
            assert np.array_equal(got["cov_is"], np.swapaxes(got["cov_is"], 1, 2))
            bare = _fused(p, lp, moments=False)
            assert bare["mean_is"] is None and bare["cov_is"] is None
            assert all(np.array_equal(bare[n], got[n]) for n in ("logr",) + W_NAMES + ("info",))
    print(f"{target} D={D}: worst " + ", ".join(f"{n} {e:.1e}" for n, e in worst.items()))
    assert worst.pop("logr") <= LOGR_BAR
    for n, e in worst.items():
        assert e <= BAR, (n, e)


@pytest.mark.parametrize("D", [2, 17, 64])
def test_a_covariance_that_is_not_positive_definite_flags_its_problem_alone(D):
    K, S = 5, 33
    p = ref.fused_inputs("gauss", K, D, S)
    lp = _target_lp("gauss", p)
    clean = _fused(p, lp)
    j = min(D - 1, 3)
    q = dict(p, cov=p["cov"].copy())
    q["cov"][2, j, j] = -1.0
    got = _fused(q, lp)
    assert list(got["info"]) == [0, 0, 1 + j, 0, 0]
    assert ref.chol_upper(q["cov"][2])[1] == 1 + j
    rest = [0, 1, 3, 4]
    for n in ("logr", "lw", "khat", "ess", "log_z", "mean_is", "cov_is"):
        assert np.isnan(got[n][2]).all(), n
        assert np.array_equal(got[n][rest], clean[n][rest]), n
    # a NaN in the target's values: info = -1, the ratios are written as computed, everything else of the problem is NaN
    lp2 = lp.copy()
    lp2[1, 5] = np.nan
    got = _fused(p, lp2)
    assert list(got["info"]) == [0, -1, 0, 0, 0] and np.isnan(got["logr"][1, 5])
    assert np.array_equal(np.delete(got["logr"][1], 5), np.delete(clean["logr"][1], 5))
    assert all(np.isnan(got[n][1]).all() for n in ("lw", "khat", "ess", "log_z", "mean_is", "cov_is"))
    assert all(np.array_equal(got[n][[0, 2, 3, 4]], clean[n][[0, 2, 3, 4]]) for n in ("lw", "khat", "mean_is", "cov_is"))


# ---- 3. bits and the path ----------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_the_path_bit_is_set():
    eng = _engine()
    p = ref.fused_inputs("glm", 5, 33, 257)
    eng.last_path()
    a = _fused(p, p["lp"])
    assert eng.last_path() == {"batched_psis"}
    b = _fused(p, p["lp"])
    assert all(np.array_equal(a[n], b[n]) for n in a)
    logr = ref.weight_inputs("ties", 9, 1000)
    w1 = _weights(logr)
    path = eng.last_path()
    assert path == {"batched_psis"} and not any(n.endswith("_generic") for n in path)
    w2 = _weights(logr)
    assert all(np.array_equal(w1[n], w2[n]) for n in w1)
    # a problem's bits do not depend on its neighbours
    alone = _weights(logr[4:5])
    assert all(np.array_equal(alone[n][0], w1[n][4]) for n in w1)


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1.25, 0.5])
def test_psis_batched_end_to_end_on_gaussian_targets(s):
    """K = 8 Gaussian targets, D = 4, S = 1000, q_k = the target with its covariance divided by s (the ratios' tail shape is
    1 - 1 / s): every problem is ok, and log_z estimates the log normaliser of the unnormalised ``lp_rows`` within 0.2"""
    import gsmvi_amd
    K, D, S = 8, 4, 1000
    rs = np.random.default_rng(7)
    mt = rs.normal(size=(K, D))
    A = rs.normal(size=(K, D, D)) / np.sqrt(D)
    ct = 0.5 * np.eye(D)[None] + A @ np.swapaxes(A, 1, 2)
    tgt = gsmvi_amd.BatchedGaussianTarget(mt, cov=ct)
    log_norm = 0.5 * (D * np.log(2 * np.pi) + np.linalg.slogdet(ct)[1])
    shift = tgt.engine.asarray(log_norm)[:, None]
    mean, cov = tgt.engine.asarray(mt), tgt.engine.asarray(ct / s)
    m0, c0 = mean.clone(), cov.clone()
    r = gsmvi_amd.psis_batched(lambda X: tgt.lp_rows(X) - shift, mean, cov, list(range(K)), num_draws=S)
    assert torch.equal(mean, m0) and torch.equal(cov, c0)
    print(f"s = {s}: khat {np.array2string(r.khat, precision=2)}, log_z {np.array2string(r.log_z, precision=3)}, "
          f"ess {np.array2string(r.ess, precision=0)}")
    assert r.nlaunch == 2 and r.threshold == min(1 - 1 / np.log10(S), 0.7) and (r.info == 0).all()
    assert r.ok.all()
    assert (np.abs(r.log_z) <= 0.2).all()
    assert r.samples.shape == (K, S, D) and r.log_weights.shape == (K, S) and r.mean.shape == (K, D) and r.cov.shape == (K, D, D)
    t = gsmvi_amd.psis_batched(lambda X: tgt.lp_rows(X) - shift, mean, cov, list(range(K)), num_draws=S, as_torch=True, moments=False)
    assert t.khat.is_cuda and t.mean is None and np.array_equal(t.khat.cpu().numpy(), r.khat) and bool(t.ok.all())
    w = gsmvi_amd.psis_weights_batched(r.log_ratios)
    assert w.nlaunch == 1 and np.array_equal(w.khat, r.khat) and np.array_equal(w.log_weights, r.log_weights)
