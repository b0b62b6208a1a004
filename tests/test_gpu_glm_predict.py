"""The batched GLM posterior predictive on the GPU (csrc/gsmvi_glm_predict_batched.hip): parity with the longdouble restatement
(tests/glm_predict_ref.py) over every D, M and K at which the kernel takes another path, the tie to the batched GLM target's
log-density, the independence of the problems bit for bit, the sign of eta_var, the path bit and the argument checks, and the
held-out score of a Laplace fit end to end."""
import numpy as np
import pytest
import torch
from scipy import special

import glm_predict_ref as ref

pytestmark = pytest.mark.gpu

NAMES = ("eta_mean", "eta_var", "mean", "lpd", "elpd")
CASES = [(f, s) for f in ref.FAMILIES for s in ref.SHAPES]


def _engine():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _run(family, p, with_offset=True, with_y=True, sel=None, mean=None, cov=None, A=None, y=None, offset=None, nodes=32):
    """the engine call on the problems ``sel`` of ``p`` -> a dict of numpy arrays (lpd, elpd None without y)"""
    eng = _engine()
    sel = np.arange(p["A"].shape[0]) if sel is None else np.asarray(sel)
    pick = lambda name, given: (p[name] if given is None else given)[sel]       # noqa: E731
    tau = p["tau"]
    tau = eng.batched_regs(tau[sel]) if isinstance(tau, np.ndarray) else tau
    out = eng.glm_predict_batched(eng.asarray(pick("mean", mean)), eng.asarray(pick("cov", cov)), eng.asarray(pick("A", A)),
                                  family, offset=eng.asarray(pick("offset", offset)) if with_offset else None,
                                  y=eng.asarray(pick("y", y)) if with_y else None, counts=eng.batched_counts(p["counts"][sel]),
                                  noise_prec=tau, nodes=nodes)
    torch.cuda.synchronize()
    return {n: (t.cpu().numpy() if t is not None else None) for n, t in zip(NAMES, out)}


def _same(a, b, names=NAMES):
    return all(np.array_equal(a[n], b[n], equal_nan=True) for n in names if a[n] is not None)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", CASES)
def test_predict_matches_the_restatement(family, shape):
    """1e-11 relative to max(1, |value|); eta_var relative to sum_ij |a_i| |Sigma_ij| |a_j|; with and without offset and y; the
    rows beyond counts are NaN; the outputs without y are the bits of those with it.  Measured worst over all cases: see
    DESIGN.md section 9."""
    D, M, K = shape
    worst = {n: 0.0 for n in NAMES}
    for off in (True, False):
        p, want = ref.reference(family, shape, off)
        live = np.arange(M)[None, :] < p["counts"][:, None]
        got = _run(family, p, with_offset=off)
        for n in ("eta_mean", "mean", "lpd"):
            assert np.isnan(got[n][~live]).all(), n
            e = float((np.abs(got[n][live] - want[n][live]) / np.maximum(1.0, np.abs(want[n][live]))).max()) if live.any() else 0.0
            worst[n] = max(worst[n], e)
        assert np.isnan(got["eta_var"][~live]).all()
        if live.any():
            worst["eta_var"] = max(worst["eta_var"], float((np.abs(got["eta_var"][live] - want["eta_var"][live])
                                                            / want["scale_var"][live]).max()))
        worst["elpd"] = max(worst["elpd"], float((np.abs(got["elpd"] - want["elpd"]) / np.maximum(1.0, np.abs(want["elpd"]))).max()))
        assert (got["elpd"][p["counts"] == 0] == 0.0).all()
        noy = _run(family, p, with_offset=off, with_y=False)
        assert noy["lpd"] is None and noy["elpd"] is None and _same(noy, got, NAMES[:3])
    print(f"{family} D={D} M={M} K={K}: worst " + ", ".join(f"{n} {e:.1e}" for n, e in worst.items()))
    for n, e in worst.items():
        assert e <= 1e-11, (n, e)


def test_node_counts_from_one_to_sixty_four():
    """Q = 1, 7 and 64 in both packings against the restatement at the same Q (1e-11)"""
    for family in ("logistic", "poisson"):
        for shape in ((10, 32, 7), (33, 65, 7)):
            p, _ = ref.reference(family, shape, True)
            live = np.arange(shape[1])[None, :] < p["counts"][:, None]
            for Q in (1, 7, 64):
                want = ref.predict(family, p["A"], p["offset"], p["y"], p["counts"], p["tau"], p["mean"], p["cov"], Q)
                got = _run(family, p, nodes=Q)
                for n in ("mean", "lpd"):
                    e = float((np.abs(got[n][live] - want[n][live]) / np.maximum(1.0, np.abs(want[n][live]))).max())
                    assert e <= 1e-11, (family, shape, Q, n, e)


# ---- 2. the tie to the existing kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("shape", [(10, 33, 7), (33, 65, 3)])
def test_zero_covariance_is_the_plug_in_prediction_and_the_targets_log_density(family, shape):
    import gsmvi_amd
    D, M, K = shape
    p = ref.make_problem(family, K, M, D)
    got = _run(family, p, cov=np.zeros_like(p["cov"]))
    live = np.arange(M)[None, :] < p["counts"][:, None]
    assert (got["eta_var"][live] == 0.0).all()
    m = got["eta_mean"]
    inv = {"logistic": special.expit, "probit": special.ndtr, "poisson": np.exp, "gaussian": lambda x: x}[family](m)
    e = float((np.abs(got["mean"][live] - inv[live]) / np.maximum(1.0, np.abs(inv[live]))).max())
    assert e <= 1e-11, e
    tgt = gsmvi_amd.BatchedGLMTarget(p["A"], p["y"], family, prior_precision=0.0, counts=p["counts"], offset=p["offset"],
                                     noise_precision=p["tau"])
    lp = tgt.lp(p["mean"][:, None, :]).cpu().numpy()[:, 0]
    for k in range(K):
        n = int(p["counts"][k])
        norm = 0.0
        if family == "gaussian":
            norm = n * 0.5 * np.log(p["tau"][k] / (2.0 * np.pi))
        elif family == "poisson":
            norm = -special.gammaln(p["y"][k, :n] + 1.0).sum()
        want = lp[k] + norm
        have = got["lpd"][k, :n].sum()
        assert abs(have - want) <= 1e-11 * max(1.0, abs(want)), (k, have, want)
        assert abs(got["elpd"][k] - want) <= 1e-11 * max(1.0, abs(want)), (k, got["elpd"][k], want)


# ---- 3. isolation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("D,M", [(10, 33), (33, 65)])
def test_a_problem_gives_the_same_bits_alone_and_in_every_slot(family, D, M):
    p = ref.make_problem(family, 7, M, D)
    j = 3                                                               # counts[3] = M
    alone = _run(family, p, sel=[j])
    for slot in range(7):
        sel = [k if k != j else slot for k in range(7)]
        sel[slot] = j
        batch = _run(family, p, sel=sel)
        for n in NAMES:
            assert np.array_equal(batch[n][slot], alone[n][0], equal_nan=True), (slot, n)
    again = _run(family, p, sel=[j])
    assert _same(again, alone)                                          # two calls, identical bits


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("D,M", [(10, 33), (33, 65)])
def test_a_nan_stays_in_its_problem(family, D, M):
    p = ref.make_problem(family, 7, M, D)
    p["counts"] = np.array([M, M, M // 2, M, 1, M - 1, M], dtype=np.int32)
    base = _run(family, p)
    others = [k for k in range(7) if k != 2]
    for name, at in (("cov", (2, D - 1, 0)), ("mean", (2, D - 1))):
        arr = p[name].copy()
        arr[at] = np.nan
        got = _run(family, p, **{name: arr})
        for n in NAMES:
            assert np.isnan(got[n][2]).all(), (name, n)
            assert np.array_equal(got[n][others], base[n][others], equal_nan=True), (name, n)


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("D,M", [(10, 33), (33, 65)])
def test_rows_beyond_counts_are_never_read_and_come_back_nan(family, D, M):
    p = ref.make_problem(family, 7, M, D)
    base = _run(family, p)
    A, y, o = p["A"].copy(), p["y"].copy(), p["offset"].copy()
    for k in range(7):
        A[k, p["counts"][k]:] = np.nan
        y[k, p["counts"][k]:] = np.nan
        o[k, p["counts"][k]:] = np.nan
    got = _run(family, p, A=A, y=y, offset=o)
    assert _same(got, base)
    live = np.arange(M)[None, :] < p["counts"][:, None]
    for n in NAMES[:4]:
        assert np.isnan(got[n][~live]).all() and np.isfinite(got[n][live]).all(), n
    assert np.isfinite(got["elpd"]).all()


# ---- 4. the sign of eta_var --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_a_negative_definite_covariance_shows_in_eta_var_alone(family):
    for D, M in ((10, 33), (33, 65)):
        p = ref.make_problem(family, 7, M, D)
        cov = p["cov"] + 0.01 * np.eye(D)
        live = np.arange(M)[None, :] < p["counts"][:, None]
        neg, zero = _run(family, p, cov=-cov), _run(family, p, cov=np.zeros_like(cov))
        assert (neg["eta_var"][live] < 0.0).all()
        assert _same(neg, zero, ("eta_mean", "mean", "lpd", "elpd"))


# ---- 5. integration ----------------------------------------------------------------------------------------------------------
def test_path_bit_argument_checks_and_the_public_interface():
    import gsmvi_amd
    eng = _engine()
    p = ref.make_problem("poisson", 3, 33, 10)
    eng.last_path(reset=True)
    got = _run("poisson", p)
    assert eng.last_path(reset=True) == {"batched_predict"}
    ref.check_bad_arguments(eng.lib)
    tgt = gsmvi_amd.BatchedGLMTarget(p["A"], p["y"], "poisson", offset=p["offset"])
    r = tgt.predict(p["mean"], p["cov"], p["A"], offset=p["offset"], y=p["y"], counts=p["counts"])
    assert isinstance(r, gsmvi_amd.GLMPrediction) and all(isinstance(getattr(r, n), np.ndarray) for n in NAMES)
    assert all(np.array_equal(getattr(r, n), got[n], equal_nan=True) for n in NAMES)
    dev = [eng.asarray(p[n]) for n in ("mean", "cov", "A")]
    rt = tgt.predict(*dev, offset=eng.asarray(p["offset"]), y=eng.asarray(p["y"]), counts=eng.batched_counts(p["counts"]))
    assert all(isinstance(getattr(rt, n), torch.Tensor) and getattr(rt, n).is_cuda for n in NAMES)
    assert all(np.array_equal(getattr(rt, n).cpu().numpy(), got[n], equal_nan=True) for n in NAMES)
    r0 = tgt.predict(p["mean"], p["cov"], p["A"])                       # built with an offset; none is required here
    assert r0.lpd is None and r0.elpd is None and np.isfinite(r0.mean).all()
    with pytest.raises(ValueError, match="^nodes:"):
        tgt.predict(p["mean"], p["cov"], p["A"], nodes=65)
    lt = gsmvi_amd.BatchedLogisticTarget(p["A"], (p["y"] > 0).astype(np.float64))
    lg = gsmvi_amd.BatchedGLMTarget(p["A"], (p["y"] > 0).astype(np.float64), "logistic")
    a = lt.predict(p["mean"], p["cov"], p["A"], y=(p["y"] > 1).astype(np.float64))
    b = lg.predict(p["mean"], p["cov"], p["A"], y=(p["y"] > 1).astype(np.float64))
    assert all(np.array_equal(getattr(a, n), getattr(b, n)) for n in NAMES)


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
def test_laplace_fit_scores_higher_than_its_overdispersed_copy():
    """K = 8 logistic problems at (N, D) = (96, 5), 32 rows held out: after laplace_init_batched the elpd of the Laplace Gaussian
    exceeds the elpd of the same mean with the covariance scaled by 25, on every problem (on the restatement alone: 0.84 at the
    least, tests/test_glm_predict_cpu.py)"""
    import gsmvi_amd
    (A, y, lam), (An, yn) = ref.e2e_problem()
    tgt = gsmvi_amd.BatchedLogisticTarget(A, y, prior_precision=lam)
    mean, cov, res = gsmvi_amd.laplace_init_batched(tgt)
    assert res.success.all()
    a = tgt.predict(mean, cov, An, y=yn)
    b = tgt.predict(mean, 25.0 * cov, An, y=yn)
    print("elpd(laplace) - elpd(25 cov):", np.array2string(a.elpd - b.elpd, precision=3))
    assert np.isfinite(a.elpd).all() and (a.elpd > b.elpd).all()
    want = ref.predict("logistic", An, None, yn, None, 1.0, mean, cov)
    assert float((np.abs(a.elpd - want["elpd"]) / np.maximum(1.0, np.abs(want["elpd"]))).max()) <= 1e-11
