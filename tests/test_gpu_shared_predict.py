"""The shared-design GLM posterior predictive on the GPU (csrc/gsmvi_glm_shared_predict_batched.hip): parity with the longdouble
restatement (tests/shared_predict_ref.py) over every D, M and K at which the kernel takes another path, with and without offset, y
and weights; the bit contract with the per-problem launch on the replicated rows; the rows that are not valid are never read; a
NaN in one row of the shared A_new; the independence of the problems bit for bit; the sign of eta_var; the path bits and the
public function; and K-fold cross-validation of a Laplace fit end to end.

Measured on the MI355X, worst over test 1's 48 cases: see DESIGN.md section 9, "Shared-design GLM predictive"."""
import numpy as np
import pytest
import torch

import shared_predict_ref as ref

pytestmark = pytest.mark.gpu

NAMES = ref.NAMES
CASES = [(f, s) for f in ref.FAMILIES for s in ref.SHAPES]
PACKINGS = ((5, 65, 7), (33, 65, 3))                                   # four slots per workgroup, one slot per workgroup


def _engine():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _tau(eng, p, sel):
    tau = p["tau"]
    return eng.batched_regs(tau[sel]) if isinstance(tau, np.ndarray) else tau


def _run(family, p, with_offset=True, with_y=True, weights=None, sel=None, mean=None, cov=None, A=None, y=None, offset=None,
         nodes=32):
    """the engine call on the problems ``sel`` of ``p`` -> a dict of numpy arrays (lpd, elpd None without y)"""
    eng = _engine()
    sel = np.arange(p["mean"].shape[0]) if sel is None else np.asarray(sel)
    pick = lambda name, given: (p[name] if given is None else given)[sel]       # noqa: E731
    out = eng.glm_shared_predict_batched(eng.asarray(pick("mean", mean)), eng.asarray(pick("cov", cov)),
                                         eng.asarray(p["A"] if A is None else A), family,
                                         offset=eng.asarray(pick("offset", offset)) if with_offset else None,
                                         y=eng.asarray(pick("y", y)) if with_y else None,
                                         weights=eng.asarray(weights[sel]) if weights is not None else None,
                                         noise_prec=_tau(eng, p, sel), nodes=nodes)
    torch.cuda.synchronize()
    return {n: (t.cpu().numpy() if t is not None else None) for n, t in zip(NAMES, out)}


def _run_replicated(family, p, counts=None, with_offset=True, with_y=True, nodes=32):
    """the per-problem launch (gsmvi_glm_predict_batched_f64) on the K-fold replicated rows"""
    eng = _engine()
    K = p["mean"].shape[0]
    rep = np.ascontiguousarray(np.broadcast_to(p["A"], (K,) + p["A"].shape))
    out = eng.glm_predict_batched(eng.asarray(p["mean"]), eng.asarray(p["cov"]), eng.asarray(rep), family,
                                  offset=eng.asarray(p["offset"]) if with_offset else None,
                                  y=eng.asarray(p["y"]) if with_y else None,
                                  counts=eng.batched_counts(counts) if counts is not None else None,
                                  noise_prec=_tau(eng, p, np.arange(K)), nodes=nodes)
    torch.cuda.synchronize()
    return {n: (t.cpu().numpy() if t is not None else None) for n, t in zip(NAMES, out)}


def _same(a, b, names=NAMES):
    return all(np.array_equal(a[n], b[n], equal_nan=True) for n in names if a[n] is not None)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", CASES)
def test_predict_matches_the_restatement(family, shape):
    """1e-11 relative to max(1, |value|); eta_var relative to sum_ij |a_i| |Sigma_ij| |a_j|; elpd relative to max(1, sum v |lpd|);
    with and without offset, y and weights (y = NaN and offset = +inf under every zero weight); the rows that are not valid are
    NaN, a problem without a valid row has elpd = 0; the outputs without y are the bits of those with it"""
    D, M, K = shape
    worst = {n: 0.0 for n in NAMES}
    for off in (True, False):
        for wts in (True, False):
            p, want = ref.reference(family, shape, off, wts)
            w = p["weights"]
            live = ref.valid_mask(w, K, M)
            got = _run(family, p, with_offset=off, weights=w)
            for n in ("eta_mean", "mean", "lpd"):
                assert np.isnan(got[n][~live]).all() and np.isfinite(got[n][live]).all(), n
                worst[n] = max(worst[n], ref.rel(got[n], want[n]))
            assert np.isnan(got["eta_var"][~live]).all() and np.isfinite(got["eta_var"][live]).all()
            worst["eta_var"] = max(worst["eta_var"], ref.rel(got["eta_var"], want["eta_var"], want["scale_var"]))
            assert np.isfinite(got["elpd"]).all()
            worst["elpd"] = max(worst["elpd"], ref.rel(got["elpd"], want["elpd"], np.maximum(1.0, want["scale_elpd"])))
            assert (got["elpd"][~live.any(1)] == 0.0).all()
            noy = _run(family, p, with_offset=off, with_y=False, weights=w)
            assert noy["lpd"] is None and noy["elpd"] is None and _same(noy, got, NAMES[:3])
    print(f"{family} D={D} M={M} K={K}: worst " + ", ".join(f"{n} {e:.1e}" for n, e in worst.items()))
    for n, e in worst.items():
        assert e <= 1e-11, (n, e)


# ---- 2. the bit contract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("shape", PACKINGS)
def test_without_weights_the_bits_are_the_per_problem_launch_on_the_replicated_rows(family, shape):
    """weights None and np.ones: every output equals glm_predict_batched on the K-fold replicated A_new bit for bit, in both
    packings, at Q = 1, 7, 32, 64, with and without y and the offset; a 0 / 1 prefix mask equals that launch with counts"""
    D, M, K = shape
    p = ref.make_problem(family, K, M, D)
    ones = np.ones((K, M))
    for Q in (1, 7, 32, 64):
        want = _run_replicated(family, p, nodes=Q)
        for w in (None, ones):
            assert _same(_run(family, p, weights=w, nodes=Q), want), (Q, w is None)
    for off, wy in ((False, True), (True, False), (False, False)):
        want = _run_replicated(family, p, with_offset=off, with_y=wy)
        for w in (None, ones):
            assert _same(_run(family, p, with_offset=off, with_y=wy, weights=w), want, NAMES if wy else NAMES[:3]), (off, wy)
    cyc = [M, 0, 1, 32, M - 1, 33, 31]
    counts = np.array([cyc[k % len(cyc)] for k in range(K)], dtype=np.int32)
    mask = (np.arange(M)[None, :] < counts[:, None]).astype(np.float64)
    for Q in (7, 32):
        assert _same(_run(family, p, weights=mask, nodes=Q), _run_replicated(family, p, counts=counts, nodes=Q)), Q
    assert _same(_run(family, p, with_y=False, weights=mask), _run_replicated(family, p, counts=counts, with_y=False), NAMES[:3])


# ---- 3. the rows that are not valid are never read ---------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("shape", PACKINGS)
def test_rows_of_weight_zero_are_never_read(family, shape):
    """y = NaN and offset = +inf, then -inf, under the zero weights leave every bit unchanged"""
    D, M, K = shape
    p = ref.make_problem(family, K, M, D)
    w = ref.weight_pattern(K, M)
    base = _run(family, p, weights=w)
    y, o = ref.plant(p["y"], p["offset"], w)
    assert _same(_run(family, p, weights=w, y=y, offset=o), base)
    assert _same(_run(family, p, weights=w, y=y, offset=np.where(w == 0.0, -np.inf, p["offset"])), base)
    wn = np.where(w == 0.0, np.nan, w)                                  # a NaN weight removes the row as a zero does
    assert _same(_run(family, p, weights=wn, y=y, offset=o), base)
    live = w > 0
    for n in NAMES[:4]:
        assert np.isnan(base[n][~live]).all() and np.isfinite(base[n][live]).all(), n
    assert np.isfinite(base["elpd"]).all() and base["elpd"][1] == 0.0


# ---- 4. a NaN in one row of the shared A_new ---------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("shape", PACKINGS)
def test_a_nan_in_a_row_of_a_new_reaches_that_row_of_every_problem_and_no_other(family, shape):
    D, M, K = shape
    p = ref.make_problem(family, K, M, D)
    w = ref.weight_pattern(K, M)
    w[0, 40], w[0, 3] = 1.25, 0.75                                     # both rows are valid somewhere (and not in problem 1)
    base = _run(family, p, weights=w)
    for row, col in ((40, D - 1), (3, 0)):
        A = p["A"].copy()
        A[row, col] = np.nan
        got = _run(family, p, weights=w, A=A)
        hit = w[:, row] > 0                                             # the problems where that row is valid
        assert hit.any() and not hit.all()
        for n in NAMES[:4]:
            assert np.isfinite(base[n][hit, row]).all() and np.isnan(got[n][:, row]).all(), n
            keep = np.ones(M, dtype=bool)
            keep[row] = False
            assert np.array_equal(got[n][:, keep], base[n][:, keep], equal_nan=True), n
        assert np.isnan(got["elpd"][hit]).all()
        assert np.array_equal(got["elpd"][~hit], base["elpd"][~hit])


# ---- 5. isolation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("D,M", [(5, 33), (33, 65)])
def test_a_problem_gives_the_same_bits_alone_and_in_every_slot(family, D, M):
    p = ref.make_problem(family, 7, M, D)
    w = ref.weight_pattern(7, M)
    j = 3
    alone = _run(family, p, weights=w, sel=[j])
    for slot in range(7):
        sel = [k if k != j else slot for k in range(7)]
        sel[slot] = j
        batch = _run(family, p, weights=w, sel=sel)
        for n in NAMES:
            assert np.array_equal(batch[n][slot], alone[n][0], equal_nan=True), (slot, n)
    assert _same(_run(family, p, weights=w, sel=[j]), alone)            # two calls, identical bits


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("D,M", [(5, 33), (33, 65)])
def test_a_nan_stays_in_its_problem(family, D, M):
    p = ref.make_problem(family, 7, M, D)
    w = ref.weight_pattern(7, M)
    base = _run(family, p, weights=w)
    others = [k for k in range(7) if k != 3]
    for name, at in (("cov", (3, D - 1, 0)), ("mean", (3, D - 1))):
        arr = p[name].copy()
        arr[at] = np.nan
        got = _run(family, p, weights=w, **{name: arr})
        for n in NAMES:
            assert np.isnan(got[n][3]).all(), (name, n)
            assert np.array_equal(got[n][others], base[n][others], equal_nan=True), (name, n)


# ---- 6. the sign of eta_var --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_a_negative_definite_covariance_shows_in_eta_var_alone(family):
    for D, M in ((5, 33), (33, 65)):
        p = ref.make_problem(family, 7, M, D)
        w = ref.weight_pattern(7, M)
        cov = p["cov"] + 0.01 * np.eye(D)
        neg, zero = _run(family, p, weights=w, cov=-cov), _run(family, p, weights=w, cov=np.zeros_like(cov))
        assert (neg["eta_var"][w > 0] < 0.0).all() and (zero["eta_var"][w > 0] == 0.0).all()
        assert _same(neg, zero, ("eta_mean", "mean", "lpd", "elpd"))


# ---- 7. the surface ----------------------------------------------------------------------------------------------------------
def test_path_bits_argument_checks_and_the_public_function():
    import gsmvi_amd
    eng = _engine()
    p = ref.make_problem("poisson", 5, 33, 10)
    w = ref.weight_pattern(5, 33)
    y, o = ref.plant(p["y"], p["offset"], w)
    eng.last_path(reset=True)
    got = _run("poisson", p, weights=w, y=y, offset=o)
    assert eng.last_path(reset=True) == {"batched_predict", "batched_target"}
    ref.check_bad_arguments(eng.lib)
    tgt = gsmvi_amd.SharedDesignGLMTarget(p["A"], p["y"], "poisson", offset=p["offset"])
    assert not hasattr(tgt, "predict")
    r = gsmvi_amd.predict_shared_batched(tgt, p["mean"], p["cov"], p["A"], offset=o, y=y, weights=w)
    assert isinstance(r, gsmvi_amd.GLMPrediction) and all(isinstance(getattr(r, n), np.ndarray) for n in NAMES)
    assert all(np.array_equal(getattr(r, n), got[n], equal_nan=True) for n in NAMES)
    dev = [eng.asarray(p[n]) for n in ("mean", "cov")]
    rt = gsmvi_amd.predict_shared_batched(tgt, *dev, tgt.A, offset=eng.asarray(o), y=eng.asarray(y), weights=eng.asarray(w))
    assert all(isinstance(getattr(rt, n), torch.Tensor) and getattr(rt, n).is_cuda for n in NAMES)
    assert all(np.array_equal(getattr(rt, n).cpu().numpy(), got[n], equal_nan=True) for n in NAMES)
    r0 = gsmvi_amd.predict_shared_batched(tgt, p["mean"], p["cov"], p["A"][:7])     # built with an offset; none is required here
    assert r0.lpd is None and r0.elpd is None and r0.mean.shape == (5, 7) and np.isfinite(r0.mean).all()
    with pytest.raises(ValueError, match="^nodes:"):
        gsmvi_amd.predict_shared_batched(tgt, p["mean"], p["cov"], p["A"], nodes=65)
    rep = np.ascontiguousarray(np.broadcast_to(p["A"], (5, 33, 10)))
    with pytest.raises(TypeError, match=r"BatchedGLMTarget\.predict"):
        gsmvi_amd.predict_shared_batched(gsmvi_amd.BatchedGLMTarget(rep, p["y"], "poisson"), p["mean"], p["cov"], p["A"])


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------
def test_kfold_cross_validation_of_a_laplace_fit_end_to_end():
    """gaussian family, F = 4 folds x 3 values of lam on one design of (N, D) = (48, 5): the fit with the training weights
    (laplace_init_shared_batched; every problem converges), the score with the fold masks on target.A; elpd is the restatement's
    on the device's own (mean, cov) to 1e-11, and the fold-summed elpd beats the same with 25 cov for every lam"""
    import gsmvi_amd
    N, D, F = 48, 5, 4
    lams = np.array([0.1, 1.0, 10.0])
    rs = np.random.default_rng(48)
    A = rs.standard_normal((N, D)) / np.sqrt(D)
    y1 = A @ rs.standard_normal(D) + rs.standard_normal(N) / np.sqrt(2.0)
    fold = rs.permutation(N) % F
    mask = np.repeat((fold[None, :] == np.arange(F)[:, None]).astype(np.float64), len(lams), axis=0)        # problem f L + l
    K = F * len(lams)
    lam = np.tile(lams, F)
    y = np.ascontiguousarray(np.broadcast_to(y1, (K, N)))
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, "gaussian", lam, weights=1.0 - mask, noise_precision=2.0)
    mean, cov, res = gsmvi_amd.laplace_init_shared_batched(tgt)
    assert res.success.all()
    a = gsmvi_amd.predict_shared_batched(tgt, mean, cov, tgt.A, y=y, weights=mask)
    b = gsmvi_amd.predict_shared_batched(tgt, mean, 25.0 * cov, tgt.A, y=y, weights=mask)
    assert np.array_equal(np.isnan(a.lpd), mask == 0.0) and np.isfinite(a.elpd).all()
    want = ref.predict("gaussian", A, None, y, mask, 2.0, mean, cov)
    assert ref.rel(a.elpd, want["elpd"], np.maximum(1.0, want["scale_elpd"])) <= 1e-11
    assert ref.rel(a.lpd, want["lpd"]) <= 1e-11
    cv, cv25 = a.elpd.reshape(F, -1).sum(0), b.elpd.reshape(F, -1).sum(0)
    print("K-fold elpd per lam:", np.array2string(cv, precision=3), " with 25 cov:", np.array2string(cv25, precision=3))
    assert (cv > cv25).all()
