"""The batched negative binomial posterior predictive on the GPU (csrc/gsmvi_negbin_predict_batched.hip): the log moments and lpd
against the longdouble restatement (tests/negbin_predict_ref.py) at every P, S around the tile of 64 draws, M around the tile of 16
rows, K and counts of negbin_predict_ref.CASES; lpd against the leave-one-out launch's on the training rows and the score launch's
lp under one-hot weights; large linear predictors; the NaN rules among healthy neighbours and the padded positions of the MFMA
operand; run-to-run bits and the pair of path bits; ``predict_negbin_batched`` end to end."""
import dataclasses

import numpy as np
import pytest
import torch
from scipy import special

import negbin_predict_ref as ref
import psis_loo_negbin_ref as nref
from gsmvi_amd import predict_negbin_batched      # noqa: F401  (the feature: without it nothing here can pass)

pytestmark = pytest.mark.gpu


def _engine():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _launch(p, y=True):
    eng = _engine()
    dev = lambda a: None if a is None else eng.asarray(a)      # noqa: E731
    lmom, lpd = eng.negbin_predict_batched(dev(p["X"]), dev(p["lw"]), dev(p["A"]), y=dev(p["y"]) if y else None,
                                           offset=dev(p["offset"]),
                                           counts=None if p["counts"] is None else eng.batched_counts(p["counts"]))
    torch.cuda.synchronize()
    return lmom.cpu().numpy(), None if lpd is None else lpd.cpu().numpy()


def _want(p):
    return ref.predict(p["A"], p["y"], p["offset"], p["counts"], p["X"], p["lw"])


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_launch_matches_the_restatement(case):
    """lmom and lpd against the longdouble restatement at 1e-11 relative to max(1, |value|); rows i >= n_k NaN, the others finite;
    without y the same bits of lmom and no lpd"""
    p = ref.make_case(case)
    lmom, lpd = _launch(p)
    assert lmom.shape == (p["K"], p["M"], 3) and lpd.shape == (p["K"], p["M"])
    wm, wl = p["want"]
    gm, gl = ref.rel_gap(lmom, wm), ref.rel_gap(lpd, wl)
    print(f"{ref.case_id(case)}: lmom {gm:.1e}, lpd {gl:.1e}, LDS {ref.lds_bytes(p['P'])} B")
    assert gm <= ref.BAR and gl <= ref.BAR
    nk = ref.valid_rows(p["counts"], p["K"], p["M"])
    dead = np.arange(p["M"])[None, :] >= nk[:, None]
    assert np.isnan(lmom[dead]).all() and np.isnan(lpd[dead]).all() and np.isfinite(lmom[~dead]).all() and np.isfinite(lpd[~dead]).all()
    bare, none = _launch(p, y=False)
    assert none is None and bare.tobytes() == lmom.tobytes()


# ---- 2. a second reference: the leave-one-out launch's lpd on the training rows, the score launch's lp ---------------------------------
@pytest.mark.parametrize("case", [nref.CASES[1], nref.CASES[2], nref.CASES[5]], ids=nref.case_id)
def test_lpd_is_the_leave_one_out_launchs_on_the_training_rows(case):
    """A_new = A, y and offset the training rows', the same X and lw: lpd against the lpd output of
    gsmvi_psis_loo_negbin_batched_f64 within psis_loo_negbin_ref.BAR; the rows beyond counts NaN in both"""
    p = nref.make_case(case)
    assert case[0] % 4 == 3 or p["S"] % 64 != 0
    eng = _engine()
    dev = lambda a: None if a is None else eng.asarray(a)      # noqa: E731
    cnt = None if p["counts"] is None else eng.batched_counts(p["counts"])
    X, lw, A, y, o = dev(p["X"]), dev(p["lw"]), dev(p["A"]), dev(p["y"]), dev(p["offset"])
    loo = eng.psis_loo_negbin_batched(X, dev(p["logr"]), lw, A, y, offset=o, counts=cnt)[1]
    _, lpd = eng.negbin_predict_batched(X, lw, A, y=y, offset=o, counts=cnt)
    torch.cuda.synchronize()
    g = ref.rel_gap(lpd.cpu().numpy(), loo.cpu().numpy())
    print(f"{nref.case_id(case)}: lpd against the leave-one-out launch {g:.1e}")
    assert g <= nref.BAR


@pytest.mark.parametrize("case", [ref.CASES[1], ref.CASES[2]], ids=ref.case_id)
def test_one_hot_weights_give_the_score_launchs_lp(case):
    """lw one-hot on a draw, flat priors (lam = kap = 0): sum_i (lpd_i + lgamma(y_i + 1)) over the valid rows is the score launch's
    lp at that draw, within 1e-12 relative"""
    p = ref.make_case(case)
    eng = _engine()
    K, S, M = p["K"], p["S"], p["M"]
    dev = lambda a: None if a is None else eng.asarray(a)      # noqa: E731
    cnt = None if p["counts"] is None else eng.batched_counts(p["counts"])
    lp = eng.negbin_batched(dev(p["X"]), dev(p["A"]), dev(p["y"]), offset=dev(p["offset"]), counts=cnt, prior_prec=0.0,
                            log_size_mean=0.0, log_size_prec=0.0, want="lp")
    lp = lp.cpu().numpy()
    nk = ref.valid_rows(p["counts"], K, M)
    lg = special.gammaln(p["y"] + 1.0)
    for star in (0, S - 1):
        lw = np.full((K, S), -np.inf)
        lw[:, star] = 0.0
        _, lpd = _launch(dict(p, lw=lw))
        for k in range(K):
            n = int(nk[k])
            if n:
                got = float((lpd[k, :n].astype(ref.LD) + lg[k, :n].astype(ref.LD)).sum())
                assert abs(got - lp[k, star]) <= 1e-12 * max(1.0, abs(lp[k, star])), (star, k, got, lp[k, star])


# ---- 3. large linear predictors ----------------------------------------------------------------------------------------------------
def test_large_eta_keeps_every_output_finite():
    """S = 64, uniform weights, the draws pulled to a tenth of their spread and scaled so that max |eta| is 1000: the log moments
    (about 1000 and 2000 in the rows of large eta) and lpd are finite and within the bar of the restatement, lpd also where every
    l_si of the row lies below log(DBL_MIN) = -745 (the log of a linear-space sum would be -inf); NegBinPrediction.mean is +inf
    exactly where log E[mu] is above 709.78, and nothing is NaN"""
    import gsmvi_amd
    p = dict(ref.make_case(ref.CASES[3]), counts=None, lw=None)
    assert p["S"] == 64 and p["offset"] is None
    K, S, P, M = p["K"], p["S"], p["P"], p["M"]
    Xc = p["X"].mean(1, keepdims=True)
    X = Xc + 0.1 * (p["X"] - Xc)
    eta = np.einsum("kmp,ksp->kms", p["A"], X[:, :, :P])
    X[:, :, :P] *= 1000.0 / np.abs(eta).max()
    p.update(X=X)
    eta = np.einsum("kmp,ksp->kms", p["A"], X[:, :, :P])
    assert abs(np.abs(eta).max() - 1000.0) < 1e-9
    lmom, lpd = _launch(p)
    wm, wl = _want(p)
    gm, gl = ref.rel_gap(lmom, wm), ref.rel_gap(lpd, wl)
    ell = np.asarray(ref.loglik_negbin(p["A"], p["y"], None, None, X, np.float64), dtype=np.float64)
    deep = (ell < -745.0).all(2)
    print(f"max |eta| 1000: largest lmom {lmom[..., 0].max():.1f} / {lmom[..., 1].max():.1f}, most negative lpd {lpd.min():.1f}, "
          f"{int(deep.sum())} rows with every l_si below -745, lmom {gm:.1e}, lpd {gl:.1e}")
    assert np.isfinite(lmom).all() and np.isfinite(lpd).all() and gm <= ref.BAR and gl <= ref.BAR
    assert lmom[..., 0].max() > 900.0 and lmom[..., 1].max() > 1800.0 and deep.any() and np.isfinite(lpd[deep]).all()
    # through the public function, on the same draws
    eng = _engine()
    tgt = gsmvi_amd.BatchedNegBinomialTarget(p["A"], p["y"])
    z = torch.zeros(K, S, dtype=torch.float64, device=eng.device)
    held = gsmvi_amd.PSISBatchedResult(khat=None, ess=None, log_z=None, log_weights=z, log_ratios=z, samples=eng.asarray(X),
                                       mean=None, cov=None, info=None, threshold=0.7, ok=None, nlaunch=0)
    r = gsmvi_amd.predict_negbin_batched(tgt, np.zeros((K, P + 1)), np.stack([np.eye(P + 1)] * K), p["A"], list(range(K)),
                                         y=p["y"], psis=held)
    assert r.log_moments.tobytes() == lmom.tobytes() and r.lpd.tobytes() == lpd.tobytes()
    over = lmom[..., 0] > ref.LOG_DBL_MAX
    assert over.any() and (~over).any() and np.array_equal(r.mean == np.inf, over)
    assert not np.isnan(r.mean).any() and not np.isnan(r.var).any() and not np.isnan(r.elpd).any() and (r.var[over] == np.inf).all()


# ---- 4. confinement ------------------------------------------------------------------------------------------------------------
def _five_problems(case):
    """problems 0 and 1 of a K = 3 case without counts, twice, and one more copy of problem 0: five healthy problems"""
    p = ref.make_case(case)
    idx = [0, 1, 0, 1, 0]
    out = dict(p, K=5, counts=None)
    for n in ("A", "y", "offset", "X", "lw"):
        out[n] = p[n][idx].copy()
    del out["want"]
    return out


@pytest.mark.parametrize("case", [ref.CASES[1], ref.CASES[2]], ids=ref.case_id)
def test_nan_rules_touch_only_their_own_rows_and_problems(case):
    """P % 4 != 0 (the padded operand positions).  Non-finite beta entries in three draws of problem 0 -- the first entries of one
    draw, the last beta entry of another, the last draw of the partial tile -- make NaN every row of problem 0 alone; so does
    theta = 710 or theta = -746 on one draw (e^theta is not a positive normal number), while theta = 709 and theta = -708 on draws
    of problem 4 are not flagged; one non-finite a entry each in two rows of problem 1 makes NaN those rows alone; a NaN in lw
    makes NaN problem 2 alone; problem 3 and everything else keeps the bits of the clean run"""
    base = _five_problems(case)
    S, P, M = base["S"], base["P"], base["M"]
    assert P % 4 != 0 and base["lw"] is not None
    cm, cl = _launch(base)
    assert np.isfinite(cm).all() and np.isfinite(cl).all()
    d = {n: base[n].copy() for n in ("A", "y", "offset", "X", "lw")}
    d["X"][0, 5, :2] = np.inf                                                 # the first entries of draw 5
    d["X"][0, 16, P - 1] = -np.inf                                            # the last beta entry of draw 16: next to the padded columns
    d["X"][0, S - 1, 0] = np.nan                                              # the last draw: its tile is partial
    d["lw"][0, [5, 16, S - 1]] = -np.inf                                      # (whatever its weight)
    d["A"][1, 0, P - 1] = np.nan                                              # next to the padded columns
    d["A"][1, M - 1, 0] = np.inf                                              # the last row: its tile is partial
    d["lw"][2, S // 2] = np.nan
    d["X"][4, 3, P], d["X"][4, S - 2, P] = 709.0, -708.0                      # still positive normal numbers: not flagged
    lmom, lpd = _launch(dict(base, **d))
    assert np.isnan(lmom[0]).all() and np.isnan(lpd[0]).all()
    hit = np.zeros(M, dtype=bool)
    hit[[0, M - 1]] = True
    assert np.isnan(lmom[1][hit]).all() and np.isnan(lpd[1][hit]).all()
    assert _same(lmom[1][~hit], cm[1][~hit]) and _same(lpd[1][~hit], cl[1][~hit])
    assert np.isnan(lmom[2]).all() and np.isnan(lpd[2]).all()
    assert _same(lmom[3], cm[3]) and _same(lpd[3], cl[3])
    assert np.isfinite(lmom[4]).all() and np.isfinite(lpd[4]).all()
    wm, wl = ref.predict(d["A"], d["y"], d["offset"], None, d["X"], d["lw"])
    gm, gl = ref.rel_gap(lmom, wm), ref.rel_gap(lpd, wl)                      # (the NaN patterns are compared inside)
    print(f"{ref.case_id(case)}: theta = 709 and -708 in problem 4: lmom {gm:.1e}, lpd {gl:.1e}")
    assert gm <= ref.BAR and gl <= ref.BAR
    for th in (710.0, -746.0):                                                # separately: theta alone flags the draw
        X = base["X"].copy()
        X[0, 9, P] = th
        lmom, lpd = _launch(dict(base, X=X))
        assert np.isnan(lmom[0]).all() and np.isnan(lpd[0]).all() and _same(lmom[1:], cm[1:]) and _same(lpd[1:], cl[1:]), th


def test_infinite_weights():
    """-inf weights are weight 0 and match the restatement (whatever the draw holds is still checked for finiteness); +inf, or -inf
    everywhere, refuses the problem; the neighbours keep their bits"""
    base = _five_problems(ref.CASES[2])
    S = base["S"]
    cm, cl = _launch(base)
    lw = base["lw"].copy()
    lw[0, [0, 63, 64, S - 1]] = -np.inf                                       # the ends of two tiles, the partial one
    lw[1, :] = -np.inf
    lw[2, 3] = np.inf
    lw[3, 1:] = -np.inf                                                       # one draw carries everything (not normalised: as given)
    p = dict(base, lw=lw)
    lmom, lpd = _launch(p)
    wm, wl = _want(p)
    gm, gl = ref.rel_gap(lmom, wm), ref.rel_gap(lpd, wl)
    print(f"-inf weights: lmom {gm:.1e}, lpd {gl:.1e}")
    assert gm <= ref.BAR and gl <= ref.BAR
    assert np.isfinite(lmom[0]).all() and np.isfinite(lpd[0]).all() and not _same(lmom[0], cm[0])
    assert np.isnan(lmom[1]).all() and np.isnan(lpd[1]).all() and np.isnan(lmom[2]).all() and np.isnan(lpd[2]).all()
    assert np.isfinite(lmom[3]).all() and np.isfinite(lpd[3]).all()
    assert _same(lmom[4], cm[4]) and _same(lpd[4], cl[4])


# ---- 5. bits and the path ----------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_the_path_is_the_pair_of_bits():
    eng = _engine()
    p = ref.make_case(ref.CASES[2])
    eng.last_path()                                                           # reset
    a = _launch(p)
    assert eng.last_path() == {"batched_predict", "batched_target"}
    b = _launch(p)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # a problem's bits do not depend on its neighbours
    one = {k: (v[1:2] if isinstance(v, np.ndarray) and v.shape[:1] == (3,) else v) for k, v in p.items() if k != "want"}
    alone = _launch(dict(one, K=1))
    assert _same(alone[0][0], a[0][1]) and _same(alone[1][0], a[1][1])
    # the largest LDS request
    big = ref.make_case(ref.CASES[5])
    assert ref.lds_bytes(big["P"]) == 48192
    eng.last_path()
    _launch(big)
    assert eng.last_path() == {"batched_predict", "batched_target"}


def test_abi_checks_arguments_before_the_context():
    from gsmvi_amd import _lib
    ref.check_bad_arguments(_lib.load_library())


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
def test_predict_negbin_batched_end_to_end():
    """K = 6 overdispersed count regressions, laplace_init_negbin_batched as the fit, predictions on held-out rows: the uniform
    draws are bit for bit the samples of psis_batched for the same keys and call; both weightings match the restatement fed the
    call's own draws (and weights); var against the restatement's with the bound that carries each log's absolute error into its
    exponential; var > mean; elpd and the counts mask"""
    import gsmvi_amd
    K, N, M, P, S = 6, 60, 21, 3, 257
    rs = np.random.default_rng(5)
    A = rs.standard_normal((K, N + M, P)) / np.sqrt(P)
    offset = 0.3 * rs.standard_normal((K, N + M))
    y = ref.draw_counts(rs, A, offset, 0.7 * rs.standard_normal((K, P)) + np.array([1.0, 0.0, 0.0]), np.exp(rs.uniform(0.5, 2.0, K)))
    tgt = gsmvi_amd.BatchedNegBinomialTarget(A[:, :N], y[:, :N], 1.0, offset=offset[:, :N], log_size_mean=1.5, log_size_precision=1.0)
    mean, cov, res = gsmvi_amd.laplace_init_negbin_batched(tgt, as_torch=True)
    assert bool(np.asarray(res.success).all())
    A_new, y_new, o_new = A[:, N:], y[:, N:], offset[:, N:]
    counts = np.array([M, M - 4, 0, 17, M, 16])
    keys = list(range(7, 7 + K))
    mk, ck = mean.clone(), cov.clone()
    r = gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A_new, keys, offset=o_new, y=y_new, counts=counts, num_draws=S, call=3)
    assert torch.equal(mean, mk) and torch.equal(cov, ck) and r.nlaunch == 2 and r.psis is None and r.num_draws == S
    top = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, call=3, moments=False, as_torch=True)
    Xs, lws = top.samples.cpu().numpy(), top.log_weights.cpu().numpy()
    wm, wl = ref.predict(A_new, y_new, o_new, counts, Xs, None)
    gm, gl = ref.rel_gap(r.log_moments, wm), ref.rel_gap(r.lpd, wl)            # (bit for bit the same draws, or far outside the bar)
    reuse = gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A_new, keys, offset=o_new, y=y_new, counts=counts, psis=top)
    assert reuse.nlaunch == 1 and reuse.psis is top
    names = ("mean", "var", "log_moments", "lpd", "elpd")
    for n in names:                                                           # the same draws, bit for bit: the same outputs
        assert _same(getattr(reuse, n), getattr(r, n)), n
    mask = np.arange(M)[None, :] < counts[:, None]
    for n in names[:4]:
        assert np.isfinite(getattr(r, n)[mask]).all() and np.isnan(getattr(r, n)[~mask]).all(), n
    # var: each exponential carries its log's absolute error (at most BAR L) as a relative one
    m1, m2, m2r = (np.exp(wm[..., j].astype(np.float64)) for j in (0, 1, 2))
    L = max(1.0, float(np.abs(np.asarray(wm, dtype=np.float64)[mask]).max()))
    wv = np.asarray(ref.variance(wm)[1], dtype=np.float64)
    bound = ref.BAR * L * (m1 + m2r + m2 + 2.0 * m1 * m1)
    assert (np.abs(r.var - wv)[mask] <= bound[mask]).all() and np.allclose(r.mean[mask], np.exp(r.log_moments[..., 0])[mask], rtol=1e-15, atol=0)
    assert (r.var[mask] > r.mean[mask]).all()
    want = np.array([r.lpd[k, :counts[k]].sum() for k in range(K)])
    assert np.allclose(r.elpd, want, rtol=1e-13, atol=0) and r.elpd[2] == 0.0
    inside = float((np.abs(y_new - r.mean)[mask] <= 2.0 * np.sqrt(r.var[mask])).mean())
    w = gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A_new, keys, offset=o_new, y=y_new, counts=counts, num_draws=S, call=3,
                                         weights="psis", as_torch=True)
    assert w.nlaunch == top.nlaunch + 1 and all(getattr(w, n).is_cuda for n in names)
    assert torch.equal(w.psis.samples, top.samples) and torch.equal(w.psis.log_weights, top.log_weights)
    vm, vl = ref.predict(A_new, y_new, o_new, counts, Xs, lws)
    hm, hl = ref.rel_gap(w.log_moments.cpu().numpy(), vm), ref.rel_gap(w.lpd.cpu().numpy(), vl)
    print(f"uniform: lmom {gm:.1e}, lpd {gl:.1e}; psis: lmom {hm:.1e}, lpd {hl:.1e}; inside mean +- 2 sd {inside:.2f}, elpd per row "
          f"{r.elpd.sum() / mask.sum():.3f} (uniform) {float(w.elpd.sum()) / mask.sum():.3f} (psis), khat {np.array2string(top.khat.cpu().numpy(), precision=2)}")
    assert max(gm, gl, hm, hl) <= ref.BAR
    assert not hasattr(tgt, "predict")
    assert dataclasses.is_dataclass(r)
