"""The batched softmax posterior predictive on the GPU (csrc/gsmvi_softmax_predict_batched.hip): prob and lpd against the longdouble
restatement (tests/softmax_predict_ref.py) at every (C, P), S around the tile of 64 draws, M around the tile of 16 rows, K and counts
of softmax_predict_ref.CASES; lpd against the leave-one-out launch's on the training rows; large linear predictors; the NaN rules
among healthy neighbours and the padded positions of the MFMA operand; run-to-run bits and the pair of path bits;
``predict_softmax_batched`` end to end."""
import numpy as np
import pytest
import torch

import psis_loo_softmax_ref as sref
import softmax_predict_ref as ref
from gsmvi_amd import predict_softmax_batched      # noqa: F401  (the feature: without it nothing here can pass)

pytestmark = pytest.mark.gpu


def _engine():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _launch(p, labels=True):
    eng = _engine()
    prob, lpd = eng.softmax_predict_batched(eng.asarray(p["X"]), None if p["lw"] is None else eng.asarray(p["lw"]), eng.asarray(p["A"]),
                                            p["C"], labels=eng.batched_labels(p["y"]) if labels else None,
                                            counts=None if p["counts"] is None else eng.batched_counts(p["counts"]))
    torch.cuda.synchronize()
    return prob.cpu().numpy(), None if lpd is None else lpd.cpu().numpy()


def _want(p):
    return ref.predict(p["A"], p["y"], p["C"], p["counts"], p["X"], p["lw"])


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_launch_matches_the_restatement(case):
    """prob and lpd against the longdouble restatement at 1e-11 relative to max(1, |value|); rows i >= n_k NaN; without labels the
    same bits of prob and no lpd"""
    p = ref.make_case(case)
    prob, lpd = _launch(p)
    assert prob.shape == (p["K"], p["M"], p["C"]) and lpd.shape == (p["K"], p["M"])
    wp, wl = _want(p)
    gp, gl = ref.rel_gap(prob, wp), ref.rel_gap(lpd, wl)
    print(f"{ref.case_id(case)}: prob {gp:.1e}, lpd {gl:.1e}, LDS {_engine().softmax_predict_lds_bytes(p['C'], p['P'])} B")
    assert gp <= ref.BAR and gl <= ref.BAR
    nk = ref.valid_rows(p["counts"], p["K"], p["M"])
    dead = np.arange(p["M"])[None, :] >= nk[:, None]
    assert np.isnan(prob[dead]).all() and np.isnan(lpd[dead]).all() and np.isfinite(prob[~dead]).all() and np.isfinite(lpd[~dead]).all()
    if (~dead).any():
        assert np.abs(prob[~dead].sum(1) - 1.0).max() <= 1e-13
    bare, none = _launch(p, labels=False)
    assert none is None and _same(bare, prob)


# ---- 2. a second reference: the leave-one-out launch's lpd on the training rows ------------------------------------------------------
@pytest.mark.parametrize("case", [sref.CASES[2], sref.CASES[4], sref.CASES[7]], ids=sref.case_id)
def test_lpd_is_the_leave_one_out_launchs_on_the_training_rows(case):
    """A_new = A, y = the training labels, the same X and lw: lpd against the lpd output of gsmvi_psis_loo_softmax_batched_f64 within
    psis_loo_softmax_ref.BAR; the rows beyond counts NaN in both"""
    p = sref.make_case(case)
    eng = _engine()
    cnt = None if p["counts"] is None else eng.batched_counts(p["counts"])
    X, lw, A, y = eng.asarray(p["X"]), eng.asarray(p["lw"]), eng.asarray(p["A"]), eng.batched_labels(p["y"])
    loo = eng.psis_loo_softmax_batched(X, eng.asarray(p["logr"]), lw, A, y, p["C"], counts=cnt)[1]
    prob, lpd = eng.softmax_predict_batched(X, lw, A, p["C"], labels=y, counts=cnt)
    torch.cuda.synchronize()
    g = ref.rel_gap(lpd.cpu().numpy(), loo.cpu().numpy())
    print(f"{sref.case_id(case)}: lpd against the leave-one-out launch {g:.1e}")
    assert g <= sref.BAR


# ---- 3. large linear predictors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ref.CASES[3], ref.CASES[7]], ids=ref.case_id)
def test_large_eta_keeps_lpd_finite_and_prob_exact(case):
    """the draws pulled to a tenth of their spread and scaled so that max |eta| is 1000, every second row labelled with its least
    likely class (S = 64: the uniform weights 1 / 64 and their sums are exact).  The maximum is subtracted before any exponential
    and lpd is a log-sum-exp of pairs, so lpd is finite and within the bar of the restatement where every l_si of the row lies
    below log(DBL_MIN) = -745 (the log of a linear-space sum would be -inf); prob is exactly 0 or 1 where the restatement's is;
    nothing is NaN"""
    p = dict(ref.make_case(case), counts=None, lw=None)
    assert p["S"] == 64
    K, S, Cc, P = p["K"], p["S"], p["C"], p["P"]
    Xc = p["X"].mean(1, keepdims=True)
    X = Xc + 0.1 * (p["X"] - Xc)
    eta = np.einsum("kmp,kscp->kmsc", p["A"], X.reshape(K, S, Cc - 1, P))
    scale = 1000.0 / np.abs(eta).max()
    eta = np.concatenate([eta * scale, np.zeros(eta.shape[:3] + (1,))], axis=3)
    y = p["y"].copy()
    y[:, ::2] = eta.mean(2).argmin(2)[:, ::2]
    p.update(X=X * scale, y=y)
    prob, lpd = _launch(p)
    wp, wl = _want(p)
    wp64 = np.asarray(wp, dtype=np.float64)
    gp, gl = ref.rel_gap(prob, wp), ref.rel_gap(lpd, wl)
    print(f"{ref.case_id(case)}, max |eta| 1000: most negative lpd {lpd.min():.1f}, {int((lpd < -745.0).sum())} rows below -745, "
          f"prob {gp:.1e}, lpd {gl:.1e}, exact zeros {int((wp64 == 0).sum())}, exact ones {int((wp64 == 1).sum())} of {wp64.size}")
    assert np.isfinite(lpd).all() and np.isfinite(prob).all() and (lpd < -745.0).any() and gl <= ref.BAR and gp <= ref.BAR
    assert (wp64 == 0).any() and (wp64 == 1).any()
    assert (prob[wp64 == 0] == 0).all() and (prob[wp64 == 1] == 1).all()


# ---- 4. confinement ------------------------------------------------------------------------------------------------------------
def _five_problems(case):
    """problems 1 and 2 of a K = 3 case without counts, twice, and one more copy of problem 1: five problems, 3 and 4 the healthy
    neighbours"""
    p = ref.make_case(case)
    idx = [1, 2, 1, 2, 1]
    out = dict(p, K=5, counts=None)
    for n in ("A", "y", "X", "lw"):
        out[n] = p[n][idx].copy()
    return out


@pytest.mark.parametrize("case", [ref.CASES[1], ref.CASES[2]], ids=ref.case_id)
def test_nan_rules_touch_only_their_own_rows_and_problems(case):
    """P % 4 != 0 (the padded operand positions): non-finite x entries in problem 0 -- the first entries of one draw, where the
    previous draw's last class would overshoot, the last entry of another, the last draw of the partial tile -- make NaN every
    row of problem 0 alone; one non-finite a entry each in two rows of problem 1 makes NaN those rows alone; a NaN in lw makes NaN
    problem 2 alone; an out-of-range label touches the lpd of its row alone; everything else keeps the bits of the clean run"""
    base = _five_problems(case)
    S, D, P, M = base["S"], base["D"], base["P"], base["M"]
    assert P % 4 != 0 and base["lw"] is not None
    cp, cl = _launch(base)
    assert np.isfinite(cp).all() and np.isfinite(cl).all()
    d = {n: base[n].copy() for n in ("A", "y", "X", "lw")}
    d["X"][0, 5, :P] = np.inf                                                 # class 0 of draw 5: the overshoot of draw 4's last class
    d["X"][0, 16, D - 1] = -np.inf                                            # the last entry of draw 16
    d["X"][0, S - 1, 0] = np.nan                                              # the last draw: its tile is partial
    d["A"][1, 0, P - 1] = np.nan                                              # next to the padded columns
    d["A"][1, M - 1, 0] = np.inf                                              # the last row: its tile is partial
    d["lw"][2, S // 2] = np.nan
    d["y"][3, 2], d["y"][3, M - 1] = base["C"], -1
    prob, lpd = _launch(dict(base, **d))
    assert np.isnan(prob[0]).all() and np.isnan(lpd[0]).all()
    hit = np.zeros(M, dtype=bool)
    hit[[0, M - 1]] = True
    assert np.isnan(prob[1][hit]).all() and np.isnan(lpd[1][hit]).all()
    assert _same(prob[1][~hit], cp[1][~hit]) and _same(lpd[1][~hit], cl[1][~hit])
    assert np.isnan(prob[2]).all() and np.isnan(lpd[2]).all()
    bad_y = np.zeros(M, dtype=bool)
    bad_y[[2, M - 1]] = True
    assert _same(prob[3], cp[3]) and np.isnan(lpd[3][bad_y]).all() and _same(lpd[3][~bad_y], cl[3][~bad_y])
    assert _same(prob[4], cp[4]) and _same(lpd[4], cl[4])
    wp, wl = ref.predict(d["A"], d["y"], base["C"], None, d["X"], d["lw"])
    assert ref.rel_gap(prob, wp) <= ref.BAR and ref.rel_gap(lpd, wl) <= ref.BAR    # (the NaN patterns are compared inside)


def test_infinite_weights():
    """-inf weights are weight 0 and match the restatement (whatever the draw holds is still checked for finiteness); +inf, or -inf
    everywhere, refuses the problem; the neighbours keep their bits"""
    base = _five_problems(ref.CASES[2])
    S = base["S"]
    cp, cl = _launch(base)
    lw = base["lw"].copy()
    lw[0, [0, 63, 64, S - 1]] = -np.inf                                       # the ends of two tiles, the partial one
    lw[1, :] = -np.inf
    lw[2, 3] = np.inf
    lw[3, 1:] = -np.inf                                                       # one draw carries everything (not normalised: as given)
    p = dict(base, lw=lw)
    prob, lpd = _launch(p)
    wp, wl = _want(p)
    gp, gl = ref.rel_gap(prob, wp), ref.rel_gap(lpd, wl)
    print(f"-inf weights: prob {gp:.1e}, lpd {gl:.1e}")
    assert gp <= ref.BAR and gl <= ref.BAR
    assert np.isfinite(prob[0]).all() and np.isfinite(lpd[0]).all() and not _same(prob[0], cp[0])
    assert np.isnan(prob[1]).all() and np.isnan(lpd[1]).all() and np.isnan(prob[2]).all() and np.isnan(lpd[2]).all()
    assert np.isfinite(prob[3]).all() and np.isfinite(lpd[3]).all()
    assert _same(prob[4], cp[4]) and _same(lpd[4], cl[4])


# ---- 5. bits and the path ----------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_the_path_is_the_pair_of_bits():
    eng = _engine()
    p = ref.make_case(ref.CASES[2])
    eng.last_path()                                                           # reset
    a = _launch(p)
    assert eng.last_path() == {"batched_predict", "batched_softmax"}
    b = _launch(p)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # a problem's bits do not depend on its neighbours
    one = {k: (v[2:3] if isinstance(v, np.ndarray) and v.shape[:1] == (3,) else v) for k, v in p.items()}
    alone = _launch(dict(one, K=1))
    assert _same(alone[0][0], a[0][2]) and _same(alone[1][0], a[1][2])
    # the largest LDS request (above 64 KB) launches: the kernel attribute is set
    big = ref.make_case(ref.CASES[5])
    assert eng.softmax_predict_lds_bytes(big["C"], big["P"]) == 69952 > 64 * 1024
    eng.last_path()
    _launch(big)
    assert eng.last_path() == {"batched_predict", "batched_softmax"}


def test_abi_checks_arguments_before_the_context():
    from gsmvi_amd import _lib
    ref.check_bad_arguments(_lib.load_library())


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
def test_predict_softmax_batched_end_to_end():
    """K = 6 three-class posteriors, laplace_init_softmax_batched as the fit, predictions on held-out rows: the uniform draws are bit
    for bit the samples of psis_batched for the same keys and call; both weightings match the restatement fed the call's own draws
    (and weights); label, elpd and the counts mask"""
    import gsmvi_amd
    K, N, M, Cc, P, S = 6, 60, 21, 3, 3, 257
    D = (Cc - 1) * P
    rs = np.random.default_rng(5)
    A = rs.standard_normal((K, N + M, P))
    y = ref.draw_labels(rs, A, 1.5 * rs.standard_normal((K, Cc - 1, P)))
    tgt = gsmvi_amd.BatchedSoftmaxTarget(A[:, :N], y[:, :N], Cc, prior_precision=1.0)
    mean, cov, res = gsmvi_amd.laplace_init_softmax_batched(tgt, as_torch=True)
    assert bool(np.asarray(res.success).all())
    A_new, y_new = A[:, N:], y[:, N:]
    counts = np.array([M, M - 4, 0, 17, M, 16])
    keys = list(range(7, 7 + K))
    mk, ck = mean.clone(), cov.clone()
    r = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, y=y_new, counts=counts, num_draws=S, call=3)
    assert torch.equal(mean, mk) and torch.equal(cov, ck) and r.nlaunch == 2 and r.psis is None and r.num_draws == S
    top = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, call=3, moments=False, as_torch=True)
    Xs, lws = top.samples.cpu().numpy(), top.log_weights.cpu().numpy()
    wp, wl = ref.predict(A_new, y_new, Cc, counts, Xs, None)
    gp, gl = ref.rel_gap(r.prob, wp), ref.rel_gap(r.lpd, wl)
    reuse = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, y=y_new, counts=counts, psis=top)
    assert reuse.nlaunch == 1 and reuse.psis is top
    for n in ("prob", "label", "lpd", "elpd"):                                # the same draws, bit for bit: the same outputs
        assert _same(getattr(reuse, n), getattr(r, n)), n
    mask = np.arange(M)[None, :] < counts[:, None]
    assert r.label.dtype == np.int64 and (r.label[~mask] == -1).all() and np.array_equal(r.label[mask], r.prob[mask].argmax(1))
    want = np.array([r.lpd[k, :counts[k]].sum() for k in range(K)])
    assert np.allclose(r.elpd, want, rtol=1e-13, atol=0) and r.elpd[2] == 0.0
    acc = float((r.label[mask] == y_new[mask]).mean())
    w = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, y=y_new, counts=counts, num_draws=S, call=3, weights="psis",
                                          as_torch=True)
    assert w.nlaunch == 3 and w.prob.is_cuda and w.label.is_cuda and w.elpd.is_cuda and w.label.dtype == torch.int64
    assert torch.equal(w.psis.samples, top.samples) and torch.equal(w.psis.log_weights, top.log_weights)
    vp, vl = ref.predict(A_new, y_new, Cc, counts, Xs, lws)
    hp, hl = ref.rel_gap(w.prob.cpu().numpy(), vp), ref.rel_gap(w.lpd.cpu().numpy(), vl)
    print(f"uniform: prob {gp:.1e}, lpd {gl:.1e}; psis: prob {hp:.1e}, lpd {hl:.1e}; accuracy {acc:.2f}, elpd per row "
          f"{r.elpd.sum() / mask.sum():.3f} (uniform) {float(w.elpd.sum()) / mask.sum():.3f} (psis), khat {np.array2string(top.khat.cpu().numpy(), precision=2)}")
    assert max(gp, gl, hp, hl) <= ref.BAR
    assert acc > 1.0 / Cc
    with pytest.raises(TypeError, match="predict_softmax_batched"):
        tgt.predict(mean, cov, A_new)
