"""The batched ordinal posterior predictive on the GPU (csrc/gsmvi_ordinal_predict_batched.hip): prob and lpd against the longdouble
restatement (tests/ordinal_predict_ref.py) at every (P, C), S around the tile of 64 draws, M around the tile of 16 rows, K and counts
of ordinal_predict_ref.CASES; lpd against the leave-one-out launch's on the training rows; large linear predictors; the NaN rules
among healthy neighbours and the padded positions of the MFMA operand; -inf weights at tile edges; run-to-run bits, the pair of path
bits and the above-64 KB LDS request; ``predict_ordinal_batched`` end to end."""
import numpy as np
import pytest
import torch

import ordinal_predict_ref as ref
import psis_loo_ordinal_ref as lo
from gsmvi_amd import predict_ordinal_batched      # noqa: F401  (the feature: without it nothing here can pass)

pytestmark = pytest.mark.gpu


def _engine():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _launch(p, labels=True):
    eng = _engine()
    prob, lpd = eng.ordinal_predict_batched(eng.asarray(p["X"]), None if p["lw"] is None else eng.asarray(p["lw"]), eng.asarray(p["A"]),
                                            p["C"], y=eng.batched_labels(p["y"]) if labels else None,
                                            offset=None if p["offset"] is None else eng.asarray(p["offset"]),
                                            counts=None if p["counts"] is None else eng.batched_counts(p["counts"]))
    torch.cuda.synchronize()
    return prob.cpu().numpy(), None if lpd is None else lpd.cpu().numpy()


def _want(p):
    return ref.predict(p["A"], p["y"], p["offset"], p["counts"], p["X"], p["lw"], p["C"])


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_launch_matches_the_restatement(case):
    """prob and lpd against the longdouble restatement at 1e-11 relative to max(1, |value|); rows i >= n_k NaN, the others finite;
    the rows of prob sum to 1 within 1e-13; without labels the same bits of prob and no lpd"""
    p = ref.make_case(case)
    prob, lpd = _launch(p)
    assert prob.shape == (p["K"], p["M"], p["C"]) and lpd.shape == (p["K"], p["M"])
    wp, wl = ref.expected(case)
    nk = ref.valid_rows(p["counts"], p["K"], p["M"])
    dead = np.arange(p["M"])[None, :] >= nk[:, None]
    rows = float(np.abs(prob[~dead].sum(1) - 1.0).max()) if (~dead).any() else 0.0
    gp, gl = ref.rel_gap(prob, wp), ref.rel_gap(lpd, wl)
    print(f"{ref.case_id(case)}: prob {gp:.1e}, lpd {gl:.1e}, |sum_c prob - 1| {rows:.1e}, "
          f"LDS {_engine().ordinal_predict_lds_bytes(p['P'], p['C'])} B")
    assert gp <= ref.BAR and gl <= ref.BAR
    assert np.isnan(prob[dead]).all() and np.isnan(lpd[dead]).all() and np.isfinite(prob[~dead]).all() and np.isfinite(lpd[~dead]).all()
    assert rows <= ref.ROWSUM_BAR
    bare, none = _launch(p, labels=False)
    assert none is None and _same(bare, prob)


# ---- 2. a second reference: the leave-one-out launch's lpd on the training rows ------------------------------------------------------
@pytest.mark.parametrize("case", [lo.CASES[2], lo.CASES[5], lo.CASES[6]], ids=lo.case_id)
def test_lpd_is_the_leave_one_out_launchs_on_the_training_rows(case):
    """A_new = A, y = the training labels, the same X, lw, offset and counts: lpd against the lpd output of
    gsmvi_psis_loo_ordinal_batched_f64 within psis_loo_ordinal_ref.BAR; the rows beyond counts NaN in both.  One case has C = 2"""
    p = lo.make_case(case)
    assert lo.CASES[5][1] == 2
    eng = _engine()
    cnt = None if p["counts"] is None else eng.batched_counts(p["counts"])
    off = None if p["offset"] is None else eng.asarray(p["offset"])
    X, lw, A, y = eng.asarray(p["X"]), eng.asarray(p["lw"]), eng.asarray(p["A"]), eng.batched_labels(p["y"])
    loo = eng.psis_loo_ordinal_batched(X, eng.asarray(p["logr"]), lw, A, y, p["C"], offset=off, counts=cnt)[1]
    prob, lpd = eng.ordinal_predict_batched(X, lw, A, p["C"], y=y, offset=off, counts=cnt)
    torch.cuda.synchronize()
    g = ref.rel_gap(lpd.cpu().numpy(), loo.cpu().numpy())
    print(f"{lo.case_id(case)}: lpd against the leave-one-out launch {g:.1e}")
    assert g <= lo.BAR


# ---- 3. large linear predictors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ref.CASES[3], ref.CASES[7]], ids=ref.case_id)
def test_large_eta_keeps_lpd_finite_and_prob_exact(case):
    """S = 64, uniform weights (1 / 64 and its sums are exact), the beta part of the draws and the offsets scaled so that max |eta|
    is 1000, every second row labelled with its least likely class.  The sigmoids come from exp(-|z|) and lpd is a log-sum-exp of
    pairs, so lpd is finite and within the bar of the restatement with rows below log(DBL_MIN) = -745 (the log of a linear-space
    sum would be -inf); prob is exactly 0 where the longdouble value is below 1e-400 and exactly 1 where it is within 1e-30 of 1;
    the entries in between are compared at the bar; nothing is NaN"""
    p = dict(ref.make_case(case), counts=None, lw=None)
    assert p["S"] == 64
    K, S, Cc, P = p["K"], p["S"], p["C"], p["P"]
    X, o = p["X"].copy(), p["offset"].copy()
    Xc = X[:, :, :P].mean(1, keepdims=True)
    X[:, :, :P] = Xc + 0.01 * (X[:, :, :P] - Xc)                                # beta pulled to a hundredth of its spread: a row keeps its sign
    eta = np.einsum("kmp,ksp->kms", p["A"], X[:, :, :P]) + o[:, :, None]
    scale = 1000.0 / np.abs(eta).max()
    X[:, :, :P] *= scale
    o *= scale
    eta = eta * scale
    y = p["y"].copy()
    worst = np.where(eta.mean(2) > 0, 0, Cc - 1)                              # eta far above the cutpoints: class 0 is the least likely
    for k in range(K):                                                        # every second row, the row of the problem's largest |eta| among them
        par = int(np.abs(eta[k]).max(1).argmax()) % 2
        y[k, par::2] = worst[k, par::2]
    p.update(X=X, offset=o, y=y)
    prob, lpd = _launch(p)
    wp, wl = _want(p)
    LD = ref.LD
    zero, one = wp < LD("1e-400"), np.abs(wp - 1) <= LD("1e-30")
    mid = ~zero & ~one
    gm = ref.rel_gap(prob[mid], wp[mid])
    gl = ref.rel_gap(lpd, wl)
    print(f"{ref.case_id(case)}, max |eta| 1000: most negative lpd {lpd.min():.1f}, {int((lpd < -745.0).sum())} rows below -745, "
          f"prob between {gm:.1e}, lpd {gl:.1e}, zeros {int(zero.sum())}, ones {int(one.sum())} of {wp.size}")
    assert zero.any() and one.any()                                           # (on the restatement: the test has entries of each kind)
    assert np.isfinite(lpd).all() and np.isfinite(prob).all() and (lpd < -745.0).any() and gl <= ref.BAR and gm <= ref.BAR
    assert (prob[zero] == 0.0).all() and (prob[one] == 1.0).all()


# ---- 4. confinement ------------------------------------------------------------------------------------------------------------
def _five_problems(case):
    """problems 1 and 2 of a K = 3 case without counts, twice, and one more copy of problem 1: five problems, 3 and 4 the healthy
    neighbours"""
    p = ref.make_case(case)
    idx = [1, 2, 1, 2, 1]
    out = dict(p, K=5, counts=None)
    for n in ("A", "y", "X", "lw", "offset"):
        out[n] = None if p[n] is None else p[n][idx].copy()
    return out


@pytest.mark.parametrize("case", [ref.CASES[1], ref.CASES[2]], ids=ref.case_id)
def test_nan_rules_touch_only_their_own_rows_and_problems(case):
    """P % 4 != 0 (the padded operand positions): a non-finite beta entry, a non-finite delta_0 and a delta_j of 800 (w overflows)
    in three draws of problem 0, one of them in the partial draw tile, make NaN every row of problem 0 alone; one non-finite a
    entry each in two rows of problem 1, one next to the padded columns and one in the partial row tile, makes NaN those rows
    alone; a NaN in lw makes NaN problem 2 alone; out-of-range labels touch the lpd of their rows alone; everything else keeps the
    bits of the clean run; the whole result has the restatement's NaN pattern"""
    base = _five_problems(case)
    S, P, M, Cc = base["S"], base["P"], base["M"], base["C"]
    assert P % 4 != 0 and base["lw"] is not None and Cc >= 3 and S % 64 != 0 and M % 16 != 0
    cp, cl = _launch(base)
    assert np.isfinite(cp).all() and np.isfinite(cl).all()
    d = {n: base[n].copy() for n in ("A", "y", "X", "lw")}
    d["X"][0, 5, P - 1] = np.inf                                              # a beta entry, next to the padded columns
    d["X"][0, 16, P] = np.nan                                                 # delta_0
    d["X"][0, S - 1, P + 1] = 800.0                                           # w = e^800 overflows; the last draw: its tile is partial
    d["A"][1, 0, P - 1] = np.nan                                              # next to the padded columns
    d["A"][1, M - 1, 0] = np.inf                                              # the last row: its tile is partial
    d["lw"][2, S // 2] = np.nan
    d["y"][3, 2], d["y"][3, M - 1] = Cc, -1
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
    wp, wl = ref.predict(d["A"], d["y"], base["offset"], None, d["X"], d["lw"], Cc)
    assert ref.rel_gap(prob, wp) <= ref.BAR and ref.rel_gap(lpd, wl) <= ref.BAR    # (the NaN patterns are compared inside)


# ---- 5. -inf weights ---------------------------------------------------------------------------------------------------------------
def test_infinite_weights():
    """-inf weights at tile edges are weight 0 and match the restatement; +inf, or -inf everywhere, refuses the problem; the
    neighbours keep their bits"""
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


# ---- 6. bits and the path ----------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_the_path_is_the_pair_of_bits():
    eng = _engine()
    p = ref.make_case(ref.CASES[2])
    eng.last_path()                                                           # reset
    a = _launch(p)
    assert eng.last_path() == {"batched_predict", "batched_target"}
    b = _launch(p)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # a problem's bits do not depend on K or on its neighbours
    one = {k: (v[2:3] if isinstance(v, np.ndarray) and v.shape[:1] == (3,) else v) for k, v in p.items()}
    alone = _launch(dict(one, K=1))
    assert _same(alone[0][0], a[0][2]) and _same(alone[1][0], a[1][2])
    # the largest LDS request (above 64 KB) launches: the kernel attribute is set
    big = ref.make_case(ref.CASES[5])
    assert (big["P"], big["C"]) == (1, 64)
    assert eng.ordinal_predict_lds_bytes(1, 64) == ref.lds_bytes(1, 64) == 105408 > 64 * 1024
    eng.last_path()
    _launch(big)
    assert eng.last_path() == {"batched_predict", "batched_target"}


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------
def test_predict_ordinal_batched_end_to_end():
    """K = 6 four-class posteriors, laplace_init_ordinal_batched as the fit, predictions on held-out rows: the uniform draws are bit
    for bit the samples of psis_batched for the same keys and call; both weightings match the restatement fed the call's own draws
    (and weights); psis= reuse, label, median, elpd and the counts mask; mean and cov untouched; the median class beats chance"""
    import gsmvi_amd
    K, N, M, Cc, P, S = 6, 60, 21, 4, 3, 257
    rs = np.random.default_rng(5)
    A = rs.standard_normal((K, N + M, P))
    o = 0.3 * rs.standard_normal((K, N + M))
    y = lo.draw_labels(rs, A, o, 1.2 * rs.standard_normal((K, P)), Cc)
    tgt = gsmvi_amd.BatchedOrdinalTarget(A[:, :N], y[:, :N], Cc, prior_precision=1.0, cut_precision=1.0, offset=o[:, :N])
    mean, cov, res = gsmvi_amd.laplace_init_ordinal_batched(tgt, as_torch=True)
    assert bool(np.asarray(res.success).all())
    A_new, o_new, y_new = A[:, N:], o[:, N:], y[:, N:]
    counts = np.array([M, M - 4, 0, 17, M, 16])
    keys = list(range(7, 7 + K))
    mk, ck = mean.clone(), cov.clone()
    r = gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, offset=o_new, y=y_new, counts=counts, num_draws=S, call=3)
    assert torch.equal(mean, mk) and torch.equal(cov, ck) and r.nlaunch == 2 and r.psis is None and r.num_draws == S
    top = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, call=3, moments=False, as_torch=True)
    Xs, lws = top.samples.cpu().numpy(), top.log_weights.cpu().numpy()
    wp, wl = ref.predict(A_new, y_new, o_new, counts, Xs, None, Cc)
    gp, gl = ref.rel_gap(r.prob, wp), ref.rel_gap(r.lpd, wl)
    reuse = gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, offset=o_new, y=y_new, counts=counts, psis=top)
    assert reuse.nlaunch == 1 and reuse.psis is top
    for n in ("prob", "label", "median", "lpd", "elpd"):                      # the same draws, bit for bit: the same outputs
        assert _same(getattr(reuse, n), getattr(r, n)), n
    mask = np.arange(M)[None, :] < counts[:, None]
    assert r.label.dtype == np.int64 and (r.label[~mask] == -1).all() and np.array_equal(r.label[mask], r.prob[mask].argmax(1))
    med = (np.cumsum(r.prob[mask], axis=1) < 0.5).sum(1)
    assert r.median.dtype == np.int64 and (r.median[~mask] == -1).all() and np.array_equal(r.median[mask], np.minimum(med, Cc - 1))
    want = np.array([r.lpd[k, :counts[k]].sum() for k in range(K)])
    assert np.allclose(r.elpd, want, rtol=1e-13, atol=0) and r.elpd[2] == 0.0
    acc = float((r.median[mask] == y_new[mask]).mean())
    w = gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, offset=o_new, y=y_new, counts=counts, num_draws=S, call=3,
                                          weights="psis", as_torch=True)
    assert w.nlaunch == top.nlaunch + 1 and w.prob.is_cuda and w.label.is_cuda and w.median.is_cuda and w.elpd.is_cuda
    assert w.label.dtype == torch.int64 and w.median.dtype == torch.int64
    assert torch.equal(w.psis.samples, top.samples) and torch.equal(w.psis.log_weights, top.log_weights)
    vp, vl = ref.predict(A_new, y_new, o_new, counts, Xs, lws, Cc)
    hp, hl = ref.rel_gap(w.prob.cpu().numpy(), vp), ref.rel_gap(w.lpd.cpu().numpy(), vl)
    print(f"uniform: prob {gp:.1e}, lpd {gl:.1e}; psis: prob {hp:.1e}, lpd {hl:.1e}; accuracy of the median {acc:.2f}, elpd per row "
          f"{r.elpd.sum() / mask.sum():.3f} (uniform) {float(w.elpd.sum()) / mask.sum():.3f} (psis), khat {np.array2string(top.khat.cpu().numpy(), precision=2)}")
    assert max(gp, gl, hp, hl) <= ref.BAR
    assert acc > 1.0 / Cc
    assert not hasattr(tgt, "predict")
