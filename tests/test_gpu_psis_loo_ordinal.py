"""The batched ordinal PSIS leave-one-out on the GPU (csrc/gsmvi_psis_loo_ordinal_batched.hip): l_si against the longdouble
restatement (tests/psis_loo_ordinal_ref.py) and every other output against the restatement fed the device's own l_si, logr and lw,
at every P, C, S, N around the tile of observations, K, offset and counts of psis_loo_ordinal_ref.CASES; C = 2 against the
logistic GLM launch; the sum over the rows against the score launch; extreme draws and the draw flag; the verdicts among healthy
neighbours and the padded positions of the MFMA operand; run-to-run bits and the pair of path bits; ``psis_loo_ordinal_batched``
end to end."""
import numpy as np
import pytest
import torch

import ordinal_batched_ref as oref
import psis_batched_ref as pref
import psis_loo_ordinal_ref as ref

pytestmark = pytest.mark.gpu

NAMES = ("elpd", "lpd", "khat", "ess")
ALL = NAMES + ("info", "loglik")
LD = ref.LD


def _engine():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _launch(p, pointwise=True):
    eng = _engine()
    out = eng.psis_loo_ordinal_batched(eng.asarray(p["X"]), eng.asarray(p["logr"]), eng.asarray(p["lw"]), eng.asarray(p["A"]),
                                       eng.batched_labels(p["y"]), p["C"],
                                       offset=None if p["offset"] is None else eng.asarray(p["offset"]),
                                       counts=None if p["counts"] is None else eng.batched_counts(p["counts"]),
                                       pointwise_loglik=pointwise)
    torch.cuda.synchronize()
    return {n: (t.cpu().numpy() if t is not None else None) for n, t in zip(ALL, out)}


def _same(a, b, names=NAMES + ("info",)):
    return all(np.array_equal(a[n], b[n], equal_nan=True) for n in names)


def _restated(p):
    return ref.loglik_ordinal(p["A"], p["y"], p["offset"], p["counts"], p["X"], p["C"])


def _case(P, C, nspec=None):
    return next(c for c in ref.CASES if c[:2] == (P, C) and (nspec is None or c[4] == nspec))


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_launch_matches_the_restatement(case):
    """l_si against the longdouble restatement at 1e-11; elpd, lpd, khat, ess and info against the restatement fed the device's
    own l_si, logr and lw (a rounding of l_si cannot then move a draw across the cutoff) at 1000 times the float64 noise floor;
    rows i >= n_k NaN with info = -3; without the pointwise block the same bits"""
    p = ref.make_case(case)
    assert ref.loo_tile(p["P"], p["C"], p["S"]) == _engine().psis_loo_ordinal_tile(p["P"], p["C"], p["S"])
    got = _launch(p)
    assert got["loglik"].shape == (p["K"], p["N"], p["S"])
    g_ell = pref.rel_gap(got["loglik"], _restated(p))
    want = ref.loo_batched(got["loglik"], p["logr"], p["lw"], p["counts"])
    gaps = {n: ref.rel_gap(got[n], want[n]) for n in NAMES}
    print(f"{ref.case_id(case)} N={p['N']}: loglik {g_ell:.1e}, " + ", ".join(f"{n} {e:.1e}" for n, e in gaps.items()))
    assert np.array_equal(got["info"], want["info"]), (got["info"], want["info"])
    assert g_ell <= ref.LOGLIK_BAR
    for n, e in gaps.items():
        assert e <= ref.BAR, (n, e)
    nk = ref.valid_rows(p["counts"], p["K"], p["N"])
    dead = np.arange(p["N"])[None, :] >= nk[:, None]
    assert (got["info"][dead] == -3).all() and (got["info"][~dead] != -3).all() and np.isnan(got["loglik"][dead]).all()
    assert all(np.isnan(got[n][dead]).all() for n in NAMES) and np.isfinite(got["loglik"][~dead]).all()
    bare = _launch(p, pointwise=False)
    assert bare["loglik"] is None and _same(bare, got)


# ---- 2. two classes: the GLM launch with the logistic family ------------------------------------------------------------------------
def test_two_classes_match_the_logistic_glm_launch():
    """C = 2 is logistic regression on the design [A, -1] (delta_0 is the coefficient of the last column): against
    gsmvi_psis_loo_batched_f64 (logistic) on the same draws, logr and lw: l_si within 1e-11, elpd and lpd within the bar, info
    equal"""
    case = _case(17, 2)
    p = ref.make_case(case)
    got = _launch(p)
    eng = _engine()
    A1 = np.concatenate([p["A"], -np.ones((p["K"], p["N"], 1))], axis=2)
    out = eng.psis_loo_batched(eng.asarray(p["X"]), eng.asarray(p["logr"]), eng.asarray(p["lw"]), eng.asarray(A1),
                               eng.asarray(p["y"].astype(np.float64)), "logistic", offset=eng.asarray(p["offset"]),
                               counts=eng.batched_counts(p["counts"]), pointwise_loglik=True)
    torch.cuda.synchronize()
    glm = {n: t.cpu().numpy() for n, t in zip(ALL, out)}
    g_ell = pref.rel_gap(got["loglik"], glm["loglik"])
    gaps = {n: ref.rel_gap(got[n], glm[n]) for n in NAMES}
    print(f"{ref.case_id(case)} against logistic on [A, -1]: loglik {g_ell:.1e}, " + ", ".join(f"{n} {e:.1e}" for n, e in gaps.items()))
    assert np.array_equal(got["info"], glm["info"]) and (got["info"][1:] != -1).all()
    assert g_ell <= 1e-11
    for n in ("elpd", "lpd"):
        assert gaps[n] <= ref.BAR, (n, gaps[n])


# ---- 3. the sum over the rows: the score launch's lp ----------------------------------------------------------------------------------
def test_rows_sum_to_the_score_launch_lp():
    """for each draw sum_{i < n_k} l_si - lam |beta|^2 / 2 - kap |delta|^2 / 2 is target.lp(x_s) of the score launch, within 1e-11
    of sum |l_si| + 1"""
    import gsmvi_amd
    case = _case(6, 5, "2NI+3")
    p = ref.make_case(case)
    K, N, P = p["K"], p["N"], p["P"]
    lam, kap = 0.7, 0.4
    tgt = gsmvi_amd.BatchedOrdinalTarget(p["A"], p["y"], p["C"], lam, kap, counts=p["counts"], offset=p["offset"])
    lp = tgt.lp(tgt.engine.asarray(p["X"])).cpu().numpy()
    got = _launch(p)
    nk = ref.valid_rows(p["counts"], K, N)
    worst = 0.0
    for k in range(K):
        n = int(nk[k])
        t = got["loglik"][k, :n].astype(LD)                                                             # (n, S)
        beta, delta = p["X"][k, :, :P].astype(LD), p["X"][k, :, P:].astype(LD)
        total = t.sum(0) - LD(lam) * (beta * beta).sum(1) / 2 - LD(kap) * (delta * delta).sum(1) / 2
        scale = np.abs(t).sum(0) + 1
        worst = max(worst, float(np.max(np.abs(total - lp[k].astype(LD)) / scale)))
    print(f"{ref.case_id(case)}: sum of l_si against the score launch's lp {worst:.1e} of sum |l_si| + 1")
    assert np.isfinite(lp).all() and worst <= 1e-11


# ---- 4. extreme draws ----------------------------------------------------------------------------------------------------------------
def test_extreme_eta_and_gaps_stay_finite():
    """the beta part of the draws scaled so that max |eta - cut| is 400, and delta_j = +-700 in four draws of every problem (w =
    1e304 and 1e-304: both ends of the normal range): no e^{+|z|} and no difference of sigmoids exists to overflow or cancel, so
    l_si is finite and within 1e-11 of the longdouble restatement, and no verdict is -1"""
    case = _case(9, 16)
    p = dict(ref.make_case(case), counts=None)
    P, Cc = p["P"], p["C"]
    dots = np.einsum("knp,ksp->kns", p["A"], p["X"][:, :, :P])
    cut = np.stack([oref.cutpoints(p["X"][k, :, P:])[0] for k in range(p["K"])])                       # (K, S, C - 1)
    reach_at = lambda c: np.abs((c * dots + p["offset"][:, :, None])[:, :, :, None] - cut[:, None, :, :]).max()      # noqa: E731
    lo, hi = 0.0, 1e4
    for _ in range(80):                                                       # max |c dots + o - cut| = 400 (increasing in c out there)
        c = 0.5 * (lo + hi)
        lo, hi = (c, hi) if reach_at(c) < 400.0 else (lo, c)
    reach = reach_at(lo)
    assert 399.0 < reach <= 400.0
    X = p["X"].copy()
    X[:, :, :P] *= lo
    X[:, 3, P + 2], X[:, 5, P + 1], X[:, 8, P + Cc - 2], X[:, 70, P + 3] = 700.0, -700.0, 700.0, -700.0
    p["X"] = X
    assert not any(ref.draw_flag(X[k], P).any() for k in range(p["K"]))
    got = _launch(p)
    g = pref.rel_gap(got["loglik"], _restated(p))
    print(f"max |eta - cut| {reach:.1f}: most negative l_si {got['loglik'].min():.3g}, loglik gap {g:.1e}, verdicts "
          f"{np.unique(got['info'])}")
    assert np.isfinite(got["loglik"]).all() and got["loglik"].min() < -1e300 and g <= ref.LOGLIK_BAR
    assert (got["info"] != -1).all()


# ---- 5. the flag ---------------------------------------------------------------------------------------------------------------------
def test_the_flag_is_the_score_launch_row_flag_and_touches_its_draw_alone():
    """three poisoned draws of problem 1: delta_j = 720 (e^720 overflows) at an interior class that no row of the problem is
    labelled with, delta_0 = NaN, and a beta entry +inf: each has NaN l_si in its own draw alone, for every valid row -- the score
    launch's lp is NaN at exactly these rows of X; the problem's rows get info = -1; every other draw keeps the bits of the
    unpoisoned run, and so does every output of the other problems"""
    import gsmvi_amd
    base = dict(ref.make_case(_case(9, 16)), counts=None)
    S, P, Cc, N = base["S"], base["P"], base["C"], base["N"]
    unused = next(j for j in range(1, Cc - 1) if not (base["y"][1] == j).any())
    clean = _launch(base)
    X = base["X"].copy()
    X[1, 6, P + unused], X[1, 65, P], X[1, S - 1, 2] = 720.0, np.nan, np.inf
    hit = np.zeros(S, dtype=bool)
    hit[[6, 65, S - 1]] = True
    assert np.array_equal(ref.draw_flag(X[1], P), hit)
    got = _launch(dict(base, X=X))
    tgt = gsmvi_amd.BatchedOrdinalTarget(base["A"], base["y"], Cc, 1.0, 1.0, offset=base["offset"])
    lp = tgt.lp(tgt.engine.asarray(X)).cpu().numpy()
    assert np.array_equal(np.isnan(lp[1]), hit) and np.isfinite(lp[[0, 2]]).all()                        # the score launch's flag
    assert np.isnan(got["loglik"][1][:, hit]).all() and (got["info"][1] == -1).all()
    assert np.array_equal(got["loglik"][1][:, ~hit], clean["loglik"][1][:, ~hit]) and np.isfinite(got["loglik"][1][:, ~hit]).all()
    assert all(np.isnan(got[n][1]).all() for n in NAMES)
    for n in ALL:
        assert np.array_equal(got[n][[0, 2]], clean[n][[0, 2]]), n
    # 709 is the other side of the edge: e^709 = 8.2e307 is a normal number, the draw is not flagged
    X = base["X"].copy()
    X[1, 6, P + unused] = 709.0
    edge = _launch(dict(base, X=X))
    assert np.isfinite(edge["loglik"]).all() and not ref.draw_flag(X[1], P).any()


# ---- 6. isolation ------------------------------------------------------------------------------------------------------------
def test_verdicts_touch_only_their_own_problem():
    """five problems: a poisoned one (a NaN in one draw), one with counts 0, one with constant ratios (info = -2), and two healthy
    neighbours, whose outputs are bit for bit those of a launch of the two alone"""
    p = ref.make_case(_case(9, 16))
    idx = [0, 1, 2, 1, 2]
    five = dict(p, K=5)
    for n in ("A", "y", "offset", "X", "logr", "lw"):
        five[n] = p[n][idx].copy()
    S, N = p["S"], p["N"]
    five["counts"] = np.array([N, 0, N, N, N], dtype=np.int32)
    five["X"][0, 7, 3] = np.nan
    five["X"][2, :, :] = five["X"][2, :1, :]                                  # one point S times: l_si the same at every draw
    five["logr"][2] = 0.25
    five["lw"][2] = -np.log(S)
    got = _launch(five)
    want = np.zeros((5, N), dtype=np.int64)
    want[0], want[1], want[2] = -1, -3, -2
    assert np.array_equal(got["info"], want)
    for n in NAMES:
        assert np.isnan(got[n][:2]).all(), n
    assert np.isnan(got["loglik"][1]).all() and np.isnan(got["loglik"][0, :, 7]).all()
    assert np.isfinite(np.delete(got["loglik"][0], 7, axis=1)).all()
    assert np.isposinf(got["khat"][2]).all() and np.abs(got["ess"][2] - S).max() < 1e-9 * S and np.isfinite(got["elpd"][2]).all()
    assert np.allclose(got["elpd"][2], got["loglik"][2, :, 0], rtol=1e-13, atol=0)
    two = dict(p, K=2, counts=None)
    for n in ("A", "y", "offset", "X", "logr", "lw"):
        two[n] = p[n][[1, 2]].copy()
    alone = _launch(two)
    assert (alone["info"] == 0).all()
    for n in ALL:
        assert np.array_equal(got[n][3:], alone[n]), n


# ---- 7. the operand holds beta and zeros, nothing else ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [_case(17, 2), _case(3, 2)], ids=ref.case_id)
def test_delta_is_not_in_the_operand_and_the_padding_is_zero(case):
    """P % 4 = 1 and 3, C = 2: delta_0 sits right behind beta in memory, where the operand's padded k positions would read.  With
    delta_0 = +-1e300 in some draws of problem 1 (the last draw among them: its tile is partial) eta does not move: l_si of those
    draws is the restatement's -- 0 or -1e300, delta_0 acts through the cutpoint alone --, every other draw of problem 1 and all of
    problems 0 and 2 keep their bits"""
    base = dict(ref.make_case(case), counts=None)
    S, P = base["S"], base["P"]
    assert P % 4 in (1, 3) and S % 64 != 0 and base["C"] == 2
    clean = _launch(base)
    X = base["X"].copy()
    hit = np.zeros(S, dtype=bool)
    hit[[5, 9, 20, S - 1]] = True
    X[1, [5, 20, S - 1], P], X[1, 9, P] = 1e300, -1e300
    p = dict(base, X=X)
    got = _launch(p)
    want = np.asarray(_restated(p), dtype=np.float64)
    assert np.isfinite(got["loglik"]).all() and pref.rel_gap(got["loglik"], want) <= ref.LOGLIK_BAR
    y1 = base["y"][1][:, None]
    big = np.where(hit[None, :] & ((X[1, :, P][None, :] > 0) == (y1 == 1)), -1e300, 0.0)                 # (N, S): the cutpoint alone
    assert np.array_equal(got["loglik"][1][:, hit], big[:, hit])
    assert np.array_equal(got["loglik"][1][:, ~hit], clean["loglik"][1][:, ~hit])
    for n in ALL:
        assert np.array_equal(got[n][[0, 2]], clean[n][[0, 2]]), n


# ---- 8. bits and the path ------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_the_path_is_the_pair_of_bits():
    eng = _engine()
    p = ref.make_case(_case(9, 16))
    eng.last_path()                                                           # reset
    a = _launch(p)
    assert eng.last_path() == {"batched_loo", "batched_target"}
    b = _launch(p)
    assert _same(a, b, ALL)
    # a problem's bits do not depend on its neighbours
    one = {k: (v[2:3] if isinstance(v, np.ndarray) and v.shape[:1] == (3,) else v) for k, v in p.items()}
    alone = _launch(dict(one, K=1))
    assert all(np.array_equal(alone[n][0], a[n][2], equal_nan=True) for n in a)
    # the ordinal score launch sets the second bit alone
    eng.last_path()                                                           # reset
    eng.ordinal_batched(eng.asarray(p["X"]), eng.asarray(p["A"]), eng.batched_labels(p["y"]), p["C"], offset=eng.asarray(p["offset"]),
                        want="lp")
    assert eng.last_path() == {"batched_target"}
    torch.cuda.synchronize()


def test_abi_checks_arguments_before_the_context():
    from gsmvi_amd import _lib
    ref.check_bad_arguments(_lib.load_library())


# ---- 9. end to end -------------------------------------------------------------------------------------------------------------
def test_psis_loo_ordinal_batched_end_to_end():
    """K = 3 ordinal regressions with counts, lbfgs_init_batched -> GSMBatch.fit -> psis_loo_ordinal_batched: the summaries are
    psis_loo_ref.summaries of the device's pointwise outputs; psis= reuse gives the bits of the one-call form in one launch;
    as_torch returns device tensors; mean and cov are untouched; the other functions still refuse the target, which has gained no
    method"""
    import gsmvi_amd
    K, N, P, Cc, S = 3, 60, 3, 4, 1024
    D = P + Cc - 1
    rs = np.random.default_rng(11)
    A = rs.standard_normal((K, N, P))
    y = ref.draw_labels(rs, A, None, 0.8 * rs.standard_normal((K, P)), Cc)
    counts = np.array([N, N - 7, 41])
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, Cc, 1.0, 1.0, counts=counts)
    m0, c0, res = gsmvi_amd.lbfgs_init_batched(np.zeros((K, D)), tgt.lp, tgt.lp_g, as_torch=True)
    assert bool(np.asarray(res.success).all())
    keys = list(range(3, 3 + K))
    mean, cov = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, mean=m0, cov=c0, batch_size=8, niter=20, verbose=False,
                                                                as_torch=True)
    mk, ck = mean.clone(), cov.clone()
    r = gsmvi_amd.psis_loo_ordinal_batched(tgt, mean, cov, keys, num_draws=S, pointwise_loglik=True)
    assert torch.equal(mean, mk) and torch.equal(cov, ck) and r.nlaunch == 3 and r.loglik.shape == (K, N, S)
    mask = np.arange(N)[None, :] < counts[:, None]
    assert np.array_equal(r.info != -3, mask) and (r.info[mask] == 0).all() and np.isnan(r.loglik[~mask]).all()
    s = ref.summaries(dict(elpd=r.elpd_i, lpd=r.lpd_i, khat=r.khat, info=r.info), counts, S)
    assert np.allclose(r.elpd_loo, s["elpd_loo"], rtol=1e-13, atol=0) and np.allclose(r.p_loo, s["p_loo"], rtol=1e-11, atol=1e-12)
    assert np.allclose(r.se, s["se"], rtol=1e-12, atol=0) and np.array_equal(r.n_bad, s["n_bad"])
    assert np.array_equal(r.ok, np.asarray(r.psis.ok.cpu().numpy()) & (r.n_bad == 0))
    assert (r.p_loo > 0).all() and (r.p_loo < 2 * D).all() and (r.se > 0).all()
    assert (r.loglik[mask] < 0).all()
    print(f"elpd_loo {np.array2string(r.elpd_loo, precision=2)} +- {np.array2string(r.se, precision=2)}, p_loo "
          f"{np.array2string(r.p_loo, precision=2)}, largest khat {np.nanmax(r.khat):.2f}, n_bad {r.n_bad}")
    again = gsmvi_amd.psis_loo_ordinal_batched(tgt, mean, cov, keys, psis=r.psis, as_torch=True)
    assert again.nlaunch == 1 and again.loglik is None and again.elpd_i.is_cuda and again.elpd_loo.is_cuda and again.info.is_cuda
    for n in ("elpd_loo", "p_loo", "se", "elpd_i", "lpd_i", "khat", "ess", "info", "n_bad", "ok"):
        assert np.array_equal(getattr(again, n).cpu().numpy(), getattr(r, n), equal_nan=True), n
    with pytest.raises(TypeError, match="BatchedGLMTarget"):
        gsmvi_amd.psis_loo_batched(tgt, mean, cov, keys)
    assert not hasattr(tgt, "loo")
