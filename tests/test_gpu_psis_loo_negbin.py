"""The batched negative binomial PSIS leave-one-out on the GPU (csrc/gsmvi_psis_loo_negbin_batched.hip): l_si against the
longdouble restatement (tests/psis_loo_negbin_ref.py) and every other output against the restatement fed the device's own l_si, logr
and lw, at every P, S, N around the tile of observations, K, offset and counts of psis_loo_negbin_ref.CASES; the Poisson limit
against the GLM launch; the sum over the rows against the score launch; extreme draws and the draw flag; the verdicts among healthy
neighbours and the padded positions of the MFMA operand; run-to-run bits, the pair of path bits, the argument checks;
``psis_loo_negbin_batched`` end to end."""
import numpy as np
import pytest
import torch
from scipy import special

import psis_batched_ref as pref
import psis_loo_negbin_ref as ref

pytestmark = pytest.mark.gpu

NAMES = ("elpd", "lpd", "khat", "ess")
LD = ref.LD


def _engine():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _launch(p, pointwise=True):
    eng = _engine()
    out = eng.psis_loo_negbin_batched(eng.asarray(p["X"]), eng.asarray(p["logr"]), eng.asarray(p["lw"]), eng.asarray(p["A"]),
                                      eng.asarray(p["y"]), offset=None if p["offset"] is None else eng.asarray(p["offset"]),
                                      counts=None if p["counts"] is None else eng.batched_counts(p["counts"]),
                                      pointwise_loglik=pointwise)
    torch.cuda.synchronize()
    return {n: (t.cpu().numpy() if t is not None else None) for n, t in zip(NAMES + ("info", "loglik"), out)}


def _same(a, b, names=NAMES + ("info",)):
    return all(np.array_equal(a[n], b[n], equal_nan=True) for n in names)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_launch_matches_the_restatement(case):
    """l_si against the longdouble restatement at 1e-11; elpd, lpd, khat, ess and info against the restatement fed the device's
    own l_si, logr and lw (a rounding of l_si cannot then move a draw across the cutoff) at 1000 times the float64 noise floor;
    rows i >= n_k NaN with info = -3; without the pointwise block the same bits"""
    p = ref.make_case(case)
    assert ref.loo_tile(p["P"], p["S"]) == _engine().psis_loo_negbin_tile(p["P"], p["S"])
    got = _launch(p)
    assert got["loglik"].shape == (p["K"], p["N"], p["S"])
    g_ell = pref.rel_gap(got["loglik"], ref.loglik_negbin(p["A"], p["y"], p["offset"], p["counts"], p["X"]))
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


# ---- 2. the Poisson limit: the GLM launch with the poisson family -------------------------------------------------------------------
def test_large_size_matches_the_poisson_glm_launch():
    """theta = 35 in every draw of the P = 15 case against gsmvi_psis_loo_batched_f64 (poisson) on the same A, y, offset, beta draws,
    logr and lw: l_si within 1e-11, elpd and lpd within the bar, info equal -- both launches include -lgamma(y + 1), so the two
    elpd are on one scale"""
    case = next(c for c in ref.CASES if c[0] == 15)
    p = dict(ref.make_case(case))
    P = p["P"]
    p["X"] = np.concatenate([p["X"][:, :, :P], np.full((p["K"], p["S"], 1), 35.0)], axis=2)
    got = _launch(p)
    eng = _engine()
    out = eng.psis_loo_batched(eng.asarray(np.ascontiguousarray(p["X"][:, :, :P])), eng.asarray(p["logr"]), eng.asarray(p["lw"]),
                               eng.asarray(p["A"]), eng.asarray(p["y"]), "poisson", offset=eng.asarray(p["offset"]),
                               counts=eng.batched_counts(p["counts"]), pointwise_loglik=True)
    torch.cuda.synchronize()
    glm = {n: t.cpu().numpy() for n, t in zip(NAMES + ("info", "loglik"), out)}
    g_ell = pref.rel_gap(got["loglik"], glm["loglik"])
    gaps = {n: ref.rel_gap(got[n], glm[n]) for n in NAMES}
    print(f"{ref.case_id(case)} theta = 35: loglik {g_ell:.1e}, " + ", ".join(f"{n} {e:.1e}" for n, e in gaps.items()))
    assert np.array_equal(got["info"], glm["info"]) and (got["info"][1:] != -1).all()
    assert g_ell <= 1e-11
    for n in ("elpd", "lpd"):
        assert gaps[n] <= ref.BAR, (n, gaps[n])


# ---- 3. the sum over the rows: the score launch's lp ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in ref.CASES if c[3] == "2NI+3" and c[2] == 33], ids=ref.case_id)
def test_rows_sum_to_the_score_launch_lp(case):
    """for each draw sum_{i < n_k} l_si + sum lgamma(y_i + 1) - lam |beta|^2 / 2 - kap (theta - m)^2 / 2 is target.lp(x_s) of the
    score launch, within 1e-11 of sum |t_i| + 1 (t_i = l_si + lgamma(y_i + 1), the terms that the score launch sums)"""
    import gsmvi_amd
    p = ref.make_case(case)
    K, N, S, P = p["K"], p["N"], p["S"], p["P"]
    lam, tm, tk = 0.7, 1.2, 0.4
    tgt = gsmvi_amd.BatchedNegBinomialTarget(p["A"], p["y"], lam, counts=p["counts"], offset=p["offset"], log_size_mean=tm,
                                             log_size_precision=tk)
    lp = tgt.lp(tgt.engine.asarray(p["X"])).cpu().numpy()
    got = _launch(p)
    nk = ref.valid_rows(p["counts"], K, N)
    worst = 0.0
    for k in range(K):
        n = int(nk[k])
        t = got["loglik"][k, :n].astype(LD) + special.gammaln(p["y"][k, :n, None] + 1.0).astype(LD)       # (n, S)
        beta, theta = p["X"][k, :, :P].astype(LD), p["X"][k, :, P].astype(LD)
        total = t.sum(0) - LD(lam) * (beta * beta).sum(1) / 2 - LD(tk) * (theta - LD(tm)) ** 2 / 2
        scale = np.abs(t).sum(0) + 1
        worst = max(worst, float(np.max(np.abs(total - lp[k].astype(LD)) / scale)))
    print(f"{ref.case_id(case)}: sum of l_si against the score launch's lp {worst:.1e} of sum |t_i| + 1")
    assert np.isfinite(lp).all() and worst <= 1e-11


# ---- 4. extreme draws ----------------------------------------------------------------------------------------------------------------
def test_extreme_eta_minus_theta_stays_finite():
    """the beta part of the draws scaled so that max |eta - theta| is 400: e^eta is never formed, so l_si is finite and within
    1e-11 of the longdouble restatement, and no verdict is -1"""
    case = next(c for c in ref.CASES if c[0] == 15)
    p = dict(ref.make_case(case), counts=None)
    P = p["P"]
    dots = np.einsum("knp,ksp->kns", p["A"], p["X"][:, :, :P])
    rest = p["offset"][:, :, None] - p["X"][:, None, :, P]
    lo, hi = 0.0, 1e4
    for _ in range(80):                                                       # max |c dots + rest| = 400 (increasing in c out there)
        c = 0.5 * (lo + hi)
        lo, hi = (c, hi) if np.abs(c * dots + rest).max() < 400.0 else (lo, c)
    X = p["X"].copy()
    X[:, :, :P] *= lo
    p["X"] = X
    reach = np.abs(lo * dots + rest).max()
    assert 399.0 < reach <= 400.0
    got = _launch(p)
    want = ref.loglik_negbin(p["A"], p["y"], p["offset"], None, p["X"])
    g = pref.rel_gap(got["loglik"], want)
    print(f"max |eta - theta| {reach:.1f}: most negative l_si {got['loglik'].min():.1f}, loglik gap {g:.1e}, verdicts "
          f"{np.unique(got['info'])}")
    assert np.isfinite(got["loglik"]).all() and got["loglik"].min() < -100.0 and g <= ref.LOGLIK_BAR
    assert (got["info"] != -1).all() and all(np.isfinite(got[n]).all() for n in ("elpd", "lpd", "ess"))


def test_a_size_that_is_not_a_normal_number_flags_its_draw_alone():
    """theta = -709 (e^theta = 1.2e-308, below the smallest normal number), 710 and -710 (e^theta overflows, or is 0 to within a
    subnormal) each flag their own draw and nothing else: l_si NaN in that draw for every observation, every other draw keeps its
    bits, and the rows' verdict is -1.  theta = 709 is the edge on the other side: e^709 = 8.2e307 is still a normal number, so by
    the definition (the score launch's row flag, checked here on the same draws) that draw is NOT flagged and its l_si is finite."""
    import gsmvi_amd
    case = next(c for c in ref.CASES if c[0] == 9 and c[3] == "NI+1" and c[2] == 33)
    base = dict(ref.make_case(case), counts=None)
    S, P = base["S"], base["P"]
    clean = _launch(base)
    tgt = gsmvi_amd.BatchedNegBinomialTarget(base["A"], base["y"], 1.0, offset=base["offset"])
    for theta, flagged in ((709.0, False), (-709.0, True), (710.0, True), (-710.0, True)):
        X = base["X"].copy()
        X[1, 6, P] = theta
        assert bool(ref.draw_flag(X[1])[6]) == flagged and ref.draw_flag(X[1]).sum() == int(flagged)
        got = _launch(dict(base, X=X))
        lp = tgt.lp(tgt.engine.asarray(X)).cpu().numpy()
        keep = np.arange(S) != 6
        assert np.isnan(lp[1, 6]) == flagged and np.isfinite(lp[1, keep]).all()            # the score launch's flag
        assert np.array_equal(got["loglik"][1][:, keep], clean["loglik"][1][:, keep]), theta
        if flagged:
            assert np.isnan(got["loglik"][1][:, 6]).all() and (got["info"][1] == -1).all(), theta
        else:
            assert np.isfinite(got["loglik"][1][:, 6]).all(), theta
        for n in NAMES + ("info", "loglik"):
            assert np.array_equal(got[n][[0, 2]], clean[n][[0, 2]]), (theta, n)


# ---- 5. isolation ------------------------------------------------------------------------------------------------------------
def _five_problems():
    """problems 0, 1, 2 of the P = 15 case without counts, and copies of 1 and 2 as the healthy neighbours 3 and 4"""
    p = ref.make_case(next(c for c in ref.CASES if c[0] == 15))
    idx = [0, 1, 2, 1, 2]
    out = dict(p, K=5, counts=None)
    for n in ("A", "y", "offset", "X", "logr", "lw"):
        out[n] = p[n][idx].copy()
    return out


def test_verdicts_touch_only_their_own_problem():
    """a NaN entry in one draw of problem 0 (its logr NaN there too), a NaN logr row in problem 1 and constant ratios in problem 2:
    info = -1 in every row of the first two, -2 in every row of the third; problems 3 and 4 keep the bits of the unplanted run"""
    base = _five_problems()
    S, N = base["S"], base["N"]
    clean = _launch(base)
    assert (clean["info"] == 0).all()
    dirty = dict(base, X=base["X"].copy(), logr=base["logr"].copy(), lw=base["lw"].copy())
    dirty["X"][0, 7, 3] = np.nan
    dirty["logr"][0, 7] = np.nan
    dirty["logr"][1, :] = np.nan
    dirty["X"][2, :, :] = dirty["X"][2, :1, :]                                # one point S times: l_si the same at every draw
    dirty["logr"][2] = 0.25
    dirty["lw"][2] = -np.log(S)
    got = _launch(dirty)
    want = np.zeros((5, N), dtype=np.int64)
    want[0], want[1], want[2] = -1, -1, -2
    assert np.array_equal(got["info"], want)
    for n in NAMES:
        assert np.isnan(got[n][:2]).all(), n
    assert np.isposinf(got["khat"][2]).all() and np.abs(got["ess"][2] - S).max() < 1e-9 * S and np.isfinite(got["elpd"][2]).all()
    assert np.allclose(got["elpd"][2], got["loglik"][2, :, 0], rtol=1e-13, atol=0)
    # the NaN entry flags its own draw alone; a NaN logr leaves l_si alone
    keep = np.arange(S) != 7
    assert np.isnan(got["loglik"][0, :, 7]).all() and np.array_equal(got["loglik"][0][:, keep], clean["loglik"][0][:, keep])
    assert np.array_equal(got["loglik"][1], clean["loglik"][1])
    for n in NAMES + ("info", "loglik"):
        assert np.array_equal(got[n][3:], clean[n][3:]), n


@pytest.mark.parametrize("case", [c for c in ref.CASES if c[0] in (15, 17)], ids=ref.case_id)
def test_padded_operand_positions_hold_zero(case):
    """the zero-times-NaN trap: with P % 4 != 0 the k positions past P of the operand meet padded zeros of A, and theta sits right
    behind beta in memory.  Non-finite values in problem 1 -- the beta entries of one draw, all of another, theta alone, the last
    beta entry alone, the last draw (its tile is partial) -- flag exactly those draws of problem 1: every other draw of problem 1
    and all of problems 0 and 2 keep their bits"""
    base = dict(ref.make_case(case), counts=None)
    S, P = base["S"], base["P"]
    assert P % 4 != 0 and S % 64 != 0
    clean = _launch(base)
    X = base["X"].copy()
    X[1, 5, :P] = np.inf
    X[1, 9, :] = np.nan
    X[1, 16, P] = -np.inf                                                     # theta alone
    X[1, 20, P - 1] = np.nan                                                  # the last beta entry: next to the padded positions
    X[1, 70, P] = np.nan
    X[1, S - 1, 0] = np.nan                                                   # the last draw: its tile is partial
    got = _launch(dict(base, X=X))
    hit = np.zeros(S, dtype=bool)
    hit[[5, 9, 16, 20, 70, S - 1]] = True
    assert np.array_equal(ref.draw_flag(X[1]), hit)
    assert np.isnan(got["loglik"][1][:, hit]).all() and (got["info"][1] == -1).all()
    assert np.array_equal(got["loglik"][1][:, ~hit], clean["loglik"][1][:, ~hit])
    for n in NAMES + ("info", "loglik"):
        assert np.array_equal(got[n][[0, 2]], clean[n][[0, 2]]), n


# ---- 6. bits, the path, the arguments ------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_the_path_is_the_pair_of_bits():
    eng = _engine()
    p = ref.make_case(next(c for c in ref.CASES if c[0] == 17))
    eng.last_path()                                                           # reset
    a = _launch(p)
    path = eng.last_path()
    assert path == {"batched_loo", "batched_target"}
    b = _launch(p)
    assert _same(a, b, NAMES + ("info", "loglik"))
    bare = _launch(p, pointwise=False)
    assert bare["loglik"] is None and _same(bare, a)
    # a problem's bits do not depend on its neighbours
    one = {k: (v[2:3] if isinstance(v, np.ndarray) and v.shape[:1] == (3,) else v) for k, v in p.items()}
    alone = _launch(dict(one, K=1))
    assert all(np.array_equal(alone[n][0], a[n][2], equal_nan=True) for n in a)
    # the pair is this launch's alone: the GLM leave-one-out sets the first bit, the negative binomial score launch the second
    g = ref.lref.make_case(ref.lref.CASES[1])
    eng.last_path()                                                           # reset
    eng.psis_loo_batched(eng.asarray(g["X"]), eng.asarray(g["logr"]), eng.asarray(g["lw"]), eng.asarray(g["A"]), eng.asarray(g["y"]),
                         g["family"], offset=eng.asarray(g["offset"]), counts=eng.batched_counts(g["counts"]))
    assert eng.last_path() == {"batched_loo"}
    eng.negbin_batched(eng.asarray(p["X"]), eng.asarray(p["A"]), eng.asarray(p["y"]), offset=eng.asarray(p["offset"]), want="lp")
    assert eng.last_path() == {"batched_target"}
    torch.cuda.synchronize()


def test_abi_checks_arguments_before_the_context():
    from gsmvi_amd import _lib
    ref.check_bad_arguments(_lib.load_library())


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------
def test_psis_loo_negbin_batched_end_to_end():
    """K = 8 count regressions with counts, lbfgs_init_batched -> GSMBatch.fit -> psis_loo_negbin_batched: the summaries are
    psis_loo_ref.summaries of the device's pointwise outputs; psis= reuse gives the bits of the one-call form in one launch; mean
    and cov are untouched; the GLM function still refuses the target, which has gained no method"""
    import gsmvi_amd
    K, N, P, S = 8, 40, 3, 1024
    D = P + 1
    rs = np.random.default_rng(11)
    A = np.concatenate([np.ones((K, N, 1)), rs.standard_normal((K, N, P - 1))], axis=2)
    beta = np.concatenate([1.0 + 0.3 * rs.standard_normal((K, 1)), 0.4 * rs.standard_normal((K, P - 1))], axis=1)
    y = ref.draw_counts(rs, A, None, beta, np.exp(rs.uniform(0.5, 2.0, K)))
    counts = np.array([N, N - 7, N, 25, N, N, 31, N])
    tgt = gsmvi_amd.BatchedNegBinomialTarget(A, y, prior_precision=1.0, counts=counts, log_size_mean=1.0, log_size_precision=1.0)
    m0, c0, res = gsmvi_amd.lbfgs_init_batched(np.zeros((K, D)), tgt.lp, tgt.lp_g, as_torch=True)
    assert bool(np.asarray(res.success).all())
    keys = list(range(3, 3 + K))
    mean, cov = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, mean=m0, cov=c0, batch_size=8, niter=20, verbose=False,
                                                                as_torch=True)
    mk, ck = mean.clone(), cov.clone()
    r = gsmvi_amd.psis_loo_negbin_batched(tgt, mean, cov, keys, num_draws=S, pointwise_loglik=True)
    assert torch.equal(mean, mk) and torch.equal(cov, ck) and r.nlaunch == 3 and r.loglik.shape == (K, N, S)
    mask = np.arange(N)[None, :] < counts[:, None]
    assert np.array_equal(r.info != -3, mask) and (r.info[mask] == 0).all() and np.isnan(r.loglik[~mask]).all()
    s = ref.summaries(dict(elpd=r.elpd_i, lpd=r.lpd_i, khat=r.khat, info=r.info), counts, S)
    assert np.allclose(r.elpd_loo, s["elpd_loo"], rtol=1e-13, atol=0) and np.allclose(r.p_loo, s["p_loo"], rtol=1e-11, atol=1e-12)
    assert np.allclose(r.se, s["se"], rtol=1e-12, atol=0) and np.array_equal(r.n_bad, s["n_bad"])
    assert np.array_equal(r.ok, np.asarray(r.psis.ok.cpu().numpy()) & (r.n_bad == 0))
    assert (r.p_loo > 0).all() and (r.p_loo < 2 * D).all() and (r.se > 0).all()
    print(f"elpd_loo {np.array2string(r.elpd_loo, precision=2)} +- {np.array2string(r.se, precision=2)}, p_loo "
          f"{np.array2string(r.p_loo, precision=2)}, largest khat {np.nanmax(r.khat):.2f}, n_bad {r.n_bad}")
    again = gsmvi_amd.psis_loo_negbin_batched(tgt, mean, cov, keys, psis=r.psis, as_torch=True)
    assert again.nlaunch == 1 and again.loglik is None and again.elpd_i.is_cuda and again.elpd_loo.is_cuda and again.info.is_cuda
    for n in ("elpd_loo", "p_loo", "se", "elpd_i", "lpd_i", "khat", "ess", "info", "n_bad", "ok"):
        assert np.array_equal(getattr(again, n).cpu().numpy(), getattr(r, n), equal_nan=True), n
    with pytest.raises(TypeError, match="BatchedGLMTarget"):
        gsmvi_amd.psis_loo_batched(tgt, mean, cov, keys)
    assert not hasattr(tgt, "loo")
