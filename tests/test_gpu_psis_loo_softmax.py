"""The batched softmax PSIS leave-one-out on the GPU (csrc/gsmvi_psis_loo_softmax_batched.hip): l_si against the longdouble
restatement (tests/psis_loo_softmax_ref.py) and every other output against the restatement fed the device's own l_si, logr and lw,
at every (C, P), S, N around the tile of observations, K and counts of psis_loo_softmax_ref.CASES; two classes against the GLM
launch; large linear predictors; the verdicts among healthy neighbours and the padded positions of the MFMA operand; run-to-run
bits, the pair of path bits, the argument checks; ``psis_loo_softmax_batched`` end to end."""
import numpy as np
import pytest
import torch

import psis_batched_ref as pref
import psis_loo_softmax_ref as ref

pytestmark = pytest.mark.gpu

NAMES = ("elpd", "lpd", "khat", "ess")


def _engine():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _launch(p, pointwise=True):
    eng = _engine()
    out = eng.psis_loo_softmax_batched(eng.asarray(p["X"]), eng.asarray(p["logr"]), eng.asarray(p["lw"]), eng.asarray(p["A"]),
                                       eng.batched_labels(p["y"]), p["C"],
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
    assert ref.loo_tile(p["C"], p["P"], p["S"]) == _engine().psis_loo_softmax_tile(p["C"], p["P"], p["S"])
    got = _launch(p)
    assert got["loglik"].shape == (p["K"], p["N"], p["S"])
    g_ell = pref.rel_gap(got["loglik"], ref.loglik_softmax(p["A"], p["y"], p["C"], p["counts"], p["X"]))
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
@pytest.mark.parametrize("case", [c for c in ref.CASES if c[0] == 2], ids=ref.case_id)
def test_two_classes_match_the_glm_launch(case):
    """C = 2 with P = D against gsmvi_psis_loo_batched_f64 (logistic, y = [label = 0]) on the same A, X, logr and lw: l_si within
    1e-13, the four outputs within the bar, info equal"""
    p = ref.make_case(case)
    assert p["C"] == 2 and p["P"] == p["D"]
    got = _launch(p)
    eng = _engine()
    out = eng.psis_loo_batched(eng.asarray(p["X"]), eng.asarray(p["logr"]), eng.asarray(p["lw"]), eng.asarray(p["A"]),
                               eng.asarray((p["y"] == 0).astype(np.float64)), "logistic", pointwise_loglik=True)
    torch.cuda.synchronize()
    glm = {n: t.cpu().numpy() for n, t in zip(NAMES + ("info", "loglik"), out)}
    g_ell = pref.rel_gap(got["loglik"], glm["loglik"])
    gaps = {n: ref.rel_gap(got[n], glm[n]) for n in NAMES}
    print(f"{ref.case_id(case)}: loglik {g_ell:.1e}, " + ", ".join(f"{n} {e:.1e}" for n, e in gaps.items()))
    assert np.array_equal(got["info"], glm["info"])
    assert g_ell <= 1e-13
    for n, e in gaps.items():
        assert e <= ref.BAR, (n, e)


# ---- 3. large linear predictors ----------------------------------------------------------------------------------------------------
def test_large_eta_stays_finite():
    """the draws scaled so that max |eta| is 400: the maximum is subtracted before any exponential, so l_si is finite and within
    1e-11 of the longdouble restatement, and no verdict is -1"""
    p = dict(ref.make_case(ref.CASES[2]), counts=None)
    K, S = p["K"], p["S"]
    eta = np.einsum("knp,kscp->knsc", p["A"], p["X"].reshape(K, S, p["C"] - 1, p["P"]))
    p["X"] = p["X"] * (400.0 / np.abs(eta).max())
    got = _launch(p)
    want = ref.loglik_softmax(p["A"], p["y"], p["C"], None, p["X"])
    g = pref.rel_gap(got["loglik"], want)
    print(f"max |eta| 400: most negative l_si {got['loglik'].min():.1f}, loglik gap {g:.1e}, verdicts {np.unique(got['info'])}")
    assert np.isfinite(got["loglik"]).all() and got["loglik"].min() < -100.0 and g <= ref.LOGLIK_BAR
    assert (got["info"] != -1).all() and all(np.isfinite(got[n]).all() for n in ("elpd", "lpd", "ess"))


# ---- 4. isolation ------------------------------------------------------------------------------------------------------------
def _five_problems():
    """problems 0, 1, 2 of the (3, 5) case without counts, and copies of 1 and 2 as the healthy neighbours 3 and 4"""
    p = ref.make_case(ref.CASES[2])
    idx = [0, 1, 2, 1, 2]
    out = dict(p, K=5, counts=None)
    for n in ("A", "y", "X", "logr", "lw"):
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


@pytest.mark.parametrize("case", [ref.CASES[2], ref.CASES[7]], ids=ref.case_id)
def test_padded_operand_positions_hold_zero(case):
    """the zero-times-NaN trap: with P % 4 != 0 the k positions past P of a class would meet the next class's x entries (the next
    draw's first entries at the last class) against padded zeros of A.  Non-finite x in problem 1 -- the first entries of one
    draw, all of another, the last entries of a third -- flag those draws of problem 1 alone: every other draw of problem 1 and
    all of problems 0 and 2 keep their bits"""
    base = dict(ref.make_case(case), counts=None)
    S, D, P = base["S"], base["D"], base["P"]
    assert P % 4 != 0
    clean = _launch(base)
    X = base["X"].copy()
    X[1, 5, :P] = np.inf                                                      # class 0 of draw 5: the overshoot of draw 4's last class
    X[1, 9, :] = np.nan
    X[1, 16, D - 1] = -np.inf                                                 # the last entry of draw 16
    X[1, S - 1, 0] = np.nan                                                   # the last draw: its tile is partial
    got = _launch(dict(base, X=X))
    hit = np.zeros(S, dtype=bool)
    hit[[5, 9, 16, S - 1]] = True
    assert np.isnan(got["loglik"][1][:, hit]).all() and (got["info"][1] == -1).all()
    assert np.array_equal(got["loglik"][1][:, ~hit], clean["loglik"][1][:, ~hit])
    for n in NAMES + ("info", "loglik"):
        assert np.array_equal(got[n][[0, 2]], clean[n][[0, 2]]), n


# ---- 5. bits, the path, the arguments ------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_the_path_is_the_pair_of_bits():
    eng = _engine()
    p = ref.make_case(ref.CASES[4])
    eng.last_path()                                                           # reset
    a = _launch(p)
    path = eng.last_path()
    assert path == {"batched_loo", "batched_softmax"}
    b = _launch(p)
    assert _same(a, b, NAMES + ("info", "loglik"))
    bare = _launch(p, pointwise=False)
    assert bare["loglik"] is None and _same(bare, a)
    # a problem's bits do not depend on its neighbours
    one = {k: (v[2:3] if isinstance(v, np.ndarray) and v.shape[:1] == (3,) else v) for k, v in p.items()}
    alone = _launch(dict(one, K=1))
    assert all(np.array_equal(alone[n][0], a[n][2], equal_nan=True) for n in a)
    # the pair is this launch's alone: the GLM leave-one-out sets the first bit, the softmax score launch the second
    g = ref.lref.make_case(ref.lref.CASES[1])
    eng.last_path()                                                           # reset
    eng.psis_loo_batched(eng.asarray(g["X"]), eng.asarray(g["logr"]), eng.asarray(g["lw"]), eng.asarray(g["A"]), eng.asarray(g["y"]),
                         g["family"], offset=eng.asarray(g["offset"]), counts=eng.batched_counts(g["counts"]))
    assert eng.last_path() == {"batched_loo"}
    eng.softmax_batched(eng.asarray(p["X"]), eng.asarray(p["A"]), eng.batched_labels(p["y"]), p["C"], want="lp")
    assert eng.last_path() == {"batched_softmax"}
    torch.cuda.synchronize()


def test_abi_checks_arguments_before_the_context():
    from gsmvi_amd import _lib
    ref.check_bad_arguments(_lib.load_library())


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
def test_psis_loo_softmax_batched_end_to_end():
    """K = 8 three-class posteriors, laplace_init_softmax_batched -> GSMBatch.fit -> psis_loo_softmax_batched: the summaries are
    psis_loo_ref.summaries of the device's pointwise outputs; psis= reuse gives the bits of the one-call form in one launch"""
    import gsmvi_amd
    K, N, Cc, P, S = 8, 40, 3, 3, 1024
    D = (Cc - 1) * P
    rs = np.random.default_rng(11)
    A = rs.standard_normal((K, N, P))
    y = ref.draw_labels(rs, A, rs.standard_normal((K, Cc - 1, P)))
    counts = np.array([N, N - 7, N, 25, N, N, 31, N])
    tgt = gsmvi_amd.BatchedSoftmaxTarget(A, y, Cc, prior_precision=1.0, counts=counts)
    m0, c0, res = gsmvi_amd.laplace_init_softmax_batched(tgt, as_torch=True)
    assert bool(np.asarray(res.success).all())
    keys = list(range(3, 3 + K))
    mean, cov = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, mean=m0, cov=c0, batch_size=8, niter=20, verbose=False,
                                                                as_torch=True)
    mk, ck = mean.clone(), cov.clone()
    r = gsmvi_amd.psis_loo_softmax_batched(tgt, mean, cov, keys, num_draws=S, pointwise_loglik=True)
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
    again = gsmvi_amd.psis_loo_softmax_batched(tgt, mean, cov, keys, psis=r.psis, as_torch=True)
    assert again.nlaunch == 1 and again.loglik is None and again.elpd_i.is_cuda and again.elpd_loo.is_cuda and again.info.is_cuda
    for n in ("elpd_loo", "p_loo", "se", "elpd_i", "lpd_i", "khat", "ess", "info", "n_bad", "ok"):
        assert np.array_equal(getattr(again, n).cpu().numpy(), getattr(r, n), equal_nan=True), n
    with pytest.raises(TypeError, match="BatchedGLMTarget"):
        tgt.loo(mean, cov, keys)
