"""The shared-design PSIS leave-one-out on the GPU (csrc/gsmvi_psis_loo_batched.hip, SHARED): l_si against the longdouble
restatement (tests/psis_loo_shared_ref.py) and every other output against the restatement fed the device's own l_si, logr and lw,
on every case of psis_loo_ref.CASES with A = A[0] and weights from {0, 0.5, 1, 2.5}; the bits of the per-problem launch on the
replicated design where the weights say nothing new; the weighted sum over the rows against the target's lp; the verdicts among
healthy neighbours; run-to-run bits and the pair of path bits; ``psis_loo_shared_batched`` end to end on a lambda sweep."""
import numpy as np
import pytest
import torch
from scipy import special

import psis_batched_ref as pref
import psis_loo_ref as lref
import psis_loo_shared_ref as ref
import shared_glm_ref as sref

pytestmark = pytest.mark.gpu

NAMES = ("elpd", "lpd", "khat", "ess")
ALL = NAMES + ("info", "loglik")
LD = ref.LD


def _engine():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _opt(eng, a):
    return None if a is None else eng.asarray(a)


def _tau(eng, tau):
    return tau if np.ndim(tau) == 0 else eng.batched_regs(tau)


def _out(out):
    torch.cuda.synchronize()
    return {n: (t.cpu().numpy() if t is not None else None) for n, t in zip(ALL, out)}


def _launch(p, pointwise=True):
    eng = _engine()
    return _out(eng.psis_loo_shared_batched(eng.asarray(p["X"]), eng.asarray(p["logr"]), eng.asarray(p["lw"]), eng.asarray(p["A"]),
                                            eng.asarray(p["y"]), p["family"], offset=_opt(eng, p["offset"]),
                                            weights=_opt(eng, p["weights"]), noise_prec=_tau(eng, p["tau"]),
                                            pointwise_loglik=pointwise))


def _launch_replicated(p, counts=None):
    """the per-problem launch (gsmvi_psis_loo_batched_f64) on the K-fold replicated design"""
    eng = _engine()
    return _out(eng.psis_loo_batched(eng.asarray(p["X"]), eng.asarray(p["logr"]), eng.asarray(p["lw"]),
                                     eng.asarray(sref.replicate(p["A"], p["K"])), eng.asarray(p["y"]), p["family"],
                                     offset=_opt(eng, p["offset"]), counts=None if counts is None else eng.batched_counts(counts),
                                     noise_prec=_tau(eng, p["tau"]), pointwise_loglik=True))


def _same(a, b, names=NAMES + ("info",)):
    return all(np.array_equal(a[n], b[n], equal_nan=True) for n in names)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_launch_matches_the_restatement(case):
    """l_si against the longdouble restatement at 1e-11; elpd, lpd, khat, ess and info against the restatement fed the device's
    own l_si, logr and lw at 1000 times the float64 noise floor, no row left out; the rows that are not valid NaN with info = -3;
    without the pointwise block the same bits"""
    p = ref.make_case(case)
    assert ref.loo_tile(p["D"], p["S"]) == _engine().psis_loo_tile(p["D"], p["S"])
    got = _launch(p)
    assert got["loglik"].shape == (p["K"], p["N"], p["S"])
    g_ell = pref.rel_gap(got["loglik"], ref.loglik(p["family"], p["A"], p["y"], p["offset"], p["weights"], p["tau"], p["X"]))
    want = ref.loo_batched(got["loglik"], p["logr"], p["lw"], p["weights"])
    gaps = {n: ref.rel_gap(got[n], want[n]) for n in NAMES}
    print(f"{ref.case_id(case)} N={p['N']}: loglik {g_ell:.1e}, " + ", ".join(f"{n} {e:.1e}" for n, e in gaps.items()))
    assert np.array_equal(got["info"], want["info"]), (got["info"], want["info"])
    assert g_ell <= ref.LOGLIK_BAR
    for n, e in gaps.items():
        assert e <= ref.BAR, (n, e)
    dead = ~ref.valid_mask(p["weights"], p["K"], p["N"])
    assert (got["info"][dead] == -3).all() and (got["info"][~dead] != -3).all() and (got["info"][~dead] != -1).all()
    assert np.isnan(got["loglik"][dead]).all() and np.isfinite(got["loglik"][~dead]).all()
    assert all(np.isnan(got[n][dead]).all() for n in NAMES)
    bare = _launch(p, pointwise=False)
    assert bare["loglik"] is None and _same(bare, got)


# ---- 2. the bits of the per-problem launch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lref.CASES, ids=lref.case_id)
def test_no_weights_unit_weights_and_a_prefix_mask_have_the_bits_of_the_per_problem_launch(case):
    """weights None and weights all ones: every output equals gsmvi_psis_loo_batched_f64 on the replicated A; 0 / 1 weights that
    form a prefix: its ``counts`` (y, offset, logr and lw of psis_loo_ref's case: finite everywhere)"""
    b = lref.make_case(case)
    p = dict(b, A=np.ascontiguousarray(b["A"][0]), weights=None)
    K, N = p["K"], p["N"]
    want = _launch_replicated(p)
    assert (want["info"] != -3).all()
    for w in (None, np.ones((K, N))):
        got = _launch(dict(p, weights=w))
        assert _same(got, want, ALL), "None" if w is None else "ones"
    counts = np.array([0, max(1, N // 2), N] if K == 3 else [max(1, N - 1)], dtype=np.int32)
    w = (np.arange(N)[None, :] < counts[:, None]).astype(np.float64)
    got, want = _launch(dict(p, weights=w)), _launch_replicated(p, counts)
    assert _same(got, want, ALL) and np.array_equal(got["info"] == -3, w == 0)


# ---- 3. the weighted sum over the rows: the target's lp -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in ref.CASES if c[5] == 3 and (c[4] == "2NI+3" or c[0] == "poisson")], ids=ref.case_id)
def test_weighted_rows_sum_to_the_target_lp(case):
    """for each draw sum_i v_ki (l_si - its normalising term) - lam_k |x_s|^2 / 2 over the valid rows is target.lp(x_s), within
    1e-11 relative to max(1, |lp|)"""
    import gsmvi_amd
    p = ref.make_case(case)
    K, N, fam = p["K"], p["N"], p["family"]
    lam = np.array([0.7, 0.0, 1.9])
    tgt = gsmvi_amd.SharedDesignGLMTarget(p["A"], p["y"], fam, lam, offset=p["offset"], weights=p["weights"],
                                          noise_precision=p["tau"])
    lp = tgt.lp(tgt.engine.asarray(p["X"])).cpu().numpy()
    got = _launch(p)
    ok = ref.valid_mask(p["weights"], K, N)
    tau = np.broadcast_to(np.asarray(p["tau"], dtype=np.float64), (K,))
    worst = 0.0
    for k in range(K):
        sel = np.flatnonzero(ok[k])
        norm = np.zeros(len(sel), dtype=LD)
        if fam == "poisson":
            norm = -special.gammaln(p["y"][k, sel] + 1.0).astype(LD)
        elif fam == "gaussian":
            norm = np.full(len(sel), np.log(LD(tau[k]) / (2 * LD(np.pi))) / 2)
        t = got["loglik"][k, sel].astype(LD) - norm[:, None]                                             # (n_k, S)
        x = p["X"][k].astype(LD)
        total = (p["weights"][k, sel].astype(LD)[:, None] * t).sum(0) - LD(lam[k]) * (x * x).sum(1) / 2
        worst = max(worst, float(np.max(np.abs(total - lp[k].astype(LD)) / np.maximum(1, np.abs(lp[k])))))
    print(f"{ref.case_id(case)}: weighted sum of l_si against target.lp {worst:.1e}")
    assert np.isfinite(lp).all() and worst <= 1e-11


# ---- 4. isolation --------------------------------------------------------------------------------------------------------------
def _isolation_base():
    """three poisson problems on one design (D = 10, S = 257, N = 2 NI + 3 = 11), every weight value present, rows 1 of problem 0
    and N - 2 of problem 2 valid, problem 2 with constant problem-level ratios (equal weights)"""
    b = lref.make_case(("poisson", True, 10, 257, "2NI+3", 3))
    N, S = b["N"], b["S"]
    w = np.random.default_rng(3).choice(np.array(ref.WEIGHT_VALUES), size=(3, N))
    w[0, 1], w[2, N - 2], w[1, 0], w[1, 3], w[0, 4] = 2.5, 0.5, 1.0, 0.0, 0.0
    logr, lw = b["logr"].copy(), b["lw"].copy()
    logr[2], lw[2] = 0.25, -np.log(S)
    return dict(b, A=np.ascontiguousarray(b["A"][0]), y=b["y"].copy(), offset=b["offset"].copy(), weights=w, logr=logr, lw=lw)


def test_verdicts_touch_only_their_own_row():
    """a poisson row driven to overflow (-1), a problem whose logr holds a NaN (-1 in all its valid rows), a row whose l_si is the
    same at every draw under constant problem-level ratios (-2: y = 0 and an offset of -1e4, so that l = -e^eta = -0; the design
    is shared, so a zero row of A cannot be planted in one problem alone), and NaN y with an infinite offset at every row of
    weight 0 (-3 before and after, flagging nothing): every other (k, i) keeps the bits of the batch without the planted rows"""
    base = _isolation_base()
    S, N, w = base["S"], base["N"], base["weights"]
    dead = w == 0
    assert dead.sum() >= 3 and dead.any(1).all()
    clean = _launch(base)
    assert (clean["info"][~dead] == 0).all() and (clean["info"][dead] == -3).all()
    dirty = dict(base, y=base["y"].copy(), offset=base["offset"].copy(), logr=base["logr"].copy())
    dirty["offset"][0, 1] = 800.0                                             # e^eta overflows at every draw
    dirty["logr"][1, 7] = np.nan
    dirty["y"][2, N - 2], dirty["offset"][2, N - 2] = 0.0, -1e4               # l_si = -0 at every draw
    dirty["y"][dead], dirty["offset"][dead] = np.nan, np.inf
    got = _launch(dirty)
    want = np.where(dead, -3, 0)
    want[0, 1], want[2, N - 2] = -1, -2
    want[1, ~dead[1]] = -1
    assert np.array_equal(got["info"], want)
    assert np.isnan(got["loglik"][0, 1]).all() and (got["loglik"][2, N - 2] == 0).all() and np.isposinf(got["khat"][2, N - 2])
    assert abs(got["ess"][2, N - 2] - S) < 1e-9 * S and abs(got["elpd"][2, N - 2]) < 1e-12
    planted = (want == -1) | (want == -2)
    for n in NAMES:
        assert np.isnan(got[n][want == -1]).all() and np.isnan(got[n][dead]).all(), n
        assert np.array_equal(got[n][~planted], clean[n][~planted], equal_nan=True), n
    keep = np.ones((3, N), dtype=bool)
    keep[0, 1] = keep[2, N - 2] = False                                       # (a NaN logr leaves l_si alone)
    assert np.array_equal(got["loglik"][keep], clean["loglik"][keep], equal_nan=True) and np.isnan(got["loglik"][dead]).all()


def test_a_nan_weight_removes_its_row_like_a_zero():
    base = _isolation_base()
    clean = _launch(base)
    w = base["weights"].copy()
    dead = w == 0
    w[dead] = np.nan
    got = _launch(dict(base, weights=w))
    assert _same(got, clean, ALL) and (got["info"][dead] == -3).all()


# ---- 5. bits, the path -------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_the_path_is_the_pair_of_bits():
    eng = _engine()
    p = ref.make_case(next(c for c in ref.CASES if c[2] == 17))
    assert p["K"] == 3 and p["weights"] is not None
    eng.last_path()                                                           # reset
    a = _launch(p)
    assert eng.last_path() == {"batched_loo", "batched_target"}
    b = _launch(p)
    assert _same(a, b, ALL)
    # a problem's bits do not depend on its neighbours
    for k in (1, 2):
        one = {n: (v[k:k + 1] if isinstance(v, np.ndarray) and v.shape[:1] == (3,) and n != "A" else v) for n, v in p.items()}
        assert one["A"].shape == p["A"].shape and one["weights"].shape == (1, p["N"])
        alone = _launch(dict(one, K=1))
        assert all(np.array_equal(alone[n][0], a[n][k], equal_nan=True) for n in a), k
    for D, S in ((1, 5), (10, 1024), (16, 2048), (64, 2049), (64, 4096)):
        assert eng.psis_loo_tile(D, S) == ref.loo_tile(D, S)


def test_abi_checks_arguments_before_the_context():
    from gsmvi_amd import _lib
    ref.check_bad_arguments(_lib.load_library())


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
def test_psis_loo_shared_batched_end_to_end_on_a_lambda_sweep():
    """K = 8 values of lambda on one logistic design (N, D) = (64, 10), S = 256: laplace_init_shared_batched ->
    psis_loo_shared_batched; with the same ``psis=`` handed to psis_loo_batched on the K-fold replicated target every field of the
    two results is equal bit for bit; mean and cov are untouched; one launch with ``psis=``"""
    import gsmvi_amd
    K, N, D, S = 8, 64, 10, 256
    rs = np.random.default_rng(21)
    A = rs.standard_normal((N, D)) / np.sqrt(D)
    theta = 2.0 * rs.standard_normal(D)
    y1 = (rs.uniform(size=N) < 1.0 / (1.0 + np.exp(-A @ theta))).astype(np.float64)
    y = np.ascontiguousarray(np.broadcast_to(y1, (K, N)))
    lam = 10.0 ** np.linspace(-2, 2, K)
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, "logistic", lam)
    mean, cov, res = gsmvi_amd.laplace_init_shared_batched(tgt, as_torch=True)
    assert bool(np.asarray(res.success).all())
    mk, ck = mean.clone(), cov.clone()
    keys = list(range(40, 40 + K))
    r = gsmvi_amd.psis_loo_shared_batched(tgt, mean, cov, keys, num_draws=S, as_torch=True)
    assert torch.equal(mean, mk) and torch.equal(cov, ck) and r.nlaunch == 3 and r.loglik is None
    assert r.elpd_i.is_cuda and r.elpd_loo.is_cuda and tuple(r.elpd_i.shape) == (K, N) and bool((r.info != -3).all())
    rep = gsmvi_amd.BatchedGLMTarget(sref.replicate(A, K), y, "logistic", lam)
    q = gsmvi_amd.psis_loo_batched(rep, mean, cov, keys, psis=r.psis, as_torch=True)
    assert q.nlaunch == 1
    for n in ("elpd_loo", "p_loo", "se", "elpd_i", "lpd_i", "khat", "ess", "info", "n_bad", "ok"):
        assert torch.equal(getattr(q, n), getattr(r, n)) or np.array_equal(getattr(q, n).cpu().numpy(), getattr(r, n).cpu().numpy(),
                                                                            equal_nan=True), n
    elpd, se = r.elpd_loo.cpu().numpy(), r.se.cpu().numpy()
    print(f"lambda {np.array2string(lam, precision=2)}: elpd_loo {np.array2string(elpd, precision=2)} +- "
          f"{np.array2string(se, precision=2)}, best lambda {lam[int(np.argmax(elpd))]:.2g}")
    assert np.isfinite(elpd).all() and (se > 0).all()
    again = gsmvi_amd.psis_loo_shared_batched(tgt, mean, cov, keys, psis=r.psis)
    assert again.nlaunch == 1 and np.array_equal(again.elpd_loo, elpd) and again.info.dtype == np.int64
    with pytest.raises(TypeError, match="psis_loo_shared_batched"):
        gsmvi_amd.psis_loo_batched(tgt, mean, cov, keys)
    assert not hasattr(tgt, "loo")
