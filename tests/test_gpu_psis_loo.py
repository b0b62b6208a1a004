"""The batched PSIS leave-one-out on the GPU (csrc/gsmvi_psis_loo_batched.hip): l_si against the longdouble restatement
(tests/psis_loo_ref.py) and every other output against the restatement fed the device's own l_si, logr and lw, at every family,
D, S, N around the tile of observations, K and counts of psis_loo_ref.CASES; the weights entry on the same ratios; the three
verdicts among healthy neighbours; run-to-run bits, the path bit, the argument checks; ``psis_loo_batched`` end to end."""
import numpy as np
import pytest
import torch

import psis_batched_ref as pref
import psis_loo_ref as ref

pytestmark = pytest.mark.gpu

NAMES = ("elpd", "lpd", "khat", "ess")


def _engine():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _launch(p, pointwise=True):
    eng = _engine()
    tau = p["tau"] if np.ndim(p["tau"]) == 0 else eng.batched_regs(p["tau"])
    out = eng.psis_loo_batched(eng.asarray(p["X"]), eng.asarray(p["logr"]), eng.asarray(p["lw"]), eng.asarray(p["A"]),
                               eng.asarray(p["y"]), p["family"], offset=None if p["offset"] is None else eng.asarray(p["offset"]),
                               counts=None if p["counts"] is None else eng.batched_counts(p["counts"]), noise_prec=tau,
                               pointwise_loglik=pointwise)
    torch.cuda.synchronize()
    return {n: (t.cpu().numpy() if t is not None else None) for n, t in zip(NAMES + ("info", "loglik"), out)}


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_launch_matches_the_restatement(case):
    """l_si against the longdouble restatement at 1e-11; elpd, lpd, khat, ess and info against the restatement fed the device's
    own l_si, logr and lw (a rounding of l_si cannot then move a draw across the cutoff) at 1000 times the float64 noise floor;
    without the pointwise block the same bits"""
    p = ref.make_case(case)
    assert ref.loo_tile(p["D"], p["S"]) == _engine().psis_loo_tile(p["D"], p["S"])
    got = _launch(p)
    g_ell = pref.rel_gap(got["loglik"], ref.loglik(p["family"], p["A"], p["y"], p["offset"], p["counts"], p["tau"], p["X"]))
    want = ref.loo_batched(got["loglik"], p["logr"], p["lw"], p["counts"])
    assert np.array_equal(got["info"], want["info"]), (got["info"], want["info"])
    gaps = {n: ref.rel_gap(got[n], want[n]) for n in NAMES}
    print(f"{ref.case_id(case)} N={p['N']}: loglik {g_ell:.1e}, " + ", ".join(f"{n} {e:.1e}" for n, e in gaps.items()))
    assert g_ell <= ref.LOGLIK_BAR
    for n, e in gaps.items():
        assert e <= ref.BAR, (n, e)
    if p["counts"] is not None:
        assert (got["info"][0] == -3).all() and (got["info"][2] != -3).all() and np.isnan(got["loglik"][0]).all()
    bare = _launch(p, pointwise=False)
    assert bare["loglik"] is None and all(np.array_equal(bare[n], got[n], equal_nan=True) for n in NAMES + ("info",))


# ---- 2. the cross-check without the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ref.CASES[4], ref.CASES[6], ref.CASES[-2]], ids=ref.case_id)
def test_weights_entry_on_the_same_ratios_gives_khat_and_ess(case):
    p = ref.make_case(case)
    got = _launch(p)
    eng = _engine()
    rho = (p["logr"][:, None, :] - got["loglik"]).reshape(p["K"] * p["N"], p["S"])
    lw, khat, ess, log_z, info = eng.psis_weights_batched(eng.asarray(rho))
    torch.cuda.synchronize()
    live = (got["info"] != -3).reshape(-1)
    khat, ess, info = (t.cpu().numpy()[live] for t in (khat, ess, info))
    assert np.array_equal(info, got["info"].reshape(-1)[live])
    gk, ge = pref.rel_gap(got["khat"].reshape(-1)[live], khat), pref.rel_gap(got["ess"].reshape(-1)[live], ess)
    bits = np.array_equal(got["khat"].reshape(-1)[live], khat) and np.array_equal(got["ess"].reshape(-1)[live], ess)
    print(f"{ref.case_id(case)}: khat {gk:.1e}, ess {ge:.1e}, bits equal: {bits}")
    assert gk <= ref.BAR and ge <= ref.BAR


# ---- 3. isolation ------------------------------------------------------------------------------------------------------------
def test_verdicts_touch_only_their_own_row():
    """a poisson row driven to overflow (-1), a problem whose logr holds a NaN (-1 in all its rows) and a row with fewer than five
    distinct ratios (-2: plain weights, khat = +inf); every other (k, i) keeps the bits of the batch without the planted rows"""
    base = dict(ref.make_case(("poisson", True, 10, 257, "2NI+3", 3)), counts=None)
    S, N = base["S"], base["N"]
    base["logr"] = base["logr"].copy()
    base["lw"] = base["lw"].copy()
    base["logr"][2] = 0.25                                                    # problem 2: constant ratios, so equal weights
    base["lw"][2] = -np.log(S)
    clean = _launch(base)
    assert (clean["info"] == 0).all()
    dirty = dict(base, offset=base["offset"].copy(), logr=base["logr"].copy(), A=base["A"].copy())
    dirty["offset"][0, 1] = 800.0                                             # e^eta overflows at every draw
    dirty["logr"][1, 7] = np.nan
    dirty["A"][2, N - 2] = 0.0                                                # eta = offset: l_si the same at every draw
    got = _launch(dirty)
    want = np.zeros((3, N), dtype=np.int64)
    want[0, 1], want[1], want[2, N - 2] = -1, -1, -2
    assert np.array_equal(got["info"], want)
    assert np.isnan(got["loglik"][0, 1]).all() and np.isposinf(got["khat"][2, N - 2])
    assert abs(got["ess"][2, N - 2] - S) < 1e-9 * S and np.isfinite(got["elpd"][2, N - 2])
    planted = want != 0
    for n in NAMES:
        assert np.isnan(got[n][want == -1]).all(), n
        assert np.array_equal(got[n][~planted], clean[n][~planted]), n
    assert np.array_equal(got["loglik"][[0, 2]][:, [0, 2]], clean["loglik"][[0, 2]][:, [0, 2]])


# ---- 4. bits, the path, the arguments ------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_the_path_bit_is_set():
    eng = _engine()
    p = ref.make_case(ref.CASES[4])
    eng.last_path()
    a = _launch(p)
    path = eng.last_path()
    assert path == {"batched_loo"} and not any(n.endswith("_generic") for n in path)
    b = _launch(p)
    assert all(np.array_equal(a[n], b[n], equal_nan=True) for n in a)
    # a problem's bits do not depend on its neighbours
    one = {k: (v[2:3] if isinstance(v, np.ndarray) and v.shape[:1] == (3,) else v) for k, v in p.items()}
    alone = _launch(dict(one, K=1))
    assert all(np.array_equal(alone[n][0], a[n][2], equal_nan=True) for n in a)


def test_abi_checks_arguments_before_the_context():
    from gsmvi_amd import _lib
    ref.check_bad_arguments(_lib.load_library())


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------
def test_psis_loo_batched_end_to_end_on_logistic_posteriors():
    """K = 4 logistic posteriors from laplace_init_batched: elpd_loo is the masked sum of elpd_i; psis= reuse gives the bits of the
    one-call form; psis_batched gives the same bits before and after"""
    import gsmvi_amd
    K, N, D, S = 4, 40, 4, 256
    rs = np.random.RandomState(11)
    A = 1.5 * rs.standard_normal((K, N, D)) / np.sqrt(D)
    theta = rs.standard_normal((K, D))
    y = (rs.random_sample((K, N)) < 1.0 / (1.0 + np.exp(-np.einsum("knd,kd->kn", A, theta)))).astype(np.float64)
    counts = np.array([N, N - 7, N, 25])
    tgt = gsmvi_amd.BatchedLogisticTarget(A, y, prior_precision=1.0, counts=counts)
    mean, cov, res = gsmvi_amd.laplace_init_batched(tgt, as_torch=True)
    assert bool(np.asarray(res.success).all())
    keys = [3, 4, 5, 6]
    fields = ("khat", "ess", "log_z", "log_weights", "log_ratios", "samples", "info")
    before = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, moments=False, as_torch=True)
    m0, c0 = mean.clone(), cov.clone()
    r = gsmvi_amd.psis_loo_batched(tgt, mean, cov, keys, num_draws=S)
    assert torch.equal(mean, m0) and torch.equal(cov, c0) and r.nlaunch == 3 and r.loglik is None
    mask = np.arange(N)[None, :] < counts[:, None]
    assert np.array_equal(r.info != -3, mask) and (r.info[mask] == 0).all()
    assert np.allclose(r.elpd_loo, np.where(mask, r.elpd_i, 0.0).sum(1), rtol=1e-13, atol=0)
    assert np.allclose(r.p_loo, np.where(mask, r.lpd_i - r.elpd_i, 0.0).sum(1), rtol=1e-12, atol=1e-12)
    assert (r.p_loo > 0).all() and (r.p_loo < 2 * D).all() and (r.se > 0).all()
    assert np.array_equal(r.n_bad, (mask & ((r.info != 0) | (r.khat >= r.threshold))).sum(1))
    assert np.array_equal(r.ok, before.ok.cpu().numpy() & (r.n_bad == 0))
    print(f"elpd_loo {np.array2string(r.elpd_loo, precision=2)} +- {np.array2string(r.se, precision=2)}, p_loo "
          f"{np.array2string(r.p_loo, precision=2)}, largest khat {np.nanmax(r.khat):.2f}, n_bad {r.n_bad}")
    again = gsmvi_amd.psis_loo_batched(tgt, mean, cov, keys, psis=before, as_torch=True, pointwise_loglik=True)
    assert again.nlaunch == 1 and again.elpd_i.is_cuda and tuple(again.loglik.shape) == (K, N, S)
    for n in ("elpd_loo", "p_loo", "se", "elpd_i", "lpd_i", "khat", "ess", "info", "n_bad", "ok"):
        assert np.array_equal(getattr(again, n).cpu().numpy(), getattr(r, n), equal_nan=True), n
    via = tgt.loo(mean, cov, keys, num_draws=S)
    assert np.array_equal(via.elpd_i, r.elpd_i, equal_nan=True)
    after = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, moments=False, as_torch=True)
    for n in fields:
        assert torch.equal(getattr(after, n), getattr(before, n)), n
        assert torch.equal(getattr(r.psis, n), getattr(before, n)), n
