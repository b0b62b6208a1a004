"""The negative binomial Laplace initialiser without a GPU: the restatements of tests/negbin_laplace_ref.py against the mpmath
truth of the link curvature (tests/negbin_curv_truth.py), against central differences of the score restatement and against each
other; the last-pivot rule on the named test sets; the margins of the trajectories the GPU test replays; the host logic of
``laplace_init_negbin_batched`` and ``neg_hessian_negbin_batched`` on the stand-in engine; the C ABI's declarations and argument
checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import negbin_batched_ref as nref
import negbin_curv_truth as ct
import negbin_laplace_ref as ref
from gsmvi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the link curvature ---------------------------------------------------------------------------------------------------------
def test_the_committed_truth_table_is_the_grid_and_mpmath_reproduces_it():
    """the table covers negbin_link_truth.grid(); a spread of its points recomputed with mpmath (60 and 120 digits agreeing) gives
    the committed values and scales"""
    pytest.importorskip("mpmath")
    tab = ct.load_table()
    eta, theta, y = ct.grid()
    assert all(tab[q].shape == (2, len(eta)) and tab["scale_" + q].shape == (len(eta),) for q in ct.QUANTITIES)
    for i in range(3, len(eta), 97):
        if abs(eta[i] - theta[i]) > 100:                                # (the 700-digit derivatives: one of them is enough)
            continue
        v = ct.values(eta[i], theta[i], y[i])
        for q in ct.QUANTITIES:
            assert ct.split(v[q]) == (tab[q][0, i], tab[q][1, i]), (q, i)
            assert np.nextafter(float(v["scale_" + q]), 0.0) == tab["scale_" + q][i], (q, i)


def test_float64_restatement_of_the_curvature_is_within_c_cpu_of_the_truth():
    """the worst ratio over the whole grid per quantity is C_CPU (recorded in negbin_curv_truth); the GPU bound max(16, 4 C_CPU)
    follows from it and not from any device figure; the long double restatement, the GPU tests' reference, is well inside one"""
    tab = ct.load_table()
    eta, theta, y = ct.grid()
    got = ref.curv(eta, theta, y)[3:]
    ld = ref.curv_ld(eta, theta, y)[3:6]
    for q, v, w in zip(ct.QUANTITIES, got, ld):
        worst, worst_ld = ct.ratio(v, tab, q).max(), ct.ratio(w.astype(np.float64), tab, q).max()
        print(f"{q}: float64 restatement {worst:.3f} (C_CPU {ct.C_CPU[q]}), long double {worst_ld:.3f}, GPU bound {ct.c_gpu(q)}")
        assert worst <= ct.C_CPU[q] and worst > 0.5 * ct.C_CPU[q], (q, worst)
        assert worst_ld <= 0.5 and ct.c_gpu(q) == max(16.0, 4.0 * ct.C_CPU[q])
    # the first three outputs are the score restatement's, bit for bit
    for a, b in zip(ref.curv(eta, theta, y)[:3], nref.link(eta, theta, y)):
        assert np.array_equal(a, b, equal_nan=True)


def test_r_squared_dtg_neither_underflows_nor_cancels():
    """r = 1e-200 (r^2 = 0 in float64) with y = 3: r dps -> 1 and r^2 dtg -> -1, both from their terms j = 0, and what is left of
    w_tt is sigma(d) y sigma(-d); a product r^2 dtg formed from r^2 would have lost the -1"""
    theta = np.log(1e-200)
    eta, y = np.array([theta + 0.5]), np.array([3.0])
    wtt = ref.curv(eta, np.array([theta]), y)[5]
    ld = ref.curv_ld(eta, np.array([theta]), y)[5]
    sg = 1.0 / (1.0 + np.exp(-0.5))
    assert abs(wtt[0] - float(ld[0])) <= 4e-16 and abs(wtt[0] - 3.0 * sg * (1.0 - sg)) <= 1e-13


@pytest.mark.parametrize("N,P", [(7, 1), (40, 3), (33, 16)])
def test_restated_h_is_the_central_difference_of_the_restated_score(N, P):
    """H of ``evaluate`` against central differences of negbin_batched_ref.score_and_lp_ld (the existing score restatement), with
    offset, counts and per-problem priors (kap = 0 and lam = 0 for problem 0)"""
    K = 4
    A, y, o, counts, lam, tm, tk, X = nref.make_inputs(K, N, P, 1, theta_lo=-0.5, theta_hi=3.0)
    X = X[:, 0, :] * 0.5
    H, sH = ref.neg_hessian(A, y, o, counts, lam, tm, tk, X, L=np.longdouble)
    h = 1e-5
    for k in range(K):
        for j in range(P + 1):
            xp, xm = X.copy(), X.copy()
            xp[k, j] += h
            xm[k, j] -= h
            gp = nref.score_and_lp_ld(A, y, o, counts, lam, tm, tk, xp[:, None, :])[0][k, 0]
            gm = nref.score_and_lp_ld(A, y, o, counts, lam, tm, tk, xm[:, None, :])[0][k, 0]
            fd = -np.asarray((gp - gm) / (2 * h), dtype=np.float64)
            assert np.allclose(fd, H[k, :, j], rtol=0, atol=2e-8 * max(1.0, sH[k].max())), (k, j, np.abs(fd - H[k, :, j]).max())
        assert np.array_equal(H[k], H[k].T)
    # float64 and long double restatements agree to 1e-13 of the scale
    H64 = ref.neg_hessian(A, y, o, counts, lam, tm, tk, X)[0]
    assert (np.abs(H64 - H) <= 1e-13 * sH).all()
    # problem 1 has counts = 0: its Hessian is its prior
    assert np.array_equal(H[1], np.diag([lam[1]] * P + [tk[1]]))


def test_flag_rules_of_the_restatement():
    A, y, o, counts, lam, tm, tk, X = nref.make_inputs(3, 12, 2, 1, poison=False)
    X = X[:, 0, :].copy()
    X[0, 2], X[1, 0] = 800.0, np.inf
    H = ref.neg_hessian(A, y, o, None, 1.0, 0.0, 1.0, X)[0]
    assert np.isnan(H[0]).all() and np.isnan(H[1]).all() and np.isfinite(H[2]).all()
    cov, info = ref.inverse(H[0])
    assert np.array_equal(cov, np.eye(3)) and info == 1


# ---- 2. the last-pivot rule -------------------------------------------------------------------------------------------------------
def test_factor_is_a_cholesky_factorisation_and_the_rule_replaces_exactly_the_last_pivot():
    rs = np.random.RandomState(5)
    M = rs.standard_normal((6, 6))
    H = M @ M.T + 0.1 * np.eye(6)
    info, R, notes = ref.factor(H, True)
    assert info == 0 and not notes["mod"] and np.allclose(R.T @ R, H, atol=1e-13) and np.allclose(R, np.linalg.cholesky(H).T)
    H2 = H.copy()
    H2[5, 5] -= 2.0 * R[5, 5] ** 2                                       # the last Schur complement changes sign
    assert ref.factor(H2)[0] == 6 and ref.factor(H2, False)[2]["margin"] > 1e-3
    info, R2, notes = ref.factor(H2, True)
    assert info == 0 and notes["mod"] and np.allclose(R2, R, atol=1e-12)   # |s| is the old pivot
    assert np.linalg.eigvalsh(R2.T @ R2).min() > 0 and np.linalg.eigvalsh(H2).min() < 0
    H3 = H.copy()
    H3[5, 5] -= R[5, 5] ** 2 * (1 - 1e-16)                               # s = 0 up to rounding: below 64 eps m, status 5
    info, _, notes = ref.factor(H3, True)
    assert info == 6 and not notes["mod"] and notes["margin"] < ref.PIVOT_REL
    H4 = H.copy()
    H4[2, 2] = -1.0                                                      # a pivot before the last: never modified
    assert ref.factor(H4, True)[0] == 3 and not ref.factor(H4, True)[2]["mod"]


@pytest.mark.parametrize("name", sorted(ref.SETS))
def test_plain_newton_stops_at_an_indefinite_hessian_and_the_rule_converges_every_problem(name):
    """the named set (64 problems, kap = 1, x0 = 0, the defaults): rule off = the status-5 rule of every other Laplace kernel; rule
    on: every problem converges, the final Hessian is positive definite, within the recorded iteration and evaluation maxima"""
    N, P, size = ref.SETS[name]
    plain, ruled = ref.set_runs(name, False), ref.set_runs(name, True)
    n5 = sum(s["status"] == 5 for s in plain)
    nit, nfev = max(s["nit"] for s in ruled), max(s["nfev"] for s in ruled)
    print(f"{name} (N, P, size) = {(N, P, size)}: plain Newton status 5 in {n5} of {ref.SET_K}; with the rule nit <= {nit}, nfev <= "
          f"{nfev}, problems with a modified pivot {sum(s['nmod'] > 0 for s in ruled)}")
    assert all(s["status"] in (1, 5) for s in plain)
    if name != "r0.3":                                                   # (strong overdispersion: H(0) is positive definite)
        assert n5 >= ref.SET_PLAIN_STATUS5_MIN
    assert all(s["status"] == 1 for s in ruled) and nit <= ref.SET_MAX_NIT and nfev <= ref.SET_MAX_NFEV
    assert sum(s["nmod"] > 0 for s in ruled) == n5                       # exactly the problems plain Newton gave up
    inp = ref.make_problems(N, P, size)
    for k, s in enumerate(ruled):
        H = ref.evaluate(ref.problem(*inp, k), s["x"])[2]
        assert ref.factor(H)[0] == 0 and np.linalg.eigvalsh(H).min() > 0, (name, k)
        if plain[k]["status"] == 1:                                      # the rule never fired: the same run, bit for bit
            assert np.array_equal(s["x"], plain[k]["x"]) and s["nfev"] == plain[k]["nfev"]


def test_recorded_maxima_are_attained():
    nit = max(s["nit"] for n in ref.SETS for s in ref.set_runs(n, True))
    nfev = max(s["nfev"] for n in ref.SETS for s in ref.set_runs(n, True))
    assert (nit, nfev) == (ref.SET_MAX_NIT, ref.SET_MAX_NFEV)


@pytest.mark.parametrize("shape", ref.STEP_SHAPES)
@pytest.mark.parametrize("with_offset", [True, False])
def test_margins_of_every_replayed_trajectory(shape, with_offset):
    """what the GPU step test relies on: every run converges, no decision on its threshold, every last-pivot decision with |s| >=
    1e-6 m; the set from x0 = 0 has rounds with a modified pivot, the set started near the mode has none"""
    far, near = ref.trajectories(shape, False, with_offset), ref.trajectories(shape, True, with_offset)
    ok, low, piv, mar, nmod = ref.margins_hold(far)
    assert ok and nmod > 0 and mar >= ref.MOD_MARGIN, (ok, low, piv, mar, nmod)
    assert sum(st["nmod"] for _, st, _, _ in far) == nmod
    ok2, low2, piv2, mar2, nmod2 = ref.margins_hold(near)
    assert ok2 and nmod2 == 0 and mar2 == np.inf, (ok2, low2, piv2)
    assert any(a["nls"] > 0 for _, _, rec, _ in far for _, a, _ in rec) or shape[1] > 0      # rejected trials are replayed too
    print(f"{shape} offset={with_offset}: from 0: Armijo {low:.1e}, pivots {piv:.1e}, |s|/m {mar:.1e}, modified rounds {nmod}; near: "
          f"Armijo {low2:.1e}, pivots {piv2:.1e}")


def test_a_stopped_state_is_frozen_and_nmod_is_carried():
    traj = ref.trajectories((70, 9), False)
    p = ref.problem(*ref.step_inputs((70, 9)), 0)
    _, end, rec, _ = traj[0]
    again, notes = ref.step(p, end, False)
    assert notes == {} and all(np.array_equal(again[k], end[k]) for k in end)
    packed = ref.pack([a for _, a, _ in rec])
    assert packed["ist"][:, 4].tolist() == [a["nmod"] for _, a, _ in rec] and (np.diff(packed["ist"][:, 4]) >= 0).all()


# ---- 3. the host logic on the stand-in engine --------------------------------------------------------------------------------------
def _target(name="r2", K=6, rule=True, kap=1.0, **kw):
    import gsmvi_amd
    N, P, size = ref.SETS[name]
    A, y, o, _, lam, tm, tk = ref.make_problems(N, P, size, K=ref.SET_K, kap=kap)
    eng = ref.StandInEngine(rule)
    tgt = gsmvi_amd.BatchedNegBinomialTarget(A[:K], y[:K], prior_precision=lam, offset=o[:K], log_size_mean=tm, log_size_precision=tk,
                                             engine=eng, **kw)
    return tgt, eng


def test_laplace_init_negbin_batched_on_the_stand_in_engine():
    import gsmvi_amd
    K = 6
    tgt, eng = _target(K=K)
    runs = {c: gsmvi_amd.laplace_init_negbin_batched(tgt, check_every=c) for c in (1, 4, 1000)}
    mean, cov, res = runs[4]
    D = tgt.D
    assert isinstance(res, gsmvi_amd.LaplaceBatchedResult) and isinstance(res, gsmvi_amd.LaplaceNegBinBatchedResult)
    assert mean.shape == (K, D) and cov.shape == (K, D, D) and res.nmod.shape == (K,)
    assert res.success.all() and (res.status == 1).all() and (res.info == 0).all() and res.nlaunch % 4 == 0
    assert runs[1][2].nlaunch == runs[1][2].nfev.max() and runs[1000][2].nlaunch == 200
    for c in (1, 1000):                                                 # the result does not depend on check_every
        assert np.array_equal(runs[c][0], mean) and np.array_equal(runs[c][1], cov)
        for f in ("x", "fun", "jac", "nit", "nfev", "status", "info", "nmod"):
            assert np.array_equal(getattr(runs[c][2], f), getattr(res, f)), (c, f)
    want = ref.set_runs("r2", True)[:K]
    assert res.nmod.tolist() == [s["nmod"] for s in want] and res.nit.tolist() == [s["nit"] for s in want]
    assert res.nfev.tolist() == [s["nfev"] for s in want] and all(np.array_equal(mean[k], want[k]["x"]) for k in range(K))
    H = gsmvi_amd.neg_hessian_negbin_batched(tgt, mean)
    assert H.shape == (K, D, D) and np.allclose(np.einsum("kij,kjl->kil", cov, H), np.eye(D), atol=1e-9)
    assert ("negbin_laplace_step", True) in eng.calls and ("negbin_hessian", "cov") in eng.calls and ("negbin_hessian", "h") in eng.calls
    assert np.array_equal(gsmvi_amd.neg_hessian_negbin_batched(tgt, torch.tensor(mean)), H)
    # the three forms of x0
    x1 = np.concatenate([np.zeros(D - 1), [1.0]])
    a = gsmvi_amd.laplace_init_negbin_batched(tgt, x0=x1)
    b = gsmvi_amd.laplace_init_negbin_batched(tgt, x0=np.tile(x1, (K, 1)))
    c = gsmvi_amd.laplace_init_negbin_batched(tgt, x0=torch.tensor(x1))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0]) and np.allclose(a[0], mean, atol=1e-6)


def test_with_the_rule_off_the_stand_in_engine_reports_status_5():
    """the same call on an engine without the rule: the problems whose Hessian at x0 = 0 is indefinite end at their first round
    with status 5, their x0 and the identity; with the rule they succeed"""
    import gsmvi_amd
    K = 24
    off, on = _target(K=K, rule=False)[0], _target(K=K)[0]
    m0, c0, r0 = gsmvi_amd.laplace_init_negbin_batched(off)
    m1, c1, r1 = gsmvi_amd.laplace_init_negbin_batched(on)
    lost = np.flatnonzero(r0.status == 5)
    assert lost.size >= 1 and set(r0.status.tolist()) == {1, 5} and (r0.nmod == 0).all()
    assert (r0.nit[lost] == 0).all() and not m0[lost].any() and not r0.success[lost].any()
    assert all(np.array_equal(c0[k], np.eye(on.D)) for k in lost)
    assert r1.success.all() and (r1.nmod[lost] > 0).all() and (np.delete(r1.nmod, lost) == 0).all()


def test_failures_return_the_last_point_and_the_identity():
    import gsmvi_amd
    tgt, eng = _target(K=5)
    D = tgt.D
    mean, cov, res = gsmvi_amd.laplace_init_negbin_batched(tgt, maxiter=1)          # one iteration: status 2 everywhere
    assert (res.status == 2).all() and not res.success.any() and (res.nit == 1).all()
    assert np.array_equal(cov, np.broadcast_to(np.eye(D), (5, D, D))) and np.isfinite(mean).all() and mean.any()
    x0 = np.zeros((5, D))
    x0[2, D - 1] = 800.0                                                 # e^theta overflows: status 4, info 1, cov = I
    x0[3, 0] = np.nan
    mean, cov, res = gsmvi_amd.laplace_init_negbin_batched(tgt, x0=x0)
    assert res.status.tolist() == [1, 1, 4, 4, 1] and res.info.tolist() == [0, 0, 1, 1, 0]
    assert np.array_equal(cov[2], np.eye(D)) and mean[2, D - 1] == 800.0 and not np.array_equal(cov[1], np.eye(D))
    # all counts zero with a flat prior on theta: f = g = 0 at once, H = diag(lam, 0): a stationary point that is no mode
    N, P, size = ref.SETS["p1"]
    A, y, o, _, lam, tm, tk = ref.make_problems(N, P, size, K=3)
    t2 = gsmvi_amd.BatchedNegBinomialTarget(A, y, prior_precision=lam, offset=o, counts=np.array([0, N, N]),
                                            log_size_precision=np.array([0.0, 1.0, 1.0]), engine=ref.StandInEngine())
    mean, cov, res = gsmvi_amd.laplace_init_negbin_batched(t2)
    assert res.status.tolist() == [5, 1, 1] and res.info[0] == 2 and res.success.tolist() == [0, 1, 1]
    assert res.nit[0] == 0 and res.nfev[0] == 1 and np.array_equal(cov[0], np.eye(2)) and not mean[0].any()


def test_argument_and_type_errors_need_no_gpu():
    import gsmvi_amd
    import glm_batched_ref as gref
    import laplace_batched_ref as lref
    tgt, eng = _target(K=5)
    D = tgt.D
    n = len(eng.calls)
    A, y, o, counts, lam, tau, _ = gref.make_inputs("poisson", 3, 12, 4, 1)
    other = gsmvi_amd.BatchedGLMTarget(A, y, "poisson", counts=counts, engine=lref.StandInEngine())
    for bad, name in ((lambda x: x, "function"), (np.zeros((5, 3)), "ndarray"), (other, "BatchedGLMTarget")):
        with pytest.raises(TypeError, match=f"laplace_init_negbin_batched: target must be a BatchedNegBinomialTarget, got {name}"):
            gsmvi_amd.laplace_init_negbin_batched(bad)
        with pytest.raises(TypeError, match=f"neg_hessian_negbin_batched: target must be a BatchedNegBinomialTarget, got {name}"):
            gsmvi_amd.neg_hessian_negbin_batched(bad, np.zeros((5, 3)))
    for x0 in (np.zeros(D - 1), np.zeros((4, D)), np.zeros((5, D, 1)), 0.0):
        with pytest.raises(ValueError, match=r"laplace_init_negbin_batched: x0 must be None, \(D,\)"):
            gsmvi_amd.laplace_init_negbin_batched(tgt, x0=x0)
    for kw in (dict(maxiter=0), dict(maxfun=1), dict(check_every=0)):
        with pytest.raises(ValueError, match="laplace_init_negbin_batched: maxiter and check_every must be at least 1, maxfun at least 2"):
            gsmvi_amd.laplace_init_negbin_batched(tgt, **kw)
    for badtol in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="laplace_init_negbin_batched: gtol must be >= 0"):
            gsmvi_amd.laplace_init_negbin_batched(tgt, gtol=badtol)
    for x in (np.zeros(D), np.zeros((4, D)), np.zeros((5, 1, D))):
        with pytest.raises(ValueError, match=r"neg_hessian_negbin_batched: x must be \(K, D\)"):
            gsmvi_amd.neg_hessian_negbin_batched(tgt, x)
    assert len(eng.calls) == n                                          # nothing reached the engine
    # the other initialisers keep refusing this target, in their own words
    with pytest.raises(TypeError) as e:
        gsmvi_amd.laplace_init_batched(tgt)
    assert str(e.value) == ("laplace_init_batched: target must be a BatchedGLMTarget or a BatchedLogisticTarget, got "
                            "BatchedNegBinomialTarget")
    with pytest.raises(TypeError, match="laplace_init_shared_batched"):
        gsmvi_amd.laplace_init_shared_batched(tgt)
    assert not hasattr(tgt, "neg_hessian")
    assert "neg_hessian_negbin_batched" in type(tgt).__doc__ and "laplace_init_negbin_batched" in type(tgt).__doc__


# ---- 4. the C ABI ------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    head = hdr.split("#ifndef GSMVI_HIP_H")[0]
    for name in ref.NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr)
        for mp in ("exports.map", "exports_debug.map"):
            assert re.search(r"^\s*" + name + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), (mp, name)
        assert name in _lib.exported_symbols() and name in built and name in head
        res, args = _lib._SIGS[name]
        decl = re.search(r"int\s+" + name + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert res is C.c_int and len(args) == len(params) == (19 if "hessian" in name else 26)
        # the model's arguments are gsmvi_negbin_batched_f64's, in its order (without nc)
        score = re.search(r"int\s+gsmvi_negbin_batched_f64\s*\(([^;]*)\);", hdr, re.S).group(1)
        sp = [" ".join(p.split()) for p in score.split(",")]
        assert params[:4] == sp[:4] and params[4:15] == sp[5:16]
        for p, a in zip(params, args):
            want = C.c_double if p.startswith("double ") else C.c_int64 if p.startswith("int64_t") else \
                C.c_int if p.startswith("int ") else C.c_void_p
            assert a is want, (name, p, a)
    block = hdr[:hdr.index("int " + ref.NAMES[0])].rsplit("/*", 1)[1]
    for word in ("initializers.py:5-17", "example_gsm.py:34-35", "GSMVI_PATH_BATCHED_LAPLACE |", "GSMVI_PATH_BATCHED_TARGET",
                 "64 eps", "1e-10 max(1, |f|)", "last-pivot rule", "ist[4]", "NOT positive semi-definite"):
        assert word in block, word
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_LAPLACE\s+0x80000u", hdr)
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_TARGET\s+0x20000u", hdr)
    for define in ("GSMVI_PATH_BATCHED_LAPLACE", "GSMVI_PATH_BATCHED_TARGET"):
        assert "k_negbin_laplace_batched" in re.search(r"#define\s+" + define + r"\s.*", hdr).group(0), define
    assert len(re.findall(r"#define\s+GSMVI_PATH_\w+\s+0x", hdr)) == 32 and _lib.load_library().gsmvi_abi_version() == 1   # no new bit
    mk = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "Makefile")).read()
    assert "gsmvi_negbin_laplace_batched.hip" in mk
    src = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_negbin_laplace_batched.hip")).read()
    assert '#include "gsmvi_laplace_stage.h"' in src and "lp_chol_lds(bool" not in src      # no third copy of the stage
    assert '#include "gsmvi_negbin_link.h"' in src and "lgamma(" not in src and "digamma" not in src


def test_entry_points_reject_bad_arguments_without_a_gpu():
    ref.check_bad_arguments(_lib.load_library())


def test_lds_of_every_d_fits_without_a_kernel_attribute():
    """gsmvi_debug_negbin_laplace_lds for every D = 2 .. 64: at most 65536 bytes (the limit without a kernel attribute), four
    problems per workgroup up to D = 16 and one above, and the bytes of csrc/gsmvi_negbin_laplace_batched.hip's formula"""
    path = os.path.join(os.path.dirname(_lib.library_path()), "libgsmvi_hip_debug.so")
    lib = C.CDLL(path)
    fn = lib.gsmvi_debug_negbin_laplace_lds
    fn.restype, fn.argtypes = _lib._DEBUG_SIGS["gsmvi_debug_negbin_laplace_lds"]
    worst = 0
    for D in range(2, 65):
        b, ppw = C.c_size_t(), C.c_int()
        assert fn(D, C.byref(b), C.byref(ppw)) == 0
        Dp = 16 * ((D + 15) // 16)
        assert ppw.value == (4 if D <= 16 else 1)
        assert b.value == 8 * ppw.value * (32 * (Dp + 1) + 8 * 32 + 5 * Dp + 4 + D * (D | 1)) <= 65536
        worst = max(worst, b.value)
    assert worst == 8 * 6820
    assert fn(1, C.byref(b), C.byref(ppw)) == 1 and fn(65, C.byref(b), C.byref(ppw)) == 1


def test_the_public_names_are_exported():
    import gsmvi_amd
    assert callable(gsmvi_amd.laplace_init_negbin_batched) and callable(gsmvi_amd.neg_hessian_negbin_batched)
    from gsmvi_amd.engine import HipEngine
    assert callable(HipEngine.negbin_hessian_batched) and callable(HipEngine.negbin_laplace_step_batched)
