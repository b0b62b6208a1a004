"""The ordinal Laplace initialiser without a GPU: the restatements of tests/ordinal_laplace_ref.py against the mpmath truth of the
link curvature (tests/ordinal_curv_truth.py), against central differences of the score restatement and against each other; the
retry rule on the named test sets; the margins of the trajectories the GPU test replays; the host logic of
``laplace_init_ordinal_batched`` and ``neg_hessian_ordinal_batched`` on the stand-in engine; the C ABI's declarations and argument
checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ordinal_batched_ref as oref
import ordinal_curv_truth as ct
import ordinal_laplace_ref as ref
from gsmvi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the link curvature ---------------------------------------------------------------------------------------------------------
def test_the_committed_truth_table_is_the_grid_and_mpmath_reproduces_it():
    """the table covers ordinal_link_truth.grid(); a spread of its points recomputed with mpmath (60 and 120 digits agreeing) gives
    the committed values and scales"""
    pytest.importorskip("mpmath")
    tab = ct.load_table()
    eta, d0, d1, y = ct.grid()
    assert all(tab[q].shape == (2, len(eta)) and tab["scale_" + q].shape == (len(eta),) for q in ct.QUANTITIES)
    for i in range(5, len(eta), 199):
        v = ct.values(eta[i], d0[i], d1[i], int(y[i]))
        for q in ct.QUANTITIES:
            assert ct.split(v[q]) == (tab[q][0, i], tab[q][1, i]), (q, i)
            m, e = ct.pack_scale(v["scale_" + q])
            assert m == tab["scale_" + q][i] and e == tab["scexp_" + q][i], (q, i)


def _restated_grid(L):
    A, y, o, X = ct.problems()
    H = ref.neg_hessian(A, y, o, None, 0.0, 0.0, 3, X, L=L)[0]
    return ct.entries(H)


def test_float64_restatement_of_the_curvature_is_within_c_cpu_of_the_truth():
    """the worst ratio over the whole grid per quantity is C_CPU (recorded in ordinal_curv_truth); the GPU bound max(16, 4 C_CPU)
    follows from it and not from any device figure; the long double restatement, the GPU tests' reference, is well inside one; a
    point whose truth overflows float64 is held to the same infinity"""
    tab = ct.load_table()
    got, ld = _restated_grid(np.float64), _restated_grid(np.longdouble)
    for q in ct.QUANTITIES:
        worst, worst_ld = ct.ratio(got[q], tab, q).max(), ct.ratio(ld[q], tab, q).max()
        print(f"{q}: float64 restatement {worst:.3f} (C_CPU {ct.C_CPU[q]}), long double {worst_ld:.3f}, GPU bound {ct.c_gpu(q)}")
        assert worst <= ct.C_CPU[q] and worst > 0.5 * ct.C_CPU[q], (q, worst)
        assert worst_ld <= 0.6 and ct.c_gpu(q) == max(16.0, 4.0 * ct.C_CPU[q])
        inf = np.isinf(tab[q][0])
        assert np.array_equal(got[q][inf], tab[q][0][inf])
    # the symmetry that the forms give: he0 = -hee = -h00 whatever the label, and h01 = -he1
    assert np.array_equal(got["he0"], -got["hee"]) and np.array_equal(got["h00"], got["hee"]) and np.array_equal(got["h01"], -got["he1"])


def test_link_outputs_shared_with_the_score_restatement_are_its_bits():
    """r_eta and t of ``curv`` are ordinal_batched_ref.link's, bit for bit; sigma(-b) is its u_hi without the gap term"""
    rs = np.random.RandomState(2)
    C, n = 6, 200
    delta = np.concatenate([[0.3], rs.uniform(-2, 1.5, C - 2)])
    cut, w = oref.cutpoints(delta[None, :])
    lm, qe = oref.gap(w)
    eta, y = 3 * rs.standard_normal(n), rs.randint(0, C, n)
    re, ulo, uhi, t = oref.link(eta[None, :], y, cut, lm, qe)
    lm0 = lm[0].copy()
    lm0[0] = 0.0
    r2, sb, fab, fb, t2, _, _ = ref.curv(eta, y, cut[0], lm0)
    assert np.array_equal(re[0], r2) and np.array_equal(t[0], t2)
    inner = (y >= 1) & (y <= C - 2)
    assert np.array_equal(uhi[0][~inner], sb[~inner]) and (fab >= fb).all() and (fb >= 0).all()


@pytest.mark.parametrize("N,P,C", [(40, 3, 2), (40, 3, 3), (60, 2, 5), (70, 9, 8)])
def test_restated_h_is_the_central_difference_of_the_restated_score(N, P, C):
    """H of ``evaluate`` against central differences of ordinal_batched_ref.score_and_lp_ld (the existing score restatement), with
    offset, counts and per-problem priors (lam = kap = 0 for problem 0); f and g against the same restatement"""
    K = 4
    A, y, o, counts, lam, kap, X = oref.make_inputs(K, N, P, C, 1)
    X = X[:, 0, :] * 0.5
    H, sH = ref.neg_hessian(A, y, o, counts, lam, kap, C, X, L=np.longdouble)
    h = 1e-5
    D = P + C - 1
    for k in range(K):
        for j in range(D):
            xp, xm = X.copy(), X.copy()
            xp[k, j] += h
            xm[k, j] -= h
            gp = oref.score_and_lp_ld(A, y, o, counts, lam, kap, xp[:, None, :], C)[0][k, 0]
            gm = oref.score_and_lp_ld(A, y, o, counts, lam, kap, xm[:, None, :], C)[0][k, 0]
            fd = -np.asarray((gp - gm) / (2 * h), dtype=np.float64)
            assert np.allclose(fd, H[k, :, j], rtol=0, atol=2e-8 * max(1.0, sH[k].max())), (k, j, np.abs(fd - H[k, :, j]).max())
        assert np.array_equal(H[k], H[k].T)
        f, g, _, sc = ref.evaluate(ref.problem(A, y, o, counts, lam, kap, C, k), X[k])
        G, lp = oref.score_and_lp_ld(A, y, o, counts, lam, kap, X[:, None, :], C)
        assert abs(f + float(lp[k, 0])) <= 1e-13 * max(sc["f"], 1e-300) and (np.abs(g + G[k, 0].astype(np.float64)) <= 1e-13 * sc["g"] + 1e-300).all()
    # float64 and long double restatements agree to 1e-13 of the scale
    H64 = ref.neg_hessian(A, y, o, counts, lam, kap, C, X)[0]
    assert (np.abs(H64 - H) <= 1e-13 * sH).all()
    # problem 1 has counts = 0: its Hessian is its prior
    assert np.array_equal(H[1], np.diag([lam[1]] * P + [kap[1]] * (C - 1)))


def test_two_classes_are_logistic_regression_on_the_design_with_a_minus_one_column():
    rs = np.random.RandomState(4)
    N, P = 30, 4
    A, y, x = rs.standard_normal((1, N, P)), rs.randint(0, 2, (1, N)), rs.standard_normal(P + 1)
    H = ref.neg_hessian(A, y, None, None, 0.7, 0.7, 2, x[None, :])[0][0]
    A2 = np.concatenate([A[0], -np.ones((N, 1))], axis=1)
    s = 1.0 / (1.0 + np.exp(-(A2 @ x)))
    assert np.allclose(H, (A2 * (s * (1 - s))[:, None]).T @ A2 + 0.7 * np.eye(P + 1), rtol=0, atol=1e-13)


def test_flag_rules_of_the_restatement():
    A, y, o, counts, lam, kap, X = oref.make_inputs(4, 12, 2, 4, 1, poison=False)
    X = X[:, 0, :].copy()
    X[0, 3], X[1, 0], X[3, 2] = 800.0, np.inf, 1e6                      # a gap overflows; a non-finite beta; delta_0 is a location
    H = ref.neg_hessian(A, y, o, None, 1.0, 1.0, 4, X)[0]
    assert np.isnan(H[0]).all() and np.isnan(H[1]).all() and np.isfinite(H[2]).all() and np.isfinite(H[3]).all()
    X[2, 4] = -740.0                                                     # a subnormal gap
    assert np.isnan(ref.neg_hessian(A, y, o, None, 1.0, 1.0, 4, X)[0][2]).all()
    cov, info = ref.inverse(H[0])
    assert np.array_equal(cov, np.eye(5)) and info == 1


# ---- 2. the retry rule -------------------------------------------------------------------------------------------------------------
def test_factor_is_a_cholesky_factorisation_and_the_rule_retries_once_without_the_negative_chain_terms():
    rs = np.random.RandomState(5)
    M = rs.standard_normal((6, 6))
    H = M @ M.T + 0.1 * np.eye(6)
    c = np.array([0.0, -3.0, 0.5])                                       # P = 3, C = 4
    info, R, notes = ref.factor(H, c, True)
    assert info == 0 and not notes["mod"] and np.allclose(R.T @ R, H, atol=1e-13) and np.allclose(R, np.linalg.cholesky(H).T)
    H2 = H.copy()
    H2[4, 4] += c[1] - 100.0                                             # the chain term and more: indefinite
    assert ref.factor(H2)[0] == 5 and ref.factor(H2, c, False)[0] == 5
    info, R2, notes = ref.factor(H2, c, True)                            # the retry takes only min(c, 0) off: still indefinite
    assert info == 5 and not notes["mod"]
    H3 = H.copy()
    H3[4, 4] += 0.9 * c[1]
    H3[3, 3] = -1.0                                                      # a failure elsewhere (c_0 = 0 is never taken off)
    assert ref.factor(H3, c, True)[0] == 4
    H4 = H.copy()
    H4[4, 4] += c[1]
    if ref.factor(H4)[0] != 0:
        info, R4, notes = ref.factor(H4, c, True)
        assert info == 0 and notes["mod"] and np.allclose(R4.T @ R4, H, atol=1e-12)
    assert np.array_equal(ref.retried(H4, c), H4 - np.diag([0, 0, 0, 0, c[1], 0]))
    assert ref.factor(H2, np.array([0.0, 1.0, 2.0]), True)[0] == 5       # no negative c_i: no retry


@pytest.mark.parametrize("N,P,C", [(40, 3, 3), (60, 2, 5), (70, 9, 8), (120, 3, 30)])
def test_the_retried_matrix_is_positive_semi_definite_without_priors(N, P, C):
    """H - diag(min(c, 0)) with lam = kap = 0 is J^T (PSD) J + diag(max(c, 0)): its smallest eigenvalue is >= 0 up to rounding, at
    x0 = 0 and at random points"""
    K = 6
    A, y, o, _, _, _, X = oref.make_inputs(K, N, P, C, 1, poison=False)
    for X0 in (np.zeros((K, P + C - 1)), X[:, 0, :]):
        for k in range(K):
            _, _, H, sc = ref.evaluate(ref.problem(A, y, o, None, 0.0, 0.0, C, k), X0[k])
            ev = np.linalg.eigvalsh(ref.retried(H, sc["c"]))
            assert ev.min() >= -1e-12 * max(1.0, ev.max()), (k, ev.min())


@pytest.mark.parametrize("name", ["c8", "c30"])
def test_where_plain_newton_gave_up_h_is_indefinite_and_the_retried_matrix_is_not(name):
    """the points at which the plain runs of the named set ended with status 5: H (lam = kap = 1) fails its factorisation and has
    a negative eigenvalue; the retried matrix factors, and without the priors its smallest eigenvalue is >= 0 up to rounding"""
    N, P, C = ref.SETS[name]
    inp = ref.make_problems(N, P, C)
    flat = ref.make_problems(N, P, C, lam=0.0, kap=0.0)
    n = 0
    for k, s in enumerate(ref.set_runs(name, False)):
        if s["status"] != 5:
            continue
        n += 1
        _, _, H, sc = ref.evaluate(ref.problem(*inp, k), s["x"])
        assert ref.factor(H)[0] != 0 and np.linalg.eigvalsh(H).min() < 0 and (sc["c"] < 0).any()
        info, _, notes = ref.factor(H, sc["c"], True)
        assert info == 0 and notes["mod"]
        _, _, H0, sc0 = ref.evaluate(ref.problem(*flat, k), s["x"])
        ev = np.linalg.eigvalsh(ref.retried(H0, sc0["c"]))
        assert ev.min() >= -1e-12 * max(1.0, ev.max()), (k, ev.min())
    assert n >= ref.SET_PLAIN_STATUS5_MIN[name]


@pytest.mark.parametrize("name", sorted(ref.SETS))
def test_plain_newton_stops_at_an_indefinite_hessian_and_the_rule_converges_every_problem(name):
    """the named set (16 problems, lam = kap = 1, x0 = 0, the defaults): rule off = the status-5 rule of every other Laplace kernel;
    rule on: every problem converges and the final Hessian is positive definite"""
    N, P, C = ref.SETS[name]
    plain, ruled = ref.set_runs(name, False), ref.set_runs(name, True)
    n5 = sum(s["status"] == 5 for s in plain)
    nit, nfev = max(s["nit"] for s in ruled), max(s["nfev"] for s in ruled)
    print(f"{name} (N, P, C) = {(N, P, C)}: plain Newton status 5 in {n5} of {ref.SET_K}; with the rule all converge, nit <= {nit}, "
          f"nfev <= {nfev}, problems with a retried round {sum(s['nmod'] > 0 for s in ruled)}")
    assert all(s["status"] in (1, 5) for s in plain) and n5 >= ref.SET_PLAIN_STATUS5_MIN[name]
    assert all(s["status"] == 1 for s in ruled)
    assert sum(s["nmod"] > 0 for s in ruled) == n5                       # exactly the problems plain Newton gave up
    inp = ref.make_problems(N, P, C)
    for k, s in enumerate(ruled):
        H = ref.evaluate(ref.problem(*inp, k), s["x"])[2]
        assert ref.factor(H)[0] == 0 and np.linalg.eigvalsh(H).min() > 0, (name, k)
        if plain[k]["status"] == 1:                                      # the rule never fired: the same run, bit for bit
            assert np.array_equal(s["x"], plain[k]["x"]) and s["nfev"] == plain[k]["nfev"]


@pytest.mark.parametrize("shape", ref.STEP_SHAPES)
@pytest.mark.parametrize("with_offset", [True, False])
def test_margins_of_every_replayed_trajectory(shape, with_offset):
    """what the GPU step test relies on: every run converges, no decision on its threshold, every pivot test of every factorisation
    with |pivot| >= 1e-6 m; the sets from x0 = 0 at C >= 8 have retried rounds, the sets started near the mode have none"""
    far, near = ref.trajectories(shape, False, with_offset), ref.trajectories(shape, True, with_offset)
    ok, low, mar, nmod = ref.margins_hold(far)
    assert ok and mar >= ref.MOD_MARGIN, (ok, low, mar, nmod)
    assert nmod > 0 or shape not in ref.RETRY_SHAPES
    assert sum(st["nmod"] for _, st, _, _ in far) == nmod
    ok2, low2, mar2, nmod2 = ref.margins_hold(near)
    assert ok2 and nmod2 == 0 and mar2 >= ref.MOD_MARGIN, (ok2, low2, mar2)
    print(f"{shape} offset={with_offset}: from 0: Armijo {low:.1e}, |pivot|/m {mar:.1e}, retried rounds {nmod}; near: Armijo {low2:.1e}, "
          f"|pivot|/m {mar2:.1e}")


def test_a_stopped_state_is_frozen_and_nmod_is_carried():
    traj = ref.trajectories((70, 9, 8), False)
    p = ref.problem(*ref.step_inputs((70, 9, 8)), 0)
    _, end, rec, _ = traj[0]
    again, notes = ref.step(p, end, False)
    assert notes == {} and all(np.array_equal(again[k], end[k]) for k in end)
    packed = ref.pack([a for _, a, _ in rec])
    assert packed["ist"][:, 4].tolist() == [a["nmod"] for _, a, _ in rec] and (np.diff(packed["ist"][:, 4]) >= 0).all()


# ---- 3. the host logic on the stand-in engine --------------------------------------------------------------------------------------
def _target(name="c8", K=6, rule=True, **kw):
    import gsmvi_amd
    N, P, C = ref.SETS[name]
    A, y, o, _, lam, kap, _ = ref.make_problems(N, P, C)
    eng = ref.StandInEngine(rule)
    tgt = gsmvi_amd.BatchedOrdinalTarget(A[:K], y[:K], C, prior_precision=lam, cut_precision=kap, offset=o[:K], engine=eng, **kw)
    return tgt, eng


def test_laplace_init_ordinal_batched_on_the_stand_in_engine():
    import gsmvi_amd
    K = 6
    tgt, eng = _target(K=K)
    runs = {c: gsmvi_amd.laplace_init_ordinal_batched(tgt, check_every=c) for c in (1, 4, 1000)}
    mean, cov, res = runs[4]
    D = tgt.D
    assert isinstance(res, gsmvi_amd.LaplaceBatchedResult) and isinstance(res, gsmvi_amd.LaplaceOrdinalBatchedResult)
    assert mean.shape == (K, D) and cov.shape == (K, D, D) and res.nmod.shape == (K,)
    assert res.success.all() and (res.status == 1).all() and (res.info == 0).all() and res.nlaunch % 4 == 0
    assert runs[1][2].nlaunch == runs[1][2].nfev.max() and runs[1000][2].nlaunch == 200
    for c in (1, 1000):                                                 # the result does not depend on check_every
        assert np.array_equal(runs[c][0], mean) and np.array_equal(runs[c][1], cov)
        for f in ("x", "fun", "jac", "nit", "nfev", "status", "info", "nmod"):
            assert np.array_equal(getattr(runs[c][2], f), getattr(res, f)), (c, f)
    want = ref.set_runs("c8", True)[:K]
    assert res.nmod.tolist() == [s["nmod"] for s in want] and res.nit.tolist() == [s["nit"] for s in want] and res.nmod.max() > 0
    assert res.nfev.tolist() == [s["nfev"] for s in want] and all(np.array_equal(mean[k], want[k]["x"]) for k in range(K))
    H = gsmvi_amd.neg_hessian_ordinal_batched(tgt, mean)
    assert H.shape == (K, D, D) and np.allclose(np.einsum("kij,kjl->kil", cov, H), np.eye(D), atol=1e-9)
    assert ("ordinal_laplace_step", True) in eng.calls and ("ordinal_hessian", "cov") in eng.calls and ("ordinal_hessian", "h") in eng.calls
    assert np.array_equal(gsmvi_amd.neg_hessian_ordinal_batched(tgt, torch.tensor(mean)), H)
    # the three forms of x0
    x1 = np.concatenate([np.zeros(D - 1), [0.2]])
    a = gsmvi_amd.laplace_init_ordinal_batched(tgt, x0=x1)
    b = gsmvi_amd.laplace_init_ordinal_batched(tgt, x0=np.tile(x1, (K, 1)))
    c = gsmvi_amd.laplace_init_ordinal_batched(tgt, x0=torch.tensor(x1))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0]) and np.allclose(a[0], mean, atol=1e-6)


def test_with_the_rule_off_the_stand_in_engine_reports_status_5():
    """the same call on an engine without the rule: the problems whose Hessian on the way is indefinite end with status 5, their
    last point and the identity; with the rule they succeed"""
    import gsmvi_amd
    K = 16
    off, on = _target(K=K, rule=False)[0], _target(K=K)[0]
    m0, c0, r0 = gsmvi_amd.laplace_init_ordinal_batched(off)
    m1, c1, r1 = gsmvi_amd.laplace_init_ordinal_batched(on)
    lost = np.flatnonzero(r0.status == 5)
    assert lost.size >= 1 and set(r0.status.tolist()) == {1, 5} and (r0.nmod == 0).all()
    assert not r0.success[lost].any() and all(np.array_equal(c0[k], np.eye(on.D)) for k in lost)
    assert r1.success.all() and (r1.nmod[lost] > 0).all() and (np.delete(r1.nmod, lost) == 0).all()


def test_failures_return_the_last_point_and_the_identity():
    import gsmvi_amd
    tgt, eng = _target(K=5)
    D, P = tgt.D, tgt.P
    mean, cov, res = gsmvi_amd.laplace_init_ordinal_batched(tgt, maxiter=1)         # one iteration: status 2 everywhere
    assert (res.status == 2).all() and not res.success.any() and (res.nit == 1).all()
    assert np.array_equal(cov, np.broadcast_to(np.eye(D), (5, D, D))) and np.isfinite(mean).all() and mean.any()
    x0 = np.zeros((5, D))
    x0[2, D - 1] = 800.0                                                 # a gap overflows: status 4, info 1, cov = I
    x0[3, 0] = np.nan
    x0[4, P] = 1e6                                                       # delta_0 is a location: not flagged
    mean, cov, res = gsmvi_amd.laplace_init_ordinal_batched(tgt, x0=x0)
    assert res.status[:4].tolist() == [1, 1, 4, 4] and res.info[:4].tolist() == [0, 0, 1, 1] and res.status[4] != 4
    assert np.array_equal(cov[2], np.eye(D)) and mean[2, D - 1] == 800.0 and not np.array_equal(cov[1], np.eye(D))
    # all counts zero with a flat prior on delta: f = g = 0 at once, H = diag(lam, 0): a stationary point that is no mode
    N, P, C = ref.SETS["c3"]
    A, y, o, _, lam, kap, _ = ref.make_problems(N, P, C, K=3)
    t2 = gsmvi_amd.BatchedOrdinalTarget(A, y, C, prior_precision=lam, offset=o, counts=np.array([0, N, N]),
                                        cut_precision=np.array([0.0, 1.0, 1.0]), engine=ref.StandInEngine())
    mean, cov, res = gsmvi_amd.laplace_init_ordinal_batched(t2)
    assert res.status.tolist() == [5, 1, 1] and res.info[0] == 2 and res.success.tolist() == [0, 1, 1]
    assert res.nit[0] == 0 and res.nfev[0] == 1 and np.array_equal(cov[0], np.eye(3)) and not mean[0].any()


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
        with pytest.raises(TypeError, match=f"laplace_init_ordinal_batched: target must be a BatchedOrdinalTarget, got {name}"):
            gsmvi_amd.laplace_init_ordinal_batched(bad)
        with pytest.raises(TypeError, match=f"neg_hessian_ordinal_batched: target must be a BatchedOrdinalTarget, got {name}"):
            gsmvi_amd.neg_hessian_ordinal_batched(bad, np.zeros((5, 3)))
    for x0 in (np.zeros(D - 1), np.zeros((4, D)), np.zeros((5, D, 1)), 0.0):
        with pytest.raises(ValueError, match=r"laplace_init_ordinal_batched: x0 must be None, \(D,\)"):
            gsmvi_amd.laplace_init_ordinal_batched(tgt, x0=x0)
    for kw in (dict(maxiter=0), dict(maxfun=1), dict(check_every=0)):
        with pytest.raises(ValueError, match="laplace_init_ordinal_batched: maxiter and check_every must be at least 1, maxfun at least 2"):
            gsmvi_amd.laplace_init_ordinal_batched(tgt, **kw)
    for badtol in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="laplace_init_ordinal_batched: gtol must be >= 0"):
            gsmvi_amd.laplace_init_ordinal_batched(tgt, gtol=badtol)
    for x in (np.zeros(D), np.zeros((4, D)), np.zeros((5, 1, D))):
        with pytest.raises(ValueError, match=r"neg_hessian_ordinal_batched: x must be \(K, D\)"):
            gsmvi_amd.neg_hessian_ordinal_batched(tgt, x)
    assert len(eng.calls) == n                                          # nothing reached the engine
    # the other initialisers keep refusing this target, in their own words
    with pytest.raises(TypeError) as e:
        gsmvi_amd.laplace_init_batched(tgt)
    assert str(e.value) == ("laplace_init_batched: target must be a BatchedGLMTarget or a BatchedLogisticTarget, got "
                            "BatchedOrdinalTarget")
    for fn in (gsmvi_amd.laplace_init_softmax_batched, gsmvi_amd.laplace_init_shared_batched, gsmvi_amd.laplace_init_negbin_batched):
        with pytest.raises(TypeError, match=fn.__name__):
            fn(tgt)
    assert not hasattr(tgt, "neg_hessian")
    doc = " ".join(type(tgt).__doc__.split())
    assert "neg_hessian_ordinal_batched" in doc and "laplace_init_ordinal_batched" in doc
    assert "Only the posterior predictive is missing now" in doc


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
        assert res is C.c_int and len(args) == len(params) == (18 if "hessian" in name else 25)
        # the model's arguments are gsmvi_ordinal_batched_f64's, in its order (without nc)
        score = re.search(r"int\s+gsmvi_ordinal_batched_f64\s*\(([^;]*)\);", hdr, re.S).group(1)
        sp = [" ".join(p.split()) for p in score.split(",")]
        assert params[:5] == sp[:5] and params[5:14] == sp[6:15] and "const int* y" in params
        for p, a in zip(params, args):
            want = C.c_double if p.startswith("double ") else C.c_int64 if p.startswith("int64_t") else \
                C.c_int if p.startswith("int ") else C.c_void_p
            assert a is want, (name, p, a)
    block = hdr[:hdr.index("int " + ref.NAMES[0])].rsplit("/*", 1)[1]
    for word in ("initializers.py:5-17", "example_gsm.py:34-35", "GSMVI_PATH_BATCHED_LAPLACE |", "GSMVI_PATH_BATCHED_TARGET",
                 "64 eps", "1e-10 max(1, |f|)", "retry rule", "ist[4]", "min(c_i, 0)"):
        assert word in block, word
    for define in ("GSMVI_PATH_BATCHED_LAPLACE", "GSMVI_PATH_BATCHED_TARGET"):
        assert "k_ordinal_laplace_batched" in re.search(r"#define\s+" + define + r"\s.*", hdr).group(0), define
    assert len(re.findall(r"#define\s+GSMVI_PATH_\w+\s+0x", hdr)) == 32 and _lib.load_library().gsmvi_abi_version() == 1   # no new bit
    mk = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "Makefile")).read()
    assert "gsmvi_ordinal_laplace_batched.hip" in mk
    src = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_ordinal_laplace_batched.hip")).read()
    assert '#include "gsmvi_laplace_stage.h"' in src and "lp_chol_lds(bool" not in src      # no copy of the stage
    assert '#include "gsmvi_ordinal_link.h"' in src and "atomic" not in src.split("#include", 1)[1]


def test_entry_points_reject_bad_arguments_without_a_gpu():
    ref.check_bad_arguments(_lib.load_library())


def test_lds_of_every_d_fits_without_a_kernel_attribute():
    """gsmvi_debug_ordinal_laplace_lds for every D = 2 .. 64: at most 65536 bytes (the limit without a kernel attribute), four
    problems per workgroup up to D = 16 and one above, and the bytes of csrc/gsmvi_ordinal_laplace_batched.hip's formula"""
    path = os.path.join(os.path.dirname(_lib.library_path()), "libgsmvi_hip_debug.so")
    lib = C.CDLL(path)
    fn = lib.gsmvi_debug_ordinal_laplace_lds
    fn.restype, fn.argtypes = _lib._DEBUG_SIGS["gsmvi_debug_ordinal_laplace_lds"]
    worst = 0
    for D in range(2, 65):
        b, ppw = C.c_size_t(), C.c_int()
        assert fn(D, C.byref(b), C.byref(ppw)) == 0
        Dp = 16 * ((D + 15) // 16)
        assert ppw.value == (4 if D <= 16 else 1)
        assert b.value == 8 * ppw.value * (32 * (Dp + 1) + 7 * 32 + 11 * Dp + 4 + D * (D | 1)) <= 65536
        worst = max(worst, b.value)
    assert worst == 8 * 7172
    assert fn(1, C.byref(b), C.byref(ppw)) == 1 and fn(65, C.byref(b), C.byref(ppw)) == 1


def test_the_public_names_are_exported():
    import gsmvi_amd
    assert callable(gsmvi_amd.laplace_init_ordinal_batched) and callable(gsmvi_amd.neg_hessian_ordinal_batched)
    assert "laplace_init_ordinal_batched" in gsmvi_amd.__doc__ and "neg_hessian_ordinal_batched" in gsmvi_amd.__doc__
    from gsmvi_amd.engine import HipEngine
    assert callable(HipEngine.ordinal_hessian_batched) and callable(HipEngine.ordinal_laplace_step_batched)
