"""The batched Pathfinder initialiser without a GPU: the numpy restatement (tests/pathfinder_batched_ref.py) is pinned to scipy's
dense inverse-Hessian product and to the exactness of the pair base on isotropic targets, the host logic of
``pathfinder_init_batched`` runs on the stand-in engine, and the declarations, export lists, ctypes signatures and argument checks
of the two entry points are checked before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.optimize import LbfgsInvHessProduct

import lbfgs_batched_ref as lref
import logistic_batched_ref as logref
import pathfinder_batched_ref as ref
import softmax_batched_ref as sref
from conftest import ROOT

NAMES = ("gsmvi_pathfinder_propose_batched_f64", "gsmvi_pathfinder_select_batched_f64")


def _states():
    """packed L-BFGS states with 0, 1, 3, 10 pairs and wrapped ring buffers: every state of the D = 16 Gaussian run and the end
    states of the logistic runs (tests/test_lbfgs_batched_cpu.py pins ``hess_inv`` on the same runs)"""
    _, rec = lref.run(lref.gaussian_fun(16), np.ones(16), record=True)
    out = [st for _, _, _, st in rec]
    assert {(s["npairs"], s["head"]) for s in out} >= {(0, 0), (1, 1), (3, 3), (10, 0), (10, 5)}
    for N, D in lref.LOGISTIC_SHAPES:
        A, y, counts, lam, _ = logref.make_inputs(4, N, D, 1)
        out += [lref.run(lref.logistic_fun(A[k], y[k], counts[k], lam[k]), np.zeros(D)) for k in (1, 3)]
    return out


def test_sigma_on_the_identity_base_is_scipys_dense_product():
    worst = 0.0
    for st in _states():
        p = lref.pack([st])
        idx = lref.held(st)
        assert ref.held(p["ist"][0]) == idx
        for dtype in (np.float64, ref.LD):
            H = ref.sigma(p["S"][0], p["Y"][0], p["sc"][0], p["ist"][0], h0=1.0, dtype=dtype)
            assert np.array_equal(H, H.T)
            if not idx:
                assert np.array_equal(H, np.eye(st["x"].shape[0]))
                continue
            Hs = LbfgsInvHessProduct(st["S"][idx], st["Y"][idx]).todense()
            worst = max(worst, ref.rel_err(H, Hs))
    print(f"sigma(h0 = 1) against LbfgsInvHessProduct.todense(): worst relative {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("D", [2, 7, 16, 33])
def test_sigma_on_the_pair_base_is_positive_definite_on_a_quadratic(D):
    """pairs from an SPD quadratic have s.y > 0, so every H along the path is SPD and gamma is a Rayleigh quotient of the inverse
    Hessian: inside its spectrum"""
    fun = ref.quadratic(D)
    w = np.linalg.eigvalsh(fun.P)
    assert w[-1] / w[0] <= 100.0 * (1 + 1e-9)
    _, rec = lref.run(fun, np.ones(D), record=True, maxfun=40)
    seen = set()
    for _, _, _, st in rec:
        p = lref.pack([st])
        g = ref.base(p["sc"][0], p["ist"][0])
        if st["npairs"]:
            assert 1.0 / w[-1] * (1 - 1e-9) <= g <= 1.0 / w[0] * (1 + 1e-9)
        else:
            assert g == 1.0
        H = ref.sigma(p["S"][0], p["Y"][0], p["sc"][0], p["ist"][0], dtype=np.float64)
        assert np.array_equal(H, H.T) and np.linalg.eigvalsh(H).min() > 0.0
        seen.add(st["npairs"])
    assert {0, 1} <= seen


@pytest.mark.parametrize("D", [1, 5])
@pytest.mark.parametrize("var", [0.25, 1.0, 9.0])
def test_the_pair_base_is_exact_on_an_isotropic_target(var, D):
    """N(m, var I): the first pair has y = s / var, so gamma = var, Sigma = var I and mu = m exactly; lp - log q is then the same
    constant at every draw and the ELBO of path point 1 is lp(m) + D / 2 log(2 pi var) whatever the draws are.  Held to 1e-11
    relative to max(1, |value|), the single-update bar."""
    means, x0 = ref.isotropic(3, D, var)
    M = 5
    for k in range(3):
        m = means[k]
        fun = lambda x: (0.5 * float((x - m) @ (x - m)) / var, (x - m) / var)      # noqa: E731
        _, rec = lref.run(fun, x0[k], record=True)
        st = next(a for _, _, _, a in rec if a["nit"] == 1)
        assert st["npairs"] == 1 and rec[1][3]["nit"] == 1                        # the first trial is accepted
        state = lref.pack([st])
        Z = np.random.RandomState(7 + k).standard_normal((M, D))
        for dtype in (np.float64, ref.LD):
            p = ref.propose(state, [0], lambda k_, nit: Z, M, dtype=dtype)
            assert p["fresh"][0] == 1 and p["info"][0] == 0 and p["seen"][0] == 1
            assert ref.rel_gap(p["cov"][0], var * np.eye(D)) <= 1e-11 and ref.rel_gap(p["mu"][0], m) <= 1e-11
            X = np.asarray(p["X"][0], dtype=np.float64)
            lpsum = sum(-fun(x)[0] for x in X)
            best = ref.select([lpsum], [float(p["logq"][0])], p["fresh"], p["info"], [1], p["mu"], p["cov"],
                              ref.new_best(x0[k:k + 1]), M)
            want = ref.isotropic_elbo(D, var)
            assert abs(best["elbo_last"][0] - want) <= 1e-11 * max(1.0, abs(want)), (var, D, k, best["elbo_last"][0], want)
            assert best["best_it"][0] == 1 and best["npts"][0] == 1


def test_propose_leaves_a_problem_that_is_not_fresh_alone_and_flags_bad_inputs():
    states = [lref.run(ref.quadratic(5, seed=s), np.ones(5), maxfun=6) for s in range(4)]
    state = lref.pack(states)
    seen = state["ist"][:, 1].copy()
    seen[[0, 2, 3]] -= 1                                                      # problem 1 was proposed at this nit already
    state["g"][2, 3] = np.nan                                                 # a NaN gradient
    state["Y"][3, ref.held(state["ist"][3])[0], 1] = np.nan                   # a NaN pair
    Z = np.random.RandomState(0).standard_normal((4, 3, 5))
    p = ref.propose(state, seen, lambda k, nit: Z[k], 3, dtype=np.float64)
    assert p["fresh"].tolist() == [1, 0, 1, 1] and np.array_equal(p["seen"], state["ist"][:, 1])
    assert np.array_equal(p["X"][1], np.broadcast_to(state["x"][1], (3, 5))) and np.isnan(p["logq"][1])
    assert np.isnan(p["mu"][1]).all() and np.isnan(p["cov"][1]).all()
    assert np.isfinite(p["X"][0]).all() and np.isfinite(p["logq"][0]) and p["info"][0] == 0
    for k in (2, 3):
        assert p["info"][k] != 0 or np.isnan(p["logq"][k])
        assert np.isnan(p["X"][k]).all()


def test_select_keeps_the_first_maximum_and_ignores_what_is_not_finite():
    K, D, M = 8, 2, 4
    best = ref.new_best(np.zeros((K, D)))
    best["best_elbo"][:] = [-np.inf, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5, -np.inf]
    mu, cov = np.arange(K * D, dtype=np.float64).reshape(K, D), np.ones((K, D, D))
    lpsum = np.array([4.0, 6.0, 8.0, np.nan, np.inf, -np.inf, 8.0, 8.0])      # e = 1, 1.5 (a tie), 2, NaN, +inf, -inf, 2, 2
    fresh = np.array([1, 1, 1, 1, 1, 1, 0, 1])
    info = np.array([0, 0, 0, 0, 0, 0, 0, 3])
    out = ref.select(lpsum, np.zeros(K), fresh, info, np.full(K, 9), mu, cov, best, M)
    assert out["best_it"].tolist() == [9, -1, 9, -1, -1, -1, -1, -1]
    assert out["best_elbo"].tolist()[:3] == [1.0, 1.5, 2.0] and out["npts"].tolist() == [1, 1, 1, 1, 1, 1, 0, 1]
    assert np.array_equal(out["elbo_last"], [1.0, 1.5, 2.0, np.nan, np.inf, -np.inf, np.nan, np.nan], equal_nan=True)
    assert np.array_equal(out["best_mean"][2], mu[2]) and np.array_equal(out["best_mean"][1], np.zeros(D))
    assert np.array_equal(best["best_elbo"][:2], [-np.inf, 1.5])              # the input is not written


# ---- host logic on the stand-in engine ---------------------------------------------------------------------------------------
def _gaussian_callables(K, D, seed=0):
    funs = [ref.quadratic(D, seed=seed + k) for k in range(K)]

    def lp(X):
        X = np.asarray(X)
        return np.array([[-f(x)[0] for x in X[k]] for k, f in enumerate(funs)])

    def lp_g(X):
        X = np.asarray(X)
        return np.array([[-f(x)[1] for x in X[k]] for k, f in enumerate(funs)])
    return lp, lp_g, funs


def _run(K=3, D=4, **kw):
    import gsmvi_amd
    eng = ref.StandInEngine()
    lp, lp_g, funs = _gaussian_callables(K, D)
    out = gsmvi_amd.pathfinder_init_batched(np.ones((K, D)), lp, lp_g, engine=eng, **kw)
    return out, eng, funs


def test_argument_errors_need_no_gpu():
    import gsmvi_amd
    lp = lambda x: np.zeros(x.shape[0])                                 # noqa: E731
    lp_g = lambda x: np.zeros_like(x)                                   # noqa: E731
    f = gsmvi_amd.pathfinder_init_batched
    with pytest.raises(ValueError, match="pathfinder_init_batched: D = 0 is outside 1 <= D <= 64"):
        f(np.zeros((3, 0)), lp, lp_g)
    with pytest.raises(ValueError, match="outside 1 <= D <= 64"):
        f(np.zeros((3, 65)), lp, lp_g)
    with pytest.raises(ValueError, match=r"pathfinder_init_batched: x0 must be \(K, D\) or \(D,\)"):
        f(np.zeros((3, 1, 4)), lp, lp_g)
    with pytest.raises(ValueError, match="K = 0"):
        f(np.zeros((0, 4)), lp, lp_g)
    with pytest.raises(ValueError, match="pathfinder_init_batched: lp and lp_g are both required"):
        f(np.zeros((3, 4)), None, lp_g)
    with pytest.raises(ValueError, match="both required"):
        f(np.zeros((3, 4)), lp, None)
    with pytest.raises(ValueError, match="pathfinder_init_batched: maxiter and check_every must be at least 1, maxfun at least 2"):
        f(np.zeros((3, 4)), lp, lp_g, maxfun=1)
    with pytest.raises(ValueError, match="at least 1"):
        f(np.zeros((3, 4)), lp, lp_g, check_every=0)
    with pytest.raises(ValueError, match="pathfinder_init_batched: gtol and ftol must be >= 0"):
        f(np.zeros((3, 4)), lp, lp_g, gtol=-1.0)
    for bad in (0, 4097, -3, 2.5):
        with pytest.raises(ValueError, match="num_elbo_draws"):
            f(np.zeros((3, 4)), lp, lp_g, num_elbo_draws=bad)
    for bad in ("diag", 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="h0 must be"):
            f(np.zeros((3, 4)), lp, lp_g, h0=bad)


def test_launch_order_nevals_and_the_result_fields():
    (mean, cov, res), eng, funs = _run(num_elbo_draws=5, check_every=1)
    launches = [c for c in eng.calls if c == "select" or (isinstance(c, tuple) and c[0] in ("lbfgs_step", "propose"))
                or c in ("host_score", "read_flag")]
    per_round = launches[:5]
    assert per_round == ["host_score", ("lbfgs_step", True), ("propose", 0.0), "select", "read_flag"]
    assert len(launches) == 5 * res.nlaunch and launches[5:10] == ["host_score", ("lbfgs_step", False), ("propose", 0.0), "select",
                                                                   "read_flag"]
    assert ("pathfinder_state", 5) in eng.calls
    assert res.nevals == res.nlaunch * 6 and res.nlaunch == res.nfev.max()
    K, D = mean.shape
    assert cov.shape == (K, D, D) and res.success.all() and (res.best_it >= 0).all() and np.isfinite(res.elbo).all()
    assert (res.n_points == res.nit + 1).all() and (res.best_it <= res.nit).all() and (res.status == 1).all()
    for k, f in enumerate(funs):                                          # a quadratic: the optimum, and a covariance near P^-1
        assert np.abs(res.x[k] - f.mean).max() <= 1e-3
        assert np.array_equal(cov[k], cov[k].T) and np.linalg.eigvalsh(cov[k]).min() > 0.0
    # the L-BFGS fields are the plain L-BFGS run's
    for k, f in enumerate(funs):
        st = lref.run(f, np.ones(D))
        assert np.array_equal(res.x[k], st["x"]) and res.nit[k] == st["nit"] and res.nfev[k] == st["nfev"] and res.fun[k] == st["f"]
    # a fixed base goes to the launch as it is
    (_, _, _), eng2, _ = _run(num_elbo_draws=2, h0=2.5)
    assert ("propose", 2.5) in eng2.calls and ("pathfinder_state", 2) in eng2.calls


def test_the_result_does_not_depend_on_check_every_or_on_the_neighbours():
    runs = {c: _run(check_every=c, maxfun=40)[0] for c in (1, 8, 1000)}
    for c in (1, 1000):
        for a, b in zip(runs[c][:2], runs[8][:2]):
            assert np.array_equal(a, b)
        for name in ("x", "fun", "jac", "nit", "nfev", "status", "elbo", "best_it", "n_points", "success"):
            assert np.array_equal(getattr(runs[c][2], name), getattr(runs[8][2], name)), (c, name)
    assert runs[1000][2].nlaunch == 40 and runs[1000][2].nevals == 40 * 6 and runs[8][2].nlaunch % 8 == 0
    # keys are per problem (seed + k): problem 0 of K = 3 is the run of K = 1 with the same seed
    import gsmvi_amd
    lp, lp_g, _ = _gaussian_callables(1, 4)
    m1, c1, r1 = gsmvi_amd.pathfinder_init_batched(np.ones((1, 4)), lp, lp_g, engine=ref.StandInEngine())
    assert np.array_equal(m1[0], runs[8][0][0]) and np.array_equal(c1[0], runs[8][1][0]) and r1.elbo[0] == runs[8][2].elbo[0]
    other = _run(check_every=8, maxfun=40, seed=11)[0]
    assert np.array_equal(other[2].x, runs[8][2].x) and not np.array_equal(other[2].elbo, runs[8][2].elbo)


def test_a_problem_without_a_finite_elbo_keeps_its_last_x_and_the_identity():
    import gsmvi_amd
    K, D = 3, 4
    lp, lp_g, funs = _gaussian_callables(K, D)

    def lp_lost(X):                                                       # problem 1: lp of every draw is NaN, the trial points are fine
        v = lp(X)
        if np.asarray(X).shape[1] > 1:
            v[1] = np.nan
        return v
    mean, cov, res = gsmvi_amd.pathfinder_init_batched(np.ones((K, D)), lp_lost, lp_g, engine=ref.StandInEngine())
    clean = _run(K, D)[0]
    assert res.success.tolist() == [True, False, True] and res.best_it[1] == -1 and res.elbo[1] == -np.inf
    assert np.array_equal(mean[1], res.x[1]) and np.array_equal(cov[1], np.eye(D)) and res.n_points[1] == res.nit[1] + 1
    assert np.array_equal(res.x, clean[2].x)
    for k in (0, 2):
        assert np.array_equal(mean[k], clean[0][k]) and np.array_equal(cov[k], clean[1][k])


def test_logistic_softmax_and_gaussian_targets_are_accepted():
    """the GLM and softmax target classes on the stand-in engine (their ``lp_g`` is device-native: called with ``out=``), a Gaussian
    through plain numpy callables; ``laplace_init_batched`` still refuses the softmax target"""
    import gsmvi_amd
    eng = ref.StandInEngine()
    A, y, counts, lam, _ = logref.make_inputs(4, 64, 10, 1)
    tgt = gsmvi_amd.BatchedLogisticTarget(A[1:], y[1:], prior_precision=lam[1:], counts=counts[1:], engine=eng)
    mean, cov, res = gsmvi_amd.pathfinder_init_batched(np.zeros(10), tgt.lp, tgt.lp_g, engine=eng)
    assert mean.shape == (3, 10) and res.success.all() and np.isfinite(res.elbo).all() and (res.status == 1).all()
    for k in range(3):
        assert np.abs(mean[k] - logref.newton_map(A[1 + k], y[1 + k], lam[1 + k], n=counts[1 + k])).max() <= 1.0
        assert np.linalg.eigvalsh(cov[k]).min() > 0.0
    eng = ref.StandInEngine()
    A, y, counts, lam, _ = sref.make_inputs(3, 64, 3, 5, 1)
    soft = gsmvi_amd.BatchedSoftmaxTarget(A[1:], y[1:], 3, prior_precision=lam[1:], counts=counts[1:], engine=eng)
    mean, cov, res = gsmvi_amd.pathfinder_init_batched(np.zeros((2, 10)), soft.lp, soft.lp_g, num_elbo_draws=3, engine=eng)
    assert mean.shape == (2, 10) and res.success.all() and np.isfinite(res.elbo).all()
    with pytest.raises(TypeError):
        gsmvi_amd.laplace_init_batched(soft)
    (mean, cov, res), _, _ = _run(2, 7)
    assert res.success.all()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_export_maps_and_ctypes_signatures_agree():
    from gsmvi_amd import _lib
    from gsmvi_amd.engine import HipEngine
    head = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    built = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "Makefile")).read()
    assert "gsmvi_pathfinder_batched.hip" in built
    for name in NAMES:
        for mp in ("exports.map", "exports_debug.map"):
            assert f"    {name};" in open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), (name, mp)
        assert name in _lib.exported_symbols()
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", head)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib._SIGS[name][1]), name
        assert hasattr(_lib.load_library(), name)
    assert "gsmvi/initializers.py:5-17" in head[head.index("Batched Pathfinder initialiser"):head.index("int " + NAMES[0])]
    assert "gsmvi_debug_pathfinder_batched_lds" in _lib._DEBUG_SIGS
    assert "gsmvi_debug_pathfinder_batched_lds" not in open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "exports.map")).read()
    m = re.search(r"#define GSMVI_PATH_BATCHED_PATHFINDER (0x[0-9a-fA-F]+)u", head)
    assert m and int(m.group(1), 16) == ref.PATH_BIT == HipEngine.PATH_BITS["batched_pathfinder"]
    assert not HipEngine.PATH_GENERIC_MASK & ref.PATH_BIT and len(set(HipEngine.PATH_BITS.values())) == len(HipEngine.PATH_BITS)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from gsmvi_amd import _lib
    ref.check_bad_arguments(_lib.load_library())


def test_lds_of_every_dimension_fits_the_default_limit():
    """the debug query walks every D: the matrix (D x (D | 1)), the ring buffers (20 D), four vectors, ten sums, the row tile
    (max(1, 4 NT / D) rows of stride D | 1) and four partial sums per problem; four problems per workgroup for D <= 16; never above
    64 KB, so no kernel attribute is set, and M plays no part"""
    from gsmvi_amd import _lib
    lib = ctypes.CDLL(_lib.library_path(debug=True))
    fn = lib.gsmvi_debug_pathfinder_batched_lds
    fn.restype, fn.argtypes = _lib._DEBUG_SIGS["gsmvi_debug_pathfinder_batched_lds"]
    worst = 0
    for D in range(1, 65):
        nbytes, ppw, tr = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0)
        assert fn(D, ctypes.byref(nbytes), ctypes.byref(ppw), ctypes.byref(tr)) == 0
        nt = 64 if D <= 16 else 256
        assert ppw.value == 256 // nt and tr.value == max(1, 4 * nt // D)
        per = D * (D | 1) + 20 * D + 4 * D + 10 + tr.value * (D | 1) + 4
        assert nbytes.value == 8 * per * ppw.value and nbytes.value <= 64 * 1024
        worst = max(worst, nbytes.value)
    assert worst == 8 * (64 * 65 + 24 * 64 + 10 + 16 * 65 + 4)
    nbytes, ppw, tr = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0)
    assert fn(65, ctypes.byref(nbytes), ctypes.byref(ppw), ctypes.byref(tr)) == 1
    assert fn(4, None, ctypes.byref(ppw), ctypes.byref(tr)) == 1
