"""The batched Laplace initialiser without a GPU: the numpy restatement (tests/laplace_batched_ref.py) is pinned to torch
autograd of the written densities (Hessian) and to scipy's Newton methods (mode); the margins that let the GPU step test compare
decisions are asserted for every trajectory it replays; the host logic of ``laplace_init_batched`` and ``neg_hessian`` runs on a
stand-in engine; the C ABI is declared, exported, bound and checks its arguments before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from scipy.optimize import minimize

import glm_batched_ref as gref
import laplace_batched_ref as ref
from gsmvi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gsmvi_glm_hessian_batched_f64", "gsmvi_laplace_step_batched_f64")


# ---- 1. the restated Hessian is autograd of the written densities --------------------------------------------------------
def _lp_torch(family, A, y, o, lam, tau):
    At, yt, ot = torch.tensor(A), torch.tensor(y), torch.tensor(o)

    def lp(x):
        t = At @ x + ot
        if family == "logistic":
            terms = yt * t - (torch.clamp(t, min=0) + torch.log1p(torch.exp(-torch.abs(t))))
        elif family == "poisson":
            terms = yt * t - torch.exp(t)
        elif family == "probit":
            terms = yt * torch.special.log_ndtr(t) + (1.0 - yt) * torch.special.log_ndtr(-t)
        else:
            terms = -0.5 * tau * (yt - t) ** 2
        return terms.sum() - 0.5 * lam * (x * x).sum()
    return lp


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("K,N,D", [(3, 1, 1), (4, 33, 17), (3, 70, 10)])
def test_restated_hessian_is_autograd_of_the_written_density(family, K, N, D):
    """offsets, counts, per-problem lam and tau; X scaled so that |eta| <= 8, where float64 autograd of log_ndtr is itself
    good to the bar of 1e-10 of max|H| (the weights at any eta are held to mpmath in tests/test_glm_link_truth_cpu.py)"""
    A, y, o, counts, lam, tau, X = gref.make_inputs(family, K, N, D, 1)
    X = X[:, 0, :]
    for k in range(K):                                                  # hold |eta| to 8
        eta = A[k, :counts[k]] @ X[k] + o[k, :counts[k]]
        X[k] *= min(1.0, 7.0 / max(np.abs(eta).max(), 1e-300))
    H = ref.neg_hessian(family, A, y, o, counts, lam, tau, X)
    worst, emax = 0.0, 0.0
    for k in range(K):
        p = ref.problem(family, A, y, o, counts, lam, tau, k)
        emax = max(emax, float(np.abs(p["A"] @ X[k] + p["o"]).max()))
        Ht = -torch.autograd.functional.hessian(_lp_torch(family, p["A"], p["y"], p["o"], p["lam"], p["tau"]),
                                                torch.tensor(X[k])).numpy()
        e = np.abs(H[k] - Ht).max() / np.abs(Ht).max()
        worst = max(worst, e)
        assert e <= 1e-10, (family, k, e)
        assert np.array_equal(H[k], H[k].T)
    assert emax <= 8.0
    print(f"{family} K={K} N={N} D={D}: worst error {worst:.2e} of max|H|, max|eta| {emax:.2f}")


def test_weights_are_minus_the_derivative_of_the_links_r():
    """w against a central difference (h = 1e-5) of glm_batched_ref.link's r, all families, |eta| <= 8"""
    eta = np.linspace(-8.0, 8.0, 161)
    for family in ref.FAMILIES:
        for yv in ((0.0, 1.0, 0.3) if family in ("logistic", "probit") else (0.0, 3.0)):
            y = np.full_like(eta, yv)
            w, flag = ref.weights(family, eta, y, 1.7)
            h = 1e-5
            rp, rm = gref.link(family, eta + h, y, 1.7)[0], gref.link(family, eta - h, y, 1.7)[0]
            fd = -(rp - rm) / (2 * h)
            assert not flag.any() and (w >= 0.0).all()
            assert np.abs(w - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max()), (family, yv)
    with np.errstate(over="ignore"):
        w, flag = ref.weights("poisson", np.array([0.0, 710.0, np.nan]), np.zeros(3))
    assert flag.tolist() == [False, True, True]


# ---- 2. the restated run finds scipy's mode ----------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("shape", [(5, 40, 3), (5, 65, 17)])
def test_restated_run_finds_the_mode_scipy_finds(family, shape):
    K, N, D = shape
    A, y, o, counts, lam, tau, _ = ref.inputs(family, shape)
    for k in range(1, K):                                               # lam_k > 0
        p = ref.problem(family, A, y, o, counts, lam, tau, k)
        st = ref.run(p, np.zeros(D))
        assert st["status"] == 1 and np.abs(st["g"]).max() <= 1e-8 and st["nit"] <= 7 and st["nfev"] <= 9, (k, st)
        sp = minimize(lambda x: ref.evaluate(p, x)[0], np.zeros(D), jac=lambda x: ref.evaluate(p, x)[1],
                      hess=lambda x: ref.evaluate(p, x)[2], method="trust-exact", options={"gtol": 1e-8})
        assert np.abs(sp.jac).max() <= 1e-6, (k, sp.message)          # (near the mode scipy may stop on its own rounding)
        # -grad^2 lp >= lam I: |x - x*|_2 <= |g|_2 / lam at either point
        bound = (np.linalg.norm(st["g"]) + np.linalg.norm(sp.jac)) / p["lam"]
        assert np.linalg.norm(st["x"] - sp.x) <= bound + 1e-12, (k, np.linalg.norm(st["x"] - sp.x), bound)


def test_the_slack_keeps_the_line_search_from_stalling():
    """every make_inputs problem with a proper prior, the six shapes, the four families, gtol = 1e-8: at most 7 iterations, 9
    evaluations and one rejected trial per search"""
    worst = [0, 0, 0]
    for family in ref.FAMILIES:
        for shape in ref.SHAPES:
            A, y, o, counts, lam, tau, _ = gref.make_inputs(family, *shape, 1)
            for k in range(1, shape[0]):
                st, rec = ref.run(ref.problem(family, A, y, o, counts, lam, tau, k), np.zeros(shape[2]), record=True)
                nls = max(a["nls"] for _, a, _ in rec)
                worst = [max(worst[0], st["nit"]), max(worst[1], st["nfev"]), max(worst[2], nls)]
                assert st["status"] == 1 and st["nit"] <= 7 and st["nfev"] <= 9 and nls <= 1, (family, shape, k, st["nit"], st["nfev"], nls)
    print(f"worst nit {worst[0]}, nfev {worst[1]}, rejected trials per search {worst[2]}")


# ---- 3. the margins the GPU step test relies on -------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_margins_of_every_replayed_trajectory(family, shape):
    """no max|g| within a factor 1.5 of gtol, every Armijo decision by at least 1e-11 max(1, |f|), every run converged (so no
    pivot decides anything): a kernel that differs from the restatement by rounding takes the same branches"""
    low = 1.0
    for off in (False, True):
        for k, st, rec in ref.trajectories(family, shape, off):
            assert st["status"] == 1, (off, k, st["status"])
            for _, _, notes in rec:
                if "gmax" in notes:
                    assert not ref.STEP_GTOL / 1.5 <= notes["gmax"] <= 1.5 * ref.STEP_GTOL, (off, k, notes["gmax"])
                if "armijo" in notes:
                    low = min(low, notes["armijo"])
                    assert notes["armijo"] >= 1e-11, (off, k, notes["armijo"])
                assert notes.get("info", 0) == 0
    print(f"{family} {shape} (seed {ref.SEEDS.get((family, shape), 'N + D')}): smallest Armijo margin {low:.2e} max(1, |f|)")


def test_the_trajectories_reject_trials_and_a_stopped_state_is_frozen():
    rej = sum(1 for fam in ref.FAMILIES for sh in ref.SHAPES for _, _, rec in ref.trajectories(fam, sh, True)
              for b, a, _ in rec if a["nls"] > b["nls"])
    assert rej > 0                                                      # the reject branch is replayed too
    k, st, rec = ref.trajectories("poisson", ref.SHAPES[0], True)[1]
    A, y, o, counts, lam, tau, _ = ref.inputs("poisson", ref.SHAPES[0])
    again, notes = ref.step(ref.problem("poisson", A, y, o, counts, lam, tau, k), st, False)
    assert notes == {} and all(np.array_equal(again[key], st[key]) for key in st)
    one = ref.pack([st])
    assert one["ist"].dtype == np.int32 and one["ist"][0, :4].tolist() == [1, st["nit"], st["nfev"], st["nls"]]
    assert one["sc"][0].tolist() == [st["f"], st["t"], st["gd"], 0.0]


def test_the_pivot_rule_fails_rank_deficient_and_zero_matrices():
    A, y, o, counts, lam, tau, _ = gref.make_inputs("logistic", 3, 9, 16, 1)
    H = ref.neg_hessian("logistic", A, y, o, counts, lam, tau, np.zeros((3, 16)))
    cov, info = ref.inverse(H[0])                                       # rank 9, flat prior
    assert 1 <= info <= 16 and info >= 10 and np.array_equal(cov, np.eye(16))
    assert ref.inverse(H[1])[1] == 0
    assert ref.inverse(np.zeros((4, 4)))[1] == 1 and ref.inverse(np.full((2, 2), np.nan))[1] == 1


# ---- 4. host logic on a stand-in engine ----------------------------------------------------------------------------------------
def _targets(family="poisson", shape=(5, 40, 3), flat=False):
    import gsmvi_amd
    A, y, o, counts, lam, tau, _ = gref.make_inputs(family, *shape, 1)
    if not flat:
        lam[0] = 0.5
    eng = ref.StandInEngine()
    tgt = gsmvi_amd.BatchedGLMTarget(A, y, family, prior_precision=lam, counts=counts, offset=o, noise_precision=tau, engine=eng)
    return tgt, eng, (A, y, o, counts, lam, tau)


def test_laplace_init_batched_on_the_stand_in_engine():
    import gsmvi_amd
    tgt, eng, (A, y, o, counts, lam, tau) = _targets()
    K, D = 5, 3
    runs = {c: gsmvi_amd.laplace_init_batched(tgt, check_every=c) for c in (1, 4, 1000)}
    mean, cov, res = runs[4]
    assert isinstance(res, gsmvi_amd.LaplaceBatchedResult) and mean.shape == (K, D) and cov.shape == (K, D, D)
    assert res.success.all() and (res.status == 1).all() and (res.info == 0).all() and res.nlaunch % 4 == 0
    assert runs[1][2].nlaunch == runs[1][2].nfev.max() and runs[1000][2].nlaunch == 200
    for c in (1, 1000):                                                 # the result does not depend on check_every
        assert np.array_equal(runs[c][0], mean) and np.array_equal(runs[c][1], cov)
        for f in ("x", "fun", "jac", "nit", "nfev", "status", "info"):
            assert np.array_equal(getattr(runs[c][2], f), getattr(res, f)), (c, f)
    for k in range(K):
        st = ref.run(ref.problem("poisson", A, y, o, counts, lam, tau, k), np.zeros(D))
        assert np.array_equal(mean[k], st["x"]) and res.nit[k] == st["nit"] and res.nfev[k] == st["nfev"]
        assert np.allclose(cov[k], np.linalg.inv(ref.neg_hessian("poisson", A, y, o, counts, lam, tau, mean)[k]), rtol=1e-12)
    # the three forms of x0
    x1 = 0.1 * np.ones(D)
    a = gsmvi_amd.laplace_init_batched(tgt, x0=x1)
    b = gsmvi_amd.laplace_init_batched(tgt, x0=np.tile(x1, (K, 1)))
    c = gsmvi_amd.laplace_init_batched(tgt, x0=torch.tensor(x1))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0]) and np.allclose(a[0], mean, atol=1e-7)
    assert not np.array_equal(a[2].nfev, 0 * a[2].nfev)


def test_failures_return_the_last_point_and_the_identity():
    import gsmvi_amd
    tgt, eng, _ = _targets()
    mean, cov, res = gsmvi_amd.laplace_init_batched(tgt, maxiter=1)     # one iteration: status 2 everywhere
    assert (res.status == 2).all() and not res.success.any() and (res.info == 0).all() and (res.nit == 1).all()
    assert np.array_equal(cov, np.broadcast_to(np.eye(3), (5, 3, 3))) and np.isfinite(mean).all() and mean.any()
    x0 = np.zeros((5, 3))
    x0[2, 1] = np.nan                                                   # a non-finite start: status 4, info 1, cov = I
    mean, cov, res = gsmvi_amd.laplace_init_batched(tgt, x0=x0)
    assert res.status.tolist() == [1, 1, 4, 1, 1] and res.info.tolist() == [0, 0, 1, 0, 0] and res.success.tolist() == [1, 1, 0, 1, 1]
    assert np.array_equal(cov[2], np.eye(3)) and np.isnan(mean[2, 1]) and not np.array_equal(cov[1], np.eye(3))
    # a flat prior on fewer rows than dimensions: H is singular, status 5
    import gsmvi_amd as g
    A, y, o, counts, lam, tau, _ = gref.make_inputs("logistic", 3, 9, 16, 1)
    t2 = g.BatchedLogisticTarget(A, y, prior_precision=lam, counts=counts, engine=ref.StandInEngine())
    mean, cov, res = g.laplace_init_batched(t2)
    assert res.status[0] == 5 and not res.success[0] and np.array_equal(cov[0], np.eye(16)) and res.success[1:].all()


def test_argument_errors_need_no_gpu():
    import gsmvi_amd
    tgt, eng, _ = _targets()
    n = len(eng.calls)
    with pytest.raises(TypeError, match="BatchedGLMTarget or a BatchedLogisticTarget"):
        gsmvi_amd.laplace_init_batched(lambda x: x)
    with pytest.raises(TypeError, match="BatchedGLMTarget or a BatchedLogisticTarget"):
        gsmvi_amd.laplace_init_batched(np.zeros((5, 3)))
    for x0 in (np.zeros(4), np.zeros((4, 3)), np.zeros((5, 3, 1)), 0.0):
        with pytest.raises(ValueError, match=r"x0 must be None, \(D,\)"):
            gsmvi_amd.laplace_init_batched(tgt, x0=x0)
    for kw in (dict(maxiter=0), dict(maxfun=1), dict(check_every=0)):
        with pytest.raises(ValueError, match="maxiter and check_every must be at least 1, maxfun at least 2"):
            gsmvi_amd.laplace_init_batched(tgt, **kw)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="gtol must be >= 0"):
            gsmvi_amd.laplace_init_batched(tgt, gtol=bad)
    assert len(eng.calls) == n                                          # nothing reached the engine


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_neg_hessian_of_the_targets_on_the_stand_in_engine(family):
    import gsmvi_amd
    tgt, eng, (A, y, o, counts, lam, tau) = _targets(family, (4, 33, 17), flat=True)
    X = 0.3 * np.random.RandomState(1).standard_normal((4, 17))
    H = tgt.neg_hessian(X)
    assert H.shape == (4, 17, 17) and ("hessian", family, "h") in eng.calls
    assert np.array_equal(H, ref.neg_hessian(family, A, y, o, counts, lam, tau, X))
    assert np.array_equal(tgt.neg_hessian(torch.tensor(X)), H)
    if family == "logistic":
        t2 = gsmvi_amd.BatchedLogisticTarget(A, y, prior_precision=lam, counts=counts, engine=ref.StandInEngine())
        t3 = gsmvi_amd.BatchedGLMTarget(A, y, family, prior_precision=lam, counts=counts, engine=ref.StandInEngine())
        assert np.array_equal(t2.neg_hessian(X), t3.neg_hessian(X))
        assert (t2.family, t2.offset, t2.noise_precision) == ("logistic", None, 1.0)


# ---- 5. the C ABI ------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    head = hdr.split("#ifndef GSMVI_HIP_H")[0]
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr)
        for mp in ("exports.map", "exports_debug.map"):
            assert re.search(r"^\s*" + name + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), (mp, name)
        assert name in _lib.exported_symbols() and name in built and name in head
        res, args = _lib._SIGS[name]
        decl = re.search(r"int\s+" + name + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert res is C.c_int and len(args) == len(params) == (18 if "hessian" in name else 25)
        for p, a in zip(params, args):
            want = C.c_double if p.startswith("double ") else C.c_int64 if p.startswith("int64_t") else \
                C.c_int if p.startswith("int ") else C.c_void_p
            assert a is want, (name, p, a)
    block = hdr[:hdr.index("int " + NAMES[0])].rsplit("/*", 1)[1]
    for word in ("initializers.py:5-17", "example_gsm.py:34-35", "GSMVI_PATH_BATCHED_LAPLACE", "64 eps", "eps eta^2", "1e-10 max(1, |f|)"):
        assert word in block, word
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_LAPLACE\s+0x80000u", hdr)
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_laplace"] == 0x80000
    mk = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "Makefile")).read()
    assert "gsmvi_laplace_batched.hip" in mk and "gsmvi_glm_link.h" in mk


def test_entry_points_reject_bad_arguments_without_a_gpu():
    ref.check_bad_arguments(_lib.load_library())
