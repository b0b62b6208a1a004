"""The shared-design Laplace initialiser without a GPU: the numpy restatement (tests/shared_laplace_ref.py) is pinned to torch
autograd of the written density with observation weights and, at v = 1, to laplace_batched_ref.evaluate on the replicated design
bit for bit; the margins that let the GPU step test compare decisions are asserted for every trajectory it replays; the host logic
of ``laplace_init_shared_batched`` and ``neg_hessian_shared_batched`` runs on a stand-in engine; the C ABI is declared, exported,
bound and checks its arguments before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import laplace_batched_ref as lref
import shared_laplace_ref as ref
from gsmvi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement is pinned -------------------------------------------------------------------------------------------
def _phi_torch(family, A, y, o, v, lam, tau):
    At, yt, ot, vt = torch.tensor(A), torch.tensor(y), torch.tensor(o), torch.tensor(v)

    def phi(x):
        t = At @ x + ot
        if family == "logistic":
            terms = yt * t - (torch.clamp(t, min=0) + torch.log1p(torch.exp(-torch.abs(t))))
        elif family == "poisson":
            terms = yt * t - torch.exp(t)
        elif family == "probit":
            terms = yt * torch.special.log_ndtr(t) + (1.0 - yt) * torch.special.log_ndtr(-t)
        else:
            terms = -0.5 * tau * (yt - t) ** 2
        return -((vt * terms).sum() - 0.5 * lam * (x * x).sum())
    return phi


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("K,N,D", [(3, 1, 1), (4, 33, 17), (3, 70, 10)])
def test_restated_f_g_h_are_autograd_of_the_written_density(family, K, N, D):
    """weights (a quarter of them zero, with y = NaN and offset = inf there), offsets, per-problem lam and tau; the zero-weight
    observations are taken out of the written density, which cannot hold a NaN; X scaled so that |eta| <= 8, where float64
    autograd of log_ndtr is itself good to the bars: 1e-10 of max|H|, 1e-11 of the scales of f and g"""
    A, y, o, v, lam, tau, X = ref.make_inputs(family, K, N, D, 1, poison=True)
    if N == 1:
        v[:, 0], y[:, 0], o[:, 0] = 1.3, 1.0, 0.2                        # one selected observation
    X = X[:, 0, :]
    worst = [0.0, 0.0, 0.0]
    for k in range(K):
        p = ref.problem(family, A, y, o, v, lam, tau, k)
        assert np.isfinite(p["y"]).all() and np.isfinite(p["o"]).all() and (p["v"] > 0).all() and len(p["v"]) == (v[k] > 0).sum()
        eta = p["A"] @ X[k] + p["o"]
        X[k] *= min(1.0, 7.0 / max(np.abs(eta).max(), 1e-300))
        assert np.abs(p["A"] @ X[k] + p["o"]).max() <= 8.0
        f, g, H, sc = ref.evaluate(p, X[k])
        phi = _phi_torch(family, p["A"], p["y"], p["o"], p["v"], p["lam"], p["tau"])
        xt = torch.tensor(X[k], requires_grad=True)
        ft = phi(xt)
        gt, = torch.autograd.grad(ft, xt)
        Ht = torch.autograd.functional.hessian(phi, torch.tensor(X[k])).numpy()
        e = [abs(f - ft.item()) / sc["f"], (np.abs(g - gt.numpy()) / sc["g"]).max(), np.abs(H - Ht).max() / np.abs(Ht).max()]
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert e[0] <= 1e-11 and e[1] <= 1e-11 and e[2] <= 1e-10, (family, k, e)
        assert np.array_equal(H, H.T)
    print(f"{family} K={K} N={N} D={D}: worst errors f {worst[0]:.1e}, g {worst[1]:.1e} of their scales, H {worst[2]:.1e} of max|H|")


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_unit_weights_are_the_per_problem_restatement_on_the_replicated_design(family):
    K, N, D = 4, 33, 17
    A, y, o, v, lam, tau, X = ref.make_inputs(family, K, N, D, 1)
    Ar = ref.replicate(A, K)
    for weights in (None, np.ones((K, N))):
        for k in range(K):
            a = ref.evaluate(ref.problem(family, A, y, o, weights, lam, tau, k), X[k, 0])
            b = lref.evaluate(lref.problem(family, Ar, y, o, None, lam, tau, k), X[k, 0])
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            assert all(np.array_equal(a[3][n], b[3][n]) for n in ("f", "g", "H"))
    H = ref.neg_hessian(family, A, y, None, None, lam, tau, X[:, 0])
    assert np.array_equal(H, lref.neg_hessian(family, Ar, y, None, None, lam, tau, X[:, 0]))


def test_an_observation_without_weight_contributes_nothing_and_flags_nothing():
    K, N, D = 3, 20, 4
    A, y, o, v, lam, tau, X = ref.make_inputs("poisson", K, N, D, 1)
    clean = [ref.evaluate(ref.problem("poisson", A, y, o, v, lam, tau, k), X[k, 0]) for k in range(K)]
    y2, o2, v2 = y.copy(), o.copy(), v.copy()
    y2[v == 0], o2[v == 0] = np.nan, 4000.0                             # exp(eta) overflows there
    v2[1, np.flatnonzero(v[1] == 0)[0]] = np.nan                        # a NaN weight is not > 0
    for k in range(K):
        got = ref.evaluate(ref.problem("poisson", A, y2, o2, v2, lam, tau, k), X[k, 0])
        assert got[0] == clean[k][0] and np.array_equal(got[1], clean[k][1]) and np.array_equal(got[2], clean[k][2])
    o3 = o.copy()
    o3[2, np.flatnonzero(v[2] > 0)[0]] = 4000.0                         # the same overflow at v > 0 flags its problem
    f, g, H, _ = ref.evaluate(ref.problem("poisson", A, y, o3, v, lam, tau, 2), X[2, 0])
    assert np.isnan(f) and np.isnan(g).all() and np.isnan(H).all()
    # no observation left: the prior alone
    f, g, H, _ = ref.evaluate(ref.problem("logistic", A, y, o, np.zeros((K, N)), 0.7, 1.0, 0), X[0, 0])
    assert np.array_equal(H, 0.7 * np.eye(D)) and np.array_equal(g, 0.7 * X[0, 0])


# ---- 2. the margins the GPU step test relies on -------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_margins_of_every_replayed_trajectory(family, shape):
    """tests/test_laplace_batched_cpu.py's margins for every trajectory tests/test_gpu_shared_laplace.py replays: every run
    converged, no max|g| within a factor 1.5 of gtol, every Armijo decision by at least 1e-11 max(1, |f|), no failed
    factorisation, and every pivot at least 1e3 times its threshold: a kernel that differs from the restatement by rounding
    takes the same branches"""
    for full in (True, False):
        traj = ref.trajectories(family, shape, full)
        assert len(traj) == ref.STEP_K
        ok, low, piv = ref.margins_hold(traj)
        assert ok, (full, low, piv, [st["status"] for _, st, _ in traj])
        print(f"{family} {shape} full={full} (seed {ref.SEEDS.get((family, shape), 'N + D')}): smallest Armijo margin {low:.2e} "
              f"max(1, |f|), smallest pivot {piv:.1e} thresholds")


def test_iteration_counts_of_the_trajectories_and_of_the_defaults():
    """with a proper prior: at most 7 iterations and 9 evaluations, as for the per-problem initialiser, and at most 2 rejected
    trials per search (1 there: the new maximum, with weights); the flat-prior problem 0 of the step test's trajectories, whose
    weighted data are close to separable at the small N / D, takes up to 17 iterations, 18 evaluations and 4 rejected trials"""
    proper, flat = [0, 0, 0], [0, 0, 0]
    for family in ref.FAMILIES:
        for shape in ref.SHAPES:
            for full in (True, False):
                for k, st, rec in ref.trajectories(family, shape, full):
                    nls = max(a["nls"] for _, a, _ in rec)
                    acc = flat if k == 0 else proper
                    acc[:] = [max(acc[0], st["nit"]), max(acc[1], st["nfev"]), max(acc[2], nls)]
            A, y, o, v, lam, tau, _ = ref.make_inputs(family, ref.STEP_K, *shape, 1)
            for k in range(1, ref.STEP_K):                              # the defaults: gtol = 1e-8, the default seed
                for oo, vv in ((o, v), (None, None)):
                    st, rec = ref.run(ref.problem(family, A, y, oo, vv, lam, tau, k), np.zeros(shape[1]), record=True)
                    nls = max(a["nls"] for _, a, _ in rec)
                    assert st["status"] == 1, (family, shape, k)
                    proper[:] = [max(proper[0], st["nit"]), max(proper[1], st["nfev"]), max(proper[2], nls)]
    print(f"proper prior: worst nit {proper[0]}, nfev {proper[1]}, rejected trials {proper[2]}; flat prior: {flat}")
    assert proper[0] <= 7 and proper[1] <= 9 and proper[2] <= 2, proper
    assert flat[0] <= 17 and flat[1] <= 18 and flat[2] <= 4, flat


def test_the_trajectories_reject_trials_and_a_stopped_state_is_frozen():
    rej = sum(1 for fam in ref.FAMILIES for sh in ref.SHAPES for _, _, rec in ref.trajectories(fam, sh, True)
              for b, a, _ in rec if a["nls"] > b["nls"])
    assert rej > 0                                                      # the reject branch is replayed too
    k, st, rec = ref.trajectories("poisson", ref.SHAPES[0], True)[1]
    A, y, o, v, lam, tau, _ = ref.inputs("poisson", ref.SHAPES[0])
    again, notes = ref.step(ref.problem("poisson", A, y, o, v, lam, tau, k), st, False)
    assert notes == {} and all(np.array_equal(again[key], st[key]) for key in st)


# ---- 3. host logic on the stand-in engine --------------------------------------------------------------------------------------
def _target(family="poisson", N=40, D=3, K=5, flat=False, weights=True):
    import gsmvi_amd
    A, y, o, v, lam, tau, _ = ref.make_inputs(family, K, N, D, 1)
    if not flat:
        lam[0] = 0.5
    eng = ref.StandInEngine()
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, family, prior_precision=lam, offset=o, weights=v if weights else None,
                                          noise_precision=tau, engine=eng)
    return tgt, eng, (A, y, o, v if weights else None, lam, tau)


def test_laplace_init_shared_batched_on_the_stand_in_engine():
    import gsmvi_amd
    tgt, eng, (A, y, o, v, lam, tau) = _target()
    K, D = 5, 3
    runs = {c: gsmvi_amd.laplace_init_shared_batched(tgt, check_every=c) for c in (1, 4, 1000)}
    mean, cov, res = runs[4]
    assert isinstance(res, gsmvi_amd.LaplaceBatchedResult) and mean.shape == (K, D) and cov.shape == (K, D, D)
    assert res.success.all() and (res.status == 1).all() and (res.info == 0).all() and res.nlaunch % 4 == 0
    assert runs[1][2].nlaunch == runs[1][2].nfev.max() and runs[1000][2].nlaunch == 200
    for c in (1, 1000):                                                 # the result does not depend on check_every
        assert np.array_equal(runs[c][0], mean) and np.array_equal(runs[c][1], cov)
        for f in ("x", "fun", "jac", "nit", "nfev", "status", "info"):
            assert np.array_equal(getattr(runs[c][2], f), getattr(res, f)), (c, f)
    for k in range(K):
        st = ref.run(ref.problem("poisson", A, y, o, v, lam, tau, k), np.zeros(D))
        assert np.array_equal(mean[k], st["x"]) and res.nit[k] == st["nit"] and res.nfev[k] == st["nfev"]
        assert np.allclose(cov[k], np.linalg.inv(ref.neg_hessian("poisson", A, y, o, v, lam, tau, mean)[k]), rtol=1e-12)
    assert ("laplace_shared_step", "poisson", True) in eng.calls and ("shared_hessian", "poisson", "cov") in eng.calls
    assert not any(isinstance(c, tuple) and c[0] in ("laplace_step", "hessian", "glm_shared") for c in eng.calls)
    # the three forms of x0
    x1 = 0.1 * np.ones(D)
    a = gsmvi_amd.laplace_init_shared_batched(tgt, x0=x1)
    b = gsmvi_amd.laplace_init_shared_batched(tgt, x0=np.tile(x1, (K, 1)))
    c = gsmvi_amd.laplace_init_shared_batched(tgt, x0=torch.tensor(x1))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0]) and np.allclose(a[0], mean, atol=1e-7)
    assert not np.array_equal(a[2].nfev, 0 * a[2].nfev)


def test_failures_return_the_last_point_and_the_identity():
    import gsmvi_amd
    tgt, eng, _ = _target()
    mean, cov, res = gsmvi_amd.laplace_init_shared_batched(tgt, maxiter=1)          # one iteration: status 2 everywhere
    assert (res.status == 2).all() and not res.success.any() and (res.info == 0).all() and (res.nit == 1).all()
    assert np.array_equal(cov, np.broadcast_to(np.eye(3), (5, 3, 3))) and np.isfinite(mean).all() and mean.any()
    x0 = np.zeros((5, 3))
    x0[2, 1] = np.nan                                                   # a non-finite start: status 4, info 1, cov = I
    mean, cov, res = gsmvi_amd.laplace_init_shared_batched(tgt, x0=x0)
    assert res.status.tolist() == [1, 1, 4, 1, 1] and res.info.tolist() == [0, 0, 1, 0, 0] and res.success.tolist() == [1, 1, 0, 1, 1]
    assert np.array_equal(cov[2], np.eye(3)) and np.isnan(mean[2, 1]) and not np.array_equal(cov[1], np.eye(3))
    # all weights zero: with lam > 0 the prior alone (status 1 at x = 0, cov = I / lam exactly); with lam = 0 f = g = H = 0: the
    # launches stop it by the gradient test (the state machine tests max|g| <= gtol before it factors H), the final
    # factorisation fails (info = 1), and the function reports such a stationary point as status 5, with the identity
    A, y, o, v, lam, tau, _ = ref.make_inputs("logistic", 4, 12, 3, 1)
    v[0], v[1], lam[0], lam[1] = 0.0, 0.0, 0.0, 0.25
    t2 = gsmvi_amd.SharedDesignGLMTarget(A, y, "logistic", prior_precision=lam, offset=o, weights=v, engine=ref.StandInEngine())
    mean, cov, res = gsmvi_amd.laplace_init_shared_batched(t2)
    assert res.status.tolist() == [5, 1, 1, 1] and res.success.tolist() == [0, 1, 1, 1] and res.info[0] == 1 and res.info[1] == 0
    assert res.nit[0] == 0 and res.nfev[0] == 1                       # (stopped at its start)
    assert np.array_equal(cov[0], np.eye(3)) and np.array_equal(cov[1], 4.0 * np.eye(3)) and not mean[1].any()


def test_argument_and_type_errors_need_no_gpu():
    import gsmvi_amd
    import glm_batched_ref as gref
    tgt, eng, _ = _target()
    n = len(eng.calls)
    A, y, o, counts, lam, tau, _ = gref.make_inputs("poisson", 3, 12, 4, 1)
    other = gsmvi_amd.BatchedGLMTarget(A, y, "poisson", counts=counts, engine=lref.StandInEngine())
    for bad, name in ((lambda x: x, "function"), (np.zeros((5, 3)), "ndarray"), (other, "BatchedGLMTarget")):
        with pytest.raises(TypeError, match=f"laplace_init_shared_batched: target must be a SharedDesignGLMTarget, got {name}"):
            gsmvi_amd.laplace_init_shared_batched(bad)
        with pytest.raises(TypeError, match=f"neg_hessian_shared_batched: target must be a SharedDesignGLMTarget, got {name}"):
            gsmvi_amd.neg_hessian_shared_batched(bad, np.zeros((5, 3)))
    for x0 in (np.zeros(4), np.zeros((4, 3)), np.zeros((5, 3, 1)), 0.0):
        with pytest.raises(ValueError, match=r"laplace_init_shared_batched: x0 must be None, \(D,\)"):
            gsmvi_amd.laplace_init_shared_batched(tgt, x0=x0)
    for kw in (dict(maxiter=0), dict(maxfun=1), dict(check_every=0)):
        with pytest.raises(ValueError, match="maxiter and check_every must be at least 1, maxfun at least 2"):
            gsmvi_amd.laplace_init_shared_batched(tgt, **kw)
    for badtol in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="gtol must be >= 0"):
            gsmvi_amd.laplace_init_shared_batched(tgt, gtol=badtol)
    for x in (np.zeros(3), np.zeros((4, 3)), np.zeros((5, 1, 3))):
        with pytest.raises(ValueError, match=r"neg_hessian_shared_batched: x must be \(K, D\)"):
            gsmvi_amd.neg_hessian_shared_batched(tgt, x)
    assert len(eng.calls) == n                                          # nothing reached the engine


def test_laplace_init_batched_names_the_new_function_for_the_shared_target():
    import gsmvi_amd
    tgt, _, _ = _target()
    with pytest.raises(TypeError) as e:
        gsmvi_amd.laplace_init_batched(tgt)
    assert str(e.value) == ("laplace_init_batched: target must be a BatchedGLMTarget or a BatchedLogisticTarget, got "
                            "SharedDesignGLMTarget; call laplace_init_shared_batched(target, ...) for it")
    with pytest.raises(TypeError) as e:                                  # any other type: the message as it was
        gsmvi_amd.laplace_init_batched(3)
    assert str(e.value) == "laplace_init_batched: target must be a BatchedGLMTarget or a BatchedLogisticTarget, got int"
    assert not hasattr(tgt, "neg_hessian")
    assert "neg_hessian_shared_batched" in type(tgt).__doc__ and "laplace_init_shared_batched" in type(tgt).__doc__


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_neg_hessian_shared_batched_on_the_stand_in_engine(family):
    import gsmvi_amd
    tgt, eng, (A, y, o, v, lam, tau) = _target(family, 33, 17, K=4, flat=True)
    X = 0.3 * np.random.RandomState(1).standard_normal((4, 17))
    H = gsmvi_amd.neg_hessian_shared_batched(tgt, X)
    assert H.shape == (4, 17, 17) and ("shared_hessian", family, "h") in eng.calls
    assert np.array_equal(H, ref.neg_hessian(family, A, y, o, v, lam, tau, X))
    assert np.array_equal(gsmvi_amd.neg_hessian_shared_batched(tgt, torch.tensor(X)), H)
    other = ref.StandInEngine()
    assert np.array_equal(gsmvi_amd.neg_hessian_shared_batched(tgt, X, engine=other), H) and other.calls


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
        assert "const double* weights" in params and not any("counts" in p for p in params)
        for p, a in zip(params, args):
            want = C.c_double if p.startswith("double ") else C.c_int64 if p.startswith("int64_t") else \
                C.c_int if p.startswith("int ") else C.c_void_p
            assert a is want, (name, p, a)
    block = hdr[:hdr.index("int " + ref.NAMES[0])].rsplit("/*", 1)[1]
    for word in ("initializers.py:5-17", "example_gsm.py:34-35", "GSMVI_PATH_BATCHED_LAPLACE |", "GSMVI_PATH_BATCHED_TARGET",
                 "64 eps", "1e-10 max(1, |f|)", "removed by selection", "never replicated", "word for word"):
        assert word in block, word
    # the ABI version and the path bits are unchanged: the pair of two existing bits names the new kernel
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_LAPLACE\s+0x80000u", hdr)
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_TARGET\s+0x20000u", hdr)
    for define in ("GSMVI_PATH_BATCHED_LAPLACE", "GSMVI_PATH_BATCHED_TARGET"):
        line = re.search(r"#define\s+" + define + r"\s.*", hdr).group(0)
        assert "k_laplace_shared_batched" in line, define
    assert _lib.load_library().gsmvi_abi_version() == 1
    mk = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "Makefile")).read()
    assert "gsmvi_laplace_shared_batched.hip" in mk and "gsmvi_laplace_stage.h" in mk
    src = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_laplace_shared_batched.hip")).read()
    assert '#include "gsmvi_laplace_stage.h"' in src and "lp_chol_lds(bool" not in src      # no third copy of the stage


def test_entry_points_reject_bad_arguments_without_a_gpu():
    ref.check_bad_arguments(_lib.load_library())


def test_the_public_names_are_exported():
    import gsmvi_amd
    assert callable(gsmvi_amd.laplace_init_shared_batched) and callable(gsmvi_amd.neg_hessian_shared_batched)
    from gsmvi_amd.engine import HipEngine
    assert callable(HipEngine.glm_shared_hessian_batched) and callable(HipEngine.laplace_shared_step_batched)
