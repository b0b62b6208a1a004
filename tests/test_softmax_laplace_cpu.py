"""The batched softmax Laplace initialiser without a GPU: the numpy restatement (tests/softmax_laplace_ref.py) is pinned to torch
autograd of the written density (Hessian), to softmax_batched_ref (f, g), to scipy (mode) and, at C = 2, to the logistic
restatement; the accurate 1 - p holds the bar on saturated inputs where the difference of two Gram sums does not; the margins that
let the GPU step test compare decisions are asserted for every trajectory it replays; the host logic of
``laplace_init_softmax_batched`` and ``neg_hessian`` runs on a stand-in engine, and ``laplace_init_batched`` makes the engine
calls it made before the two shared a loop; the C ABI is declared, exported, bound and checks its arguments before any device
work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from scipy.optimize import minimize

import glm_batched_ref as gref
import laplace_batched_ref as lref
import softmax_batched_ref as sref
import softmax_laplace_ref as ref
from gsmvi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gsmvi_softmax_hessian_batched_f64", "gsmvi_softmax_laplace_step_batched_f64")
BAR = 1e-11


# ---- 1. the restatement's pins ------------------------------------------------------------------------------------------------
def _lp_torch(A, y, C, lam):
    At, yt = torch.tensor(A), torch.tensor(y)

    def lp(x):
        eta = torch.cat([At @ x.reshape(C - 1, At.shape[1]).T, torch.zeros(At.shape[0], 1, dtype=torch.float64)], dim=1)
        return (eta.gather(1, yt[:, None])[:, 0] - torch.logsumexp(eta, dim=1)).sum() - 0.5 * lam * (x * x).sum()
    return lp


@pytest.mark.parametrize("shape", [(3, 1, 2, 1), (4, 33, 18, 1), (3, 70, 3, 5), (3, 40, 5, 4), (3, 33, 2, 16)])
def test_restated_hessian_is_autograd_of_the_written_density(shape):
    K, N, Cc, P = shape
    A, y, counts, lam, X = ref.inputs(shape)
    H = ref.neg_hessian(A, y, Cc, counts, lam, X)
    worst = 0.0
    for k in range(K):
        p = ref.problem(A, y, Cc, counts, lam, k)
        Ht = -torch.autograd.functional.hessian(_lp_torch(p["A"], p["y"], Cc, p["lam"]), torch.tensor(X[k])).numpy()
        scale = ref.evaluate(p, X[k])[3]["H"]
        e = float((np.abs(H[k] - Ht) / np.where(scale > 0, scale, 1.0)).max())
        worst = max(worst, e)
        assert e <= BAR, (k, e)
        assert np.array_equal(H[k], H[k].T)
    assert np.array_equal(H[1], lam[1] * np.eye((Cc - 1) * P))          # the problem without a row: the prior alone
    print(f"{shape}: worst error {worst:.2e} of the entry's scale")


@pytest.mark.parametrize("shape", [(4, 33, 18, 1), (3, 70, 3, 5), (3, 33, 2, 16)])
def test_restated_f_and_g_are_the_softmax_restatements(shape):
    K, N, Cc, P = shape
    A, y, counts, lam, X = ref.inputs(shape)
    G, lp = sref.score_and_lp(A, y, Cc, counts, lam, X[:, None, :])
    for k in range(K):
        f, g, _, sc = ref.evaluate(ref.problem(A, y, Cc, counts, lam, k), X[k])
        assert abs(f + lp[k, 0]) <= BAR * max(sc["f"], 1e-300) and (np.abs(g + G[k, 0]) <= BAR * np.maximum(sc["g"], 1e-300)).all(), k
    Xb = X.copy()
    Xb[2, 0] = np.inf
    f, g, H, _ = ref.evaluate(ref.problem(A, y, Cc, counts, lam, 2), Xb[2])
    assert np.isnan(f) and np.isnan(g).all() and np.isnan(H).all()


@pytest.mark.parametrize("shape", [(5, 40, 3, 2), (5, 65, 18, 1)])
def test_restated_run_finds_the_mode_scipy_finds(shape):
    K, N, Cc, P = shape
    D = (Cc - 1) * P
    A, y, counts, lam, _ = ref.inputs(shape)
    for k in range(1, K):                                               # lam_k > 0
        p = ref.problem(A, y, Cc, counts, lam, k)
        st = ref.run(p, np.zeros(D))
        assert st["status"] == 1 and np.abs(st["g"]).max() <= 1e-8 and st["nit"] <= 9, (k, st)
        sp = minimize(lambda x: float(ref.evaluate(p, x)[0]), np.zeros(D), jac=lambda x: ref.evaluate(p, x)[1],
                      hess=lambda x: ref.evaluate(p, x)[2], method="Newton-CG", options={"xtol": 1e-12})
        assert np.abs(st["x"] - sp.x).max() <= 1e-8, (k, np.abs(st["x"] - sp.x).max())
        # and by reasoning: -grad^2 lp >= lam I, so |x - x*|_2 <= |g|_2 / lam at either point
        bound = (np.linalg.norm(st["g"]) + np.linalg.norm(sp.jac)) / p["lam"]
        assert np.linalg.norm(st["x"] - sp.x) <= bound + 1e-12, (k, np.linalg.norm(st["x"] - sp.x), bound)


def test_two_classes_are_the_logistic_restatement():
    K, N, D = 4, 33, 16
    A, y, counts, lam, X = ref.inputs((K, N, 2, D))
    yl = (y == 0).astype(np.float64)                                    # class 0 against the reference class
    for k in range(K):
        f, g, H, sc = ref.evaluate(ref.problem(A, y, 2, counts, lam, k), X[k])
        fl, gl, Hl, _ = lref.evaluate(lref.problem("logistic", A, yl, None, counts, lam, 1.0, k), X[k])
        assert abs(f - fl) <= BAR * max(sc["f"], 1e-300) and (np.abs(g - gl) <= BAR * np.maximum(sc["g"], 1e-300)).all()
        assert (np.abs(H - Hl) <= BAR * np.maximum(sc["H"], 1e-300)).all(), k


# ---- 2. the accurate 1 - p on saturated inputs --------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Cc,P", ref.SATURATED)
def test_saturated_class_keeps_its_digits_and_a_difference_of_grams_does_not(N, Cc, P):
    worst, worst_diff = 0.0, 0.0
    for top in (25.0, 27.5, 30.0):
        p, x = ref.saturated_inputs(N, Cc, P, top)
        _, _, H, sc = ref.evaluate(p, x)
        _, _, Hl, _ = ref.evaluate(p, x.astype(np.longdouble))
        e = float((np.abs(H - Hl) / sc["H"]).max())
        ed = float((np.abs(ref.hessian_difference_of_grams(p, x) - Hl) / sc["H"]).max())
        worst, worst_diff = max(worst, e), max(worst_diff, ed)
        assert e <= BAR, (top, e)
        assert ed > BAR, (top, ed)                                      # the ruled-out form misses the bar: the test can fail
    print(f"({N}, {Cc}, {P}): the specified form {worst:.2e}, the difference of Gram sums {worst_diff:.2e} of the scale")


# ---- 3. the margins the GPU step test relies on -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_margins_of_every_replayed_trajectory(shape):
    """no max|g| within a factor 1.5 of gtol, every Armijo decision by at least 1e-11 max(1, |f|), every run converged (so no
    pivot decides anything): a kernel that differs from the restatement by rounding takes the same branches"""
    low = 1.0
    for k, st, rec in ref.trajectories(shape):
        assert st["status"] == 1, (k, st["status"])
        for _, _, notes in rec:
            if "gmax" in notes:
                assert not ref.STEP_GTOL / 1.5 <= notes["gmax"] <= 1.5 * ref.STEP_GTOL, (k, notes["gmax"])
            if "armijo" in notes:
                low = min(low, notes["armijo"])
                assert notes["armijo"] >= 1e-11, (k, notes["armijo"])
            assert notes.get("info", 0) == 0
    print(f"{shape} (seed {ref.SEEDS.get(shape, 'N + 64 C + P')}): smallest Armijo margin {low:.2e} max(1, |f|)")


def test_the_trajectories_reject_trials_and_a_stopped_state_is_frozen():
    rej = sum(1 for sh in ref.SHAPES for _, _, rec in ref.trajectories(sh) for b, a, _ in rec if a["nls"] > b["nls"])
    assert rej > 0                                                      # the reject branch is replayed too
    sh = ref.SHAPES[0]
    k, st, rec = ref.trajectories(sh)[2]
    A, y, counts, lam, _ = ref.inputs(sh, flat0=False)
    again, notes = ref.step(ref.problem(A, y, sh[2], counts, lam, k), st, False)
    assert notes == {} and all(np.array_equal(again[key], st[key]) for key in st)
    k1, st1, rec1 = ref.trajectories(sh)[1]                             # no rows: the gradient at 0 is 0, converged at the start
    assert st1["status"] == 1 and st1["nfev"] == 1 and len(rec1) == 1


# ---- 4. host logic on a stand-in engine ----------------------------------------------------------------------------------------
def _target(shape=(5, 40, 3, 2), flat=False):
    import gsmvi_amd
    A, y, counts, lam, _ = ref.inputs(shape, flat0=flat)
    eng = ref.StandInEngine()
    return gsmvi_amd.BatchedSoftmaxTarget(A, y, shape[2], prior_precision=lam, counts=counts, engine=eng), eng, (A, y, counts, lam)


def test_laplace_init_softmax_batched_on_the_stand_in_engine():
    import gsmvi_amd
    tgt, eng, (A, y, counts, lam) = _target()
    K, D = 5, 4
    runs = {c: gsmvi_amd.laplace_init_softmax_batched(tgt, check_every=c) for c in (1, 4, 1000)}
    mean, cov, res = runs[4]
    assert isinstance(res, gsmvi_amd.LaplaceBatchedResult) and mean.shape == (K, D) and cov.shape == (K, D, D)
    assert res.success.all() and (res.status == 1).all() and (res.info == 0).all() and res.nlaunch % 4 == 0
    assert runs[1][2].nlaunch == runs[1][2].nfev.max() and runs[1000][2].nlaunch == 200
    for c in (1, 1000):                                                 # the result does not depend on check_every
        assert np.array_equal(runs[c][0], mean) and np.array_equal(runs[c][1], cov)
        for f in ("x", "fun", "jac", "nit", "nfev", "status", "info"):
            assert np.array_equal(getattr(runs[c][2], f), getattr(res, f)), (c, f)
    Hm = ref.neg_hessian(A, y, 3, counts, lam, mean)
    for k in range(K):
        st = ref.run(ref.problem(A, y, 3, counts, lam, k), np.zeros(D))
        assert np.array_equal(mean[k], st["x"]) and res.nit[k] == st["nit"] and res.nfev[k] == st["nfev"]
        assert np.allclose(cov[k], np.linalg.inv(Hm[k]), rtol=1e-12)
    # the three forms of x0, and tensors out
    x1 = 0.1 * np.ones(D)
    a = gsmvi_amd.laplace_init_softmax_batched(tgt, x0=x1)
    b = gsmvi_amd.laplace_init_softmax_batched(tgt, x0=np.tile(x1, (K, 1)))
    c = gsmvi_amd.laplace_init_softmax_batched(tgt, x0=torch.tensor(x1))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0]) and np.allclose(a[0], mean, atol=1e-7)
    m2, c2, _ = gsmvi_amd.laplace_init_softmax_batched(tgt, as_torch=True)          # (the stand-in's arrays, not copies)
    assert np.array_equal(np.asarray(m2), mean) and np.array_equal(np.asarray(c2), cov)


def test_failures_return_the_last_point_and_the_identity():
    import gsmvi_amd
    tgt, eng, _ = _target()
    mean, cov, res = gsmvi_amd.laplace_init_softmax_batched(tgt, maxiter=1)          # one iteration: status 2, but for the empty problem
    assert res.status.tolist() == [2, 1, 2, 2, 2] and res.success.tolist() == [0, 1, 0, 0, 0] and (res.info == 0).all()
    assert all(np.array_equal(cov[k], np.eye(4)) for k in (0, 2, 3, 4)) and np.isfinite(mean).all() and mean.any()
    x0 = np.zeros((5, 4))
    x0[2, 1] = np.nan                                                   # a non-finite start: status 4, info 1, cov = I
    mean, cov, res = gsmvi_amd.laplace_init_softmax_batched(tgt, x0=x0)
    assert res.status.tolist() == [1, 1, 4, 1, 1] and res.info.tolist() == [0, 0, 1, 0, 0] and res.success.tolist() == [1, 1, 0, 1, 1]
    assert np.array_equal(cov[2], np.eye(4)) and np.isnan(mean[2, 1]) and not np.array_equal(cov[0], np.eye(4))
    # a flat prior on fewer rows than the rank needs: H is singular, status 5
    A, y, counts, lam, _ = ref.inputs((3, 5, 3, 8))
    counts[:] = 5
    t2 = gsmvi_amd.BatchedSoftmaxTarget(A, y, 3, prior_precision=lam, counts=counts, engine=ref.StandInEngine())
    mean, cov, res = gsmvi_amd.laplace_init_softmax_batched(t2)
    assert res.status[0] == 5 and not res.success[0] and np.array_equal(cov[0], np.eye(16)) and res.success[1:].all()


def test_argument_errors_need_no_gpu():
    import gsmvi_amd
    tgt, eng, _ = _target()
    n = len(eng.calls)
    with pytest.raises(TypeError, match="must be a BatchedSoftmaxTarget"):
        gsmvi_amd.laplace_init_softmax_batched(lambda x: x)
    A, y, o, counts, lam, tau, _ = gref.make_inputs("logistic", 3, 9, 4, 1)
    glm = gsmvi_amd.BatchedLogisticTarget(A, y, prior_precision=lam, counts=counts, engine=lref.StandInEngine())
    with pytest.raises(TypeError, match="must be a BatchedSoftmaxTarget"):
        gsmvi_amd.laplace_init_softmax_batched(glm)
    with pytest.raises(TypeError, match="BatchedGLMTarget or a BatchedLogisticTarget"):
        gsmvi_amd.laplace_init_batched(tgt)                             # (unchanged: the GLM initialiser does not take it)
    for x0 in (np.zeros(3), np.zeros((4, 4)), np.zeros((5, 4, 1)), 0.0):
        with pytest.raises(ValueError, match=r"laplace_init_softmax_batched: x0 must be None, \(D,\)"):
            gsmvi_amd.laplace_init_softmax_batched(tgt, x0=x0)
    for kw in (dict(maxiter=0), dict(maxfun=1), dict(check_every=0)):
        with pytest.raises(ValueError, match="laplace_init_softmax_batched: maxiter and check_every must be at least 1, maxfun"):
            gsmvi_amd.laplace_init_softmax_batched(tgt, **kw)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="laplace_init_softmax_batched: gtol must be >= 0"):
            gsmvi_amd.laplace_init_softmax_batched(tgt, gtol=bad)
    assert len(eng.calls) == n                                          # nothing reached the engine


def test_neg_hessian_of_the_target_on_the_stand_in_engine():
    tgt, eng, (A, y, counts, lam) = _target((4, 33, 18, 1), flat=True)
    X = 0.3 * np.random.RandomState(1).standard_normal((4, 17))
    H = tgt.neg_hessian(X)
    assert H.shape == (4, 17, 17) and ("softmax_hessian", 18, "h") in eng.calls
    assert np.array_equal(H, ref.neg_hessian(A, y, 18, counts, lam, X))
    assert np.array_equal(tgt.neg_hessian(torch.tensor(X)), H)


def test_laplace_init_batched_makes_the_engine_calls_it_made_before():
    """the GLM initialiser through the shared loop: the recorded engine calls, written out (three rounds of check_every = 2 reach
    the count of stopped problems twice ... the poisson problems of (5, 40, 3) need six evaluations at most)"""
    import gsmvi_amd

    class Recorder(lref.StandInEngine):
        def laplace_step_batched(self, state, A, y, family, **kw):
            self.seen.append(("step", family, sorted(kw), kw["start"], kw["maxiter"], kw["maxfun"], kw["gtol"], kw["offset"] is not None,
                              kw["counts"] is not None))
            return super().laplace_step_batched(state, A, y, family, **kw)

        def glm_hessian_batched(self, X, A, y, family, **kw):
            self.seen.append(("hessian", family, sorted(kw), kw["want"]))
            return super().glm_hessian_batched(X, A, y, family, **kw)

    A, y, o, counts, lam, tau, _ = gref.make_inputs("poisson", 5, 40, 3, 1)
    lam[0] = 0.5
    eng = Recorder()
    eng.seen = []
    tgt = gsmvi_amd.BatchedGLMTarget(A, y, "poisson", prior_precision=lam, counts=counts, offset=o, noise_precision=tau, engine=eng)
    n0 = len(eng.calls)
    mean, cov, res = gsmvi_amd.laplace_init_batched(tgt, maxiter=50, maxfun=90, gtol=1e-9, check_every=2)
    assert res.success.all()
    rounds = res.nlaunch
    assert rounds % 2 == 0 and rounds in (res.nfev.max(), res.nfev.max() + 1)
    step_kw = ["counts", "gtol", "maxfun", "maxiter", "noise_prec", "offset", "prior_prec", "start"]
    want = [("step", "poisson", step_kw, r == 0, 50, 90, 1e-9, True, True) for r in range(rounds)]
    want.append(("hessian", "poisson", ["counts", "noise_prec", "offset", "prior_prec", "want"], "cov"))
    assert eng.seen == want
    calls = eng.calls[n0:]
    expect = ["asarray", "laplace_state"]
    for r in range(rounds):
        expect.append(("laplace_step", "poisson", r == 0))
        if r % 2 == 1:
            expect.append("read_flag")
    expect.append(("hessian", "poisson", "cov"))
    assert calls == expect


# ---- 5. the C ABI ------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    dbg_hdr = open(os.path.join(ROOT, "include", "gsmvi_hip_debug.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    head = hdr.split("#ifndef GSMVI_HIP_H")[0]
    maps = {mp: open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read() for mp in ("exports.map", "exports_debug.map")}
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr)
        for mp in maps:
            assert re.search(r"^\s*" + name + r";", maps[mp], re.M), (mp, name)
        assert name in _lib.exported_symbols() and name in built and name in head
        res, args = _lib._SIGS[name]
        decl = re.search(r"int\s+" + name + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert res is C.c_int and len(args) == len(params) == (15 if "hessian" in name else 22)
        for p, a in zip(params, args):
            want = C.c_double if p.startswith("double ") else C.c_int64 if p.startswith("int64_t") else \
                C.c_int if p.startswith("int ") else C.c_void_p
            assert a is want, (name, p, a)
        assert params[3:6] == ["int C", "int P", "int64_t N"] and params[7] == "const int* labels"
    block = hdr[:hdr.index("int " + NAMES[0])].rsplit("/*", 1)[1]
    for word in ("initializers.py:5-17", "example_gsm.py:34-35", "GSMVI_PATH_BATCHED_SOFTMAX_LAPLACE", "w_n,cc  = p_nc (1 - p_nc)",
                 "w_n,cc' = -p_nc p_nc'", "1 - p_c* = s_rest / s", "(s - e_c) / s", "sum over the other classes",
                 "d_newton = -H^{-1} g", "gsmvi_laplace_step_batched_f64"):
        assert word in block, word
    # the debug entry: declared in the debug header, exported by the debug library only, bound with the declaration's arguments
    dbg = "gsmvi_debug_softmax_laplace_lds"
    decl = re.search(r"int\s+" + dbg + r"\s*\(([^;]*)\);", dbg_hdr, re.S).group(1)
    assert len(decl.split(",")) == len(_lib._DEBUG_SIGS[dbg][1]) == 4 and dbg not in hdr
    assert re.search(r"^\s*" + dbg + r";", maps["exports_debug.map"], re.M) and dbg not in maps["exports.map"]
    dout = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path(debug=True)], check=True, capture_output=True,
                          text=True).stdout
    assert dbg in dout and dbg not in out
    assert re.search(r"#define\s+GSMVI_ABI_VERSION\s+1\b", hdr)
    mk = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "Makefile")).read()
    assert "gsmvi_softmax_laplace_batched.hip" in mk and "gsmvi_laplace_stage.h" in mk


def test_path_bit():
    from gsmvi_amd.engine import HipEngine
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_SOFTMAX_LAPLACE\s+0x10000000u", hdr)
    mask = re.search(r"#define\s+GSMVI_PATH_GENERIC_MASK\s+\(([^)]*)\)", hdr).group(1)
    bits = 0
    for tok in re.findall(r"0x[0-9a-fA-F]+", mask):
        bits |= int(tok, 16)
    assert bits == HipEngine.PATH_GENERIC_MASK and not bits & 0x10000000
    assert HipEngine.PATH_BITS["batched_softmax_laplace"] == 0x10000000
    assert len(set(HipEngine.PATH_BITS.values())) == len(HipEngine.PATH_BITS)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    ref.check_bad_arguments(_lib.load_library())


def test_every_shape_in_bounds_launches_within_64_kb_of_lds():
    """gsmvi_debug_softmax_laplace_lds for EVERY (C, P) with (C - 1) P <= 64: at most 65536 bytes (the limit without a kernel
    attribute; with H aliased onto the sweep's tiles the worst corners stay under 40 KB), four problems per workgroup exactly
    when D <= 16; shapes out of bounds are rejected"""
    lib = C.CDLL(_lib.library_path(debug=True))
    fn = lib.gsmvi_debug_softmax_laplace_lds
    fn.restype, fn.argtypes = _lib._DEBUG_SIGS["gsmvi_debug_softmax_laplace_lds"]
    worst = (0, None)
    n = 0
    for P in range(1, 65):
        for Cc in range(2, 64 // P + 2):
            D = (Cc - 1) * P
            assert 1 <= D <= 64
            b, ppw = C.c_size_t(0), C.c_int(0)
            assert fn(Cc, P, C.byref(b), C.byref(ppw)) == 0, (Cc, P)
            assert ppw.value == (4 if D <= 16 else 1), (Cc, P, ppw.value)
            Dp = 16 * ((D + 15) // 16)
            per = 5 * Dp + 4 + max(32 * (P | 1) + 64 + 66 * (Cc - 1), D * (D | 1))
            assert b.value == 8 * per * ppw.value <= 65536, (Cc, P, b.value)
            worst = max(worst, (b.value, (Cc, P)))
            n += 1
    assert n == sum(64 // P for P in range(1, 65)) and worst[0] <= 40 * 1024
    b, ppw = C.c_size_t(0), C.c_int(0)
    for Cc, P in ((1, 4), (2, 0), (2, 65), (66, 1), (3, 33)):
        assert fn(Cc, P, C.byref(b), C.byref(ppw)) == 1, (Cc, P)
    assert fn(3, 2, None, C.byref(ppw)) == 1
    print(f"{n} shapes, worst {worst[0]} bytes at (C, P) = {worst[1]}")
