"""The batched L-BFGS initialiser on the GPU (csrc/gsmvi_lbfgs_batched.hip): every step of the restatement's trajectories
(tests/lbfgs_batched_ref.py) through the C ABI from uploaded states, the dense inverse-Hessian product against scipy's,
``lbfgs_init_batched`` end to end on the logistic posteriors against their Newton MAP, as the start of the batched fits,
and the independence of the problems bit for bit."""
import numpy as np
import pytest
import torch
from scipy.optimize import LbfgsInvHessProduct

import lbfgs_batched_ref as ref
import logistic_batched_ref as lref
from conftest import rel_err

pytestmark = pytest.mark.gpu

VECS = ("x", "g", "d", "Xt", "S", "Y")


def _upload(eng, packed):
    st = {k: eng.asarray(v).contiguous() for k, v in packed.items() if k != "ist"}
    st["ist"] = torch.as_tensor(packed["ist"], device=st["x"].device).contiguous()
    st["stopped"] = eng.new_flag()
    return st


def _download(st):
    return {k: v.cpu().numpy() for k, v in st.items()}


def _same_nonfinite(a, b):
    return np.array_equal(np.isfinite(a), np.isfinite(b)) and np.array_equal(a[~np.isfinite(a)], b[~np.isfinite(b)], equal_nan=True)


def _compare(got, want, where):
    """integers equal; doubles to 1e-11 relative per problem and array (the scalars one by one); returns the largest error"""
    assert np.array_equal(got["ist"], want["ist"]), (where, np.flatnonzero((got["ist"] != want["ist"]).any(1)).tolist())
    worst = 0.0
    for k in range(want["x"].shape[0]):
        for name in VECS:
            a, b = got[name][k], want[name][k]
            assert _same_nonfinite(a, b), (where, k, name)
            fin = np.isfinite(b)
            if fin.any():
                e = rel_err(a[fin], b[fin])
                worst = max(worst, e)
                assert e <= 1e-11, (where, k, name, e)
        a, b = got["sc"][k], want["sc"][k]
        assert _same_nonfinite(a, b), (where, k, "sc")
        fin = np.isfinite(b)
        e = float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), 1e-300)))
        worst = max(worst, e)
        assert e <= 1e-11, (where, k, "sc", e, a, b)
    return worst


# ---- per step, every step -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ref.GPU_DS)
def test_every_step_of_every_trajectory_matches_the_restatement(D):
    """each step of each input's trajectory is one problem of a launch: the restatement's state before it and its (ft, gt) go
    up, everything the launch leaves is compared with the restatement's state after it; the stopped end state of every
    trajectory rides along with a made-up evaluation and must come back bit for bit"""
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    groups = {}
    for name, fun, x0, opt in ref.gpu_cases(D):
        st, rec = ref.run(fun, x0, record=True, **opt)
        full = dict(gtol=1e-5, ftol=ref.FTOL, maxiter=1000, maxfun=1000)
        full.update(opt)
        g = groups.setdefault(tuple(sorted(full.items())), {"start": [], "step": []})
        g["start"].append(rec[0])
        g["step"] += rec[1:]
        g["step"].append((st, 0.125, np.full(D, -3.0), st))                       # frozen: nothing of it may change
    worst, nsteps = 0.0, 0
    for key, g in groups.items():
        opt = dict(key)
        # the first evaluation
        x0s = np.stack([after["x"] for _, _, _, after in g["start"]])
        fv = np.array([f for _, f, _, _ in g["start"]], dtype=np.float64)
        gv = np.stack([gt for _, _, gt, _ in g["start"]])
        st = eng.lbfgs_state_batched(eng.asarray(x0s))
        eng.last_path(reset=True)
        eng.lbfgs_step_batched(eng.asarray(fv), eng.asarray(gv), st, start=True, sign=1.0, **opt)
        assert eng.last_path(reset=True) == {"batched_lbfgs"}
        want = ref.pack([after for _, _, _, after in g["start"]])
        worst = max(worst, _compare(_download(st), want, (D, "start", key)))
        assert int(st["stopped"].item()) == int((want["ist"][:, 0] != 0).sum())
        # every later evaluation
        before = ref.pack([b for b, _, _, _ in g["step"]])
        want = ref.pack([a for _, _, _, a in g["step"]])
        fv = np.array([f for _, f, _, _ in g["step"]], dtype=np.float64)
        gv = np.stack([gt for _, _, gt, _ in g["step"]])
        st = _upload(eng, before)
        d_fv, d_gv = eng.asarray(fv), eng.asarray(gv)
        eng.lbfgs_step_batched(d_fv, d_gv, st, sign=1.0, **opt)
        got = _download(st)
        worst = max(worst, _compare(got, want, (D, "step", key)))
        nsteps += len(g["step"])
        assert int(st["stopped"].item()) == int(((want["ist"][:, 0] != 0) & (before["ist"][:, 0] == 0)).sum())
        assert np.array_equal(d_fv.cpu().numpy(), fv) and np.array_equal(d_gv.cpu().numpy(), gv, equal_nan=True)
        frozen = before["ist"][:, 0] != 0
        assert frozen.any()
        for name in VECS + ("sc", "ist"):
            assert np.array_equal(got[name][frozen], before[name][frozen], equal_nan=True), (D, name)
        # lp and its score with sign = -1 are the same computation: the same bits
        st2 = _upload(eng, before)
        eng.lbfgs_step_batched(eng.asarray(-fv), eng.asarray(-gv), st2, sign=-1.0, **opt)
        got2 = _download(st2)
        for name in VECS + ("sc", "ist"):
            assert np.array_equal(got[name], got2[name], equal_nan=True), (D, name)
    print(f"D = {D}: {nsteps} steps, worst relative error {worst:.2e}")


# ---- finish -----------------------------------------------------------------------------------------------------------------
def _finish_states():
    """states whose ring buffers hold 0, 1, 3 and 10 pairs and a wrapped buffer whose oldest pair sits mid-array, from the runs
    tests/test_lbfgs_batched_cpu.py pins to scipy: the six logistic shapes and the D = 16 Gaussian"""
    out = {}
    _, rec = ref.run(ref.gaussian_fun(16), np.ones(16), record=True)
    seen = set()
    for _, _, _, st in rec:
        key = (st["npairs"], st["head"])
        if key in ((0, 0), (1, 1), (3, 3), (10, 0), (10, 5), (10, 7)) and key not in seen:
            seen.add(key)
            out.setdefault(16, []).append(st)
    assert seen == {(0, 0), (1, 1), (3, 3), (10, 0), (10, 5), (10, 7)}
    out[16].append(rec[-1][3])
    for N, D in ref.LOGISTIC_SHAPES:
        A, y, counts, lam, _ = lref.make_inputs(13, N, D, 1)
        for k in (1, 5, 12):
            out.setdefault(D, []).append(ref.run(ref.logistic_fun(A[k], y[k], counts[k], lam[k]), np.zeros(D)))
    for D in (1, 2, 17):                                                # the remaining dimensions of the step test
        for name, fun, x0, opt in ref.gpu_cases(D):
            if name in ("logistic1", "logistic2", "far_logistic", "nan_start"):
                out.setdefault(D, []).append(ref.run(fun, x0, **opt))
    return out


def test_dense_inverse_hessian_product_matches_scipy():
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    worst = 0.0
    for D, states in sorted(_finish_states().items()):
        st = _upload(eng, ref.pack(states))
        S0, Y0 = st["S"].clone(), st["Y"].clone()
        eng.last_path(reset=True)
        cov = eng.lbfgs_hess_inv_batched(st).cpu().numpy()
        assert eng.last_path(reset=True) == {"batched_lbfgs"}
        assert torch.equal(st["S"], S0) and torch.equal(st["Y"], Y0)
        for k, s in enumerate(states):
            idx = ref.held(s)
            assert np.array_equal(cov[k], cov[k].T), (D, k)
            if not idx:
                assert np.array_equal(cov[k], np.eye(D)), (D, k)
                continue
            Hs = LbfgsInvHessProduct(s["S"][idx], s["Y"][idx]).todense()
            e = rel_err(cov[k], Hs)
            worst = max(worst, e)
            assert e <= 1e-11, (D, k, s["npairs"], s["head"], e)
            assert np.linalg.eigvalsh(cov[k]).min() > 0.0
    print(f"dense inverse-Hessian product against LbfgsInvHessProduct.todense(): worst relative error {worst:.2e}")


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _target(N, D, K=13):
    import gsmvi_amd
    A, y, counts, lam, _ = lref.make_inputs(K, N, D, 1)
    return gsmvi_amd.BatchedLogisticTarget(A, y, prior_precision=lam, counts=counts), (A, y, counts, lam)


def _check_bound(mean, res, inputs, D, gmax=None):
    A, y, counts, lam = inputs
    worst = 0.0
    for k in range(1, A.shape[0]):
        assert res.success[k] and res.status[k] == 1, (k, res.status[k])
        xs = lref.newton_map(A[k], y[k], lam[k], n=counts[k])
        bound = np.sqrt(D) * (1e-5 if gmax is None else gmax[k]) / lam[k]
        dist = np.linalg.norm(mean[k] - xs)
        worst = max(worst, dist / bound)
        assert dist <= bound, (k, dist, bound)
    return worst


@pytest.mark.parametrize("N,D", ref.LOGISTIC_SHAPES)
def test_end_to_end_on_the_logistic_posteriors(N, D):
    """ftol = 0: every problem with a proper prior converges on the gradient test, and then |x - x*|_2 <= sqrt(D) gtol / lam_k
    (derived in tests/test_lbfgs_batched_cpu.py); the same through plain numpy callables.  nit / nfev beside the restatement's
    are printed, not asserted: near the end the Armijo test is decided by the last bits of lp."""
    import gsmvi_amd
    tgt, inputs = _target(N, D)
    A, y, counts, lam = inputs
    K = A.shape[0]
    x0 = np.zeros((K, D))
    mean, cov, res = gsmvi_amd.lbfgs_init_batched(x0, tgt.lp, tgt.lp_g, ftol=0.0)
    assert mean.shape == (K, D) and cov.shape == (K, D, D) and res.x.shape == (K, D) and res.jac.shape == (K, D)
    assert np.array_equal(mean, res.x) and not x0.any()
    share = _check_bound(mean, res, inputs, D)
    assert (np.abs(res.jac[1:]).max(1) <= 1e-5).all() and (res.nfev <= res.nlaunch).all() and res.nlaunch % 8 == 0
    G, lp = lref.score_and_lp(A, y, counts, lam, mean[:, None, :])
    assert rel_err(res.fun[1:], -lp[1:, 0]) <= 1e-11
    for k in range(K):
        assert np.array_equal(cov[k], cov[k].T) and np.linalg.eigvalsh(cov[k]).min() > 0.0, k
    want = [ref.run(ref.logistic_fun(A[k], y[k], counts[k], lam[k]), np.zeros(D), ftol=0.0) for k in range(1, K)]
    print(f"(N, D) = {(N, D)}: share of the bound {share:.3f}; nit {res.nit[1:].tolist()} (restatement "
          f"{[s['nit'] for s in want]}), nfev {res.nfev[1:].tolist()} (restatement {[s['nfev'] for s in want]}), "
          f"nlaunch {res.nlaunch}")
    # the host-callable path: plain numpy callables
    lp_g_np = lambda X: lref.score_and_lp(A, y, counts, lam, X)[0]                # noqa: E731
    lp_np = lambda X: lref.score_and_lp(A, y, counts, lam, np.asarray(X))[1]      # noqa: E731
    mean2, cov2, res2 = gsmvi_amd.lbfgs_init_batched(x0, lp_np, lp_g_np, ftol=0.0)
    _check_bound(mean2, res2, inputs, D)
    # the default tolerances: the bound of the run's own final gradient
    mean3, _, res3 = gsmvi_amd.lbfgs_init_batched(x0, tgt.lp, tgt.lp_g)
    _check_bound(mean3, res3, inputs, D, gmax=np.abs(res3.jac).max(1))


@pytest.mark.parametrize("N,D", ref.LOGISTIC_SHAPES)
def test_it_initialises_the_batched_fits(N, D):
    import gsmvi_amd
    tgt, inputs = _target(N, D)
    K = inputs[0].shape[0]
    mean, cov, res = gsmvi_amd.lbfgs_init_batched(np.zeros((K, D)), tgt.lp, tgt.lp_g)
    keys = np.arange(K) + 7
    mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=16, checkpoint=10, offset_evals=res.nlaunch)
    m1, c1 = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, mean=mean, cov=cov, batch_size=2, niter=20, verbose=False,
                                                          monitor=mon)
    assert mon.nevals[0] == res.nlaunch + 1 and len(mon.rkl) == 4 and np.isfinite(m1).all() and np.isfinite(c1).all()
    mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=16, checkpoint=10, offset_evals=res.nlaunch)
    m2, c2, _ = gsmvi_amd.ADVIBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, gsmvi_amd.Adam(1e-2), mean=mean, cov=cov, batch_size=2,
                                                               niter=20, monitor=mon, verbose=False)
    assert mon.nevals[0] == res.nlaunch + 1 and np.isfinite(m2).all() and np.isfinite(c2).all()


# ---- isolation and determinism -------------------------------------------------------------------------------------------------
def _run(tgt, x0, **kw):
    import gsmvi_amd
    mean, cov, res = gsmvi_amd.lbfgs_init_batched(x0, tgt.lp, tgt.lp_g, **kw)
    return mean, cov, res


def _same(a, b, ka, kb):
    """problem ka of run a and problem kb of run b: the same bits"""
    return (np.array_equal(a[0][ka], b[0][kb], equal_nan=True) and np.array_equal(a[1][ka], b[1][kb])
            and all(np.array_equal(getattr(a[2], f)[ka], getattr(b[2], f)[kb], equal_nan=True)
                    for f in ("x", "fun", "jac", "nit", "nfev", "status")))


@pytest.mark.parametrize("N,D", [(200, 10), (257, 33)])
def test_a_problem_alone_among_16_and_among_1024(N, D):
    import gsmvi_amd
    A, y, counts, lam, _ = lref.make_inputs(16, N, D, 1)
    j = 5
    x0 = 0.1 * np.random.RandomState(D).standard_normal((16, D))
    mk = lambda sel: gsmvi_amd.BatchedLogisticTarget(A[sel], y[sel], prior_precision=lam[sel], counts=counts[sel])   # noqa: E731
    among16 = _run(mk(np.arange(16)), x0)
    alone = _run(mk(np.array([j])), x0[j:j + 1])
    sel = np.tile(np.arange(16), 64)
    among1024 = _run(mk(sel), x0[sel])
    assert among16[2].status[j] == 1
    assert _same(alone, among16, 0, j)
    for k in (j, 16 + j, 1024 - 16 + j):
        assert _same(among1024, among16, k, j), k


@pytest.mark.parametrize("N,D", [(200, 10), (257, 33)])
def test_a_failing_problem_leaves_its_neighbours_alone(N, D):
    import gsmvi_amd
    tgt, inputs = _target(N, D, K=16)
    x0 = np.zeros((16, D))
    clean = _run(tgt, x0)
    # lp of problem j turns NaN from its fourth evaluation on: 21 rejected trials, then status 3
    j, calls = 5, [0]

    def lp_bad(X):
        v = tgt.lp(X).clone()
        calls[0] += 1
        if calls[0] > 3:
            v[j] = float("nan")
        return v
    mean, cov, res = gsmvi_amd.lbfgs_init_batched(x0, lp_bad, tgt.lp_g)
    assert res.status[j] == 3 and not res.success[j] and 3 + 20 <= res.nfev[j] <= 3 + 21 and np.isfinite(mean[j]).all()
    assert np.array_equal(cov[j], cov[j].T)
    for k in range(16):
        if k != j:
            assert _same((mean, cov, res), clean, k, k), k
    # a NaN start: status 4, mean = x0, cov = I; nobody else notices
    x0n = x0.copy()
    x0n[j] = np.nan
    mean, cov, res = _run(tgt, x0n)
    assert res.status[j] == 4 and res.nfev[j] == 1 and res.nit[j] == 0
    assert np.isnan(mean[j]).all() and np.array_equal(cov[j], np.eye(D))
    for k in range(16):
        if k != j:
            assert _same((mean, cov, res), clean, k, k), k


def test_stopped_problems_keep_every_bit_over_further_launches():
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    for D in (10, 33):
        states = [ref.run(fun, x0, **opt) for _, fun, x0, opt in ref.gpu_cases(D)]
        assert {s["status"] for s in states} == {1, 2, 3, 4}
        before = ref.pack(states)
        st = _upload(eng, before)
        rs = np.random.RandomState(D)
        for _ in range(16):
            eng.lbfgs_step_batched(eng.asarray(rs.standard_normal(len(states))), eng.asarray(rs.standard_normal((len(states), D))),
                                   st, sign=1.0)
        got = _download(st)
        for name in VECS + ("sc", "ist"):
            assert np.array_equal(got[name], before[name], equal_nan=True), (D, name)
        assert int(st["stopped"].item()) == 0


def test_check_every_does_not_change_the_result_and_runs_are_identical():
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    tgt, inputs = _target(200, 10, K=16)
    x0 = 0.1 * np.random.RandomState(3).standard_normal((16, 10))
    keep = x0.copy()
    A0, y0 = tgt.A.clone(), tgt.y.clone()
    eng.last_path(reset=True)
    runs = {c: _run(tgt, x0, check_every=c) for c in (1, 8, 1000)}
    path = eng.last_path(reset=True)
    assert "batched_lbfgs" in path and not any(p.endswith("_generic") for p in path), path
    assert np.array_equal(x0, keep) and torch.equal(tgt.A, A0) and torch.equal(tgt.y, y0)
    for c in (1, 1000):
        for k in range(16):
            assert _same(runs[c], runs[8], k, k), (c, k)
    assert runs[1][2].nlaunch == runs[1][2].nfev.max() and runs[1000][2].nlaunch == 1000
    assert runs[8][2].nlaunch == 8 * -(-int(runs[8][2].nfev.max()) // 8)
    again = _run(tgt, x0)
    for k in range(16):
        assert _same(again, runs[8], k, k), k
    # device tensors out, and a (D,) start for every problem of the target
    mt, ct, res = _run(tgt, x0, as_torch=True)
    assert mt.is_cuda and ct.is_cuda and np.array_equal(mt.cpu().numpy(), runs[8][0]) and np.array_equal(ct.cpu().numpy(), runs[8][1])
    one = _run(tgt, np.zeros(10))
    assert one[0].shape == (16, 10) and _same(one, _run(tgt, np.zeros((16, 10))), 3, 3)
