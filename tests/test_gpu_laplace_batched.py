"""The batched Laplace initialiser on the GPU (csrc/gsmvi_laplace_batched.hip): the fp64-MFMA Hessian and its inverse against
the numpy restatement (tests/laplace_batched_ref.py), every step of the restatement's trajectories through the C ABI from
uploaded states, frozen problems, ``laplace_init_batched`` end to end and as the start of the batched fits, the independence of
the problems bit for bit, and the argument checks."""
import numpy as np
import pytest
import torch

import glm_batched_ref as gref
import laplace_batched_ref as ref

pytestmark = pytest.mark.gpu

CASES = [(f, s) for f in ref.FAMILIES for s in ref.SHAPES]


def _target(family, inp, with_offset=True, sel=None):
    import gsmvi_amd
    A, y, o, counts, lam, tau = inp[:6]
    sel = np.arange(A.shape[0]) if sel is None else np.asarray(sel)
    tau_s = tau[sel] if isinstance(tau, np.ndarray) else tau
    return gsmvi_amd.BatchedGLMTarget(A[sel], y[sel], family, prior_precision=lam[sel], counts=counts[sel],
                                      offset=o[sel] if with_offset else None, noise_precision=tau_s)


def _model(tgt):
    return dict(offset=tgt.offset, counts=tgt.counts, prior_prec=tgt.prior_precision, noise_prec=tgt.noise_precision)


def _hess(tgt, X, want="both"):
    eng = tgt.engine
    out = eng.glm_hessian_batched(eng.asarray(X), tgt.A, tgt.y, tgt.family, want=want, **_model(tgt))
    return tuple(t.cpu().numpy() for t in out) if isinstance(out, tuple) else out.cpu().numpy()


def _points(family, inp):
    """one point per problem, |eta| of order one (make_inputs' X with its poisson cap, halved)"""
    return 0.5 * inp[6][:, 0, :]


# ---- 1. the Hessian ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", CASES)
def test_hessian_matches_the_restatement(family, shape):
    """1e-11 of max|H| per problem, with and without an offset; exactly symmetric; inputs unchanged"""
    inp = gref.make_inputs(family, *shape, 1)
    A, y, o, counts, lam, tau, _ = inp
    X = _points(family, inp)
    worst = 0.0
    for off in (True, False):
        tgt = _target(family, inp, off)
        keep = [t.clone() for t in (tgt.A, tgt.y)] + ([tgt.offset.clone()] if off else [])
        eng = tgt.engine
        Xd = eng.asarray(X)
        eng.last_path(reset=True)
        H = tgt.neg_hessian(Xd).cpu().numpy()
        assert eng.last_path(reset=True) == {"batched_laplace"}
        assert np.array_equal(Xd.cpu().numpy(), X)
        for t, k in zip([tgt.A, tgt.y] + ([tgt.offset] if off else []), keep):
            assert torch.equal(t, k)
        want = ref.neg_hessian(family, A, y, o if off else None, counts, lam, tau, X)
        for k in range(shape[0]):
            assert np.array_equal(H[k], H[k].T), (off, k)
            e = np.abs(H[k] - want[k]).max() / np.abs(want[k]).max()
            worst = max(worst, e)
            assert e <= 1e-11, (off, k, e)
        assert np.array_equal(tgt.neg_hessian(X).cpu().numpy(), H)      # numpy in
    print(f"{family} {shape}: worst error {worst:.2e} of max|H|")


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("N,D", [(70, 10), (70, 33)])
def test_a_problem_alone_among_16_and_among_1024(family, N, D):
    inp = gref.make_inputs(family, 16, N, D, 1)
    X = _points(family, inp)
    j = 5
    among16 = _hess(_target(family, inp), X)
    alone = _hess(_target(family, inp, sel=[j]), X[j:j + 1])
    sel = np.tile(np.arange(16), 64)
    among1024 = _hess(_target(family, inp, sel=sel), X[sel])
    assert among16[2][j] == 0 and np.isfinite(among16[0][j]).all()
    for a, b, c in zip(alone, among16, among1024):
        assert np.array_equal(a[0], b[j])
        for k in (j, 16 + j, 1024 - 16 + j):
            assert np.array_equal(c[k], b[j]), k


def test_the_two_target_classes_agree_bitwise():
    import gsmvi_amd
    for shape in ((5, 40, 3), (5, 70, 33)):
        A, y, o, counts, lam, tau, X = gref.make_inputs("logistic", *shape, 1)
        t1 = gsmvi_amd.BatchedLogisticTarget(A, y, prior_precision=lam, counts=counts)
        t2 = gsmvi_amd.BatchedGLMTarget(A, y, "logistic", prior_precision=lam, counts=counts)
        H1, H2 = t1.neg_hessian(X[:, 0, :]), t2.neg_hessian(X[:, 0, :])
        assert isinstance(H1, torch.Tensor) and H1.is_cuda and torch.equal(H1, H2)
        t3 = gsmvi_amd.BatchedLogisticTarget(A, y, prior_precision=0.7)          # scalar prior, no counts
        assert np.abs(t3.neg_hessian(X[:, 0, :]).cpu().numpy() -
                      ref.neg_hessian("logistic", A, y, None, None, 0.7, 1.0, X[:, 0, :])).max() <= 1e-11 * shape[1]


# ---- 2. the inverse ----------------------------------------------------------------------------------------------------------
def _check_inverse(cov, H_ref, where):
    """max|cov H_ref - I| <= 1e-11 cond_2(H_ref); returns the share of the bound used"""
    D = H_ref.shape[0]
    bound = 1e-11 * np.linalg.cond(H_ref)
    e = np.abs(cov @ H_ref - np.eye(D)).max()
    assert e <= bound, (where, e, bound)
    assert np.array_equal(cov, cov.T), where
    return e / bound


@pytest.mark.parametrize("family,shape", CASES)
def test_inverse_of_the_hessian(family, shape):
    inp = gref.make_inputs(family, *shape, 1)
    A, y, o, counts, lam, tau, _ = inp
    X = _points(family, inp)
    worst, cmax = 0.0, 0.0
    for off in (True, False):
        H, cov, info = _hess(_target(family, inp, off), X)
        cov_only, info_only = _hess(_target(family, inp, off), X, want="cov")
        assert np.array_equal(cov, cov_only) and np.array_equal(info, info_only)
        want = ref.neg_hessian(family, A, y, o if off else None, counts, lam, tau, X)
        for k in range(1, shape[0]):                                    # lam_k > 0
            assert info[k] == 0, (off, k, info[k])
            cmax = max(cmax, np.linalg.cond(want[k]))
            worst = max(worst, _check_inverse(cov[k], want[k], (off, k)))
        assert np.array_equal(cov[0], cov[0].T)
    print(f"{family} {shape}: worst share of 1e-11 cond used {worst:.3f}, largest cond {cmax:.1f}")


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_failing_problems_are_flagged_and_leave_their_neighbours_alone(family):
    """counts = 0 with lam = 0 is H = 0 exactly; (N, D) = (9, 16) problem 0 is rank 9 with a flat prior; a NaN in one x_k"""
    inp = list(gref.make_inputs(family, 6, 9, 16, 1))
    A, y, o, counts, lam, tau, _ = inp
    X = _points(family, inp)
    counts, lam = counts.copy(), lam.copy()
    counts[3], lam[3] = 0, 0.0
    bad = inp[:3] + [counts, lam] + inp[5:]
    H, cov, info = _hess(_target(family, bad), X)
    assert info[0] != 0 and np.array_equal(cov[0], np.eye(16)) and np.isfinite(H[0]).all()
    assert info[3] == 1 and np.array_equal(cov[3], np.eye(16)) and not H[3].any()
    ok = [1, 2, 4, 5]
    assert (info[ok] == 0).all()
    good = inp[:3] + [inp[3], np.where(np.arange(6) == 0, 1.0, inp[4])] + inp[5:]     # the same batch without the two failures
    H2, cov2, info2 = _hess(_target(family, good), X)
    assert (info2 == 0).all()
    for k in ok:
        assert np.array_equal(H[k], H2[k]) and np.array_equal(cov[k], cov2[k]), k
    Xn = X.copy()
    Xn[2, 7] = np.nan
    H3, cov3, info3 = _hess(_target(family, good), Xn)
    assert np.isnan(H3[2]).all() and info3[2] == 1 and np.array_equal(cov3[2], np.eye(16))
    for k in (0, 1, 3, 4, 5):
        assert np.array_equal(H3[k], H2[k]) and np.array_equal(cov3[k], cov2[k]) and info3[k] == 0, k
    if family == "poisson":                                             # a valid row whose exp(eta) overflows flags its problem
        Xb = X.copy()
        Xb[4] = 4000.0 * np.sign(A[4, 0])
        H4, cov4, info4 = _hess(_target(family, good), Xb)
        assert np.isnan(H4[4]).all() and info4[4] == 1 and np.array_equal(cov4[4], np.eye(16))
        for k in (0, 1, 2, 3, 5):
            assert np.array_equal(H4[k], H2[k]) and np.array_equal(cov4[k], cov2[k]), k


# ---- 3. every step of every trajectory ---------------------------------------------------------------------------------------
def _upload(eng, packed):
    st = {k: eng.asarray(v).contiguous() for k, v in packed.items() if k != "ist"}
    st["ist"] = torch.as_tensor(packed["ist"], device=st["x"].device).contiguous()
    st["stopped"] = eng.new_flag()
    return st


def _download(st):
    return {k: v.cpu().numpy() for k, v in st.items()}


def _compare(got, recs, where):
    """integers equal, t equal, every other double within 1e-11 of its scale (zero where the launch writes nothing: the
    uploaded bits must come back); returns the largest share of a bound used"""
    want = ref.pack([a for _, a, _ in recs])
    assert np.array_equal(got["ist"], want["ist"]), (where, got["ist"][:, :4].tolist(), want["ist"][:, :4].tolist())
    worst = 0.0

    def close(name, k, a, b, scale):
        nonlocal worst
        a, b = np.atleast_1d(a), np.atleast_1d(b)
        assert np.array_equal(np.isfinite(a), np.isfinite(b)), (where, k, name)
        fin = np.isfinite(b)
        err, bound = np.abs(a - b)[fin], (1e-11 * np.broadcast_to(scale, np.shape(b)))[fin]
        assert (err <= bound).all(), (where, k, name, err.max(), bound.min())
        if err.size and bound.min() > 0:
            worst = max(worst, float((err / bound).max()))

    for k, (before, after, notes) in enumerate(recs):
        sd = notes.get("scale_d", 0.0)
        close("x", k, got["x"][k], want["x"][k], 0.0)                   # a copy of the uploaded trial point
        close("g", k, got["g"][k], want["g"][k], notes.get("scale_g", 0.0))
        close("d", k, got["d"][k], want["d"][k], sd)
        moved = not np.array_equal(before["Xt"], after["Xt"])
        close("Xt", k, got["Xt"][k], want["Xt"][k], (np.abs(after["x"]).max() + sd + np.abs(after["d"]).max()) if moved else 0.0)
        close("f", k, got["sc"][k, 0], want["sc"][k, 0], notes.get("scale_f", 0.0))
        close("t", k, got["sc"][k, 1], want["sc"][k, 1], 0.0)
        close("gd", k, got["sc"][k, 2], want["sc"][k, 2], notes.get("scale_gd", 0.0))
        assert got["sc"][k, 3] == 0.0
    return worst


@pytest.mark.parametrize("family,shape", CASES)
def test_every_step_of_every_trajectory_matches_the_restatement(family, shape):
    """each round of each problem's trajectory (gtol = 1e-6; margins asserted in tests/test_laplace_batched_cpu.py) is one
    problem of a launch: the restatement's state before it goes up, everything the launch leaves is compared with the
    restatement's state after it; every trajectory's stopped end state rides along and must come back bit for bit"""
    inp = ref.inputs(family, shape)
    eng, worst, nsteps = None, 0.0, 0
    opt = dict(maxiter=30, maxfun=60, gtol=ref.STEP_GTOL)
    for off in (True, False):
        traj = ref.trajectories(family, shape, off)
        # the first launch
        tgt = _target(family, inp, off)
        eng = tgt.engine
        st = eng.laplace_state_batched(eng.asarray(np.zeros((shape[0], shape[2]))))
        eng.last_path(reset=True)
        eng.laplace_step_batched(st, tgt.A, tgt.y, family, start=True, **opt, **_model(tgt))
        assert eng.last_path(reset=True) == {"batched_laplace"}
        first = [rec[0] for _, _, rec in traj]
        worst = max(worst, _compare(_download(st), first, (off, "start")))
        assert int(st["stopped"].item()) == sum(a["status"] != 0 for _, a, _ in first)
        # every later launch, and the frozen end states
        recs, ks = [], []
        for k, end, rec in traj:
            recs += rec[1:] + [(end, end, {})]
            ks += [k] * len(rec)
        tgt = _target(family, inp, off, sel=ks)
        before = ref.pack([b for b, _, _ in recs])
        st = _upload(eng, before)
        keepA = tgt.A.clone()
        eng.laplace_step_batched(st, tgt.A, tgt.y, family, **opt, **_model(tgt))
        got = _download(st)
        worst = max(worst, _compare(got, recs, (off, "step")))
        nsteps += len(recs)
        assert int(st["stopped"].item()) == sum(a["status"] != 0 and b["status"] == 0 for b, a, _ in recs)
        assert torch.equal(tgt.A, keepA)
        frozen = before["ist"][:, 0] != 0
        assert frozen.sum() == len(traj)
        for name in ("x", "g", "d", "Xt", "sc", "ist"):
            assert np.array_equal(got[name][frozen], before[name][frozen], equal_nan=True), name
    print(f"{family} {shape}: {nsteps} steps, worst share of 1e-11 scale used {worst:.3f}")


# ---- 4. frozen problems --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(6, 70, 10), (5, 70, 33)])
def test_stopped_problems_keep_every_bit_and_are_counted_once(shape):
    family = "poisson"
    inp = ref.inputs(family, shape)
    tgt = _target(family, inp)
    eng = tgt.engine
    K, D = shape[0], shape[2]
    st = eng.laplace_state_batched(eng.asarray(np.zeros((K, D))))
    opt = dict(maxiter=30, maxfun=60, gtol=ref.STEP_GTOL)
    want = [end for _, end, _ in ref.trajectories(family, shape, True)]
    rounds = max(e["nfev"] for e in want)
    for r in range(rounds):
        eng.laplace_step_batched(st, tgt.A, tgt.y, family, start=r == 0, **opt, **_model(tgt))
    assert int(st["stopped"].item()) == K
    done = _download(st)
    assert np.array_equal(done["ist"], ref.pack(want)["ist"])
    for _ in range(5):                                                  # everything is frozen: whole workgroups leave at once
        eng.laplace_step_batched(st, tgt.A, tgt.y, family, **opt, **_model(tgt))
    again = _download(st)
    for name in ("x", "g", "d", "Xt", "sc", "ist", "stopped"):
        assert np.array_equal(again[name], done[name], equal_nan=True), name
    # made-up stopped states of every code among running ones
    states = [dict(e) for e in want]
    for k, code in zip(range(1, K), (2, 3, 4, 5, 1)):
        states[k]["status"] = code
    states[0] = ref.trajectories(family, shape, True)[0][2][1][0]       # problem 0 before its second launch: running
    before = ref.pack(states)
    st = _upload(eng, before)
    eng.laplace_step_batched(st, tgt.A, tgt.y, family, **opt, **_model(tgt))
    got = _download(st)
    for name in ("x", "g", "d", "Xt", "sc", "ist"):
        assert np.array_equal(got[name][1:], before[name][1:], equal_nan=True), name
    assert got["ist"][0, 2] == before["ist"][0, 2] + 1 and int(st["stopped"].item()) == int(got["ist"][0, 0] != 0)


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", CASES)
def test_end_to_end_at_the_defaults(family, shape):
    """every problem with a proper prior (and the flat-prior problem 0 at the two smallest shapes) converges; the existing score
    kernel, an independent path, confirms the gradient; the mean is within 2 sqrt(D) gtol / lam_k of the restatement's (each is
    within sqrt(D) gtol / lam_k of the mode: -grad^2 lp >= lam I); the covariance inverts the restated Hessian"""
    import gsmvi_amd
    K, N, D = shape
    inp = gref.make_inputs(family, K, N, D, 1)
    A, y, o, counts, lam, tau, _ = inp
    gtol = 1e-8
    first = 0 if (N, D) in ((40, 3), (70, 10)) else 1
    for off in (True, False):
        tgt = _target(family, inp, off)
        mean, cov, res = gsmvi_amd.laplace_init_batched(tgt)
        assert mean.shape == (K, D) and cov.shape == (K, D, D) and np.array_equal(mean, res.x) and res.nlaunch % 4 == 0
        G = -tgt.lp_g(tgt.engine.asarray(mean[:, None, :])).cpu().numpy()[:, 0, :]
        Href = ref.neg_hessian(family, A, y, o if off else None, counts, lam, tau, mean)
        want = []
        for k in range(first, K):
            assert res.status[k] == 1 and res.success[k] and res.info[k] == 0, (off, k, res.status[k], res.info[k])
            p = ref.problem(family, A, y, o if off else None, counts, lam, tau, k)
            scale = ref.evaluate(p, mean[k])[3]["g"]
            assert (np.abs(G[k]) <= gtol + 1e-11 * scale).all(), (off, k, np.abs(G[k]).max())
            assert np.abs(res.jac[k]).max() <= gtol
            s = ref.run(p, np.zeros(D))
            want.append(s)
            if lam[k] > 0:
                dist, bound = np.linalg.norm(mean[k] - s["x"]), 2 * np.sqrt(D) * gtol / lam[k]
                assert dist <= bound, (off, k, dist, bound)
            _check_inverse(cov[k], Href[k], (off, k))
            assert res.nit[k] <= 10 and res.nfev[k] <= 12, (off, k, res.nit[k], res.nfev[k])
        print(f"{family} {shape} offset={off}: nit {res.nit[first:].tolist()} (restatement {[s['nit'] for s in want]}), nfev "
              f"{res.nfev[first:].tolist()} (restatement {[s['nfev'] for s in want]}), nlaunch {res.nlaunch}")


def test_check_every_does_not_change_the_result_and_failures_get_the_identity():
    import gsmvi_amd
    family, shape = "probit", (6, 70, 10)
    inp = gref.make_inputs(family, *shape, 1)
    tgt = _target(family, inp)
    x0 = 0.1 * np.random.RandomState(3).standard_normal((6, 10))
    runs = {c: gsmvi_amd.laplace_init_batched(tgt, x0, check_every=c) for c in (1, 4, 1000)}
    for c in (1, 1000):
        assert np.array_equal(runs[c][0], runs[4][0]) and np.array_equal(runs[c][1], runs[4][1])
        for f in ("x", "fun", "jac", "nit", "nfev", "status", "info"):
            assert np.array_equal(getattr(runs[c][2], f), getattr(runs[4][2], f)), (c, f)
    assert runs[1][2].nlaunch == runs[1][2].nfev.max() and runs[1000][2].nlaunch == 200
    mt, ct, _ = gsmvi_amd.laplace_init_batched(tgt, x0, as_torch=True)
    assert mt.is_cuda and ct.is_cuda and np.array_equal(mt.cpu().numpy(), runs[4][0]) and np.array_equal(ct.cpu().numpy(), runs[4][1])
    one = gsmvi_amd.laplace_init_batched(tgt, x0[2])
    assert np.array_equal(one[0][2], runs[4][0][2]) and np.array_equal(one[1][2], runs[4][1][2])
    mean, cov, res = gsmvi_amd.laplace_init_batched(tgt, x0, maxiter=1)
    assert (res.status == 2).all() and not res.success.any() and np.array_equal(cov, np.broadcast_to(np.eye(10), (6, 10, 10)))
    with pytest.raises(TypeError, match="BatchedGLMTarget or a BatchedLogisticTarget"):
        gsmvi_amd.laplace_init_batched(gsmvi_amd.BatchedGaussianTarget(np.zeros((2, 3)), cov=np.stack([np.eye(3)] * 2)))


# ---- 6. as a start ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B", [(5, 2), (17, 4)])
def test_it_initialises_the_batched_fits(D, B):
    import gsmvi_amd
    K, N = 6, 8 * D
    A, y, o, counts, lam, tau, _ = gref.make_inputs("logistic", K, N, D, 1)
    lam[0] = 0.5
    tgt = gsmvi_amd.BatchedLogisticTarget(A, y, prior_precision=lam, counts=counts)
    mean, cov, res = gsmvi_amd.laplace_init_batched(tgt)
    assert res.success.all()
    keys = np.arange(K) + 7
    mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=16, checkpoint=10, offset_evals=res.nlaunch)
    m1, c1 = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, mean=mean, cov=cov, batch_size=B, niter=50, verbose=False,
                                                          monitor=mon)
    assert mon.nevals[0] == res.nlaunch + 1 and np.isfinite(m1).all() and np.isfinite(c1).all()
    mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=16, checkpoint=10, offset_evals=res.nlaunch)
    m2, c2 = gsmvi_amd.BaMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, lambda i: 100 / (1 + i), mean=mean, cov=cov, batch_size=B,
                                                          niter=50, verbose=False, monitor=mon)
    assert mon.nevals[0] == res.nlaunch + 1 and np.isfinite(m2).all() and np.isfinite(c2).all()


# ---- 7. bad arguments --------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_with_nothing_enqueued():
    import gsmvi_amd
    from gsmvi_amd import _lib
    eng = gsmvi_amd.get_engine()
    eng.last_path(reset=True)
    ref.check_bad_arguments(_lib.load_library())
    assert eng.last_path(reset=True) == set()
