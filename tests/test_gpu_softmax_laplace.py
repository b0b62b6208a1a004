"""The batched softmax Laplace initialiser on the GPU (csrc/gsmvi_softmax_laplace_batched.hip): the class-coupled fp64-MFMA
Hessian and its inverse against the numpy restatement (tests/softmax_laplace_ref.py), saturated inputs included; every step of the
restatement's trajectories through the C ABI from uploaded states; frozen and failing problems; ``laplace_init_softmax_batched``
end to end and as the start of the batched fits; the independence of the problems bit for bit; the argument checks."""
import numpy as np
import pytest
import torch

import laplace_batched_ref as lref
import softmax_laplace_ref as ref

pytestmark = pytest.mark.gpu

BAR = 1e-11
OPT = dict(maxiter=30, maxfun=60, gtol=ref.STEP_GTOL)


def _target(shape, inp, sel=None):
    import gsmvi_amd
    A, y, counts, lam = inp[:4]
    sel = np.arange(A.shape[0]) if sel is None else np.asarray(sel)
    return gsmvi_amd.BatchedSoftmaxTarget(A[sel], y[sel], shape[2], prior_precision=lam[sel], counts=counts[sel])


def _model(tgt):
    return dict(counts=tgt.counts, prior_prec=tgt.prior_precision)


def _hess(tgt, X, want="both"):
    eng = tgt.engine
    out = eng.softmax_hessian_batched(eng.asarray(X), tgt.A, tgt.y, tgt.C, want=want, **_model(tgt))
    return tuple(t.cpu().numpy() for t in out) if isinstance(out, tuple) else out.cpu().numpy()


def _step(tgt, st, **kw):
    tgt.engine.softmax_laplace_step_batched(st, tgt.A, tgt.y, tgt.C, **kw, **_model(tgt))


def _within(H, want, scale):
    """the largest |H - want| in units of BAR times the entry's scale (an entry of scale 0 must be exact)"""
    err = np.abs(H - want)
    assert (err[scale == 0] == 0).all()
    pos = scale > 0
    return float((err[pos] / (BAR * scale[pos])).max()) if pos.any() else 0.0


# ---- 1. the Hessian ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_hessian_matches_the_restatement(shape):
    """1e-11 of the entry's scale sum_n |w| |a_i| |a_j| + lam; exactly symmetric; inputs unchanged; ragged counts with an empty
    problem, per-problem lam with a flat prior"""
    K, N, Cc, P = shape
    inp = ref.inputs(shape)
    A, y, counts, lam, X = inp
    tgt = _target(shape, inp)
    eng = tgt.engine
    keep = [tgt.A.clone(), tgt.y.clone(), tgt.counts.clone()]
    Xd = eng.asarray(X)
    eng.last_path(reset=True)
    H = tgt.neg_hessian(Xd).cpu().numpy()
    assert eng.last_path(reset=True) == {"batched_softmax_laplace"}
    assert np.array_equal(Xd.cpu().numpy(), X)
    for t, k in zip([tgt.A, tgt.y, tgt.counts], keep):
        assert torch.equal(t, k)
    worst = 0.0
    for k in range(K):
        _, _, want, sc = ref.evaluate(ref.problem(A, y, Cc, counts, lam, k), X[k])
        assert np.array_equal(H[k], H[k].T), k
        used = _within(H[k], want, sc["H"])
        worst = max(worst, used)
        assert used <= 1.0, (k, used)
    assert np.array_equal(tgt.neg_hessian(X).cpu().numpy(), H)          # numpy in
    print(f"{shape}: worst share of 1e-11 of the scale used {worst:.2e}")


@pytest.mark.parametrize("N,Cc,P", [(70, 3, 5), (65, 5, 4), (40, 9, 8)])
def test_hessian_of_saturated_inputs(N, Cc, P):
    """W_00 = 25, 27.5, 30 with an intercept column and lam = 0: one class takes nearly all of the probability, and the diagonal
    class blocks keep their digits only if 1 - p is a sum over the other classes"""
    import gsmvi_amd
    ps = [ref.saturated_inputs(N, Cc, P, top) for top in (25.0, 27.5, 30.0)]
    A, y, X = np.stack([p["A"] for p, _ in ps]), np.stack([p["y"] for p, _ in ps]), np.stack([x for _, x in ps])
    tgt = gsmvi_amd.BatchedSoftmaxTarget(A, y, Cc, prior_precision=0.0)
    H = tgt.neg_hessian(X).cpu().numpy()
    worst = 0.0
    for k, (p, x) in enumerate(ps):
        _, _, want, sc = ref.evaluate(p, x)
        _, _, exact, _ = ref.evaluate(p, x.astype(np.longdouble))
        used = max(_within(H[k], want, sc["H"]), _within(H[k], exact.astype(np.float64), sc["H"]))
        worst = max(worst, used)
        assert used <= 1.0 and np.array_equal(H[k], H[k].T), (k, used)
    print(f"({N}, {Cc}, {P}): worst share of 1e-11 of the scale used {worst:.2e} (restatement and longdouble)")


def test_two_classes_agree_with_the_logistic_hessian():
    import gsmvi_amd
    for shape in ((5, 33, 2, 16), (4, 150, 2, 64)):
        K, N, _, D = shape
        A, y, counts, lam, X = ref.inputs(shape)
        t1 = gsmvi_amd.BatchedSoftmaxTarget(A, y, 2, prior_precision=lam, counts=counts)
        t2 = gsmvi_amd.BatchedLogisticTarget(A, (y == 0).astype(np.float64), prior_precision=lam, counts=counts)
        H1, H2 = t1.neg_hessian(X).cpu().numpy(), t2.neg_hessian(X).cpu().numpy()
        for k in range(K):
            sc = ref.evaluate(ref.problem(A, y, 2, counts, lam, k), X[k])[3]["H"]
            assert _within(H1[k], H2[k], sc) <= 1.0, (shape, k)


# ---- 2. the inverse ----------------------------------------------------------------------------------------------------------
def _check_inverse(cov, H_ref, where):
    """max|cov H_ref - I| <= 1e-11 cond_2(H_ref); returns the share of the bound used"""
    D = H_ref.shape[0]
    bound = 1e-11 * np.linalg.cond(H_ref)
    e = np.abs(cov @ H_ref - np.eye(D)).max()
    assert e <= bound, (where, e, bound)
    assert np.array_equal(cov, cov.T), where
    return e / bound


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_inverse_of_the_hessian(shape):
    inp = ref.inputs(shape)
    A, y, counts, lam, X = inp
    tgt = _target(shape, inp)
    H, cov, info = _hess(tgt, X)
    cov_only, info_only = _hess(tgt, X, want="cov")
    assert np.array_equal(cov, cov_only) and np.array_equal(info, info_only)
    assert np.array_equal(H, _hess(tgt, X, want="h"))
    want = ref.neg_hessian(A, y, shape[2], counts, lam, X)
    worst, cmax = 0.0, 0.0
    for k in range(1, shape[0]):                                        # lam_k > 0
        assert info[k] == 0, (k, info[k])
        cmax = max(cmax, np.linalg.cond(want[k]))
        worst = max(worst, _check_inverse(cov[k], want[k], k))
    assert np.array_equal(cov[0], cov[0].T)
    print(f"{shape}: worst share of 1e-11 cond used {worst:.2e}, largest cond {cmax:.1f}")


# ---- 3. a problem alone, among 16 and among 1024 -----------------------------------------------------------------------------
@pytest.mark.parametrize("N,Cc,P", [(70, 3, 5), (70, 4, 11)])
def test_a_problem_alone_among_16_and_among_1024(N, Cc, P):
    """H, cov, info and the state after the first two rounds: the same bits in the three settings, in both packings"""
    shape = (16, N, Cc, P)
    inp = ref.inputs(shape)
    X = inp[4]
    j = 5
    sel = np.tile(np.arange(16), 64)

    def everything(sel_, pick):
        tgt = _target(shape, inp, sel=sel_)
        Xs = X if sel_ is None else X[np.asarray(sel_)]
        out = list(_hess(tgt, Xs))
        st = tgt.engine.laplace_state_batched(tgt.engine.asarray(Xs))
        for r in range(2):
            _step(tgt, st, start=r == 0, **OPT)
        out += [st[name].cpu().numpy() for name in ("x", "g", "d", "Xt", "sc", "ist")]
        return [[a[k] for k in pick] for a in out]

    among16 = everything(None, [j])
    alone = everything([j], [0])
    among1024 = everything(sel, [j, 16 + j, 1024 - 16 + j])
    assert among16[2][0] == 0 and np.isfinite(among16[0][0]).all() and among16[8][0][2] == 2
    for a, b, c in zip(alone, among16, among1024):
        assert np.array_equal(a[0], b[0])
        for v in c:
            assert np.array_equal(v, b[0])


# ---- 4. every step of every trajectory ---------------------------------------------------------------------------------------
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
    want = lref.pack([a for _, a, _ in recs])
    assert np.array_equal(got["ist"], want["ist"]), (where, got["ist"][:, :4].tolist(), want["ist"][:, :4].tolist())
    worst = 0.0

    def close(name, k, a, b, scale):
        nonlocal worst
        a, b = np.atleast_1d(a), np.atleast_1d(b)
        assert np.array_equal(np.isfinite(a), np.isfinite(b)), (where, k, name)
        fin = np.isfinite(b)
        err, bound = np.abs(a - b)[fin], (BAR * np.broadcast_to(scale, np.shape(b)))[fin]
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


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_every_step_of_every_trajectory_matches_the_restatement(shape):
    """each round of each problem's trajectory (maxiter = 30, maxfun = 60, gtol = 1e-6; margins asserted in
    tests/test_softmax_laplace_cpu.py) is one problem of a launch: the restatement's state before it goes up, everything the
    launch leaves is compared with the restatement's state after it; every trajectory's stopped end state rides along and must
    come back bit for bit"""
    K, N, Cc, P = shape
    inp = ref.inputs(shape, flat0=False)
    traj = ref.trajectories(shape)
    tgt = _target(shape, inp)
    eng = tgt.engine
    st = eng.laplace_state_batched(eng.asarray(np.zeros((K, (Cc - 1) * P))))
    eng.last_path(reset=True)
    _step(tgt, st, start=True, **OPT)
    assert eng.last_path(reset=True) == {"batched_softmax_laplace"}
    first = [rec[0] for _, _, rec in traj]
    worst = _compare(_download(st), first, "start")
    assert int(st["stopped"].item()) == sum(a["status"] != 0 for _, a, _ in first) >= 1      # (the empty problem stops at once)
    recs, ks = [], []
    for k, end, rec in traj:
        recs += rec[1:] + [(end, end, {})]
        ks += [k] * len(rec)
    tgt = _target(shape, inp, sel=ks)
    before = lref.pack([b for b, _, _ in recs])
    st = _upload(eng, before)
    keepA = tgt.A.clone()
    _step(tgt, st, **OPT)
    got = _download(st)
    worst = max(worst, _compare(got, recs, "step"))
    assert int(st["stopped"].item()) == sum(a["status"] != 0 and b["status"] == 0 for b, a, _ in recs)
    assert torch.equal(tgt.A, keepA)
    frozen = before["ist"][:, 0] != 0
    assert frozen.sum() == len(traj)
    for name in ("x", "g", "d", "Xt", "sc", "ist"):
        assert np.array_equal(got[name][frozen], before[name][frozen], equal_nan=True), name
    print(f"{shape}: {len(recs) + K} steps, worst share of 1e-11 scale used {worst:.2e}")


# ---- 5. stopped and failing problems ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(6, 70, 3, 5), (5, 70, 4, 11)])
def test_stopped_problems_keep_every_bit_and_are_counted_once(shape):
    K, N, Cc, P = shape
    inp = ref.inputs(shape, flat0=False)
    tgt = _target(shape, inp)
    eng = tgt.engine
    st = eng.laplace_state_batched(eng.asarray(np.zeros((K, (Cc - 1) * P))))
    traj = ref.trajectories(shape)
    want = [end for _, end, _ in traj]
    for r in range(max(e["nfev"] for e in want)):
        _step(tgt, st, start=r == 0, **OPT)
    assert int(st["stopped"].item()) == K
    done = _download(st)
    assert np.array_equal(done["ist"], lref.pack(want)["ist"])
    for _ in range(5):                                                  # everything is frozen: whole workgroups leave at once
        _step(tgt, st, **OPT)
    again = _download(st)
    for name in ("x", "g", "d", "Xt", "sc", "ist", "stopped"):
        assert np.array_equal(again[name], done[name], equal_nan=True), name
    # made-up stopped states of every code among running ones
    states = [dict(e) for e in want]
    for k, code in zip(range(1, K), (2, 3, 4, 5, 1)):
        states[k]["status"] = code
    states[0] = traj[0][2][1][0]                                        # problem 0 before its second launch: running
    before = lref.pack(states)
    st = _upload(eng, before)
    _step(tgt, st, **OPT)
    got = _download(st)
    for name in ("x", "g", "d", "Xt", "sc", "ist"):
        assert np.array_equal(got[name][1:], before[name][1:], equal_nan=True), name
    assert got["ist"][0, 2] == before["ist"][0, 2] + 1 and int(st["stopped"].item()) == int(got["ist"][0, 0] != 0)


def test_failing_problems_are_flagged_and_leave_their_neighbours_alone():
    """(N, C, P) = (5, 3, 8): five rows give H rank <= 10 < 16, so the flat-prior problem 0 fails its factorisation; a NaN in one
    x0 is status 4; a flat prior on separable data has no mode.  For the last one the gradient test is switched off (gtol = 0):
    on separable data max|g| decays like exp(-|x|), so at the default gtol = 1e-8 the run stops with status 1 after about 24
    iterations, far from any mode, as the GLM initialiser does; with gtol = 0 it ends with status 2 (maxiter) or 5."""
    import gsmvi_amd
    shape = (6, 5, 3, 8)
    A, y, counts, lam, X = ref.inputs(shape)
    counts[:] = 5
    tgt = gsmvi_amd.BatchedSoftmaxTarget(A, y, 3, prior_precision=lam, counts=counts)
    H, cov, info = _hess(tgt, X)
    assert info[0] != 0 and np.array_equal(cov[0], np.eye(16)) and np.isfinite(H[0]).all() and (info[1:] == 0).all()
    lam2 = lam.copy()
    lam2[0] = 1.0                                                       # the same batch without the failure
    H2, cov2, info2 = _hess(gsmvi_amd.BatchedSoftmaxTarget(A, y, 3, prior_precision=lam2, counts=counts), X)
    assert (info2 == 0).all()
    for k in range(1, 6):
        assert np.array_equal(H[k], H2[k]) and np.array_equal(cov[k], cov2[k]), k
    Xn = X.copy()
    Xn[2, 7] = np.nan
    H3, cov3, info3 = _hess(tgt, Xn)
    assert np.isnan(H3[2]).all() and info3[2] == 1 and np.array_equal(cov3[2], np.eye(16))
    for k in (0, 1, 3, 4, 5):
        assert np.array_equal(H3[k], H[k]) and np.array_equal(cov3[k], cov[k]) and info3[k] == info[k], k
    Xb = X.copy()
    Xb[4] = 1e308                                                       # finite entries, an eta that is not
    H4, cov4, info4 = _hess(tgt, Xb)
    assert np.isnan(H4[4]).all() and info4[4] == 1 and np.array_equal(cov4[4], np.eye(16))
    for k in (0, 1, 2, 3, 5):
        assert np.array_equal(H4[k], H[k]) and np.array_equal(cov4[k], cov[k]), k
    # end to end: the rank-deficient flat-prior problem and a NaN start among good neighbours
    good = gsmvi_amd.laplace_init_softmax_batched(gsmvi_amd.BatchedSoftmaxTarget(A, y, 3, prior_precision=lam2, counts=counts))
    assert good[2].success.all()
    x0 = np.zeros((6, 16))
    x0[3, 2] = np.nan
    mean, cov, res = gsmvi_amd.laplace_init_softmax_batched(tgt, x0)
    assert res.status[0] == 5 and res.status[3] == 4 and res.info[3] == 1 and res.success.tolist() == [0, 1, 1, 0, 1, 1]
    assert np.array_equal(cov[0], np.eye(16)) and np.array_equal(cov[3], np.eye(16)) and np.isnan(mean[3, 2])
    for k in (1, 2, 4, 5):
        assert np.array_equal(mean[k], good[0][k]) and np.array_equal(cov[k], good[1][k]), k
    # separable data, a flat prior (problem 0) beside proper ones
    rs = np.random.RandomState(0)
    As = rs.standard_normal((3, 40, 2))
    W = 3.0 * rs.standard_normal((3, 2, 2))
    ys = np.concatenate([np.einsum("knp,kcp->knc", As, W), np.zeros((3, 40, 1))], axis=2).argmax(axis=2)
    t0 = gsmvi_amd.BatchedSoftmaxTarget(As, ys, 3, prior_precision=np.array([0.0, 0.5, 0.7]))
    t1 = gsmvi_amd.BatchedSoftmaxTarget(As, ys, 3, prior_precision=np.array([0.3, 0.5, 0.7]))
    m0, c0, r0 = gsmvi_amd.laplace_init_softmax_batched(t0, gtol=0.0, maxiter=60, maxfun=120, check_every=8)
    m1, c1, r1 = gsmvi_amd.laplace_init_softmax_batched(t1, gtol=0.0, maxiter=60, maxfun=120, check_every=8)
    assert r0.status[0] in (2, 5) and not r0.success[0] and np.array_equal(c0[0], np.eye(4)), r0.status
    for k in (1, 2):
        assert np.array_equal(m0[k], m1[k]) and np.array_equal(r0.nfev[k], r1.nfev[k]), k
    print(f"separable, flat prior, gtol = 0: status {r0.status[0]} after {r0.nit[0]} iterations, max|x| {np.abs(m0[0]).max():.1f}")


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_end_to_end_at_the_defaults(shape):
    """every problem with a proper prior converges; the existing score kernel, an independent path, confirms the gradient at the
    returned mode: |score| <= gtol + 1e-11 scale; the mean is within 2 sqrt(D) gtol / lam_k of the restatement's (each is within
    sqrt(D) gtol / lam_k of the mode: -grad^2 lp >= lam I); the covariance inverts the restated Hessian"""
    import gsmvi_amd
    K, N, Cc, P = shape
    D = (Cc - 1) * P
    inp = ref.inputs(shape)
    A, y, counts, lam, _ = inp
    gtol = 1e-8
    tgt = _target(shape, inp)
    tgt.engine.last_path(reset=True)
    mean, cov, res = gsmvi_amd.laplace_init_softmax_batched(tgt)
    assert "batched_softmax_laplace" in tgt.engine.last_path(reset=True)
    assert mean.shape == (K, D) and cov.shape == (K, D, D) and np.array_equal(mean, res.x) and res.nlaunch % 4 == 0
    G = -tgt.lp_g(tgt.engine.asarray(mean[:, None, :])).cpu().numpy()[:, 0, :]
    Href = ref.neg_hessian(A, y, Cc, counts, lam, mean)
    want = []
    for k in range(1, K):                                               # lam_k > 0
        assert res.status[k] == 1 and res.success[k] and res.info[k] == 0, (k, res.status[k], res.info[k])
        p = ref.problem(A, y, Cc, counts, lam, k)
        scale = ref.evaluate(p, mean[k])[3]["g"]
        assert (np.abs(G[k]) <= gtol + BAR * scale).all(), (k, np.abs(G[k]).max())
        assert np.abs(res.jac[k]).max() <= gtol
        s = ref.run(p, np.zeros(D))
        want.append(s)
        dist, bound = np.linalg.norm(mean[k] - s["x"]), 2 * np.sqrt(D) * gtol / lam[k]
        assert dist <= bound, (k, dist, bound)
        _check_inverse(cov[k], Href[k], k)
        assert res.nit[k] <= 12 and res.nfev[k] <= 15, (k, res.nit[k], res.nfev[k])
    print(f"{shape}: nit {res.nit[1:].tolist()} (restatement {[s['nit'] for s in want]}), nfev {res.nfev[1:].tolist()} "
          f"(restatement {[s['nfev'] for s in want]}), nlaunch {res.nlaunch}")


def test_check_every_does_not_change_the_result():
    import gsmvi_amd
    shape = (6, 70, 3, 5)
    tgt = _target(shape, ref.inputs(shape, flat0=False))
    x0 = 0.1 * np.random.RandomState(3).standard_normal((6, 10))
    runs = {c: gsmvi_amd.laplace_init_softmax_batched(tgt, x0, check_every=c) for c in (1, 4, 1000)}
    for c in (1, 1000):
        assert np.array_equal(runs[c][0], runs[4][0]) and np.array_equal(runs[c][1], runs[4][1])
        for f in ("x", "fun", "jac", "nit", "nfev", "status", "info"):
            assert np.array_equal(getattr(runs[c][2], f), getattr(runs[4][2], f)), (c, f)
    assert runs[4][2].success.all()
    assert runs[1][2].nlaunch == runs[1][2].nfev.max() and runs[1000][2].nlaunch == 200
    mt, ct, _ = gsmvi_amd.laplace_init_softmax_batched(tgt, x0, as_torch=True)
    assert mt.is_cuda and ct.is_cuda and np.array_equal(mt.cpu().numpy(), runs[4][0]) and np.array_equal(ct.cpu().numpy(), runs[4][1])
    one = gsmvi_amd.laplace_init_softmax_batched(tgt, x0[2])
    assert np.array_equal(one[0][2], runs[4][0][2]) and np.array_equal(one[1][2], runs[4][1][2])
    mean, cov, res = gsmvi_amd.laplace_init_softmax_batched(tgt, x0, maxiter=1)
    assert (res.status[[0, 2, 3, 4, 5]] == 2).all() and not res.success[[0, 2, 3, 4, 5]].any()
    assert all(np.array_equal(cov[k], np.eye(10)) for k in (0, 2, 3, 4, 5))
    with pytest.raises(TypeError, match="must be a BatchedSoftmaxTarget"):
        gsmvi_amd.laplace_init_softmax_batched(gsmvi_amd.BatchedGaussianTarget(np.zeros((2, 3)), cov=np.stack([np.eye(3)] * 2)))
    with pytest.raises(TypeError, match="BatchedGLMTarget or a BatchedLogisticTarget"):
        gsmvi_amd.laplace_init_batched(tgt)


# ---- 7. as a start ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,Cc,P,B", [(8, 40, 3, 2, 2), (6, 65, 18, 1, 4)])
def test_it_initialises_the_batched_fits(K, N, Cc, P, B):
    import gsmvi_amd
    D = (Cc - 1) * P
    tgt = _target((K, N, Cc, P), ref.inputs((K, N, Cc, P), flat0=False))
    mean, cov, res = gsmvi_amd.laplace_init_softmax_batched(tgt)
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


# ---- 8. bad arguments --------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_with_nothing_enqueued():
    import gsmvi_amd
    from gsmvi_amd import _lib
    eng = gsmvi_amd.get_engine()
    eng.last_path(reset=True)
    ref.check_bad_arguments(_lib.load_library())
    assert eng.last_path(reset=True) == set()
