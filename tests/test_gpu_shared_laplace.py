"""The shared-design Laplace initialiser on the GPU (csrc/gsmvi_laplace_shared_batched.hip): the fp64-MFMA Hessian and its inverse
against the numpy restatement (tests/shared_laplace_ref.py), neutral inputs and isolation bit for bit, exact integer data, the
replicated per-problem launch, the flags, every step of the restatement's trajectories through the C ABI from uploaded states,
frozen problems, ``laplace_init_shared_batched`` end to end and as the start of the batched fits, and its memory.

The bars are tests/test_gpu_laplace_batched.py's: H within 1e-11 of max|H_k|, max|cov H - I| <= 1e-11 cond_2(H), every written
state entry within 1e-11 of the restatement's scale for it.

K: the kernel packs PPW = 256 / gb_nt(D) problems into a workgroup, 4 for D <= 16 and 1 above, so the packing boundaries are
K = 4 (one past it: 5) and K = 1 (one past it: 2); KS = 1, 2, 5, 17, 65 holds both next to the issue's 1, 5, 17, 65 (17 and 65 are
one past four and sixteen full workgroups of four)."""
import numpy as np
import pytest
import torch

import shared_laplace_ref as ref

pytestmark = pytest.mark.gpu

KS = (1, 2, 5, 17, 65)
CASES = [(f, s) for f in ref.FAMILIES for s in ref.SHAPES]
SMALL_N = [(f, (n, 10)) for f in ref.FAMILIES for n in (1, 31, 32, 33)]


def _target(family, inp, full=True, sel=None, weights="given"):
    import gsmvi_amd
    A, y, o, v, lam, tau = inp[:6]
    sel = np.arange(y.shape[0]) if sel is None else np.asarray(sel)
    tau_s = tau[sel] if isinstance(tau, np.ndarray) else tau
    w = None if not full or weights is None else (v[sel] if isinstance(weights, str) else weights)
    return gsmvi_amd.SharedDesignGLMTarget(A, y[sel], family, prior_precision=lam[sel], offset=o[sel] if full else None,
                                           weights=w, noise_precision=tau_s)


def _model(tgt):
    return dict(offset=tgt.offset, weights=tgt.weights, prior_prec=tgt.prior_precision, noise_prec=tgt.noise_precision)


def _hess(tgt, X, want="both"):
    eng = tgt.engine
    out = eng.glm_shared_hessian_batched(eng.asarray(X), tgt.A, tgt.y, tgt.family, want=want, **_model(tgt))
    return tuple(t.cpu().numpy() for t in out) if isinstance(out, tuple) else out.cpu().numpy()


def _start(tgt, X, **opt):
    """the state after the first launch at the rows of X, as numpy"""
    eng = tgt.engine
    st = eng.laplace_state_batched(eng.asarray(X))
    eng.laplace_shared_step_batched(st, tgt.A, tgt.y, tgt.family, start=True, **opt, **_model(tgt))
    return {k: v.cpu().numpy() for k, v in st.items()}


def _points(inp):
    """one point per problem, |eta| of order one (make_inputs' X with its poisson cap, halved)"""
    return 0.5 * inp[6][:, 0, :]


def _check_inverse(cov, H_ref, where):
    """max|cov H_ref - I| <= 1e-11 cond_2(H_ref); returns the share of the bound used"""
    D = H_ref.shape[0]
    bound = 1e-11 * np.linalg.cond(H_ref)
    e = np.abs(cov @ H_ref - np.eye(D)).max()
    assert e <= bound, (where, e, bound)
    assert np.array_equal(cov, cov.T), where
    return e / bound


# ---- 1. the Hessian and its inverse ------------------------------------------------------------------------------------------
def _hessian_case(family, shape, Ks):
    import gsmvi_amd
    N, D = shape
    worst, share = 0.0, 0.0
    for K in Ks:
        inp = ref.make_inputs(family, K, N, D, 1)
        A, y, o, v, lam, tau, _ = inp
        X = _points(inp)
        for full in (True, False):
            tgt = _target(family, inp, full)
            ins = [tgt.A, tgt.y] + ([tgt.offset, tgt.weights] if full else [])
            keep = [t.clone() for t in ins]
            eng = tgt.engine
            Xd = eng.asarray(X)
            eng.last_path(reset=True)
            H, cov, info = _hess(tgt, Xd)
            assert eng.last_path(reset=True) == {"batched_laplace", "batched_target"}
            assert np.array_equal(Xd.cpu().numpy(), X) and all(torch.equal(t, k) for t, k in zip(ins, keep))
            Hpub = gsmvi_amd.neg_hessian_shared_batched(tgt, X)
            assert isinstance(Hpub, torch.Tensor) and np.array_equal(Hpub.cpu().numpy(), H)
            want = ref.neg_hessian(family, A, y, o if full else None, v if full else None, lam, tau, X)
            for k in range(K):
                assert np.array_equal(H[k], H[k].T) and np.array_equal(cov[k], cov[k].T), (K, full, k)
                e, top = np.abs(H[k] - want[k]).max(), np.abs(want[k]).max()
                assert e <= 1e-11 * top, (K, full, k, e, top)
                worst = max(worst, e / top if top > 0 else 0.0)
                checked = ref.inverse(want[k])[1] == 0 and np.linalg.cond(want[k]) < 1e8     # (far from the pivot rule's threshold)
                assert checked or k == 0, (K, full, k)                  # every problem with a proper prior
                if checked:
                    assert info[k] == 0, (K, full, k, info[k])
                    share = max(share, _check_inverse(cov[k], want[k], (K, full, k)))
                elif info[k] != 0:
                    assert np.array_equal(cov[k], np.eye(D)), (K, full, k)
    print(f"{family} {shape} K={Ks}: worst error {worst:.2e} of max|H|, worst share of 1e-11 cond used {share:.3f}")


@pytest.mark.parametrize("family,shape", CASES)
def test_hessian_and_inverse_match_the_restatement(family, shape):
    """every K of KS, with offset and weights and with neither: 1e-11 of max|H_k|, the inverse within 1e-11 cond, both exactly
    symmetric, inputs unchanged, the path bits of this kernel alone, and the public function gives the same bits"""
    _hessian_case(family, shape, KS)


@pytest.mark.parametrize("family,shape", SMALL_N)
def test_hessian_and_inverse_at_n_around_one_row_tile(family, shape):
    _hessian_case(family, shape, (5,))


# ---- 2. neutral inputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("N,D", [(70, 10), (70, 33)])
def test_neutral_inputs_give_the_same_bits(family, N, D):
    """weights = None and weights = 1; y = NaN and offset = inf where v = 0 against clean values there: H, cov, info and the
    whole state after the first launch, bit for bit"""
    K = 6
    inp = ref.make_inputs(family, K, N, D, 1)
    X = _points(inp)
    opt = dict(maxiter=30, maxfun=60, gtol=1e-8)
    none, ones = _target(family, inp, weights=None), _target(family, inp, weights=np.ones((K, N)))
    for a, b in zip(_hess(none, X), _hess(ones, X)):
        assert np.array_equal(a, b)
    sa, sb = _start(none, X, **opt), _start(ones, X, **opt)
    assert all(np.array_equal(sa[n], sb[n]) for n in sa)
    dirty = ref.make_inputs(family, K, N, D, 1, poison=True)
    assert np.isnan(dirty[1]).any() and np.isinf(dirty[2]).any() and np.array_equal(dirty[3], inp[3])
    clean_t, dirty_t = _target(family, inp), _target(family, dirty)
    for a, b in zip(_hess(clean_t, X), _hess(dirty_t, X)):
        assert np.isfinite(a).all() and np.array_equal(a, b)
    sa, sb = _start(clean_t, X, **opt), _start(dirty_t, X, **opt)
    assert all(np.array_equal(sa[n], sb[n]) for n in sa) and (sa["ist"][:, 0] != 4).all()


# ---- 3. integer data -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,K", [(5, 37, 3), (17, 16, 2), (64, 65, 3)])
def test_integer_data_is_exact(D, N, K):
    """gaussian, tau = 1, small integers everywhere: every product and partial sum is an integer below 2^53, so H = sum_n v a a^T +
    lam I and g = -(sum_n v (y - eta) a - lam x) must equal the integer arithmetic in any order of summation"""
    import gsmvi_amd
    rs = np.random.RandomState(D + N)
    A = rs.randint(-3, 4, (N, D)).astype(np.float64)
    y, o = rs.randint(-5, 6, (K, N)).astype(np.float64), rs.randint(-2, 3, (K, N)).astype(np.float64)
    v = rs.randint(0, 4, (K, N)).astype(np.float64)
    lam, X = rs.randint(0, 4, K).astype(np.float64), rs.randint(-2, 3, (K, D)).astype(np.float64)
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, "gaussian", prior_precision=lam, offset=o, weights=v)
    H = _hess(tgt, X, want="h")
    g = _start(tgt, X, maxiter=5, maxfun=5, gtol=0.0)["g"]
    Ai = A.astype(np.int64)
    for k in range(K):
        vi = v[k].astype(np.int64)
        Hk = (Ai * vi[:, None]).T @ Ai + int(lam[k]) * np.eye(D, dtype=np.int64)
        res = y[k].astype(np.int64) - (Ai @ X[k].astype(np.int64) + o[k].astype(np.int64))
        gk = -((vi * res) @ Ai - int(lam[k]) * X[k].astype(np.int64))
        assert np.array_equal(H[k], Hk.astype(np.float64)), k
        assert np.array_equal(g[k], gk.astype(np.float64)), k


# ---- 4. the replicated per-problem launch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("K,N,D", [(9, 70, 10), (9, 70, 33)])
def test_agreement_with_the_replicated_per_problem_launch(family, K, N, D):
    import gsmvi_amd
    inp = ref.make_inputs(family, K, N, D, 1)
    A, y, o, v, lam, tau, _ = inp
    X = _points(inp)
    H = _hess(_target(family, inp, weights=None), X, want="h")
    rep = gsmvi_amd.BatchedGLMTarget(ref.replicate(A, K), y, family, prior_precision=lam, offset=o, noise_precision=tau)
    Hr = rep.neg_hessian(X).cpu().numpy()
    worst = max(np.abs(H[k] - Hr[k]).max() / np.abs(Hr[k]).max() for k in range(K))
    print(f"{family} {(K, N, D)}: worst difference {worst:.2e} of max|H|")
    assert worst <= 1e-11


# ---- 5. isolation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("N,D", [(70, 10), (70, 33)])
def test_a_problem_alone_among_16_and_among_1024(family, N, D):
    inp = ref.make_inputs(family, 16, N, D, 1)
    X = _points(inp)
    j = 5
    opt = dict(maxiter=30, maxfun=60, gtol=1e-8)
    among16 = _hess(_target(family, inp), X)
    alone = _hess(_target(family, inp, sel=[j]), X[j:j + 1])
    sel = np.tile(np.arange(16), 64)
    big = _target(family, inp, sel=sel)
    among1024 = _hess(big, X[sel])
    assert among16[2][j] == 0 and np.isfinite(among16[0][j]).all()
    for a, b, c in zip(alone, among16, among1024):
        assert np.array_equal(a[0], b[j])
        for k in (j, 16 + j, 1024 - 16 + j):
            assert np.array_equal(c[k], b[j]), k
    s1, s16, s1024 = _start(_target(family, inp, sel=[j]), X[j:j + 1], **opt), _start(_target(family, inp), X, **opt), \
        _start(big, X[sel], **opt)
    for name in ("x", "g", "d", "Xt", "sc", "ist"):
        assert np.array_equal(s1[name][0], s16[name][j]) and np.array_equal(s1024[name][1024 - 16 + j], s16[name][j]), name


# ---- 6. flags ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [10, 33])
def test_flags_reach_their_problem_alone(D):
    """a NaN in one x_k; a poisson e^eta that overflows at a v > 0 observation; the same overflow at v = 0 flags nothing"""
    family, K, N = "poisson", 6, 40
    inp = ref.make_inputs(family, K, N, D, 1)
    A, y, o, v, lam, tau, _ = inp
    X = _points(inp)
    opt = dict(maxiter=30, maxfun=60, gtol=1e-8)
    tgt = _target(family, inp)
    H0, cov0, info0 = _hess(tgt, X)
    st0 = _start(tgt, X, **opt)
    assert (info0[1:] == 0).all() and (st0["ist"][:, 0] != 4).all()

    def only(k, Hn, covn, infon, stn):
        assert np.isnan(Hn[k]).all() and infon[k] == 1 and np.array_equal(covn[k], np.eye(D)) and stn["ist"][k, 0] == 4
        for j in range(K):
            if j != k:
                assert np.array_equal(Hn[j], H0[j]) and np.array_equal(covn[j], cov0[j]) and infon[j] == info0[j], j
                assert all(np.array_equal(stn[n][j], st0[n][j]) for n in ("x", "g", "d", "Xt", "sc", "ist")), j

    Xn = X.copy()
    Xn[2, D - 1] = np.nan
    only(2, *_hess(tgt, Xn), _start(tgt, Xn, **opt))
    n = int(np.flatnonzero(v[4] > 0)[0])
    Xb = X.copy()
    Xb[4] = 4000.0 * np.sign(A[n])                                      # eta_n = 4000 sum_j |a_nj|: e^eta overflows
    only(4, *_hess(tgt, Xb), _start(tgt, Xb, **opt))
    o2 = o.copy()
    o2[v == 0] = 4000.0                                                 # the same overflow where v = 0
    quiet = _target(family, (A, y, o2, v, lam, tau))
    for a, b in zip(_hess(quiet, X), (H0, cov0, info0)):
        assert np.array_equal(a, b)
    stq = _start(quiet, X, **opt)
    assert all(np.array_equal(stq[n], st0[n]) for n in st0)


# ---- 7. every step of every trajectory -----------------------------------------------------------------------------------------------
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
    """each round of each problem's trajectory (K = 5, gtol = 1e-6; margins asserted in tests/test_shared_laplace_cpu.py) is one
    problem of a launch: the restatement's state before it goes up, everything the launch leaves is compared with the
    restatement's state after it; every trajectory's stopped end state rides along and must come back bit for bit"""
    inp = ref.inputs(family, shape)
    worst, nsteps = 0.0, 0
    opt = dict(maxiter=30, maxfun=60, gtol=ref.STEP_GTOL)
    for full in (True, False):
        traj = ref.trajectories(family, shape, full)
        tgt = _target(family, inp, full)                                # the first launch
        eng = tgt.engine
        st = eng.laplace_state_batched(eng.asarray(np.zeros((ref.STEP_K, shape[1]))))
        eng.last_path(reset=True)
        eng.laplace_shared_step_batched(st, tgt.A, tgt.y, family, start=True, **opt, **_model(tgt))
        assert eng.last_path(reset=True) == {"batched_laplace", "batched_target"}
        first = [rec[0] for _, _, rec in traj]
        worst = max(worst, _compare(_download(st), first, (full, "start")))
        assert int(st["stopped"].item()) == sum(a["status"] != 0 for _, a, _ in first)
        recs, ks = [], []                                               # every later launch, and the frozen end states
        for k, end, rec in traj:
            recs += rec[1:] + [(end, end, {})]
            ks += [k] * len(rec)
        tgt = _target(family, inp, full, sel=ks)
        before = ref.pack([b for b, _, _ in recs])
        st = _upload(eng, before)
        ins = [tgt.A, tgt.y] + ([tgt.offset, tgt.weights] if full else [])
        keep = [t.clone() for t in ins]
        eng.laplace_shared_step_batched(st, tgt.A, tgt.y, family, **opt, **_model(tgt))
        got = _download(st)
        worst = max(worst, _compare(got, recs, (full, "step")))
        nsteps += len(recs)
        assert int(st["stopped"].item()) == sum(a["status"] != 0 and b["status"] == 0 for b, a, _ in recs)
        assert all(torch.equal(t, k) for t, k in zip(ins, keep))
        frozen = before["ist"][:, 0] != 0
        assert frozen.sum() == len(traj)
        for name in ("x", "g", "d", "Xt", "sc", "ist"):
            assert np.array_equal(got[name][frozen], before[name][frozen], equal_nan=True), name
    print(f"{family} {shape}: {nsteps} steps, worst share of 1e-11 scale used {worst:.3f}")


# ---- 8. frozen problems ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(70, 10), (70, 33)])
def test_stopped_problems_keep_every_bit_and_are_counted_once(shape):
    family = "poisson"
    inp = ref.inputs(family, shape)
    A, y, o, v, lam, tau, _ = inp
    tgt = _target(family, inp)
    eng = tgt.engine
    K, D = ref.STEP_K, shape[1]
    st = eng.laplace_state_batched(eng.asarray(np.zeros((K, D))))
    opt = dict(maxiter=30, maxfun=60, gtol=ref.STEP_GTOL)
    traj = ref.trajectories(family, shape, True)
    want = [end for _, end, _ in traj]
    for r in range(max(e["nfev"] for e in want)):
        eng.laplace_shared_step_batched(st, tgt.A, tgt.y, family, start=r == 0, **opt, **_model(tgt))
    assert int(st["stopped"].item()) == K
    done = _download(st)
    assert np.array_equal(done["ist"], ref.pack(want)["ist"])
    for _ in range(5):                                                  # everything is frozen: whole workgroups leave at once
        eng.laplace_shared_step_batched(st, tgt.A, tgt.y, family, **opt, **_model(tgt))
    again = _download(st)
    for name in ("x", "g", "d", "Xt", "sc", "ist", "stopped"):
        assert np.array_equal(again[name], done[name], equal_nan=True), name
    # the f and g left in the state against the score kernel, an independent path, at the final points
    G, lp = tgt.lp_and_score(eng.asarray(done["x"][:, None, :]))
    G, lp = G.cpu().numpy()[:, 0, :], lp.cpu().numpy()[:, 0]
    for k in range(K):
        sc = ref.evaluate(ref.problem(family, A, y, o, v, lam, tau, k), done["x"][k])[3]
        assert abs(done["sc"][k, 0] + lp[k]) <= 1e-11 * sc["f"], k
        assert (np.abs(done["g"][k] + G[k]) <= 1e-11 * sc["g"]).all(), k
    # made-up stopped states of every code among running ones
    states = [dict(e) for e in want]
    for k, code in zip(range(1, K), (2, 3, 4, 5)):
        states[k]["status"] = code
    states[0] = traj[0][2][1][0]                                        # problem 0 before its second launch: running
    before = ref.pack(states)
    st = _upload(eng, before)
    eng.laplace_shared_step_batched(st, tgt.A, tgt.y, family, **opt, **_model(tgt))
    got = _download(st)
    for name in ("x", "g", "d", "Xt", "sc", "ist"):
        assert np.array_equal(got[name][1:], before[name][1:], equal_nan=True), name
    assert got["ist"][0, 2] == before["ist"][0, 2] + 1 and int(st["stopped"].item()) == int(got["ist"][0, 0] != 0)


# ---- 9. end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", CASES)
def test_end_to_end_at_the_defaults(family, shape):
    """every problem with a proper prior converges; the score kernel, an independent path, confirms the gradient; the mean is
    within 2 sqrt(D) gtol / lam_k of the restatement's ``run`` (each is within sqrt(D) gtol / lam_k of the mode: -grad^2 lp >=
    lam I); the covariance inverts the restated Hessian at the mean"""
    import gsmvi_amd
    N, D = shape
    K = ref.STEP_K
    inp = ref.make_inputs(family, K, N, D, 1)
    A, y, o, v, lam, tau, _ = inp
    gtol = 1e-8
    for full in (True, False):
        tgt = _target(family, inp, full)
        mean, cov, res = gsmvi_amd.laplace_init_shared_batched(tgt)
        assert mean.shape == (K, D) and cov.shape == (K, D, D) and np.array_equal(mean, res.x) and res.nlaunch % 4 == 0
        G = -tgt.lp_g(tgt.engine.asarray(mean[:, None, :])).cpu().numpy()[:, 0, :]
        args = (o if full else None, v if full else None, lam, tau)
        Href = ref.neg_hessian(family, A, y, *args, mean)
        want = []
        for k in range(1, K):                                           # lam_k > 0
            assert res.status[k] == 1 and res.success[k] and res.info[k] == 0, (full, k, res.status[k], res.info[k])
            p = ref.problem(family, A, y, *args, k)
            scale = ref.evaluate(p, mean[k])[3]["g"]
            assert (np.abs(G[k]) <= gtol + 1e-11 * scale).all(), (full, k, np.abs(G[k]).max())
            assert np.abs(res.jac[k]).max() <= gtol
            s = ref.run(p, np.zeros(D))
            want.append(s)
            dist, bound = np.linalg.norm(mean[k] - s["x"]), 2 * np.sqrt(D) * gtol / lam[k]
            assert dist <= bound, (full, k, dist, bound)
            _check_inverse(cov[k], Href[k], (full, k))
            assert res.nit[k] <= 7 and res.nfev[k] <= 9, (full, k, res.nit[k], res.nfev[k])
        print(f"{family} {shape} full={full}: nit {res.nit[1:].tolist()} (restatement {[s['nit'] for s in want]}), nfev "
              f"{res.nfev[1:].tolist()} (restatement {[s['nfev'] for s in want]}), nlaunch {res.nlaunch}")


def _all_weights_zero():
    """problem 0 (the issue's A): lam = 0.25 and all weights zero; problem 1 (B): lam = 0 and all weights zero; two ordinary ones"""
    import gsmvi_amd
    A, y, o, v, lam, tau, _ = ref.make_inputs("logistic", 4, 40, 3, 1)
    v[0], v[1], lam[0], lam[1] = 0.0, 0.0, 0.25, 0.0
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, "logistic", prior_precision=lam, offset=o, weights=v)
    return gsmvi_amd.laplace_init_shared_batched(tgt)


def test_problems_whose_weights_are_all_zero():
    """A (lam > 0): status 1, info 0, cov exactly I / lam, x = 0.  B (lam = 0): status 5, info != 0, cov = I, no success: the
    launches stop it by the gradient test at its start (f = g = 0, H = 0), the final factorisation fails, and
    ``laplace_init_shared_batched`` reports a stationary point whose Hessian is not positive definite as status 5.  Their
    neighbours converge."""
    mean, cov, res = _all_weights_zero()
    print(f"problem B: status {res.status[1]}, nit {res.nit[1]}, nfev {res.nfev[1]}, info {res.info[1]}, success {res.success[1]}")
    assert res.status[0] == 1 and res.info[0] == 0 and res.success[0]
    assert np.array_equal(cov[0], 4.0 * np.eye(3)) and not mean[0].any()
    assert res.status[1] == 5 and res.info[1] != 0 and np.array_equal(cov[1], np.eye(3)) and not res.success[1]
    assert not mean[1].any() and res.nit[1] == 0 and res.nfev[1] == 1
    assert res.success[2:].all() and (res.status[2:] == 1).all()


def test_check_every_x0_and_as_torch():
    import gsmvi_amd
    family, (N, D), K = "probit", (70, 10), 6
    inp = ref.make_inputs(family, K, N, D, 1)
    tgt = _target(family, inp)
    x0 = 0.1 * np.random.RandomState(3).standard_normal((K, D))
    runs = {c: gsmvi_amd.laplace_init_shared_batched(tgt, x0, check_every=c) for c in (1, 4, 1000)}
    for c in (1, 1000):
        assert np.array_equal(runs[c][0], runs[4][0]) and np.array_equal(runs[c][1], runs[4][1])
        for f in ("x", "fun", "jac", "nit", "nfev", "status", "info"):
            assert np.array_equal(getattr(runs[c][2], f), getattr(runs[4][2], f)), (c, f)
    assert runs[1][2].nlaunch == runs[1][2].nfev.max() and runs[1000][2].nlaunch == 200
    mt, ct, _ = gsmvi_amd.laplace_init_shared_batched(tgt, x0, as_torch=True)
    assert mt.is_cuda and ct.is_cuda and np.array_equal(mt.cpu().numpy(), runs[4][0]) and np.array_equal(ct.cpu().numpy(), runs[4][1])
    one = gsmvi_amd.laplace_init_shared_batched(tgt, x0[2])
    assert np.array_equal(one[0][2], runs[4][0][2]) and np.array_equal(one[1][2], runs[4][1][2])
    mean, cov, res = gsmvi_amd.laplace_init_shared_batched(tgt, x0, maxiter=1)
    assert (res.status == 2).all() and not res.success.any() and np.array_equal(cov, np.broadcast_to(np.eye(D), (K, D, D)))
    with pytest.raises(TypeError, match="laplace_init_shared_batched"):
        gsmvi_amd.laplace_init_batched(tgt)


# ---- 10. as a start --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B", [(5, 2), (17, 4)])
def test_it_initialises_the_batched_fits(D, B):
    import gsmvi_amd
    K, N = 6, 8 * D
    A, y, o, v, lam, tau, _ = ref.make_inputs("logistic", K, N, D, 1)
    lam[0] = 0.5
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, "logistic", prior_precision=lam, offset=o, weights=v)
    mean, cov, res = gsmvi_amd.laplace_init_shared_batched(tgt)
    assert res.success.all()
    keys = np.arange(K) + 7
    m1, c1 = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, mean=mean, cov=cov, batch_size=B, niter=50, verbose=False)
    assert np.isfinite(m1).all() and np.isfinite(c1).all()
    m2, c2 = gsmvi_amd.BaMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, lambda i: 100 / (1 + i), mean=mean, cov=cov, batch_size=B,
                                                          niter=50, verbose=False)
    assert np.isfinite(m2).all() and np.isfinite(c2).all()


# ---- 11. memory ------------------------------------------------------------------------------------------------------------------------
def test_the_design_is_never_replicated_in_device_memory():
    """K = 2048, N = 256, D = 16: one replicated design is K N D 8 = 67 MB; the whole call stays below half of that above the
    target's own arrays"""
    import gsmvi_amd
    K, N, D = 2048, 256, 16
    A, y, o, v, lam, tau, _ = ref.make_inputs("logistic", K, N, D, 1)
    lam[0] = 0.5
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, "logistic", prior_precision=lam, offset=o, weights=v)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    mean, cov, res = gsmvi_amd.laplace_init_shared_batched(tgt)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak rise {rise / 1e6:.1f} MB over the target's arrays; one replicated design is {K * N * D * 8 / 1e6:.1f} MB")
    assert res.success.all() and rise < K * N * D * 8 // 2


# ---- 12. bad arguments -----------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_with_nothing_enqueued():
    import gsmvi_amd
    from gsmvi_amd import _lib
    eng = gsmvi_amd.get_engine()
    eng.last_path(reset=True)
    ref.check_bad_arguments(_lib.load_library())
    assert eng.last_path(reset=True) == set()
