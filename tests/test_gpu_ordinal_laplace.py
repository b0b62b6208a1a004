"""The ordinal Laplace initialiser on the GPU (csrc/gsmvi_ordinal_laplace_batched.hip): the link curvature against the mpmath
truth, the fp64-MFMA Hessian with its delta block and its inverse against the long double restatement
(tests/ordinal_laplace_ref.py), C = 2 against the logistic launch of the GLM Hessian, exact symmetry, exact integer data and
isolation bit for bit, the flags, every round of the restatement's trajectories -- with and without the retry rule -- through the
C ABI from uploaded states, frozen problems, ``laplace_init_ordinal_batched`` end to end, the reported cases, and as the start of the
batched fits and diagnostics.

The bars: a curvature entry within max(16, 4 C_CPU) of its truth scale (tests/ordinal_curv_truth.py); every entry of H within 1e-11
of its scale (the sum over n of the magnitudes of its terms, plus the prior); max|cov H - I| <= 1e-11 cond_2(H); every written
state entry within 1e-11 of the restatement's scale for it (tests/test_gpu_negbin_laplace.py's bars).

K: the kernel packs 4 problems into a workgroup for D <= 16 and 1 above: KS = 1, 2, 5, 17, 65."""
import numpy as np
import pytest
import torch

import ordinal_batched_ref as oref
import ordinal_curv_truth as ct
import ordinal_laplace_ref as ref

pytestmark = pytest.mark.gpu

KS = (1, 2, 5, 17, 65)
OPT = dict(maxiter=40, maxfun=80, gtol=ref.STEP_GTOL)


def _target(inp, full=True, sel=None, scalar=False):
    """inp = (A, y, offset, counts, lam, kap, C); full: with offset and counts; scalar: scalar priors"""
    import gsmvi_amd
    A, y, o, counts, lam, kap, C = inp[:7]
    sel = np.arange(y.shape[0]) if sel is None else np.asarray(sel)
    pick = lambda v: v[sel] if isinstance(v, np.ndarray) else v          # noqa: E731
    if scalar:
        lam, kap = 0.5, 0.25
    return gsmvi_amd.BatchedOrdinalTarget(A[sel], y[sel], C, prior_precision=pick(lam), cut_precision=pick(kap),
                                          counts=pick(counts) if full else None, offset=o[sel] if full and o is not None else None)


def _model(tgt):
    return dict(offset=tgt.offset, counts=tgt.counts, prior_prec=tgt.prior_precision, cut_prec=tgt.cut_precision)


def _hess(tgt, X, want="both"):
    eng = tgt.engine
    out = eng.ordinal_hessian_batched(eng.asarray(X), tgt.A, tgt.y, tgt.C, want=want, **_model(tgt))
    return tuple(t.cpu().numpy() for t in out) if isinstance(out, tuple) else out.cpu().numpy()


def _start(tgt, X, **opt):
    eng = tgt.engine
    st = eng.laplace_state_batched(eng.asarray(X))
    eng.ordinal_laplace_step_batched(st, tgt.A, tgt.y, tgt.C, start=True, **opt, **_model(tgt))
    return {k: v.cpu().numpy() for k, v in st.items()}


def _inputs(K, N, P, C):
    """(A, y, offset, counts, lam, kap, C), X (K, D) of ordinal_batched_ref.make_inputs: poisoned rows beyond counts, counts 0 for
    problem 1, lam = kap = 0 for problem 0, a class absent from the last problem's data"""
    A, y, o, counts, lam, kap, X = oref.make_inputs(K, N, P, C, 1)
    return (A, y, o, counts, lam, kap, C), X[:, 0, :]


def _clean(inp, full):
    """the inputs as the restatement of an unrestricted target takes them (no counts: the poisoned rows replaced)"""
    A, y, o, counts, lam, kap, C = inp
    if full:
        return inp
    return np.nan_to_num(A, nan=0.25), np.clip(y, 0, C - 1), None, None, lam, kap, C


def _check_inverse(cov, H_ref, where):
    D = H_ref.shape[0]
    bound = 1e-11 * np.linalg.cond(H_ref)
    e = np.abs(cov @ H_ref - np.eye(D)).max()
    assert e <= bound, (where, e, bound)
    assert np.array_equal(cov, cov.T), where
    return e / bound


# ---- 1. the link curvature against the truth ---------------------------------------------------------------------------------------
def test_link_curvature_is_within_the_bound_of_the_truth_on_the_whole_grid():
    """N = 1, P = 1, C = 3, a = 1, beta = 0, the offset eta, no priors: H is the row's 3 x 3 block, one problem per grid point"""
    import gsmvi_amd
    tab = ct.load_table()
    A, y, o, X = ct.problems()
    eta, d0, d1, yy = ct.grid()
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, 3, prior_precision=0.0, cut_precision=0.0, offset=o)
    H = _hess(tgt, X, want="h")
    for q, got in ct.entries(H).items():
        r = ct.ratio(got, tab, q)
        i = int(np.argmax(r))
        print(f"{q}: worst ratio {r.max():.3f} at eta = {eta[i]!r}, delta = ({d0[i]!r}, {d1[i]!r}), y = {yy[i]}; bound {ct.c_gpu(q)}")
        assert r.max() <= ct.c_gpu(q), (q, r.max(), eta[i], d0[i], d1[i], yy[i])
    assert np.array_equal(H, np.swapaxes(H, 1, 2))


# ---- 2. the Hessian and its inverse -------------------------------------------------------------------------------------------------
def _hessian_case(shape, Ks):
    import gsmvi_amd
    N, P, C = shape
    D = P + C - 1
    worst, share, floor = 0.0, 0.0, 0.0
    for K in Ks:
        inp0, X = _inputs(K, N, P, C)
        for full, scalar in ((True, False), (False, False), (False, True)):
            inp = _clean(inp0, full)
            tgt = _target(inp, full, scalar=scalar)
            eng = tgt.engine
            ins = [tgt.A, tgt.y] + ([tgt.offset, tgt.counts] if full else [])
            keep = [t.clone() for t in ins]
            Xd = eng.asarray(X)
            eng.last_path(reset=True)
            H, cov, info = _hess(tgt, Xd)
            assert eng.last_path(reset=True) == {"batched_laplace", "batched_target"}
            assert np.array_equal(Xd.cpu().numpy(), X)
            assert all(np.array_equal(t.cpu().numpy(), k.cpu().numpy(), equal_nan=True) for t, k in zip(ins, keep))
            Hpub = gsmvi_amd.neg_hessian_ordinal_batched(tgt, X)
            assert isinstance(Hpub, torch.Tensor) and np.array_equal(Hpub.cpu().numpy(), H)
            A, y, o, counts, lam, kap, _ = inp
            if scalar:
                lam, kap = 0.5, 0.25
            want, sH = ref.neg_hessian(A, y, o, counts, lam, kap, C, X, L=np.longdouble)
            w64 = ref.neg_hessian(A, y, o, counts, lam, kap, C, X)[0]
            for k in range(K):
                assert np.array_equal(H[k], H[k].T) and np.array_equal(cov[k], cov[k].T), (K, full, k)
                pos = sH[k] > 0
                assert np.array_equal(H[k][~pos], want[k][~pos])        # (a scale of zero: an exact zero)
                e = np.abs(H[k] - want[k])[pos] / sH[k][pos]
                assert (e <= 1e-11).all(), (K, full, scalar, k, e.max())
                worst = max(worst, e.max() if e.size else 0.0)
                floor = max(floor, (np.abs(w64[k] - want[k])[pos] / sH[k][pos]).max() if e.size else 0.0)
                ok = ref.inverse(want[k])[1] == 0 and np.linalg.cond(want[k]) < 1e8
                if ok:
                    assert info[k] == 0, (K, full, k, info[k])
                    share = max(share, _check_inverse(cov[k], want[k], (K, full, k)))
                elif info[k] != 0:
                    assert np.array_equal(cov[k], np.eye(D)), (K, full, k)
    print(f"{shape} K={Ks}: worst error {worst:.2e} of the entry's scale (float64 restatement: {floor:.2e}), worst share of 1e-11 "
          f"cond used {share:.3f}")


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_hessian_and_inverse_match_the_high_precision_restatement(shape):
    """every K of KS; with offset, counts (0 among them) and per-problem priors (lam = kap = 0 for problem 0), without either, and
    with scalar priors; a class absent from the last problem's data"""
    _hessian_case(shape, KS)


@pytest.mark.parametrize("shape", ref.SMALL_N)
def test_hessian_and_inverse_at_n_around_one_row_tile(shape):
    _hessian_case(shape, (5,))


@pytest.mark.parametrize("N,P", [(70, 9), (33, 15), (70, 16), (70, 63)])
def test_two_classes_match_the_logistic_glm_launch(N, P):
    """C = 2 is logistic regression on the design [A, -1] with lam = kap: gsmvi_glm_hessian_batched_f64, an independent path"""
    K, D = 6, P + 1
    rs = np.random.RandomState(N + P)
    A = rs.standard_normal((K, N, P)) / np.sqrt(P)
    y = rs.randint(0, 2, (K, N))
    lam = 0.1 + rs.random_sample(K)
    X = rs.standard_normal((K, D))
    tgt = _target((A, y, None, None, lam, lam, 2), full=False)
    eng = tgt.engine
    H, cov, info = _hess(tgt, X)
    A2 = np.concatenate([A, -np.ones((K, N, 1))], axis=2)
    Hg, covg, infog = (t.cpu().numpy() for t in eng.glm_hessian_batched(eng.asarray(X), eng.asarray(A2), eng.asarray(y.astype(np.float64)),
                                                                       "logistic", prior_prec=eng.batched_regs(lam), want="both"))
    sH = ref.neg_hessian(A, y, None, None, lam, lam, 2, X)[1]
    e = (np.abs(H - Hg) / sH).max()
    print(f"(N, P) = {(N, P)}: worst |H_ordinal - H_logistic| {e:.2e} of the entry's scale")
    assert e <= 1e-11 and np.array_equal(info, infog) and (info == 0).all()
    for k in range(K):
        _check_inverse(cov[k], Hg[k], k)


# ---- 3. exact data, isolation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P", [(70, 9), (70, 16), (33, 40)])
def test_integer_data_give_the_exact_matrix_at_two_classes(N, P):
    """C = 2, x = 0: a = b = 0, fa = fb = 1/4 exactly, so with integer A and priors every term and every partial sum is a multiple
    of 1/4 below 2^53: H[:P, :P] = A^T A / 4 + lam I, H[:P, P] = -sum_n a_n / 4, H[P, P] = N / 4 + kap, exact in any order"""
    K = 6
    rs = np.random.RandomState(N + P)
    A = rs.randint(-3, 4, (K, N, P)).astype(np.float64)
    y = rs.randint(0, 2, (K, N))
    lam = rs.randint(0, 4, K).astype(np.float64)
    kap = rs.randint(0, 4, K).astype(np.float64)
    tgt = _target((A, y, None, None, lam, kap, 2), full=False)
    H = _hess(tgt, np.zeros((K, P + 1)), want="h")
    for k in range(K):
        Ai = A[k].astype(np.int64)
        assert np.array_equal(H[k, :P, :P], (Ai.T @ Ai).astype(np.float64) / 4.0 + lam[k] * np.eye(P)), k
        assert np.array_equal(H[k, :P, P], -Ai.sum(0).astype(np.float64) / 4.0), k
        assert H[k, P, P] == N / 4.0 + kap[k]
        assert np.array_equal(H[k], H[k].T)


@pytest.mark.parametrize("N,P,C", [(70, 9, 4), (70, 20, 13)])
def test_a_problem_alone_among_16_and_among_1024(N, P, C):
    inp, X = _inputs(16, N, P, C)
    j = 5
    opt = dict(maxiter=30, maxfun=60, gtol=1e-8)
    among16 = _hess(_target(inp), X)
    alone = _hess(_target(inp, sel=[j]), X[j:j + 1])
    sel = np.tile(np.arange(16), 64)
    big = _target(inp, sel=sel)
    among1024 = _hess(big, X[sel])
    assert np.isfinite(among16[0][j]).all()
    for a, b, c in zip(alone, among16, among1024):
        assert np.array_equal(a[0], b[j])
        for k in (j, 16 + j, 1024 - 16 + j):
            assert np.array_equal(c[k], b[j]), k
    s1, s16, s1024 = _start(_target(inp, sel=[j]), X[j:j + 1], **opt), _start(_target(inp), X, **opt), _start(big, X[sel], **opt)
    for name in ("x", "g", "d", "Xt", "sc", "ist"):
        assert np.array_equal(s1[name][0], s16[name][j]) and np.array_equal(s1024[name][1024 - 16 + j], s16[name][j]), name


# ---- 4. flags -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,C", [(9, 4), (20, 13)])
def test_flags_reach_their_problem_alone(P, C):
    """a NaN in one beta; a delta_j, j >= 1, whose gap overflows; one whose gap is subnormal; an infinite delta_0.  delta_0 = 1e6 is a
    location and is NOT flagged"""
    K, N, D = 6, 40, P + C - 1
    inp, X = _inputs(K, N, P, C)
    opt = dict(maxiter=30, maxfun=60, gtol=1e-8)
    tgt = _target(inp)
    H0, cov0, info0 = _hess(tgt, X)
    st0 = _start(tgt, X, **opt)
    assert (st0["ist"][:, 0] != 4).all() and np.isfinite(H0).all()

    def only(k, Hn, covn, infon, stn):
        assert np.isnan(Hn[k]).all() and infon[k] == 1 and np.array_equal(covn[k], np.eye(D)) and stn["ist"][k, 0] == 4
        for j in range(K):
            if j != k:
                assert np.array_equal(Hn[j], H0[j]) and np.array_equal(covn[j], cov0[j]) and infon[j] == info0[j], j
                assert all(np.array_equal(stn[n][j], st0[n][j]) for n in ("x", "g", "d", "Xt", "sc", "ist")), j

    for k, j, val in ((2, 0, np.nan), (3, P + 1, 710.0), (4, D - 1, -740.0), (0, P, np.inf)):
        Xn = X.copy()
        Xn[k, j] = val
        only(k, *_hess(tgt, Xn), _start(tgt, Xn, **opt))
    Xn = X.copy()
    Xn[3, P] = 1e6
    Hn, covn, infon = _hess(tgt, Xn)
    stn = _start(tgt, Xn, **opt)
    assert np.isfinite(Hn[3]).all() and stn["ist"][3, 0] != 4 and np.isfinite(stn["sc"][3, 0])
    want = ref.neg_hessian(*inp, Xn, L=np.longdouble)
    assert (np.abs(Hn[3] - want[0][3]) <= 1e-11 * want[1][3]).all()


# ---- 5. every round of every trajectory -----------------------------------------------------------------------------------------------
def _upload(eng, packed):
    st = {k: eng.asarray(v).contiguous() for k, v in packed.items() if k != "ist"}
    st["ist"] = torch.as_tensor(packed["ist"], device=st["x"].device).contiguous()
    st["stopped"] = eng.new_flag()
    return st


def _download(st):
    return {k: v.cpu().numpy() for k, v in st.items()}


def _compare(got, recs, where):
    """integers (ist[4], the retried rounds, among them) equal, t equal, every other double within 1e-11 of its scale (zero where
    the launch writes nothing: the uploaded bits must come back); returns the largest share of a bound used"""
    want = ref.pack([a for _, a, _ in recs])
    assert np.array_equal(got["ist"], want["ist"]), (where, got["ist"][:, :5].tolist(), want["ist"][:, :5].tolist())
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


@pytest.mark.parametrize("shape", ref.STEP_SHAPES)
@pytest.mark.parametrize("near", [False, True])
def test_every_round_of_every_trajectory_matches_the_restatement(shape, near):
    """each round of each problem's trajectory (K = 5, gtol = 1e-6; margins, every pivot test by 1e-6 of its magnitudes among them,
    asserted in tests/test_ordinal_laplace_cpu.py and again here) is one problem of a launch: the restatement's state before it goes
    up, everything the launch leaves is compared with the restatement's state after it.  From x0 = 0 the retry rule fires at the
    shapes with C >= 8 (asserted from the CPU run, and ist[4] > 0 on the device); started near the mode it does not."""
    worst, nsteps = 0.0, 0
    for full in (True, False):
        traj = ref.trajectories(shape, near, full)
        ok, _, mar, nmod = ref.margins_hold(traj)
        assert ok and mar >= ref.MOD_MARGIN
        fires = shape in ref.RETRY_SHAPES and not near
        assert nmod == 0 if near else (nmod > 0 or not fires)
        inp = ref.step_inputs(shape, full, near)
        tgt = _target(inp, full)                                        # the first launch
        eng = tgt.engine
        st = eng.laplace_state_batched(eng.asarray(np.stack([x0 for _, _, _, x0 in traj])))
        eng.last_path(reset=True)
        eng.ordinal_laplace_step_batched(st, tgt.A, tgt.y, tgt.C, start=True, **OPT, **_model(tgt))
        assert eng.last_path(reset=True) == {"batched_laplace", "batched_target"}
        first = [rec[0] for _, _, rec, _ in traj]
        worst = max(worst, _compare(_download(st), first, (full, "start")))
        assert int(st["stopped"].item()) == sum(a["status"] != 0 for _, a, _ in first)
        recs, ks = [], []                                               # every later launch, and the frozen end states
        for k, end, rec, _ in traj:
            recs += rec[1:] + [(end, end, {})]
            ks += [k] * len(rec)
        tgt = _target(inp, full, sel=ks)
        before = ref.pack([b for b, _, _ in recs])
        st = _upload(eng, before)
        eng.ordinal_laplace_step_batched(st, tgt.A, tgt.y, tgt.C, **OPT, **_model(tgt))
        got = _download(st)
        worst = max(worst, _compare(got, recs, (full, "step")))
        nsteps += len(recs)
        assert int(st["stopped"].item()) == sum(a["status"] != 0 and b["status"] == 0 for b, a, _ in recs)
        frozen = before["ist"][:, 0] != 0
        assert frozen.sum() == len(traj)
        for name in ("x", "g", "d", "Xt", "sc", "ist"):
            assert np.array_equal(got[name][frozen], before[name][frozen], equal_nan=True), name
        if fires:
            assert got["ist"][:, 4].max() > 0
        if near:
            assert got["ist"][:, 4].max() == 0
    print(f"{shape} near={near}: {nsteps} rounds, worst share of 1e-11 scale used {worst:.3f}")


# ---- 6. frozen problems ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(70, 9, 8), (90, 40, 17)])
def test_stopped_problems_keep_every_bit_and_are_counted_once(shape):
    inp = ref.step_inputs(shape)
    tgt = _target(inp)
    eng = tgt.engine
    K, D = ref.STEP_K, shape[1] + shape[2] - 1
    st = eng.laplace_state_batched(eng.asarray(np.zeros((K, D))))
    traj = ref.trajectories(shape, False)
    want = [end for _, end, _, _ in traj]
    for r in range(max(e["nfev"] for e in want)):
        eng.ordinal_laplace_step_batched(st, tgt.A, tgt.y, tgt.C, start=r == 0, **OPT, **_model(tgt))
    assert int(st["stopped"].item()) == K
    done = _download(st)
    assert np.array_equal(done["ist"], ref.pack(want)["ist"])
    for _ in range(5):                                                  # everything is frozen: whole workgroups leave at once
        eng.ordinal_laplace_step_batched(st, tgt.A, tgt.y, tgt.C, **OPT, **_model(tgt))
    again = _download(st)
    for name in ("x", "g", "d", "Xt", "sc", "ist", "stopped"):
        assert np.array_equal(again[name], done[name], equal_nan=True), name
    # the f and g left in the state against the score kernel, an independent path, at the final points, with its own scales
    G, lp = tgt.lp_and_score(eng.asarray(done["x"][:, None, :]))
    G, lp = G.cpu().numpy()[:, 0, :], lp.cpu().numpy()[:, 0]
    for k in range(K):
        sc = ref.evaluate(ref.problem(*inp, k), done["x"][k])[3]
        assert abs(done["sc"][k, 0] + lp[k]) <= 1e-11 * sc["f"], k
        assert (np.abs(done["g"][k] + G[k]) <= 1e-11 * sc["g"]).all(), k
    # made-up stopped states of every code among running ones
    states = [dict(e) for e in want]
    for k, code in zip(range(1, K), (2, 3, 4, 5)):
        states[k]["status"] = code
    states[0] = traj[0][2][1][0]                                        # problem 0 before its second launch: running
    before = ref.pack(states)
    st = _upload(eng, before)
    eng.ordinal_laplace_step_batched(st, tgt.A, tgt.y, tgt.C, **OPT, **_model(tgt))
    got = _download(st)
    for name in ("x", "g", "d", "Xt", "sc", "ist"):
        assert np.array_equal(got[name][1:], before[name][1:], equal_nan=True), name
    assert got["ist"][0, 2] == before["ist"][0, 2] + 1 and int(st["stopped"].item()) == int(got["ist"][0, 0] != 0)


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c5", "c8"])
def test_end_to_end_at_the_defaults(name):
    """(N, P, C) = (64, 6, 5) and (70, 9, 8), lam = kap = 1, the 16 problems of the named set: every problem succeeds, nit, nfev and
    nmod are the restatement's, the score launch (an independent path) gives max|score| <= 1e-6 at the mean, cov inverts the
    restated Hessian"""
    import gsmvi_amd
    N, P, C = ref.SETS[name]
    K, D = ref.SET_K, P + C - 1
    inp = ref.make_problems(N, P, C)
    tgt = _target(inp)
    mean, cov, res = gsmvi_amd.laplace_init_ordinal_batched(tgt)
    want = ref.set_runs(name, True)
    assert isinstance(res, gsmvi_amd.LaplaceOrdinalBatchedResult)
    assert mean.shape == (K, D) and cov.shape == (K, D, D) and np.array_equal(mean, res.x) and res.nlaunch % 4 == 0
    assert res.success.all() and (res.status == 1).all() and (res.info == 0).all()
    assert res.nit.tolist() == [s["nit"] for s in want] and res.nfev.tolist() == [s["nfev"] for s in want]
    assert res.nmod.tolist() == [s["nmod"] for s in want] and res.nmod.max() > 0
    G = tgt.lp_g(tgt.engine.asarray(mean[:, None, :])).cpu().numpy()[:, 0, :]
    assert np.abs(G).max() <= 1e-6 and np.abs(res.jac).max() <= 1e-8
    Href = ref.neg_hessian(*inp, mean, L=np.longdouble)[0]
    share = max(_check_inverse(cov[k], Href[k], k) for k in range(K))
    print(f"{name}: nit {res.nit.tolist()}, nfev {res.nfev.tolist()}, nmod {res.nmod.tolist()}, max|score| {np.abs(G).max():.1e}, "
          f"share of 1e-11 cond used {share:.3f}")


def test_the_reported_cases():
    """a flat case: all counts 0 with kap = 0 (f = g = 0 at once, H = diag(lam, 0)): status 5, info != 0, no success, the
    identity.  lam = 0 on separable data (y decided by the sign of a_n . b): there is no mode; whatever the run ends with is
    reported consistently: success only with a positive definite Hessian that cov inverts, the identity otherwise."""
    import gsmvi_amd
    N, P, C, K = 64, 6, 3, 8
    A, y, o, _, _, _, _ = ref.make_problems(N, P, C, K=K)
    counts = np.full(K, N, dtype=np.int32)
    counts[0] = 0
    rs = np.random.RandomState(3)
    b = rs.standard_normal((K, P))
    score = np.einsum("knp,kp->kn", A, b) + o
    y = y.copy()
    y[1:] = (score[1:] > -0.3).astype(np.int64) + (score[1:] > 0.3)
    lam = np.zeros(K)
    lam[0] = 1.0
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, C, prior_precision=lam, cut_precision=0.0, counts=counts, offset=o)
    mean, cov, res = gsmvi_amd.laplace_init_ordinal_batched(tgt)
    D = P + C - 1
    assert res.status[0] == 5 and res.info[0] == P + 1 and not res.success[0] and np.array_equal(cov[0], np.eye(D))
    assert res.nit[0] == 0 and res.nfev[0] == 1 and not mean[0].any()
    print(f"separable data, lam = 0: status {res.status[1:].tolist()}, info {res.info[1:].tolist()}, nit {res.nit[1:].tolist()}, nmod "
          f"{res.nmod[1:].tolist()}, max|beta| {np.round(np.abs(mean[1:, :P]).max(1), 1).tolist()}")
    H = ref.neg_hessian(A, y, o, counts, lam, 0.0, C, mean, L=np.longdouble)[0]
    for k in range(1, K):
        assert res.success[k] == (res.status[k] == 1 and res.info[k] == 0)
        if res.success[k]:
            assert np.linalg.eigvalsh(H[k]).min() > 0
            if np.linalg.cond(H[k]) < 1e10:
                _check_inverse(cov[k], H[k], k)
        else:
            assert res.status[k] in (2, 3, 5) and np.array_equal(cov[k], np.eye(D))


def test_check_every_x0_and_as_torch():
    import gsmvi_amd
    N, P, C = ref.SETS["c5"]
    K, D = 6, P + C - 1
    inp = ref.make_problems(N, P, C, K=K)
    tgt = _target(inp)
    x0 = 0.1 * np.random.RandomState(3).standard_normal((K, D))
    runs = {c: gsmvi_amd.laplace_init_ordinal_batched(tgt, x0, check_every=c) for c in (1, 4, 1000)}
    for c in (1, 1000):
        assert np.array_equal(runs[c][0], runs[4][0]) and np.array_equal(runs[c][1], runs[4][1])
        for f in ("x", "fun", "jac", "nit", "nfev", "status", "info", "nmod"):
            assert np.array_equal(getattr(runs[c][2], f), getattr(runs[4][2], f)), (c, f)
    assert runs[4][2].success.all()
    assert runs[1][2].nlaunch == runs[1][2].nfev.max() and runs[1000][2].nlaunch == 200
    mt, ct_, _ = gsmvi_amd.laplace_init_ordinal_batched(tgt, x0, as_torch=True)
    assert mt.is_cuda and ct_.is_cuda and np.array_equal(mt.cpu().numpy(), runs[4][0]) and np.array_equal(ct_.cpu().numpy(), runs[4][1])
    one = gsmvi_amd.laplace_init_ordinal_batched(tgt, x0[2])
    assert np.array_equal(one[0][2], runs[4][0][2]) and np.array_equal(one[1][2], runs[4][1][2])
    mean, cov, res = gsmvi_amd.laplace_init_ordinal_batched(tgt, x0, maxiter=1)
    assert (res.status == 2).all() and not res.success.any() and np.array_equal(cov, np.broadcast_to(np.eye(D), (K, D, D)))
    for fn in (gsmvi_amd.laplace_init_batched, gsmvi_amd.laplace_init_softmax_batched, gsmvi_amd.laplace_init_negbin_batched):
        with pytest.raises(TypeError, match=fn.__name__):
            fn(tgt)
    assert not hasattr(tgt, "neg_hessian")


# ---- 8. as a start ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,C,B", [(4, 3, 2), (10, 7, 4)])
def test_it_starts_the_batched_fit_and_the_diagnostics(P, C, B):
    import gsmvi_amd
    K, N, D = 6, 12 * (P + C), P + C - 1
    inp = ref.make_problems(N, P, C, K=K)
    tgt = _target(inp)
    mean, cov, res = gsmvi_amd.laplace_init_ordinal_batched(tgt)
    assert res.success.all()
    keys = np.arange(K) + 7
    m1, c1 = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, mean=mean, cov=cov, batch_size=B, niter=50, verbose=False)
    assert np.isfinite(m1).all() and np.isfinite(c1).all()
    ps = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=256, moments=False)
    assert np.isfinite(ps.khat).all()
    loo = gsmvi_amd.psis_loo_ordinal_batched(tgt, mean, cov, keys, num_draws=256)
    assert np.isfinite(loo.elpd_loo).all()
    print(f"(P, C) = {(P, C)}: khat of the Laplace start {np.round(ps.khat, 2).tolist()}, elpd_loo {np.round(loo.elpd_loo, 1).tolist()}")


# ---- 9. bad arguments -------------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_with_nothing_enqueued():
    import gsmvi_amd
    from gsmvi_amd import _lib
    eng = gsmvi_amd.get_engine()
    eng.last_path(reset=True)
    ref.check_bad_arguments(_lib.load_library())
    assert eng.last_path(reset=True) == set()
