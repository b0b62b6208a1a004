"""The batched Pathfinder initialiser on the GPU (csrc/gsmvi_pathfinder_batched.hip): the propose launch against the longdouble
restatement (tests/pathfinder_batched_ref.py) fed the device's own L-BFGS state, launch by launch, at every D, M and K at which
the kernel takes another path; the select launch bit for bit; the independence of the problems; and ``pathfinder_init_batched``
end to end against a hand-driven loop, ``lbfgs_init_batched`` and the exactness of the pair base on isotropic targets.

The bar of test 1 is 1000 times the largest distance of the float64 restatement from the longdouble one on the same inputs (the
rule of tests/test_gpu_psis_batched.py); the measured figures are in that test's docstring."""
import numpy as np
import pytest
import torch

import lbfgs_batched_ref as lref
import logistic_batched_ref as logref
import pathfinder_batched_ref as ref
import softmax_batched_ref as sref

pytestmark = pytest.mark.gpu

LBFGS = ("x", "g", "d", "Xt", "S", "Y", "sc", "ist")
PROPOSED = ("fresh", "seen", "mu", "cov", "X", "logq", "info")
BEST = ("best_elbo", "best_mean", "best_cov", "best_it", "npts", "elbo_last")


def _engine():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _np(d, names):
    return {n: d[n].cpu().numpy() for n in names}


def _quadratics(K, D, at_optimum=(0,)):
    """K quadratics of condition <= 100 and their starts: ones, except the problems ``at_optimum`` (status 1 at the first
    evaluation: frozen from then on, fresh once)"""
    funs = [ref.quadratic(D, seed=k) for k in range(K)]
    x0 = np.ones((K, D))
    for k in at_optimum:
        if k < K:
            x0[k] = funs[k].mean
    return funs, x0


def _evaluate(funs, Xt):
    vals = [f(x) for f, x in zip(funs, Xt)]
    return np.array([v[0] for v in vals]), np.stack([v[1] for v in vals])


def _walk(eng, funs, x0, rounds, **opt):
    """the device's L-BFGS states after each of ``rounds`` launches (the functions are evaluated on the host): yields the state"""
    st = eng.lbfgs_state_batched(eng.asarray(x0))
    for r in range(rounds):
        fv, gv = _evaluate(funs, st["Xt"].cpu().numpy())
        eng.lbfgs_step_batched(eng.asarray(fv), eng.asarray(gv), st, start=r == 0, sign=1.0, **opt)
        yield st


def _normals(eng, seeds, M, D):
    cache = {}

    def get(k, nit):
        key = (int(seeds[k]), int(nit))
        if key not in cache:
            cache[key] = eng.normal(M, D, key[0], call=key[1]).cpu().numpy()
        return cache[key]
    return get


# ---- 1. propose ----------------------------------------------------------------------------------------------------------------
CASES = [(D, 3, 5, 16) for D in ref.GPU_DS] + [(2, 3, 1, 3), (64, 3, 1, 3), (7, 3, 32, 4), (17, 3, 32, 4), (64, 3, 32, 12),
                                               (7, 1, 5, 4), (7, 130, 5, 4), (16, 130, 1, 3), (17, 130, 5, 3), (33, 1, 5, 4)]


def test_propose_matches_the_restatement_launch_by_launch():
    """Every launch of every case (D, K, M, rounds): the device's L-BFGS state goes through the propose launch and through the
    restatement in longdouble and in float64, fed the rows of the engine's ``normal`` stream.  fresh, seen, info equal; Sigma, mu,
    X (relative to the largest entry) and logq (relative to max(1, |value|)) within 1000 times the float64 restatement's own
    distance from the longdouble one, the worst over the grid; Sigma bitwise symmetric; with h0 = 1 Sigma is
    ``lbfgs_hess_inv_batched``'s; X and logq are ``kl_draw_batched``'s on (mu, cov) with call = nit.  A problem that is not fresh
    keeps mu and cov bit for bit, gets its point in every row of X and a NaN logq.
    Measured on the MI355X: worst error 9.9e-16 (Sigma), 2.9e-16 (mu), 1.8e-15 (X), 3.0e-14 (logq); the float64 restatement's own
    distance 9.6e-16, 3.4e-16, 1.1e-15, 2.1e-14, so a floor of 2.1e-14 and a bar of 2.1e-11; 0 ... 10 pairs held, 40 wrapped states,
    401 launches of a problem that was not fresh; h0 = 1 and the KL draw agree bit for bit."""
    eng = _engine()
    worst = {n: 0.0 for n in ("cov", "mu", "X", "logq")}
    floor = dict(worst)
    held, wrapped, nonfresh, bitwise = set(), 0, 0, True
    eng.last_path(reset=True)
    for D, K, M, rounds in CASES:
        funs, x0 = _quadratics(K, D)
        seeds_h = [1000 + 7 * k for k in range(K)]
        seeds = eng.batched_seeds(seeds_h)
        normals = _normals(eng, seeds_h, M, D)
        pf = eng.pathfinder_state_batched(eng.asarray(x0), M)
        for st in _walk(eng, funs, x0, rounds, gtol=1e-9, ftol=0.0):
            state, before = _np(st, LBFGS), _np(pf, PROPOSED)
            eng.pathfinder_propose_batched(st, pf, seeds)
            got = _np(pf, PROPOSED)
            after = _np(st, LBFGS)
            assert all(np.array_equal(after[n], state[n], equal_nan=True) for n in LBFGS), "the L-BFGS state is only read"
            want = ref.propose(state, before["seen"], normals, M)
            w64 = ref.propose(state, before["seen"], normals, M, dtype=np.float64)
            for n in ("fresh", "seen"):
                assert np.array_equal(got[n], want[n]), (D, K, M, n)
            fr = want["fresh"] != 0
            assert np.array_equal(got["info"][fr], want["info"][fr]) and not want["info"][fr].any(), (D, K, M)
            for k in range(K):
                if not fr[k]:
                    nonfresh += 1
                    assert np.array_equal(got["X"][k], np.broadcast_to(state["x"][k], (M, D))) and np.isnan(got["logq"][k])
                    for n in ("mu", "cov", "info"):
                        assert np.array_equal(got[n][k], before[n][k]), (D, K, M, k, n)
                    continue
                n_held, head = int(state["ist"][k, 4]), int(state["ist"][k, 5])
                held.add(n_held)
                wrapped += n_held == 10 and head != 0
                assert np.array_equal(got["cov"][k], got["cov"][k].T), (D, K, M, k)
                for n in ("cov", "mu", "X"):
                    worst[n] = max(worst[n], ref.rel_err(got[n][k], want[n][k]))
                    floor[n] = max(floor[n], ref.rel_err(w64[n][k], want[n][k]))
                worst["logq"] = max(worst["logq"], ref.rel_gap(got["logq"][k], want["logq"][k]))
                floor["logq"] = max(floor["logq"], ref.rel_gap(w64["logq"][k], want["logq"][k]))
            # the draws are the KL monitor's on (mu, cov), one call number at a time
            for nit in sorted(set(state["ist"][fr, 1].tolist())):
                sel = np.flatnonzero(fr & (state["ist"][:, 1] == nit))
                X2, lq2, info2 = eng.kl_draw_batched(pf["mu"], pf["cov"], seeds, int(nit), 0, M)
                a, b = (X2.cpu().numpy()[sel], lq2.cpu().numpy()[sel]), (got["X"][sel], got["logq"][sel])
                bitwise = bitwise and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                worst["X"] = max(worst["X"], max(ref.rel_err(a[0][i], want["X"][k]) for i, k in enumerate(sel)))
                worst["logq"] = max(worst["logq"], max(ref.rel_gap(a[1][i], want["logq"][k]) for i, k in enumerate(sel)))
                assert not info2.cpu().numpy()[sel].any()
            # the identity base: the dense product of the L-BFGS finish
            pf1 = eng.pathfinder_state_batched(eng.asarray(x0), M)
            eng.pathfinder_propose_batched(st, pf1, seeds, h0=1.0)
            c1, ch = pf1["cov"].cpu().numpy(), eng.lbfgs_hess_inv_batched(st).cpu().numpy()
            assert pf1["fresh"].cpu().numpy().all()
            bitwise = bitwise and np.array_equal(c1, ch)
            w1 = np.stack([np.asarray(ref.sigma(state["S"][k], state["Y"][k], state["sc"][k], state["ist"][k], h0=1.0)) for k in range(K)])
            for k in range(K):
                worst["cov"] = max(worst["cov"], ref.rel_err(c1[k], w1[k]), ref.rel_err(ch[k], w1[k]))
    assert eng.last_path(reset=True) >= {"batched_pathfinder"}
    bar = 1000.0 * max(floor.values())
    print(f"propose against the longdouble restatement: worst {worst}, float64 restatement's own distance {floor}, bar {bar:.2e}; "
          f"pairs held {sorted(held)}, wrapped {wrapped}, not fresh {nonfresh}, h0 = 1 and the KL draw bitwise: {bitwise}")
    assert held >= {0, 1, 3, 10} and wrapped > 0 and nonfresh > 0
    assert max(floor.values()) > 0.0
    for n, e in worst.items():
        assert e <= bar, (n, e, bar)


# ---- 2. select -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [7, 17])
def test_select_matches_the_restatement_bit_for_bit(D):
    """hand-built lpsum, logq, fresh and info over three launches: a tie (the first maximum stays), NaN, +inf and -inf candidates,
    info != 0, problems that are not fresh; K = 130 covers the tail slots at four problems per workgroup.  Copies and one
    subtract-divide: the best state, npts and elbo_last equal the numpy restatement bit for bit."""
    eng = _engine()
    K, M = 130, 4                                                         # (a power of two: e M / M is e, so ties can be built)
    rs = np.random.RandomState(D)
    st = {"ist": torch.zeros(K, 8, dtype=torch.int32, device=eng.device)}
    pf = eng.pathfinder_state_batched(eng.asarray(rs.standard_normal((K, D))), M)
    best = {n: pf[n].cpu().numpy() for n in BEST}
    for launch in range(3):
        lpsum, logq = rs.standard_normal(K) * 10.0, rs.standard_normal(K) * 10.0
        if launch == 1:                                                   # ties with the best so far: (lpsum - logq) / M exactly
            lpsum[:20], logq[:20] = best["best_elbo"][:20] * M, 0.0
            lpsum[:20] = np.where(np.isfinite(lpsum[:20]), lpsum[:20], 1.0)
        lpsum[20:23], lpsum[23:26], lpsum[26:29] = np.nan, np.inf, -np.inf
        logq[29:32] = np.nan
        fresh = (rs.random_sample(K) < 0.7).astype(np.int32)
        fresh[20:32] = 1
        info = np.where(rs.random_sample(K) < 0.1, 3, 0).astype(np.int32)
        nit = rs.randint(0, 50, size=K).astype(np.int32)
        if launch == 1:
            ties = (fresh[:20] != 0) & (info[:20] == 0) & np.isfinite(best["best_elbo"][:20])
            assert ties.any() and ((lpsum[:20] - logq[:20]) / M == best["best_elbo"][:20])[ties].all()
            kept = best["best_it"][:20].copy()
        mu, cov = rs.standard_normal((K, D)), rs.standard_normal((K, D, D))
        st["ist"][:, 1] = torch.as_tensor(nit, device=eng.device)
        for n, v in (("logq", logq), ("mu", mu), ("cov", cov)):
            pf[n].copy_(eng.asarray(v))
        for n, v in (("fresh", fresh), ("info", info)):
            pf[n].copy_(torch.as_tensor(v, device=eng.device))
        eng.last_path(reset=True)
        eng.pathfinder_select_batched(eng.asarray(lpsum), st, pf)
        assert eng.last_path(reset=True) == {"batched_pathfinder"}
        best = ref.select(lpsum, logq, fresh, info, nit, mu, cov, best, M)
        if launch == 1:
            assert np.array_equal(best["best_it"][:20][ties], kept[ties])  # a tie: the first maximum stays
        for n in BEST:
            assert np.array_equal(pf[n].cpu().numpy(), best[n], equal_nan=True), (launch, n)
        for n, v in (("logq", logq), ("mu", mu), ("cov", cov)):
            assert np.array_equal(pf[n].cpu().numpy(), v, equal_nan=True), n


# ---- 3. isolation and determinism ---------------------------------------------------------------------------------------------
def _propose_after(eng, D, sel, rounds, M=5, poison=None):
    """problems ``sel`` of the 130 quadratics after ``rounds`` L-BFGS launches, then one propose launch on fresh Pathfinder state"""
    funs, x0 = _quadratics(130, D)
    funs, x0 = [funs[k] for k in sel], x0[sel]
    seeds = eng.batched_seeds([1000 + 7 * k for k in sel])
    st = None
    for st in _walk(eng, funs, x0, rounds, gtol=1e-9, ftol=0.0):
        pass
    if poison is not None:
        poison(st)
    pf = eng.pathfinder_state_batched(eng.asarray(x0), M)
    eng.pathfinder_propose_batched(st, pf, seeds)
    return st, pf, seeds


@pytest.mark.parametrize("D", [7, 17])
def test_a_problem_alone_and_among_130_and_two_runs_give_the_same_bits(D):
    eng = _engine()
    _, among, _ = _propose_after(eng, D, list(range(130)), 5)
    _, again, _ = _propose_after(eng, D, list(range(130)), 5)
    _, alone, _ = _propose_after(eng, D, [77], 5)
    a, b, c = _np(among, PROPOSED), _np(again, PROPOSED), _np(alone, PROPOSED)
    assert a["fresh"].all() and not a["info"].any() and np.isfinite(a["logq"]).all()
    for n in PROPOSED:
        assert np.array_equal(a[n], b[n]), n
        assert np.array_equal(a[n][77], c[n][0]), n


@pytest.mark.parametrize("D", [7, 17])
def test_a_nan_gradient_or_pair_stays_in_its_own_problem(D):
    eng = _engine()

    def poison(st):
        st["g"][5, D // 2] = float("nan")
        slot = (int(st["ist"][6, 5]) - 1) % 10
        st["Y"][6, slot, 0] = float("nan")
    _, clean, _ = _propose_after(eng, D, list(range(130)), 5)
    _, dirty, _ = _propose_after(eng, D, list(range(130)), 5, poison=poison)
    a, b = _np(clean, PROPOSED), _np(dirty, PROPOSED)
    for k in (5, 6):
        assert b["fresh"][k] == 1 and (b["info"][k] != 0 or np.isnan(b["logq"][k])), k
        assert np.isnan(b["logq"][k]) and np.isnan(b["X"][k]).all()
    keep = np.setdiff1d(np.arange(130), [5, 6])
    for n in PROPOSED:
        assert np.array_equal(a[n][keep], b[n][keep]), n


def test_a_problem_that_is_not_fresh_keeps_every_bit_over_further_launches():
    eng = _engine()
    D, M = 17, 5
    st, pf, seeds = _propose_after(eng, D, list(range(6)), 4)
    lp = eng.asarray(np.linspace(-3.0, 2.0, 6))
    eng.pathfinder_select_batched(lp, st, pf)
    before = _np(pf, PROPOSED + BEST)
    assert before["fresh"].all() and (before["best_it"] >= 0).all()
    for _ in range(3):
        eng.pathfinder_propose_batched(st, pf, seeds)
        eng.pathfinder_select_batched(eng.asarray(np.full(6, 1e6)), st, pf)
    after = _np(pf, PROPOSED + BEST)
    assert not after["fresh"].any() and np.isnan(after["logq"]).all() and np.isnan(after["elbo_last"]).all()
    assert np.array_equal(after["X"], np.broadcast_to(st["x"].cpu().numpy()[:, None, :], (6, M, D)))
    for n in ("seen", "mu", "cov", "info", "best_elbo", "best_mean", "best_cov", "best_it", "npts"):
        assert np.array_equal(after[n], before[n]), n


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------
def _logistic(K=8, N=64, D=10):
    import gsmvi_amd
    A, y, counts, lam, _ = logref.make_inputs(K + 1, N, D, 1)
    return gsmvi_amd.BatchedLogisticTarget(A[1:], y[1:], prior_precision=lam[1:], counts=counts[1:])


def _softmax(K=8, N=64, C=3, P=5):
    import gsmvi_amd
    A, y, counts, lam, _ = sref.make_inputs(K + 1, N, C, P, 1)
    return gsmvi_amd.BatchedSoftmaxTarget(A[1:], y[1:], C, prior_precision=lam[1:], counts=counts[1:])


def test_the_driver_is_the_hand_driven_loop_and_its_best_is_the_first_argmax():
    """score, lp, step, propose, lp, select by hand from the engine methods, every fresh ELBO recorded: the final best state is
    the first argmax of the record, bit for bit; ``pathfinder_init_batched`` returns the same bits for check_every 1 and 8, and
    its L-BFGS fields are ``lbfgs_init_batched``'s"""
    import gsmvi_amd
    from gsmvi_amd.monitors import lp_sums
    eng = _engine()
    tgt = _logistic()
    K, D, M, seed = tgt.K, tgt.D, 5, 3
    x0 = 0.1 * np.random.RandomState(1).standard_normal((K, D))
    st = eng.lbfgs_state_batched(eng.asarray(x0))
    pf = eng.pathfinder_state_batched(st["x"], M)
    seeds = eng.batched_seeds([seed + k for k in range(K)])
    Xt, G = st["Xt"].reshape(K, 1, D), eng.empty(K, 1, D)
    record = []
    for r in range(1, 200):
        tgt.lp_g(Xt, out=G)
        v = lp_sums(tgt.lp, Xt, eng, K)
        eng.lbfgs_step_batched(v.contiguous(), G.reshape(K, D), st, start=r == 1, sign=-1.0)
        eng.pathfinder_propose_batched(st, pf, seeds)
        eng.pathfinder_select_batched(lp_sums(tgt.lp, pf["X"], eng, K).contiguous(), st, pf)
        record.append((_np(pf, ("fresh", "elbo_last", "mu", "cov")), st["ist"][:, 1].cpu().numpy()))
        if eng.read_flag(st["stopped"]) == K:
            break
    assert eng.read_flag(st["stopped"]) == K
    best = _np(pf, BEST)
    for k in range(K):
        elbos = np.array([rec["elbo_last"][k] if rec["fresh"][k] and np.isfinite(rec["elbo_last"][k]) else -np.inf for rec, _ in record])
        i = int(np.argmax(elbos))                                         # the first maximum
        assert best["best_elbo"][k] == elbos[i] and best["best_it"][k] == record[i][1][k], k
        assert np.array_equal(best["best_mean"][k], record[i][0]["mu"][k]) and np.array_equal(best["best_cov"][k], record[i][0]["cov"][k])
        assert best["npts"][k] == sum(int(rec["fresh"][k]) for rec, _ in record) == int(st["ist"][k, 1]) + 1
    plain = gsmvi_amd.lbfgs_init_batched(x0, tgt.lp, tgt.lp_g)[2]
    for c in (1, 8):
        mean, cov, res = gsmvi_amd.pathfinder_init_batched(x0, tgt.lp, tgt.lp_g, num_elbo_draws=M, seed=seed, check_every=c)
        assert np.array_equal(mean, best["best_mean"]) and np.array_equal(cov, best["best_cov"]), c
        assert np.array_equal(res.elbo, best["best_elbo"]) and np.array_equal(res.best_it, best["best_it"])
        assert np.array_equal(res.n_points, best["npts"]) and res.success.all() and res.nevals == res.nlaunch * (1 + M)
        for n in ("x", "fun", "jac", "nit", "nfev", "status"):
            assert np.array_equal(getattr(res, n), getattr(plain, n)), (c, n)
        assert res.nlaunch == (plain.nlaunch if c == 8 else plain.nfev.max())


@pytest.mark.parametrize("D", [1, 5, 17])
def test_the_pair_base_is_exact_on_isotropic_targets(D):
    """N(m, var I) through ``BatchedGaussianTarget`` (lp(m) = 0): the ELBO of path point 1 is D / 2 log(2 pi var) whatever the draws
    are (derived in tests/test_pathfinder_batched_cpu.py), to 1e-11 relative to max(1, |value|)"""
    import gsmvi_amd
    from gsmvi_amd.monitors import lp_sums
    eng = _engine()
    K, M = 3, 5
    for var in (0.25, 1.0, 9.0):
        means, x0 = ref.isotropic(K, D, var)
        tgt = gsmvi_amd.BatchedGaussianTarget(means, cov=np.broadcast_to(var * np.eye(D), (K, D, D)))
        st = eng.lbfgs_state_batched(eng.asarray(x0))
        pf = eng.pathfinder_state_batched(st["x"], M)
        seeds = eng.batched_seeds([5 + k for k in range(K)])
        Xt = st["Xt"].reshape(K, 1, D)
        for r in (1, 2):
            G = tgt.lp_g(Xt)
            eng.lbfgs_step_batched(lp_sums(tgt.lp, Xt, eng, K).contiguous(), G.reshape(K, D), st, start=r == 1, sign=-1.0)
            eng.pathfinder_propose_batched(st, pf, seeds)
            eng.pathfinder_select_batched(lp_sums(tgt.lp, pf["X"], eng, K).contiguous(), st, pf)
        assert (st["ist"][:, 1].cpu().numpy() == 1).all() and pf["fresh"].cpu().numpy().all()
        got, want = pf["elbo_last"].cpu().numpy(), ref.isotropic_elbo(D, var)
        err = np.abs(got - want).max() / max(1.0, abs(want))
        print(f"D = {D}, var = {var}: ELBO of path point 1 {got.tolist()} against {want!r}: {err:.2e}")
        assert err <= 1e-11, (D, var, got, want)
        assert ref.rel_gap(pf["cov"].cpu().numpy(), np.broadcast_to(var * np.eye(D), (K, D, D))) <= 1e-11


@pytest.mark.parametrize("kind", ["logistic", "softmax"])
def test_it_starts_the_batched_fit_on_logistic_and_softmax_posteriors(kind):
    import gsmvi_amd
    tgt = _logistic() if kind == "logistic" else _softmax()
    K, D = tgt.K, tgt.D
    mean, cov, res = gsmvi_amd.pathfinder_init_batched(np.zeros((K, D)), tgt.lp, tgt.lp_g)
    assert np.isfinite(res.elbo).all() and res.success.all() and (res.best_it >= 0).all() and np.isfinite(mean).all()
    for k in range(K):
        assert np.array_equal(cov[k], cov[k].T) and np.linalg.eigvalsh(cov[k]).min() > 0.0, k
    gsm = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g)
    m1, c1 = gsm.fit(np.arange(K) + 7, mean=mean, cov=cov, batch_size=2, niter=5, verbose=False)
    assert np.isfinite(m1).all() and np.isfinite(c1).all() and not np.asarray(gsm.n_reverts).any()
    print(f"{kind}: elbo {res.elbo.tolist()}, best_it {res.best_it.tolist()} of nit {res.nit.tolist()}")


# ---- 5. the path bit and the LDS request ----------------------------------------------------------------------------------------
def test_both_entries_set_the_path_bit_and_the_lds_stays_below_64_kb():
    import ctypes
    from gsmvi_amd import _lib
    eng = _engine()
    st, pf, seeds = _propose_after(eng, 7, [1, 2], 2)
    eng.last_path(reset=True)
    eng.pathfinder_propose_batched(st, pf, seeds)
    assert eng.last_path(reset=True) == {"batched_pathfinder"}
    eng.pathfinder_select_batched(eng.asarray(np.zeros(2)), st, pf)
    assert eng.last_path(reset=True) == {"batched_pathfinder"}
    lib = ctypes.CDLL(_lib.library_path(debug=True))
    fn = lib.gsmvi_debug_pathfinder_batched_lds
    fn.restype, fn.argtypes = _lib._DEBUG_SIGS["gsmvi_debug_pathfinder_batched_lds"]
    for D in range(1, 65):
        nbytes, ppw, tr = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0)
        assert fn(D, ctypes.byref(nbytes), ctypes.byref(ppw), ctypes.byref(tr)) == 0 and 0 < nbytes.value < 64 * 1024
