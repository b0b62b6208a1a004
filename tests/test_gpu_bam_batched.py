"""Batched BaM on the GPU (csrc/gsmvi_bam_batched.hip): one-shot parity with the per-problem oracle and the defining equation,
the reference's loop on forced samples, equality with the single dense BaM.fit, independence of the problems, per-problem
reverts, bounds and types."""
import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu


def _orc():
    from oracle import gsm_oracle as orc
    from oracle import bam_oracle as borc
    return orc, borc


def _states(K, B, D, seed):
    """random one-shot inputs: S0 = A A^T / D + 0.1 I, samples around mu0, arbitrary scores"""
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((K, D, D))
    S0 = A @ np.swapaxes(A, 1, 2) / D + 0.1 * np.eye(D)
    S0 = 0.5 * (S0 + np.swapaxes(S0, 1, 2))
    mu0 = rs.standard_normal((K, D))
    X = mu0[:, None, :] + rs.standard_normal((K, B, D))
    V = -0.5 * (X - rs.standard_normal((K, 1, D)))
    return X, V, mu0, S0


def _uv(X, G, mu0, S0, reg):
    """U, V of bam.py:50-60 and the batch means"""
    B = X.shape[0]
    xbar, gbar = X.mean(0), G.mean(0)
    xd, gd = X - xbar, G - gbar
    r1 = reg / (1 + reg)
    U = reg * gd.T @ gd / B + r1 * np.outer(gbar, gbar)
    V = S0 + reg * xd.T @ xd / B + r1 * np.outer(mu0 - xbar, mu0 - xbar)
    return U, V, xbar, gbar


def _backward_error(S, U, V):
    n2 = lambda M: np.linalg.norm(M, 2)
    return n2(S @ U @ S + S - V) / (n2(S) ** 2 * n2(U) + n2(S) + n2(V))


@pytest.mark.parametrize("D", [1, 2, 5, 7, 10, 16, 17, 31, 32, 33, 63, 64])
def test_one_shot_matches_the_per_problem_oracle(D):
    """shapes, paths and types on easy states at a fixed bar; accuracy at the float64 floor: tests/test_gpu_batched_hard.py"""
    import gsmvi_amd
    _, borc = _orc()
    eng = gsmvi_amd.get_engine()
    for B in sorted({1, 2, 5, 8, 32, min(D + 3, 32)}):
        for n, (per_problem, jitter) in enumerate(((False, 0.0), (True, 0.0), (False, 1e-6), (True, 1e-6))):
            K = 3 if n % 2 else 4
            X, V, mu0, S0 = _states(K, B, D, 1000 * D + 10 * B + n)
            regs = np.array([0.3, 1.0, 7.5, 100.0])[:K] if per_problem else np.full(K, 2.5)
            as_torch = n == 1
            args = [torch.tensor(a, device="cuda") for a in (X, V, mu0, S0)] if as_torch else [a.copy() for a in (X, V, mu0, S0)]
            reg = (torch.tensor(regs, device="cuda") if as_torch else regs) if per_problem else 2.5
            eng.last_path(reset=True)
            mu, S = gsmvi_amd.bam_update_batched(*args, reg, jitter=jitter)
            assert eng.last_path(reset=True) == {"batched_bam"}      # the batched kernel alone: no loop over single problems
            if as_torch:
                assert isinstance(mu, torch.Tensor) and mu.is_cuda
                mu, S = mu.cpu().numpy(), S.cpu().numpy()
                args = [a.cpu().numpy() for a in args]
            else:
                assert isinstance(mu, np.ndarray) and mu.dtype == np.float64
            for a, b in zip(args, (X, V, mu0, S0)):
                assert np.array_equal(a, b)                          # inputs untouched
            assert mu.shape == (K, D) and S.shape == (K, D, D)
            for k in range(K):
                assert np.array_equal(S[k], S[k].T)
                Sk = S[k] - jitter * np.eye(D)
                mo, So = borc.bam_lowrank_update_exact(X[k], V[k], mu0[k], S0[k], regs[k])
                assert rel_err(mu[k], mo) <= 1e-8 and rel_err(Sk, 0.5 * (So + So.T)) <= 1e-8, (D, B, n, k)
                U, Vm, xbar, gbar = _uv(X[k], V[k], mu0[k], S0[k], regs[k])
                assert _backward_error(Sk, U, Vm) < 1e-14, (D, B, n, k)
                mu_def = mu0[k] / (1 + regs[k]) + regs[k] / (1 + regs[k]) * (Sk @ gbar + xbar)
                assert rel_err(mu[k], mu_def) < 1e-8, (D, B, n, k)


def test_one_shot_failure_stays_in_its_slice():
    import gsmvi_amd
    K, D, B, bad = 6, 9, 3, 4
    X, V, mu0, S0 = _states(K, B, D, 3)
    V[bad, 1, 2] = np.nan
    eng = gsmvi_amd.get_engine()
    info = eng.batched_ints(K)
    mu, S = eng.bam_update_batched(*(eng.asarray(a) for a in (X, V, mu0, S0)), 1.5, 0.0, info=info)
    assert eng.read_ints(info).tolist() == [int(k == bad) for k in range(K)]
    mu, S = mu.cpu().numpy(), S.cpu().numpy()
    assert np.isnan(mu[bad]).all() and np.isnan(S[bad]).all()
    keep = [k for k in range(K) if k != bad]
    mu_c, S_c = gsmvi_amd.bam_update_batched(X[keep], V[keep], mu0[keep], S0[keep], 1.5)
    assert np.array_equal(mu[keep], mu_c) and np.array_equal(S[keep], S_c)


def test_unconverged_square_root_fails_its_problem_alone():
    """A chain whose Newton-Schulz bound does not close in its 32 steps (trace(N + I/4) beyond ~1e21: scores ~1e11 at
    reg = 100) is a failure, as gsmvi_bam_update_f64 flags it: UPDATE gives info = 1 and NaN for that problem, STEP reverts
    it; the other problems are untouched."""
    import gsmvi_amd
    K, D, B, bad, reg = 5, 6, 3, 2, 100.0
    X, V, mu0, S0 = _states(K, B, D, 21)
    V[bad] *= 1e11
    U, _, _, _ = _uv(X[bad], V[bad], mu0[bad], S0[bad], reg)
    assert np.trace(S0[bad] @ U) > 1e22                      # trace(N0) alone, a lower bound of trace(N + I/4)
    eng = gsmvi_amd.get_engine()
    _, _, flag = eng.bam_update(*(eng.asarray(a[bad]) for a in (X, V, mu0, S0)), reg, 0.0)
    assert eng.read_flag(flag) == 1                          # the single update flags this input
    Xd, Vd, m0d, S0d = (eng.asarray(a) for a in (X, V, mu0, S0))
    info = eng.batched_ints(K)
    mu, S = eng.bam_update_batched(Xd, Vd, m0d, S0d, reg, 1e-6, info=info)
    assert eng.read_ints(info).tolist() == [int(k == bad) for k in range(K)]
    mu, S = mu.cpu().numpy(), S.cpu().numpy()
    assert np.isnan(mu[bad]).all() and np.isnan(S[bad]).all()
    keep = [k for k in range(K) if k != bad]
    mu_c, S_c = gsmvi_amd.bam_update_batched(X[keep], V[keep], mu0[keep], S0[keep], reg, jitter=1e-6)
    assert np.array_equal(mu[keep], mu_c) and np.array_equal(S[keep], S_c)
    mean, cov, n_rev = eng.asarray(mu0), eng.asarray(S0), eng.batched_ints(K)
    eng.bam_fit_step_batched(Xd, Vd, mean, cov, None, reg, 1e-6, info, n_rev)
    assert eng.read_ints(n_rev).tolist() == [int(k == bad) for k in range(K)] and eng.read_ints(info)[bad] != 0
    mean, cov = mean.cpu().numpy(), cov.cpu().numpy()
    assert np.array_equal(mean[bad], mu0[bad]) and np.array_equal(cov[bad], S0[bad])
    assert np.array_equal(mean[keep], mu_c) and np.array_equal(cov[keep], S_c)


def _targets(K, D, seed, cond=3.0):
    """well-conditioned Gaussian targets: means U(0, 1)^D, covariance spectra log-spaced in [1, cond], random eigenvectors"""
    ms, covs, Ps = np.zeros((K, D)), np.zeros((K, D, D)), np.zeros((K, D, D))
    for k in range(K):
        rs = np.random.RandomState(seed + k)
        Q, _ = np.linalg.qr(rs.standard_normal((D, D)))
        c = (Q * np.logspace(0.0, np.log10(cond), D)) @ Q.T
        covs[k] = 0.5 * (c + c.T)
        ms[k], Ps[k] = rs.random_sample(D), np.linalg.inv(covs[k])
    return ms, covs, Ps


@pytest.mark.parametrize("D,B", [(5, 2), (10, 2), (16, 8), (33, 4)])
def test_forced_samples_follow_the_reference_loop(D, B):
    """bam.py:189-212 per problem on the same samples (jitter 1e-6): oracle/bam_oracle.py::bam_fit with its default update,
    as test_gpu_bam.py::test_default_fit_is_the_reference_loop does for the single fit; per-problem regularisers"""
    import gsmvi_amd
    orc, borc = _orc()
    K, niter = 6, 30
    ms, covs, Ps = _targets(K, D, 5 * D)
    forced = ms[None, :, None, :] + np.random.RandomState(D).standard_normal((niter + 1, K, B, D))
    base = np.array([100.0, 30.0, 10.0, 3.0, 1.0, 0.5])
    calls = []

    def regf(i):
        calls.append(i)
        return base / (1.0 + i)

    def lp_g(X):
        return np.stack([orc.gaussian_score(X[k], ms[k], Ps[k]) for k in range(K)])

    fit = gsmvi_amd.BaMBatch(K, D, None, lp_g)
    mean, cov = fit.fit(range(K), regf, batch_size=B, niter=niter, verbose=False, forced_samples=forced)
    assert calls == list(range(niter + 1)) and fit.n_reverts.tolist() == [0] * K
    for k in range(K):
        mo, co = borc.bam_fit(D, None, lambda x, k=k: orc.gaussian_score(x, ms[k], Ps[k]), 0, lambda i, k=k: base[k] / (1.0 + i),
                              batch_size=B, niter=niter, forced_samples=forced[:, k], jitter=1e-6)
        assert rel_err(mean[k], mo) <= 1e-7 and rel_err(cov[k], co) <= 1e-7, k


@pytest.mark.parametrize("D,B", [(5, 2), (10, 2), (32, 8), (64, 8)])
def test_each_problem_equals_the_single_dense_fit(D, B):
    """Problem k after 100 iterations equals BaM.fit(keys[k], method="dense", rng="device") of its own target (same draws,
    same regulariser schedule), and by then it has converged to its target."""
    import gsmvi_amd
    K, niter = 8, 100
    ms, covs, Ps = _targets(K, D, 7 * D)
    keys = [31 * k + 5 for k in range(K)]
    tgt = gsmvi_amd.BatchedGaussianTarget(ms, precision=Ps)
    fit = gsmvi_amd.BaMBatch(K, D, tgt.lp, tgt.lp_g)
    mean, cov = fit.fit(keys, gsmvi_amd.Regularizers().custom(lambda c: 100.0 / c), batch_size=B, niter=niter, verbose=False)
    assert fit.n_reverts.tolist() == [0] * K
    for k in range(K):
        t1 = gsmvi_amd.GaussianTarget(ms[k], precision=Ps[k])
        bam = gsmvi_amd.BaM(D, t1.lp, t1.lp_g)
        m1, c1 = bam.fit(keys[k], gsmvi_amd.Regularizers().custom(lambda c: 100.0 / c), batch_size=B, niter=niter,
                         verbose=False, method="dense", rng="device")
        assert bam.n_reverts == 0
        assert rel_err(mean[k], m1) < 1e-8 and rel_err(cov[k], c1) < 1e-8, (k, rel_err(mean[k], m1), rel_err(cov[k], c1))
        # converged: what is left is the jitter the loop adds every iteration (~niter * 1e-6 on the diagonal at most)
        assert rel_err(mean[k], ms[k]) < 1e-3 and rel_err(cov[k], covs[k]) < 1e-3, (k, rel_err(mean[k], ms[k]),
                                                                                 rel_err(cov[k], covs[k]))


@pytest.mark.parametrize("D,B", [(10, 2), (12, 16), (33, 4)])
def test_problem_is_independent_of_its_batch(D, B):
    """the same bits alone, in slot 5 of 16 and in slot 778 of 1024 (neighbours with other targets, keys and regularisers, so
    other Newton-Schulz step counts in the same workgroup when four problems share one: D <= 16), and from run to run"""
    import gsmvi_amd
    niter, key = 40, 424242
    ms, covs, Ps = _targets(1024, D, 3)
    rbase = 0.5 + np.arange(1024) % 13
    mine = (ms[0].copy(), Ps[0].copy())
    results = []
    for K, slot, run in ((1, 0, 0), (16, 5, 0), (1024, 778, 0), (1024, 778, 1)):
        m, P, r = ms[:K].copy(), Ps[:K].copy(), rbase[:K].copy()
        m[[0, slot]], P[[0, slot]], r[[0, slot]] = m[[slot, 0]], P[[slot, 0]], r[[slot, 0]]
        assert np.array_equal(m[slot], mine[0])
        keys = np.arange(K) + 17
        keys[slot] = key
        tgt = gsmvi_amd.BatchedGaussianTarget(m, precision=P)
        mean, cov = gsmvi_amd.BaMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, lambda i, r=r: r * 10.0 / (1 + i), batch_size=B,
                                                                   niter=niter, verbose=False)
        results.append((mean[slot], cov[slot], mean, cov))
    for mean_k, cov_k, _, _ in results[1:]:
        assert np.array_equal(mean_k, results[0][0]) and np.array_equal(cov_k, results[0][1])
    assert np.array_equal(results[2][2], results[3][2]) and np.array_equal(results[2][3], results[3][3])   # run to run, K = 1024


@pytest.mark.parametrize("D,B", [(6, 2), (20, 5)])
def test_nan_score_reverts_one_problem_bit_for_bit(D, B):
    import gsmvi_amd
    orc, _ = _orc()
    K, niter, bad = 8, 25, 3
    ms, covs, Ps = _targets(K, D, 11)
    rs = np.random.RandomState(2)
    mean0 = rs.standard_normal((K, D))
    cov0 = np.stack([np.eye(D) * (0.5 + k / K) for k in range(K)])

    def clean(X):
        return np.stack([orc.gaussian_score(X[k], ms[k], Ps[k]) for k in range(K)])

    def poisoned(X):
        G = clean(X)
        G[bad] = np.nan
        return G

    f0, f1 = gsmvi_amd.BaMBatch(K, D, None, clean), gsmvi_amd.BaMBatch(K, D, None, poisoned)
    m0, c0 = f0.fit(range(K), gsmvi_amd.Regularizers().linear(50.0), mean=mean0, cov=cov0, batch_size=B, niter=niter,
                    verbose=False)
    m1, c1 = f1.fit(range(K), gsmvi_amd.Regularizers().linear(50.0), mean=mean0, cov=cov0, batch_size=B, niter=niter,
                    verbose=False)
    assert f0.n_reverts.tolist() == [0] * K
    assert f1.n_reverts.tolist() == [niter + 1 if k == bad else 0 for k in range(K)]
    assert np.array_equal(m1[bad], mean0[bad]) and np.array_equal(c1[bad], cov0[bad])
    keep = [k for k in range(K) if k != bad]
    assert np.array_equal(m1[keep], m0[keep]) and np.array_equal(c1[keep], c0[keep])


def test_paths_bounds_and_types():
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    with pytest.raises(ValueError, match="D = 65"):
        gsmvi_amd.bam_update_batched(*_states(2, 2, 65, 0), 1.0)
    with pytest.raises(ValueError, match="B = 33"):
        gsmvi_amd.bam_update_batched(*_states(2, 33, 8, 0), 1.0)
    with pytest.raises(ValueError, match="3 values"):
        gsmvi_amd.bam_update_batched(*_states(2, 2, 8, 0), np.ones(3))
    with pytest.raises(ValueError, match="D = 65"):
        gsmvi_amd.BaMBatch(2, 65, None, lambda X: -X)
    with pytest.raises(ValueError, match="B = 33"):
        gsmvi_amd.BaMBatch(2, 8, None, lambda X: -X).fit([1, 2], lambda i: 1.0, batch_size=33, niter=2, verbose=False)
    cov = np.broadcast_to(np.eye(4), (6, 4, 4)).copy()
    cov[4] = -np.eye(4)
    with pytest.raises(ValueError, match=r"\[4\]"):
        gsmvi_amd.BaMBatch(6, 4, None, lambda X: -X).fit(range(6), lambda i: 1.0, cov=cov, niter=2, verbose=False)
    K, D, B = 5, 8, 4
    ms, covs, Ps = _targets(K, D, 90)
    tgt = gsmvi_amd.BatchedGaussianTarget(ms, cov=covs)
    eng.last_path(reset=True)
    mean, cov = gsmvi_amd.BaMBatch(K, D, tgt.lp, tgt.lp_g).fit(torch.arange(K), lambda i: 10.0 / (1 + i), batch_size=B,
                                                               niter=20, verbose=False, as_torch=True)
    used = eng.last_path(reset=True)
    assert "batched_bam" in used and not any(p.endswith("_generic") for p in used), used
    assert isinstance(mean, torch.Tensor) and mean.is_cuda and cov.shape == (K, D, D)
    X, V, mu0, S0 = (torch.tensor(a, device="cuda") for a in _states(K, B, D, 1))
    mu, S = gsmvi_amd.bam_lowrank_update_batched(X, V, mu0, S0, torch.linspace(0.5, 2.0, K, dtype=torch.float64))
    assert isinstance(mu, torch.Tensor) and mu.is_cuda and S.shape == (K, D, D)
    with pytest.raises(TypeError, match="monitor"):
        gsmvi_amd.BaMBatch(K, D, tgt.lp, tgt.lp_g).fit(range(K), lambda i: 1.0, niter=2, verbose=False, monitor=object())
