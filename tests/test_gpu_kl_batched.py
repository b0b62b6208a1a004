"""The batched KL monitor on the GPU (csrc/gsmvi_kl_batched.hip, BatchedKLMonitor): per-problem equality with DeviceKLMonitor,
the draws against the single-problem sampler, chunking, the closed-form KL, isolation of a bad problem, and the monitor
inside GSMBatch.fit / BaMBatch.fit (gsmvi/monitors.py:83-125 per problem)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOG2PI = np.log(2 * np.pi)


def _kl_gauss(m0, S0, m1, S1):
    D = m0.shape[0]
    iS1 = np.linalg.inv(S1)
    d = m1 - m0
    return 0.5 * (np.trace(iS1 @ S0) + d @ iS1 @ d - D + np.linalg.slogdet(S1)[1] - np.linalg.slogdet(S0)[1])


def _qstate(K, D, seed=0):
    rs = np.random.RandomState(seed)
    mean = rs.standard_normal((K, D))
    A = rs.standard_normal((K, D, D))
    return mean, A @ np.swapaxes(A, 1, 2) / D + 0.5 * np.eye(D)


def _targets(K, D, seed=1):
    from oracle import gsm_oracle as orc
    ms, covs, Ps = zip(*[orc.make_gaussian_target(D, 100 * seed + k) for k in range(K)])
    return np.array(ms), np.array(covs), np.array(Ps)


def _norms(covs):
    D = covs.shape[1]
    return np.array([-0.5 * D * LOG2PI - 0.5 * np.linalg.slogdet(c)[1] for c in covs])


def _batched_lp(ms, Ps, norms, seen=None):
    """normalised log N(x; m_k, P_k^-1) of the (K, rows, D) device tensor, (K, rows) values -- torch only, one problem at a time
    (the same ops for any K, so a problem's bits do not depend on its batch)"""
    import torch
    m_t, P_t = torch.as_tensor(ms, device="cuda"), torch.as_tensor(Ps, device="cuda")

    def lp(X):
        assert isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float64
        if seen is not None:
            seen.append(tuple(X.shape))
        out = []
        for k in range(X.shape[0]):
            r = X[k] - m_t[k][None, :]
            out.append(-0.5 * torch.einsum("bi,ij,bj->b", r, P_t[k], r) + float(norms[k]))
        return torch.stack(out)
    return lp


def _single_lp(m, P, norm):
    import torch
    m_t, P_t = torch.as_tensor(m, device="cuda"), torch.as_tensor(P, device="cuda")

    def lp(x):
        r = x - m_t[None, :]
        return (-0.5 * torch.einsum("bi,ij,bj->b", r, P_t, r) + norm).sum()
    return lp


def _host_fkl(Y, mean, cov, ms, Ps, norms):
    """(sum lp_k(y) - sum log q_k(y)) / rows for every k: oracle.gsm_oracle.gaussian_logp (+ the normalisation) and numpy"""
    from gsmvi_amd.monitors import mvn_logpdf
    from oracle import gsm_oracle as orc
    n = Y.shape[1]
    return np.array([(orc.gaussian_logp(Y[k], ms[k], Ps[k]) + n * norms[k] - mvn_logpdf(Y[k], mean[k], cov[k]).sum()) / n
                     for k in range(Y.shape[0])])


@pytest.mark.parametrize("D", [1, 5, 16, 17, 33, 64])
def test_each_problem_equals_the_device_monitor(D):
    import gsmvi_amd
    K, n, N = 37, 24, 300
    keys = [1000 + 7 * k for k in range(K - 1)] + [2 ** 40 + 3]
    mean, cov = _qstate(K, D)
    ms, covs, Ps = _targets(K, D)
    norms = _norms(covs)
    ref = np.stack([np.random.RandomState(5 + k).multivariate_normal(ms[k], covs[k], size=N) for k in range(K)])
    eng = gsmvi_amd.get_engine()
    mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=n, checkpoint=1, ref_samples=ref)
    singles = [gsmvi_amd.DeviceKLMonitor(batch_size_kl=n, checkpoint=1, ref_samples=ref[0] if k == 0 else None)
               for k in range(K)]
    md, cd = eng.asarray(mean), eng.asarray(cov)
    rs = np.random.RandomState(keys[0] % 2 ** 32)
    for c in range(2):
        assert mon(c, [md, cd], _batched_lp(ms, Ps, norms), keys, nevals=3) is keys
        for k in range(K):
            singles[k](c, [md[k], cd[k]], _single_lp(ms[k], Ps[k], norms[k]), keys[k], nevals=3)
        rkl, fkl = mon.rkl[c], mon.fkl[c]
        assert rkl.shape == (K,) and fkl.shape == (K,)
        for k in range(K):
            assert abs(rkl[k] - singles[k].rkl[c]) < 1e-9, (c, k, rkl[k], singles[k].rkl[c])
        assert abs(fkl[0] - singles[0].fkl[c]) < 1e-9
        idx = rs.permutation(N)[:n]
        np.testing.assert_allclose(fkl, _host_fkl(ref[:, idx], mean, cov, ms, Ps, norms), rtol=0, atol=1e-9)
    assert mon.nevals == [3, 6]


@pytest.mark.parametrize("D", [5, 17, 64])
def test_draws_are_the_single_problem_sampler_and_chunks_change_no_bit(D):
    import torch
    import gsmvi_amd
    K, n, c = 9, 24, 3
    mean, cov = _qstate(K, D, seed=2)
    eng = gsmvi_amd.get_engine()
    md, cd = eng.asarray(mean), eng.asarray(cov)
    seeds = [(k * 977 + 5) ^ 0x5DEECE66D for k in range(K)]
    st = eng.batched_seeds(seeds)
    X, logq, info = eng.kl_draw_batched(md, cd, st, c, 0, n)
    assert eng.read_ints(info).tolist() == [0] * K
    Xh = X.cpu().numpy()
    for k in range(K):
        R, flag = eng.potrf(cd[k])
        assert eng.read_flag(flag) == 0
        Z = eng.normal(n, D, seeds[k], c)
        ref = eng.sample(Z, md[k], R).cpu().numpy()
        assert np.abs(Xh[k] - ref).max() <= 1e-12 * np.abs(ref).max(), k
        Zh = Z.cpu().numpy()
        Rh = R.cpu().numpy()
        lq = -0.5 * np.sum(Zh * Zh) - n * np.sum(np.log(np.diag(Rh))) - 0.5 * n * D * LOG2PI
        assert abs(logq[k].item() - lq) < 1e-10 * max(1.0, abs(lq))
    for chunk in (1, 5, 7, 23):                              # s0 D odd for odd D: a Philox pair straddles two calls
        parts = [eng.kl_draw_batched(md, cd, st, c, s0, min(chunk, n - s0))[0] for s0 in range(0, n, chunk)]
        assert torch.equal(torch.cat(parts, dim=1), X), chunk


@pytest.mark.parametrize("D", [4, 8])
def test_against_the_closed_form_gaussian_kl(D):
    import gsmvi_amd
    K = 8
    ms, covs = _qstate(K, D, seed=3)                            # well-conditioned targets: KL(q || p) 0.3 - 1
    Ps = np.linalg.inv(covs)
    norms = _norms(covs)
    mq = ms + 0.3
    Sq = covs * 1.5 + 0.1 * np.eye(D)
    ref = np.stack([np.random.RandomState(3 + k).multivariate_normal(ms[k], covs[k], size=100000) for k in range(K)])
    mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=40000, checkpoint=1, ref_samples=ref)
    eng = gsmvi_amd.get_engine()
    mon(0, [eng.asarray(mq), eng.asarray(Sq)], _batched_lp(ms, Ps, norms), list(range(11, 11 + K)), nevals=5)
    for k in range(K):
        assert abs(mon.rkl[0][k] - _kl_gauss(mq[k], Sq[k], ms[k], covs[k])) < 3e-2, k
        assert abs(mon.fkl[0][k] - _kl_gauss(ms[k], covs[k], mq[k], Sq[k])) < 3e-2, k
    assert mon.nevals == [5]


@pytest.mark.parametrize("D", [5, 33])
def test_a_bad_problem_touches_no_other(D):
    """a non-PD and a NaN covariance, in the same workgroup as clean problems for D <= 16: NaN for those two alone, and every
    other problem's values bit-identical to the clean call and to a K = 1 call of that problem"""
    import gsmvi_amd
    K, n, N, bad = 12, 20, 64, (2, 5)
    keys = [11 + k * 2 ** 32 for k in range(K)]                 # one RandomState seed (keys[0]) for any subset of problems
    mean, cov = _qstate(K, D, seed=4)
    ms, covs, Ps = _targets(K, D, seed=5)
    norms = _norms(covs)
    ref = np.random.RandomState(6).standard_normal((K, N, D))
    poisoned = cov.copy()
    poisoned[bad[0]] = -np.eye(D)
    poisoned[bad[1], 0, 0] = np.nan
    eng = gsmvi_amd.get_engine()

    def run(mean, cov, ks):
        mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=n, ref_samples=ref[ks])
        for c in range(2):
            mon(c, [eng.asarray(mean[ks]), eng.asarray(cov[ks])], _batched_lp(ms[ks], Ps[ks], norms[ks]),
                [keys[k] for k in ks])
        return np.array(mon.rkl), np.array(mon.fkl)

    allk = list(range(K))
    rp, fp = run(mean, poisoned, allk)
    rc, fc = run(mean, cov, allk)
    good = [k for k in allk if k not in bad]
    assert np.isnan(rp[:, list(bad)]).all() and np.isnan(fp[:, list(bad)]).all()
    assert np.isfinite(rp[:, good]).all() and np.isfinite(fp[:, good]).all()
    assert np.array_equal(rp[:, good], rc[:, good]) and np.array_equal(fp[:, good], fc[:, good])
    for k in good[:4] + good[-2:]:
        r1, f1 = run(mean, cov, [k])
        assert np.array_equal(r1[:, 0], rp[:, k]) and np.array_equal(f1[:, 0], fp[:, k]), k


def _fit_setup(K, D, seed):
    import gsmvi_amd
    ms, covs, Ps = _targets(K, D, seed=seed)
    norms = _norms(covs)
    tgt = gsmvi_amd.BatchedGaussianTarget(ms, precision=Ps)
    norms_t = tgt.mean.new_tensor(norms)

    def lp(x):                                                  # BatchedGaussianTarget.lp, normalised: (K,) sums
        return tgt.lp(x) + norms_t * x.shape[1]
    ref = np.stack([np.random.RandomState(1 + k).multivariate_normal(ms[k], covs[k], size=4096) for k in range(K)])
    return ms, covs, tgt, lp, ref


def test_monitor_inside_the_gsm_batch_fit():
    import gsmvi_amd
    K, D, B, niter = 64, 8, 4, 600
    ms, covs, tgt, lp, ref = _fit_setup(K, D, 7)
    keys = list(range(300, 300 + K))
    mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=256, checkpoint=100, ref_samples=ref)
    mean, cov = gsmvi_amd.GSMBatch(K, D, lp, tgt.lp_g).fit(keys, batch_size=B, niter=niter, verbose=False, monitor=mon)
    m0, c0 = gsmvi_amd.GSMBatch(K, D, lp, tgt.lp_g).fit(keys, batch_size=B, niter=niter, verbose=False)
    assert np.array_equal(mean, m0) and np.array_equal(cov, c0)
    assert len(mon.rkl) == 8 and len(mon.fkl) == 8              # i = 0, 100, ..., 600 and the final call
    assert (mon.rkl[0] > 0.5).all()
    assert np.abs(mon.rkl[-1]).max() < 1e-8 and np.abs(mon.fkl[-1]).max() < 1e-8
    assert mon.nevals[:2] == [1, 401]


def test_monitor_inside_the_bam_batch_fit():
    import gsmvi_amd
    K, D, B, niter = 64, 8, 4, 600
    ms, covs, tgt, lp, ref = _fit_setup(K, D, 8)
    keys = list(range(500, 500 + K))
    mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=256, checkpoint=100, ref_samples=ref)
    regf = lambda i: 10.0                                       # noqa: E731
    mean, cov = gsmvi_amd.BaMBatch(K, D, lp, tgt.lp_g).fit(keys, regf, batch_size=B, niter=niter, verbose=False, monitor=mon)
    m0, c0 = gsmvi_amd.BaMBatch(K, D, lp, tgt.lp_g).fit(keys, regf, batch_size=B, niter=niter, verbose=False)
    assert np.array_equal(mean, m0) and np.array_equal(cov, c0)
    assert len(mon.rkl) == 8 and mon.nevals[:2] == [1, 401]
    r = np.array(mon.rkl)
    assert np.isfinite(r).all() and (r[-1] < r[0]).all()


def test_last_path_of_a_standalone_call_is_the_batched_kl_kernel():
    import gsmvi_amd
    K, D = 5, 6
    mean, cov = _qstate(K, D, seed=9)
    ms, covs, Ps = _targets(K, D, seed=9)
    seen = []
    eng = gsmvi_amd.get_engine()
    md, cd = eng.asarray(mean), eng.asarray(cov)
    mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=10, ref_samples=np.zeros((K, 20, D)))
    mon._CHUNK = 4
    eng.last_path(reset=True)
    mon(0, [md, cd], _batched_lp(ms, Ps, _norms(covs), seen), range(K))
    assert eng.last_path() == {"batched_kl"}
    assert seen == [(K, 4, D), (K, 4, D), (K, 2, D)] * 2        # DRAW chunks, then the EVAL chunks of the reference rows
    assert np.isfinite(mon.rkl[0]).all() and np.isfinite(mon.fkl[0]).all()
