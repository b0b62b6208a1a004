"""Batched ADVI on the GPU (csrc/gsmvi_advi_batched.hip), each through the C ABI: one step, the init and the covariance against
the numpy restatement (tests/advi_batched_ref.py), 501 chained iterations of ADVIBatch.fit against the restatement's loop and
against torch autograd + torch.optim.Adam, independence of the problems bit for bit, determinism, the path bit, the monitor."""
import numpy as np
import pytest
import torch

import advi_batched_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

DS = [1, 2, 5, 7, 10, 16, 17, 31, 32, 33, 63, 64]


def _state(K, D, B, seed):
    """a random mid-fit state: L with a diagonal away from zero (both signs), non-zero moments, scores"""
    rs = np.random.RandomState(seed)
    P = ref.tri(D)
    scales = 0.3 * rs.standard_normal((K, P))
    diag = np.cumsum(np.arange(1, D + 1)) - 1
    scales[:, diag] = (0.5 + rs.random_sample((K, D))) * np.where(rs.random_sample((K, D)) < 0.2, -1.0, 1.0)
    loc = rs.standard_normal((K, D))
    mom = (0.1 * rs.standard_normal((K, D)), 0.01 * rs.random_sample((K, D)), 0.1 * rs.standard_normal((K, P)),
           0.01 * rs.random_sample((K, P)))
    G = rs.standard_normal((K, B, D))
    return loc, scales, mom, G


def _dev(eng, *arrs):
    return [eng.asarray(a).contiguous() for a in arrs]


def _targets(K, D, seed=0):
    import gsmvi_amd
    ms, Ps = ref.gaussian_targets(K, D, seed=seed)
    return gsmvi_amd.BatchedGaussianTarget(ms, precision=Ps), ms, Ps


# ---- 4. one step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DS)
def test_one_step_matches_the_restatement(D):
    """a step from a random state (non-zero moments, t = 7) per problem at 1e-11, the project's single-update tolerance: state,
    moments, Xout and logq_sum; scalar lr and per-problem lr_dev; the stream's z and given z"""
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    K, t = 5, 7
    for B in (1, 32):
        for n, per_problem in enumerate((False, True)):
            loc, scales, mom, G = _state(K, D, B, 1000 * D + 10 * B + n)
            lr = np.array([0.003, 0.01, 0.05, 0.1, 0.3]) if per_problem else 0.02
            keys = [3, 2 ** 40 + 1, 17, 99, 12345]
            call = 4
            Zc = np.stack([ref.draw(k, call - 1, B, D) for k in keys])
            Zn = np.stack([ref.draw(k, call, B, D) for k in keys])
            want = ref.step(G, Zc, loc, scales, mom, t, lr, 0.9, 0.999, 1e-8, Znext=Zn)
            for forced in (True, False):                                     # (the stream's run last: compared below)
                d_loc, d_sc, d_G = _dev(eng, loc, scales, G)
                d_mom = tuple(_dev(eng, *mom))
                X, logq = eng.empty(K, B, D), eng.empty(K)
                lr_d = eng.batched_regs(lr) if per_problem else lr
                eng.last_path(reset=True)
                if forced:
                    eng.advi_step_batched(d_G, d_loc, d_sc, d_mom, t, lr_d, Zcur=eng.asarray(Zc), Znext=eng.asarray(Zn), Xout=X,
                                          logq=logq)
                else:
                    eng.advi_step_batched(d_G, d_loc, d_sc, d_mom, t, lr_d, seeds=eng.batched_seeds(keys), call=call, Xout=X,
                                          logq=logq)
                assert eng.last_path(reset=True) == {"batched_advi"}
                assert np.array_equal(d_G.cpu().numpy(), G)                      # the score is only read
                got = [d_loc, d_sc, *d_mom, X, logq]
                exp = [want[0], want[1], *want[2], want[3], want[4]]
                names = ["loc", "scales", "m_loc", "v_loc", "m_s", "v_s", "Xout", "logq_sum"]
                for k in range(K):
                    errs = {nm: rel_err(g[k].cpu().numpy(), e[k]) for nm, g, e in zip(names, got, exp)}
                    assert max(errs.values()) <= 1e-11, (D, B, per_problem, forced, k, errs)
            # without Xout the state moves the same way and nothing else is written
            d_loc, d_sc, d_G = _dev(eng, loc, scales, G)
            d_mom = tuple(_dev(eng, *mom))
            eng.advi_step_batched(d_G, d_loc, d_sc, d_mom, t, lr_d, seeds=eng.batched_seeds(keys), call=call)
            assert torch.equal(d_loc, got[0]) and torch.equal(d_sc, got[1]) and all(torch.equal(a, b) for a, b in zip(d_mom, got[2:6]))


# ---- 6. init and cov -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DS)
def test_init_and_cov(D):
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    K, B = 6, 5
    rs = np.random.RandomState(D)
    A = rs.standard_normal((K, D, D))
    cov = A @ np.swapaxes(A, 1, 2) / D + 0.2 * np.eye(D)
    cov = 0.5 * (cov + np.swapaxes(cov, 1, 2))
    mean = rs.standard_normal((K, D))
    keys = [5, 6, 7, 2 ** 33, 9, 10]
    d_mean, d_cov = _dev(eng, mean, cov)
    seeds = eng.batched_seeds(keys)
    scales, info = eng.empty(K, ref.tri(D)), eng.batched_ints(K)
    X, logq = eng.empty(K, B, D), eng.empty(K)
    eng.last_path(reset=True)
    eng.advi_init_batched(d_mean, d_cov, scales, info, seeds, None, X, logq)
    assert eng.last_path(reset=True) == {"batched_advi"}
    assert eng.read_ints(info).tolist() == [0] * K
    assert np.array_equal(d_mean.cpu().numpy(), mean) and np.array_equal(d_cov.cpu().numpy(), cov)
    Z = np.stack([ref.draw(k, 0, B, D) for k in keys])
    s_ref, X_ref, q_ref = ref.init(mean, cov, Z)
    for k in range(K):
        assert rel_err(scales[k].cpu().numpy(), np.linalg.cholesky(cov[k])[np.tril_indices(D)]) <= 1e-11, (D, k)
        assert rel_err(X[k].cpu().numpy(), X_ref[k]) <= 1e-11 and rel_err(logq[k].cpu().numpy(), q_ref[k]) <= 1e-11, (D, k)
    # the shared draw layout: the GSM fit's init draws the same samples from the same keys and state
    R, info2, Xg = eng.empty(K, D, D), eng.batched_ints(K), eng.empty(K, B, D)
    eng.gsm_fit_init_batched(d_mean, d_cov, R, info2, seeds, Xg)
    for k in range(K):
        assert rel_err(X[k].cpu().numpy(), Xg[k].cpu().numpy()) <= 1e-11, (D, k)
    # given normals in place of the stream
    X2, logq2, scales2 = eng.empty(K, B, D), eng.empty(K), eng.empty(K, ref.tri(D))
    eng.advi_init_batched(d_mean, d_cov, scales2, info, None, eng.asarray(Z), X2, logq2)
    assert torch.equal(scales2, scales)
    for k in range(K):
        assert rel_err(X2[k].cpu().numpy(), X_ref[k]) <= 1e-11 and rel_err(logq2[k].cpu().numpy(), q_ref[k]) <= 1e-11
    # no samples asked for
    scales3 = eng.empty(K, ref.tri(D))
    eng.advi_init_batched(d_mean, d_cov, scales3, info, None, None, None, None)
    assert torch.equal(scales3, scales)
    # cov = L L^T, exactly symmetric
    c = eng.advi_cov_batched(scales, D).cpu().numpy()
    c_ref = ref.cov_of(scales.cpu().numpy(), D)
    for k in range(K):
        assert np.array_equal(c[k], c[k].T) and rel_err(c[k], c_ref[k]) <= 1e-11 and rel_err(c[k], cov[k]) <= 1e-11, (D, k)
    loc_r, sc_r, _, _ = _state(K, D, B, D)                                      # a general L (negative diagonal entries too)
    c = eng.advi_cov_batched(eng.asarray(sc_r), D).cpu().numpy()
    c_ref = ref.cov_of(sc_r, D)
    for k in range(K):
        assert np.array_equal(c[k], c[k].T) and rel_err(c[k], c_ref[k]) <= 1e-11, (D, k)


def test_non_pd_initial_covariance_raises_naming_the_problem():
    import gsmvi_amd
    K, D = 6, 9
    tgt, _, _ = _targets(K, D)
    cov = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    cov[1, 3, 3] = -1.0
    cov[4] = np.nan
    with pytest.raises(ValueError, match=r"\[1, 4\]"):
        gsmvi_amd.ADVIBatch(K, D, tgt.lp, tgt.lp_g).fit(range(K), gsmvi_amd.Adam(0.1), cov=cov, niter=3, verbose=False)


# ---- 5. 501 chained iterations -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B", [(5, 2), (10, 8), (33, 4), (64, 8)])
def test_fit_matches_the_restatements_loop_over_501_iterations(D, B):
    """free-running (the z stream does not depend on the state): 1e-8 on loc, cov and losses, the bar for 501 chained updates"""
    import gsmvi_amd
    K, niter, lr = 3, 500, 0.02
    keys = [21, 22, 2 ** 35 + 5]
    tgt, ms, Ps = _targets(K, D, seed=D)
    rs = np.random.RandomState(D)
    mean0 = rs.standard_normal((K, D))
    cov0 = np.stack([np.eye(D) * (0.5 + 0.5 * k) for k in range(K)])
    fit = gsmvi_amd.ADVIBatch(K, D, tgt.lp, tgt.lp_g)
    m, c, losses = fit.fit(keys, gsmvi_amd.Adam(lr), mean=mean0, cov=cov0, batch_size=B, niter=niter, verbose=False)
    assert isinstance(m, np.ndarray) and losses.shape == (niter + 1, K)
    mo, co, lo = ref.fit(keys, ref.gaussian_lp(ms, Ps), ref.gaussian_score(ms, Ps), lr, mean0, cov0, B, niter)
    errs = [(rel_err(m[k], mo[k]), rel_err(c[k], co[k]), rel_err(losses[:, k], lo[:, k])) for k in range(K)]
    print(f"D={D} B={B}: (loc, cov, losses) per problem {errs}")
    assert max(max(e) for e in errs) <= 1e-8, errs
    # forced_z fed the stream's own normals gives the same fit
    eng = gsmvi_amd.get_engine()
    Dz = D + (D & 1)
    Zs = torch.stack([torch.stack([eng.normal(B, Dz, k, i)[:, :D] for k in keys]) for i in range(niter + 1)]).contiguous()
    mf, cf, lf = fit.fit(keys, gsmvi_amd.Adam(lr), mean=mean0, cov=cov0, batch_size=B, niter=niter, verbose=False, forced_z=Zs)
    assert np.array_equal(mf, m) and np.array_equal(cf, c)
    assert rel_err(lf, losses) <= 1e-12                                          # (the sum of |z|^2 runs in another order)


# ---- 9. it fits, and the endpoint is the reference estimator's ---------------------------------------------------------------
@pytest.mark.parametrize("D,B,lr", [(5, 2, 1e-2), (10, 8, 1e-1), (33, 32, 1e-2)])
def test_it_fits_and_the_endpoint_is_torch_autograd_with_adam(D, B, lr):
    import gsmvi_amd
    K, niter = 4, 500
    keys = [31, 32, 33, 34]
    tgt, ms, Ps = _targets(K, D, seed=7)
    m, c, losses = gsmvi_amd.ADVIBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, gsmvi_amd.Adam(lr), batch_size=B, niter=niter,
                                                                  verbose=False)
    assert (losses[-1] < losses[0]).all(), (losses[0], losses[-1])
    for k in (0, K - 1):
        loc_t, scales_t, losses_t, _ = ref.torch_advi_run(ms[k], Ps[k], keys[k], lr, B, niter + 1)
        Lt = ref.unpack(scales_t, D)
        errs = (rel_err(m[k], loc_t), rel_err(c[k], Lt @ Lt.T), rel_err(losses[:, k], losses_t))
        print(f"D={D} B={B} k={k}: (loc, cov, losses) against torch {errs}")
        assert max(errs) <= 1e-8, (k, errs)


# ---- 7. isolation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B", [(10, 2), (16, 8), (17, 4), (40, 8)])
def test_a_problem_gives_the_same_bits_alone_and_in_any_batch(D, B):
    import gsmvi_amd
    niter, lr = 20, 0.05
    Kbig = 1024
    ms, Ps = ref.gaussian_targets(16, D, seed=1)
    msb, Psb = np.tile(ms, (Kbig // 16, 1)), np.tile(Ps, (Kbig // 16, 1, 1))
    keys_big = np.arange(Kbig) + 100
    pick = [0, 5, 15]                                                           # problems followed through the batch sizes
    tgt = gsmvi_amd.BatchedGaussianTarget(msb, precision=Psb)
    mb, cb, lb = gsmvi_amd.ADVIBatch(Kbig, D, tgt.lp, tgt.lp_g).fit(keys_big, gsmvi_amd.Adam(lr), batch_size=B, niter=niter,
                                                                    verbose=False)
    tgt16 = gsmvi_amd.BatchedGaussianTarget(ms, precision=Ps)
    m16, c16, l16 = gsmvi_amd.ADVIBatch(16, D, tgt16.lp, tgt16.lp_g).fit(keys_big[:16], gsmvi_amd.Adam(lr), batch_size=B,
                                                                        niter=niter, verbose=False)
    assert np.array_equal(m16, mb[:16]) and np.array_equal(c16, cb[:16])
    assert rel_err(l16, lb[:, :16]) <= 1e-13            # (logq_sum has the same bits; lp is torch's einsum, whose order may depend on K)
    for k in pick:
        t1 = gsmvi_amd.BatchedGaussianTarget(ms[k:k + 1], precision=Ps[k:k + 1])
        m1, c1, l1 = gsmvi_amd.ADVIBatch(1, D, t1.lp, t1.lp_g).fit([keys_big[k]], gsmvi_amd.Adam(lr), batch_size=B, niter=niter,
                                                                   verbose=False)
        assert np.array_equal(m1[0], mb[k]) and np.array_equal(c1[0], cb[k]) and rel_err(l1[:, 0], lb[:, k]) <= 1e-13, k


@pytest.mark.parametrize("D,B", [(10, 2), (33, 4)])
def test_a_nan_score_poisons_its_own_problem_alone(D, B):
    import gsmvi_amd
    K, niter, bad = 9, 12, 5                                                    # (D = 10: problems 4 .. 7 share a workgroup)
    tgt, _, _ = _targets(K, D, seed=2)
    keys = list(range(50, 50 + K))
    n = [0]

    def poisoned(x, out=None):
        G = tgt.lp_g(x, out=out)
        if n[0] >= 3:
            G[bad] = float("nan")
        n[0] += 1
        return G
    poisoned.device_native = True

    m_ref, c_ref, l_ref = gsmvi_amd.ADVIBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, gsmvi_amd.Adam(0.05), batch_size=B, niter=niter,
                                                                         verbose=False)
    m, c, l = gsmvi_amd.ADVIBatch(K, D, tgt.lp, poisoned).fit(keys, gsmvi_amd.Adam(0.05), batch_size=B, niter=niter, verbose=False)
    others = [k for k in range(K) if k != bad]
    assert np.isnan(m[bad]).all() and np.isnan(c[bad]).all() and np.isnan(l[4:, bad]).all()
    assert np.array_equal(l[:4, bad], l_ref[:4, bad])
    assert np.array_equal(m[others], m_ref[others]) and np.array_equal(c[others], c_ref[others])
    assert np.array_equal(l[:, others], l_ref[:, others])


# ---- 8. determinism, inputs, path, monitor -------------------------------------------------------------------------------
def test_determinism_inputs_untouched_and_the_path_bit():
    import gsmvi_amd
    K, D, B, niter = 37, 12, 4, 40
    tgt, _, _ = _targets(K, D, seed=3)
    eng = gsmvi_amd.get_engine()
    rs = np.random.RandomState(0)
    mean0 = rs.standard_normal((K, D))
    cov0 = np.stack([np.eye(D) * (1.0 + 0.01 * k) for k in range(K)])
    keys = np.arange(K) + 7
    lrs = np.linspace(0.01, 0.1, K)
    m_in, c_in, k_in, lr_in = mean0.copy(), cov0.copy(), keys.copy(), lrs.copy()
    fit = gsmvi_amd.ADVIBatch(K, D, tgt.lp, tgt.lp_g)
    eng.last_path(reset=True)
    a = fit.fit(keys, gsmvi_amd.Adam(lrs), mean=mean0, cov=cov0, batch_size=B, niter=niter, verbose=False)
    path = eng.last_path(reset=True)
    assert "batched_advi" in path and path <= {"batched_advi", "batched"}       # ("batched": the target's score kernel)
    assert not any(p.endswith("_generic") for p in path)
    b = fit.fit(keys, gsmvi_amd.Adam(lrs), mean=mean0, cov=cov0, batch_size=B, niter=niter, verbose=False)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(mean0, m_in) and np.array_equal(cov0, c_in) and np.array_equal(keys, k_in) and np.array_equal(lrs, lr_in)
    # device tensors in, as_torch out, the same bits; track_loss=False skips lp
    mt, ct = torch.tensor(mean0, device="cuda"), torch.tensor(cov0, device="cuda")
    c = fit.fit(keys, gsmvi_amd.Adam(lrs), mean=mt, cov=ct, batch_size=B, niter=niter, verbose=False, as_torch=True)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in c)
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(c, a))
    assert np.array_equal(mt.cpu().numpy(), mean0) and np.array_equal(ct.cpu().numpy(), cov0)
    calls = []

    def lp(x):
        calls.append(1)
        return tgt.lp(x)

    d = gsmvi_amd.ADVIBatch(K, D, lp, tgt.lp_g).fit(keys, gsmvi_amd.Adam(lrs), mean=mean0, cov=cov0, batch_size=B, niter=niter,
                                                   verbose=False, track_loss=False)
    assert d[2] is None and calls == [] and np.array_equal(d[0], a[0]) and np.array_equal(d[1], a[1])
    # a host score (numpy in, numpy out) gives the same fit
    ms, Ps = ref.gaussian_targets(K, D, seed=3)
    e = gsmvi_amd.ADVIBatch(K, D, tgt.lp, ref.gaussian_score(ms, Ps)).fit(keys, gsmvi_amd.Adam(lrs), mean=mean0, cov=cov0,
                                                                         batch_size=B, niter=niter, verbose=False)
    assert rel_err(e[0], a[0]) <= 1e-9 and rel_err(e[1], a[1]) <= 1e-9


def test_a_batched_kl_monitor_follows_the_fit_and_leaves_it_alone():
    import gsmvi_amd
    K, D, B, niter, ck = 8, 6, 8, 100, 25
    tgt, ms, Ps = _targets(K, D, seed=4)
    keys = list(range(K))
    fit = gsmvi_amd.ADVIBatch(K, D, tgt.lp, tgt.lp_g)
    m0, c0, l0 = fit.fit(keys, gsmvi_amd.Adam(0.05), batch_size=B, niter=niter, verbose=False)
    mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=64, checkpoint=ck)
    m1, c1, l1 = fit.fit(keys, gsmvi_amd.Adam(0.05), None, None, B, niter, 10, mon, verbose=False)
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1) and np.array_equal(l0, l1)
    assert len(mon.rkl) == niter // ck + 2 and all(r.shape == (K,) and np.isfinite(r).all() for r in mon.rkl)
    assert mon.nevals == [1 + i * B for i in (0, 25, 50, 75, 100)] + [1 + (niter + 1) * B]
    with pytest.raises(TypeError, match="monitor"):
        fit.fit(keys, gsmvi_amd.Adam(0.05), niter=2, verbose=False, monitor=gsmvi_amd.KLMonitor(batch_size_kl=4, checkpoint=1))
