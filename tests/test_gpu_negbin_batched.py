"""The batched negative binomial target on the GPU (gsmvi_negbin_batched_f64, csrc/gsmvi_negbin_batched.hip) through the C ABI:
the kernel against the longdouble restatement (tests/negbin_batched_ref.py) at the edges of its tiling, the row flags, isolation
and determinism bit for bit, counts = 0, the Poisson limit against the Poisson launch, the target inside the fits against the
same fits scored by the float64 restatement on the host, a planted log size recovered, and a captured launch."""
import numpy as np
import pytest
import torch

import negbin_batched_ref as ref
import negbin_link_truth as truth
from conftest import rel_err

pytestmark = pytest.mark.gpu

DS = [2, 16, 17, 33, 64]                    # the smallest D, the packing switch at 16 / 17, odd D, the maximum
# (N, nc, K, with an offset): every N of {1, 31, 32, 33, 70} (the 32-row tile of A and its prefetch), every nc of {1, 15, 16, 17, 32,
# 33, 40} (TC = 16 and 32), every K of {1, 5, 9} (tail slots of the four-problem packing), with and without an offset
CASES = [(1, 1, 1, True), (31, 15, 5, False), (32, 16, 9, True), (33, 17, 5, True), (70, 32, 1, False), (33, 33, 9, False),
         (70, 40, 5, True), (32, 1, 9, False), (1, 40, 5, False)]


def _eng():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _dev(eng, A, y, o, counts, lam, tm, tk, X):
    reg = lambda v: v if np.ndim(v) == 0 else eng.batched_regs(v)                # noqa: E731
    return dict(A=eng.asarray(A), y=eng.asarray(y), offset=None if o is None else eng.asarray(o),
                counts=None if counts is None else eng.batched_counts(counts), prior_prec=reg(lam), log_size_mean=reg(tm),
                log_size_prec=reg(tk)), eng.asarray(X)


def _call(eng, A, y, o, counts, lam, tm, tk, X, want="both"):
    """host arrays in, host arrays out: (G, lp), None for what was not asked"""
    d, dX = _dev(eng, A, y, o, counts, lam, tm, tk, X)
    out = eng.negbin_batched(dX, want=want, **d)
    torch.cuda.synchronize()
    if want == "both":
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return (out.cpu().numpy(), None) if want == "g" else (None, out.cpu().numpy())


def _check(eng, A, y, o, counts, lam, tm, tk, X, tag):
    """the three calls against the longdouble restatement at 1e-11 per problem and against each other bit for bit; inputs only
    read; the path bit.  Returns the worst error."""
    K = A.shape[0]
    d, dX = _dev(eng, A, y, o, counts, lam, tm, tk, X)
    eng.last_path(reset=True)
    G, lp = eng.negbin_batched(dX, want="both", **d)
    assert eng.last_path(reset=True) == {"batched_target"}
    G1 = eng.negbin_batched(dX, want="g", **d)
    lp1 = eng.negbin_batched(dX, want="lp", **d)
    assert eng.last_path(reset=True) == {"batched_target"}
    assert torch.equal(G1, G) and torch.equal(lp1, lp), tag
    assert np.array_equal(d["A"].cpu().numpy(), A, equal_nan=True) and np.array_equal(d["y"].cpu().numpy(), y, equal_nan=True)
    assert np.array_equal(dX.cpu().numpy(), X)
    Gr, lpr = ref.score_and_lp_ld(A, y, o, counts, lam, tm, tk, X)
    Gr, lpr = Gr.astype(np.float64), lpr.astype(np.float64)
    G, lp = G.cpu().numpy(), lp.cpu().numpy()
    worst = 0.0
    for k in range(K):
        eg, el = rel_err(G[k], Gr[k]), rel_err(lp[k], lpr[k])
        worst = max(worst, eg, el)
        assert eg <= 1e-11 and el <= 1e-11, (tag, k, eg, el)
    return worst


# ---- 1. the kernel against the longdouble restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("D", DS)
def test_kernel_matches_the_longdouble_restatement(D):
    """G and lp at 1e-11 per problem (rel_err, the measure of tests/test_gpu_glm_batched.py), all three wants; per-problem
    precisions and counts (0 and N among them, the dead rows poisoned) with an offset, scalars and counts = NULL without"""
    eng = _eng()
    worst, sides = 0.0, 0
    for N, nc, K, off in CASES:
        A, y, o, counts, lam, tm, tk, X = ref.make_inputs(K, N, D - 1, nc)
        r = np.exp(X[:, :, -1])
        sides |= (1 if (r < ref.SHIFT_BELOW).any() else 0) | (2 if (r >= ref.SHIFT_BELOW).any() else 0)
        if nc >= 15:                                                            # both sides of the shift threshold in one call
            assert (r < ref.SHIFT_BELOW).any() and (r >= ref.SHIFT_BELOW).any()
        if off:
            assert counts[0] == N and (K == 1 or counts[1] == 0)
            worst = max(worst, _check(eng, A, y, o, counts, lam, tm, tk, X, (D, N, nc, K, "offset, counts")))
        else:
            A, y = np.nan_to_num(A), np.abs(np.nan_to_num(y))                   # every row counts: no poison
            worst = max(worst, _check(eng, A, y, None, None, 0.7, 0.4, 1.3, X, (D, N, nc, K, "scalars")))
    assert sides == 3
    print(f"negbin D={D}: worst rel_err against the longdouble restatement {worst:.2e}")


# ---- 2. the row flags --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [10, 33])
def test_a_flagged_row_is_nan_alone(D):
    """a non-finite entry in a row of X (beta or theta), or theta = +-800 (e^theta is not a positive normal number): that row is
    NaN, every other row and problem (its workgroup neighbours included) keeps its bits"""
    eng = _eng()
    K, N, nc, P = 9, 70, 40, D - 1
    A, y, o, counts, lam, tm, tk, X = ref.make_inputs(K, N, P, nc, seed=3 * D)
    G, lp = _call(eng, A, y, o, counts, lam, tm, tk, X)
    assert np.isfinite(G).all() and np.isfinite(lp).all()
    for col, badv in ((P // 2, np.nan), (0, np.inf), (P, -np.inf), (P, np.nan), (P, 800.0), (P, -800.0)):
        for (k, c) in ((5, 17), (0, 0), (8, 39)):
            X2 = X.copy()
            X2[k, c, col] = badv
            G3, lp3 = _call(eng, A, y, o, counts, lam, tm, tk, X2)
            assert np.isnan(G3[k, c]).all() and np.isnan(lp3[k, c]), (col, badv, k, c)
            keep = np.ones((K, nc), dtype=bool)
            keep[k, c] = False
            assert np.array_equal(G3[keep], G[keep]) and np.array_equal(lp3[keep], lp[keep]), (col, badv, k, c)
            for want in ("g", "lp"):
                g1, l1 = _call(eng, A, y, o, counts, lam, tm, tk, X2, want=want)
                assert np.array_equal(g1 if want == "g" else l1, G3 if want == "g" else lp3, equal_nan=True), want
    # theta = +-700 is inside: e^theta is a normal number and the outputs are finite
    X2 = X.copy()
    X2[5, 17, P], X2[0, 0, P] = 700.0, -700.0
    G3, lp3 = _call(eng, A, y, o, counts, lam, tm, tk, X2)
    assert np.isfinite(G3).all() and np.isfinite(lp3).all()


# ---- 3. isolation and determinism, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [10, 33])
def test_a_problem_gives_the_same_bits_alone_and_in_any_batch(D):
    eng = _eng()
    N, nc = 70, 5
    A, y, o, counts, lam, tm, tk, X = ref.make_inputs(64, N, D - 1, nc, seed=7 + D)
    Gb, lpb = _call(eng, A, y, o, counts, lam, tm, tk, X)
    Gb2, lpb2 = _call(eng, A, y, o, counts, lam, tm, tk, X)
    assert np.array_equal(Gb, Gb2) and np.array_equal(lpb, lpb2)                 # two runs
    G16, lp16 = _call(eng, A[:16], y[:16], o[:16], counts[:16], lam[:16], tm[:16], tk[:16], X[:16])
    assert np.array_equal(G16, Gb[:16]) and np.array_equal(lp16, lpb[:16])
    for k in (0, 1, 6, 15, 63):
        s = slice(k, k + 1)
        G1, lp1 = _call(eng, A[s], y[s], o[s], counts[s], lam[s], tm[s], tk[s], X[s])
        assert np.array_equal(G1[0], Gb[k]) and np.array_equal(lp1[0], lpb[k]), k
    # the scalar priors and counts = NULL take the same arithmetic
    G1, lp1 = _call(eng, A[0:1], y[0:1], o[0:1], None, float(lam[0]), float(tm[0]), float(tk[0]), X[0:1])
    assert counts[0] == N and np.array_equal(G1[0], Gb[0]) and np.array_equal(lp1[0], lpb[0])


@pytest.mark.parametrize("D", [10, 33])
def test_a_row_gives_the_same_bits_alone_and_among_64(D):
    eng = _eng()
    A, y, o, counts, lam, tm, tk, X = ref.make_inputs(7, 90, D - 1, 64, seed=D)
    G, lp = _call(eng, A, y, o, counts, lam, tm, tk, X)
    for c in (0, 15, 16, 31, 32, 63):
        G1, lp1 = _call(eng, A, y, o, counts, lam, tm, tk, np.ascontiguousarray(X[:, c:c + 1]))
        assert np.array_equal(G1[:, 0], G[:, c]) and np.array_equal(lp1[:, 0], lp[:, c]), c
    G40, lp40 = _call(eng, A, y, o, counts, lam, tm, tk, np.ascontiguousarray(X[:, 20:60]))
    assert np.array_equal(G40, G[:, 20:60]) and np.array_equal(lp40, lp[:, 20:60])


@pytest.mark.parametrize("D", [10, 33])
def test_counts_zero_is_the_two_priors_and_dead_rows_play_no_part(D):
    eng = _eng()
    K, N, nc, P = 9, 70, 17, D - 1
    A, y, o, counts, lam, tm, tk, X = ref.make_inputs(K, N, P, nc, seed=5 * D)
    assert counts[1] == 0 and np.isnan(A[1]).all() and np.isinf(o[1]).all()
    G, lp = _call(eng, A, y, o, counts, lam, tm, tk, X)
    beta, th = X[1, :, :P], X[1, :, P]
    dm = th - tm[1]
    assert np.array_equal(G[1, :, :P], 0.0 - lam[1] * beta) and np.array_equal(G[1, :, P], 0.0 - tk[1] * dm)
    assert np.array_equal(lp[1], 0.0 - 0.5 * lam[1] * np.array([np.cumsum(b * b)[-1] for b in beta]) - 0.5 * tk[1] * (dm * dm))
    # the same data without the poison in the dead rows: the same bits
    A2, y2, o2 = ref.make_inputs(K, N, P, nc, seed=5 * D, poison=False)[:3]
    G2, lp2 = _call(eng, A2, y2, o2, counts, lam, tm, tk, X)
    assert np.isfinite(A2).all() and np.array_equal(G2, G) and np.array_equal(lp2, lp)


# ---- 4. the Poisson limit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [10, 33])
def test_poisson_limit_on_the_device(D):
    """theta = 30 (r = 1.07e13): G[:, :, :P] and lp against glm_batched(..., "poisson") at beta on the same data, within the sums
    over the valid rows of the per-observation bounds |t - (y eta - mu)| <= (y + mu)^2 / (2 r) and |r_eta - (y - mu)| <= |y - mu|
    mu / r (tests/test_negbin_batched_cpu.py) plus the rounding both launches are allowed: c_gpu eps scale per term (the link
    bound of tests/test_gpu_negbin_link_truth.py and of the GLM links, 16 each) and N eps per term for the chain of N additions,
    (2 * 16 + 2 N) eps sum_n scale_n in all, with scale_n evaluated in float64 on the host; lam is shared and kap = 0"""
    eng = _eng()
    K, N, nc, P, theta = 5, 70, 6, D - 1, 30.0
    A, y, o, counts, lam, tm, tk, X = ref.make_inputs(K, N, P, nc, seed=9 * D)
    X[:, :, P] = theta
    X[:, :, :P] *= 0.5
    G, lp = _call(eng, A, y, o, counts, lam, tm, 0.0, X)
    beta = np.ascontiguousarray(X[:, :, :P])
    Gp, lpp = eng.glm_batched(eng.asarray(beta), eng.asarray(A), eng.asarray(y), "poisson", offset=eng.asarray(o),
                              counts=eng.batched_counts(counts), prior_prec=eng.batched_regs(lam), want="both")
    Gp, lpp = Gp.cpu().numpy(), lpp.cpu().numpy()
    r, c = np.exp(theta), 2.0 * max(truth.c_gpu("t"), truth.c_gpu("re")) + 2.0 * N
    for k in range(K):
        n = int(counts[k])
        Ak, yk = A[k, :n], y[k, None, :n]
        eta = beta[k] @ Ak.T + o[k, None, :n]                                   # (nc, n)
        mu = np.exp(eta)
        d = eta - theta
        sg, sn = 1.0 / (1.0 + np.exp(-d)), 1.0 / (1.0 + np.exp(d))
        spd, spn = np.logaddexp(0.0, d), np.logaddexp(0.0, -d)
        tp, rp = yk * eta - mu, yk - mu
        s = (yk + r) * sg * sn
        scale_t = 2.0 * (np.abs(tp) + yk * np.abs(eta) + mu) + np.abs(eta * rp) + yk * theta + r * spd + yk * spn
        scale_r = np.abs(rp) + np.abs(eta) * s + theta * np.abs(s - r * sg) + yk * sn + r * sg + yk + mu
        bt = ((yk + mu) ** 2 / (2.0 * r) + c * truth.EPS * scale_t).sum(1)
        bg = ((np.abs(yk - mu) * mu / r + c * truth.EPS * scale_r)[:, :, None] * np.abs(Ak)[None, :, :]).sum(1)
        assert (np.abs(lp[k] - lpp[k]) <= bt).all(), (k, np.abs(lp[k] - lpp[k]).max(), bt.min())
        assert (np.abs(G[k, :, :P] - Gp[k]) <= bg).all(), (k, (np.abs(G[k, :, :P] - Gp[k]) / bg).max())
    assert np.isfinite(G).all() and np.isfinite(lp).all()


# ---- 5. in the fits ----------------------------------------------------------------------------------------------------------
def _per_problem(a, b):
    return max(rel_err(a[k], b[k]) for k in range(a.shape[0]))


@pytest.mark.parametrize("D,B", [(5, 2), (17, 4)])
def test_forced_fits_match_the_same_fits_scored_by_the_restatement(D, B):
    """GSMBatch (forced samples) and ADVIBatch (forced normals, losses tracked) over 30 iterations, scored by the target and by
    the float64 restatement as a plain numpy callable: the same recursion, so the same reverts and mean, cov (and ADVI's losses)
    at 1e-8 per problem, the chained tolerance of the softmax and GLM tests of the same name"""
    import gsmvi_amd
    K, N, niter, P = 6, 40, 30, D - 1
    A, y, o, counts, lam, tm, tk, _ = ref.make_inputs(K, N, P, 1)
    lam, tk = lam + 0.5, tk + 0.5
    tgt = gsmvi_amd.BatchedNegBinomialTarget(A, y, lam, counts, o, tm, tk)
    lp_h = lambda X: ref.score_and_lp(A, y, o, counts, lam, tm, tk, X)[1]       # noqa: E731
    lpg_h = lambda X: ref.score_and_lp(A, y, o, counts, lam, tm, tk, X)[0]      # noqa: E731
    keys = np.arange(K) + 40
    forced = np.random.RandomState(1000 + D).standard_normal((niter + 1, K, B, D))
    res = []
    for lp, lpg in ((tgt.lp, tgt.lp_g), (lp_h, lpg_h)):
        f = gsmvi_amd.GSMBatch(K, D, lp, lpg)
        m, c = f.fit(keys, batch_size=B, niter=niter, verbose=False, forced_samples=forced)
        res.append((m, c, f.n_reverts.copy()))
    (m0, c0, r0), (m1, c1, r1) = res
    em, ec = _per_problem(m0, m1), _per_problem(c0, c1)
    print(f"negbin GSM D={D} B={B}: forced fit, target against numpy-scored: mean {em:.2e} cov {ec:.2e} reverts {int(r0.sum())}")
    assert np.array_equal(r0, r1), (r0, r1)
    assert np.isfinite(m0).all() and np.isfinite(c0).all()
    assert em <= 1e-8 and ec <= 1e-8, (em, ec)
    res = []
    for lp, lpg in ((tgt.lp, tgt.lp_g), (lp_h, lpg_h)):
        res.append(gsmvi_amd.ADVIBatch(K, D, lp, lpg).fit(keys, gsmvi_amd.Adam(1e-2), batch_size=B, niter=niter, verbose=False,
                                                         track_loss=True, forced_z=forced))
    (m0, c0, l0), (m1, c1, l1) = res
    em, ec, el = _per_problem(m0, m1), _per_problem(c0, c1), _per_problem(l0.T, l1.T)
    print(f"negbin ADVI D={D} B={B}: forced fit, target against numpy-scored: mean {em:.2e} cov {ec:.2e} losses {el:.2e}")
    assert np.isfinite(m0).all() and np.isfinite(c0).all() and np.isfinite(l0).all()
    assert em <= 1e-8 and ec <= 1e-8 and el <= 1e-8, (em, ec, el)


PLANTED = dict(K=16, N=200, P=3, seed=77, niter=300, B=8)


def planted_problem():
    """K count data sets with a planted log size in [0.5, 2.5]: an intercept of about 1.5, slopes of 0.4 N(0, 1), y negative binomial"""
    p = PLANTED
    rs = np.random.RandomState(p["seed"])
    K, N, P = p["K"], p["N"], p["P"]
    A = np.concatenate([np.ones((K, N, 1)), rs.standard_normal((K, N, P - 1))], axis=2)
    beta = np.concatenate([1.5 + 0.5 * rs.standard_normal((K, 1)), 0.4 * rs.standard_normal((K, P - 1))], axis=1)
    theta = rs.uniform(0.5, 2.5, K)
    mu = np.exp(np.einsum("knp,kp->kn", A, beta))
    y = rs.poisson(rs.gamma(np.exp(theta)[:, None], mu / np.exp(theta)[:, None])).astype(np.float64)
    return A, y, theta


def test_lbfgs_start_then_gsm_fit_recovers_a_planted_log_size():
    """K = 16, N = 200, P = 3: from the L-BFGS start, GSMBatch.fit's mean of theta is within 4 posterior standard deviations (its
    own cov) of the planted log r for every problem (the seed passes on the CPU restatement with the same draws)"""
    import gsmvi_amd
    p = PLANTED
    A, y, theta = planted_problem()
    tgt = gsmvi_amd.BatchedNegBinomialTarget(A, y, prior_precision=0.01, log_size_mean=0.0, log_size_precision=0.01)
    m0, c0, res = gsmvi_amd.lbfgs_init_batched(np.zeros((p["K"], p["P"] + 1)), tgt.lp, tgt.lp_g)
    assert res.success.all()
    fit = gsmvi_amd.GSMBatch(p["K"], p["P"] + 1, tgt.lp, tgt.lp_g)
    mean, cov = fit.fit(np.arange(p["K"]) + 7, mean=m0, cov=c0, batch_size=p["B"], niter=p["niter"], verbose=False)
    sd = np.sqrt(cov[:, -1, -1])
    z = (mean[:, -1] - theta) / sd
    print(f"planted log r: worst |z| {np.abs(z).max():.2f}, sd {sd.min():.3f} .. {sd.max():.3f}, reverts {int(fit.n_reverts.sum())}")
    assert np.isfinite(mean).all() and (sd > 0.0).all() and (sd < 1.0).all()
    assert (np.abs(z) <= 4.0).all(), z


# ---- 6. a captured launch ----------------------------------------------------------------------------------------------------
def test_lp_g_captured_into_a_graph_replays_the_eager_bits():
    import gsmvi_amd
    K, P, B = 37, 9, 2
    A, y, o, counts, lam, tm, tk, X = ref.make_inputs(K, 120, P, B)
    tgt = gsmvi_amd.BatchedNegBinomialTarget(A, y, lam, counts, o, tm, tk)
    eng = tgt.engine
    x = eng.asarray(X)
    eager = tgt.lp_g(x).clone()
    out = eng.empty(K, B, P + 1)
    eng.last_path(reset=True)
    tgt.lp_g(x, out=out)                                                        # warm: the context exists before the capture
    assert "batched_target" in eng.last_path()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tgt.lp_g(x, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(eng.asarray(X[::-1].copy()))                                         # new inputs in the captured buffer
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, tgt.lp_g(x))
