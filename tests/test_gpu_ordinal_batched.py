"""The batched ordinal target on the GPU (gsmvi_ordinal_batched_f64, csrc/gsmvi_ordinal_batched.hip) through the C ABI: the kernel
against the longdouble restatement (tests/ordinal_batched_ref.py) at the edges of its tiling and of (C, P), the row flags, isolation
and determinism bit for bit, counts = 0, dead rows, C = 2 against the logistic launch, the target inside the fits against the same
fits scored by the float64 restatement on the host, planted cutpoints recovered, and a captured launch."""
import numpy as np
import pytest
import torch

import ordinal_batched_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

# (C, P): the smallest D, C = 3, both extremes of D = 64, both packings at D = 16 / 17 ((5, 12) and (9, 8) are D = 16, (5, 11) is
# D = 15, (4, 61) is D = 64 with a wide A tile)
SHAPES = [(2, 1), (3, 1), (2, 63), (64, 1), (5, 12), (5, 11), (9, 8), (4, 61), (5, 13)]
# (N, nc, K, with an offset): every N of {1, 31, 32, 33, 65} (the 32-row tile of A and its prefetch), every nc of {1, 15, 16, 17, 32,
# 33} (TC = 16 and 32), every K of {1, 3, 4, 5} (tail slots of the four-problem packing), with and without an offset
CASES = [(1, 1, 1, True), (31, 15, 5, False), (32, 16, 4, True), (33, 17, 5, True), (65, 32, 1, False), (33, 33, 3, False),
         (65, 33, 5, True), (32, 1, 4, False)]


def _eng():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _dev(eng, A, y, o, counts, lam, kap, X):
    reg = lambda v: v if np.ndim(v) == 0 else eng.batched_regs(v)                # noqa: E731
    return dict(A=eng.asarray(A), y=eng.batched_labels(y), offset=None if o is None else eng.asarray(o),
                counts=None if counts is None else eng.batched_counts(counts), prior_prec=reg(lam), cut_prec=reg(kap)), eng.asarray(X)


def _call(eng, A, y, o, counts, lam, kap, X, C, want="both"):
    """host arrays in, host arrays out: (G, lp), None for what was not asked"""
    d, dX = _dev(eng, A, y, o, counts, lam, kap, X)
    out = eng.ordinal_batched(dX, C=C, want=want, **d)
    torch.cuda.synchronize()
    if want == "both":
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return (out.cpu().numpy(), None) if want == "g" else (None, out.cpu().numpy())


def _check(eng, A, y, o, counts, lam, kap, X, C, tag):
    """the three calls against the longdouble restatement at 1e-11 per problem and against each other bit for bit; inputs only
    read; the path bit.  Returns the worst error."""
    K = A.shape[0]
    d, dX = _dev(eng, A, y, o, counts, lam, kap, X)
    eng.last_path(reset=True)
    G, lp = eng.ordinal_batched(dX, C=C, want="both", **d)
    assert eng.last_path(reset=True) == {"batched_target"}
    G1 = eng.ordinal_batched(dX, C=C, want="g", **d)
    lp1 = eng.ordinal_batched(dX, C=C, want="lp", **d)
    assert eng.last_path(reset=True) == {"batched_target"}
    assert torch.equal(G1, G) and torch.equal(lp1, lp), tag
    assert np.array_equal(d["A"].cpu().numpy(), A, equal_nan=True) and np.array_equal(d["y"].cpu().numpy(), y)
    assert np.array_equal(dX.cpu().numpy(), X)
    Gr, lpr = ref.score_and_lp_ld(A, y, o, counts, lam, kap, X, C)
    Gr, lpr = Gr.astype(np.float64), lpr.astype(np.float64)
    G, lp = G.cpu().numpy(), lp.cpu().numpy()
    worst = 0.0
    for k in range(K):
        eg, el = rel_err(G[k], Gr[k]), rel_err(lp[k], lpr[k])
        worst = max(worst, eg, el)
        assert eg <= 1e-11 and el <= 1e-11, (tag, k, eg, el)
    return worst


# ---- 1. the kernel against the longdouble restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("C,P", SHAPES)
def test_kernel_matches_the_longdouble_restatement(C, P):
    """G and lp at 1e-11 per problem (rel_err, the measure of tests/test_gpu_glm_batched.py), all three wants; per-problem
    precisions and counts (0 and N among them, the dead rows poisoned, a class absent from the last problem) with an offset,
    scalars and counts = NULL without"""
    eng = _eng()
    worst = 0.0
    for N, nc, K, off in CASES:
        A, y, o, counts, lam, kap, X = ref.make_inputs(K, N, P, C, nc)
        if off:
            assert counts[0] == N and (K == 1 or counts[1] == 0)
            if K > 2 and C > 2:
                assert not (y[K - 1, :counts[K - 1]] == C - 1).any()
            worst = max(worst, _check(eng, A, y, o, counts, lam, kap, X, C, (C, P, N, nc, K, "offset, counts")))
        else:
            A, y = np.nan_to_num(A), np.clip(y, 0, C - 1)                       # every row counts: no poison
            worst = max(worst, _check(eng, A, y, None, None, 0.7, 1.3, X, C, (C, P, N, nc, K, "scalars")))
    print(f"ordinal C={C} P={P}: worst rel_err against the longdouble restatement {worst:.2e}")


# ---- 2. the row flags --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,P", [(4, 7), (6, 28)])
def test_a_flagged_row_is_nan_alone(C, P):
    """a non-finite entry in a row of X (beta or delta), or delta_j = +-750 for some j >= 1 (e^delta_j is not a positive normal
    number): that row is NaN, every other row and problem (its workgroup neighbours included) keeps its bits; delta_0 = +-750 is a
    location: not flagged, and finite"""
    eng = _eng()
    K, N, nc, D = 9, 65, 33, P + C - 1
    A, y, o, counts, lam, kap, X = ref.make_inputs(K, N, P, C, nc, seed=3 * D)
    G, lp = _call(eng, A, y, o, counts, lam, kap, X, C)
    assert np.isfinite(G).all() and np.isfinite(lp).all()
    for col, badv in ((P // 2, np.nan), (0, np.inf), (P, -np.inf), (P, np.nan), (D - 1, np.nan), (P + 1, 750.0), (D - 1, -750.0)):
        for (k, c) in ((5, 17), (0, 0), (8, 32)):
            X2 = X.copy()
            X2[k, c, col] = badv
            G3, lp3 = _call(eng, A, y, o, counts, lam, kap, X2, C)
            assert np.isnan(G3[k, c]).all() and np.isnan(lp3[k, c]), (col, badv, k, c)
            keep = np.ones((K, nc), dtype=bool)
            keep[k, c] = False
            assert np.array_equal(G3[keep], G[keep]) and np.array_equal(lp3[keep], lp[keep]), (col, badv, k, c)
            for want in ("g", "lp"):
                g1, l1 = _call(eng, A, y, o, counts, lam, kap, X2, C, want=want)
                assert np.array_equal(g1 if want == "g" else l1, G3 if want == "g" else lp3, equal_nan=True), want
    # delta_0 = +-750 and delta_j = +-700 are inside: the outputs are finite, and those of the restatement
    X2 = X.copy()
    X2[5, 17, P], X2[0, 0, P], X2[2, 3, P + 1], X2[2, 4, D - 1] = 750.0, -750.0, 700.0, -700.0
    G3, lp3 = _call(eng, A, y, o, counts, lam, kap, X2, C)
    assert np.isfinite(G3).all() and np.isfinite(lp3).all()
    Gr, lpr = ref.score_and_lp_ld(A, y, o, counts, lam, kap, X2, C)
    for k in (0, 2, 5):
        assert rel_err(G3[k], Gr[k].astype(np.float64)) <= 1e-11 and rel_err(lp3[k], lpr[k].astype(np.float64)) <= 1e-11, k


# ---- 3. isolation and determinism, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("C,P", [(4, 7), (6, 28)])
def test_a_problem_gives_the_same_bits_alone_and_in_any_batch(C, P):
    eng = _eng()
    N, nc = 65, 5
    A, y, o, counts, lam, kap, X = ref.make_inputs(64, N, P, C, nc, seed=7 + P)
    Gb, lpb = _call(eng, A, y, o, counts, lam, kap, X, C)
    Gb2, lpb2 = _call(eng, A, y, o, counts, lam, kap, X, C)
    assert np.array_equal(Gb, Gb2) and np.array_equal(lpb, lpb2)                 # two runs
    G16, lp16 = _call(eng, A[:16], y[:16], o[:16], counts[:16], lam[:16], kap[:16], X[:16], C)
    assert np.array_equal(G16, Gb[:16]) and np.array_equal(lp16, lpb[:16])
    for k in (0, 1, 6, 15, 63):
        s = slice(k, k + 1)
        G1, lp1 = _call(eng, A[s], y[s], o[s], counts[s], lam[s], kap[s], X[s], C)
        assert np.array_equal(G1[0], Gb[k]) and np.array_equal(lp1[0], lpb[k]), k
    # the scalar priors and counts = NULL take the same arithmetic
    G1, lp1 = _call(eng, A[0:1], y[0:1], o[0:1], None, float(lam[0]), float(kap[0]), X[0:1], C)
    assert counts[0] == N and np.array_equal(G1[0], Gb[0]) and np.array_equal(lp1[0], lpb[0])


@pytest.mark.parametrize("C,P", [(4, 7), (6, 28)])
def test_a_row_gives_the_same_bits_alone_and_among_64(C, P):
    eng = _eng()
    A, y, o, counts, lam, kap, X = ref.make_inputs(7, 90, P, C, 64, seed=P)
    G, lp = _call(eng, A, y, o, counts, lam, kap, X, C)
    for c in (0, 15, 16, 31, 32, 63):
        G1, lp1 = _call(eng, A, y, o, counts, lam, kap, np.ascontiguousarray(X[:, c:c + 1]), C)
        assert np.array_equal(G1[:, 0], G[:, c]) and np.array_equal(lp1[:, 0], lp[:, c]), c
    G40, lp40 = _call(eng, A, y, o, counts, lam, kap, np.ascontiguousarray(X[:, 20:60]), C)
    assert np.array_equal(G40, G[:, 20:60]) and np.array_equal(lp40, lp[:, 20:60])


@pytest.mark.parametrize("C,P", [(4, 7), (6, 28)])
def test_counts_zero_is_the_two_priors_and_dead_rows_play_no_part(C, P):
    eng = _eng()
    K, N, nc = 9, 65, 17
    A, y, o, counts, lam, kap, X = ref.make_inputs(K, N, P, C, nc, seed=5 * P)
    assert counts[1] == 0 and np.isnan(A[1]).all() and np.isinf(o[1]).all() and (y[1] < 0).all()
    G, lp = _call(eng, A, y, o, counts, lam, kap, X, C)
    beta, delta = X[1, :, :P], X[1, :, P:]
    chain = lambda v: np.array([np.cumsum(r * r)[-1] for r in v])                # noqa: E731
    assert np.array_equal(G[1, :, :P], 0.0 - lam[1] * beta) and np.array_equal(G[1, :, P:], 0.0 - kap[1] * delta)
    assert np.array_equal(lp[1], (0.0 - 0.5 * lam[1] * chain(beta)) - 0.5 * kap[1] * chain(delta))
    # the same data without the poison in the dead rows (NaN, labels out of range, inf): the same bits
    A2, y2, o2 = ref.make_inputs(K, N, P, C, nc, seed=5 * P, poison=False)[:3]
    G2, lp2 = _call(eng, A2, y2, o2, counts, lam, kap, X, C)
    assert np.isfinite(A2).all() and (y2 >= 0).all() and (y2 < C).all() and np.array_equal(G2, G) and np.array_equal(lp2, lp)


# ---- 4. two classes: logistic regression on [A, -1] -------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [3, 15, 40])
def test_two_classes_match_the_logistic_target_on_the_design_with_a_minus_one_column(P):
    import gsmvi_amd
    eng = _eng()
    K, N, nc = 5, 65, 6
    A, y, _, _, _, _, X = ref.make_inputs(K, N, P, 2, nc, poison=False)
    lam = 0.6
    G, lp = _call(eng, A, y, None, None, lam, lam, X, 2)
    tl = gsmvi_amd.BatchedLogisticTarget(np.concatenate([A, -np.ones((K, N, 1))], axis=2), y.astype(np.float64), prior_precision=lam)
    Gl, lpl = tl.lp_and_score(eng.asarray(X))
    Gl, lpl = Gl.cpu().numpy(), lpl.cpu().numpy()
    for k in range(K):
        assert rel_err(G[k], Gl[k]) <= 1e-11 and rel_err(lp[k], lpl[k]) <= 1e-11, k


# ---- 5. in the fits ----------------------------------------------------------------------------------------------------------
def _per_problem(a, b):
    return max(rel_err(a[k], b[k]) for k in range(a.shape[0]))


@pytest.mark.parametrize("C,P,B", [(3, 3, 2), (5, 13, 4)])
def test_forced_fits_match_the_same_fits_scored_by_the_restatement(C, P, B):
    """GSMBatch and BaMBatch (forced samples) and ADVIBatch (forced normals, losses tracked) over 30 iterations, scored by the
    target and by the float64 restatement as a plain numpy callable: the same recursion, so the same reverts and mean, cov (and
    ADVI's losses) at 1e-8 per problem, the chained tolerance of the softmax and negative binomial tests of the same name"""
    import gsmvi_amd
    K, N, niter, D = 6, 40, 30, P + C - 1
    A, y, o, counts, lam, kap, _ = ref.make_inputs(K, N, P, C, 1)
    lam, kap = lam + 0.5, kap + 0.5
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, C, lam, kap, counts, o)
    lp_h = lambda X: ref.score_and_lp(A, y, o, counts, lam, kap, X, C)[1]       # noqa: E731
    lpg_h = lambda X: ref.score_and_lp(A, y, o, counts, lam, kap, X, C)[0]      # noqa: E731
    keys = np.arange(K) + 40
    forced = np.random.RandomState(1000 + D).standard_normal((niter + 1, K, B, D))
    regf = lambda i: 100 / (1 + i)                                              # noqa: E731
    for name, cls in (("GSM", gsmvi_amd.GSMBatch), ("BaM", gsmvi_amd.BaMBatch)):
        res = []
        for lp, lpg in ((tgt.lp, tgt.lp_g), (lp_h, lpg_h)):
            f = cls(K, D, lp, lpg)
            args = (keys,) if name == "GSM" else (keys, regf)
            m, c = f.fit(*args, batch_size=B, niter=niter, verbose=False, forced_samples=forced)
            res.append((m, c, f.n_reverts.copy()))
        (m0, c0, r0), (m1, c1, r1) = res
        em, ec = _per_problem(m0, m1), _per_problem(c0, c1)
        print(f"ordinal {name} C={C} P={P} B={B}: forced fit, target against numpy-scored: mean {em:.2e} cov {ec:.2e} "
              f"reverts {int(r0.sum())}")
        assert np.array_equal(r0, r1), (r0, r1)
        assert np.isfinite(m0).all() and np.isfinite(c0).all()
        assert em <= 1e-8 and ec <= 1e-8, (name, em, ec)
    res = []
    for lp, lpg in ((tgt.lp, tgt.lp_g), (lp_h, lpg_h)):
        res.append(gsmvi_amd.ADVIBatch(K, D, lp, lpg).fit(keys, gsmvi_amd.Adam(1e-2), batch_size=B, niter=niter, verbose=False,
                                                         track_loss=True, forced_z=forced))
    (m0, c0, l0), (m1, c1, l1) = res
    em, ec, el = _per_problem(m0, m1), _per_problem(c0, c1), _per_problem(l0.T, l1.T)
    print(f"ordinal ADVI C={C} P={P} B={B}: forced fit, target against numpy-scored: mean {em:.2e} cov {ec:.2e} losses {el:.2e}")
    assert np.isfinite(m0).all() and np.isfinite(c0).all() and np.isfinite(l0).all()
    assert em <= 1e-8 and ec <= 1e-8 and el <= 1e-8, (em, ec, el)


PLANTED = dict(K=8, N=300, P=2, C=4, seed=77, niter=200, B=8)
# the worst |fitted - planted| cutpoint of the same run scored by the float64 restatement on the CPU stand-in engines (the same
# draws) is 0.263 (the posterior standard deviations of the cutpoint parameters reach 0.18); the test allows 0.4
PLANTED_TOL = 0.4


def planted_problem():
    """K rating data sets of C = 4 ordered classes with planted slopes 0.8 N(0, 1) and cutpoints (-1.2, 0.1, 1.4) + 0.2 N(0, 1)"""
    p = PLANTED
    rs = np.random.RandomState(p["seed"])
    K, N, P, C = p["K"], p["N"], p["P"], p["C"]
    A = rs.standard_normal((K, N, P))
    beta = 0.8 * rs.standard_normal((K, P))
    cuts = np.sort(np.array([-1.2, 0.1, 1.4])[None, :] + 0.2 * rs.standard_normal((K, C - 1)), axis=1)
    eta = np.einsum("knp,kp->kn", A, beta)
    cdf = 1.0 / (1.0 + np.exp(-(cuts[:, None, :] - eta[:, :, None])))
    y = (rs.random_sample((K, N))[:, :, None] > cdf).sum(2)
    return A, y, beta, cuts


def planted_fit(gsmvi_amd, tgt, lbfgs_engine=None, fit_engine=None):
    """lbfgs_init_batched, then GSMBatch.fit from it: (mean, cov, the fit) on the given engines (None: the device)"""
    p = PLANTED
    D = p["P"] + p["C"] - 1
    m0, c0, res = gsmvi_amd.lbfgs_init_batched(np.zeros((p["K"], D)), tgt.lp, tgt.lp_g, **({} if lbfgs_engine is None else
                                                                                          {"engine": lbfgs_engine}))
    assert res.success.all()
    fit = gsmvi_amd.GSMBatch(p["K"], D, tgt.lp, tgt.lp_g, **({} if fit_engine is None else {"engine": fit_engine}))
    mean, cov = fit.fit(np.arange(p["K"]) + 7, mean=m0, cov=c0, batch_size=p["B"], niter=p["niter"], verbose=False)
    return np.asarray(mean), np.asarray(cov), fit


def test_lbfgs_start_then_gsm_fit_recovers_planted_cutpoints():
    """K = 8, N = 300, P = 2, C = 4: from the L-BFGS start, the cutpoints of GSMBatch.fit's mean are within PLANTED_TOL of the
    planted ones for every problem (the tolerance is from the CPU restatement's run of the same fit, with a margin)"""
    import gsmvi_amd
    A, y, beta, cuts = planted_problem()
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, PLANTED["C"], prior_precision=0.01, cut_precision=0.01)
    mean, cov, fit = planted_fit(gsmvi_amd, tgt)
    got = tgt.cutpoints(mean)
    err = np.abs(got - cuts).max()
    print(f"planted cutpoints: worst |fitted - planted| {err:.3f} (allowed {PLANTED_TOL}), reverts {int(fit.n_reverts.sum())}")
    assert np.isfinite(mean).all() and np.isfinite(cov).all() and (np.diff(got, axis=1) > 0).all()
    assert err <= PLANTED_TOL, (got, cuts)


# ---- 6. a captured launch ----------------------------------------------------------------------------------------------------
def test_lp_g_captured_into_a_graph_replays_the_eager_bits():
    import gsmvi_amd
    K, P, C, B = 37, 9, 5, 2
    A, y, o, counts, lam, kap, X = ref.make_inputs(K, 120, P, C, B)
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, C, lam, kap, counts, o)
    eng = tgt.engine
    x = eng.asarray(X)
    eager = tgt.lp_g(x).clone()
    out = eng.empty(K, B, P + C - 1)
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
