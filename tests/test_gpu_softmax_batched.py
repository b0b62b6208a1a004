"""The batched softmax target on the GPU (gsmvi_softmax_batched_f64, csrc/gsmvi_softmax_batched.hip), each through the C ABI: the
kernel against the longdouble restatement (tests/softmax_batched_ref.py) at the edges of the tiling and of the C-dependent X
tile, C = 2 against the logistic entry point, large eta, the row flags, isolation and determinism bit for bit, the target inside
GSMBatch, BaMBatch and ADVIBatch against the same fits scored by the restatement on the host, the L-BFGS initialiser and the
PSIS diagnostic on it, and a captured launch."""
import numpy as np
import pytest
import torch

import softmax_batched_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu


def _eng():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _dev(eng, A, y, counts, lam, X):
    return dict(A=eng.asarray(A), labels=eng.batched_labels(y), counts=None if counts is None else eng.batched_counts(counts),
                prior_prec=lam if np.ndim(lam) == 0 else eng.batched_regs(lam)), eng.asarray(X)


def _call(eng, A, y, Cc, counts, lam, X, want="both"):
    """host arrays in, host arrays out: (G, lp), None for what was not asked"""
    d, dX = _dev(eng, A, y, counts, lam, X)
    out = eng.softmax_batched(dX, num_classes=Cc, want=want, **d)
    torch.cuda.synchronize()
    if want == "both":
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return (out.cpu().numpy(), None) if want == "g" else (None, out.cpu().numpy())


def _check(eng, A, y, Cc, counts, lam, X, tag):
    """the three calls against the longdouble restatement at 1e-11 per problem and against each other bit for bit; inputs only
    read; the path bit.  Returns the worst error."""
    K = A.shape[0]
    d, dX = _dev(eng, A, y, counts, lam, X)
    eng.last_path(reset=True)
    G, lp = eng.softmax_batched(dX, num_classes=Cc, want="both", **d)
    assert eng.last_path(reset=True) == {"batched_softmax"}
    G1 = eng.softmax_batched(dX, num_classes=Cc, want="g", **d)
    lp1 = eng.softmax_batched(dX, num_classes=Cc, want="lp", **d)
    assert eng.last_path(reset=True) == {"batched_softmax"}
    assert torch.equal(G1, G) and torch.equal(lp1, lp), tag
    assert np.array_equal(d["A"].cpu().numpy(), A) and np.array_equal(d["labels"].cpu().numpy(), y) and np.array_equal(dX.cpu().numpy(), X)
    if counts is not None:
        assert np.array_equal(d["counts"].cpu().numpy(), counts)
    Gr, lpr = ref.score_and_lp(A, y, Cc, counts, lam, X, dtype=np.longdouble)
    G, lp = G.cpu().numpy(), lp.cpu().numpy()
    worst = 0.0
    for k in range(K):
        eg, el = rel_err(G[k], Gr[k]), rel_err(lp[k], lpr[k])
        worst = max(worst, eg, el)
        assert eg <= 1e-11 and el <= 1e-11, (tag, k, eg, el)
    return worst


# ---- 1. the kernel against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,P", ref.SHAPES)
def test_kernel_matches_the_longdouble_restatement(Cc, P):
    """G and lp at 1e-11 per problem (the single-call tolerance; the float64 restatement is within 1e-13 of the longdouble one,
    tests/test_softmax_batched_cpu.py) over N x nc, nc at 1, 17, 33 and on both sides of the shape's X tile; with per-problem
    precisions and counts, and with a scalar precision and counts = NULL; K = 5 leaves tail slots in the four-problem packing"""
    eng = _eng()
    worst = 0.0
    for N in ref.NS:
        for nc in ref.nc_grid(Cc, P):
            A, y, counts, lam, X = ref.make_inputs(5, N, Cc, P, nc)
            worst = max(worst, _check(eng, A, y, Cc, counts, lam, X, (Cc, P, N, nc, "counts")))
            worst = max(worst, _check(eng, A, y, Cc, None, 0.7, X, (Cc, P, N, nc, "scalar")))
    print(f"C={Cc} P={P} (X tile {ref.x_tile(Cc, P)}): worst rel_err against the longdouble restatement {worst:.2e}")


# ---- 2. two classes are the logistic model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,P,nc", [(9, 70, 10, 40), (9, 70, 33, 40)])
def test_two_classes_match_the_logistic_entry_point(K, N, P, nc):
    """C = 2 with y = [label = 0] against gsmvi_logistic_batched_f64 on the same data: 1e-13 per problem (the restatements differ
    by 3e-16 there)"""
    eng = _eng()
    A, y, counts, lam, X = ref.make_inputs(K, N, 2, P, nc)
    G, lp = _call(eng, A, y, 2, counts, lam, X)
    Gl, lpl = eng.logistic_batched(eng.asarray(X), eng.asarray(A), eng.asarray((y == 0).astype(np.float64)),
                                   eng.batched_counts(counts), eng.batched_regs(lam), want="both")
    Gl, lpl = Gl.cpu().numpy(), lpl.cpu().numpy()
    for k in range(K):
        eg, el = rel_err(G[k], Gl[k]), rel_err(lp[k], lpl[k])
        print(f"C=2 P={P} k={k}: rel_err against the logistic launch G {eg:.2e} lp {el:.2e}")
        assert eg <= 1e-13 and el <= 1e-13, (k, eg, el)


# ---- 3. large eta ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,Cc,P,rows,scale,eta_min", [(2, 64, 3, 32, 8, 10, 250.0), (2, 100, 5, 16, 4, 40, 800.0)])
def test_large_eta_is_finite_and_matches(K, N, Cc, P, rows, scale, eta_min):
    eng = _eng()
    A, y, counts, lam, X = ref.make_inputs(K, N, Cc, P, rows, scale)
    eta = ref.max_abs_eta(A, counts, X, Cc)
    assert eta > eta_min, eta
    G, lp = _call(eng, A, y, Cc, counts, lam, X)
    print(f"N={N} C={Cc} P={P} scale={scale}: max|eta| {eta:.0f}")
    assert np.isfinite(G).all() and np.isfinite(lp).all()
    _check(eng, A, y, Cc, counts, lam, X, (K, N, Cc, P, rows, scale))


# ---- 4. the row flags ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,P", [(3, 5), (5, 8)])
def test_a_non_finite_row_of_x_is_nan_alone(Cc, P):
    """one row of X in one problem with a NaN or +inf entry: that row is NaN in G and lp, every other row and problem keeps the
    bits of the call with the row zeroed ((3, 5): problems 4 .. 7 share a workgroup)"""
    eng = _eng()
    K, N, nc = 9, 70, 40
    A, y, counts, lam, X = ref.make_inputs(K, N, Cc, P, nc)
    D = (Cc - 1) * P
    for badv in (np.nan, np.inf):
        for (k, c) in ((5, 17), (0, 0), (8, 39)):
            X2, X0 = X.copy(), X.copy()
            X2[k, c, D // 2] = badv
            X0[k, c] = 0.0
            G2, lp2 = _call(eng, A, y, Cc, counts, lam, X2)
            G0, lp0 = _call(eng, A, y, Cc, counts, lam, X0)
            assert np.isfinite(G0).all() and np.isfinite(lp0).all()
            assert np.isnan(G2[k, c]).all() and np.isnan(lp2[k, c]), (badv, k, c)
            keep = np.ones((K, nc), dtype=bool)
            keep[k, c] = False
            assert np.array_equal(G2[keep], G0[keep]) and np.array_equal(lp2[keep], lp0[keep]), (badv, k, c)
            for want in ("g", "lp"):
                g1, l1 = _call(eng, A, y, Cc, counts, lam, X2, want=want)
                assert np.array_equal(g1 if want == "g" else l1, G2 if want == "g" else lp2, equal_nan=True), want


def test_a_non_finite_eta_flags_its_row_alone():
    """finite entries of X and of A whose product is not: the row is NaN, the others keep their bits"""
    eng = _eng()
    K, N, Cc, P, nc = 9, 70, 3, 5, 40
    A, y, counts, lam, X = ref.make_inputs(K, N, Cc, P, nc)
    A[5, 0] = 4.0
    X2, X0 = X.copy(), X.copy()
    X2[5, 17], X0[5, 17] = 1e308, 0.0
    G2, lp2 = _call(eng, A, y, Cc, counts, lam, X2)
    G0, lp0 = _call(eng, A, y, Cc, counts, lam, X0)
    keep = np.ones((K, nc), dtype=bool)
    keep[5, 17] = False
    assert np.isfinite(G0).all() and np.isfinite(lp0).all()
    assert np.isnan(G2[5, 17]).all() and np.isnan(lp2[5, 17])
    assert np.array_equal(G2[keep], G0[keep]) and np.array_equal(lp2[keep], lp0[keep])


# ---- 5. isolation and determinism, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,P", [(3, 5), (5, 8)])
def test_a_problem_gives_the_same_bits_alone_and_in_any_batch(Cc, P):
    eng = _eng()
    N, nc = 70, 5
    A, y, counts, lam, X = ref.make_inputs(1024, N, Cc, P, nc, seed=7 + P)
    Gb, lpb = _call(eng, A, y, Cc, counts, lam, X)
    Gb2, lpb2 = _call(eng, A, y, Cc, counts, lam, X)
    assert np.array_equal(Gb, Gb2) and np.array_equal(lpb, lpb2)                 # two runs
    G16, lp16 = _call(eng, A[:16], y[:16], Cc, counts[:16], lam[:16], X[:16])
    assert np.array_equal(G16, Gb[:16]) and np.array_equal(lp16, lpb[:16])
    for k in (3, 0, 1023):
        s = slice(k, k + 1)
        G1, lp1 = _call(eng, A[s], y[s], Cc, counts[s], lam[s], X[s])
        assert np.array_equal(G1[0], Gb[k]) and np.array_equal(lp1[0], lpb[k]), k
    # the scalar precision and counts = NULL take the same arithmetic
    G1, lp1 = _call(eng, A[5:6], y[5:6], Cc, None, float(lam[5]), X[5:6])
    G2, lp2 = _call(eng, A[5:6], y[5:6], Cc, np.array([N], dtype=np.int32), lam[5:6], X[5:6])
    assert np.array_equal(G1, G2) and np.array_equal(lp1, lp2)


@pytest.mark.parametrize("Cc,P", [(3, 5), (17, 4)])
def test_a_row_gives_the_same_bits_alone_and_among_64(Cc, P):
    """the X tile ((3, 5): 16 rows, (17, 4): 12) plays no part in a row's bits"""
    eng = _eng()
    A, y, counts, lam, X = ref.make_inputs(7, 90, Cc, P, 64, seed=P)
    G, lp = _call(eng, A, y, Cc, counts, lam, X)
    t = ref.x_tile(Cc, P)
    for c in (0, t - 1, t, 2 * t + 1, 63):
        G1, lp1 = _call(eng, A, y, Cc, counts, lam, np.ascontiguousarray(X[:, c:c + 1]))
        assert np.array_equal(G1[:, 0], G[:, c]) and np.array_equal(lp1[:, 0], lp[:, c]), c
    G40, lp40 = _call(eng, A, y, Cc, counts, lam, np.ascontiguousarray(X[:, 20:60]))
    assert np.array_equal(G40, G[:, 20:60]) and np.array_equal(lp40, lp[:, 20:60])


@pytest.mark.parametrize("Cc,P", [(3, 5), (5, 8)])
def test_counts_zero_leaves_the_prior_exactly_and_rows_beyond_counts_play_no_part(Cc, P):
    eng = _eng()
    K, N, nc = 9, 70, 7
    A, y, counts, lam, X = ref.make_inputs(K, N, Cc, P, nc)
    G, lp = _call(eng, A, y, Cc, np.zeros(K, dtype=np.int32), lam, X)
    xx = np.zeros((K, nc))
    for j in range(X.shape[2]):                                                 # the kernel's order of |x|^2
        xx = xx + X[:, :, j] * X[:, :, j]
    assert np.array_equal(G, -(lam[:, None, None] * X)) and np.array_equal(lp, -(0.5 * lam[:, None] * xx))
    Gc, lpc = _call(eng, A, y, Cc, counts, lam, X)
    A2, y2 = A.copy(), y.copy()
    for k in range(1, K):
        A2[k, counts[k]:] = [np.nan, np.inf, -np.inf][k % 3]
        y2[k, counts[k]:] = [-5, 2 ** 31 - 1, Cc][k % 3]
    G2, lp2 = _call(eng, A2, y2, Cc, counts, lam, X)
    assert np.array_equal(G2, Gc) and np.array_equal(lp2, lpc)


# ---- 6. in the fits --------------------------------------------------------------------------------------------------------
def _per_problem(a, b):
    return max(rel_err(a[k], b[k]) for k in range(a.shape[0]))


def test_forced_fits_match_the_same_fits_scored_by_the_restatement():
    """GSMBatch, BaMBatch (forced samples) and ADVIBatch (forced normals, losses tracked) over 30 iterations at K = 8,
    (N, C, P) = (40, 3, 3), scored by the target and by the restatement as a plain numpy callable: the same recursion, so the same
    reverts and mean, cov (and ADVI's losses) at 1e-8 per problem, the chained tolerance of the GLM test of the same name; a
    BatchedKLMonitor fed by the target's lp leaves the fit's bits alone; lbfgs_init_batched converges on all 8 and psis_batched
    returns finite khat."""
    import gsmvi_amd
    K, N, Cc, P, B, niter = 8, 40, 3, 3, 4, 30
    D = (Cc - 1) * P
    A, y, counts, lam, _ = ref.make_inputs(K, N, Cc, P, 1)
    lam = lam + 0.5                                                             # (a proper posterior for every problem)
    tgt = gsmvi_amd.BatchedSoftmaxTarget(A, y, Cc, lam, counts)
    assert (tgt.K, tgt.N, tgt.D, tgt.P, tgt.C) == (K, N, D, P, Cc)
    lp_h = lambda X: ref.score_and_lp(A, y, Cc, counts, lam, X)[1]              # noqa: E731
    lpg_h = lambda X: ref.score_and_lp(A, y, Cc, counts, lam, X)[0]             # noqa: E731
    keys = np.arange(K) + 40
    forced = np.random.RandomState(1000 + D).standard_normal((niter + 1, K, B, D))
    regf = lambda i: 100 / (1 + i)                                              # noqa: E731

    fits = {
        "GSM": lambda lp, lpg: gsmvi_amd.GSMBatch(K, D, lp, lpg),
        "BaM": lambda lp, lpg: gsmvi_amd.BaMBatch(K, D, lp, lpg),
    }
    for name, make in fits.items():
        res = []
        for lp, lpg in ((tgt.lp, tgt.lp_g), (lp_h, lpg_h)):
            f = make(lp, lpg)
            args = (keys,) if name == "GSM" else (keys, regf)
            m, c = f.fit(*args, batch_size=B, niter=niter, verbose=False, forced_samples=forced)
            res.append((m, c, f.n_reverts.copy()))
        (m0, c0, r0), (m1, c1, r1) = res
        em, ec = _per_problem(m0, m1), _per_problem(c0, c1)
        print(f"{name}: forced fit, target against numpy-scored: mean {em:.2e} cov {ec:.2e} reverts {int(r0.sum())}")
        assert np.array_equal(r0, r1), (name, r0, r1)
        assert np.isfinite(m0).all() and np.isfinite(c0).all()
        assert em <= 1e-8 and ec <= 1e-8, (name, em, ec)
    res = []
    for lp, lpg in ((tgt.lp, tgt.lp_g), (lp_h, lpg_h)):
        res.append(gsmvi_amd.ADVIBatch(K, D, lp, lpg).fit(keys, gsmvi_amd.Adam(1e-2), batch_size=B, niter=niter, verbose=False,
                                                         track_loss=True, forced_z=forced))
    (m0, c0, l0), (m1, c1, l1) = res
    em, ec, el = _per_problem(m0, m1), _per_problem(c0, c1), _per_problem(l0.T, l1.T)
    print(f"ADVI: forced fit, target against numpy-scored: mean {em:.2e} cov {ec:.2e} losses {el:.2e}")
    assert np.isfinite(m0).all() and np.isfinite(c0).all() and np.isfinite(l0).all()
    assert em <= 1e-8 and ec <= 1e-8 and el <= 1e-8, (em, ec, el)

    # free-running GSM with and without a monitor whose lp is the target's
    run = lambda monitor: gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, batch_size=B, niter=niter, verbose=False,    # noqa: E731
                                                                        monitor=monitor)
    plain = run(None)
    mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=64, checkpoint=10)
    watched = run(mon)
    assert all(np.array_equal(a, b) for a, b in zip(plain, watched))
    assert len(mon.rkl) == niter // 10 + 2 and all(r.shape == (K,) for r in mon.rkl)

    # the initialiser and the diagnostic take the target through its lp / lp_g
    mean, cov, res = gsmvi_amd.lbfgs_init_batched(np.zeros((K, D)), tgt.lp, tgt.lp_g)
    assert res.success.all() and (res.status == 1).all(), res.status
    g = lpg_h(mean[:, None, :])[:, 0]
    print(f"lbfgs_init_batched: max |score| at the maximisers {np.abs(g).max():.2e}, nit {res.nit.tolist()}")
    assert np.abs(g).max() <= 1e-3
    ps = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=256)
    print(f"psis_batched: khat {np.round(np.asarray(ps.khat), 2).tolist()}")
    assert np.isfinite(np.asarray(ps.khat)).all() and np.asarray(ps.khat).shape == (K,)


# ---- 7. a captured launch --------------------------------------------------------------------------------------------------
def test_lp_g_captured_into_a_graph_replays_the_eager_bits():
    import gsmvi_amd
    K, Cc, P, B = 37, 3, 5, 2
    A, y, counts, lam, X = ref.make_inputs(K, 120, Cc, P, B)
    tgt = gsmvi_amd.BatchedSoftmaxTarget(A, y, Cc, lam, counts)
    eng = tgt.engine
    x = eng.asarray(X)
    eager = tgt.lp_g(x).clone()
    out = eng.empty(K, B, tgt.D)
    tgt.lp_g(x, out=out)                                                        # warm: the context exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tgt.lp_g(x, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(eng.asarray(X[::-1].copy()))                                         # new inputs in the captured buffer
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, tgt.lp_g(x))
