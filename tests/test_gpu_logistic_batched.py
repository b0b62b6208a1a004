"""The batched logistic target on the GPU (csrc/gsmvi_logistic_batched.hip), each through the C ABI: the kernel against the numpy
restatement (tests/logistic_batched_ref.py), isolation and determinism bit for bit, the target inside GSMBatch, BaMBatch and
ADVIBatch against the same fits scored by the restatement on the host, and a captured launch."""
import numpy as np
import pytest
import torch

import logistic_batched_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

DS = [1, 2, 5, 7, 10, 16, 17, 31, 32, 33, 63, 64]           # the list of tests/test_gpu_advi_batched.py
NS = [1, 7, 64, 257, 1000]
NCS = [1, 32, 128]


def _eng():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _dev(eng, A, y, counts, lam, X):
    return (eng.asarray(A), eng.asarray(y), None if counts is None else eng.batched_counts(counts),
            lam if np.ndim(lam) == 0 else eng.batched_regs(lam), eng.asarray(X))


def _call(eng, A, y, counts, lam, X, want="both"):
    """host arrays in, host arrays out: (G, lp), None for what was not asked"""
    dA, dy, dc, dl, dX = _dev(eng, A, y, counts, lam, X)
    out = eng.logistic_batched(dX, dA, dy, dc, dl, want=want)
    torch.cuda.synchronize()
    if want == "both":
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return (out.cpu().numpy(), None) if want == "g" else (None, out.cpu().numpy())


def _check(eng, A, y, counts, lam, X, tag):
    """the three calls against the restatement at 1e-11 per problem and against each other bit for bit; inputs only read; the
    path bit.  Returns the worst error."""
    K = A.shape[0]
    dA, dy, dc, dl, dX = _dev(eng, A, y, counts, lam, X)
    eng.last_path(reset=True)
    G, lp = eng.logistic_batched(dX, dA, dy, dc, dl, want="both")
    assert eng.last_path(reset=True) == {"batched_target"}
    G1 = eng.logistic_batched(dX, dA, dy, dc, dl, want="g")
    lp1 = eng.logistic_batched(dX, dA, dy, dc, dl, want="lp")
    assert eng.last_path(reset=True) == {"batched_target"}
    assert torch.equal(G1, G) and torch.equal(lp1, lp), tag
    assert np.array_equal(dA.cpu().numpy(), A) and np.array_equal(dy.cpu().numpy(), y) and np.array_equal(dX.cpu().numpy(), X)
    if counts is not None:
        assert np.array_equal(dc.cpu().numpy(), counts)
    Gr, lpr = ref.score_and_lp(A, y, counts, lam, X)
    G, lp = G.cpu().numpy(), lp.cpu().numpy()
    worst = 0.0
    for k in range(K):
        eg, el = rel_err(G[k], Gr[k]), rel_err(lp[k], lpr[k])
        worst = max(worst, eg, el)
        assert eg <= 1e-11 and el <= 1e-11, (tag, k, eg, el)
    return worst


# ---- 6. the kernel against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DS)
def test_kernel_matches_the_restatement(D):
    """G and lp at 1e-11 per problem (the single-call tolerance) over N x nc; per-problem precisions with counts, and a scalar
    precision with counts = NULL; K = 5 leaves tail slots in the four-problem packing"""
    eng = _eng()
    worst = 0.0
    for N in NS:
        for nc in NCS:
            A, y, counts, lam, X = ref.make_inputs(5, N, D, nc)
            worst = max(worst, _check(eng, A, y, counts, lam, X, (D, N, nc, "counts")))
            worst = max(worst, _check(eng, A, y, None, 0.7, X, (D, N, nc, "scalar")))
    print(f"D={D}: worst rel_err against the restatement {worst:.2e}")


@pytest.mark.parametrize("K,N,D,rows,scale,eta_min", [(3, 257, 17, 32, 3, 30.0), (2, 64, 64, 8, 10, 250.0), (2, 64, 16, 8, 40, 800.0),
                                                      (2, 100, 33, 4, 40, 800.0)])
def test_large_eta_is_finite_and_matches(K, N, D, rows, scale, eta_min):
    eng = _eng()
    A, y, counts, lam, X = ref.make_inputs(K, N, D, rows, scale)
    eta = max(float(np.abs(X[k] @ A[k, :counts[k]].T).max()) for k in range(K))
    assert eta > eta_min, eta
    worst = _check(eng, A, y, counts, lam, X, (K, N, D, rows, scale))
    G, lp = _call(eng, A, y, counts, lam, X)
    assert np.isfinite(G).all() and np.isfinite(lp).all()
    print(f"N={N} D={D} scale={scale}: max|eta| {eta:.0f}, worst rel_err {worst:.2e}")


def test_soft_labels_and_clamped_counts():
    eng = _eng()
    A, y, counts, lam, X = ref.make_inputs(6, 50, 12, 9, soft=True)
    _check(eng, A, y, counts, lam, X, "soft")
    # counts outside 0 .. N are clamped in the kernel (the host does not read them); 0 rows leave the prior alone
    wild = np.array([-5, 0, 51, 2 ** 30, 50, 17], dtype=np.int32)
    G, lp = _call(eng, A, y, wild, lam, X)
    Gr, lpr = ref.score_and_lp(A, y, np.clip(wild, 0, 50), lam, X)
    assert rel_err(G, Gr) <= 1e-11 and rel_err(lp, lpr) <= 1e-11
    assert np.array_equal(G[1], -lam[1] * X[1]) and rel_err(lp[1], -0.5 * lam[1] * (X[1] * X[1]).sum(1)) <= 1e-15


# ---- 7. isolation and determinism, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [10, 33])
def test_a_problem_gives_the_same_bits_alone_and_in_any_batch(D):
    eng = _eng()
    N, nc = 70, 5
    A, y, counts, lam, X = ref.make_inputs(1024, N, D, nc, seed=7 + D)
    Gb, lpb = _call(eng, A, y, counts, lam, X)
    Gb2, lpb2 = _call(eng, A, y, counts, lam, X)
    assert np.array_equal(Gb, Gb2) and np.array_equal(lpb, lpb2)                 # two runs
    G16, lp16 = _call(eng, A[:16], y[:16], counts[:16], lam[:16], X[:16])
    assert np.array_equal(G16, Gb[:16]) and np.array_equal(lp16, lpb[:16])
    for k in (0, 1, 6, 15, 1023):
        s = slice(k, k + 1)
        G1, lp1 = _call(eng, A[s], y[s], counts[s], lam[s], X[s])
        assert np.array_equal(G1[0], Gb[k]) and np.array_equal(lp1[0], lpb[k]), k
    # the scalar precision and counts = NULL take the same arithmetic
    G1, lp1 = _call(eng, A[5:6], y[5:6], None, float(lam[5]), X[5:6])
    G2, lp2 = _call(eng, A[5:6], y[5:6], np.array([N], dtype=np.int32), lam[5:6], X[5:6])
    assert np.array_equal(G1, G2) and np.array_equal(lp1, lp2)


@pytest.mark.parametrize("D", [10, 33])
def test_a_row_gives_the_same_bits_alone_and_among_128(D):
    eng = _eng()
    A, y, counts, lam, X = ref.make_inputs(7, 90, D, 128, seed=D)
    G, lp = _call(eng, A, y, counts, lam, X)
    for c in (0, 15, 16, 31, 32, 77, 127):
        G1, lp1 = _call(eng, A, y, counts, lam, np.ascontiguousarray(X[:, c:c + 1]))
        assert np.array_equal(G1[:, 0], G[:, c]) and np.array_equal(lp1[:, 0], lp[:, c]), c
    G40, lp40 = _call(eng, A, y, counts, lam, np.ascontiguousarray(X[:, 20:60]))
    assert np.array_equal(G40, G[:, 20:60]) and np.array_equal(lp40, lp[:, 20:60])


@pytest.mark.parametrize("D", [10, 33])
def test_non_finite_entries_stay_where_they_are(D):
    eng = _eng()
    K, N, nc = 9, 70, 40                                                        # (D = 10: problems 4 .. 7 share a workgroup)
    A, y, counts, lam, X = ref.make_inputs(K, N, D, nc, seed=3 * D)
    G, lp = _call(eng, A, y, counts, lam, X)
    assert np.isfinite(G).all() and np.isfinite(lp).all()
    # rows beyond counts[k] contribute nothing, whatever they hold
    A2, y2 = A.copy(), y.copy()
    for k in range(1, K):
        A2[k, counts[k]:] = [np.nan, np.inf, -np.inf][k % 3]
        y2[k, counts[k]:] = [np.inf, np.nan, 7.0][k % 3]
    G2, lp2 = _call(eng, A2, y2, counts, lam, X)
    assert np.array_equal(G2, G) and np.array_equal(lp2, lp)
    # a non-finite entry in one row of X: that row NaN, every other row (its workgroup neighbours included) unchanged
    for badv in (np.nan, np.inf, -np.inf):
        for (k, c) in ((5, 17), (0, 0), (8, 39)):
            X2 = X.copy()
            X2[k, c, D // 2] = badv
            G3, lp3 = _call(eng, A, y, counts, lam, X2)
            assert np.isnan(G3[k, c]).all() and np.isnan(lp3[k, c]), (badv, k, c)
            keep = np.ones((K, nc), dtype=bool)
            keep[k, c] = False
            assert np.array_equal(G3[keep], G[keep]) and np.array_equal(lp3[keep], lp[keep]), (badv, k, c)
    # a NaN in a valid row of A_k, or of y_k: problem k NaN, the rest unchanged
    for which in ("A", "y"):
        A3, y3 = A.copy(), y.copy()
        if which == "A":
            A3[5, 3, D - 1] = np.nan
        else:
            y3[5, 3] = np.nan
        G4, lp4 = _call(eng, A3, y3, counts, lam, X)
        others = [k for k in range(K) if k != 5]
        assert np.isnan(lp4[5]).all() and np.isnan(G4[5]).all(), which
        assert np.array_equal(G4[others], G[others]) and np.array_equal(lp4[others], lp[others]), which


# ---- 8. in the fits --------------------------------------------------------------------------------------------------------
FIT_SHAPES = [(5, 2), (10, 8), (33, 32)]


def _fit_problem(K, D, seed=None):
    A, y, counts, lam, _ = ref.make_inputs(K, 200, D, 1, seed=seed)
    return A, y, counts, lam


def _host_callables(A, y, counts, lam):
    return (lambda X: ref.score_and_lp(A, y, counts, lam, X)[1]), (lambda X: ref.score_and_lp(A, y, counts, lam, X)[0])


def _per_problem(a, b):
    return max(rel_err(a[k], b[k]) for k in range(a.shape[0]))


@pytest.mark.parametrize("D,B", FIT_SHAPES)
def test_forced_fits_match_the_same_fits_scored_by_the_restatement(D, B):
    """GSMBatch, BaMBatch (forced samples) and ADVIBatch (forced normals, losses tracked) over 201 iterations, scored by the
    target and by the restatement as a plain numpy callable: the same recursion, so the same reverts and mean, cov (and ADVI's
    losses) at 1e-8 per problem, the chained tolerance.
    Measured on the MI355X: see DESIGN.md section 9, "Batched logistic target"."""
    import gsmvi_amd
    K, niter = 13, 200
    A, y, counts, lam = _fit_problem(K, D)
    tgt = gsmvi_amd.BatchedLogisticTarget(A, y, lam, counts)
    lp_h, lpg_h = _host_callables(A, y, counts, lam)
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
        print(f"{name} D={D} B={B}: forced fit, target against numpy-scored: mean {em:.2e} cov {ec:.2e} reverts {int(r0.sum())}")
        assert np.array_equal(r0, r1), (name, r0, r1)
        assert np.isfinite(m0).all() and np.isfinite(c0).all()
        assert em <= 1e-8 and ec <= 1e-8, (name, em, ec)
    res = []
    for lp, lpg in ((tgt.lp, tgt.lp_g), (lp_h, lpg_h)):
        res.append(gsmvi_amd.ADVIBatch(K, D, lp, lpg).fit(keys, gsmvi_amd.Adam(1e-2), batch_size=B, niter=niter, verbose=False,
                                                         track_loss=True, forced_z=forced))
    (m0, c0, l0), (m1, c1, l1) = res
    em, ec, el = _per_problem(m0, m1), _per_problem(c0, c1), _per_problem(l0.T, l1.T)
    print(f"ADVI D={D} B={B}: forced fit, target against numpy-scored: mean {em:.2e} cov {ec:.2e} losses {el:.2e}")
    assert np.isfinite(m0).all() and np.isfinite(c0).all() and np.isfinite(l0).all()
    assert em <= 1e-8 and ec <= 1e-8 and el <= 1e-8, (em, ec, el)


@pytest.mark.parametrize("D,B", FIT_SHAPES)
def test_free_running_fits_are_deterministic_isolated_and_left_alone_by_the_monitor(D, B):
    import gsmvi_amd
    niter, Kbig = 200, 1024
    A16, y16, counts16, lam16 = _fit_problem(16, D, seed=50 + D)
    rep = Kbig // 16
    A, y = np.tile(A16, (rep, 1, 1)), np.tile(y16, (rep, 1))
    counts, lam = np.tile(counts16, rep), np.tile(lam16, rep)
    keys = np.arange(Kbig) + 500
    regf = lambda i: 100 / (1 + i)                                              # noqa: E731
    tgt = gsmvi_amd.BatchedLogisticTarget(A, y, lam, counts)
    t13 = gsmvi_amd.BatchedLogisticTarget(A[:13], y[:13], lam[:13], counts[:13])
    lp_h, lpg_h = _host_callables(A[:13], y[:13], counts[:13], lam[:13])

    def run(name, K, t, ks, monitor=None, lp=None, lpg=None):
        lp, lpg = (t.lp, t.lp_g) if lpg is None else (lp, lpg)
        if name == "GSM":
            return gsmvi_amd.GSMBatch(K, D, lp, lpg).fit(ks, batch_size=B, niter=niter, verbose=False, monitor=monitor)
        if name == "BaM":
            return gsmvi_amd.BaMBatch(K, D, lp, lpg).fit(ks, regf, batch_size=B, niter=niter, verbose=False, monitor=monitor)
        return gsmvi_amd.ADVIBatch(K, D, lp, lpg).fit(ks, gsmvi_amd.Adam(1e-2), batch_size=B, niter=niter, verbose=False,
                                                     monitor=monitor)

    for name in ("GSM", "BaM", "ADVI"):
        big = run(name, Kbig, tgt, keys)
        again = run(name, Kbig, tgt, keys)
        assert all(np.array_equal(a, b) for a, b in zip(big, again)), name              # run to run
        assert np.isfinite(big[0]).all() and np.isfinite(big[1]).all(), name
        for k in (0, 5, 15, 1023):                                                      # alone and among 1024
            t1 = gsmvi_amd.BatchedLogisticTarget(A[k:k + 1], y[k:k + 1], lam[k:k + 1], counts[k:k + 1])
            one = run(name, 1, t1, keys[k:k + 1])
            assert np.array_equal(one[0][0], big[0][k]) and np.array_equal(one[1][0], big[1][k]), (name, k)
            if name == "ADVI":
                assert np.array_equal(one[2][:, 0], big[2][:, k]), k
        # the first 13 problems: with and without a monitor whose lp is the target's, and against the numpy-scored fit
        plain = run(name, 13, t13, keys[:13])
        assert np.array_equal(plain[0], big[0][:13]) and np.array_equal(plain[1], big[1][:13]), name
        mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=200, checkpoint=50)
        watched = run(name, 13, t13, keys[:13], monitor=mon)
        assert all(np.array_equal(a, b) for a, b in zip(plain, watched)), name
        assert len(mon.rkl) == niter // 50 + 2 and all(np.isfinite(r).all() and r.shape == (13,) for r in mon.rkl), name
        host = run(name, 13, None, keys[:13], lp=lp_h, lpg=lpg_h)
        print(f"{name} D={D} B={B}: free-running fit, target against numpy-scored (reported, not asserted): "
              f"mean {_per_problem(plain[0], host[0]):.2e} cov {_per_problem(plain[1], host[1]):.2e}; "
              f"reverse KL first -> last, median: {np.median(mon.rkl[0]):.3f} -> {np.median(mon.rkl[-1]):.3f}")


# ---- 9. a captured launch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B", [(10, 8), (33, 32)])
def test_lp_g_captured_into_a_graph_replays_the_eager_bits(D, B):
    import gsmvi_amd
    K = 37
    A, y, counts, lam, X = ref.make_inputs(K, 120, D, B)
    tgt = gsmvi_amd.BatchedLogisticTarget(A, y, lam, counts)
    eng = tgt.engine
    x = eng.asarray(X)
    eager = tgt.lp_g(x).clone()
    out = eng.empty(K, B, D)
    tgt.lp_g(x, out=out)                                                        # warm: the context exists before the capture
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
