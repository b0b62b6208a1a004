"""The batched GLM targets on the GPU (gsmvi_glm_batched_f64, csrc/gsmvi_logistic_batched.hip), each through the C ABI: the kernel
against the numpy restatement (tests/glm_batched_ref.py) per family at the edges of the tiling, the logistic family against its
sibling entry point bit for bit, large eta and the Poisson overflow rule, isolation and determinism bit for bit, the target
inside GSMBatch, BaMBatch and ADVIBatch against the same fits scored by the restatement on the host, and a captured launch."""
import numpy as np
import pytest
import torch

import glm_batched_ref as ref
import logistic_batched_ref as lref
from conftest import rel_err

pytestmark = pytest.mark.gpu

NEW = ("poisson", "probit", "gaussian")
DS = [1, 2, 7, 16, 17, 33, 64]            # the packing switch at 16 / 17, odd D, the maximum
NS = [1, 31, 32, 33, 65]                  # the edges of the 32-row tile of A and of its prefetch
NCS = [1, 17, 33]                         # the edges of TC = 16 and 32


def _eng():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _dev(eng, A, y, o, counts, lam, tau, X):
    reg = lambda v: v if np.ndim(v) == 0 else eng.batched_regs(v)                # noqa: E731
    return dict(A=eng.asarray(A), y=eng.asarray(y), offset=None if o is None else eng.asarray(o),
                counts=None if counts is None else eng.batched_counts(counts), prior_prec=reg(lam), noise_prec=reg(tau)), \
        eng.asarray(X)


def _call(eng, family, A, y, o, counts, lam, tau, X, want="both"):
    """host arrays in, host arrays out: (G, lp), None for what was not asked"""
    d, dX = _dev(eng, A, y, o, counts, lam, tau, X)
    out = eng.glm_batched(dX, family=family, want=want, **d)
    torch.cuda.synchronize()
    if want == "both":
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return (out.cpu().numpy(), None) if want == "g" else (None, out.cpu().numpy())


def _check(eng, family, A, y, o, counts, lam, tau, X, tag):
    """the three calls against the restatement at 1e-11 per problem and against each other bit for bit; inputs only read; the
    path bit.  Returns the worst error."""
    K = A.shape[0]
    d, dX = _dev(eng, A, y, o, counts, lam, tau, X)
    eng.last_path(reset=True)
    G, lp = eng.glm_batched(dX, family=family, want="both", **d)
    assert eng.last_path(reset=True) == {"batched_target"}
    G1 = eng.glm_batched(dX, family=family, want="g", **d)
    lp1 = eng.glm_batched(dX, family=family, want="lp", **d)
    assert eng.last_path(reset=True) == {"batched_target"}
    assert torch.equal(G1, G) and torch.equal(lp1, lp), tag
    assert np.array_equal(d["A"].cpu().numpy(), A) and np.array_equal(d["y"].cpu().numpy(), y) and np.array_equal(dX.cpu().numpy(), X)
    if o is not None:
        assert np.array_equal(d["offset"].cpu().numpy(), o)
    if counts is not None:
        assert np.array_equal(d["counts"].cpu().numpy(), counts)
    Gr, lpr = ref.score_and_lp(family, A, y, o, counts, lam, tau, X)
    G, lp = G.cpu().numpy(), lp.cpu().numpy()
    worst = 0.0
    for k in range(K):
        eg, el = rel_err(G[k], Gr[k]), rel_err(lp[k], lpr[k])
        worst = max(worst, eg, el)
        assert eg <= 1e-11 and el <= 1e-11, (tag, k, eg, el)
    return worst


# ---- 1. the kernel against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_kernel_matches_the_restatement(family, D):
    """G and lp at 1e-11 per problem (the single-call tolerance) over N x nc; with an offset, per-problem precisions and counts,
    and with offset = NULL, a scalar precision and counts = NULL; K = 5 leaves tail slots in the four-problem packing"""
    eng = _eng()
    worst = 0.0
    for N in NS:
        for nc in NCS:
            A, y, o, counts, lam, tau, X = ref.make_inputs(family, 5, N, D, nc)
            worst = max(worst, _check(eng, family, A, y, o, counts, lam, tau, X, (family, D, N, nc, "offset, counts")))
            tau0 = 1.3 if family == "gaussian" else 1.0
            worst = max(worst, _check(eng, family, A, y, None, None, 0.7, tau0, X, (family, D, N, nc, "scalar")))
    print(f"{family} D={D}: worst rel_err against the restatement {worst:.2e}")


@pytest.mark.parametrize("K,N,D,nc", [(9, 70, 10, 40), (9, 70, 33, 40)])
def test_logistic_family_without_offset_is_the_sibling_bit_for_bit(K, N, D, nc):
    eng = _eng()
    A, y, counts, lam, X = lref.make_inputs(K, N, D, nc)
    dA, dy, dc, dl, dX = eng.asarray(A), eng.asarray(y), eng.batched_counts(counts), eng.batched_regs(lam), eng.asarray(X)
    for want in ("g", "lp", "both"):
        for c, l in ((dc, dl), (None, 0.7)):
            a = eng.logistic_batched(dX, dA, dy, c, l, want=want)
            b = eng.glm_batched(dX, dA, dy, "logistic", offset=None, counts=c, prior_prec=l, want=want)
            a, b = (a, b) if want == "both" else ((a,), (b,))
            assert all(torch.equal(u, v) for u, v in zip(a, b)), (want, c is None)


# ---- 2. large eta ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["probit", "gaussian"])
@pytest.mark.parametrize("K,N,D,rows,scale,eta_min", [(2, 64, 64, 8, 10, 250.0), (2, 100, 33, 4, 40, 800.0)])
def test_large_eta_is_finite_and_matches(family, K, N, D, rows, scale, eta_min):
    eng = _eng()
    A, y, o, counts, lam, tau, X = ref.make_inputs(family, K, N, D, rows, scale)
    eta = max(float(np.abs(X[k] @ A[k, :counts[k]].T + o[k, None, :counts[k]]).max()) for k in range(K))
    assert eta > eta_min, eta
    G, lp = _call(eng, family, A, y, o, counts, lam, tau, X)
    Gr, lpr = ref.score_and_lp(family, A, y, o, counts, lam, tau, X)
    for k in range(K):
        print(f"{family} N={N} D={D} scale={scale} k={k}: max|eta| {eta:.0f}, rel_err G {rel_err(G[k], Gr[k]):.2e} "
              f"lp {rel_err(lp[k], lpr[k]):.2e}")
    assert np.isfinite(G).all() and np.isfinite(lp).all()
    _check(eng, family, A, y, o, counts, lam, tau, X, (family, K, N, D, rows, scale))


@pytest.mark.parametrize("D", [10, 33])
def test_poisson_overflow_flags_its_row_alone(D):
    """one row of X in one problem scaled so that eta > 710: that row is NaN (no inf, no inf * 0), every other row and problem
    has the bits of the same call with that row replaced by zeros"""
    eng = _eng()
    K, N, nc = 9, 70, 40
    A, y, o, counts, lam, tau, X = ref.make_inputs("poisson", K, N, D, nc, seed=11 * D)
    for (k, c) in ((5, 17), (0, 0), (8, 39)):
        X2, X0 = X.copy(), X.copy()
        ax = X[k, c] @ A[k, :counts[k]].T
        X2[k, c] *= 800.0 / ax[np.argmax(np.abs(ax))]                           # the largest a_n . x becomes + 800
        assert (X2[k, c] @ A[k, :counts[k]].T + o[k, :counts[k]]).max() > 710.0
        X0[k, c] = 0.0
        G2, lp2 = _call(eng, "poisson", A, y, o, counts, lam, tau, X2)
        G0, lp0 = _call(eng, "poisson", A, y, o, counts, lam, tau, X0)
        assert np.isnan(G2[k, c]).all() and np.isnan(lp2[k, c]), (k, c)
        keep = np.ones((K, nc), dtype=bool)
        keep[k, c] = False
        assert np.isfinite(G0).all() and np.isfinite(lp0).all()
        assert np.array_equal(G2[keep], G0[keep]) and np.array_equal(lp2[keep], lp0[keep]), (k, c)
        for want in ("g", "lp"):
            g1, l1 = _call(eng, "poisson", A, y, o, counts, lam, tau, X2, want=want)
            assert np.array_equal(g1 if want == "g" else l1, G2 if want == "g" else lp2, equal_nan=True), want
        Gr, lpr = ref.score_and_lp("poisson", A, y, o, counts, lam, tau, X2)
        assert np.array_equal(np.isnan(G2), np.isnan(Gr)) and np.array_equal(np.isnan(lp2), np.isnan(lpr))


# ---- 3. isolation and determinism, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [10, 33])
@pytest.mark.parametrize("family", ["poisson", "probit"])
def test_a_problem_gives_the_same_bits_alone_and_in_any_batch(family, D):
    eng = _eng()
    N, nc = 70, 5
    A, y, o, counts, lam, tau, X = ref.make_inputs(family, 1024, N, D, nc, seed=7 + D)
    Gb, lpb = _call(eng, family, A, y, o, counts, lam, tau, X)
    Gb2, lpb2 = _call(eng, family, A, y, o, counts, lam, tau, X)
    assert np.array_equal(Gb, Gb2) and np.array_equal(lpb, lpb2)                 # two runs
    G16, lp16 = _call(eng, family, A[:16], y[:16], o[:16], counts[:16], lam[:16], tau, X[:16])
    assert np.array_equal(G16, Gb[:16]) and np.array_equal(lp16, lpb[:16])
    for k in (0, 1, 6, 15, 1023):
        s = slice(k, k + 1)
        G1, lp1 = _call(eng, family, A[s], y[s], o[s], counts[s], lam[s], tau, X[s])
        assert np.array_equal(G1[0], Gb[k]) and np.array_equal(lp1[0], lpb[k]), k
    # the scalar precision and counts = NULL take the same arithmetic
    G1, lp1 = _call(eng, family, A[5:6], y[5:6], o[5:6], None, float(lam[5]), tau, X[5:6])
    G2, lp2 = _call(eng, family, A[5:6], y[5:6], o[5:6], np.array([N], dtype=np.int32), lam[5:6], tau, X[5:6])
    assert np.array_equal(G1, G2) and np.array_equal(lp1, lp2)


@pytest.mark.parametrize("D", [10, 33])
@pytest.mark.parametrize("family", ["poisson", "probit"])
def test_a_row_gives_the_same_bits_alone_and_among_128(family, D):
    eng = _eng()
    A, y, o, counts, lam, tau, X = ref.make_inputs(family, 7, 90, D, 128, seed=D)
    G, lp = _call(eng, family, A, y, o, counts, lam, tau, X)
    for c in (0, 15, 16, 31, 32, 77, 127):
        G1, lp1 = _call(eng, family, A, y, o, counts, lam, tau, np.ascontiguousarray(X[:, c:c + 1]))
        assert np.array_equal(G1[:, 0], G[:, c]) and np.array_equal(lp1[:, 0], lp[:, c]), c
    G40, lp40 = _call(eng, family, A, y, o, counts, lam, tau, np.ascontiguousarray(X[:, 20:60]))
    assert np.array_equal(G40, G[:, 20:60]) and np.array_equal(lp40, lp[:, 20:60])


@pytest.mark.parametrize("D", [10, 33])
@pytest.mark.parametrize("family", ["poisson", "probit"])
def test_non_finite_entries_stay_where_they_are(family, D):
    eng = _eng()
    K, N, nc = 9, 70, 40                                                        # (D = 10: problems 4 .. 7 share a workgroup)
    A, y, o, counts, lam, tau, X = ref.make_inputs(family, K, N, D, nc, seed=3 * D)
    G, lp = _call(eng, family, A, y, o, counts, lam, tau, X)
    assert np.isfinite(G).all() and np.isfinite(lp).all()
    # rows beyond counts[k] contribute nothing, whatever they hold
    A2, y2, o2 = A.copy(), y.copy(), o.copy()
    for k in range(1, K):
        A2[k, counts[k]:] = [np.nan, np.inf, -np.inf][k % 3]
        y2[k, counts[k]:] = [np.inf, np.nan, 7.0][k % 3]
        o2[k, counts[k]:] = [-np.inf, 900.0, np.nan][k % 3]
    G2, lp2 = _call(eng, family, A2, y2, o2, counts, lam, tau, X)
    assert np.array_equal(G2, G) and np.array_equal(lp2, lp)
    # a non-finite entry in one row of X: that row NaN, every other row (its workgroup neighbours included) unchanged
    for badv in (np.nan, np.inf, -np.inf):
        for (k, c) in ((5, 17), (0, 0), (8, 39)):
            X2 = X.copy()
            X2[k, c, D // 2] = badv
            G3, lp3 = _call(eng, family, A, y, o, counts, lam, tau, X2)
            assert np.isnan(G3[k, c]).all() and np.isnan(lp3[k, c]), (badv, k, c)
            keep = np.ones((K, nc), dtype=bool)
            keep[k, c] = False
            assert np.array_equal(G3[keep], G[keep]) and np.array_equal(lp3[keep], lp[keep]), (badv, k, c)
    # a NaN in a valid row of A_k, y_k or the offset: problem k NaN, the rest unchanged
    for which in ("A", "y", "offset"):
        A3, y3, o3 = A.copy(), y.copy(), o.copy()
        if which == "A":
            A3[5, 3, D - 1] = np.nan
        elif which == "y":
            y3[5, 3] = np.nan
        else:
            o3[5, 3] = np.nan
        G4, lp4 = _call(eng, family, A3, y3, o3, counts, lam, tau, X)
        others = [k for k in range(K) if k != 5]
        assert np.isnan(lp4[5]).all() and np.isnan(G4[5]).all(), which
        assert np.array_equal(G4[others], G[others]) and np.array_equal(lp4[others], lp[others]), which


# ---- 4. in the fits --------------------------------------------------------------------------------------------------------
def _per_problem(a, b):
    return max(rel_err(a[k], b[k]) for k in range(a.shape[0]))


@pytest.mark.parametrize("D,B", [(5, 2), (17, 4)])
@pytest.mark.parametrize("family", NEW)
def test_forced_fits_match_the_same_fits_scored_by_the_restatement(family, D, B):
    """GSMBatch, BaMBatch (forced samples) and ADVIBatch (forced normals, losses tracked) over 30 iterations, scored by the
    target and by the restatement as a plain numpy callable: the same recursion, so the same reverts and mean, cov (and ADVI's
    losses) at 1e-8 per problem, the chained tolerance; and a BatchedKLMonitor fed by the target's lp leaves the fit's bits
    alone."""
    import gsmvi_amd
    K, N, niter = 6, 40, 30
    A, y, o, counts, lam, tau, _ = ref.make_inputs(family, K, N, D, 1)
    tgt = gsmvi_amd.BatchedGLMTarget(A, y, family, lam, counts, o, noise_precision=tau)
    lp_h = lambda X: ref.score_and_lp(family, A, y, o, counts, lam, tau, X)[1]   # noqa: E731
    lpg_h = lambda X: ref.score_and_lp(family, A, y, o, counts, lam, tau, X)[0]  # noqa: E731
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
        print(f"{family} {name} D={D} B={B}: forced fit, target against numpy-scored: mean {em:.2e} cov {ec:.2e} "
              f"reverts {int(r0.sum())}")
        assert np.array_equal(r0, r1), (name, r0, r1)
        assert np.isfinite(m0).all() and np.isfinite(c0).all()
        assert em <= 1e-8 and ec <= 1e-8, (name, em, ec)
    res = []
    for lp, lpg in ((tgt.lp, tgt.lp_g), (lp_h, lpg_h)):
        res.append(gsmvi_amd.ADVIBatch(K, D, lp, lpg).fit(keys, gsmvi_amd.Adam(1e-2), batch_size=B, niter=niter, verbose=False,
                                                         track_loss=True, forced_z=forced))
    (m0, c0, l0), (m1, c1, l1) = res
    em, ec, el = _per_problem(m0, m1), _per_problem(c0, c1), _per_problem(l0.T, l1.T)
    print(f"{family} ADVI D={D} B={B}: forced fit, target against numpy-scored: mean {em:.2e} cov {ec:.2e} losses {el:.2e}")
    assert np.isfinite(m0).all() and np.isfinite(c0).all() and np.isfinite(l0).all()
    assert em <= 1e-8 and ec <= 1e-8 and el <= 1e-8, (em, ec, el)

    # free-running, with and without a monitor whose lp is the target's
    def run(name, monitor=None):
        if name == "GSM":
            return gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, batch_size=B, niter=niter, verbose=False, monitor=monitor)
        if name == "BaM":
            return gsmvi_amd.BaMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, regf, batch_size=B, niter=niter, verbose=False,
                                                                  monitor=monitor)
        return gsmvi_amd.ADVIBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, gsmvi_amd.Adam(1e-2), batch_size=B, niter=niter,
                                                               verbose=False, monitor=monitor)

    for name in ("GSM", "BaM", "ADVI"):
        plain = run(name)
        mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=64, checkpoint=10)
        watched = run(name, monitor=mon)
        assert all(np.array_equal(a, b) for a, b in zip(plain, watched)), name
        assert len(mon.rkl) == niter // 10 + 2 and all(r.shape == (K,) for r in mon.rkl), name


# ---- 5. a captured launch --------------------------------------------------------------------------------------------------
def test_lp_g_captured_into_a_graph_replays_the_eager_bits():
    import gsmvi_amd
    K, D, B = 37, 10, 2
    A, y, o, counts, lam, tau, X = ref.make_inputs("poisson", K, 120, D, B)
    tgt = gsmvi_amd.BatchedGLMTarget(A, y, "poisson", lam, counts, o)
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
