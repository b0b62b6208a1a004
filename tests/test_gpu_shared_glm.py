"""The shared-design GLM target on the GPU (gsmvi_glm_shared_batched_f64, csrc/gsmvi_glm_shared_batched.hip), each through the C
ABI: the kernel against the numpy restatement (tests/shared_glm_ref.py) per family at the edges of its tiles, against the
per-problem launch on the replicated design, an exact integer probe of both MFMA layouts, isolation and determinism bit for bit,
saturation and the Poisson overflow rule, the target inside GSMBatch, BaMBatch and ADVIBatch against the same fits scored by the
restatement on the host, and a captured launch."""
import numpy as np
import pytest
import torch

import shared_glm_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

# the kernel's tile constants (csrc/gsmvi_glm_shared_batched.hip): column blocks of 16 (NB = 1 .. 4), k-steps of 4 columns,
# MFMA sub-tiles of 16 observations, tiles of 32, 16 rows of X per wave, 64 per workgroup
DS = [1, 3, 4, 5, 16, 17, 32, 33, 48, 49, 64]
NS = [1, 15, 16, 17, 31, 32, 33, 65]
KNC = [(1, 1), (5, 3), (23, 3), (5, 16), (3, 17), (2, 70)]     # blocks that straddle problems, tail blocks and waves, nc > 64


def _eng():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _dev(eng, A, y, o, w, lam, tau, X):
    reg = lambda v: v if np.ndim(v) == 0 else eng.batched_regs(v)                # noqa: E731
    opt = lambda v: None if v is None else eng.asarray(v)                        # noqa: E731
    return dict(A=eng.asarray(A), y=eng.asarray(y), offset=opt(o), weights=opt(w), prior_prec=reg(lam), noise_prec=reg(tau)), \
        eng.asarray(X)


def _call(eng, family, A, y, o, w, lam, tau, X, want="both"):
    """host arrays in, host arrays out: (G, lp), None for what was not asked"""
    d, dX = _dev(eng, A, y, o, w, lam, tau, X)
    out = eng.glm_shared_batched(dX, family=family, want=want, **d)
    torch.cuda.synchronize()
    if want == "both":
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return (out.cpu().numpy(), None) if want == "g" else (None, out.cpu().numpy())


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _check(eng, family, A, y, o, w, lam, tau, X, tag):
    """the three calls against the restatement at 1e-11 per problem and against each other bit for bit; inputs only read; the
    path bit.  Returns the worst error."""
    K = y.shape[0]
    d, dX = _dev(eng, A, y, o, w, lam, tau, X)
    eng.last_path(reset=True)
    G, lp = eng.glm_shared_batched(dX, family=family, want="both", **d)
    assert eng.last_path(reset=True) == {"batched_target"}
    G1 = eng.glm_shared_batched(dX, family=family, want="g", **d)
    lp1 = eng.glm_shared_batched(dX, family=family, want="lp", **d)
    assert eng.last_path(reset=True) == {"batched_target"}
    assert torch.equal(G1, G) and torch.equal(lp1, lp), tag
    assert _same(d["A"].cpu().numpy(), A) and _same(d["y"].cpu().numpy(), y) and _same(dX.cpu().numpy(), X)
    for name, host in (("offset", o), ("weights", w)):
        assert host is None or _same(d[name].cpu().numpy(), host)
    Gr, lpr = ref.score_and_lp(family, A, y, o, w, lam, tau, X)
    G, lp = G.cpu().numpy(), lp.cpu().numpy()
    assert np.isfinite(Gr).all() and np.isfinite(lpr).all(), tag
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
    """G and lp at 1e-11 per problem (the single-call tolerance) over N x (K, nc): with an offset, weights (exact zeros where y is
    NaN and the offset infinite) and per-problem precisions, and with offset = weights = NULL and scalar precisions"""
    eng = _eng()
    worst = 0.0
    for N in NS:
        for K, nc in KNC:
            A, y, o, w, lam, tau, X = ref.make_inputs(family, K, N, D, nc)
            yp, op = y.copy(), o.copy()
            yp[w == 0.0], op[w == 0.0] = np.nan, np.inf
            worst = max(worst, _check(eng, family, A, yp, op, w, lam, tau, X, (family, D, N, K, nc, "offset, weights")))
            tau0 = 1.3 if family == "gaussian" else 1.0
            worst = max(worst, _check(eng, family, A, y, None, None, 0.7, tau0, X, (family, D, N, K, nc, "scalar")))
    print(f"{family} D={D}: worst rel_err against the restatement {worst:.2e}")


# ---- 2. against the per-problem launch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,D,nc", [(9, 70, 10, 5), (9, 70, 33, 40)])
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_matches_the_per_problem_launch_on_the_replicated_design(family, K, N, D, nc):
    """weights = NULL against glm_batched on the K-fold copy of A, and 0/1 prefix weights against its counts: 1e-11 per problem
    (the two kernels sum in different orders)"""
    eng = _eng()
    A, y, o, _, lam, tau, X = ref.make_inputs(family, K, N, D, nc)
    counts = np.array([N if k == 0 else max(0, N - 1 - 9 * k) for k in range(K)], dtype=np.int32)
    w = (np.arange(N)[None, :] < counts[:, None]).astype(np.float64)
    dA, dy, do, dX = eng.asarray(ref.replicate(A, K)), eng.asarray(y), eng.asarray(o), eng.asarray(X)
    dl = eng.batched_regs(lam)
    dt = eng.batched_regs(tau) if family == "gaussian" else 1.0
    for wk, cnt in ((None, None), (w, eng.batched_counts(counts))):
        Gr, lpr = eng.glm_batched(dX, dA, dy, family, offset=do, counts=cnt, prior_prec=dl, noise_prec=dt, want="both")
        G, lp = _call(eng, family, A, y, o, wk, lam, tau, X)
        Gr, lpr = Gr.cpu().numpy(), lpr.cpu().numpy()
        for k in range(K):
            eg, el = rel_err(G[k], Gr[k]), rel_err(lp[k], lpr[k])
            assert eg <= 1e-11 and el <= 1e-11, (family, wk is None, k, eg, el)


# ---- 3. the layout probe -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,K,nc", [(5, 37, 3, 7), (17, 16, 2, 9), (64, 65, 3, 23)])
def test_integer_data_gives_the_integer_arithmetic_exactly(D, N, K, nc):
    """integer A, X, y and weights without symmetry, gaussian family, tau = 1, lam = 0: every product and partial sum is an
    integer (or a half) below 2^53, so G = sum_n w (y - a . x) a and lp = -sum_n w (y - a . x)^2 / 2 are exact in any order, and
    a row / column swap or a wrong k order in either MFMA product changes them"""
    eng = _eng()
    rs = np.random.RandomState(100 + D)
    A = rs.randint(-4, 6, size=(N, D))
    X = rs.randint(-3, 5, size=(K, nc, D))
    y = rs.randint(-9, 12, size=(K, N))
    for w in (None, rs.randint(0, 4, size=(K, N))):
        r = y[:, None, :] - np.einsum("kcd,nd->kcn", X, A)                       # int64
        wi = np.ones((K, N), dtype=np.int64) if w is None else w
        Gi = np.einsum("kcn,nd->kcd", r * wi[:, None, :], A)
        lpi = -0.5 * (wi[:, None, :] * r * r).sum(2)
        f = lambda v: None if v is None else v.astype(np.float64)                # noqa: E731
        G, lp = _call(eng, "gaussian", f(A), f(y), None, f(w), 0.0, 1.0, f(X))
        assert np.array_equal(G, Gi.astype(np.float64)) and np.array_equal(lp, lpi), (D, w is None)


# ---- 4. isolation and determinism, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [10, 33])
@pytest.mark.parametrize("family", ["poisson", "probit"])
def test_a_problem_and_a_row_give_the_same_bits_alone_and_among_others(family, D):
    eng = _eng()
    K, N, nc = 23, 70, 3
    A, y, o, w, lam, tau, X = ref.make_inputs(family, K, N, D, nc, seed=7 + D)
    G, lp = _call(eng, family, A, y, o, w, lam, tau, X)
    G2, lp2 = _call(eng, family, A, y, o, w, lam, tau, X)
    assert np.isfinite(G).all() and np.isfinite(lp).all()
    assert np.array_equal(G, G2) and np.array_equal(lp, lp2)                     # two runs
    for k in (0, 1, 5, 6, 21, 22):                                              # (problems 5 and 21 straddle two 16-row blocks)
        s = slice(k, k + 1)
        G1, lp1 = _call(eng, family, A, y[s], o[s], w[s], lam[s], tau, X[s])
        assert np.array_equal(G1[0], G[k]) and np.array_equal(lp1[0], lp[k]), k
        for c in range(nc):
            Gc, lpc = _call(eng, family, A, y[s], o[s], w[s], float(lam[k]), tau, np.ascontiguousarray(X[s, c:c + 1]))
            assert np.array_equal(Gc[0, 0], G[k, c]) and np.array_equal(lpc[0, 0], lp[k, c]), (k, c)
    G8, lp8 = _call(eng, family, A, y[:8], o[:8], w[:8], lam[:8], tau, X[:8])
    assert np.array_equal(G8, G[:8]) and np.array_equal(lp8, lp[:8])


@pytest.mark.parametrize("D", [10, 33])
@pytest.mark.parametrize("family", ["poisson", "probit"])
def test_a_non_finite_row_of_x_is_nan_alone(family, D):
    """NaN or an infinity in one row of X: that row's outputs are NaN and every other row keeps its bits -- the other 15 rows of
    its MFMA block and the other rows of its problem among them"""
    eng = _eng()
    K, N, nc = 23, 40, 3
    A, y, o, w, lam, tau, X = ref.make_inputs(family, K, N, D, nc, seed=3 * D)
    G, lp = _call(eng, family, A, y, o, w, lam, tau, X)
    assert np.isfinite(G).all() and np.isfinite(lp).all()
    for badv in (np.nan, np.inf, -np.inf):
        for (k, c, j) in ((0, 0, 0), (2, 1, D // 2), (5, 0, D - 1), (22, 2, D - 1)):     # rows 0, 7, 15 (the last of a block), 68
            X2 = X.copy()
            X2[k, c, j] = badv
            G3, lp3 = _call(eng, family, A, y, o, w, lam, tau, X2)
            assert np.isnan(G3[k, c]).all() and np.isnan(lp3[k, c]), (badv, k, c)
            keep = np.ones((K, nc), dtype=bool)
            keep[k, c] = False
            assert np.array_equal(G3[keep], G[keep]) and np.array_equal(lp3[keep], lp[keep]), (badv, k, c)
            for want in ("g", "lp"):
                g1, l1 = _call(eng, family, A, y, o, w, lam, tau, X2, want=want)
                assert _same(g1 if want == "g" else l1, G3 if want == "g" else lp3), want


# ---- 5. saturation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["probit", "logistic"])
@pytest.mark.parametrize("K,N,D,nc", [(2, 64, 64, 8), (3, 33, 17, 5)])
def test_large_eta_is_finite_and_matches(family, K, N, D, nc):
    eng = _eng()
    A, y, o, w, lam, tau, X = ref.make_inputs(family, K, N, D, nc, scale=10.0)
    X *= 1e4 / np.abs(np.einsum("kcd,nd->kcn", X, A)).max()
    eta = float(np.abs(np.einsum("kcd,nd->kcn", X, A) + o[:, None, :]).max())
    assert 0.99e4 < eta < 1.01e4
    G, lp = _call(eng, family, A, y, o, w, lam, tau, X)
    assert np.isfinite(G).all() and np.isfinite(lp).all()
    worst = _check(eng, family, A, y, o, w, lam, tau, X, (family, K, N, D, nc, "large eta"))
    print(f"{family} N={N} D={D}: max|eta| {eta:.0f}, worst rel_err {worst:.2e}")


@pytest.mark.parametrize("D", [10, 33])
def test_poisson_overflow_flags_its_row_alone_and_not_at_weight_zero(D):
    """one row of X scaled so that eta = 800 at an observation with w > 0: that row is NaN (no inf, no inf * 0), every other row
    has the bits of the same call with that row replaced by zeros; an observation of weight 0 whose exp(eta) would overflow for
    every row of its problem changes nothing"""
    eng = _eng()
    K, N, nc = 9, 70, 5
    A, y, o, w, lam, tau, X = ref.make_inputs("poisson", K, N, D, nc, seed=11 * D)
    for (k, c) in ((5, 2), (0, 0), (8, 4)):
        X2, X0 = X.copy(), X.copy()
        ax = np.where(w[k] > 0.0, A @ X[k, c], 0.0)
        X2[k, c] *= 800.0 / ax[np.argmax(np.abs(ax))]                           # the largest weighted a_n . x becomes + 800
        assert np.where(w[k] > 0.0, A @ X2[k, c] + o[k], 0.0).max() > 710.0
        X0[k, c] = 0.0
        G2, lp2 = _call(eng, "poisson", A, y, o, w, lam, tau, X2)
        G0, lp0 = _call(eng, "poisson", A, y, o, w, lam, tau, X0)
        assert np.isnan(G2[k, c]).all() and np.isnan(lp2[k, c]), (k, c)
        keep = np.ones((K, nc), dtype=bool)
        keep[k, c] = False
        assert np.isfinite(G0).all() and np.isfinite(lp0).all()
        assert np.array_equal(G2[keep], G0[keep]) and np.array_equal(lp2[keep], lp0[keep]), (k, c)
        for want in ("g", "lp"):
            g1, l1 = _call(eng, "poisson", A, y, o, w, lam, tau, X2, want=want)
            assert _same(g1 if want == "g" else l1, G2 if want == "g" else lp2), want
        Gr, lpr = ref.score_and_lp("poisson", A, y, o, w, lam, tau, X2)
        assert np.array_equal(np.isnan(G2), np.isnan(Gr)) and np.array_equal(np.isnan(lp2), np.isnan(lpr))
    n = int(np.flatnonzero(w[4] > 0.0)[0])
    o2, w0 = o.copy(), w.copy()
    o2[4, n], w0[4, n] = 900.0, 0.0
    G, lp = _call(eng, "poisson", A, y, o, w0, lam, tau, X)
    G2, lp2 = _call(eng, "poisson", A, y, o2, w0, lam, tau, X)
    assert np.isfinite(G).all() and np.array_equal(G2, G) and np.array_equal(lp2, lp)
    G3, lp3 = _call(eng, "poisson", A, y, o2, w, lam, tau, X)                   # with its weight back, problem 4 overflows, alone
    others = [k for k in range(K) if k != 4]
    assert np.isnan(G3[4]).all() and np.isnan(lp3[4]).all()
    Gw, lpw = _call(eng, "poisson", A, y, o, w, lam, tau, X)
    assert np.array_equal(G3[others], Gw[others]) and np.array_equal(lp3[others], lpw[others])


# ---- 6. in the fits ----------------------------------------------------------------------------------------------------------
def _per_problem(a, b):
    return max(rel_err(a[k], b[k]) for k in range(a.shape[0]))


@pytest.mark.parametrize("D,B", [(3, 2), (3, 8), (17, 2), (17, 8)])
@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_forced_fits_match_the_same_fits_scored_by_the_restatement(family, D, B):
    """GSMBatch, BaMBatch (forced samples) and ADVIBatch (forced normals, losses tracked) over 30 iterations, scored by the
    target and by the restatement as a plain numpy callable: the same recursion, so the same reverts and mean, cov (and ADVI's
    losses) at 1e-8 per problem, the chained tolerance"""
    import gsmvi_amd
    K, N, niter = 6, 40, 30
    A, y, o, w, lam, tau, _ = ref.make_inputs(family, K, N, D, 1)
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, family, lam, o, w, noise_precision=tau)
    lp_h = lambda X: ref.score_and_lp(family, A, y, o, w, lam, tau, X)[1]        # noqa: E731
    lpg_h = lambda X: ref.score_and_lp(family, A, y, o, w, lam, tau, X)[0]       # noqa: E731
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


# ---- 7. a captured launch ----------------------------------------------------------------------------------------------------
def test_lp_g_captured_into_a_graph_replays_the_eager_bits():
    """one launch on the capturing stream, no parallel branches"""
    import gsmvi_amd
    K, D, B = 37, 10, 2
    A, y, o, w, lam, tau, X = ref.make_inputs("poisson", K, 120, D, B)
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, "poisson", lam, o, w)
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
