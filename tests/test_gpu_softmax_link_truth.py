"""The multinomial logit link on the GPU, element by element, against the truth of tests/softmax_link_truth.py (mpmath, committed
as tests/golden/softmax_link_truth.npz; this file needs no mpmath).  No kernel of its own: with rows a = alpha e_1, N = 1 (or one
row per label), one vector per point and prior_prec = 0 the outputs of the public entry points ARE the link values (the layouts
of softmax_link_truth), and eta is formed exactly in two ways, (alpha = 1, x = eta) and (alpha = 1 / 2, x = 2 eta), which must
agree bit for bit where |value| >= 2^-1000.  Every value of every probe is held to

    |got - truth| <= c eps (|f| + sum_c |eta_c df/deta_c| + a_f) + 2^-1070,   c = max(16, 4 x the worst ratio of the float64
                                                                              restatement on the CPU)

(softmax_link_truth.C_CPU, asserted in tests/test_softmax_link_truth_cpu.py; never the device's own figures, which are printed).
With log(s) in place of log1p(rest) the density's term is 0 where the reference class wins by more than 1 / eps: 1.1e14 units at
C = 3, eta = (-1e150, -37.5), y = 2, and lp = 0 exactly at the realistic shape of the last test."""
import functools
import math

import numpy as np
import pytest
import torch

import softmax_link_truth as truth

pytestmark = pytest.mark.gpu

FORMS = (1.0, 0.5)                                  # alpha; x = eta / alpha


@functools.lru_cache(maxsize=None)
def _table():
    return truth.load_table()


@functools.lru_cache(maxsize=None)
def _rows(name):
    """(free entries, rows) of a set of the table: computed once and shared (do not modify)"""
    return _table()["eta_" + name], truth.rows(_table(), name, w=True)


def _eng():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _hold(probe, q, got, row, where, worst, c=None, scale=None, key=None):
    """every element within c eps of its scale; records and returns the worst ratio"""
    c = truth.c_gpu(probe, key or q) if c is None else c
    ratio = truth.ratio(got, row, q, scale)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert ratio[i] <= c, (where, probe, key or q, f"at {i}, eta = {row['eta'][i[0]][:6]!r}..: got {got[i]!r}, truth {row[q][i]!r}, "
                           f"{ratio[i]:.3g} eps of its scale, bound {c}")
    worst[probe, key or q] = max(worst.get((probe, key or q), 0.0), float(ratio[i]))
    return float(ratio[i])


def _report(worst, what):
    for (probe, q), v in sorted(worst.items()):
        print(f"{what}: {probe} {q}: worst device ratio {v:.2f} eps of the scale (CPU restatement {truth.C_CPU[probe, q]}, "
              f"bound {truth.c_gpu(probe, q)})")


def _same(a, b, what):
    """two forms of the same eta: the same bits where the value is not near the subnormal range (x / 2 of a subnormal drops a bit)"""
    big = (np.abs(a) >= 2.0 ** -1000) | (np.abs(b) >= 2.0 ** -1000)
    assert np.array_equal(a[big], b[big]), what


# ---- 1. the score and the density ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", truth.SHAPES, ids=str)
def test_softmax_batched_is_the_link_element_by_element(shape):
    """lp[y, v] = t and G[y, v, c P] = alpha r_c; want = g, lp and both agree bit for bit; a zero feature gives a zero"""
    eng = _eng()
    C, P = shape
    free, row = _rows(str(C))
    V, Cm = free.shape
    worst, out = {}, []
    for alpha in FORMS:
        A, y, X = truth.layout_score(free, P, alpha)
        A, y, X = eng.asarray(A), eng.batched_labels(y), eng.asarray(X)
        G, lp = eng.softmax_batched(X, A, y, C, prior_prec=0.0, want="both")
        assert torch.equal(eng.softmax_batched(X, A, y, C, prior_prec=0.0, want="g"), G), (shape, alpha)
        assert torch.equal(eng.softmax_batched(X, A, y, C, prior_prec=0.0, want="lp"), lp), (shape, alpha)
        Gn = G.cpu().numpy().reshape(C, V, Cm, P)
        assert not Gn[..., 1:].any(), (shape, alpha)
        t, r = lp.cpu().numpy().T, np.swapaxes(Gn[..., 0], 0, 1) / alpha
        _hold("score", "t", t, row, (shape, alpha), worst)
        _hold("score", "r", r, row, (shape, alpha), worst)
        out.append((t, r))
    _same(out[0][0], out[1][0], (shape, "t"))
    _same(out[0][1], out[1][1], (shape, "r"))
    _report(worst, f"softmax_batched {shape}")


# ---- 2. the Hessian ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", truth.SHAPES, ids=str)
def test_softmax_hessian_batched_is_the_weight_element_by_element(shape):
    """N = 1: H[c P, c' P] = alpha^2 w_cc' with 1 - p a sum over the other classes; H exactly symmetric, its diagonal >= 0, and
    every entry that multiplies a zero feature exactly 0"""
    eng = _eng()
    C, P = shape
    free, row = _rows(str(C))
    V, Cm = free.shape
    worst, out = {}, []
    for alpha in FORMS:
        A, y, X = truth.layout_point(free, P, alpha)
        H = eng.softmax_hessian_batched(eng.asarray(X), eng.asarray(A), eng.batched_labels(y), C, prior_prec=0.0, want="h")
        Hn = H.cpu().numpy()
        assert np.array_equal(Hn, np.swapaxes(Hn, 1, 2)), (shape, alpha)
        assert (np.diagonal(Hn, axis1=1, axis2=2) >= 0.0).all(), (shape, alpha)
        blocks = Hn.reshape(V, Cm, P, Cm, P)
        used = np.zeros((P, P), dtype=bool)
        used[0, 0] = True
        assert not blocks[:, :, ~used[:, None, :].repeat(Cm, 1)].any(), (shape, alpha)
        w = blocks[:, :, 0, :, 0] / (alpha * alpha)
        _hold("hessian", "w", w, row, (shape, alpha), worst)
        out.append(w)
    _same(out[0], out[1], (shape, "w"))
    _report(worst, f"softmax_hessian_batched {shape}")


# ---- 3. the Newton step's start ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", truth.SHAPES, ids=str)
def test_softmax_laplace_step_start_is_the_link_element_by_element(shape):
    """one problem per (vector, label), N = 1: after the start launch f = -t and g[c P] = -alpha r_c.  The kernel's residual at the
    label's class is q_y, a sum over the other classes, so there it is also held without a_r = [y = c] + p_c in the scale"""
    eng = _eng()
    C, P = shape
    free, row = _rows(str(C))
    V, Cm = free.shape
    label = np.eye(C, dtype=bool)[None, :, :Cm]
    worst, out = {}, []
    for alpha in FORMS:
        A, y, x0 = truth.layout_step(free, P, alpha)
        st = eng.laplace_state_batched(eng.asarray(x0))
        eng.softmax_laplace_step_batched(st, eng.asarray(A), eng.batched_labels(y), C, prior_prec=0.0, start=True, maxiter=10,
                                         maxfun=20, gtol=1e-8)
        g = st["g"].cpu().numpy().reshape(V, C, Cm, P)
        assert not g[..., 1:].any(), (shape, alpha)
        t, r = -st["sc"][:, 0].cpu().numpy().reshape(V, C), -g[..., 0] / alpha
        _hold("laplace", "t", t, row, (shape, alpha), worst)
        _hold("laplace", "r", r, row, (shape, alpha), worst)
        rq = np.where(label, r, row["r"])                               # (off the label's class: the truth itself, ratio 0)
        _hold("laplace", "r", rq, row, (shape, alpha, "q_y"), worst, scale=row["scale_rq"], key="rq")
        out.append((t, r))
    _same(out[0][0], out[1][0], (shape, "t"))
    _same(out[0][1], out[1][1], (shape, "r"))
    _report(worst, f"softmax_laplace_step_batched {shape}")


# ---- 4. the leave-one-out's pointwise log-likelihood ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", truth.SHAPES, ids=str)
def test_psis_loo_softmax_loglik_is_the_link_element_by_element(shape):
    """the draws are the vectors and the rows the C labels: loglik[k, y, s] = t; problem 0 with alpha = 1, problem 1 with 1 / 2.
    logr is any finite distinct values and lw = -log S: only loglik is held here"""
    eng = _eng()
    C, P = shape
    free, row = _rows(str(C))
    V = free.shape[0]
    lay = [truth.layout_rows(free, P, alpha, False) for alpha in FORMS]
    A, y, X = (np.concatenate([f[i] for f in lay]) for i in range(3))
    S = X.shape[1]
    assert 5 <= S <= 4096
    logr = np.tile(np.linspace(-1.0, 1.0, S), (2, 1))
    lw = np.full((2, S), -math.log(S))
    ll = eng.psis_loo_softmax_batched(eng.asarray(X), eng.asarray(logr), eng.asarray(lw), eng.asarray(A), eng.batched_labels(y), C,
                                      pointwise_loglik=True)[5].cpu().numpy()
    worst = {}
    t = [ll[k, :, :V].T for k in range(2)]
    for k in range(2):
        _hold("loo", "t", t[k], row, (shape, FORMS[k]), worst)
    _same(t[0], t[1], (shape, "t"))
    _report(worst, f"psis_loo_softmax_batched {shape}")


# ---- 5. the predictive ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draws", [1, 5])
@pytest.mark.parametrize("shape", truth.SHAPES, ids=str)
def test_softmax_predict_batched_of_equal_draws_is_the_link(shape, draws):
    """one problem per vector, its C rows labelled 0 .. C - 1, S equal draws and uniform weights: prob[k, i, c] = p_c for every row
    i and lpd[k, y] = t.  The predictive adds terms of its own, so do its bounds:
      prob   exp(eta - m) (w / z): p's bound plus 4 eps for the division w / z and the product, and (S - 1) / 2 for the fixed-tree
             sum of S equal positive terms
      lpd    max_s f_s + log sum_s exp(f_s - max), f_s = lw + t with lw = -log S: t's bound plus 4 for the final log and the two
             additions, plus (S - 1) / 2, on t's scale plus the magnitudes of what is added, |lw| and log S
    and the rows of prob sum to 1 within C eps"""
    eng = _eng()
    C, P = shape
    free, row = _rows(str(C))
    extra = 4.0 + (draws - 1) / 2.0
    worst, out = {}, []
    for alpha in FORMS:
        A, y, X = truth.layout_rows(free, P, alpha, True)
        X = np.repeat(X, draws, axis=1)
        prob, lpd = eng.softmax_predict_batched(eng.asarray(X), None, eng.asarray(A), C, labels=eng.batched_labels(y))
        prob, lpd = prob.cpu().numpy(), lpd.cpu().numpy()
        assert all(np.array_equal(prob[:, 0], prob[:, i]) for i in range(1, C)), (shape, alpha)
        p = prob[:, 0]
        assert np.abs(p.sum(axis=1) - 1.0).max() <= C * truth.EPS, (shape, alpha)
        _hold("predict", "p", p, row, (shape, alpha), worst, c=truth.c_gpu("predict", "p") + extra)
        _hold("predict", "t", lpd, row, (shape, alpha), worst, c=truth.c_gpu("predict", "t") + extra,
              scale=row["scale_t"] + 2.0 * math.log(draws))
        out.append((p, lpd))
    _same(out[0][0], out[1][0], (shape, "p"))
    _same(out[0][1], out[1][1], (shape, "t"))
    _report(worst, f"softmax_predict_batched {shape} S = {draws}")


# ---- 6. beyond the table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", sorted(truth.BEYOND))
def test_beyond_1e150_nothing_is_nan_and_the_signs_are_right(C):
    """|eta| = 1e160 and 1e300 (P = 1, eta = a x with a = BEYOND_A so that |x|^2 stays finite): no NaN where the truth is finite (it
    is everywhere), r has the truth's sign (a zero where the truth rounds to 0), p is exactly 0 or 1 where the truth rounds to that"""
    eng = _eng()
    free, row = _rows(f"b{C}")
    V, Cm = free.shape
    a = truth.BEYOND_A
    A, y, X = truth.layout_score(free, 1, a)
    G, lp = eng.softmax_batched(eng.asarray(X), eng.asarray(A), eng.batched_labels(y), C, prior_prec=0.0, want="both")
    t, r = lp.cpu().numpy().T, np.swapaxes(G.cpu().numpy(), 0, 1) / a
    A, y, X = truth.layout_point(free, 1, a)
    H = eng.softmax_hessian_batched(eng.asarray(X), eng.asarray(A), eng.batched_labels(y), C, prior_prec=0.0, want="h").cpu().numpy()
    A, y, X = truth.layout_rows(free, 1, a, True)
    prob, lpd = eng.softmax_predict_batched(eng.asarray(X), None, eng.asarray(A), C, labels=eng.batched_labels(y))
    p, lpd = prob.cpu().numpy()[:, 0], lpd.cpu().numpy()
    A, y, x0 = truth.layout_step(free, 1, a)
    st = eng.laplace_state_batched(eng.asarray(x0))
    eng.softmax_laplace_step_batched(st, eng.asarray(A), eng.batched_labels(y), C, prior_prec=0.0, start=True, maxiter=10,
                                     maxfun=20, gtol=1e-8)
    f, g = st["sc"][:, 0].cpu().numpy(), st["g"].cpu().numpy().reshape(V, C, Cm) / a
    assert np.isfinite(row["t"]).all()
    for name, v in (("t", t), ("r", r), ("H", H), ("p", p), ("lpd", lpd), ("f", f), ("g", g)):
        assert np.isfinite(v).all(), (C, name, v)
    for name, v in (("r", r), ("-g", -g)):
        assert ((np.sign(v) == np.sign(row["r"])) | ((v == 0.0) & (row["r"] == 0.0))).all(), (C, name, v, row["r"])
    sat = (row["p"] == 0.0) | (row["p"] == 1.0)
    assert sat.any() and np.array_equal(p[sat], row["p"][sat]), (C, p, row["p"])
    assert (np.diagonal(H, axis1=1, axis2=2) >= 0.0).all() and np.array_equal(H, np.swapaxes(H, 1, 2))
    assert (np.sign(t) == np.sign(row["t"])).all() and (np.sign(lpd) == np.sign(row["t"])).all(), (C, t, row["t"])


# ---- 7. one realistic shape ----------------------------------------------------------------------------------------------------------
def test_reference_class_saturated_problem_has_its_density_and_score():
    """(K, N, C, P) = (5, 33, 5, 4), every row labelled with the reference class and every valid eta <= -37.5, lam = 0: lp against the
    longdouble sum of the truth's t at 1e-11 of |lp| ITSELF (about 1e-15 per problem: with log(s) for log1p(rest) every term, and
    lp, is exactly 0), and the score against -sum_n p_nc a_n, a sum of terms of one sign, at 1e-11 of each entry"""
    A, y, counts, X, eta = truth.real_problem()
    K, N, C, P = truth.REAL_SHAPE
    free, row = _rows("real")
    assert np.array_equal(eta, free)
    valid = np.arange(N)[None, :] < counts[:, None]
    assert (eta.reshape(K, N, C - 1)[valid] <= truth.REAL_TOP).all() and (y == C - 1).all()
    L = np.longdouble
    lp_t = ((row["t"][:, C - 1].astype(L) + row["t_lo"][:, C - 1].astype(L)).reshape(K, N) * valid).sum(axis=1)
    pt = ((row["p"][:, :C - 1].astype(L) + row["p_lo"][:, :C - 1].astype(L)).reshape(K, N, C - 1) * valid[:, :, None])
    G_t = -np.einsum("knc,knp->kcp", pt, A.astype(L)).reshape(K, (C - 1) * P)
    eng = _eng()
    G, lp = eng.softmax_batched(eng.asarray(X), eng.asarray(A), eng.batched_labels(y), C, counts=eng.batched_counts(counts),
                                prior_prec=0.0, want="both")
    G, lp = G.cpu().numpy()[:, 0], lp.cpu().numpy()[:, 0]
    e_lp = np.abs(lp.astype(L) - lp_t) / np.abs(lp_t)
    e_G = np.abs(G.astype(L) - G_t) / np.abs(G_t)
    print(f"reference-class-saturated problem: lp {lp!r}, truth {lp_t.astype(np.float64)!r}: worst error {float(e_lp.max()):.2e} of "
          f"|lp|; score: worst error {float(e_G.max()):.2e} of the entry")
    assert (lp_t < 0).all() and e_lp.max() <= 1e-11, (lp, lp_t)
    assert e_G.max() <= 1e-11
