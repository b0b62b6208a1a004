"""The GLM links on the GPU, element by element, against the truth of tests/glm_link_truth.py (mpmath, committed as
tests/golden/glm_link_truth.npz; this file needs no mpmath).  No kernel of its own: with D = 1, N = 1 and lam = 0 an output of a
public entry point IS a link value, G[k, c] = a r, lp[k, c] = t, H[k, 0, 0] = a^2 w, and eta is formed exactly in three ways:
(a = 1, x = eta), (a = 1 / 2, x = 2 eta) and (a = 1, x = 0, offset = eta).  Every value of every probe is held to

    |got - truth| <= c eps (|f| + |eta f'| + a_f) + 2^-1070,   c = max(16, 4 x the worst ratio of the float64 restatement on the CPU)

(glm_link_truth.C_CPU, asserted in tests/test_glm_link_truth_cpu.py; never the device's own figures, which are printed).  The
predictive adds terms of its own to the link; its bounds are reasoned where it is probed.  Last, the one realistic shape: the
probit Hessian at |eta| up to 3e4 against the truth's weights, which the tail weight by subtraction missed by 5e-8 of max|H|
(the CPU test has both figures)."""
import math

import numpy as np
import pytest
import torch

import glm_link_truth as truth

pytestmark = pytest.mark.gpu

FORMS = {"ax": (1.0, 1.0, False), "half": (0.5, 2.0, False), "offset": (1.0, 0.0, True)}      # a, x / eta, eta as the offset


@pytest.fixture(scope="module")
def table():
    return truth.load_table()


@pytest.fixture(scope="module")
def grid(table):
    return {f: truth.rows(table, f) for f in truth.FAMILIES}


def _eng():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _layout(family, row, form):
    """(A (G, 1, 1), y (G, 1), offset (G, 1) or None, tau (G,), X (G, m, 1)): one problem per (y, tau) with the eta grid as the rows
    of X; one problem per row where the label depends on eta (gaussian) or eta is the offset"""
    a, xs, off = FORMS[form]
    n = len(row["eta"])
    G, m = (n, 1) if off or family == "gaussian" else (len(truth.LABELS[family]), n // len(truth.LABELS[family]))
    eta, y, tau = (row[k].reshape(G, m) for k in ("eta", "y", "tau"))
    assert (y == y[:, :1]).all() and (tau == tau[:, :1]).all()
    return (np.full((G, 1, 1), a), y[:, :1].copy(), eta[:, :1].copy() if off else None, tau[:, 0].copy(),
            (xs * eta)[:, :, None].copy())


def _hold(family, q, got, row, where, c=None, worst=None):
    """every element within c eps of its scale; returns (and records) the worst ratio"""
    c = truth.c_gpu(family, q) if c is None else c
    ratio = truth.ratio(got, row, q)
    i = int(np.argmax(ratio))
    assert ratio[i] <= c, (where, family, q, f"eta = {row['eta'][i]!r}, y = {row['y'][i]!r}, tau = {row['tau'][i]!r}: got {got[i]!r}, "
                           f"truth {row[q][i]!r}, {ratio[i]:.1f} eps of its scale, bound {c}")
    if worst is not None:
        worst[family, q] = max(worst.get((family, q), 0.0), float(ratio[i]))
    return float(ratio[i])


def _report(worst, what):
    for (family, q), v in sorted(worst.items()):
        print(f"{what}: {family} {q}: worst device ratio {v:.2f} eps of the scale (CPU restatement {truth.C_CPU[family, q]}, "
              f"bound {truth.c_gpu(family, q)})")


def _score_probe(call, family, row, forms, worst, what):
    """the probe of a score entry point: ``call(A, y, offset, tau, X, want)`` -> device tensors; want = g, lp and both agree bit
    for bit, r and t of every form are within the bound, and the forms agree with each other (eta is the same number in all)"""
    out = {}
    for form in forms:
        A, y, o, tau, X = _layout(family, row, form)
        G, lp = call(A, y, o, tau, X, "both")
        assert torch.equal(call(A, y, o, tau, X, "g"), G) and torch.equal(call(A, y, o, tau, X, "lp"), lp), (what, family, form)
        G, lp = G.cpu().numpy().reshape(-1), lp.cpu().numpy().reshape(-1)
        r = G / FORMS[form][0]
        _hold(family, "r", r, row, (what, form), worst=worst)
        _hold(family, "t", lp, row, (what, form), worst=worst)
        out[form] = (r, lp)
    first = out[forms[0]]
    for form in forms[1:]:
        assert np.array_equal(out[form][1], first[1]), (what, family, form, "t")
        big = np.abs(first[0]) >= 2.0 ** -1000                         # (r / 2 of a subnormal r drops a bit)
        assert np.array_equal(out[form][0][big], first[0][big]), (what, family, form, "r")
    return first


def _probit_mirror(r, t, what):
    """(eta, y) -> (-eta, 1 - y) at the labels 0 and 1 leaves every bit of the probit t and changes only the sign of r: lb_link
    forms both from |eta| and the mirror swaps the central and the tail branch.  (Not at eta = +-0, where -0 >= 0 takes the same
    branch as +0; not for the logistic family, whose r = y - sigma is 1 - 1 / (1 + e) on one side and e / (1 + e) on the other.)
    The rows are label-major, then the sign of eta, then the magnitude."""
    n = len(truth.etas())
    h = n // 2
    i0, i1 = truth.LABELS["probit"].index(0.0), truth.LABELS["probit"].index(1.0)
    nz = truth.magnitudes() != 0.0
    for q, v, sg in (("t", t, 1.0), ("r", r, -1.0)):
        a, b = v[i0 * n:(i0 + 1) * n], v[i1 * n:(i1 + 1) * n]
        assert np.array_equal(a[:h][nz], sg * b[h:][nz]) and np.array_equal(a[h:][nz], sg * b[:h][nz]), (what, q)


# ---- 1. the score entry points -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", truth.FAMILIES)
def test_glm_batched_is_the_link_element_by_element(grid, family):
    eng = _eng()
    worst = {}

    def call(A, y, o, tau, X, want):
        return eng.glm_batched(eng.asarray(X), eng.asarray(A), eng.asarray(y), family, offset=None if o is None else eng.asarray(o),
                               prior_prec=0.0, noise_prec=eng.batched_regs(tau) if family == "gaussian" else 1.0, want=want)

    r, t = _score_probe(call, family, grid[family], ("ax", "half", "offset"), worst, "glm_batched")
    if family == "logistic":                                            # the sibling entry point: the same bits
        def sibling(A, y, o, tau, X, want):
            return eng.logistic_batched(eng.asarray(X), eng.asarray(A), eng.asarray(y), prior_prec=0.0, want=want)

        r2, t2 = _score_probe(sibling, family, grid[family], ("ax", "half"), worst, "logistic_batched")
        assert np.array_equal(r2, r) and np.array_equal(t2, t)
    if family == "probit":
        _probit_mirror(r, t, "glm_batched")
    _report(worst, "glm_batched")


@pytest.mark.parametrize("family", truth.FAMILIES)
def test_glm_shared_batched_is_the_link_element_by_element(grid, family):
    """one shared row a; without weights and with every weight 1: the same bits"""
    eng = _eng()
    worst = {}

    def run(A, y, o, tau, X, want, weights):
        return eng.glm_shared_batched(eng.asarray(X), eng.asarray(A[0]), eng.asarray(y), family,
                                      offset=None if o is None else eng.asarray(o), weights=weights, prior_prec=0.0,
                                      noise_prec=eng.batched_regs(tau) if family == "gaussian" else 1.0, want=want)

    def call(A, y, o, tau, X, want):
        out = run(A, y, o, tau, X, want, None)
        ones = run(A, y, o, tau, X, want, eng.asarray(np.ones_like(y)))
        for a, b in zip(out if want == "both" else (out,), ones if want == "both" else (ones,)):
            assert torch.equal(a, b), (family, want)
        return out

    r, t = _score_probe(call, family, grid[family], ("ax", "half", "offset"), worst, "glm_shared_batched")
    if family == "probit":
        _probit_mirror(r, t, "glm_shared_batched")
    _report(worst, "glm_shared_batched")


# ---- 2. the Hessian entry point ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", truth.FAMILIES)
def test_glm_hessian_batched_is_the_weight_element_by_element(grid, family):
    """one problem per grid row: H[k, 0, 0] = a^2 w; the invariants of w; where w is a normal number also cov = 1 / w (through
    sqrt, a reciprocal and a square: three roundings on top of w's own, inside the same bound since c >= 16) and info = 0"""
    eng = _eng()
    row = grid[family]
    worst, ws = {}, {}
    for form in FORMS:
        a, xs, off = FORMS[form]
        eta = row["eta"]
        args = dict(offset=eng.asarray(eta[:, None].copy()) if off else None, prior_prec=0.0,
                    noise_prec=eng.batched_regs(row["tau"]) if family == "gaussian" else 1.0)
        A, y = eng.asarray(np.full((len(eta), 1, 1), a)), eng.asarray(row["y"][:, None].copy())
        X = eng.asarray((xs * eta)[:, None].copy())
        H = eng.glm_hessian_batched(X, A, y, family, want="h", **args)
        w = H.cpu().numpy().reshape(-1) / (a * a)
        _hold(family, "w", w, row, ("glm_hessian_batched", form), worst=worst)
        ws[form] = w
        assert (w >= 0.0).all(), (family, form)
        if family in ("logistic", "probit"):
            assert (w <= (0.25 if family == "logistic" else 1.0)).all(), (family, form)
        if form == "half":
            continue
        ok = np.abs(row["w"]) >= 2.0 ** -1022
        sel = torch.as_tensor(np.flatnonzero(ok), device=X.device)
        Hb, cov, info = eng.glm_hessian_batched(X[sel], A[sel], y[sel], family, want="both",
                                                **{k: (v[sel] if isinstance(v, torch.Tensor) else v) for k, v in args.items()})
        assert torch.equal(Hb, H[sel]) and (info == 0).all(), (family, form)
        cov = cov.cpu().numpy().reshape(-1)
        wt = row["w"][ok].astype(np.longdouble) + row["w_lo"][ok].astype(np.longdouble)
        rel = np.abs(cov.astype(np.longdouble) * wt - 1).astype(np.float64) / (truth.EPS * row["scale_w"][ok] / np.abs(row["w"][ok]))
        assert np.isfinite(cov).all() and rel.max() <= truth.c_gpu(family, "w"), (family, form, float(rel.max()))
    assert np.array_equal(ws["offset"], ws["ax"])
    big = ws["ax"] >= 2.0 ** -1000
    assert np.array_equal(ws["half"][big], ws["ax"][big])
    if family in ("logistic", "probit"):                                # (eta, y) -> (-eta, 1 - y) changes no bit of w
        n = len(truth.etas())
        for g in range(len(truth.LABELS[family])):
            yv = truth.LABELS[family][g]
            if 1.0 - (1.0 - yv) != yv:
                continue
            g2 = truth.LABELS[family].index(1.0 - yv)
            w1, w2 = ws["ax"][g * n:(g + 1) * n], ws["ax"][g2 * n:(g2 + 1) * n]
            assert np.array_equal(w1[:n // 2], w2[n // 2:]) and np.array_equal(w1[n // 2:], w2[:n // 2]), (family, yv)
    _report(worst, "glm_hessian_batched")


# ---- 3. the predictive ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nodes", [1, 32])
@pytest.mark.parametrize("family", truth.FAMILIES)
def test_glm_predict_batched_at_zero_covariance_is_the_link(table, grid, family, nodes):
    """mean = 1, cov = 0, the rows of A the eta grid: every node sees eta, so pmean is the family's mean at eta and lpd is t plus
    the normalisation.  The predictive adds terms of its own, so do its bounds (Q nodes):
      pmean  gaussian eta itself; poisson e^eta: w's bound; logistic sum_q exp(logw_q) sigma / sqrt(pi) with sigma = -r(eta, 0):
             r's bound plus (Q - 1) / 2 eps for the recursive sum of Q positive terms and 4 eps for exp(logw_q) and the division;
             probit Phi(eta) from erfc: 16 eps of |Phi| + |eta phi(eta)|
      lpd    (max_q f_q + log sum_q exp(f_q - max)) - log(pi) / 2 [- lgamma(y + 1)], f_q = logw_q + t: t's bound plus (Q - 1) / 2 + 4
             on t's scale plus the magnitudes of what is added: |logw| at the largest weight, log Q, log(pi) / 2 and lgamma(y + 1)
             (whose float64 value is the truth here: below one of the 16 eps); gaussian: t + log(tau / 2 pi) / 2, 16 eps of t's
             scale plus |log(2 pi / tau)| / 2"""
    eng = _eng()
    row = grid[family]
    m = len(table["poisson_eta"]) if family == "poisson" else len(truth.etas())
    G = len(row["eta"]) // m
    eta, y, tau = (row[k].reshape(G, m) for k in ("eta", "y", "tau"))
    assert (tau == tau[:, :1]).all() and (eta == eta[:1]).all()
    em, ev, pm, lpd, elpd = eng.glm_predict_batched(eng.asarray(np.ones((G, 1))), eng.asarray(np.zeros((G, 1, 1))),
                                                    eng.asarray(eta[:, :, None].copy()), family, y=eng.asarray(y.copy()),
                                                    noise_prec=eng.batched_regs(tau[:, 0].copy()) if family == "gaussian" else 1.0,
                                                    nodes=nodes)
    em, ev, pm, lpd = (t.cpu().numpy() for t in (em, ev, pm, lpd))
    assert np.array_equal(em, eta) and not ev.any()
    extra = (nodes - 1) / 2 + 4
    one = {k: v[:m] for k, v in row.items()}                           # the first label's rows
    if family == "gaussian":
        assert np.array_equal(pm, eta)
    elif family == "poisson":
        for g in range(G):
            _hold(family, "w", pm[g], one, ("pmean", nodes))
    elif family == "logistic":
        assert truth.LABELS[family][0] == 0.0                          # sigma(eta) = -r(eta, y = 0)
        for g in range(G):
            _hold(family, "r", -pm[g], one, ("pmean", nodes), c=truth.c_gpu(family, "r") + extra)
    else:
        assert truth.LABELS[family][1] == 1.0                          # phi / Phi(eta) = r(eta, y = 1)
        cdf = np.concatenate([table["probit_cdf"][0], table["probit_cdf"][1]])
        hp = np.abs(row["r"][m:2 * m])
        mean = {"eta": one["eta"], "y": one["y"], "tau": one["tau"], "w": cdf[:, 0], "w_lo": cdf[:, 1],
                "scale_w": cdf[:, 0] * (1.0 + np.abs(one["eta"]) * hp)}
        for g in range(G):
            _hold(family, "w", pm[g], mean, ("pmean", nodes), c=truth.C_FLOOR)
    gt, gl = eng.gauss_hermite(nodes)
    for g in range(G):
        sl = {k: v[g * m:(g + 1) * m] for k, v in row.items()}
        if family == "gaussian":
            const = 0.5 * math.log(tau[g, 0] / (2.0 * math.pi)) * np.ones(m)
            added, c = np.abs(const), truth.C_FLOOR
        else:
            const = -np.array([math.lgamma(v + 1.0) for v in sl["y"]]) if family == "poisson" else np.zeros(m)
            added = abs(gl[np.argmax(gl)]) + math.log(nodes) + 0.5 * math.log(math.pi) + np.abs(const)
            c = truth.c_gpu(family, "t") + extra
        want = dict(sl, scale_t=sl["scale_t"] + added)
        hi = sl["t"] + const
        want["t"], want["t_lo"] = hi, ((sl["t"] - hi) + const) + sl["t_lo"]                     # (two-sum: t + const exactly)
        _hold(family, "t", lpd[g], want, ("lpd", nodes), c=c)


# ---- 4. beyond the table ---------------------------------------------------------------------------------------------------------
def test_beyond_1e150_nothing_is_nan_and_r_keeps_its_sign(table):
    """|eta| = 1e160, 1e170, 1e300 as the offset (x = 0: |x|^2 stays finite): no NaN in r, t, w; r has the truth's sign (a zero
    where the truth underflows); an infinity only where the truth's float64 value is that infinity"""
    eng = _eng()
    for fi, family in enumerate(truth.FAMILIES):
        b = table["beyond"][table["beyond"][:, 0] == fi]
        K = len(b)
        A, y, o, X = (eng.asarray(v) for v in (np.ones((K, 1, 1)), b[:, 2:3].copy(), b[:, 1:2].copy(), np.zeros((K, 1, 1))))
        G, lp = eng.glm_batched(X, A, y, family, offset=o, prior_prec=0.0, want="both")
        Gs, lps = eng.glm_shared_batched(X, A[0], y, family, offset=o, prior_prec=0.0, want="both")
        assert torch.equal(Gs, G) and torch.equal(lps, lp), family
        H = eng.glm_hessian_batched(X[:, 0, :], A, y, family, offset=o, prior_prec=0.0, want="h")
        got = {"t": lp.cpu().numpy().reshape(-1), "r": G.cpu().numpy().reshape(-1), "w": H.cpu().numpy().reshape(-1)}
        for q, col in (("t", 3), ("r", 4), ("w", 5)):
            g, want = got[q], b[:, col]
            assert not np.isnan(g).any(), (family, q, b[np.isnan(g), 1:3])
            bad = ~(np.isfinite(g) | (g == want))
            assert not bad.any(), (family, q, b[bad, 1:3], g[bad], want[bad])
        sign = np.sign(got["r"])
        assert ((sign == b[:, 6]) | ((sign == 0.0) & (b[:, 4] == 0.0))).all(), (family, b[:, 1:3], got["r"], b[:, 4])
        assert (got["w"] >= 0.0).all() and (family not in ("logistic", "probit") or (got["w"] <= 1.0).all())


# ---- 5. one realistic shape ----------------------------------------------------------------------------------------------------------
def test_large_eta_probit_hessian_matches_the_truth(table):
    """probit, (K, N, D) = (5, 33, 16), make_inputs at scale 100 (seed 49): max|eta| = 3.2e4.  H against sum_n w_n a_n a_n^T + lam I
    with the truth's weights, accumulated in np.longdouble, at the single-launch bar of 1e-11 of max|H|.  With the tail weight
    formed by subtraction the float64 restatement of the same sum is at 4.8e-8 (tests/test_glm_link_truth_cpu.py computes it beside
    the present form's 1e-15), so this test fails on a kernel that subtracts"""
    import gsmvi_amd
    inp, eta, y, valid = truth.hessian_problem()
    A, y, o, counts, lam, tau, X = inp
    Ht = truth.hessian_truth(table)
    tgt = gsmvi_amd.BatchedGLMTarget(A, y, "probit", prior_precision=lam, counts=counts, offset=o)
    H = tgt.neg_hessian(X[:, 0, :]).cpu().numpy()
    worst = 0.0
    for k in range(A.shape[0]):
        e = float(np.abs(H[k] - Ht[k]).max() / np.abs(Ht[k]).max())
        worst = max(worst, e)
        assert np.array_equal(H[k], H[k].T) and e <= 1e-11, (k, e)
    print(f"large-eta probit Hessian: worst error {worst:.2e} of max|H| (max|eta| {np.abs(eta[valid]).max():.3g})")
