"""The element-wise truth of the multinomial logit link (tests/softmax_link_truth.py) on the CPU: the committed table regenerates
identically (which is also the proof that 60 and 120 digits agree on every entry), ``rows`` (the table combined in rational
arithmetic, what the GPU tests use) is the direct mpmath evaluation, the closed forms are mp.diff of the written density, the
four float64 restatements, fed the layouts of the GPU probes, are within their recorded c everywhere, and the plain form
log(s) misses the metric by fourteen orders at the reference-class-saturated points."""
import os

import mpmath as mp
import numpy as np
import pytest

import psis_loo_softmax_ref as loo_ref
import softmax_batched_ref as sref
import softmax_laplace_ref as lref
import softmax_link_truth as truth
import softmax_predict_ref as pred_ref


@pytest.fixture(scope="module")
def table():
    return truth.load_table()


def test_the_committed_table_regenerates_identically(table):
    """every array, bit for bit (the archive carries timestamps, so the arrays are compared, not the file)"""
    assert os.path.getsize(truth.GOLDEN) < 200 * 1000
    new = truth.build_table()
    assert sorted(new) == sorted(table)
    for k, v in new.items():
        assert v.dtype == table[k].dtype and v.shape == table[k].shape and v.tobytes() == table[k].tobytes(), k


def test_the_points_are_the_ones_the_issue_lists():
    assert truth.SHAPES == ((2, 1), (3, 1), (3, 3), (9, 3), (17, 1), (65, 1)) and len(truth.MAGNITUDES) == 21
    for C in (2, 3, 9, 17, 65):
        v = truth.vectors(C)
        assert v.shape[1] == C - 1 and len({r.tobytes() for r in v}) == len(v)
        has = lambda r: any(np.array_equal(r, x) for x in v)           # noqa: E731
        for h in (truth.DOZEN if C == 65 else truth.MAGNITUDES):
            assert has(np.full(C - 1, -h)) and has(np.full(C - 1, h))
            first, last = np.zeros(C - 1), np.zeros(C - 1)
            first[0], last[-1] = -h, h
            assert has(first) and has(last)
            for d in truth.DELTAS:
                r = np.full(C - 1, h - d)
                r[(C - 1) // 2] = h
                assert has(r)
    assert len(truth.vectors(65)) <= 12 * 9 and len(truth.vectors(17)) >= 100 + 150
    A, y, counts, X, eta = truth.real_problem()
    valid = (np.arange(A.shape[1])[None, :] < counts[:, None]).reshape(-1)
    assert (eta[valid] <= truth.REAL_TOP).all() and (y == truth.REAL_SHAPE[2] - 1).all() and counts.min() >= 1


def _mp_scales(free, v):
    """t (C), r (C, C - 1), w (C - 1, C - 1), p and their scales from the mpmath values, by the definitions"""
    C = len(free) + 1
    h = [mp.mpf(float(x)) for x in free] + [mp.mpf(0)]
    p, q, lse = v["p"], v["q"], v["lse"]
    dev = lambda c, j: q[c] if c == j else p[j]                        # noqa: E731  |delta_cj - p_j|
    D = [mp.fsum(abs(h[j]) * dev(c, j) for j in range(C)) for c in range(C)]
    t = [h[y] - lse for y in range(C)]
    st = [abs(t[y]) + D[y] + abs(h[y]) + abs(lse) for y in range(C)]
    r = [[q[c] if y == c else -p[c] for c in range(C - 1)] for y in range(C)]
    sr = [[abs(r[y][c]) + p[c] * D[c] + (1 if y == c else 0) + p[c] for c in range(C - 1)] for y in range(C)]
    sp = [p[c] + p[c] * D[c] for c in range(C)]
    w = [[p[c] * q[c] if c == d else -p[c] * p[d] for d in range(C - 1)] for c in range(C - 1)]
    sw = [[p[c] * q[c] + p[c] * abs(q[c] - p[c]) * D[c] if c == d else
           p[c] * p[d] * (1 + mp.fsum(abs(h[j]) * (abs(q[j] - p[j]) if j in (c, d) else 2 * p[j]) for j in range(C)))
           for d in range(C - 1)] for c in range(C - 1)]
    return t, st, r, sr, sp, w, sw


@pytest.mark.parametrize("name", ["2", "3", "9", "17", "65", "b2", "b3", "real"])
def test_rows_are_the_direct_evaluation(table, name):
    """a sample of every set: value + remainder against ``values`` to 2^-100 of the scale, the scales to 1e-9"""
    row = truth.rows(table, name, w=True)
    free = table["eta_" + name]
    step = {"65": 13, "17": 9, "9": 7}.get(name, 5)
    close = lambda a, b: abs(mp.mpf(float(a)) - b) <= mp.mpf(10) ** -9 * b + mp.mpf(2) ** -1060       # noqa: E731
    with mp.workdps(400):
        for i in list(range(0, len(free), step)) + [len(free) - 1]:
            v = truth.values(free[i])
            t, st, r, sr, sp, w, sw = _mp_scales(free[i], v)
            C = len(free[i]) + 1
            tiny = mp.mpf(2) ** -1074
            for y in range(C):
                got = mp.mpf(float(row["t"][i, y])) + mp.mpf(float(row["t_lo"][i, y]))
                assert abs(got - t[y]) <= mp.mpf(2) ** -100 * st[y] + tiny and close(row["scale_t"][i, y], st[y]), (name, i, y)
                assert close(row["scale_p"][i, y], sp[y]), (name, i, y)
                for c in range(C - 1):
                    got = mp.mpf(float(row["r"][i, y, c])) + mp.mpf(float(row["r_lo"][i, y, c]))
                    assert abs(got - r[y][c]) <= mp.mpf(2) ** -100 * sr[y][c] + tiny, (name, i, y, c)
                    assert close(row["scale_r"][i, y, c], sr[y][c]), (name, i, y, c)
            for c in range(C - 1):
                for d in range(C - 1):
                    got = mp.mpf(float(row["w"][i, c, d])) + mp.mpf(float(row["w_lo"][i, c, d]))
                    assert abs(got - w[c][d]) <= mp.mpf(2) ** -100 * sw[c][d] + tiny, (name, i, c, d)
                    assert close(row["scale_w"][i, c, d], sw[c][d]), (name, i, c, d, row["scale_w"][i, c, d], sw[c][d])


def test_closed_forms_are_the_derivatives_of_the_written_density():
    """C = 3 at moderate points: ``written`` (the literal formula) equals t, its gradient is r and its second derivatives -w"""
    with mp.workdps(60):
        for free in ((-6.0, 2.5), (0.0, 0.0), (0.7, -0.5), (3.0, 6.5), (-2.5, -4.0)):
            v = truth.values(np.array(free))
            t, _, r, _, _, w, _ = _mp_scales(free, v)
            at = [mp.mpf(x) for x in free]
            for y in range(3):
                f = lambda a, b: truth.written([a, b], y)              # noqa: E731
                assert abs(f(*at) - t[y]) <= mp.mpf(10) ** -40
                for c, order in enumerate(((1, 0), (0, 1))):
                    assert abs(mp.diff(f, at, order) - r[y][c]) <= mp.mpf(10) ** -25, (free, y, c)
                for (c, d), order in (((0, 0), (2, 0)), ((0, 1), (1, 1)), ((1, 1), (0, 2))):
                    assert abs(mp.diff(f, at, order) + w[c][d]) <= mp.mpf(10) ** -25, (free, y, c, d)


def restated(free, P, alpha=1.0):
    """what the four float64 restatements return at the layouts of the GPU probes: (probe, quantity) -> values shaped like the
    arrays of ``rows``"""
    V, Cm = free.shape
    C = Cm + 1
    out = {}
    A, y, X = truth.layout_score(free, P, alpha)
    G, lp = sref.score_and_lp(A, y, C, None, 0.0, X)
    out["score", "t"] = lp.T
    out["score", "r"] = np.swapaxes(G.reshape(C, V, Cm, P)[..., 0], 0, 1) / alpha
    A, y, X = truth.layout_point(free, P, alpha)
    H = lref.neg_hessian(A, y, C, None, 0.0, X)
    out["hessian", "w"] = H.reshape(V, Cm, P, Cm, P)[:, :, 0, :, 0] / (alpha * alpha)
    t, r = np.empty((V, C)), np.empty((V, C, Cm))
    hot = np.eye(C, dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(V):                                              # the lines of softmax_laplace_ref.evaluate, per label
            eta, m, rest, pr, q = lref.probabilities(A[i], X[i], C)
            t[i] = eta[0] - m - sref.log_s(rest, 1 + rest)
            r[i] = np.where(hot, q, -pr)[:, :Cm]
    out["laplace", "t"], out["laplace", "r"] = t, r
    A, y, X = truth.layout_rows(free, P, alpha, False)
    out["loo", "t"] = np.asarray(loo_ref.loglik_softmax(A, y, C, None, X, np.float64))[0, :, :V].T
    A, y, X = truth.layout_rows(free, P, alpha, True)
    prob, lpd = pred_ref.predict(A, y, C, None, X, None, np.float64)
    assert all(np.array_equal(prob[:, 0], prob[:, i]) for i in range(C))
    out["predict", "p"], out["predict", "t"] = prob[:, 0], lpd
    return out


def worst_ratios(table):
    worst = {}
    for C, P in truth.SHAPES:
        row = truth.rows(table, str(C), w=True)
        got = restated(table["eta_" + str(C)], P)
        label = np.eye(C, dtype=bool)[None, :, :C - 1]
        for (probe, q), v in got.items():
            ratio = truth.ratio(v, row, q)
            worst[probe, q] = max(worst.get((probe, q), 0.0), float(ratio.max()))
            if (probe, q) == ("laplace", "r"):                          # at the label's class: q_y with a_r = 0
                rq = np.where(label, truth.ratio(v, row, "r", row["scale_rq"]), 0.0)
                worst[probe, "rq"] = max(worst.get((probe, "rq"), 0.0), float(rq.max()))
    return worst


def test_the_restatements_are_within_their_recorded_c_everywhere(table):
    """the worst ratio of the float64 restatements per probe and quantity over every table point of every shape: printed, at most
    truth.C_CPU (what the GPU bound max(16, 4 C_CPU) is made from)"""
    worst = worst_ratios(table)
    assert sorted(worst) == sorted(truth.C_CPU)
    for key, v in sorted(worst.items()):
        print(f"{key[0]} {key[1]}: worst ratio {v:.2f}; recorded {truth.C_CPU[key]}, GPU bound {truth.c_gpu(*key)} eps")
        assert v <= truth.C_CPU[key], key
    # the layouts are exact at alpha = 1 / 2 too: the same eta, so the restated t does not change by a bit
    free = table["eta_3"]
    a, b = restated(free, 3, 1.0), restated(free, 3, 0.5)
    assert np.array_equal(a["score", "t"], b["score", "t"]) and np.array_equal(a["loo", "t"], b["loo", "t"])


def test_the_laplace_probe_is_evaluate_itself(table):
    """``restated`` copies two lines of softmax_laplace_ref.evaluate (which would form a D x D Hessian per label); at C = 3 they
    are held to it bit for bit"""
    free = table["eta_3"][::3]
    A, y, X = truth.layout_step(free, 3, 1.0)
    got = restated(free, 3)
    for k in range(len(y)):
        with np.errstate(all="ignore"):
            f, g, _, _ = lref.evaluate(lref.problem(A, y, 3, None, 0.0, k), X[k])
        assert f == -got["laplace", "t"][k // 3, k % 3] or (f == 0.0 and got["laplace", "t"][k // 3, k % 3] == 0.0)
        assert np.array_equal(-g.reshape(2, 3)[:, 0], got["laplace", "r"][k // 3, k % 3])


def test_the_plain_form_misses_where_the_reference_class_saturates(table):
    """C = 3, eta = (-1e150, -37.5), y = 2: z = 1 + e^-37.5 rounds to 1 and log(z) returns 0, where t = -log1p(e^-37.5) =
    -5.18e-17: 1.1e14 units of the metric.  log1p(rest) is within one unit.  And the realistic shape, every valid eta <= -37.5 and
    every label the reference class: the plain form's lp is exactly 0, the restatement's within 1e-13 of |lp|"""
    row = truth.rows({k + "_x": v for k, v in zip(("eta", "lse", "p", "q"), _one_point((-1e150, -37.5)))}, "x")
    rest = np.exp(-37.5) + np.exp(-1e150)
    plain, fixed = 0.0 - 0.0 - np.log(1.0 + rest), 0.0 - 0.0 - sref.log_s(rest, 1.0 + rest)
    assert plain == 0.0 and abs(row["t"][0, 2] + 5.18e-17) < 1e-19
    old, new = truth.ratio(plain, row, "t")[0, 2], truth.ratio(fixed, row, "t")[0, 2]
    print(f"eta = (-1e150, -37.5), y = 2: log(s) is {old:.3g} units from the truth, log1p(rest) {new:.2f}")
    assert 1.0e14 < old < 1.2e14 and new <= 1.0
    A, y, counts, X, eta = truth.real_problem()
    K, N, C, P = truth.REAL_SHAPE
    real = truth.rows(table, "real")
    valid = np.arange(N)[None, :] < counts[:, None]
    L = np.longdouble
    want = ((real["t"][:, C - 1].astype(L) + real["t_lo"][:, C - 1].astype(L)).reshape(K, N) * valid).sum(axis=1)
    z = 1.0 + np.exp(eta).sum(axis=1).reshape(K, N)
    assert (np.log(z)[valid] == 0.0).all()                              # the plain form: lp = 0 exactly
    _, lp = sref.score_and_lp(A, y, C, counts, 0.0, X)
    err = np.abs(lp[:, 0].astype(L) - want) / np.abs(want)
    print(f"realistic shape: |lp| from {float(np.abs(want).min()):.3g}, the restatement's error {float(err.max()):.2e} of |lp|")
    assert (want < 0).all() and err.max() <= 1e-13


def _one_point(free):
    v = truth.values(np.array(free))
    return (np.array([free]), np.array([truth.split(v["lse"])]), np.array([[truth.split(x) for x in v["p"]]]),
            np.array([[truth.split(x) for x in v["q"]]]))
