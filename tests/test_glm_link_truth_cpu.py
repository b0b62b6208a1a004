"""The element-wise truth of the GLM links (tests/glm_link_truth.py) on the CPU: the committed table regenerates identically, the
two precisions agree on every grid row, ``rows`` (the table combined in rational arithmetic, what the GPU tests use) is the
direct mpmath evaluation, the closed-form derivatives are mp.diff of the written densities, the float64 restatements
(glm_batched_ref.link, laplace_batched_ref.weights) are within their recorded c everywhere, and the large-eta Hessian of the
restatement, with the probit tail weight as it was (by subtraction) and as it is (continued fraction)."""
import os

import mpmath as mp
import numpy as np
import pytest
from scipy.special import erfcx

import glm_batched_ref as gref
import glm_link_truth as truth
import laplace_batched_ref as lref


@pytest.fixture(scope="module")
def table():
    return truth.load_table()


@pytest.fixture(scope="module")
def grid(table):
    return {f: truth.rows(table, f) for f in truth.FAMILIES}


def restated(family, row):
    """t, r, w of the float64 restatements at the rows"""
    with np.errstate(all="ignore"):
        r, t, flag = gref.link(family, row["eta"], row["y"], row["tau"])
        w, flag2 = lref.weights(family, row["eta"], row["y"], row["tau"])
    assert not flag.any() and not flag2.any()
    return {"t": t, "r": r, "w": w}


def weights_by_subtraction(eta, y):
    """the probit weight as it was before the continued fraction: hm - eta on the tail side at every eta"""
    s = np.abs(eta)
    u, e = erfcx(s * 0.70710678118654752440), np.exp(-0.5 * (s * s))
    q = 0.5 * (u * e)
    rt, rc = 0.79788456080286535588 / u, e * 0.39894228040143267794 / (1.0 - q)
    hp, hm = np.where(eta >= 0.0, rc, rt), np.where(eta >= 0.0, rt, rc)
    return y * (hp * (hp + eta)) + (1.0 - y) * (hm * (hm - eta))


def test_the_committed_table_regenerates_identically(table):
    """every array, bit for bit (a zip archive carries a timestamp, so the arrays are compared, not the file); under 100 KB;
    building it is also the proof that 60 and 120 digits agree on every table entry (``values`` raises otherwise)"""
    assert os.path.getsize(truth.GOLDEN) < 100 * 1000
    new = truth.build_table()
    assert sorted(new) == sorted(table)
    for k, v in new.items():
        assert v.dtype == table[k].dtype and v.shape == table[k].shape and v.tobytes() == table[k].tobytes(), k
    assert table["switch"][0] == lref.PROBIT_S0 == truth.SWITCH
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "gsm-vi_amd", "csrc", "gsmvi_glm_link.h")) as f:
        src = f.read()
    assert f"#define LB_PROBIT_S0 {truth.SWITCH}" in src and f"#define LB_PROBIT_CF {lref.PROBIT_CF}" in src


def test_the_grid_is_the_one_the_issue_lists(grid):
    m = truth.magnitudes()
    assert len(m) == 230 and m[0] == 0.0 and m[1] == 5e-324 and (m[30:] >= 1e-3).all() and (m[30:] <= 1e8).all()
    s = truth.SWITCH
    for v in (np.nextafter(s, 0.0), s, np.nextafter(s, np.inf), 709.78, 745.0, 1e150):
        assert v in m
    e = truth.etas()
    assert len(e) == 460 and np.signbit(e[230]) and e[230] == 0.0
    assert len(grid["logistic"]["eta"]) == len(grid["probit"]["eta"]) == 3 * 460
    assert len(grid["poisson"]["eta"]) == 4 * int((e <= truth.POISSON_MAX).sum()) and grid["poisson"]["eta"].max() == 709.78
    assert len(grid["gaussian"]["eta"]) == 3 * 4 * 460 and set(grid["gaussian"]["tau"]) == set(truth.TAUS)


@pytest.mark.parametrize("family", truth.FAMILIES)
def test_rows_are_the_direct_evaluation_at_two_agreeing_precisions(grid, family):
    """every grid row (every third gaussian one): value + remainder against ``values`` (which raises unless 60 and 120 digits
    agree to 1e-40) to 2^-100 of the scale, and the scales to 1e-12 (and 2^-1060: a subnormal w' has few bits)"""
    row = grid[family]
    step = 3 if family == "gaussian" else 1
    with mp.workdps(150):
        for i in range(0, len(row["eta"]), step):
            eta, y, tau = row["eta"][i], row["y"][i], row["tau"][i]
            v = truth.values(family, eta, y, tau)
            sc = truth.scales(v, mp.mpf(float(eta)), v["a_t"], v["a_r"])
            for q, s in zip("trw", sc):
                got = mp.mpf(float(row[q][i])) + mp.mpf(float(row[q + "_lo"][i]))
                assert abs(got - v[q]) <= mp.mpf(2) ** -100 * s + mp.mpf(2) ** -1074, (family, q, eta, y, tau)
                if mp.isfinite(mp.mpf(float(row["scale_" + q][i]))):
                    assert abs(mp.mpf(float(row["scale_" + q][i])) - s) <= mp.mpf(10) ** -12 * s + mp.mpf(2) ** -1060, (family, q, eta, y, tau)


def test_closed_forms_are_the_derivatives_of_the_written_densities():
    """at moderate points: ``written`` (the literal formula) equals t, and mp.diff of it gives r, -w and -w'"""
    with mp.workdps(60):
        for family in truth.FAMILIES:
            ys = (0.0, 1.0, 0.3) if family in ("logistic", "probit") else (0.0, 7.0) if family == "poisson" else (0.4, -2.0)
            for eta in (-6.0, -2.5, -0.5, 0.0, 0.7, 3.0, 6.5):
                for y in ys:
                    v = truth.values(family, eta, y, 1.7 if family == "gaussian" else 1.0)
                    f = lambda h: truth.written(family, h, y, 1.7)                   # noqa: E731
                    want = (v["t"], v["r"], -v["w"], -v["dw"])
                    for n, b in enumerate(want):
                        a = mp.diff(f, mp.mpf(eta), n) if n else f(mp.mpf(eta))
                        assert abs(a - b) <= mp.mpf(10) ** -25 * (abs(b) + 1), (family, eta, y, n, a, b)


def test_the_restatements_are_within_their_recorded_c_everywhere(grid):
    """the worst ratio of the float64 restatements per family and quantity: printed, at most truth.C_CPU (what the GPU bound
    max(16, 4 C_CPU) is made from)"""
    for family in truth.FAMILIES:
        got = restated(family, grid[family])
        for q in "trw":
            ratio = truth.ratio(got[q], grid[family], q)
            i = int(np.argmax(ratio))
            print(f"{family} {q}: worst ratio {ratio[i]:.2f} at eta = {grid[family]['eta'][i]!r}, y = {grid[family]['y'][i]!r}; "
                  f"recorded {truth.C_CPU[family, q]}, GPU bound {truth.c_gpu(family, q)} eps")
            assert ratio[i] <= truth.C_CPU[family, q], (family, q)


def test_invariants_of_the_restated_weight(grid):
    """w >= 0, probit w <= 1, logistic w <= 1 / 4.  (eta, y) -> (-eta, 1 - y), for the labels with 1 - (1 - y) == y, changes no bit
    of w (both families form it from |eta|), nor of the probit t, and only the sign of the probit r; the logistic r = y - sigma and
    t = y eta - softplus are NOT mirror images bit for bit (1 - 1 / (1 + e) against e / (1 + e)): the accepted cancellation of
    DESIGN.md section 9, held to the metric instead"""
    for family in ("logistic", "probit"):
        row = grid[family]
        got = restated(family, row)
        assert (got["w"] >= 0.0).all() and (got["w"] <= (0.25 if family == "logistic" else 1.0)).all()
        m = 1.0 - (1.0 - row["y"]) == row["y"]
        assert m.sum() == 2 * 460
        mir = restated(family, {"eta": -row["eta"], "y": 1.0 - row["y"], "tau": row["tau"]})
        assert np.array_equal(got["w"][m], mir["w"][m])
        if family == "probit":
            assert np.array_equal(got["t"][m], mir["t"][m]) and np.array_equal(got["r"][m], -mir["r"][m])
    for family in ("poisson", "gaussian"):
        assert (restated(family, grid[family])["w"] >= 0.0).all()


def test_beyond_the_table_the_restatement_stays_finite_and_signed(table):
    """|eta| = 1e160, 1e170, 1e300: no NaN, r has the truth's sign (or is a zero where the truth underflows), an infinity only
    where the truth overflows float64"""
    for fi, eta, y, t, r, w, sign in table["beyond"]:
        family = truth.FAMILIES[int(fi)]
        got = restated(family, {"eta": np.array([eta]), "y": np.array([y]), "tau": np.array([1.0])})
        for q, want in (("t", t), ("r", r), ("w", w)):
            g = got[q][0]
            assert not np.isnan(g) and (np.isfinite(g) or g == want), (family, eta, y, q, g, want)
        assert np.sign(got["r"][0]) in (sign, 0.0 if r == 0.0 else sign), (family, eta, y)


def test_large_eta_hessian_of_the_restatement_before_and_after(table):
    """probit, (K, N, D) = (5, 33, 16), max|eta| = 3.2e4: H of the restatement against sum_n w_n a_n a_n^T + lam I with the
    truth's weights in np.longdouble.  With the tail weight by subtraction (as it was) the error is far above the single-launch
    bar of 1e-11 of max|H|; with the continued fraction it is within it"""
    inp, eta, y, valid = truth.hessian_problem()
    assert 1e4 <= np.abs(eta[valid]).max() <= 1e5
    H = truth.hessian_truth(table)
    A, lam = inp[0], inp[4]

    def err(w):
        Hw = np.einsum("kn,kni,knj->kij", w * valid, A, A) + lam[:, None, None] * np.eye(A.shape[2])
        return max(float(np.abs(Hw[k] - H[k]).max() / np.abs(H[k]).max()) for k in range(A.shape[0]))

    old, new = err(weights_by_subtraction(eta, y)), err(lref.weights("probit", eta, y)[0])
    X = inp[6][:, 0, :]
    ref = max(float(np.abs(h - t).max() / np.abs(t).max()) for h, t in zip(lref.neg_hessian("probit", *inp[:6], X), H))
    print(f"large-eta probit Hessian, error of max|H|: by subtraction {old:.2e}, continued fraction {new:.2e}, "
          f"neg_hessian of the restatement {ref:.2e}")
    assert old > 1e-10 and new <= 1e-11 and ref <= 1e-11
