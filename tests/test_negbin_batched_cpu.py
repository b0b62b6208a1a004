"""The batched negative binomial target without a GPU: the float64 restatement of the link (tests/negbin_batched_ref.py) against
the mpmath truth over the whole grid (tests/negbin_link_truth.py), the golden table against fresh mpmath, the closed-form
derivatives against mp.diff of the written density, the Poisson limit, the restatements against each other; the C ABI declaration
and argument checks of gsmvi_negbin_batched_f64, its LDS budget; and the host logic of BatchedNegBinomialTarget on a stand-in
engine, inside the fits, the initialisers and psis_batched on theirs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import negbin_batched_ref as ref
import negbin_link_truth as truth
from gsmvi_amd import _lib
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsmvi_negbin_batched_f64"
DEBUG = "gsmvi_debug_negbin_batched_lds"
GB_LDS_MAX = 160 * 1024                          # csrc/gsmvi_batched.h


def _mp():
    return pytest.importorskip("mpmath")


# ---- 1. the link, element by element -------------------------------------------------------------------------------------------
def test_float64_restatement_meets_the_truth_over_the_whole_grid():
    """worst err / (eps scale) per quantity over the grid, asserted against the recorded C_CPU (measured 1.70 / 0.59 / 1.45 for
    t / r_eta / r_theta); and the naive difference of two library calls is far outside: the metric bites"""
    tab = truth.load_table()
    eta, theta, y = truth.grid()
    assert np.array_equal(tab["thetas"], truth.thetas()) and tab["t"].shape == (2, eta.size)
    r = np.exp(theta)
    assert (r < ref.SHIFT_BELOW).any() and (r >= ref.SHIFT_BELOW).any()
    near = np.abs(theta - truth.LOG10) < 1e-12                            # both sides of the threshold, a hair from it
    assert (r[near] < ref.SHIFT_BELOW).any() and (r[near] >= ref.SHIFT_BELOW).any()
    re, rt, t = ref.link(eta, theta, y)
    for q, got in (("t", t), ("re", re), ("rt", rt)):
        worst = truth.ratio(got, tab, q)
        i = int(np.argmax(worst))
        print(f"negbin {q}: worst ratio {worst[i]:.3f} at eta = {eta[i]!r}, theta = {theta[i]!r}, y = {y[i]!r} (C_CPU {truth.C_CPU[q]})")
        assert worst[i] <= truth.C_CPU[q], (q, worst[i])
    from scipy.special import digamma, expit, gammaln
    with np.errstate(all="ignore"):
        d = eta - theta
        sp, sn = np.logaddexp(0.0, d), np.logaddexp(0.0, -d)
        t_naive = gammaln(y + r) - gammaln(r) - r * sp - y * sn
        re_naive = y * expit(-d) - r * expit(d)
        rt_naive = r * (digamma(y + r) - digamma(r) - sp) - re_naive
    nt, nrt = truth.ratio(t_naive, tab, "t").max(), truth.ratio(rt_naive, tab, "rt").max()
    print(f"naive scipy differences: t {nt:.3g}, r_theta {nrt:.3g} eps of the scale")
    # (r_theta 2.9e13; t 7.9e5: the two gammaln errors are correlated, and t's scale carries r softplus(d))
    assert max(nt, nrt) > 1e6 and nt > 1e4 * truth.C_CPU["t"] and nrt > 1e6


def test_golden_table_is_fresh_mpmath():
    """a seeded sample of the grid and every point beyond it, recomputed"""
    _mp()
    tab = truth.load_table()
    eta, theta, y = truth.grid()
    pick = np.random.RandomState(3).choice(eta.size, 60, replace=False)
    for i in pick:
        v = truth.values(eta[i], theta[i], y[i])
        for q in truth.QUANTITIES:
            hi, lo = truth.split(v[q])
            assert hi == tab[q][0, i] and lo == tab[q][1, i], (q, i)
            s = float(v["scale_" + q])
            assert 0.0 <= s - float(tab["scale_" + q][i]) <= 2e-7 * s, (q, i)
    for row in tab["beyond"][::5]:
        v = dict(zip(truth.NAMES, truth._at(row[0], row[1], row[2], 400)))
        assert [truth.split(v[q])[0] for q in truth.QUANTITIES] == row[3:].tolist()


def test_closed_form_derivatives_are_mp_diff_of_the_written_density():
    mp = _mp()
    for eta, theta, y in ((0.3, 1.0, 2.0), (-2.0, 0.5, 0.3), (3.0, 4.0, 7.0), (1.5, -1.0, 0.0), (2.0, 2.5, 1e3)):
        v = truth.values(eta, theta, y)
        with mp.workdps(60):
            f = lambda a, b: truth.written(a, b, y)                       # noqa: E731
            t0 = f(mp.mpf(eta), mp.mpf(theta))
            de = mp.diff(f, (mp.mpf(eta), mp.mpf(theta)), (1, 0))
            dt = mp.diff(f, (mp.mpf(eta), mp.mpf(theta)), (0, 1))
            tol = mp.mpf(10) ** -25 * v["scale_t"]
            assert abs(t0 - v["t"]) <= tol and abs(de - v["re"]) <= tol and abs(dt - v["rt"]) <= tol, (eta, theta, y)


def test_poisson_limit_at_theta_30():
    """r -> inf: |t - (y eta - e^eta)| <= (y + mu)^2 / (2 r) and |r_eta - (y - mu)| <= |y - mu| mu / r, each plus the metric's
    rounding C_CPU eps scale, with the scale of the truth table's formula evaluated here in float64"""
    theta = 30.0
    r = np.exp(theta)
    eta, y = np.meshgrid(np.array([-3.0, 0.0, 1.0, 4.0, 8.0]), np.array([0.0, 1.0, 7.0, 250.0]), indexing="ij")
    re, rt, t = ref.link(eta, theta, y)
    mu = np.exp(eta)
    d = eta - theta
    spd, spn = np.logaddexp(0.0, d), np.logaddexp(0.0, -d)
    dlg = np.abs(t + r * spd + y * spn)
    scale_t = np.abs(t) + np.abs(eta * re) + np.abs(theta * rt) + dlg + r * spd + y * spn
    sg, sn = 1.0 / (1.0 + np.exp(-d)), 1.0 / (1.0 + np.exp(d))
    s = (y + r) * sg * sn
    scale_re = np.abs(re) + np.abs(eta) * s + theta * np.abs(s - r * sg) + y * sn + r * sg
    assert (np.abs(t - (y * eta - mu)) <= (y + mu) ** 2 / (2.0 * r) + 1.01 * truth.C_CPU["t"] * truth.EPS * scale_t).all()
    assert (np.abs(re - (y - mu)) <= np.abs(y - mu) * mu / r + 1.01 * truth.C_CPU["re"] * truth.EPS * scale_re).all()


# ---- 2. the restatements ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,P,rows", [(3, 1, 1, 1), (5, 33, 16, 3), (3, 70, 63, 5)])
def test_float64_and_longdouble_restatements_agree_and_follow_the_rules(K, N, P, rows):
    A, y, o, counts, lam, tm, tk, X = ref.make_inputs(K, N, P, rows)
    G, lp = ref.score_and_lp(A, y, o, counts, lam, tm, tk, X)
    Gl, lpl = ref.score_and_lp_ld(A, y, o, counts, lam, tm, tk, X)
    assert np.isfinite(G).all() and np.isfinite(lp).all() and G.shape == (K, rows, P + 1)
    for k in range(K):
        assert rel_err(G[k], Gl[k].astype(np.float64)) <= 1e-12 and rel_err(lp[k], lpl[k].astype(np.float64)) <= 1e-12, k
    if K > 1:                                                             # counts = 0: the two priors, exactly
        beta, th = X[1, :, :P], X[1, :, P]
        assert counts[1] == 0
        assert np.array_equal(G[1, :, :P], 0.0 - lam[1] * beta) and np.array_equal(G[1, :, P], 0.0 - tk[1] * (th - tm[1]))
    # a central difference of lp is the score (both components)
    k, h = 0, 1e-6
    for j in (0, P):
        Xp, Xm = X.copy(), X.copy()
        Xp[k, :, j] += h
        Xm[k, :, j] -= h
        fd = (ref.score_and_lp(A, y, o, counts, lam, tm, tk, Xp)[1][k] - ref.score_and_lp(A, y, o, counts, lam, tm, tk, Xm)[1][k]) / (2 * h)
        assert np.abs(fd - G[k, :, j]).max() <= 1e-5 * max(1.0, np.abs(G[k, :, j]).max()), j
    # the row flags: a non-finite entry, and theta = +-800
    X2 = np.repeat(X[:, :1], 4, axis=1).copy()
    X2[0, 1, 0], X2[0, 2, P], X2[0, 3, P] = np.inf, 800.0, -800.0
    G2, lp2 = ref.score_and_lp(A, y, o, counts, lam, tm, tk, X2)
    assert np.isnan(G2[0, 1:]).all() and np.isnan(lp2[0, 1:]).all() and np.isfinite(G2[0, 0]).all() and np.isfinite(G2[1:]).all()


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr)
    for mp in ("exports.map", "exports_debug.map"):
        assert re.search(r"^\s*" + NAME + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), mp
    assert NAME in _lib.exported_symbols() and NAME in built
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.GLM_FAMILIES == {"logistic": 0, "poisson": 1, "probit": 2, "gaussian": 3}     # no fifth family: its own entry
    block = hdr[:hdr.index("int " + NAME)].rsplit("/*", 1)[1]
    assert "example_gsm.py:34-35" in block and "GSMVI_PATH_BATCHED_TARGET" in block
    res, args = _lib._SIGS[NAME]
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert res is C.c_int and len(args) == len(params) == 19
    for p, a in zip(params, args):
        want = C.c_double if p.startswith("double ") else C.c_int64 if p.startswith("int64_t") else \
            C.c_int if p.startswith("int ") else C.c_void_p
        assert a is want, (p, a)
    assert params[3] == "int P" and params[10] == "double theta_mean" and params[13] == "const double* theta_prec_dev"
    dhdr = open(os.path.join(ROOT, "include", "gsmvi_hip_debug.h")).read()
    assert re.search(r"\bint\s+" + DEBUG + r"\s*\(", dhdr) and DEBUG not in hdr
    assert DEBUG in open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "exports_debug.map")).read()
    assert DEBUG not in open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "exports.map")).read()
    dbg = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path(debug=True)], check=True, capture_output=True,
                         text=True).stdout
    assert DEBUG in dbg and NAME in dbg and DEBUG not in out
    assert DEBUG in _lib._DEBUG_SIGS and DEBUG not in _lib._SIGS


def test_no_path_bit_is_added():
    """all 32 bits are taken: the launch reports the batched target's, 0x20000"""
    from gsmvi_amd.engine import HipEngine
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    bits = dict(re.findall(r"#define\s+(GSMVI_PATH_\w+)\s+(0x[0-9a-fA-F]+)u", hdr))
    assert len(bits) == 32 and int(bits["GSMVI_PATH_BATCHED_TARGET"], 16) == 0x20000
    assert len(HipEngine.PATH_BITS) == 32
    src = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_negbin_batched.hip")).read()
    assert re.findall(r"GSMVI_PATH_\w+", src) == ["GSMVI_PATH_BATCHED_TARGET"]


def test_abi_checks_arguments_before_the_context_and_names_overlapping_arrays():
    """every bad argument is reported with a NULL context (no device work can have started); valid ones end at the context"""
    lib = _lib.load_library()
    buf = (C.c_double * 8192)()
    p = C.cast(buf, C.c_void_p).value
    a = lambda n: p + 8 * 512 * n                                   # noqa: E731  sixteen disjoint 4 KB arrays
    err = lambda: (lib.gsmvi_last_error() or b"").decode()           # noqa: E731

    def call(K=2, P=4, nc=3, N=5, A=a(0), y=a(1), offset=a(7), counts=None, tm=0.0, tm_dev=None, tk=1.0, tk_dev=None, lam=1.0,
             lam_dev=None, X=a(3), G=a(4), lp=a(5)):
        return lib.gsmvi_negbin_batched_f64(None, None, K, P, nc, N, A, y, offset, counts, tm, tm_dev, tk, tk_dev, lam, lam_dev, X, G, lp)

    def bad(what, **kw):
        assert call(**kw) == 1 and what in err() and err().startswith(NAME + ":"), (what, kw, err())

    bad("P must be", P=0)
    bad("P must be", P=64)
    bad("K must be", K=0)
    bad("K must be", K=2 ** 27)
    bad("nc must be", nc=0)
    bad("N must be", N=0)
    bad("K N P is too large", K=2 ** 20, N=2 ** 40)
    bad("K nc D is too large", K=2 ** 24 - 1, nc=2 ** 31 - 1, P=63)
    for name in ("A", "y", "X"):
        bad("NULL array", **{name: None})
    bad("G or lp", G=None, lp=None)
    for v in (-1.0, float("nan"), float("inf")):
        bad("prior_prec must be", lam=v)
        bad("theta_prec must be", tk=v)
    for v in (float("nan"), float("inf"), float("-inf")):
        bad("theta_mean must be", tm=v)
    for name, other in (("A", a(0)), ("y", a(1)), ("X", a(3)), ("offset", a(7))):
        bad(f"G overlaps {name}", G=other)
        bad(f"lp overlaps {name}", lp=other)
    bad("G overlaps prior_prec_dev", lam_dev=a(6), G=a(6))
    bad("lp overlaps theta_mean_dev", tm_dev=a(8), lp=a(8))
    bad("G overlaps theta_prec_dev", tk_dev=a(9), G=a(9))
    bad("G overlaps counts_dev", counts=a(10), G=a(10))
    bad("lp overlaps G", lp=a(4))
    bad("G overlaps X", G=a(3) + 8 * (2 * 3 * 5 - 1))                   # the last element of X: K nc (P + 1) doubles
    bad("G overlaps A", G=a(0) + 8 * (2 * 5 * 4 - 1))                   # the last element of A: K N P doubles
    # adjacent is not overlapping, and valid calls end at the context
    bad("ctx is NULL", G=a(0) + 8 * 2 * 5 * 4)
    bad("ctx is NULL", G=a(3) + 8 * 2 * 3 * 5)
    bad("ctx is NULL")
    bad("ctx is NULL", offset=None, G=None)
    bad("ctx is NULL", lp=None, lam=0.0, tk=0.0, tm=-3.5)
    bad("ctx is NULL", P=63, K=1, nc=1, N=1)
    bad("ctx is NULL", lam=-1.0, lam_dev=a(6), tk=-1.0, tk_dev=a(9), tm=float("nan"), tm_dev=a(8))     # scalars unused with K values
    bad("ctx is NULL", y=a(0), X=a(0), lam_dev=a(0), offset=a(0), tm_dev=a(0), tk_dev=a(0))            # read-only arrays may overlap


def test_lds_budget_stays_within_gb_lds_max():
    """the dynamic LDS a launch requests (the library's own host arithmetic, through the debug build's query in a child process)
    for every D in 2 .. 64, nc in 1 .. 40, all wants, with and without an offset: the formula of DESIGN.md, at most GB_LDS_MAX;
    status 1 outside the ranges"""
    import json
    import sys
    code = (
        "import ctypes as C, json, sys\n"
        "lib = C.CDLL(sys.argv[1])\n"
        f"f = lib.{DEBUG}\n"
        "f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]\n"
        "out = {}\n"
        "for D in range(0, 67):\n"
        "    for nc in range(0, 41):\n"
        "        for want in (0, 1, 2, 3, 4):\n"
        "            for off in (0, 1):\n"
        "                n, p = C.c_size_t(0), C.c_int(0)\n"
        "                st = f(D, nc, want, off, C.byref(n), C.byref(p))\n"
        "                out[f'{D},{nc},{want},{off}'] = [st, n.value, p.value]\n"
        "out['null'] = [f(4, 1, 1, 0, None, None), 0, 0]\n"
        "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.library_path(debug=True)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got.pop("null")[0] == 1
    seen, most = 0, 0
    for key, (st, n, ppw) in got.items():
        D, nc, want, off = (int(x) for x in key.split(","))
        if not (2 <= D <= 64 and nc >= 1 and 1 <= want <= 3):
            assert st == 1, key
            continue
        seen += 1
        P, packed = D - 1, D <= 16
        tcm = min(nc, 16 if packed else 32)
        per = 32 * (P | 1) + 32 + 32 * off + tcm * ((D | 1) + 2 + 33 * ((2 if want & 1 else 0) + (1 if want & 2 else 0)))
        assert st == 0 and ppw == (4 if packed else 1) and n == 8 * ppw * per <= GB_LDS_MAX, (key, n)
        most = max(most, n)
    assert seen == 63 * 40 * 3 * 2 and most == got["16,16,3,1"][1] == 4 * 2432 * 8 and got["64,32,3,1"][1] == 7392 * 8


# ---- 4. host logic of BatchedNegBinomialTarget ------------------------------------------------------------------------------------
def test_target_validates_on_the_host_before_the_engine_is_touched():
    from gsmvi_amd import BatchedNegBinomialTarget
    eng = ref.RestatementEngine()

    def bad(match, **kw):
        A, y, o, counts, lam, tm, tk, X = ref.make_inputs(3, 12, 4, 2)
        base = dict(A=A, y=y, prior_precision=lam, counts=counts, offset=o, log_size_mean=tm, log_size_precision=tk, engine=eng)
        for k, v in kw.items():
            base[k] = v(base[k]) if callable(v) else v
        eng.calls.clear()
        with pytest.raises(ValueError, match=match):
            BatchedNegBinomialTarget(**base)
        assert eng.calls == [], (match, kw)

    def put(k, n, v):
        def f(arr):
            arr = np.array(arr, dtype=np.float64)
            arr[k, n] = v
            return arr
        return f

    bad("^A:", A=lambda A: A[0])
    bad("^A:", A=lambda A: A[:, :, :0])
    bad(r"^A: D = P \+ 1 = 65", A=np.zeros((3, 12, 64)))
    bad("^y:", y=lambda y: y[:, :11])
    bad("^y:", y=lambda y: y[0])
    for v in (-0.5, np.nan, np.inf):
        bad(r"^y: .*\[2\]", y=put(2, 0, v))                               # a live row of problem 2 (counts[2] = 5)
    bad("^counts:", counts=np.array([1, 2], dtype=np.int32))
    bad("^counts:", counts=np.array([1, 2, 13], dtype=np.int32))
    bad("^counts:", counts=np.array([1.0, 2.0, 3.0]))
    bad("^offset:", offset=lambda o: o[:, :11])
    for v in (np.nan, np.inf, -np.inf):
        bad(r"^offset: .*\[2\]", offset=put(2, 0, v))
    for badl in (-0.5, np.nan, np.inf, [0.1, 0.2], [0.1, -0.2, 0.3], [0.1, np.nan, 0.3]):
        bad("^prior_precision:", prior_precision=badl)
        bad("^log_size_precision:", log_size_precision=badl)
    for badm in (np.nan, np.inf, -np.inf, [0.1, 0.2], [0.1, np.nan, 0.3]):
        bad("^log_size_mean:", log_size_mean=badm)
    # the rows beyond counts hold NaN, -1 and inf (make_inputs poisons them): anything goes there; y need not be an integer
    A, y, o, counts, lam, tm, tk, X = ref.make_inputs(3, 12, 4, 2)
    assert np.isnan(A[2, counts[2]:]).all() and np.isinf(o[2, counts[2]:]).all() and counts[1] == 0
    t = BatchedNegBinomialTarget(A, put(2, 0, 2.5)(y), lam, counts, o, tm, tk, engine=eng)
    assert np.isfinite(t.lp_g(X)).all()
    with pytest.raises(ValueError, match=r"^y: .*\[0, 1, 2\]|^y: .*\[1, 2\]"):
        BatchedNegBinomialTarget(A, y, lam, None, o, tm, tk, engine=eng)    # ... unless every row counts
    BatchedNegBinomialTarget(A, y, lam, counts, o, -4.0, 0.0, engine=eng)  # a negative prior mean and a flat prior of theta are fine


def test_target_protocol_on_the_restatement_engine():
    from gsmvi_amd import BatchedGLMTarget, BatchedNegBinomialTarget
    K, N, P, rows = 3, 12, 4, 5
    A, y, o, counts, lam, tm, tk, X = ref.make_inputs(K, N, P, rows)
    G, lp = ref.score_and_lp(A, y, o, counts, lam, tm, tk, X)
    eng = ref.RestatementEngine()
    tgt = BatchedNegBinomialTarget(A, y, lam, counts, o, tm, tk, engine=eng)
    assert not isinstance(tgt, BatchedGLMTarget)
    assert not any(hasattr(tgt, name) for name in ("neg_hessian", "predict", "loo", "family"))
    assert (tgt.K, tgt.N, tgt.P, tgt.D) == (K, N, P, P + 1)
    assert tgt.lp_g.device_native is True and tgt.lp_g.graph_safe is True
    assert all(t.dtype == np.float64 for t in (tgt.A, tgt.y, tgt.offset)) and tgt.counts.dtype == np.int32
    assert np.array_equal(tgt.lp_g(X), G)
    # exactly the arrays it was given, the poisoned rows as they are
    last = eng.last
    assert last["A"] is tgt.A and last["y"] is tgt.y and last["offset"] is tgt.offset and last["counts"] is tgt.counts
    assert np.array_equal(tgt.A, A, equal_nan=True) and np.array_equal(tgt.y, y, equal_nan=True) and np.array_equal(tgt.offset, o)
    assert np.array_equal(tgt.counts, counts) and np.array_equal(last["prior_prec"], lam)
    assert np.array_equal(last["log_size_mean"], tm) and np.array_equal(last["log_size_prec"], tk)
    out = np.empty_like(X)
    assert tgt.lp_g(X, out=out) is out and np.array_equal(out, G)
    v = tgt.lp(X)
    assert v.shape == (K, rows) and np.array_equal(v, lp)
    g2, v2 = tgt.lp_and_score(X)
    assert np.array_equal(g2, G) and np.array_equal(v2, lp)
    assert [c for c in eng.calls if isinstance(c, tuple)] == [("negbin", "g", False), ("negbin", "g", True), ("negbin", "lp", False),
                                                              ("negbin", "both", False)]
    # tensors in, the defaults (lam = 1, m = 0, kap = 1), no counts, no offset, a float32 design
    A2, y2, _, _, _, _, _, _ = ref.make_inputs(K, N, P, rows, poison=False)
    t = BatchedNegBinomialTarget(torch.tensor(A2, dtype=torch.float32), torch.tensor(y2), engine=eng)
    Gs, lps = ref.score_and_lp(A2.astype(np.float32), y2, None, None, 1.0, 0.0, 1.0, X)
    assert t.counts is None and t.offset is None and (t.prior_precision, t.log_size_mean, t.log_size_precision) == (1.0, 0.0, 1.0)
    assert np.array_equal(t.lp_g(torch.tensor(X)), Gs) and np.array_equal(t.lp(torch.tensor(X)), lps)
    from gsmvi_amd.monitors import lp_sums
    s = lp_sums(tgt.lp, X, eng, K)
    assert s.shape == (K,) and rel_err(s, lp.sum(1)) < 1e-15
    # the engine method refuses an X that is not (beta, theta)
    from gsmvi_amd.engine import HipEngine
    with pytest.raises(ValueError, match="^X: expected P \\+ 1 = 5 columns"):
        HipEngine.negbin_batched(object.__new__(HipEngine), torch.zeros(K, rows, P), torch.zeros(K, N, P), torch.zeros(K, N))


class _Host(np.ndarray):
    """a host array with the tensor methods lbfgs_init_batched calls"""

    def dim(self):
        return self.ndim

    def contiguous(self):
        return self

    def expand(self, *shape):
        return np.broadcast_to(self, shape).view(_Host)


def _lbfgs_engine():
    """tests/pathfinder_batched_ref.py's stand-in with what lbfgs_init_batched asks beyond the Pathfinder driver"""
    import lbfgs_batched_ref as lref
    import pathfinder_batched_ref as pfref

    class Engine(pfref.StandInEngine):
        def asarray(self, x):
            return np.array(x, dtype=np.float64, copy=True).view(_Host)

        def lbfgs_hess_inv_batched(self, st):
            return np.stack([lref.hess_inv(pfref.unpack(st, k, {})) for k in range(st["x"].shape[0])])
    return Engine()


def test_the_fits_the_initialisers_and_psis_accept_the_target():
    """GSMBatch, ADVIBatch, psis_batched, lbfgs_init_batched and pathfinder_init_batched on their stand-in engines, scored by the
    target on the restatement: the results are those of the same runs scored by plain callables; what needs a Hessian or the
    pointwise likelihood refuses the target"""
    import gsmvi_amd
    import pathfinder_batched_ref as pfref
    import psis_batched_ref as pref
    from engines import OracleBatchedEngine
    from test_advi_batched_cpu import OracleBatchedADVIEngine
    K, N, P, B, niter = 3, 30, 3, 3, 5
    D = P + 1
    A, y, o, counts, lam, tm, tk, _ = ref.make_inputs(K, N, P, 1, seed=5)
    counts[1] = N - 2
    A, y, o = np.nan_to_num(A), np.abs(np.nan_to_num(y)), np.nan_to_num(o, posinf=0.0)
    lam, tk = lam + 0.5, tk + 0.5
    tgt = gsmvi_amd.BatchedNegBinomialTarget(A, y, lam, counts, o, tm, tk, engine=ref.RestatementEngine())
    lp_h = lambda X: ref.score_and_lp(A, y, o, counts, lam, tm, tk, np.asarray(X))[1]   # noqa: E731
    lpg_h = lambda X: ref.score_and_lp(A, y, o, counts, lam, tm, tk, np.asarray(X))[0]  # noqa: E731
    keys = [3, 99, 1000]
    a = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g, engine=OracleBatchedEngine()).fit(keys, batch_size=B, niter=niter, verbose=False)
    b = gsmvi_amd.GSMBatch(K, D, lp_h, lpg_h, engine=OracleBatchedEngine()).fit(keys, batch_size=B, niter=niter, verbose=False)
    assert all(np.array_equal(u, v) and np.isfinite(u).all() for u, v in zip(a, b)) and a[0].shape == (K, D)
    a = gsmvi_amd.ADVIBatch(K, D, tgt.lp, tgt.lp_g, engine=OracleBatchedADVIEngine()).fit(
        keys, gsmvi_amd.Adam(0.05), batch_size=B, niter=niter, verbose=False, track_loss=True)
    b = gsmvi_amd.ADVIBatch(K, D, lp_h, lpg_h, engine=OracleBatchedADVIEngine()).fit(
        keys, gsmvi_amd.Adam(0.05), batch_size=B, niter=niter, verbose=False, track_loss=True)
    assert all(np.array_equal(u, v) and np.isfinite(u).all() for u, v in zip(a, b)) and a[2].shape[-1] == K
    mean, cov = a[0], a[1]
    r = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=16, engine=pref.StandInEngine())
    r2 = gsmvi_amd.psis_batched(lp_h, mean, cov, keys, num_draws=16, engine=pref.StandInEngine())
    assert r.khat.shape == (K,) and np.array_equal(r.khat, r2.khat) and np.array_equal(r.log_ratios, r2.log_ratios)
    x0 = np.zeros((K, D))
    m1, c1, r1 = gsmvi_amd.lbfgs_init_batched(x0, tgt.lp, tgt.lp_g, engine=_lbfgs_engine())
    m2, c2, r2 = gsmvi_amd.lbfgs_init_batched(x0, lp_h, lpg_h, engine=_lbfgs_engine())
    assert np.array_equal(m1, m2) and np.array_equal(c1, c2) and r1.success.all() and m1.shape == (K, D)
    assert np.abs(lpg_h(m1[:, None, :])).max() <= 1e-3                     # a mode of all K posteriors
    m1, c1, r1 = gsmvi_amd.pathfinder_init_batched(x0, tgt.lp, tgt.lp_g, num_elbo_draws=4, engine=pfref.StandInEngine())
    m2, c2, r2 = gsmvi_amd.pathfinder_init_batched(x0, lp_h, lpg_h, num_elbo_draws=4, engine=pfref.StandInEngine())
    assert np.array_equal(m1, m2) and np.array_equal(c1, c2) and np.array_equal(r1.elbo, r2.elbo) and np.isfinite(r1.elbo).all()
    with pytest.raises(TypeError):
        gsmvi_amd.laplace_init_batched(tgt)
    with pytest.raises(TypeError):
        gsmvi_amd.psis_loo_batched(tgt, mean, cov, keys)
