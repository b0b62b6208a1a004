"""The batched ordinal target without a GPU: the float64 restatement of the link (tests/ordinal_batched_ref.py) against the mpmath
truth over the whole grid (tests/ordinal_link_truth.py), the golden table against fresh mpmath, the closed-form derivatives against
mp.diff of the written density, the probabilities summing to 1, the restatements against each other, the C = 2 model against
logistic regression; the C ABI declaration and argument checks of gsmvi_ordinal_batched_f64, its LDS budget; and the host logic of
BatchedOrdinalTarget on a stand-in engine, inside the fits, the initialisers and psis_batched on theirs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ordinal_batched_ref as ref
import ordinal_link_truth as truth
from gsmvi_amd import _lib
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsmvi_ordinal_batched_f64"
DEBUG = "gsmvi_debug_ordinal_batched_lds"
GB_LDS_MAX = 160 * 1024                          # csrc/gsmvi_batched.h


def _mp():
    return pytest.importorskip("mpmath")


# ---- 1. the link, element by element -------------------------------------------------------------------------------------------
def test_float64_restatement_meets_the_truth_over_the_whole_grid():
    """worst err / (eps scale) per quantity over the grid, asserted against the recorded C_CPU (measured 0.47 / 0.39 / 0.39 / 0.54
    for t / r_eta / d delta_0 / d delta_1); and the naive difference of two probabilities is far outside: the metric bites"""
    tab = truth.load_table()
    eta, d0, d1, y = truth.grid()
    assert np.array_equal(tab["delta1s"], truth.delta1s()) and tab["t"].shape == (2, eta.size)
    assert eta.size == 3 * len(truth.D0_VALUES) * len(truth.H_VALUES) * len(truth.delta1s())
    w = np.exp(d1)
    near = np.abs(d1 - truth.LOGLOG2) < 1e-12                             # both sides of the log1mexp threshold, a hair from it
    assert (w[near] < ref.LOG2).any() and (w[near] >= ref.LOG2).any()
    got = ref.link3(eta, d0, d1, y)
    for q, g in zip(truth.QUANTITIES, got):
        worst = truth.ratio(g, tab, q)
        i = int(np.argmax(worst))
        print(f"ordinal {q}: worst ratio {worst[i]:.3f} at eta = {eta[i]!r}, delta = ({d0[i]!r}, {d1[i]!r}), y = {y[i]} "
              f"(C_CPU {truth.C_CPU[q]})")
        assert worst[i] <= truth.C_CPU[q], (q, worst[i])
    # the naive log(sigmoid(b) - sigmoid(a)) and the gradient autograd would form from it
    with np.errstate(all="ignore"):
        sig = lambda x: 1.0 / (1.0 + np.exp(-x))                          # noqa: E731
        c0, c1 = d0, d0 + w
        b, a = np.where(y == 0, c0, c1) - eta, np.where(y == 1, c0, c1) - eta
        hi, lo = np.where(y <= 1, sig(b), 1.0), np.where(y >= 1, sig(a), 0.0)
        p = hi - lo
        sb, sa = np.where(y <= 1, sig(b) * (1.0 - sig(b)), 0.0), np.where(y >= 1, sig(a) * (1.0 - sig(a)), 0.0)
        naive = (np.log(p), (sa - sb) / p, (sb - sa) / p, w * np.where(y == 1, sb, np.where(y == 2, -sa, 0.0)) / p)
    for q, g in zip(truth.QUANTITIES, naive):
        r = truth.ratio(g, tab, q)
        fin = r[np.isfinite(r)]
        print(f"naive {q}: {np.isinf(r).sum()} of {r.size} points NaN or a wrong infinity; the worst finite ratio {fin.max():.3g} eps "
              f"of the scale")
        # (measured: 256 points lost, the worst finite ratio 1.1e14 for t, r_eta, d delta_0 and 9.0e14 for d delta_1)
        assert np.isinf(r).sum() >= 100 and fin.max() > 1e12 and fin.max() > 1e12 * truth.C_CPU[q]


def test_golden_table_is_fresh_mpmath():
    """a seeded sample of the grid and a part of the points beyond it, recomputed"""
    _mp()
    tab = truth.load_table()
    assert os.path.getsize(truth.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(truth.GOLDEN), "negbin_link_truth.npz"))
    eta, d0, d1, y = truth.grid()
    pick = np.random.RandomState(3).choice(eta.size, 60, replace=False)
    for i in pick:
        v = truth.values(eta[i], d0[i], d1[i], int(y[i]))
        for q in truth.QUANTITIES:
            hi, lo = truth.split(v[q])
            assert hi == tab[q][0, i] and lo == tab[q][1, i], (q, i)
            s = float(v["scale_" + q])
            assert 0.0 <= s - truth.unpack_scale(tab, q)[i] <= 2.5e-7 * s, (q, i)
    pts = truth.beyond_points()
    assert len(pts) == len(tab["beyond"])
    for pt, row in list(zip(pts, tab["beyond"]))[::5]:
        assert list(pt) == row[:4].tolist()
        v = dict(zip(truth.NAMES, truth._at(*pt, 400)))
        assert [truth.split(v[q])[0] for q in truth.QUANTITIES] == row[4:].tolist()


def test_closed_form_gradient_is_mp_diff_of_the_written_density():
    """C in {2, 3, 5}, every label: the restatement's score of one observation (P = 1, A = a, no priors) equals mp.diff of
    log(sigma(cut_y - eta) - sigma(cut_{y-1} - eta)) in beta and in every delta_j, the chain rule through the cutpoints included"""
    mp = _mp()
    rs = np.random.RandomState(11)
    for Cc in (2, 3, 5):
        for y in range(Cc):
            a, o, beta = 0.7, 0.25, float(rs.standard_normal())
            delta = np.concatenate([rs.standard_normal(1), rs.uniform(-1.5, 1.0, Cc - 2)])
            X = np.concatenate([[beta], delta])[None, None, :]
            G, lp = ref.score_and_lp(np.full((1, 1, 1), a), np.array([[y]]), np.full((1, 1), o), None, 0.0, 0.0, X, Cc)
            with mp.workdps(50):
                f = lambda *x: truth.written(mp.mpf(a) * x[0] + mp.mpf(o), list(x[1:]), y)       # noqa: E731
                at = tuple(mp.mpf(float(v)) for v in X[0, 0])
                assert abs(f(*at) - mp.mpf(float(lp[0, 0]))) <= 1e-14 * (1 + abs(f(*at)))
                for j in range(Cc):
                    d = mp.diff(f, at, tuple(int(i == j) for i in range(Cc)))
                    assert abs(d - mp.mpf(float(G[0, 0, j]))) <= 1e-13 * (1 + abs(d)), (Cc, y, j)


def test_class_probabilities_sum_to_one():
    """sum_c exp(t(y = c)) = 1 within a few eps for C in {2, 3, 7} at random (eta, delta)"""
    rs = np.random.RandomState(12)
    for Cc in (2, 3, 7):
        rows = 50
        X = np.concatenate([np.zeros((1, rows, 1)), 2.0 * rs.standard_normal((1, rows, 1)), rs.uniform(-3.0, 1.5, (1, rows, Cc - 2))], 2)
        cut, w = ref.cutpoints(X[0, :, 1:])
        lm, qe = ref.gap(w)
        eta = 3.0 * rs.standard_normal((rows, 1))
        tot = np.zeros(rows)
        for c in range(Cc):
            tot = tot + np.exp(ref.link(eta, np.array([c]), cut, lm, qe)[3][:, 0])
        assert np.abs(tot - 1.0).max() <= 8 * truth.EPS, (Cc, np.abs(tot - 1.0).max())


# ---- 2. the restatements ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,P,Cc,rows", [(3, 1, 1, 2, 1), (5, 33, 12, 5, 3), (3, 70, 1, 64, 2), (4, 40, 61, 4, 3)])
def test_float64_and_longdouble_restatements_agree_and_follow_the_rules(K, N, P, Cc, rows):
    A, y, o, counts, lam, kap, X = ref.make_inputs(K, N, P, Cc, rows)
    D = P + Cc - 1
    G, lp = ref.score_and_lp(A, y, o, counts, lam, kap, X, Cc)
    Gl, lpl = ref.score_and_lp_ld(A, y, o, counts, lam, kap, X, Cc)
    assert np.isfinite(G).all() and np.isfinite(lp).all() and G.shape == (K, rows, D)
    for k in range(K):
        assert rel_err(G[k], Gl[k].astype(np.float64)) <= 1e-12 and rel_err(lp[k], lpl[k].astype(np.float64)) <= 1e-12, k
    if K > 1:                                                             # counts = 0: the two priors, exactly
        assert counts[1] == 0
        assert np.array_equal(G[1, :, :P], 0.0 - lam[1] * X[1, :, :P]) and np.array_equal(G[1, :, P:], 0.0 - kap[1] * X[1, :, P:])
        assert np.array_equal(lp[1], (0.0 - 0.5 * lam[1] * _chain(X[1, :, :P] ** 2)) - 0.5 * kap[1] * _chain(X[1, :, P:] ** 2))
    if K > 2 and Cc > 2:                                                  # a class absent from the data is fine
        assert not (y[K - 1, :counts[K - 1]] == Cc - 1).any()
    # dead rows play no part: other values there, the same bits
    A2, y2, o2 = A.copy(), y.copy(), o.copy()
    for k in range(K):
        A2[k, counts[k]:], y2[k, counts[k]:], o2[k, counts[k]:] = 1.0, 0, 0.0
    G2, lp2 = ref.score_and_lp(A2, y2, o2, counts, lam, kap, X, Cc)
    assert np.array_equal(G, G2) and np.array_equal(lp, lp2)
    # the order of the sums: the rows reversed give other bits in general but the same value, and the sum over n is the loop's
    k = 0
    n = counts[k]
    t = ref.score_and_lp(A[k:k + 1, :n], y[k:k + 1, :n], o[k:k + 1, :n], None, 0.0, 0.0, X[k:k + 1], Cc)[1][0]
    parts = [ref.score_and_lp(A[k:k + 1, i:i + 1], y[k:k + 1, i:i + 1], o[k:k + 1, i:i + 1], None, 0.0, 0.0, X[k:k + 1], Cc)[1][0]
             for i in range(n)]
    s = np.zeros(rows)
    for v in parts:
        s = s + v
    assert np.array_equal(s, t)
    # a central difference of lp is the score (a beta, delta_0 and the last delta)
    h = 1e-6
    for j in (0, P, D - 1):
        Xp, Xm = X.copy(), X.copy()
        Xp[k, :, j] += h
        Xm[k, :, j] -= h
        fd = (ref.score_and_lp(A, y, o, counts, lam, kap, Xp, Cc)[1][k] - ref.score_and_lp(A, y, o, counts, lam, kap, Xm, Cc)[1][k]) / (2 * h)
        assert np.abs(fd - G[k, :, j]).max() <= 1e-5 * max(1.0, np.abs(G[k, :, j]).max()), j
    # the row flags: a non-finite entry, and delta_j = +-750 for j >= 1; delta_0 = +-750 is a location and stays finite
    X3 = np.repeat(X[:, :1], 6, axis=1).copy()
    X3[0, 1, 0], X3[0, 4, P], X3[0, 5, P] = np.inf, 750.0, -750.0
    if Cc > 2:
        X3[0, 2, D - 1], X3[0, 3, P + 1] = 750.0, -750.0
    G3, lp3 = ref.score_and_lp(A, y, o, counts, lam, kap, X3, Cc)
    flagged = [1, 2, 3] if Cc > 2 else [1]
    assert np.isnan(G3[0, flagged]).all() and np.isnan(lp3[0, flagged]).all()
    fine = [r for r in range(6) if r not in flagged]
    assert np.isfinite(G3[0, fine]).all() and np.isfinite(lp3[0, fine]).all() and np.isfinite(G3[1:]).all()


def _chain(sq):
    s = np.zeros(sq.shape[0])
    for j in range(sq.shape[1]):
        s = s + sq[:, j]
    return s


def test_two_classes_are_logistic_regression_on_the_design_with_a_minus_one_column():
    K, N, P, rows = 3, 37, 4, 3
    A, y, o, counts, lam, kap, X = ref.make_inputs(K, N, P, 2, rows, poison=False)
    for lamv in (0.0, 0.7):
        G, lp = ref.score_and_lp(A, y, None, None, lamv, lamv, X, 2)
        A1 = np.concatenate([A, -np.ones((K, N, 1))], axis=2)
        Gl, lpl = ref.logistic_score_and_lp(A1, y.astype(np.float64), lamv, X)
        for k in range(K):
            assert rel_err(G[k], Gl[k]) <= 1e-13 and rel_err(lp[k], lpl[k]) <= 1e-13, (k, lamv)


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr)
    for mp in ("exports.map", "exports_debug.map"):
        assert re.search(r"^\s*" + NAME + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), mp
    assert NAME in _lib.exported_symbols() and NAME in built
    block = hdr[:hdr.index("int " + NAME)].rsplit("/*", 1)[1]
    assert "example_gsm.py:34-35" in block and "GSMVI_PATH_BATCHED_TARGET" in block
    res, args = _lib._SIGS[NAME]
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert res is C.c_int and len(args) == len(params) == 18
    for p, a in zip(params, args):
        want = C.c_double if p.startswith("double ") else C.c_int64 if p.startswith("int64_t") else \
            C.c_int if p.startswith("int ") else C.c_void_p
        assert a is want, (p, a)
    assert params[3] == "int P" and params[4] == "int C" and params[8] == "const int* y" and params[13] == "double cut_prec"
    dhdr = open(os.path.join(ROOT, "include", "gsmvi_hip_debug.h")).read()
    assert re.search(r"\bint\s+" + DEBUG + r"\s*\(", dhdr) and DEBUG not in hdr
    assert DEBUG in open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "exports_debug.map")).read()
    assert DEBUG not in open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "exports.map")).read()
    dbg = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path(debug=True)], check=True, capture_output=True,
                         text=True).stdout
    assert DEBUG in dbg and NAME in dbg and DEBUG not in out
    assert DEBUG in _lib._DEBUG_SIGS and DEBUG not in _lib._SIGS
    mk = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "Makefile")).read()
    assert "gsmvi_ordinal_batched.hip" in mk and "gsmvi_ordinal_link.h" in mk


def test_build_compiled_the_twelve_instantiations_for_gfx950():
    """the library build() left holds k_ordinal_batched<NT, WANT, OFF> for both packings, the three wants, with and without an offset"""
    blob = open(_lib.library_path(), "rb").read()
    assert b"gfx950" in blob
    for nt in (64, 256):
        for want in (1, 2, 3):
            for off in (0, 1):
                assert f"_Z17k_ordinal_batchedILi{nt}ELi{want}ELb{off}EEv7ob_args".encode() in blob, (nt, want, off)


def test_no_path_bit_is_added():
    """all 32 bits are taken: the launch reports the batched target's, 0x20000"""
    from gsmvi_amd.engine import HipEngine
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    bits = dict(re.findall(r"#define\s+(GSMVI_PATH_\w+)\s+(0x[0-9a-fA-F]+)u", hdr))
    assert len(bits) == 32 and int(bits["GSMVI_PATH_BATCHED_TARGET"], 16) == 0x20000
    assert len(HipEngine.PATH_BITS) == 32
    src = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_ordinal_batched.hip")).read()
    assert re.findall(r"GSMVI_PATH_\w+", src) == ["GSMVI_PATH_BATCHED_TARGET"]


def test_abi_checks_arguments_before_the_context_and_names_overlapping_arrays():
    """every bad argument is reported with a NULL context (no device work can have started); valid ones end at the context"""
    lib = _lib.load_library()
    buf = (C.c_double * 8192)()
    p = C.cast(buf, C.c_void_p).value
    a = lambda n: p + 8 * 512 * n                                   # noqa: E731  sixteen disjoint 4 KB arrays
    err = lambda: (lib.gsmvi_last_error() or b"").decode()           # noqa: E731

    def call(K=2, P=4, Cc=3, nc=3, N=5, A=a(0), y=a(1), offset=a(7), counts=None, lam=1.0, lam_dev=None, kap=1.0, kap_dev=None,
             X=a(3), G=a(4), lp=a(5)):
        return lib.gsmvi_ordinal_batched_f64(None, None, K, P, Cc, nc, N, A, y, offset, counts, lam, lam_dev, kap, kap_dev, X, G, lp)

    def bad(what, **kw):
        assert call(**kw) == 1 and what in err() and err().startswith(NAME + ":"), (what, kw, err())

    bad("C must be", Cc=1)
    bad("C must be", Cc=65)
    bad("P must be", P=0)
    bad("P must be", P=63)                                             # D = 65 at C = 3
    bad("P must be", P=2, Cc=64)
    bad("K must be", K=0)
    bad("K must be", K=2 ** 27)
    bad("nc must be", nc=0)
    bad("N must be", N=0)
    bad("K N P is too large", K=2 ** 20, N=2 ** 40)
    bad("K nc D is too large", K=2 ** 24 - 1, nc=2 ** 31 - 1, P=62)
    for name in ("A", "y", "X"):
        bad("NULL array", **{name: None})
    bad("G or lp", G=None, lp=None)
    for v in (-1.0, float("nan"), float("inf")):
        bad("prior_prec must be", lam=v)
        bad("cut_prec must be", kap=v)
    for name, other in (("A", a(0)), ("y", a(1)), ("X", a(3)), ("offset", a(7))):
        bad(f"G overlaps {name}", G=other)
        bad(f"lp overlaps {name}", lp=other)
    bad("G overlaps prior_prec_dev", lam_dev=a(6), G=a(6))
    bad("lp overlaps cut_prec_dev", kap_dev=a(8), lp=a(8))
    bad("G overlaps counts_dev", counts=a(10), G=a(10))
    bad("lp overlaps G", lp=a(4))
    bad("G overlaps X", G=a(3) + 8 * (2 * 3 * 6 - 1))                   # the last element of X: K nc (P + C - 1) doubles
    bad("G overlaps A", G=a(0) + 8 * (2 * 5 * 4 - 1))                   # the last element of A: K N P doubles
    bad("G overlaps y", G=a(1) + 4 * (2 * 5 - 1))                       # the last label: K N ints
    # adjacent is not overlapping, and valid calls end at the context
    bad("ctx is NULL", G=a(0) + 8 * 2 * 5 * 4)
    bad("ctx is NULL", G=a(3) + 8 * 2 * 3 * 6)
    bad("ctx is NULL", G=a(1) + 4 * 2 * 5)
    bad("ctx is NULL")
    bad("ctx is NULL", offset=None, G=None)
    bad("ctx is NULL", lp=None, lam=0.0, kap=0.0)
    bad("ctx is NULL", P=63, Cc=2, K=1, nc=1, N=1)
    bad("ctx is NULL", P=1, Cc=64, K=1, nc=1, N=1)
    bad("ctx is NULL", lam=-1.0, lam_dev=a(6), kap=-1.0, kap_dev=a(9))                                 # scalars unused with K values
    bad("ctx is NULL", y=a(0), X=a(0), lam_dev=a(0), offset=a(0), kap_dev=a(0))                        # read-only arrays may overlap


def _lds_formula(Cc, P, nc, want, off):
    """bytes of dynamic LDS and problems per workgroup"""
    D = P + Cc - 1
    packed = D <= 16
    tcm = min(nc, 16 if packed else 32)
    per = 32 * (P | 1) + 16 + 32 * off + tcm * ((D | 1) + 1 + 4 * (Cc - 1) + 33 * ((3 if want & 1 else 0) + (1 if want & 2 else 0)))
    return 8 * (4 if packed else 1) * per, 4 if packed else 1


def test_lds_budget_stays_within_gb_lds_max():
    """the dynamic LDS a launch requests (the library's own host arithmetic, through the debug build's query in a child process)
    for a thinned grid of (C, P) with P + C - 1 <= 64, every nc in 1 .. 40, all wants, with and without an offset: the formula of
    DESIGN.md, at most GB_LDS_MAX; status 1 outside the ranges"""
    import json
    import sys
    Cs, Ps = [1, 2, 3, 4, 5, 8, 15, 16, 17, 33, 63, 64, 65], [0, 1, 2, 3, 5, 8, 11, 12, 13, 15, 16, 31, 32, 47, 60, 61, 62, 63, 64]
    code = (
        "import ctypes as C, json, sys\n"
        "lib = C.CDLL(sys.argv[1])\n"
        f"f = lib.{DEBUG}\n"
        "f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]\n"
        "out = {}\n"
        f"for Cc in {Cs!r}:\n"
        f"    for P in {Ps!r}:\n"
        "        for nc in range(0, 41):\n"
        "            for want in (0, 1, 2, 3, 4):\n"
        "                for off in (0, 1):\n"
        "                    n, p = C.c_size_t(0), C.c_int(0)\n"
        "                    st = f(Cc, P, nc, want, off, C.byref(n), C.byref(p))\n"
        "                    out[f'{Cc},{P},{nc},{want},{off}'] = [st, n.value, p.value]\n"
        "out['null'] = [f(3, 4, 1, 1, 0, None, None), 0, 0]\n"
        "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.library_path(debug=True)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got.pop("null")[0] == 1
    seen, most, shapes = 0, 0, set()
    for key, (st, n, ppw) in got.items():
        Cc, P, nc, want, off = (int(x) for x in key.split(","))
        if not (Cc >= 2 and P >= 1 and P + Cc - 1 <= 64 and nc >= 1 and 1 <= want <= 3):
            assert st == 1, key
            continue
        seen += 1
        shapes.add((Cc, P))
        assert st == 0 and (n, ppw) == _lds_formula(Cc, P, nc, want, off) and n <= GB_LDS_MAX, (key, n)
        most = max(most, n)
    assert seen == len(shapes) * 40 * 3 * 2 and {(2, 63), (64, 1), (5, 12), (5, 13), (16, 1), (17, 1)} <= shapes
    # the most: one problem of C = 64 (113.1 KB); four packed problems of C = 16: 107.5 KB
    assert most == got["64,1,32,3,1"][1] == 14480 * 8 and got["16,1,16,3,1"][1] == 4 * 3440 * 8


# ---- 4. host logic of BatchedOrdinalTarget ----------------------------------------------------------------------------------------
def test_target_validates_on_the_host_before_the_engine_is_touched():
    from gsmvi_amd import BatchedOrdinalTarget
    eng = ref.RestatementEngine()
    Cc = 4

    def bad(match, **kw):
        A, y, o, counts, lam, kap, X = ref.make_inputs(3, 12, 4, Cc, 2)
        base = dict(A=A, y=y, num_classes=Cc, prior_precision=lam, cut_precision=kap, counts=counts, offset=o, engine=eng)
        for k, v in kw.items():
            base[k] = v(base[k]) if callable(v) else v
        eng.calls.clear()
        with pytest.raises(ValueError, match=match):
            BatchedOrdinalTarget(**base)
        assert eng.calls == [], (match, kw)

    def put(k, n, v, dtype=np.float64):
        def f(arr):
            arr = np.array(arr, dtype=dtype)
            arr[k, n] = v
            return arr
        return f

    bad("^A:", A=lambda A: A[0])
    bad("^A:", A=lambda A: A[:, :, :0])                                   # P = 0
    bad(r"^A: D = P \+ num_classes - 1 = 65", A=np.zeros((3, 12, 62)))
    for v in (1, 0, -3, 2.0, True, None):
        bad("^num_classes:", num_classes=v)
    bad("^y:", y=lambda y: y[:, :11])
    bad("^y:", y=lambda y: y[0])
    bad(r"^y: .*\[2\]", y=put(2, 0, Cc, np.int64))                        # a live row of problem 2 (counts[2] = 5): a label C
    bad(r"^y: .*\[2\]", y=put(2, 0, -1, np.int64))
    bad(r"^y: .*\[2\]", y=put(2, 0, 1.5))                                 # a fractional label
    bad(r"^y: .*\[2\]", y=put(2, 0, np.nan))
    bad("^y: expected integer labels", y=lambda y: np.zeros(y.shape, dtype=bool))
    bad("^counts:", counts=np.array([1, 2], dtype=np.int32))
    bad("^counts:", counts=np.array([1, 2, 13], dtype=np.int32))
    bad("^counts:", counts=np.array([1.0, 2.0, 3.0]))
    bad("^offset:", offset=lambda o: o[:, :11])
    for v in (np.nan, np.inf, -np.inf):
        bad(r"^offset: .*\[2\]", offset=put(2, 0, v))
    for badl in (-0.5, np.nan, np.inf, [0.1, 0.2], [0.1, -0.2, 0.3], [0.1, np.nan, 0.3]):
        bad("^prior_precision:", prior_precision=badl)
        bad("^cut_precision:", cut_precision=badl)
    # the rows beyond counts hold NaN, labels out of range and inf (make_inputs poisons them): anything goes there; float labels
    # with integral values are fine; precisions of 0 are allowed
    A, y, o, counts, lam, kap, X = ref.make_inputs(3, 12, 4, Cc, 2)
    assert np.isnan(A[2, counts[2]:]).all() and np.isinf(o[2, counts[2]:]).all() and counts[1] == 0 and (y[2, counts[2]:] > Cc).all()
    t = BatchedOrdinalTarget(A, y.astype(np.float64), Cc, lam, kap, counts, o, engine=eng)
    assert np.isfinite(t.lp_g(X)).all() and t.y.dtype == np.int32 and (t.y[2, counts[2]:] == 0).all()
    with pytest.raises(ValueError, match=r"^y: .*\[0, 1, 2\]|^y: .*\[1, 2\]"):
        BatchedOrdinalTarget(A, y, Cc, lam, kap, None, o, engine=eng)     # ... unless every row counts
    BatchedOrdinalTarget(A, y, Cc, 0.0, 0.0, counts, o, engine=eng)


def test_target_protocol_and_cutpoints_on_the_restatement_engine():
    from gsmvi_amd import BatchedGLMTarget, BatchedOrdinalTarget
    K, N, P, Cc, rows = 3, 12, 4, 4, 5
    D = P + Cc - 1
    A, y, o, counts, lam, kap, X = ref.make_inputs(K, N, P, Cc, rows)
    G, lp = ref.score_and_lp(A, y, o, counts, lam, kap, X, Cc)
    eng = ref.RestatementEngine()
    tgt = BatchedOrdinalTarget(A, y, Cc, lam, kap, counts, o, engine=eng)
    assert not isinstance(tgt, BatchedGLMTarget)
    assert not any(hasattr(tgt, name) for name in ("neg_hessian", "predict", "loo", "family"))
    assert (tgt.K, tgt.N, tgt.P, tgt.C, tgt.D) == (K, N, P, Cc, D)
    assert tgt.lp_g.device_native is True and tgt.lp_g.graph_safe is True
    assert all(t.dtype == np.float64 for t in (tgt.A, tgt.offset)) and tgt.counts.dtype == np.int32 and tgt.y.dtype == np.int32
    assert np.array_equal(tgt.lp_g(X), G)
    last = eng.last
    assert last["A"] is tgt.A and last["y"] is tgt.y and last["offset"] is tgt.offset and last["counts"] is tgt.counts
    assert last["C"] == Cc and np.array_equal(tgt.A, A, equal_nan=True) and np.array_equal(tgt.offset, o)
    assert np.array_equal(tgt.counts, counts) and np.array_equal(last["prior_prec"], lam) and np.array_equal(last["cut_prec"], kap)
    out = np.empty_like(X)
    assert tgt.lp_g(X, out=out) is out and np.array_equal(out, G)
    v = tgt.lp(X)
    assert v.shape == (K, rows) and np.array_equal(v, lp)
    g2, v2 = tgt.lp_and_score(X)
    assert np.array_equal(g2, G) and np.array_equal(v2, lp)
    assert [c for c in eng.calls if isinstance(c, tuple)] == [("ordinal", "g", False), ("ordinal", "g", True), ("ordinal", "lp", False),
                                                              ("ordinal", "both", False)]
    # cutpoints: (..., D) -> (..., C - 1), ordered, the restatement's chain; numpy in numpy out, tensors in tensors out
    cut = tgt.cutpoints(X)
    assert isinstance(cut, np.ndarray) and cut.shape == (K, rows, Cc - 1) and (np.diff(cut, axis=-1) > 0).all()
    assert rel_err(cut[1], ref.cutpoints(X[1, :, P:])[0]) <= 1e-15
    ct = tgt.cutpoints(torch.tensor(X[0, 0]))
    assert isinstance(ct, torch.Tensor) and ct.shape == (Cc - 1,) and np.allclose(ct.numpy(), cut[0, 0], rtol=1e-15)
    with pytest.raises(ValueError, match="^x:"):
        tgt.cutpoints(X[..., :-1])
    # tensors in, the defaults (lam = kap = 1), no counts, no offset, a float32 design
    A2, y2, _, _, _, _, _ = ref.make_inputs(K, N, P, Cc, rows, poison=False)
    t = BatchedOrdinalTarget(torch.tensor(A2, dtype=torch.float32), torch.tensor(y2), Cc, engine=eng)
    Gs, lps = ref.score_and_lp(A2.astype(np.float32), y2, None, None, 1.0, 1.0, X, Cc)
    assert t.counts is None and t.offset is None and (t.prior_precision, t.cut_precision) == (1.0, 1.0)
    assert np.array_equal(t.lp_g(torch.tensor(X)), Gs) and np.array_equal(t.lp(torch.tensor(X)), lps)
    from gsmvi_amd.monitors import lp_sums
    s = lp_sums(tgt.lp, X, eng, K)
    assert s.shape == (K,) and rel_err(s, lp.sum(1)) < 1e-15
    # the engine method refuses an X that is not (beta, delta)
    from gsmvi_amd.engine import HipEngine
    with pytest.raises(ValueError, match="^X: expected P \\+ C - 1 = 7 columns"):
        HipEngine.ordinal_batched(object.__new__(HipEngine), torch.zeros(K, rows, P), torch.zeros(K, N, P), torch.zeros(K, N), Cc)
    with pytest.raises(ValueError, match="^C: expected at least 2 classes, got 1"):
        HipEngine.ordinal_batched(object.__new__(HipEngine), torch.zeros(K, rows, P), torch.zeros(K, N, P), torch.zeros(K, N), 1)


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
    K, N, P, Cc, B, niter = 3, 30, 2, 3, 3, 5
    D = P + Cc - 1
    A, y, o, counts, lam, kap, _ = ref.make_inputs(K, N, P, Cc, 1, seed=5, poison=False)
    counts[1] = N - 2
    lam, kap = lam + 0.5, kap + 0.5
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, Cc, lam, kap, counts, o, engine=ref.RestatementEngine())
    lp_h = lambda X: ref.score_and_lp(A, y, o, counts, lam, kap, np.asarray(X), Cc)[1]   # noqa: E731
    lpg_h = lambda X: ref.score_and_lp(A, y, o, counts, lam, kap, np.asarray(X), Cc)[0]  # noqa: E731
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
    for fn in (gsmvi_amd.laplace_init_batched, gsmvi_amd.laplace_init_softmax_batched, gsmvi_amd.laplace_init_negbin_batched):
        with pytest.raises(TypeError):
            fn(tgt)
    for fn in (gsmvi_amd.psis_loo_batched, gsmvi_amd.psis_loo_softmax_batched, gsmvi_amd.psis_loo_negbin_batched):
        with pytest.raises(TypeError):
            fn(tgt, mean, cov, keys)


def test_planted_cutpoints_on_the_restatement_set_the_gpu_tolerance():
    """the planted problem of tests/test_gpu_ordinal_batched.py, the same fit with the same draws on the stand-in engines scored by
    the float64 restatement: the worst |fitted - planted| cutpoint is 0.263, and the GPU test's tolerance keeps a margin of 1.5
    over what is measured here"""
    import gsmvi_amd
    import test_gpu_ordinal_batched as gpu
    from engines import OracleBatchedEngine
    A, y, beta, cuts = gpu.planted_problem()
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, gpu.PLANTED["C"], prior_precision=0.01, cut_precision=0.01, engine=ref.RestatementEngine())
    mean, cov, fit = gpu.planted_fit(gsmvi_amd, tgt, _lbfgs_engine(), OracleBatchedEngine())
    err = np.abs(tgt.cutpoints(mean) - cuts).max()
    sd = np.sqrt(np.diagonal(cov, axis1=1, axis2=2))[:, gpu.PLANTED["P"]:].max()
    print(f"planted cutpoints on the restatement: worst |fitted - planted| {err:.4f}, largest sd of delta {sd:.3f}, "
          f"reverts {int(fit.n_reverts.sum())}")
    assert np.isfinite(mean).all() and int(fit.n_reverts.sum()) == 0
    assert err <= 0.27 and 1.5 * err <= gpu.PLANTED_TOL
