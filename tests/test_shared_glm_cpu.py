"""The shared-design GLM target without a GPU: the numpy restatement (tests/shared_glm_ref.py) pinned to the per-problem
restatement on the replicated design, to duplicated rows and to a central difference; the C ABI declaration and argument checks of
gsmvi_glm_shared_batched_f64; its LDS budget; and the host logic of SharedDesignGLMTarget on a stand-in engine."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import glm_batched_ref as gref
import shared_glm_ref as ref
from gsmvi_amd import _lib
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsmvi_glm_shared_batched_f64"
DEBUG = "gsmvi_debug_glm_shared_batched_lds"
CASES = [(3, 1, 1, 1), (5, 33, 17, 3), (3, 70, 64, 5)]


# ---- 1. the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("K,N,D,rows", CASES)
def test_restatement_without_weights_is_the_per_problem_restatement_on_the_replicated_design(family, K, N, D, rows):
    """bit for bit, with and without an offset, per-problem and scalar precisions"""
    A, y, o, _, lam, tau, X = ref.make_inputs(family, K, N, D, rows)
    for off, l, t in ((o, lam, tau), (None, 0.7, 1.3 if family == "gaussian" else 1.0)):
        G, lp = ref.score_and_lp(family, A, y, off, None, l, t, X)
        Gr, lpr = gref.score_and_lp(family, ref.replicate(A, K), y, off, None, l, t, X)
        assert np.isfinite(G).all() and np.isfinite(lp).all()
        assert np.array_equal(G, Gr) and np.array_equal(lp, lpr)


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_restatement_with_prefix_weights_is_counts(family):
    """0/1 weights that form a prefix are ``counts``, bit for bit, whatever the removed observations hold"""
    K, N, D, rows = 4, 40, 7, 3
    A, y, o, _, lam, tau, X = ref.make_inputs(family, K, N, D, rows)
    counts = np.array([N, 1, 17, 0], dtype=np.int32)
    w = (np.arange(N)[None, :] < counts[:, None]).astype(np.float64)
    y2, o2 = y.copy(), o.copy()
    y2[w == 0.0], o2[w == 0.0] = np.nan, np.inf
    G, lp = ref.score_and_lp(family, A, y2, o2, w, lam, tau, X)
    Gr, lpr = gref.score_and_lp(family, ref.replicate(A, K), y, o, counts, lam, tau, X)
    assert np.isfinite(G).all() and np.array_equal(G, Gr) and np.array_equal(lp, lpr)


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_restatement_with_integer_weights_is_duplicated_rows(family):
    """a weight of m is the observation written m times: 1e-13 in rel_err per problem (the two sums differ in order only)"""
    K, N, D, rows = 3, 25, 6, 4
    A, y, o, _, lam, tau, X = ref.make_inputs(family, K, N, D, rows)
    rs = np.random.RandomState(5)
    w = rs.randint(0, 4, size=(K, N)).astype(np.float64)
    Nd = int(w.sum(1).max())
    Ad, yd, od = np.zeros((K, Nd, D)), np.zeros((K, Nd)), np.zeros((K, Nd))
    counts = w.sum(1).astype(np.int32)
    for k in range(K):
        idx = np.repeat(np.arange(N), w[k].astype(int))
        Ad[k, :len(idx)], yd[k, :len(idx)], od[k, :len(idx)] = A[idx], y[k, idx], o[k, idx]
    G, lp = ref.score_and_lp(family, A, y, o, w, lam, tau, X)
    Gr, lpr = gref.score_and_lp(family, Ad, yd, od, counts, lam, tau, X)
    for k in range(K):
        eg, el = rel_err(G[k], Gr[k]), rel_err(lp[k], lpr[k])
        print(f"{family} k={k}: integer weights against duplicated rows: G {eg:.2e} lp {el:.2e}")
        assert eg <= 1e-13 and el <= 1e-13, (k, eg, el)


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_restatement_gradient_is_a_central_difference_of_its_lp(family):
    """h = 1e-5 at |x| ~ 1: truncation h^2 |lp'''| / 6 ~ 1e-10 and rounding eps |lp| / h ~ 1e-9 of lp ~ 50, against gradients of
    size >= 1: 1e-6 relative to the largest gradient entry of the problem"""
    K, N, D, rows = 3, 30, 5, 2
    A, y, o, w, lam, tau, X = ref.make_inputs(family, K, N, D, rows, poison=True)
    G, _ = ref.score_and_lp(family, A, y, o, w, lam, tau, X)
    h = 1e-5
    num = np.empty_like(G)
    for j in range(D):
        e = np.zeros(D)
        e[j] = h
        num[:, :, j] = (ref.score_and_lp(family, A, y, o, w, lam, tau, X + e)[1]
                        - ref.score_and_lp(family, A, y, o, w, lam, tau, X - e)[1]) / (2 * h)
    for k in range(K):
        assert rel_err(num[k], G[k]) <= 1e-6, (k, rel_err(num[k], G[k]))


def test_restatement_nan_rules_and_zero_weights():
    """a non-finite row of X is NaN alone; poisson: exp(eta) overflowing at a weighted observation flags its row alone, at an
    observation of weight 0 it changes nothing"""
    for family in ref.FAMILIES:
        A, y, o, w, lam, tau, X = ref.make_inputs(family, 3, 20, 4, 5, poison=True)
        a = ref.score_and_lp(family, A, y, o, w, lam, tau, X)
        assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
        X2 = X.copy()
        X2[1, 2, 3] = np.inf
        c = ref.score_and_lp(family, A, y, o, w, lam, tau, X2)
        keep = np.ones(X.shape[:2], dtype=bool)
        keep[1, 2] = False
        assert np.isnan(c[0][1, 2]).all() and np.isnan(c[1][1, 2])
        assert np.array_equal(c[0][keep], a[0][keep]) and np.array_equal(c[1][keep], a[1][keep])
    A, y, o, w, lam, tau, X = ref.make_inputs("poisson", 3, 20, 4, 5)
    a = ref.score_and_lp("poisson", A, y, o, w, lam, tau, X)
    keep = np.ones(X.shape[:2], dtype=bool)
    keep[2, 1] = False
    ax = np.where(w[2] > 0.0, A @ X[2, 1], 0.0)
    X2 = X.copy()
    X2[2, 1] *= 800.0 / ax[np.argmax(np.abs(ax))]                      # the largest weighted a_n . x becomes + 800
    c = ref.score_and_lp("poisson", A, y, o, w, lam, tau, X2)
    assert np.isnan(c[0][2, 1]).all() and np.isnan(c[1][2, 1])
    assert np.array_equal(c[0][keep], a[0][keep]) and np.array_equal(c[1][keep], a[1][keep])
    n = int(np.flatnonzero(w[2] > 0.0)[0])
    o2, w0 = o.copy(), w.copy()
    o2[2, n], w0[2, n] = 900.0, 0.0                                    # every row of problem 2 overflows at observation n
    c = ref.score_and_lp("poisson", A, y, o2, w, lam, tau, X)
    assert np.isnan(c[0][2]).all() and np.isnan(c[1][2]).all()
    assert np.array_equal(c[0][:2], a[0][:2]) and np.array_equal(c[1][:2], a[1][:2])
    c = ref.score_and_lp("poisson", A, y, o2, w0, lam, tau, X)         # ... unless its weight is 0
    b = ref.score_and_lp("poisson", A, y, o, w0, lam, tau, X)
    assert np.array_equal(c[0], b[0]) and np.array_equal(c[1], b[1]) and np.isfinite(c[0]).all()


# ---- 2. the C ABI --------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr)
    for mp in ("exports.map", "exports_debug.map"):
        assert re.search(r"^\s*" + NAME + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), mp
    assert NAME in _lib.exported_symbols() and NAME in built
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.GLM_FAMILIES == {"logistic": 0, "poisson": 1, "probit": 2, "gaussian": 3}
    head = hdr.split("#ifndef GSMVI_HIP_H")[0]                        # the reference map names it and the callable it replaces
    assert NAME in head and head.count("example_gsm.py:34-35") >= 3
    block = hdr[:hdr.index("int " + NAME)].rsplit("/*", 1)[1]           # its own doc block cites the callable too
    assert "example_gsm.py:34-35" in block and "GSMVI_PATH_BATCHED_TARGET" in block
    # the ctypes signature is the declaration's: 18 arguments, family an int after N, weights where the sibling has counts
    res, args = _lib._SIGS[NAME]
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert res is C.c_int and len(args) == len(params) == 18
    for p, a in zip(params, args):
        want = C.c_double if p.startswith("double ") else C.c_int64 if p.startswith("int64_t") else \
            C.c_int if p.startswith("int ") else C.c_void_p
        assert a is want, (p, a)
    assert params[6] == "int family" and params[10] == "const double* weights"
    # the debug query: the debug header, the debug map and the debug library only
    dhdr = open(os.path.join(ROOT, "include", "gsmvi_hip_debug.h")).read()
    assert re.search(r"\bint\s+" + DEBUG + r"\s*\(", dhdr) and DEBUG not in hdr
    assert DEBUG in open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "exports_debug.map")).read()
    assert DEBUG not in open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "exports.map")).read()
    dbg = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path(debug=True)], check=True, capture_output=True,
                         text=True).stdout
    assert DEBUG in dbg and NAME in dbg and DEBUG not in out
    assert DEBUG in _lib._DEBUG_SIGS and DEBUG not in _lib._SIGS


def test_no_path_bit_is_added():
    """all 32 bits are taken: the launch reports the batched target's"""
    from gsmvi_amd.engine import HipEngine
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    bits = re.findall(r"#define\s+(GSMVI_PATH_\w+)\s+(0x[0-9a-fA-F]+)u", hdr)
    assert len(bits) == 32 and sorted(int(v, 16) for _, v in bits) == [1 << i for i in range(32)]
    assert len(HipEngine.PATH_BITS) == 32 and "batched_target" in set(HipEngine.PATH_BITS.values()) | set(HipEngine.PATH_BITS)
    src = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_glm_shared_batched.hip")).read()
    assert re.findall(r"GSMVI_PATH_\w+", src) == ["GSMVI_PATH_BATCHED_TARGET"]


# ---- 3. argument checks ----------------------------------------------------------------------------------------------------
def test_abi_checks_arguments_before_the_context_and_names_overlapping_arrays():
    """every bad argument is reported with a NULL context (no device work can have started); valid ones end at the context"""
    lib = _lib.load_library()
    buf = (C.c_double * 8192)()
    p = C.cast(buf, C.c_void_p).value
    a = lambda n: p + 8 * 512 * n                                   # noqa: E731  sixteen disjoint 4 KB arrays
    err = lambda: (lib.gsmvi_last_error() or b"").decode()           # noqa: E731

    def call(K=2, D=4, nc=3, N=5, family=1, A=a(0), y=a(1), offset=a(7), weights=a(2), tau=1.0, tau_dev=None, lam=1.0,
             lam_dev=None, X=a(3), G=a(4), lp=a(5)):
        return lib.gsmvi_glm_shared_batched_f64(None, None, K, D, nc, N, family, A, y, offset, weights, tau, tau_dev, lam, lam_dev,
                                                X, G, lp)

    def bad(what, **kw):
        assert call(**kw) == 1 and what in err() and err().startswith(NAME + ":"), (what, kw, err())

    bad("D must be", D=0)
    bad("D must be", D=65)
    bad("K must be", K=0)
    bad("K must be", K=2 ** 27)
    bad("nc must be", nc=0)
    bad("N must be", N=0)
    bad("too large", K=2 ** 20, N=2 ** 40)
    bad("K nc D is too large", K=2 ** 24 - 1, nc=2 ** 31 - 1, D=64)
    bad("K nc is too large", K=2 ** 26 - 4, nc=2 ** 31 - 1, D=1)
    for fam in (-1, 4, 100):
        bad("family", family=fam)
    for name in ("A", "y", "X"):
        bad("NULL array", **{name: None})
    bad("G or lp", G=None, lp=None)
    for v in (-1.0, float("nan"), float("inf")):
        bad("prior_prec", lam=v)
    # the noise precision belongs to the gaussian family
    for fam in (0, 1, 2):
        bad("noise_prec", family=fam, tau=2.0)
        bad("noise_prec", family=fam, tau_dev=a(8))
        bad("noise_prec", family=fam, tau=float("nan"))
    for v in (0.0, -1.0, float("nan"), float("inf")):
        bad("noise_prec", family=3, tau=v)
    # a written array overlapping any other array, at both ends; the message names both
    for name, other in (("A", a(0)), ("y", a(1)), ("weights", a(2)), ("X", a(3)), ("offset", a(7))):
        bad(f"G overlaps {name}", G=other)
        bad(f"lp overlaps {name}", lp=other)
    bad("G overlaps prior_prec_dev", lam_dev=a(6), G=a(6))
    bad("lp overlaps prior_prec_dev", lam_dev=a(6), lp=a(6))
    bad("G overlaps noise_prec_dev", family=3, tau_dev=a(8), G=a(8))
    bad("lp overlaps noise_prec_dev", family=3, tau_dev=a(8), lp=a(8))
    bad("lp overlaps G", lp=a(4))
    bad("G overlaps X", G=a(3) + 8 * (2 * 3 * 4 - 1))                   # the last element of X
    bad("G overlaps A", G=a(0) + 8 * (5 * 4 - 1))                       # the last element of the shared A: N D doubles, not K N D
    bad("G overlaps weights", G=a(2) + 8 * (2 * 5 - 1))                 # the last element of the weights
    bad("lp overlaps offset", lp=a(7) + 8 * (2 * 5 - 1))
    # adjacent is not overlapping, and valid calls end at the context
    bad("ctx is NULL", G=a(0) + 8 * 5 * 4)
    bad("ctx is NULL", G=a(2) + 8 * 2 * 5)
    bad("ctx is NULL", G=a(3) + 8 * 2 * 3 * 4)
    for fam in (0, 1, 2, 3):
        bad("ctx is NULL", family=fam)
        bad("ctx is NULL", family=fam, offset=None, weights=None, G=None)
        bad("ctx is NULL", family=fam, lp=None, lam=0.0)
    bad("ctx is NULL", family=3, tau=2.5)
    bad("ctx is NULL", family=3, tau=-1.0, tau_dev=a(8))                # the scalar is unused with K values
    bad("ctx is NULL", lam=-1.0, lam_dev=a(6))
    bad("ctx is NULL", y=a(0), X=a(0), weights=a(0), lam_dev=a(0), offset=a(0))     # read-only arrays may overlap
    # the sibling still reports under its own name
    assert lib.gsmvi_glm_batched_f64(None, None, 2, 0, 3, 5, 1, a(0), a(1), None, None, 1.0, None, 1.0, None, a(3), a(4), a(5)) == 1
    assert err().startswith("gsmvi_glm_batched_f64:") and "D must be" in err()


# ---- 4. LDS budget -------------------------------------------------------------------------------------------------------
def test_lds_budget_stays_below_the_default_limit():
    """the dynamic LDS a launch requests (the library's own host arithmetic, through the debug build's query in a child process):
    one tile of A, 32 x (16 ceil(D / 16) + 1) doubles, whatever want and the family; 64 rows of X per workgroup; never above the
    64 KiB a kernel gets without asking; status 1 outside the ranges"""
    import json
    import sys
    code = (
        "import ctypes as C, json, sys\n"
        "lib = C.CDLL(sys.argv[1])\n"
        f"f = lib.{DEBUG}\n"
        "f.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]\n"
        "out = {}\n"
        "for D in range(-1, 67):\n"
        "    for want in (0, 1, 2, 3, 4):\n"
        "        for fam in (-1, 0, 1, 2, 3, 4):\n"
        "            n, p = C.c_size_t(0), C.c_int(0)\n"
        "            st = f(D, want, fam, C.byref(n), C.byref(p))\n"
        "            out[f'{D},{want},{fam}'] = [st, n.value, p.value]\n"
        "out['null'] = [f(4, 1, 0, None, None), 0, 0]\n"
        "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.library_path(debug=True)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got.pop("null")[0] == 1
    seen = 0
    for key, (st, n, rows) in got.items():
        D, want, fam = (int(x) for x in key.split(","))
        if not (1 <= D <= 64 and 1 <= want <= 3 and 0 <= fam <= 3):
            assert st == 1, key
            continue
        seen += 1
        assert st == 0 and rows == 64, key
        assert n == 8 * 32 * (16 * ((D + 15) // 16) + 1) <= 64 * 1024, (key, n)
    assert seen == 64 * 3 * 4 and got["64,3,2"][1] == 16640


# ---- 5. host logic of SharedDesignGLMTarget --------------------------------------------------------------------------------
def test_target_validates_on_the_host_before_the_engine_is_touched():
    from gsmvi_amd import SharedDesignGLMTarget
    eng = ref.RestatementEngine()

    def bad(match, family="poisson", **kw):
        A, y, o, w, lam, tau, X = ref.make_inputs(family, 3, 12, 4, 2)
        base = dict(A=A, y=y, family=family, prior_precision=lam, offset=o, weights=w, engine=eng)
        if family == "gaussian":
            base["noise_precision"] = tau
        for k, v in kw.items():
            base[k] = v(base[k]) if callable(v) else v
        eng.calls.clear()
        with pytest.raises(ValueError, match=match):
            SharedDesignGLMTarget(**base)
        assert eng.calls == [], (match, kw)

    def put(k, n, v):
        def f(arr):
            arr = np.array(arr, dtype=np.float64)
            arr[k, n] = v
            return arr
        return f

    A, y, o, w, lam, tau, X = ref.make_inputs("poisson", 3, 12, 4, 2)
    live = int(np.flatnonzero(w[1] > 0.0)[0])                          # an observation of problem 1 that counts
    dead = int(np.flatnonzero(w[2] == 0.0)[0])                         # and one of problem 2 that does not
    for fam in ("binomial", "Poisson", None, 1):
        with pytest.raises(ValueError, match="^family:"):
            SharedDesignGLMTarget(A, y, fam, engine=eng)
    assert eng.calls == []
    bad("^A:", A=lambda A: A[0])
    bad("^A:", A=lambda A: A[None])                                    # a per-problem design is the other target's
    bad("^A:", A=lambda A: A[:, :0])
    bad("^A: D = 65", A=np.zeros((12, 65)))
    bad("^y:", y=lambda y: y[:, :11])
    bad("^y:", y=lambda y: y[0])
    bad("^y:", y=lambda y: y[:0])
    for fam, values in (("logistic", (-0.01, 1.01, np.nan, np.inf)), ("probit", (-0.01, 1.01, np.nan, -np.inf)),
                        ("poisson", (-0.5, np.nan, np.inf)), ("gaussian", (np.nan, np.inf, -np.inf))):
        for v in values:
            bad(r"^y: .*\[1\]", family=fam, y=put(1, live, v))
    bad("^weights:", weights=lambda w: w[:, :11])
    bad("^weights:", weights=lambda w: w[0])
    bad("^weights:", weights=lambda w: w[:2])
    for v in (-0.5, np.nan, np.inf, -np.inf):
        bad(r"^weights: .*\[1\]", weights=put(1, 3, v))
    bad("^offset:", offset=lambda o: o[:, :11])
    bad("^offset:", offset=lambda o: o[0])
    bad("^offset:", offset=lambda o: o.T)
    for v in (np.nan, np.inf, -np.inf):
        bad(r"^offset: .*\[1\]", offset=put(1, live, v))
    for badl in (-0.5, np.nan, np.inf, [0.1, 0.2], [0.1, -0.2, 0.3], [0.1, np.nan, 0.3]):
        bad("^prior_precision:", prior_precision=badl)
    for fam in ("logistic", "poisson", "probit"):
        for t in (2.0, [1.0, 1.0, 2.0], np.nan):
            bad("^noise_precision:", family=fam, noise_precision=t)
    for t in (0.0, -1.0, np.nan, np.inf, [1.0, 2.0], [1.0, 0.0, 2.0], [1.0, np.nan, 2.0]):
        bad("^noise_precision:", family="gaussian", noise_precision=t)
    bad(r"^noise_precision: .*\[1\]", family="gaussian", noise_precision=[1.0, 0.0, 2.0])
    # where the weight is 0 anything goes in y and the offset ...
    for fam in ref.FAMILIES:
        A, y, o, w, lam, tau, X = ref.make_inputs(fam, 3, 12, 4, 2, poison=True)
        assert np.isnan(y[w == 0.0]).all() and np.isinf(o[w == 0.0]).all() and (w == 0.0).any(1).all()
        t = SharedDesignGLMTarget(A, y, fam, lam, o, w, noise_precision=tau, engine=eng)
        assert np.isfinite(t.lp_g(X)).all()
        with pytest.raises(ValueError, match=r"^y: .*\[0, 1, 2\]"):
            SharedDesignGLMTarget(A, y, fam, lam, None, None, noise_precision=tau, engine=eng)     # ... unless every one counts
    A, y, o, w, lam, tau, X = ref.make_inputs("poisson", 3, 12, 4, 2)
    SharedDesignGLMTarget(A, put(2, dead, -3.0)(y), "poisson", lam, put(2, dead, np.nan)(o), w, engine=eng)


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_target_protocol_on_the_restatement_engine(family):
    from gsmvi_amd import BatchedGLMTarget, SharedDesignGLMTarget
    K, N, D, rows = 3, 12, 4, 5
    A, y, o, w, lam, tau, X = ref.make_inputs(family, K, N, D, rows, poison=True)
    G, lp = ref.score_and_lp(family, A, y, o, w, lam, tau, X)
    eng = ref.RestatementEngine()
    tgt = SharedDesignGLMTarget(A, y, family, lam, o, w, noise_precision=tau, engine=eng)
    assert not isinstance(tgt, BatchedGLMTarget)
    assert not any(hasattr(tgt, name) for name in ("neg_hessian", "predict", "loo", "counts"))
    assert (tgt.K, tgt.N, tgt.D, tgt.family) == (K, N, D, family)
    assert tgt.lp_g.device_native is True and tgt.lp_g.graph_safe is True
    assert tgt.A.shape == (N, D) and all(t.dtype == np.float64 for t in (tgt.A, tgt.y, tgt.offset, tgt.weights))
    assert np.array_equal(tgt.lp_g(X), G)
    # exactly the arrays it was given: the one A, and y and the offset as they are where the weight is 0 (NaN, inf)
    assert eng.last["A"] is tgt.A and eng.last["y"] is tgt.y and eng.last["offset"] is tgt.offset and eng.last["weights"] is tgt.weights
    assert np.array_equal(tgt.A, A) and np.array_equal(tgt.y, y, equal_nan=True) and np.array_equal(tgt.offset, o)
    assert np.array_equal(tgt.weights, w) and np.array_equal(eng.last["prior_prec"], lam)
    out = np.empty_like(X)
    assert tgt.lp_g(X, out=out) is out and np.array_equal(out, G)
    v = tgt.lp(X)
    assert v.shape == (K, rows) and np.array_equal(v, lp)
    g2, v2 = tgt.lp_and_score(X)
    assert np.array_equal(g2, G) and np.array_equal(v2, lp)
    assert [c for c in eng.calls if isinstance(c, tuple)] == [("glm_shared", family, "g", False), ("glm_shared", family, "g", True),
                                                              ("glm_shared", family, "lp", False),
                                                              ("glm_shared", family, "both", False)]
    # tensors in, scalar precisions, no weights, no offset, float32 design
    A2, y2, _, _, _, _, _ = ref.make_inputs(family, K, N, D, rows)
    t = SharedDesignGLMTarget(torch.tensor(A2, dtype=torch.float32), torch.tensor(y2), family, 0.5, engine=eng,
                              noise_precision=2.0 if family == "gaussian" else 1.0)
    Gs, lps = ref.score_and_lp(family, A2.astype(np.float32), y2, None, None, 0.5, 2.0 if family == "gaussian" else 1.0, X)
    assert t.weights is None and t.offset is None and t.prior_precision == 0.5 and isinstance(t.noise_precision, float)
    assert np.array_equal(t.lp_g(torch.tensor(X)), Gs) and np.array_equal(t.lp(torch.tensor(X)), lps)
    from gsmvi_amd.monitors import lp_sums
    s = lp_sums(tgt.lp, X, eng, K)
    assert s.shape == (K,) and rel_err(s, lp.sum(1)) < 1e-15


def test_the_fits_and_psis_accept_the_target():
    """GSMBatch, ADVIBatch and psis_batched on their stand-in engines, scored by the target on the restatement: the shapes of lp
    and lp_g are the ones they take, and the results are those of the same runs scored by plain callables"""
    import gsmvi_amd
    import psis_batched_ref as pref
    from engines import OracleBatchedEngine
    from test_advi_batched_cpu import OracleBatchedADVIEngine
    K, N, D, B, niter = 3, 30, 4, 3, 5
    A, y, o, w, lam, tau, _ = ref.make_inputs("logistic", K, N, D, 1)
    lam = lam + 0.5
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, "logistic", lam, o, w, engine=ref.RestatementEngine())
    lp_h = lambda X: ref.score_and_lp("logistic", A, y, o, w, lam, tau, X)[1]   # noqa: E731
    lpg_h = lambda X: ref.score_and_lp("logistic", A, y, o, w, lam, tau, X)[0]  # noqa: E731
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
    # what needs a Hessian or the pointwise likelihood refuses the target with its own message
    with pytest.raises(TypeError):
        gsmvi_amd.laplace_init_batched(tgt)
    with pytest.raises(TypeError):
        gsmvi_amd.psis_loo_batched(tgt, mean, cov, keys)
