"""The batched softmax target without a GPU: the numpy restatement (tests/softmax_batched_ref.py) pinned to torch autograd of
the written density, to the logistic restatement at C = 2 and to its own longdouble form over the GPU grid; the C ABI declaration
and argument checks of gsmvi_softmax_batched_f64; the LDS budget and the X-tile rule; and the host logic of BatchedSoftmaxTarget
on a stand-in engine."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import logistic_batched_ref as lref
import softmax_batched_ref as ref
from gsmvi_amd import _lib
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsmvi_softmax_batched_f64"
CASES = [(3, 1, 2, 1, 1, 1), (5, 33, 3, 8, 33, 1), (3, 100, 5, 16, 9, 1), (3, 70, 65, 1, 5, 6), (3, 40, 4, 7, 5, 3)]


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------
def _autograd(A, y, n, lam, X, Cc):
    """one problem: lp (rows,) and d sum(lp) / d X by CPU torch, float64, the density as the header writes it"""
    At, yt = torch.tensor(A[:n]), torch.tensor(y[:n].astype(np.int64))
    x = torch.tensor(X, requires_grad=True)
    rows, P = X.shape[0], A.shape[1]
    eta = torch.einsum("np,rcp->rnc", At, x.reshape(rows, Cc - 1, P))
    eta = torch.cat([eta, torch.zeros(rows, n, 1, dtype=torch.float64)], dim=2)
    m = eta.max(dim=2, keepdim=True).values
    terms = torch.gather(eta, 2, yt[None, :, None].expand(rows, n, 1))[:, :, 0] - m[:, :, 0] - torch.log(torch.exp(eta - m).sum(2))
    lp = terms.sum(1) - 0.5 * lam * (x * x).sum(1)
    (g,) = torch.autograd.grad(lp.sum(), x)
    return g.numpy(), lp.detach().numpy()


@pytest.mark.parametrize("K,N,Cc,P,rows,scale", CASES)
def test_restatement_is_autograd_of_the_written_density(K, N, Cc, P, rows, scale):
    """1e-12 per problem"""
    A, y, counts, lam, X = ref.make_inputs(K, N, Cc, P, rows, scale)
    G, lp = ref.score_and_lp(A, y, Cc, counts, lam, X)
    assert np.isfinite(G).all() and np.isfinite(lp).all()
    worst = 0.0
    for k in range(K):
        g_t, lp_t = _autograd(A[k], y[k], int(counts[k]), float(lam[k]), X[k], Cc)
        eg, el = rel_err(G[k], g_t), rel_err(lp[k], lp_t)
        worst = max(worst, eg, el)
        assert eg <= 1e-12 and el <= 1e-12, (k, eg, el)
    print(f"K={K} N={N} C={Cc} P={P} rows={rows} scale={scale}: worst rel_err {worst:.2e}, max|eta| {ref.max_abs_eta(A, counts, X, Cc):.1f}")


@pytest.mark.parametrize("K,N,P,rows", [(9, 70, 10, 40), (9, 70, 33, 40), (3, 5, 1, 4)])
def test_two_classes_are_the_logistic_restatement(K, N, P, rows):
    """C = 2 with y = [label = 0] is the logistic model: 1e-13 per problem"""
    A, y, counts, lam, X = ref.make_inputs(K, N, 2, P, rows)
    G, lp = ref.score_and_lp(A, y, 2, counts, lam, X)
    Gl, lpl = lref.score_and_lp(A, (y == 0).astype(np.float64), counts, lam, X)
    worst = max(max(rel_err(G[k], Gl[k]), rel_err(lp[k], lpl[k])) for k in range(K))
    print(f"C=2 K={K} N={N} P={P}: worst rel_err against the logistic restatement {worst:.2e}")
    assert worst <= 1e-13


def test_float64_restatement_is_the_longdouble_one_over_the_gpu_grid():
    """every shape of the GPU grid (K = 5, N x nc, the (C, P) list) and the two large-eta inputs: float64 within 1e-13 of
    np.longdouble per problem, which keeps the device bar of 1e-11 sharp"""
    worst = 0.0
    for (Cc, P) in ref.SHAPES:
        for N in ref.NS:
            A, y, counts, lam, X = ref.make_inputs(5, N, Cc, P, max(ref.nc_grid(Cc, P)))
            G, lp = ref.score_and_lp(A, y, Cc, counts, lam, X)
            Gl, lpl = ref.score_and_lp(A, y, Cc, counts, lam, X, dtype=np.longdouble)
            assert Gl.dtype == np.longdouble and lpl.dtype == np.longdouble
            for k in range(5):
                e = max(rel_err(G[k], Gl[k]), rel_err(lp[k], lpl[k]))
                worst = max(worst, e)
                assert e <= 1e-13, (Cc, P, N, k, e)
    print(f"grid: worst float64 - longdouble rel_err {worst:.2e}")
    for args, eta_min in (((2, 64, 3, 32, 8, 10), 250.0), ((2, 100, 5, 16, 4, 40), 800.0)):
        A, y, counts, lam, X = ref.make_inputs(*args)
        eta = ref.max_abs_eta(A, counts, X, args[2])
        assert eta > eta_min, eta
        G, lp = ref.score_and_lp(A, y, args[2], counts, lam, X)
        Gl, lpl = ref.score_and_lp(A, y, args[2], counts, lam, X, dtype=np.longdouble)
        assert np.isfinite(G).all() and np.isfinite(lp).all()
        e = max(max(rel_err(G[k], Gl[k]), rel_err(lp[k], lpl[k])) for k in range(args[0]))
        print(f"{args}: max|eta| {eta:.0f}, float64 - longdouble rel_err {e:.2e}")
        assert e <= 1e-13


def test_restatement_nan_rules_and_counts():
    """counts = None is all N rows, a scalar precision is K equal values, rows beyond counts play no part, a non-finite row of X
    or a non-finite eta is NaN alone, counts = 0 leaves the prior"""
    A, y, counts, lam, X = ref.make_inputs(3, 20, 4, 3, 5)
    full = np.full(3, 20, dtype=np.int32)
    a, b = ref.score_and_lp(A, y, 4, None, 0.7, X), ref.score_and_lp(A, y, 4, full, np.full(3, 0.7), X)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    A2, y2 = A.copy(), y.copy()
    for k in range(3):
        A2[k, counts[k]:] = np.nan
        y2[k, counts[k]:] = 77
    a, b = ref.score_and_lp(A, y, 4, counts, lam, X), ref.score_and_lp(A2, y2, 4, counts, lam, X)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    keep = np.ones(X.shape[:2], dtype=bool)
    keep[1, 2] = False
    X2 = X.copy()
    X2[1, 2, 3] = np.inf
    c = ref.score_and_lp(A, y, 4, counts, lam, X2)
    assert np.isnan(c[0][1, 2]).all() and np.isnan(c[1][1, 2])
    assert np.array_equal(c[0][keep], a[0][keep]) and np.array_equal(c[1][keep], a[1][keep])
    A3, X3 = A.copy(), X.copy()
    A3[1, 0], X3[1, 2] = 4.0, 1e308                                    # finite entries, an eta that is not
    a3, c = ref.score_and_lp(A3, y, 4, counts, lam, X), ref.score_and_lp(A3, y, 4, counts, lam, X3)
    assert np.isfinite(X3).all() and np.isfinite(a3[0]).all() and np.isnan(c[0][1, 2]).all() and np.isnan(c[1][1, 2])
    assert np.array_equal(c[0][keep], a3[0][keep]) and np.array_equal(c[1][keep], a3[1][keep])
    z = ref.score_and_lp(A, y, 4, np.zeros(3, dtype=np.int32), lam, X)
    assert np.array_equal(z[0], -lam[:, None, None] * X) and np.array_equal(z[1], -0.5 * lam[:, None] * (X * X).sum(2))


# ---- 2. the C ABI ----------------------------------------------------------------------------------------------------------
def test_softmax_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr)
    for mp in ("exports.map", "exports_debug.map"):
        assert re.search(r"^\s*" + NAME + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), mp
    assert NAME in _lib.exported_symbols() and NAME in built
    head = hdr.split("#ifndef GSMVI_HIP_H")[0]
    assert NAME in head
    block = hdr[:hdr.index("int " + NAME)].rsplit("/*", 1)[1]           # the definition is written above the entry point
    for line in ("eta_nc = a_n . w_c  (c < C-1),   eta_n,C-1 = 0",
                 "m_n    = max_c eta_nc            (over all C values, the 0 included)",
                 "s_n    = sum_{c=0..C-1} exp(eta_nc - m_n)     (class order; the reference class last)",
                 "lp(x)  = sum_{n<n_k} [ eta_n,y_n - m_n - log s_n ] - lam_k |x|^2 / 2",
                 "g_cj   = sum_{n<n_k} ( [y_n = c] - exp(eta_nc - m_n)/s_n ) a_nj - lam_k x_cj      (c < C-1)"):
        assert line in block, line
    assert "example_gsm.py:34-35" in block and "GSMVI_PATH_BATCHED_SOFTMAX" in block
    # the ctypes signature is the declaration's: 15 arguments
    res, args = _lib._SIGS[NAME]
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert res is C.c_int and len(args) == len(params) == 15
    for p, a in zip(params, args):
        want = C.c_double if p.startswith("double ") else C.c_int64 if p.startswith("int64_t") else \
            C.c_int if p.startswith("int ") else C.c_void_p
        assert a is want, (p, a)
    assert params[3:7] == ["int C", "int P", "int nc", "int64_t N"] and params[8] == "const int* labels"
    dbg = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path(debug=True)], check=True, capture_output=True,
                         text=True).stdout
    assert "gsmvi_debug_softmax_batched_lds" in dbg and "gsmvi_debug_softmax_batched_lds" not in out
    assert re.search(r"#define\s+GSMVI_ABI_VERSION\s+1\b", hdr)


def test_softmax_path_bit():
    from gsmvi_amd.engine import HipEngine
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_SOFTMAX\s+0x1000000u", hdr)
    mask = re.search(r"#define\s+GSMVI_PATH_GENERIC_MASK\s+\(([^)]*)\)", hdr).group(1)
    bits = 0
    for tok in re.findall(r"0x[0-9a-fA-F]+", mask):
        bits |= int(tok, 16)
    assert bits == HipEngine.PATH_GENERIC_MASK and not bits & 0x1000000
    assert HipEngine.PATH_BITS["batched_softmax"] == 0x1000000 and not HipEngine.PATH_GENERIC_MASK & 0x1000000
    assert len(set(HipEngine.PATH_BITS.values())) == len(HipEngine.PATH_BITS)


def test_abi_checks_arguments_before_the_context_and_names_overlapping_arrays():
    """every bad argument is reported with a NULL context (no device work can have started); valid ones end at the context"""
    lib = _lib.load_library()
    buf = (C.c_double * 8192)()
    p = C.cast(buf, C.c_void_p).value
    a = lambda n: p + 8 * 512 * n                                   # noqa: E731  sixteen disjoint 4 KB arrays
    err = lambda: (lib.gsmvi_last_error() or b"").decode()           # noqa: E731

    def call(K=2, Cc=3, P=2, nc=3, N=5, A=a(0), labels=a(1), counts=a(2), lam=1.0, lam_dev=None, X=a(3), G=a(4), lp=a(5)):
        return lib.gsmvi_softmax_batched_f64(None, None, K, Cc, P, nc, N, A, labels, counts, lam, lam_dev, X, G, lp)

    # shapes: C >= 2, P >= 1, (C - 1) P in 1 .. 64
    for bad in (1, 0, -1, -2 ** 31):
        assert call(Cc=bad) == 1 and "C must be" in err() and NAME in err(), bad
    for cc, pp in ((3, 0), (3, -1), (3, 33), (2, 65), (66, 1), (65, 2), (2 ** 31 - 1, 1), (3, 2 ** 31 - 1), (2 ** 16 + 1, 2 ** 16)):
        assert call(Cc=cc, P=pp) == 1 and "(C - 1) P" in err(), (cc, pp)
    assert call(K=0) == 1 and "K must be" in err()
    assert call(nc=0) == 1 and "nc must be" in err()
    assert call(N=0) == 1 and "N must be" in err()
    assert call(K=2 ** 20, N=2 ** 40) == 1 and "K N D is too large" in err()
    assert call(K=2 ** 24 - 1, Cc=2, P=64, nc=2 ** 31 - 1, N=1) == 1 and "K nc D is too large" in err()
    for name in ("A", "labels", "X"):
        assert call(**{name: None}) == 1 and "NULL array" in err(), name
    assert call(G=None, lp=None) == 1 and "G or lp" in err()
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(lam=bad) == 1 and "prior_prec" in err(), bad
    assert call(lam=-1.0, lam_dev=a(6)) == 1 and "ctx is NULL" in err()                  # the scalar is unused with K values
    # a written array overlapping any other array, at both ends; the message names both
    for name, other in (("A", a(0)), ("labels", a(1)), ("counts_dev", a(2)), ("X", a(3))):
        assert call(G=other) == 1 and f"G overlaps {name}" in err(), name
        assert call(lp=other) == 1 and f"lp overlaps {name}" in err(), name
    assert call(lam_dev=a(6), G=a(6)) == 1 and "G overlaps prior_prec_dev" in err()
    assert call(lam_dev=a(6), lp=a(6)) == 1 and "lp overlaps prior_prec_dev" in err()
    assert call(lp=a(4)) == 1 and "lp overlaps G" in err()
    nx, nA, nl = 2 * 3 * 4, 2 * 5 * 2, 2 * 5                          # elements of X / G, of A, of the labels
    assert call(G=a(3) + 8 * (nx - 1)) == 1 and "G overlaps X" in err()                  # the last element of X
    assert call(G=a(3) + 8 * nx) == 1 and "ctx is NULL" in err()                         # adjacent is not overlapping
    assert call(G=a(3) - 8 * (nx - 1)) == 1 and "G overlaps X" in err()                  # the last element of G on the first of X
    assert call(G=a(3) - 8 * nx) == 1 and "ctx is NULL" in err()
    assert call(lp=a(0) + 8 * (nA - 1)) == 1 and "lp overlaps A" in err()
    assert call(lp=a(0) + 8 * nA) == 1 and "ctx is NULL" in err()
    assert call(lp=a(1) + 4 * (nl - 1)) == 1 and "lp overlaps labels" in err()           # ints: the last label
    assert call(lp=a(1) + 4 * nl) == 1 and "ctx is NULL" in err()
    assert call(lp=a(2) + 4) == 1 and "lp overlaps counts_dev" in err()                  # K = 2 ints
    assert call(lp=a(2) + 8) == 1 and "ctx is NULL" in err()
    assert call(lp=a(5), G=a(5) + 8 * (2 * 3 - 1)) == 1 and "overlaps" in err()          # the last element of lp
    assert call(lp=a(5), G=a(5) + 8 * 2 * 3) == 1 and "ctx is NULL" in err()
    # valid calls end at the context
    for cc, pp in ref.SHAPES:
        assert call(K=1, Cc=cc, P=pp, nc=1, N=1) == 1 and "ctx is NULL" in err(), (cc, pp)
    assert call(counts=None, G=None) == 1 and "ctx is NULL" in err()
    assert call(lp=None, lam=0.0) == 1 and "ctx is NULL" in err()
    assert call(labels=a(0), X=a(0), counts=a(0), lam_dev=a(0)) == 1 and "ctx is NULL" in err()    # read-only arrays may overlap


# ---- 3. LDS budget and the X tile ------------------------------------------------------------------------------------------
def test_lds_budget_and_x_tile_over_every_shape():
    """the dynamic LDS a launch requests and its X tile (the library's own host arithmetic, through the debug build's query in a
    child process) for every (C, P) in bounds: the mirror of tests/softmax_batched_ref.py, never above the 64 KiB a kernel gets
    without asking, at least one row of X, at most 4 outputs per thread; out-of-bounds shapes are refused"""
    code = (
        "import ctypes as C, json, sys\n"
        "lib = C.CDLL(sys.argv[1])\n"
        "f = lib.gsmvi_debug_softmax_batched_lds\n"
        "f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]\n"
        "out = {}\n"
        "for Cc in range(0, 68):\n"
        "    for P in range(0, 67):\n"
        "        if Cc >= 2 and P >= 1 and (Cc - 1) * P > 64 and (Cc, P) not in ((66, 1), (2, 65), (3, 33), (67, 66)):\n"
        "            continue\n"
        "        for nc in (0, 1, 2, 100000):\n"
        "            for want in (0, 1, 2, 3, 4):\n"
        "                n, p, t = C.c_size_t(0), C.c_int(0), C.c_int(0)\n"
        "                st = f(Cc, P, nc, want, C.byref(n), C.byref(p), C.byref(t))\n"
        "                out[f'{Cc},{P},{nc},{want}'] = [st, n.value, p.value, t.value]\n"
        "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.library_path(debug=True)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    worst, seen = 0, set()
    for key, (st, n, p, t) in got.items():
        Cc, P, nc, want = (int(x) for x in key.split(","))
        if not (Cc >= 2 and P >= 1 and (Cc - 1) * P <= 64 and nc >= 1 and 1 <= want <= 3):
            assert st == 1, key
            continue
        D = (Cc - 1) * P
        ppw = 4 if D <= 16 else 1
        assert st == 0 and p == ppw and t == ref.x_tile(Cc, P), key
        assert 1 <= t <= (16 if ppw == 4 else 32) and t * D <= 4 * 256 // ppw, key
        assert n == 8 * ppw * ref.lds_doubles(Cc, P, min(nc, t), want) <= 64 * 1024, (key, n)
        worst = max(worst, n)
        seen.add((Cc, P))
    assert len(seen) == sum(1 for c in range(2, 66) for q in range(1, 65) if (c - 1) * q <= 64)
    assert min(ref.x_tile(c, q) for (c, q) in seen) == 3 == ref.x_tile(65, 1) == ref.x_tile(17, 1)
    assert 60 * 1024 < worst <= 64 * 1024
    for (Cc, P) in ref.SHAPES:                                          # the GPU grid reaches both sides of every tile
        assert {ref.x_tile(Cc, P), ref.x_tile(Cc, P) + 1} <= set(ref.nc_grid(Cc, P))


# ---- 4. host logic of BatchedSoftmaxTarget ---------------------------------------------------------------------------------
def test_target_validates_on_the_host_before_the_engine_is_touched():
    from gsmvi_amd import BatchedSoftmaxTarget
    eng = ref.RestatementEngine()

    def bad(match, **kw):
        A, y, counts, lam, X = ref.make_inputs(3, 12, 4, 3, 2)
        base = dict(A=A, y=y, num_classes=4, prior_precision=lam, counts=counts, engine=eng)
        for k, v in kw.items():
            base[k] = v(base[k]) if callable(v) else v
        eng.calls.clear()
        with pytest.raises(ValueError, match=match):
            BatchedSoftmaxTarget(**base)
        assert eng.calls == [], (match, kw)

    def put(k, n, v, dtype=np.float64):
        def f(arr):
            arr = np.array(arr, dtype=dtype)
            arr[k, n] = v
            return arr
        return f

    bad("^A:", A=lambda A: A[0])
    bad("^A:", A=lambda A: A[:, :0])
    bad("^A:", A=lambda A: A[:, :, :0])
    for nc in (1, 0, -3, 2.0, 3.5, "3", None, True):
        bad("^num_classes:", num_classes=nc)
    bad("^num_classes: D = ", num_classes=23)                          # 22 * 3 = 66
    bad("^num_classes: D = ", A=np.zeros((3, 12, 65)), num_classes=2)
    bad("^y:", y=lambda y: y[:, :11])
    bad("^y:", y=lambda y: y[:2])
    bad("^y:", y=lambda y: y[0])
    bad("^y: .*dtype", y=lambda y: y.astype(str))
    bad("^y: .*dtype", y=lambda y: y > 0)
    bad("^y: .*dtype", y=lambda y: y.astype(np.complex128))
    for v in (-1, 4, 100):
        bad(r"^y: .*\[1\]", y=put(1, 3, v, np.int64))
    for v in (-1.0, 4.0, 0.5, 2.000001, np.nan, np.inf, -np.inf):
        bad(r"^y: .*\[1\]", y=put(1, 3, v))
    bad(r"^y: .*\[0, 2\]", y=lambda y: np.where(np.arange(3)[:, None] != 1, 9, y))
    for badc in ([12, 13, 1], [-1, 2, 3], [1, 2], [1.5, 2.0, 3.0]):
        bad("^counts:", counts=badc)
    for badl in (-0.5, np.nan, np.inf, [0.1, 0.2], [0.1, -0.2, 0.3], [0.1, np.nan, 0.3]):
        bad("^prior_precision:", prior_precision=badl)
    # beyond the valid rows anything goes, and is stored as 0; floats with integral values and every integer dtype are labels
    A, y, counts, lam, X = ref.make_inputs(3, 12, 4, 3, 2)
    y2 = y.astype(np.float64)
    y2[2, counts[2]:] = np.nan
    y2[1, counts[1]:] = 17.5
    t = BatchedSoftmaxTarget(A, y2, 4, lam, counts, engine=eng)
    assert t.y.dtype == np.int32 and (t.y[2, counts[2]:] == 0).all() and (t.y[1, counts[1]:] == 0).all()
    live = np.arange(12)[None, :] < counts[:, None]
    assert np.array_equal(t.y[live], y[live])
    with pytest.raises(ValueError, match=r"^y: .*\[1, 2\]"):
        BatchedSoftmaxTarget(A, y2, 4, lam, None, engine=eng)          # ... unless every row counts
    for dt in (np.int8, np.uint8, np.int16, np.int64, np.uint64, np.float32):
        assert np.array_equal(BatchedSoftmaxTarget(A, y.astype(dt), 4, lam, counts, engine=eng).y[live], y[live])
    assert np.array_equal(BatchedSoftmaxTarget(A, torch.tensor(y.astype(np.int64)), np.int64(4), lam, counts, engine=eng).y[live],
                          y[live])
    BatchedSoftmaxTarget(np.zeros((2, 3, 1)), np.full((2, 3), 64), 65, engine=eng)       # the largest C


def test_target_protocol_on_the_restatement_engine():
    from gsmvi_amd import BatchedSoftmaxTarget, BatchedGLMTarget
    K, N, Cc, P, rows = 3, 12, 4, 3, 5
    A, y, counts, lam, X = ref.make_inputs(K, N, Cc, P, rows)
    G, lp = ref.score_and_lp(A, y, Cc, counts, lam, X)
    eng = ref.RestatementEngine()
    tgt = BatchedSoftmaxTarget(A, y, Cc, lam, counts, engine=eng)
    assert not isinstance(tgt, BatchedGLMTarget) and not issubclass(BatchedSoftmaxTarget, BatchedGLMTarget)
    assert (tgt.K, tgt.N, tgt.D, tgt.P, tgt.C) == (K, N, (Cc - 1) * P, P, Cc)
    assert tgt.lp_g.device_native is True and tgt.lp_g.graph_safe is True
    assert tgt.counts.dtype == np.int32 and tgt.A.dtype == np.float64 and tgt.y.dtype == np.int32
    assert np.array_equal(tgt.lp_g(X), G)
    out = np.empty_like(X)
    assert tgt.lp_g(X, out=out) is out and np.array_equal(out, G)
    v = tgt.lp(X)
    assert v.shape == (K, rows) and np.array_equal(v, lp)
    g2, v2 = tgt.lp_and_score(X)
    assert np.array_equal(g2, G) and np.array_equal(v2, lp)
    assert [c for c in eng.calls if isinstance(c, tuple)] == [("softmax", Cc, "g", False), ("softmax", Cc, "g", True),
                                                              ("softmax", Cc, "lp", False), ("softmax", Cc, "both", False)]
    # tensors in, a scalar precision, no counts, float32 data
    t = BatchedSoftmaxTarget(torch.tensor(A, dtype=torch.float32), torch.tensor(y), Cc, 0.5, engine=eng)
    Gs, lps = ref.score_and_lp(A.astype(np.float32), y, Cc, None, 0.5, X)
    assert t.counts is None and t.prior_precision == 0.5
    assert np.array_equal(t.lp_g(torch.tensor(X)), Gs) and np.array_equal(t.lp(torch.tensor(X)), lps)
    # the form monitors.lp_sums accepts: (K, rows) values -> (K,) sums
    from gsmvi_amd.monitors import lp_sums
    s = lp_sums(tgt.lp, X, eng, K)
    assert s.shape == (K,) and rel_err(s, lp.sum(1)) < 1e-15


def test_the_glm_only_functions_refuse_the_target():
    """the documented limit: no Laplace initialiser, predictive or leave-one-out for the softmax target"""
    import gsmvi_amd
    from gsmvi_amd import BatchedSoftmaxTarget, BatchedGLMTarget, laplace_init_batched, psis_loo_batched
    A, y, counts, lam, X = ref.make_inputs(3, 12, 3, 2, 2)
    eng = ref.RestatementEngine()
    tgt = BatchedSoftmaxTarget(A, y, 3, lam, counts, engine=eng)
    eng.calls.clear()
    mean, cov = np.zeros((3, tgt.D)), np.broadcast_to(np.eye(tgt.D), (3, tgt.D, tgt.D)).copy()
    with pytest.raises(TypeError, match="BatchedGLMTarget"):
        laplace_init_batched(tgt)
    with pytest.raises(TypeError, match="BatchedGLMTarget"):
        psis_loo_batched(tgt, mean, cov, np.arange(3))
    with pytest.raises(TypeError, match="predict"):
        tgt.predict(mean, cov, A)
    with pytest.raises(TypeError, match="BatchedGLMTarget"):
        tgt.loo(mean, cov, np.arange(3))
    assert eng.calls == []
    assert "BatchedSoftmaxTarget" in gsmvi_amd.__doc__ and "BatchedSoftmaxTarget" in gsmvi_amd.targets.__doc__
