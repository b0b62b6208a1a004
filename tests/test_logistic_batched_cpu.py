"""The batched logistic target without a GPU: the numpy restatement (tests/logistic_batched_ref.py) pinned to torch autograd of
the written density, the C ABI declaration and argument checks, the LDS budget, and the host logic of BatchedLogisticTarget on a
stub engine backed by the restatement."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import logistic_batched_ref as ref
from gsmvi_amd import _lib
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsmvi_logistic_batched_f64"
CASES = [(3, 1, 1, 1, 1), (4, 7, 5, 2, 1), (5, 100, 10, 8, 1), (3, 300, 16, 32, 1), (3, 257, 17, 32, 3), (2, 1000, 33, 32, 1),
         (2, 513, 64, 128, 1), (2, 64, 64, 8, 10)]


# ---- 1. the restatement is autograd of the written density ---------------------------------------------------------------
def _autograd(A, y, n, lam, X):
    """one problem: lp (rows,) and d sum(lp) / d X by CPU torch, float64, the density as the issue writes it"""
    At, yt = torch.tensor(A[:n]), torch.tensor(y[:n])
    x = torch.tensor(X, requires_grad=True)
    t = x @ At.T
    lp = (yt[None, :] * t - (torch.clamp(t, min=0) + torch.log1p(torch.exp(-torch.abs(t))))).sum(1) - 0.5 * lam * (x * x).sum(1)
    (g,) = torch.autograd.grad(lp.sum(), x)
    return g.numpy(), lp.detach().numpy()


def _check_against_autograd(K, N, D, rows, scale, soft):
    A, y, counts, lam, X = ref.make_inputs(K, N, D, rows, scale, soft=soft)
    G, lp = ref.score_and_lp(A, y, counts, lam, X)
    worst, eta = 0.0, 0.0
    for k in range(K):
        g_t, lp_t = _autograd(A[k], y[k], int(counts[k]), float(lam[k]), X[k])
        eg, el = rel_err(G[k], g_t), rel_err(lp[k], lp_t)
        worst = max(worst, eg, el)
        eta = max(eta, float(np.abs(X[k] @ A[k, :counts[k]].T).max()))
        assert eg <= 1e-12 and el <= 1e-12, (k, eg, el)
    print(f"K={K} N={N} D={D} rows={rows} scale={scale} soft={soft}: worst rel_err {worst:.2e}, max|eta| {eta:.1f}")


@pytest.mark.parametrize("K,N,D,rows,scale", CASES)
def test_restatement_is_autograd_of_the_written_density(K, N, D, rows, scale):
    _check_against_autograd(K, N, D, rows, scale, soft=False)


def test_restatement_is_autograd_with_soft_labels():
    _check_against_autograd(4, 100, 10, 8, 1, soft=True)


def test_restatement_counts_and_precision_forms():
    """counts = None is all N rows, a scalar precision is K equal values, rows beyond counts play no part, a non-finite row of X
    is NaN alone"""
    A, y, counts, lam, X = ref.make_inputs(3, 20, 4, 5)
    full = np.full(3, 20, dtype=np.int32)
    a, b = ref.score_and_lp(A, y, None, 0.7, X), ref.score_and_lp(A, y, full, np.full(3, 0.7), X)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    A2, y2 = A.copy(), y.copy()
    for k in range(3):
        A2[k, counts[k]:] = np.nan
        y2[k, counts[k]:] = np.inf
    a, b = ref.score_and_lp(A, y, counts, lam, X), ref.score_and_lp(A2, y2, counts, lam, X)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    X2 = X.copy()
    X2[1, 2, 3] = np.inf
    c = ref.score_and_lp(A, y, counts, lam, X2)
    assert np.isnan(c[0][1, 2]).all() and np.isnan(c[1][1, 2])
    keep = np.ones(X.shape[:2], dtype=bool)
    keep[1, 2] = False
    assert np.array_equal(c[0][keep], a[0][keep]) and np.array_equal(c[1][keep], a[1][keep])


# ---- 2. the C ABI --------------------------------------------------------------------------------------------------------
def test_logistic_entry_point_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr)
    for mp in ("exports.map", "exports_debug.map"):
        assert re.search(r"^\s*" + NAME + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), mp
    assert NAME in _lib.exported_symbols() and NAME in built
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_TARGET\s+0x20000u", hdr)
    mask = re.search(r"#define\s+GSMVI_PATH_GENERIC_MASK\s+\(([^)]*)\)", hdr).group(1)
    assert "0x20000" not in mask
    assert "#define GSMVI_ABI_VERSION 1" in hdr
    head = hdr.split("#ifndef GSMVI_HIP_H")[0]                        # the reference map names it and the callable it replaces
    assert NAME in head and "example_gsm.py:34-35" in head
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_target"] == 0x20000 and not HipEngine.PATH_GENERIC_MASK & 0x20000
    assert len(set(HipEngine.PATH_BITS.values())) == len(HipEngine.PATH_BITS)
    dbg = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path(debug=True)], check=True, capture_output=True,
                         text=True).stdout
    assert "gsmvi_debug_logistic_batched_lds" in dbg and "gsmvi_debug_logistic_batched_lds" not in out


# ---- 3. argument checks ----------------------------------------------------------------------------------------------------
def test_abi_checks_arguments_before_the_context_and_names_overlapping_arrays():
    """every bad argument is reported with a NULL context (no device work can have started); valid ones end at the context"""
    lib = _lib.load_library()
    buf = (C.c_double * 8192)()
    p = C.cast(buf, C.c_void_p).value
    a = lambda n: p + 8 * 512 * n                                   # noqa: E731  sixteen disjoint 4 KB arrays
    err = lambda: (lib.gsmvi_last_error() or b"").decode()           # noqa: E731

    def call(K=2, D=4, nc=3, N=5, A=a(0), y=a(1), counts=a(2), lam=1.0, lam_dev=None, X=a(3), G=a(4), lp=a(5)):
        return lib.gsmvi_logistic_batched_f64(None, None, K, D, nc, N, A, y, counts, lam, lam_dev, X, G, lp)

    assert call(D=0) == 1 and "D must be" in err()
    assert call(D=65) == 1 and "D must be" in err()
    assert call(K=0) == 1 and "K must be" in err()
    assert call(nc=0) == 1 and "nc must be" in err()
    assert call(N=0) == 1 and "N must be" in err()
    assert call(K=2 ** 20, N=2 ** 40) == 1 and "too large" in err()
    for name in ("A", "y", "X"):
        assert call(**{name: None}) == 1 and "NULL array" in err(), name
    assert call(G=None, lp=None) == 1 and "G or lp" in err()
    assert call(lam=-1.0) == 1 and "prior_prec" in err()
    assert call(lam=float("nan")) == 1 and "prior_prec" in err()
    # a written array overlapping any other array, at both ends; the message names both
    for name, other in (("A", a(0)), ("y", a(1)), ("counts_dev", a(2)), ("X", a(3))):
        assert call(G=other) == 1 and f"G overlaps {name}" in err(), name
        assert call(lp=other) == 1 and f"lp overlaps {name}" in err(), name
    assert call(lam_dev=a(6), G=a(6)) == 1 and "G overlaps prior_prec_dev" in err()
    assert call(lam_dev=a(6), lp=a(6)) == 1 and "lp overlaps prior_prec_dev" in err()
    assert call(lp=a(4)) == 1 and "lp overlaps G" in err()
    assert call(G=a(3) + 8 * (2 * 3 * 4 - 1)) == 1 and "G overlaps X" in err()          # the last element of X
    assert call(G=a(3) - 8 * (2 * 3 * 4 - 1)) == 1 and "G overlaps X" in err()          # the last element of G on the first of X
    assert call(lp=a(5), G=a(5) + 8 * (2 * 3 - 1)) == 1 and "lp overlaps G" in err()
    assert call(G=a(3) + 8 * 2 * 3 * 4) == 1 and "ctx is NULL" in err()                 # adjacent is not overlapping
    # valid calls end at the context
    assert call() == 1 and "ctx is NULL" in err()
    assert call(G=None) == 1 and "ctx is NULL" in err()
    assert call(lp=None) == 1 and "ctx is NULL" in err()
    assert call(counts=None) == 1 and "ctx is NULL" in err()
    assert call(lam=0.0) == 1 and "ctx is NULL" in err()
    assert call(lam=-1.0, lam_dev=a(6)) == 1 and "ctx is NULL" in err()                 # the scalar is unused with K values
    assert call(nc=100000, G=None, lp=a(5), X=a(3), K=1, D=1, N=1) == 1                 # nc has no upper bound of its own
    assert call(y=a(0), X=a(0), counts=a(0), lam_dev=a(0)) == 1 and "ctx is NULL" in err()    # read-only arrays may overlap


# ---- 4. LDS budget -------------------------------------------------------------------------------------------------------
def test_lds_budget_fits_every_in_bounds_shape():
    """the dynamic LDS a launch requests (the library's own host arithmetic, read through the debug build's query in a child
    process) is within GB_LDS_MAX = 160 KiB -- and within the 64 KiB a kernel gets without asking, which is why the kernel sets
    no attribute -- for every D in bounds, both packings, any nc; the figure is the formula of DESIGN section 9"""
    src = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_batched.h")).read()
    assert re.search(r"#define\s+GB_LDS_MAX\s+\(160 \* 1024\)", src)
    code = (
        "import ctypes as C, json, sys\n"
        "lib = C.CDLL(sys.argv[1])\n"
        "f = lib.gsmvi_debug_logistic_batched_lds\n"
        "f.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]\n"
        "out = {}\n"
        "for D in range(0, 66):\n"
        "    for nc in (0, 1, 2, 8, 15, 16, 17, 31, 32, 33, 128, 100000):\n"
        "        for want in (0, 1, 2, 3, 4):\n"
        "            n, p = C.c_size_t(0), C.c_int(0)\n"
        "            st = f(D, nc, want, C.byref(n), C.byref(p))\n"
        "            out[f'{D},{nc},{want}'] = [st, n.value, p.value]\n"
        "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.library_path(debug=True)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    worst = 0
    for key, (st, nbytes, ppw) in got.items():
        D, nc, want = (int(x) for x in key.split(","))
        if not (1 <= D <= 64 and nc >= 1 and 1 <= want <= 3):
            assert st == 1, key
            continue
        assert st == 0 and 0 < nbytes <= 160 * 1024 and nbytes <= 64 * 1024, (key, nbytes)
        assert ppw == (4 if D <= 16 else 1), key
        tcm = min(nc, 32 if ppw == 1 else 16)
        ld = D | 1
        assert nbytes == 8 * ppw * (32 * ld + 32 + tcm * (ld + 1 + 33 * bin(want).count("1"))), key
        worst = max(worst, nbytes)
    assert got["64,32,3"][1] == 8 * 6336 and got["16,16,3"][1] == 8 * 4 * 1920 == worst


# ---- 5. host logic of BatchedLogisticTarget ------------------------------------------------------------------------------
class RestatementEngine:
    """the engine calls BatchedLogisticTarget makes, on numpy and the restatement; ``calls`` records every one"""
    name = "restatement-logistic(test-only)"

    def __init__(self):
        self.calls = []

    def asarray(self, x):
        self.calls.append("asarray")
        return np.array(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)

    def batched_counts(self, values):
        self.calls.append("batched_counts")
        return np.asarray(values, dtype=np.int32).reshape(-1)

    def batched_regs(self, values):
        self.calls.append("batched_regs")
        return np.asarray(values, dtype=np.float64).reshape(-1)

    def logistic_batched(self, X, A, y, counts=None, prior_prec=1.0, out=None, lp_out=None, want="g"):
        self.calls.append(("logistic", want, out is not None))
        assert A.dtype == np.float64 and y.dtype == np.float64 and (counts is None or counts.dtype == np.int32)
        G, lp = ref.score_and_lp(A, y, counts, prior_prec, X)
        if out is not None:
            out[...] = G
            G = out
        return G if want == "g" else lp if want == "lp" else (G, lp)


def test_target_validates_on_the_host_before_the_engine_is_touched():
    from gsmvi_amd import BatchedLogisticTarget
    A, y, counts, lam, X = ref.make_inputs(3, 12, 4, 2)
    eng = RestatementEngine()
    mk = lambda **kw: BatchedLogisticTarget(**{**dict(A=A, y=y, prior_precision=lam, counts=counts, engine=eng), **kw})   # noqa: E731
    with pytest.raises(ValueError, match="^A:"):
        mk(A=A[0])
    with pytest.raises(ValueError, match="^A:"):
        mk(A=A[:, :0])
    with pytest.raises(ValueError, match="^A: D = 65"):
        mk(A=np.zeros((3, 12, 65)))
    with pytest.raises(ValueError, match="^y:"):
        mk(y=y[:, :11])
    with pytest.raises(ValueError, match="^y:"):
        mk(y=y[:2])
    for badv in (-0.01, 1.01, np.nan, np.inf):
        y2 = y.copy()
        y2[1, 3] = badv
        with pytest.raises(ValueError, match=r"^y: .*\[1\]"):
            mk(y=y2)
    y2 = y.copy()
    y2[2, counts[2]:] = np.nan                                        # beyond the valid rows anything goes
    mk(y=y2)
    with pytest.raises(ValueError, match="^y:"):
        mk(y=y2, counts=None)                                         # ... unless every row counts
    for badc in ([12, 13, 1], [-1, 2, 3], [1, 2], [1.5, 2.0, 3.0]):
        eng.calls.clear()
        with pytest.raises(ValueError, match="^counts:"):
            mk(counts=badc)
        assert eng.calls == []
    for badl in (-0.5, np.nan, np.inf, [0.1, 0.2], [0.1, -0.2, 0.3], [0.1, np.nan, 0.3]):
        eng.calls.clear()
        with pytest.raises(ValueError, match="^prior_precision:"):
            mk(prior_precision=badl)
        assert eng.calls == []


def test_target_protocol_on_the_restatement_engine():
    from gsmvi_amd import BatchedLogisticTarget
    K, N, D, rows = 3, 12, 4, 5
    A, y, counts, lam, X = ref.make_inputs(K, N, D, rows)
    G, lp = ref.score_and_lp(A, y, counts, lam, X)
    eng = RestatementEngine()
    tgt = BatchedLogisticTarget(A, y, lam, counts, engine=eng)
    assert (tgt.K, tgt.N, tgt.D) == (K, N, D)
    assert tgt.lp_g.device_native is True and tgt.lp_g.graph_safe is True
    assert tgt.counts.dtype == np.int32 and tgt.A.dtype == np.float64
    assert np.array_equal(tgt.lp_g(X), G)
    out = np.empty_like(X)
    assert tgt.lp_g(X, out=out) is out and np.array_equal(out, G)
    v = tgt.lp(X)
    assert v.shape == (K, rows) and np.array_equal(v, lp)
    g2, v2 = tgt.lp_and_score(X)
    assert np.array_equal(g2, G) and np.array_equal(v2, lp)
    assert [c for c in eng.calls if isinstance(c, tuple)] == [("logistic", "g", False), ("logistic", "g", True),
                                                              ("logistic", "lp", False), ("logistic", "both", False)]
    # tensors in, a scalar precision, no counts, float32 / integer data
    t = BatchedLogisticTarget(torch.tensor(A, dtype=torch.float32), torch.tensor(y).to(torch.int64), 0.5, None, engine=eng)
    Gs, lps = ref.score_and_lp(A.astype(np.float32), y, None, 0.5, X)
    assert t.counts is None and t.prior_precision == 0.5 and isinstance(t.prior_precision, float)
    assert np.array_equal(t.lp_g(torch.tensor(X)), Gs) and np.array_equal(t.lp(torch.tensor(X)), lps)
    # the form monitors.lp_sums accepts: (K, rows) values -> (K,) sums
    from gsmvi_amd.monitors import lp_sums

    class _E(RestatementEngine):
        def to_numpy(self, a):
            return np.asarray(a)

    e2 = _E()
    s = lp_sums(BatchedLogisticTarget(A, y, lam, counts, engine=e2).lp, X, e2, K)
    assert s.shape == (K,) and rel_err(s, lp.sum(1)) < 1e-15
    # K per-problem precisions as a list, counts as a list
    t3 = BatchedLogisticTarget(A, y, list(lam), [int(c) for c in counts], engine=eng)
    assert np.array_equal(t3.lp_g(X), G)
