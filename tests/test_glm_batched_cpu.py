"""The batched GLM targets without a GPU: the numpy restatement (tests/glm_batched_ref.py) pinned to torch autograd of the written
densities and, for the gaussian family, to the closed-form posterior; the C ABI declaration and argument checks of
gsmvi_glm_batched_f64; the LDS budget with an offset; and the host logic of BatchedGLMTarget on a stand-in engine."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import glm_batched_ref as ref
from gsmvi_amd import _lib
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsmvi_glm_batched_f64"
CASES = [(3, 1, 1, 1, 1), (5, 33, 17, 33, 1), (3, 100, 64, 9, 1), (3, 70, 64, 5, 6)]


# ---- 1. the restatement is autograd of the written densities -------------------------------------------------------------
def _autograd(family, A, y, o, n, lam, tau, X):
    """one problem: lp (rows,) and d sum(lp) / d X by CPU torch, float64, the density as the header writes it"""
    At, yt, ot = torch.tensor(A[:n]), torch.tensor(y[:n]), torch.tensor(o[:n])
    x = torch.tensor(X, requires_grad=True)
    t = x @ At.T + ot[None, :]
    if family == "logistic":
        terms = yt * t - (torch.clamp(t, min=0) + torch.log1p(torch.exp(-torch.abs(t))))
    elif family == "poisson":
        terms = yt * t - torch.exp(t)
    elif family == "probit":
        terms = yt * torch.special.log_ndtr(t) + (1.0 - yt) * torch.special.log_ndtr(-t)
    else:
        terms = -0.5 * tau * (yt - t) ** 2
    lp = terms.sum(1) - 0.5 * lam * (x * x).sum(1)
    (g,) = torch.autograd.grad(lp.sum(), x)
    return g.numpy(), lp.detach().numpy()


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("K,N,D,rows,scale", CASES)
def test_restatement_is_autograd_of_the_written_density(family, K, N, D, rows, scale):
    """1e-11 per problem (poisson's X is held to scale <= 2 by make_inputs); the worst case measured is 7e-13, probit at
    |eta| near 135"""
    A, y, o, counts, lam, tau, X = ref.make_inputs(family, K, N, D, rows, scale)
    G, lp = ref.score_and_lp(family, A, y, o, counts, lam, tau, X)
    assert np.isfinite(G).all() and np.isfinite(lp).all()
    taus = np.broadcast_to(tau, (K,))
    worst, eta = 0.0, 0.0
    for k in range(K):
        g_t, lp_t = _autograd(family, A[k], y[k], o[k], int(counts[k]), float(lam[k]), float(taus[k]), X[k])
        eg, el = rel_err(G[k], g_t), rel_err(lp[k], lp_t)
        worst = max(worst, eg, el)
        eta = max(eta, float(np.abs(X[k] @ A[k, :counts[k]].T + o[k, None, :counts[k]]).max()))
        assert eg <= 1e-11 and el <= 1e-11, (family, k, eg, el)
    print(f"{family} K={K} N={N} D={D} rows={rows} scale={scale}: worst rel_err {worst:.2e}, max|eta| {eta:.1f}")


def test_probit_forms_match_log_ndtr_elementwise_and_stay_finite():
    """the erfcx forms against torch.special.log_ndtr and its autograd for |eta| <= 40 (elementwise relative error), and finite
    out to |eta| = 1e4"""
    eta = np.concatenate([np.linspace(-40, 40, 8001), [0.0, -0.0, 1e-300, -1e-300]])
    for yv in (0.0, 1.0, 0.3):
        r, t, _ = ref.link("probit", eta, np.full_like(eta, yv))
        x = torch.tensor(eta, requires_grad=True)
        tt = yv * torch.special.log_ndtr(x) + (1.0 - yv) * torch.special.log_ndtr(-x)
        (rr,) = torch.autograd.grad(tt.sum(), x)
        et = np.abs(t - tt.detach().numpy()) / np.maximum(np.abs(tt.detach().numpy()), 1e-300)
        er = np.abs(r - rr.numpy()) / np.maximum(np.abs(rr.numpy()), 1e-300)
        print(f"probit y={yv}: elementwise relative error, t {et.max():.2e} r {er.max():.2e}")
        assert et.max() <= 1e-12 and er.max() <= 1e-12
    big = np.array([-1e4, -3e3, 3e3, 1e4])
    for yv in (0.0, 1.0, 0.5):
        r, t, _ = ref.link("probit", big, np.full_like(big, yv))
        assert np.isfinite(r).all() and np.isfinite(t).all()


@pytest.mark.parametrize("K,N,D,rows", [(4, 50, 12, 9), (3, 100, 64, 9), (3, 5, 17, 4)])
def test_gaussian_family_is_the_closed_form_posterior(K, N, D, rows):
    """score = -P (x - m) with P = tau A^T A + lam I and m = P^-1 tau A^T (y - o); lp differs from -(x - m)^T P (x - m) / 2 by a
    constant per problem.  1e-11; measured <= 4e-15"""
    A, y, o, counts, lam, tau, X = ref.make_inputs("gaussian", K, N, D, rows)
    lam = lam + 0.05                                                    # (problem 0: a proper posterior when n_k < D)
    G, lp = ref.score_and_lp("gaussian", A, y, o, counts, lam, tau, X)
    for k in range(K):
        n = int(counts[k])
        Ak, zk = A[k, :n], (y[k, :n] - o[k, :n])
        P = tau[k] * Ak.T @ Ak + lam[k] * np.eye(D)
        m = np.linalg.solve(P, tau[k] * Ak.T @ zk)
        d = X[k] - m
        Gc = -d @ P
        quad = -0.5 * np.einsum("ri,ij,rj->r", d, P, d)
        c0 = lp[k] - quad
        eg = rel_err(G[k], Gc)
        el = float(np.abs(c0 - c0[0]).max() / max(np.abs(lp[k]).max(), 1e-300))
        print(f"gaussian K={K} N={N} D={D} k={k}: score {eg:.2e}, lp - quadratic constant to {el:.2e}")
        assert eg <= 1e-11 and el <= 1e-11, (k, eg, el)


def test_restatement_nan_rules_counts_and_offset_forms():
    """counts = None is all N rows, a scalar precision is K equal values, a zero offset is no offset (bit for bit), rows beyond
    counts play no part, a non-finite row of X is NaN alone; poisson: a row whose exp(eta) overflows is NaN alone, and the
    logistic family without an offset is logistic_batched_ref bit for bit"""
    import logistic_batched_ref as lref
    for family in ref.FAMILIES:
        A, y, o, counts, lam, tau, X = ref.make_inputs(family, 3, 20, 4, 5)
        full = np.full(3, 20, dtype=np.int32)
        a = ref.score_and_lp(family, A, y, o, None, 0.7, tau, X)
        b = ref.score_and_lp(family, A, y, o, full, np.full(3, 0.7), np.broadcast_to(tau, (3,)), X)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        A2, y2, o2 = A.copy(), y.copy(), o.copy()
        for k in range(3):
            A2[k, counts[k]:] = np.nan
            y2[k, counts[k]:] = np.inf
            o2[k, counts[k]:] = -np.inf
        a, b = ref.score_and_lp(family, A, y, o, counts, lam, tau, X), ref.score_and_lp(family, A2, y2, o2, counts, lam, tau, X)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        X2 = X.copy()
        X2[1, 2, 3] = np.inf
        c = ref.score_and_lp(family, A, y, o, counts, lam, tau, X2)
        keep = np.ones(X.shape[:2], dtype=bool)
        keep[1, 2] = False
        assert np.isnan(c[0][1, 2]).all() and np.isnan(c[1][1, 2])
        assert np.array_equal(c[0][keep], a[0][keep]) and np.array_equal(c[1][keep], a[1][keep])
    A, y, o, counts, lam, tau, X = ref.make_inputs("poisson", 3, 20, 4, 5)
    a = ref.score_and_lp("poisson", A, y, o, counts, lam, tau, X)
    X2 = X.copy()
    X2[2, 1] *= 800.0 / np.abs(X[2, 1] @ A[2, :counts[2]].T).max()
    c = ref.score_and_lp("poisson", A, y, o, counts, lam, tau, X2)
    keep = np.ones(X.shape[:2], dtype=bool)
    keep[2, 1] = False
    assert np.isnan(c[0][2, 1]).all() and np.isnan(c[1][2, 1])
    assert np.array_equal(c[0][keep], a[0][keep]) and np.array_equal(c[1][keep], a[1][keep])
    assert np.isfinite(c[0][keep]).all() and np.isfinite(c[1][keep]).all()
    A, y, o, counts, lam, tau, X = ref.make_inputs("logistic", 3, 20, 4, 5)
    a, b = ref.score_and_lp("logistic", A, y, None, counts, lam, 1.0, X), lref.score_and_lp(A, y, counts, lam, X)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 2. the C ABI --------------------------------------------------------------------------------------------------------
def test_glm_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr)
    for mp in ("exports.map", "exports_debug.map"):
        assert re.search(r"^\s*" + NAME + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), mp
    assert NAME in _lib.exported_symbols() and NAME in built
    from gsmvi_amd.engine import HipEngine
    for code, fam in enumerate(("LOGISTIC", "POISSON", "PROBIT", "GAUSSIAN")):
        assert re.search(rf"#define\s+GSMVI_GLM_{fam}\s+{code}\b", hdr), fam
        assert HipEngine.GLM_FAMILIES[fam.lower()] == code
    assert len(HipEngine.GLM_FAMILIES) == 4
    head = hdr.split("#ifndef GSMVI_HIP_H")[0]                        # the reference map names it and the callable it replaces
    assert NAME in head and head.count("example_gsm.py:34-35") >= 2
    block = hdr[:hdr.index("int " + NAME)].rsplit("/*", 1)[1]           # its own doc block cites the callable too
    assert "example_gsm.py:34-35" in block and "GSMVI_PATH_BATCHED_TARGET" in block
    # the ctypes signature is the declaration's: 18 arguments, family an int after N, the two precisions as doubles
    res, args = _lib._SIGS[NAME]
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\);", hdr, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert res is C.c_int and len(args) == len(params) == 18
    for p, a in zip(params, args):
        want = C.c_double if p.startswith("double ") else C.c_int64 if p.startswith("int64_t") else \
            C.c_int if p.startswith("int ") else C.c_void_p
        assert a is want, (p, a)
    assert params[6] == "int family"
    dbg = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path(debug=True)], check=True, capture_output=True,
                         text=True).stdout
    assert "gsmvi_debug_glm_batched_lds" in dbg and "gsmvi_debug_glm_batched_lds" not in out


# ---- 3. argument checks ----------------------------------------------------------------------------------------------------
def test_abi_checks_arguments_before_the_context_and_names_overlapping_arrays():
    """every bad argument is reported with a NULL context (no device work can have started); valid ones end at the context"""
    lib = _lib.load_library()
    buf = (C.c_double * 8192)()
    p = C.cast(buf, C.c_void_p).value
    a = lambda n: p + 8 * 512 * n                                   # noqa: E731  sixteen disjoint 4 KB arrays
    err = lambda: (lib.gsmvi_last_error() or b"").decode()           # noqa: E731

    def call(K=2, D=4, nc=3, N=5, family=1, A=a(0), y=a(1), offset=a(7), counts=a(2), tau=1.0, tau_dev=None, lam=1.0,
             lam_dev=None, X=a(3), G=a(4), lp=a(5)):
        return lib.gsmvi_glm_batched_f64(None, None, K, D, nc, N, family, A, y, offset, counts, tau, tau_dev, lam, lam_dev, X, G, lp)

    assert call(D=0) == 1 and "D must be" in err()
    assert call(D=65) == 1 and "D must be" in err()
    assert call(K=0) == 1 and "K must be" in err()
    assert call(nc=0) == 1 and "nc must be" in err()
    assert call(N=0) == 1 and "N must be" in err()
    assert call(K=2 ** 20, N=2 ** 40) == 1 and "too large" in err()
    for fam in (-1, 4, 100):
        assert call(family=fam) == 1 and "family" in err() and NAME in err(), fam
    for name in ("A", "y", "X"):
        assert call(**{name: None}) == 1 and "NULL array" in err(), name
    assert call(G=None, lp=None) == 1 and "G or lp" in err()
    assert call(lam=-1.0) == 1 and "prior_prec" in err()
    assert call(lam=float("nan")) == 1 and "prior_prec" in err()
    # the noise precision belongs to the gaussian family
    for fam in (0, 1, 2):
        assert call(family=fam, tau=2.0) == 1 and "noise_prec" in err(), fam
        assert call(family=fam, tau_dev=a(8)) == 1 and "noise_prec" in err(), fam
        assert call(family=fam, tau=float("nan")) == 1 and "noise_prec" in err(), fam
        assert call(family=fam) == 1 and "ctx is NULL" in err(), fam
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(family=3, tau=bad) == 1 and "noise_prec" in err(), bad
    assert call(family=3, tau=2.5) == 1 and "ctx is NULL" in err()
    assert call(family=3, tau=-1.0, tau_dev=a(8)) == 1 and "ctx is NULL" in err()      # the scalar is unused with K values
    # a written array overlapping any other array, at both ends; the message names both
    for name, other in (("A", a(0)), ("y", a(1)), ("counts_dev", a(2)), ("X", a(3)), ("offset", a(7))):
        assert call(G=other) == 1 and f"G overlaps {name}" in err(), name
        assert call(lp=other) == 1 and f"lp overlaps {name}" in err(), name
    assert call(lam_dev=a(6), G=a(6)) == 1 and "G overlaps prior_prec_dev" in err()
    assert call(lam_dev=a(6), lp=a(6)) == 1 and "lp overlaps prior_prec_dev" in err()
    assert call(family=3, tau_dev=a(8), G=a(8)) == 1 and "G overlaps noise_prec_dev" in err()
    assert call(family=3, tau_dev=a(8), lp=a(8)) == 1 and "lp overlaps noise_prec_dev" in err()
    assert call(lp=a(4)) == 1 and "lp overlaps G" in err()
    assert call(G=a(3) + 8 * (2 * 3 * 4 - 1)) == 1 and "G overlaps X" in err()          # the last element of X
    assert call(G=a(7) + 8 * (2 * 5 - 1)) == 1 and "G overlaps offset" in err()         # the last element of the offset
    assert call(G=a(7) + 8 * 2 * 5) == 1 and "ctx is NULL" in err()                     # adjacent is not overlapping
    # valid calls end at the context
    for fam in (0, 1, 2, 3):
        assert call(family=fam) == 1 and "ctx is NULL" in err()
        assert call(family=fam, offset=None, counts=None, G=None) == 1 and "ctx is NULL" in err()
        assert call(family=fam, lp=None, lam=0.0) == 1 and "ctx is NULL" in err()
    assert call(lam=-1.0, lam_dev=a(6)) == 1 and "ctx is NULL" in err()
    assert call(y=a(0), X=a(0), counts=a(0), lam_dev=a(0), offset=a(0)) == 1 and "ctx is NULL" in err()    # read-only arrays may overlap
    # the sibling still reports under its own name
    assert lib.gsmvi_logistic_batched_f64(None, None, 2, 0, 3, 5, a(0), a(1), None, 1.0, None, a(3), a(4), a(5)) == 1
    assert "gsmvi_logistic_batched_f64" in err() and "D must be" in err()


# ---- 4. LDS budget -------------------------------------------------------------------------------------------------------
def test_lds_budget_with_an_offset_stays_below_the_default_limit():
    """the dynamic LDS a launch requests (the library's own host arithmetic, through the debug build's query in a child
    process), per family: without the offset's tile the figures of gsmvi_debug_logistic_batched_lds, with it 32 doubles per
    problem more; the tile is there with an offset and, for the poisson family, always (the launch's own rule); never above the
    64 KiB a kernel gets without asking (the worst case grows from 60 KB to 61 KB)"""
    import json
    import sys
    code = (
        "import ctypes as C, json, sys\n"
        "lib = C.CDLL(sys.argv[1])\n"
        "f, g = lib.gsmvi_debug_glm_batched_lds, lib.gsmvi_debug_logistic_batched_lds\n"
        "f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]\n"
        "g.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]\n"
        "out = {}\n"
        "for D in range(0, 66):\n"
        "    for nc in (0, 1, 15, 16, 17, 31, 32, 33, 100000):\n"
        "        for want in (0, 1, 2, 3, 4):\n"
        "            for fam in (-1, 0, 1, 2, 3, 4):\n"
        "                row = []\n"
        "                for off in (0, 1, None):\n"
        "                    n, p = C.c_size_t(0), C.c_int(0)\n"
        "                    st = g(D, nc, want, C.byref(n), C.byref(p)) if off is None else f(D, nc, want, fam, off, C.byref(n), C.byref(p))\n"
        "                    row += [st, n.value, p.value]\n"
        "                out[f'{D},{nc},{want},{fam}'] = row\n"
        "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.library_path(debug=True)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    worst = 0
    for key, (st0, n0, p0, st1, n1, p1, stl, nl, pl) in got.items():
        D, nc, want, fam = (int(x) for x in key.split(","))
        if not (1 <= D <= 64 and nc >= 1 and 1 <= want <= 3 and 0 <= fam <= 3):
            assert st0 == st1 == 1, key
            continue
        assert st0 == st1 == stl == 0 and p0 == p1 == pl == (4 if D <= 16 else 1), key
        assert n1 == nl + 8 * 32 * p1, key
        assert n0 == (n1 if fam == 1 else nl), key                     # poisson carries the tile without an offset too
        assert n1 <= 64 * 1024, (key, n1)
        worst = max(worst, n1)
    assert worst == got["16,16,3,2"][4] == got["16,16,3,1"][1] == 8 * 4 * (1920 + 32) == 61 * 1024


# ---- 5. host logic of BatchedGLMTarget -----------------------------------------------------------------------------------
def test_target_validates_on_the_host_before_the_engine_is_touched():
    from gsmvi_amd import BatchedGLMTarget
    eng = ref.RestatementEngine()

    def bad(match, family="poisson", **kw):
        A, y, o, counts, lam, tau, X = ref.make_inputs(family, 3, 12, 4, 2)
        base = dict(A=A, y=y, family=family, prior_precision=lam, counts=counts, offset=o, engine=eng)
        if family == "gaussian":
            base["noise_precision"] = tau
        for k, v in kw.items():
            base[k] = v(base[k]) if callable(v) else v
        eng.calls.clear()
        with pytest.raises(ValueError, match=match):
            BatchedGLMTarget(**base)
        assert eng.calls == [], (match, kw)

    def put(k, n, v):
        def f(arr):
            arr = np.array(arr, dtype=np.float64)
            arr[k, n] = v
            return arr
        return f

    A, y, o, counts, lam, tau, X = ref.make_inputs("poisson", 3, 12, 4, 2)
    for fam in ("binomial", "Poisson", None, 1):
        with pytest.raises(ValueError, match="^family:"):
            BatchedGLMTarget(A, y, fam, engine=eng)
    assert eng.calls == []
    bad("^A:", A=lambda A: A[0])
    bad("^A:", A=lambda A: A[:, :0])
    bad("^A: D = 65", A=np.zeros((3, 12, 65)))
    bad("^y:", y=lambda y: y[:, :11])
    bad("^y:", y=lambda y: y[:2])
    # the range of y per family, in the valid rows, naming the problems
    for fam, values in (("logistic", (-0.01, 1.01, np.nan, np.inf)), ("probit", (-0.01, 1.01, np.nan, -np.inf)),
                        ("poisson", (-0.5, np.nan, np.inf)), ("gaussian", (np.nan, np.inf, -np.inf))):
        for v in values:
            bad(r"^y: .*\[1\]", family=fam, y=put(1, 3, v))
    for fam, v in (("poisson", 2.5), ("poisson", 0.0), ("gaussian", -7.25), ("logistic", 0.5), ("probit", 0.25)):
        A, y, o, counts, lam, tau, X = ref.make_inputs(fam, 3, 12, 4, 2)
        y2 = y.copy()
        y2[1, 3] = v                                                  # non-integer counts, soft labels: allowed
        y2[2, counts[2]:] = np.nan                                    # beyond the valid rows anything goes
        BatchedGLMTarget(A, y2, fam, lam, counts, o, engine=eng)
        with pytest.raises(ValueError, match=r"^y: .*\[2\]"):
            BatchedGLMTarget(A, y2, fam, lam, None, o, engine=eng)     # ... unless every row counts
    for badc in ([12, 13, 1], [-1, 2, 3], [1, 2], [1.5, 2.0, 3.0]):
        bad("^counts:", counts=badc)
    bad("^offset:", offset=lambda o: o[:, :11])
    bad("^offset:", offset=lambda o: o[0])
    bad("^offset:", offset=lambda o: o.T)
    for v in (np.nan, np.inf, -np.inf):
        bad(r"^offset: .*\[1\]", offset=put(1, 0, v))
    A, y, o, counts, lam, tau, X = ref.make_inputs("poisson", 3, 12, 4, 2)
    o2 = o.copy()
    o2[2, counts[2]:] = np.inf
    BatchedGLMTarget(A, y, "poisson", lam, counts, o2, engine=eng)
    for badl in (-0.5, np.nan, np.inf, [0.1, 0.2], [0.1, -0.2, 0.3], [0.1, np.nan, 0.3]):
        bad("^prior_precision:", prior_precision=badl)
    for fam in ("logistic", "poisson", "probit"):
        for t in (2.0, [1.0, 1.0, 2.0], np.nan):
            bad("^noise_precision:", family=fam, noise_precision=t)
    for t in (0.0, -1.0, np.nan, np.inf, [1.0, 2.0], [1.0, 0.0, 2.0], [1.0, np.nan, 2.0]):
        bad("^noise_precision:", family="gaussian", noise_precision=t)
    bad(r"^noise_precision: .*\[1\]", family="gaussian", noise_precision=[1.0, 0.0, 2.0])


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_target_protocol_on_the_restatement_engine(family):
    from gsmvi_amd import BatchedGLMTarget
    K, N, D, rows = 3, 12, 4, 5
    A, y, o, counts, lam, tau, X = ref.make_inputs(family, K, N, D, rows)
    G, lp = ref.score_and_lp(family, A, y, o, counts, lam, tau, X)
    eng = ref.RestatementEngine()
    tgt = BatchedGLMTarget(A, y, family, lam, counts, o, noise_precision=tau, engine=eng)
    assert (tgt.K, tgt.N, tgt.D, tgt.family) == (K, N, D, family)
    assert tgt.lp_g.device_native is True and tgt.lp_g.graph_safe is True
    assert tgt.counts.dtype == np.int32 and tgt.A.dtype == np.float64 and tgt.offset.dtype == np.float64
    assert np.array_equal(tgt.lp_g(X), G)
    out = np.empty_like(X)
    assert tgt.lp_g(X, out=out) is out and np.array_equal(out, G)
    v = tgt.lp(X)
    assert v.shape == (K, rows) and np.array_equal(v, lp)
    g2, v2 = tgt.lp_and_score(X)
    assert np.array_equal(g2, G) and np.array_equal(v2, lp)
    assert [c for c in eng.calls if isinstance(c, tuple)] == [("glm", family, "g", False), ("glm", family, "g", True),
                                                              ("glm", family, "lp", False), ("glm", family, "both", False)]
    # tensors in, scalar precisions, no counts, no offset, float32 data
    t = BatchedGLMTarget(torch.tensor(A, dtype=torch.float32), torch.tensor(y), family, 0.5, engine=eng,
                         noise_precision=2.0 if family == "gaussian" else 1.0)
    Gs, lps = ref.score_and_lp(family, A.astype(np.float32), y, None, None, 0.5, 2.0 if family == "gaussian" else 1.0, X)
    assert t.counts is None and t.offset is None and t.prior_precision == 0.5 and isinstance(t.noise_precision, float)
    assert np.array_equal(t.lp_g(torch.tensor(X)), Gs) and np.array_equal(t.lp(torch.tensor(X)), lps)
    # the form monitors.lp_sums accepts: (K, rows) values -> (K,) sums
    from gsmvi_amd.monitors import lp_sums
    s = lp_sums(tgt.lp, X, eng, K)
    assert s.shape == (K,) and rel_err(s, lp.sum(1)) < 1e-15
    # lists in; K ones as the noise precision of a family without one
    t3 = BatchedGLMTarget(A, y, family, list(lam), [int(c) for c in counts], o,
                          noise_precision=list(np.broadcast_to(tau, (K,))), engine=eng)
    assert np.array_equal(t3.lp_g(X), G)
