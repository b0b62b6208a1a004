"""Batched ADVI without a GPU: the numpy restatement (tests/advi_batched_ref.py) pinned to torch autograd + torch.optim.Adam, the
C ABI declarations and argument checks, the LDS budget, and the host logic of ADVIBatch.fit driven by an engine backed by the
restatement (the pattern of tests/test_bam_batched_cpu.py)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import advi_batched_ref as ref
from gsmvi_amd import _lib
from gsmvi_amd._fitloop import seed_of
from gsmvi_amd.batched import ADVIBatch, Adam
from gsmvi_amd.monitors import KLMonitor
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gsmvi_advi_init_batched_f64", "gsmvi_advi_step_batched_f64", "gsmvi_advi_cov_batched_f64"]


# ---- 1. the restatement is the reference estimator ---------------------------------------------------------------------
@pytest.mark.parametrize("D,B,lr", [(5, 2, 1e-2), (10, 2, 1e-2), (10, 8, 1e-1), (33, 32, 1e-2), (64, 8, 1e-2)])
def test_restatement_is_autograd_with_torch_adam(D, B, lr):
    """501 steps of ADVI.neg_elbo + torch.optim.Adam on CPU torch, fed the fits' draws, against the closed-form gradient + Adam
    of the restatement: loc, scales and the losses at 1e-12 (the oracle-versus-golden bar), the first gradient too"""
    nsteps, seed = 501, 1234 + D
    ms, Ps = ref.gaussian_targets(1, D, seed=D)
    rs = np.random.RandomState(D)
    A = rs.standard_normal((D, D))
    mean0, cov0 = rs.standard_normal((1, D)), (A @ A.T / D + 0.5 * np.eye(D))[None]
    loc_t, scales_t, losses_t, g0 = ref.torch_advi_run(ms[0], Ps[0], seed, lr, B, nsteps, mean0[0], cov0[0])
    # the first gradient
    Z0 = ref.draw(seed, 0, B, D)[None]
    scales0, X0, _ = ref.init(mean0, cov0, Z0)
    gl, gs = ref.gradient(ref.gaussian_score(ms, Ps)(X0)[0], Z0[0], scales0[0])
    print(f"D={D} B={B}: first gradient {rel_err(gl, g0[0]):.2e} {rel_err(gs, g0[1]):.2e}")
    assert rel_err(gl, g0[0]) <= 1e-12 and rel_err(gs, g0[1]) <= 1e-12
    # the trajectory: run the restatement's loop and keep its packed scales
    loc, cov, losses = ref.fit([seed], ref.gaussian_lp(ms, Ps), ref.gaussian_score(ms, Ps), lr, mean0, cov0, B, nsteps - 1)
    Lt = ref.unpack(scales_t, D)
    print(f"D={D} B={B}: loc {rel_err(loc[0], loc_t):.2e} cov {rel_err(cov[0], Lt @ Lt.T):.2e} "
          f"losses {rel_err(losses[:, 0], losses_t):.2e}")
    assert rel_err(loc[0], loc_t) <= 1e-12
    assert rel_err(cov[0], Lt @ Lt.T) <= 1e-12
    assert rel_err(losses[:, 0], losses_t) <= 1e-12


@pytest.mark.parametrize("D,B", [(5, 2), (10, 8), (33, 32)])
def test_restatement_scales_match_torch_entry_by_entry(D, B):
    """the packed scales themselves (not only L L^T) after 501 steps, and the step function chained by hand"""
    nsteps, seed, lr = 501, 77, 1e-2
    ms, Ps = ref.gaussian_targets(1, D, seed=3)
    loc_t, scales_t, _, _ = ref.torch_advi_run(ms[0], Ps[0], seed, lr, B, nsteps)
    lp_g = ref.gaussian_score(ms, Ps)
    Z = ref.draw(seed, 0, B, D)[None]
    loc = np.zeros((1, D))
    scales, X, _ = ref.init(loc, np.eye(D)[None], Z)
    mom = tuple(np.zeros((1, n)) for n in (D, D, ref.tri(D), ref.tri(D)))
    for i in range(nsteps):
        Zn = ref.draw(seed, i + 1, B, D)[None]
        loc, scales, mom, X, _ = ref.step(lp_g(X), Z, loc, scales, mom, i + 1, lr, Znext=Zn)
        Z = Zn
    assert rel_err(loc[0], loc_t) <= 1e-12 and rel_err(scales[0], scales_t) <= 1e-12


# ---- 2. the C ABI ------------------------------------------------------------------------------------------------------
def test_batched_advi_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        for mp in ("exports.map", "exports_debug.map"):
            assert re.search(r"^\s*" + name + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), (mp, name)
        assert name in _lib.exported_symbols() and name in built, name
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_ADVI\s+0x10000u", hdr)
    mask = re.search(r"#define\s+GSMVI_PATH_GENERIC_MASK\s+\(([^)]*)\)", hdr).group(1)
    assert "0x10000" not in mask
    assert "#define GSMVI_ABI_VERSION 1" in hdr
    assert "gsmvi_advi_step_batched_f64" in hdr.split("#ifndef GSMVI_HIP_H")[0]          # the reference map names it
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_advi"] == 0x10000 and not HipEngine.PATH_GENERIC_MASK & 0x10000


def test_abi_checks_arguments_before_the_context_and_names_overlapping_arrays():
    """every bad argument is reported with a NULL context (no device work can have started); valid ones end at the context"""
    lib = _lib.load_library()
    buf = (C.c_double * 8192)()
    p = C.cast(buf, C.c_void_p).value
    a = lambda n: p + 8 * 512 * n                                   # noqa: E731  sixteen disjoint 4 KB arrays
    ib = (C.c_int * 64)()
    ip = C.cast(ib, C.c_void_p).value
    err = lambda: (lib.gsmvi_last_error() or b"").decode()           # noqa: E731

    def init(K=2, D=4, B=2, mean=a(0), cov=a(1), scales=a(2), info=ip, seeds=a(3), Z=None, X=a(4), logq=a(5)):
        return lib.gsmvi_advi_init_batched_f64(None, None, K, D, B, mean, cov, scales, info, seeds, Z, X, logq)

    assert init(D=65) == 1 and "D must be" in err()
    assert init(D=0) == 1 and "D must be" in err()
    assert init(B=33) == 1 and "B must be" in err()
    assert init(B=0) == 1 and "B must be" in err()
    assert init(K=0) == 1 and "K must be" in err()
    assert init(mean=None) == 1 and "NULL array" in err()
    assert init(scales=None) == 1 and "NULL array" in err()
    assert init(info=None) == 1 and "NULL array" in err()
    assert init(Z=a(6)) == 1 and "not both" in err()
    assert init(X=None) == 1 and "without X" in err()
    assert init(logq=None) == 1 and "without X" in err()
    assert init(seeds=None) == 1 and "without seeds_dev or Z" in err()
    assert init(scales=a(1)) == 1 and "scales overlaps cov" in err()
    assert init(X=a(0)) == 1 and "X overlaps mean" in err()
    assert init(logq=a(3)) == 1 and "logq_sum overlaps seeds_dev" in err()
    assert init(seeds=None, Z=a(4)) == 1 and "X overlaps Z" in err()
    assert init() == 1 and "ctx is NULL" in err()
    assert init(seeds=None, Z=a(6)) == 1 and "ctx is NULL" in err()
    assert init(seeds=None, X=None, logq=None) == 1 and "ctx is NULL" in err()
    assert init(mean=a(1)) == 1 and "ctx is NULL" in err()           # read-only arrays may overlap

    def step(K=2, D=4, B=2, G=a(0), loc=a(1), scales=a(2), m_loc=a(3), v_loc=a(4), m_s=a(5), v_s=a(6), t=1, lr=0.1, lr_dev=None,
             b1=0.9, b2=0.999, eps=1e-8, seeds=a(7), call=1, Zcur=None, Znext=None, Xout=a(8), logq=a(9)):
        return lib.gsmvi_advi_step_batched_f64(None, None, K, D, B, G, loc, scales, m_loc, v_loc, m_s, v_s, t, lr, lr_dev, b1,
                                               b2, eps, seeds, call, Zcur, Znext, Xout, logq)

    assert step(D=65) == 1 and "D must be" in err()
    assert step(B=33) == 1 and "B must be" in err()
    assert step(K=0) == 1 and "K must be" in err()
    for name in ("G", "loc", "scales", "m_loc", "v_loc", "m_s", "v_s"):
        assert step(**{name: None}) == 1 and "NULL array" in err(), name
    assert step(t=0) == 1 and "t must be" in err()
    assert step(b1=1.0) == 1 and "b1 and b2" in err()
    assert step(b2=-0.1) == 1 and "b1 and b2" in err()
    assert step(b1=float("nan")) == 1 and "b1 and b2" in err()
    assert step(Zcur=a(10)) == 1 and "not both" in err()
    assert step(call=0) == 1 and "call must be" in err()
    assert step(seeds=None) == 1 and "Zcur" in err()
    assert step(seeds=None, Zcur=a(10)) == 1 and "Znext" in err()
    assert step(logq=None) == 1 and "go together" in err()
    assert step(Xout=None) == 1 and "go together" in err()
    assert step(loc=a(0)) == 1 and "loc overlaps G" in err()
    assert step(m_s=a(2)) == 1 and "m_s overlaps scales" in err()
    assert step(v_loc=a(3)) == 1 and "v_loc overlaps m_loc" in err()
    assert step(lr_dev=a(6)) == 1 and "v_s overlaps lr_dev" in err()
    assert step(Xout=a(7)) == 1 and "Xout overlaps seeds_dev" in err()
    assert step(logq=a(8)) == 1 and "logq_sum overlaps Xout" in err()
    assert step(seeds=None, Zcur=a(10), Znext=a(11), Xout=a(11)) == 1 and "Xout overlaps Znext" in err()
    assert step() == 1 and "ctx is NULL" in err()
    assert step(lr_dev=a(10)) == 1 and "ctx is NULL" in err()
    assert step(Xout=None, logq=None) == 1 and "ctx is NULL" in err()
    assert step(seeds=None, Zcur=a(10), Znext=a(11)) == 1 and "ctx is NULL" in err()
    assert step(seeds=None, Zcur=a(0), Xout=None, logq=None) == 1 and "ctx is NULL" in err()      # Zcur may overlap G (both read)

    def cov(K=2, D=4, scales=a(0), out=a(1)):
        return lib.gsmvi_advi_cov_batched_f64(None, None, K, D, scales, out)

    assert cov(D=65) == 1 and "D must be" in err()
    assert cov(K=0) == 1 and "K must be" in err()
    assert cov(scales=None) == 1 and "NULL array" in err()
    assert cov(out=a(0)) == 1 and "cov overlaps scales" in err()
    assert cov() == 1 and "ctx is NULL" in err()


# ---- 3. LDS budget -----------------------------------------------------------------------------------------------------
def test_lds_budget_fits_every_in_bounds_shape():
    """the dynamic LDS every batched ADVI launch requests (the library's own host arithmetic, read through the debug build's
    query in a child process) stays within GB_LDS_MAX = 160 KiB -- and within the 64 KiB a kernel gets without asking, which is
    why these kernels set no attribute -- for every (D, B) in bounds; the step's figure is the formula of DESIGN section 9"""
    src = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_batched.h")).read()
    assert re.search(r"#define\s+GB_LDS_MAX\s+\(160 \* 1024\)", src)
    code = (
        "import ctypes as C, json, sys\n"
        "lib = C.CDLL(sys.argv[1])\n"
        "f = lib.gsmvi_debug_advi_batched_lds\n"
        "f.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]\n"
        "out = {}\n"
        "for D in range(0, 66):\n"
        "    for B in range(0, 34):\n"
        "        for mode in (0, 1, 2):\n"
        "            n, p = C.c_size_t(0), C.c_int(0)\n"
        "            st = f(D, B, mode, C.byref(n), C.byref(p))\n"
        "            out[f'{D},{B},{mode}'] = [st, n.value, p.value]\n"
        "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.library_path(debug=True)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for key, (st, nbytes, ppw) in got.items():
        D, B, mode = (int(x) for x in key.split(","))
        if not (1 <= D <= 64 and 1 <= B <= 32):
            assert st == 1, key
            continue
        assert st == 0 and 0 < nbytes <= 160 * 1024 and nbytes <= 64 * 1024, key
        assert ppw == (4 if D <= 16 else 1), key
        Dz, P = D + (D & 1), D * (D + 1) // 2
        want = {0: D * D + B * Dz + 2 * D + 4, 1: B * D + B * Dz + P + D + 4, 2: P}[mode]
        assert nbytes == 8 * ppw * want, key
    assert got["64,32,1"][1] == 8 * 6244 and got["64,32,0"][1] == 8 * 6276


# ---- 2 (continued). host logic on an engine backed by the restatement --------------------------------------------------
class OracleBatchedADVIEngine:
    """ADVIBatch's engine on the restatement: init, step and cov are advi_batched_ref's, the draws the device stream restated on
    the CPU.  ``calls`` records every engine call, ``steps`` the arguments of every step."""
    name = "oracle-batched-advi(test-only)"

    def __init__(self):
        self.calls, self.steps, self.draws = [], [], []

    def _rec(self, what):
        self.calls.append(what)

    def asarray(self, x):
        self._rec("asarray")
        return np.array(x, dtype=np.float64, copy=True)

    def clone(self, x):
        self._rec("clone")
        return np.array(x, dtype=np.float64, copy=True)

    def to_numpy(self, t):
        return np.asarray(t)

    def empty(self, *shape):
        self._rec("empty")
        return np.full(shape, np.nan)

    def zeros(self, *shape):
        self._rec("zeros")
        return np.zeros(shape)

    def eye_batch(self, K, D):
        self._rec("eye_batch")
        return np.broadcast_to(np.eye(D), (K, D, D)).copy()

    def batched_ints(self, K):
        self._rec("batched_ints")
        return np.zeros(K, dtype=np.int64)

    def read_ints(self, t):
        return np.array(t, dtype=np.int64)

    def batched_seeds(self, seeds):
        self._rec("batched_seeds")
        return np.array([int(s) & (2 ** 64 - 1) for s in seeds], dtype=np.uint64)

    def batched_regs(self, values):
        self._rec("batched_regs")
        return np.array(values, dtype=np.float64)

    def host_score(self, lp_g, X, out=None):
        self._rec("host_score")
        out[...] = np.asarray(lp_g(np.array(X, copy=True)), dtype=np.float64)
        return out

    def _draw(self, seeds, call, K, B, D):
        Z = np.stack([ref.draw(seeds[k], call, B, D) for k in range(K)])
        self.draws.append((call, Z.copy()))
        return Z

    def advi_init_batched(self, mean, cov, scales, info, seeds=None, Z=None, X=None, logq=None):
        self._rec("init")
        K, D = mean.shape
        from oracle import gsm_oracle as orc
        for k in range(K):
            info[k] = 0 if orc.cov_is_good(cov[k]) else 1
        if info.any():
            return
        assert (seeds is None) != (Z is None)
        Z = self._draw(seeds, 0, K, X.shape[1], D) if seeds is not None else Z
        scales[...], X[...], logq[...] = ref.init(mean, cov, Z)

    def advi_step_batched(self, G, loc, scales, moments, t, lr, b1=0.9, b2=0.999, eps=1e-8, seeds=None, call=0, Zcur=None,
                          Znext=None, Xout=None, logq=None):
        self._rec(("step", call, Xout is not None))
        K, B, D = G.shape
        self.steps.append({"t": t, "lr": np.array(lr, copy=True), "b1": b1, "b2": b2, "eps": eps})
        assert (Xout is None) == (logq is None) and (seeds is None) != (Zcur is None)
        if seeds is not None:
            assert Znext is None
            Zcur = np.stack([ref.draw(seeds[k], call - 1, B, D) for k in range(K)])
            Znext = self._draw(seeds, call, K, B, D) if Xout is not None else None
        else:
            assert (Znext is None) == (Xout is None)
        out = ref.step(G, Zcur, loc, scales, moments, t, lr, b1, b2, eps, Znext=Znext)
        loc[...], scales[...] = out[0], out[1]
        for dst, src in zip(moments, out[2]):
            dst[...] = src
        if Xout is not None:
            Xout[...], logq[...] = out[3], out[4]

    def advi_cov_batched(self, scales, D, out=None):
        self._rec("cov")
        return ref.cov_of(scales, D)


class _Recorder:
    """a batched monitor that records what it is handed"""
    batched = True
    device_native = True

    def __init__(self, checkpoint):
        self.checkpoint, self.seen = checkpoint, []

    def __call__(self, i, params, lp, keys, nevals=1):
        self.seen.append((i, np.array(params[0], copy=True), np.array(params[1], copy=True), nevals))
        return keys


def _fit(K, D, eng=None, seed=0, lp=True):
    ms, Ps = ref.gaussian_targets(K, D, seed=seed)
    fit = ADVIBatch(K, D, ref.gaussian_lp(ms, Ps) if lp else None, ref.gaussian_score(ms, Ps),
                    engine=eng if eng is not None else OracleBatchedADVIEngine())
    return fit, ms, Ps


@pytest.mark.parametrize("D,B", [(4, 2), (5, 3), (3, 8)])
def test_draws_are_each_problems_stream_and_the_fit_is_the_restatements_loop(D, B):
    K, niter = 3, 9
    keys = [7, 2 ** 40 + 3, 12345]
    eng = OracleBatchedADVIEngine()
    fit, ms, Ps = _fit(K, D, eng)
    rs = np.random.RandomState(1)
    mean0 = rs.standard_normal((K, D))
    cov0 = np.stack([np.eye(D) * (1.0 + 0.3 * k) for k in range(K)])
    mean0_in, cov0_in = mean0.copy(), cov0.copy()
    m, c, losses = fit.fit(keys, Adam(0.05), mean=mean0, cov=cov0, batch_size=B, niter=niter, verbose=False)
    assert np.array_equal(mean0, mean0_in) and np.array_equal(cov0, cov0_in)
    assert [call for call, _ in eng.draws] == list(range(niter + 1))
    for call, Z in eng.draws:
        for k in range(K):
            assert np.array_equal(Z[k], ref.draw(seed_of(keys[k], last=False), call, B, D))
    assert [s for s in eng.calls if isinstance(s, tuple)] == [("step", i + 1, i < niter) for i in range(niter + 1)]
    assert [s["t"] for s in eng.steps] == list(range(1, niter + 2))
    mo, co, lo = ref.fit(keys, fit.lp, fit.lp_g, 0.05, mean0, cov0, B, niter)
    assert np.array_equal(m, mo) and np.array_equal(c, co) and np.array_equal(losses, lo)
    assert losses.shape == (niter + 1, K) and isinstance(losses, np.ndarray)


def test_forced_z_replaces_the_stream():
    K, D, B, niter = 2, 5, 3, 6
    keys = [11, 12]
    fit, ms, Ps = _fit(K, D)
    ma, ca, la = fit.fit(keys, Adam(0.1), batch_size=B, niter=niter, verbose=False)
    Zs = np.stack([np.stack([ref.draw(keys[k], i, B, D) for k in range(K)]) for i in range(niter + 1)])
    eng = OracleBatchedADVIEngine()
    fit2, _, _ = _fit(K, D, eng)
    mb, cb, lb = fit2.fit(keys, Adam(0.1), batch_size=B, niter=niter, verbose=False, forced_z=Zs)
    assert eng.draws == [] and "batched_seeds" not in eng.calls
    assert np.array_equal(ma, mb) and np.array_equal(ca, cb) and np.array_equal(la, lb)
    other = np.random.RandomState(0).standard_normal(Zs.shape)
    mc, cc, lc = fit2.fit(keys, Adam(0.1), batch_size=B, niter=niter, verbose=False, forced_z=other)
    mo, co, lo = ref.fit(keys, fit.lp, fit.lp_g, 0.1, np.zeros((K, D)), np.stack([np.eye(D)] * K), B, niter, forced_z=other)
    assert np.array_equal(mc, mo) and np.array_equal(cc, co) and np.array_equal(lc, lo)


def test_lr_forms():
    K, D, B, niter = 3, 4, 2, 5
    keys = [1, 2, 3]
    z0, e = np.zeros((K, D)), np.stack([np.eye(D)] * K)
    # K values
    eng = OracleBatchedADVIEngine()
    fit, _, _ = _fit(K, D, eng)
    lrs = np.array([0.01, 0.1, 0.5])
    m, c, l = fit.fit(keys, Adam(lrs, b1=0.8, b2=0.99, eps=1e-6), batch_size=B, niter=niter, verbose=False)
    mo, co, lo = ref.fit(keys, fit.lp, fit.lp_g, lrs, z0, e, B, niter, b1=0.8, b2=0.99, eps=1e-6)
    assert np.array_equal(m, mo) and np.array_equal(c, co) and np.array_equal(l, lo)
    assert all(np.array_equal(s["lr"], lrs) and (s["b1"], s["b2"], s["eps"]) == (0.8, 0.99, 1e-6) for s in eng.steps)
    assert eng.calls.count("batched_regs") == niter + 1
    # each problem with its own lr is that problem fitted alone
    for k in range(K):
        fk = ADVIBatch(1, D, None, lambda X, k=k: fit.lp_g(np.repeat(X, K, 0))[k:k + 1], engine=OracleBatchedADVIEngine())
        mk, ck, lk = fk.fit([keys[k]], Adam(float(lrs[k]), b1=0.8, b2=0.99, eps=1e-6), batch_size=B, niter=niter, verbose=False)
        assert np.array_equal(mk[0], m[k]) and np.array_equal(ck[0], c[k]) and lk is None
    # a schedule: asked once per iteration, floats or K values
    asked = []

    def sched(i):
        asked.append(i)
        return 0.1 / (1 + i) if i % 2 else [0.1 / (1 + i)] * K

    eng = OracleBatchedADVIEngine()
    fit, _, _ = _fit(K, D, eng)
    m, c, l = fit.fit(keys, Adam(sched), batch_size=B, niter=niter, verbose=False)
    assert asked == list(range(niter + 1))
    mo, co, lo = ref.fit(keys, fit.lp, fit.lp_g, lambda i: 0.1 / (1 + i), z0, e, B, niter)
    assert np.array_equal(m, mo) and np.array_equal(c, co) and np.array_equal(l, lo)
    # a scalar float reaches the engine as a float
    eng = OracleBatchedADVIEngine()
    fit, _, _ = _fit(K, D, eng)
    fit.fit(keys, Adam(0.25), batch_size=B, niter=2, verbose=False)
    assert all(s["lr"].shape == () and float(s["lr"]) == 0.25 for s in eng.steps) and "batched_regs" not in eng.calls


def test_monitor_cadence_nevals_and_the_fit_is_left_alone(capsys):
    K, D, B, niter, ck = 3, 4, 2, 23, 5
    keys = [5, 6, 7]
    fit, _, _ = _fit(K, D)
    m0, c0, l0 = fit.fit(keys, Adam(0.05), batch_size=B, niter=niter, verbose=False)
    mon = _Recorder(ck)
    eng = OracleBatchedADVIEngine()
    fit2, _, _ = _fit(K, D, eng)
    m1, c1, l1 = fit2.fit(keys, Adam(0.05), None, None, B, niter, 4, mon, verbose=True)      # the reference's positional order
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1) and np.array_equal(l0, l1)
    assert [s[0] for s in mon.seen] == [0, 5, 10, 15, 20, 23]
    assert [s[3] for s in mon.seen] == [1, 5 * B, 5 * B, 5 * B, 5 * B, 4 * B]                # 1 + i B evaluations in all
    assert np.cumsum([s[3] for s in mon.seen]).tolist() == [1 + i * B for i in (0, 5, 10, 15, 20)] + [1 + (niter + 1) * B]
    assert eng.calls.count("cov") == len(mon.seen) + 1                                       # formed only at a checkpoint
    assert np.array_equal(mon.seen[-1][1], m1) and np.array_equal(mon.seen[-1][2], c1)
    assert np.array_equal(mon.seen[0][1], np.zeros((K, D))) and np.array_equal(mon.seen[0][2], np.stack([np.eye(D)] * K))
    # the state handed over at checkpoint 10 is the fit after 10 steps
    m10, c10, _ = _fit(K, D)[0].fit(keys, Adam(0.05), batch_size=B, niter=9, verbose=False)
    assert np.array_equal(mon.seen[2][1], m10) and np.array_equal(mon.seen[2][2], c10)
    out = capsys.readouterr().out
    assert out.count("Iteration ") == 5 and "Revert" not in out                              # every 23 // 4 = 5: 0, 5, ..., 20


def test_single_problem_monitors_are_refused():
    fit, _, _ = _fit(2, 3)
    with pytest.raises(TypeError, match="monitor"):
        fit.fit([1, 2], Adam(0.1), niter=2, verbose=False, monitor=KLMonitor(batch_size_kl=4, checkpoint=1))
    with pytest.raises(TypeError, match="monitor"):
        fit.fit([1, 2], Adam(0.1), niter=2, verbose=False, monitor=object())
    with pytest.raises(TypeError, match="Adam"):
        fit.fit([1, 2], lambda p: None, niter=2, verbose=False)
    assert fit._engine.calls == []


def test_track_loss_false_never_calls_lp_and_lp_forms():
    K, D, B, niter = 2, 3, 4, 5
    ms, Ps = ref.gaussian_targets(K, D)
    calls = []

    def lp(X):
        calls.append(type(X))
        return ref.gaussian_lp(ms, Ps)(X)

    fit = ADVIBatch(K, D, lp, ref.gaussian_score(ms, Ps), engine=OracleBatchedADVIEngine())
    m0, c0, l0 = fit.fit([1, 2], Adam(0.1), batch_size=B, niter=niter, verbose=False, track_loss=False)
    assert l0 is None and calls == []
    m1, c1, l1 = fit.fit([1, 2], Adam(0.1), batch_size=B, niter=niter, verbose=False)
    assert len(calls) == niter + 1 and l1.shape == (niter + 1, K)
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)

    def lp_rows(X):                                                  # (K, rows) values instead of (K,) sums
        r = ms[:, None, :] - np.asarray(X)
        return -0.5 * np.einsum("kbi,kij,kbj->kb", r, Ps, r)

    _, _, l2 = ADVIBatch(K, D, lp_rows, ref.gaussian_score(ms, Ps), engine=OracleBatchedADVIEngine()).fit(
        [1, 2], Adam(0.1), batch_size=B, niter=niter, verbose=False)
    assert rel_err(l2, l1) < 1e-14
    _, _, l3 = ADVIBatch(K, D, None, ref.gaussian_score(ms, Ps), engine=OracleBatchedADVIEngine()).fit(
        [1, 2], Adam(0.1), batch_size=B, niter=niter, verbose=False)
    assert l3 is None
    with pytest.raises(ValueError, match="lp returned shape"):
        ADVIBatch(K, D, lambda X: np.zeros(K + 1), ref.gaussian_score(ms, Ps), engine=OracleBatchedADVIEngine()).fit(
            [1, 2], Adam(0.1), batch_size=B, niter=niter, verbose=False)


def test_nan_score_poisons_one_problem_alone():
    K, D, B, niter, bad = 4, 5, 2, 8, 2
    keys = [11, 12, 13, 14]
    fit, ms, Ps = _fit(K, D, seed=2)
    clean = fit.lp_g
    n = [0]

    def poisoned(X):
        G = clean(X)
        if n[0] >= 3:
            G[bad] = np.nan
        n[0] += 1
        return G

    m_ref, c_ref, l_ref = fit.fit(keys, Adam(0.05), batch_size=B, niter=niter, verbose=False)
    m, c, l = ADVIBatch(K, D, fit.lp, poisoned, engine=OracleBatchedADVIEngine()).fit(keys, Adam(0.05), batch_size=B, niter=niter,
                                                                                      verbose=False)
    others = [k for k in range(K) if k != bad]
    assert np.isnan(m[bad]).all() and np.isnan(c[bad]).all() and np.isnan(l[4:, bad]).all()
    assert np.array_equal(l[:4, bad], l_ref[:4, bad])
    assert np.array_equal(m[others], m_ref[others]) and np.array_equal(c[others], c_ref[others])
    assert np.array_equal(l[:, others], l_ref[:, others])


def test_non_pd_initial_covariance_names_the_problem():
    K, D = 5, 3
    cov = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    cov[1, 0, 0] = -1.0
    cov[3] = np.nan
    with pytest.raises(ValueError, match=r"\[1, 3\]"):
        ADVIBatch(K, D, None, lambda X: -X, engine=OracleBatchedADVIEngine()).fit(range(K), Adam(0.1), cov=cov, niter=3,
                                                                                 verbose=False)


def test_bound_and_shape_errors_come_before_any_engine_call():
    eng = OracleBatchedADVIEngine()
    with pytest.raises(ValueError, match="D = 65"):
        ADVIBatch(2, 65, None, lambda X: -X, engine=eng)
    with pytest.raises(ValueError, match="D = 0"):
        ADVIBatch(2, 0, None, lambda X: -X, engine=eng)
    with pytest.raises(ValueError, match="K = 0"):
        ADVIBatch(0, 4, None, lambda X: -X, engine=eng)
    fit = ADVIBatch(2, 4, None, lambda X: -X, engine=eng)
    opt = Adam(0.1)
    with pytest.raises(ValueError, match="B = 33"):
        fit.fit([1, 2], opt, batch_size=33, niter=2, verbose=False)
    with pytest.raises(ValueError, match="B = 0"):
        fit.fit([1, 2], opt, batch_size=0, niter=2, verbose=False)
    with pytest.raises(ValueError, match="3 keys"):
        fit.fit([1, 2, 3], opt, niter=2, verbose=False)
    with pytest.raises(ValueError, match="lr has 3 values"):
        fit.fit([1, 2], Adam([0.1, 0.2, 0.3]), niter=2, verbose=False)
    with pytest.raises(ValueError, match="lr has 3 values"):
        fit.fit([1, 2], Adam(lambda i: np.ones(3)), niter=2, verbose=False)
    with pytest.raises(AssertionError):
        fit.fit([1, 2], opt, mean=np.zeros((2, 5)), niter=2, verbose=False)
    with pytest.raises(AssertionError):
        fit.fit([1, 2], opt, cov=np.zeros((2, 4, 3)), niter=2, verbose=False)
    with pytest.raises(AssertionError):
        fit.fit([1, 2], opt, niter=2, batch_size=2, forced_z=np.zeros((2, 2, 2, 4)), verbose=False)
    with pytest.raises(ValueError, match="b1"):
        Adam(0.1, b1=1.0)
    with pytest.raises(ValueError, match="eps"):
        Adam(0.1, eps=-1.0)
    assert eng.calls == []


def test_score_exceptions_propagate():
    def boom(X):
        raise RuntimeError("score failed")

    with pytest.raises(RuntimeError, match="score failed"):
        ADVIBatch(2, 3, None, boom, engine=OracleBatchedADVIEngine()).fit([1, 2], Adam(0.1), niter=3, verbose=False)
