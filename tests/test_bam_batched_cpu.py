"""Batched BaM without a GPU: the C ABI declarations and argument checks, and the host logic of BaMBatch.fit driven by an
oracle-backed batched engine of tests/engines.py: seeds and draw calls, the regulariser
calls, per-problem reverts, bounds and shape errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gsmvi_amd.batched import BaMBatch, bam_update_batched, bam_lowrank_update_batched
from gsmvi_amd.bam import Regularizers
from gsmvi_amd._fitloop import seed_of
from gsmvi_amd import _lib
from oracle import gsm_oracle as orc
from oracle import bam_oracle as borc
from engines import OracleBatchedBaMEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gsmvi_bam_update_batched_f64", "gsmvi_bam_fit_step_batched_f64"]


def test_batched_bam_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        for mp in ("exports.map", "exports_debug.map"):
            assert re.search(r"^\s*" + name + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), (mp, name)
        assert name in _lib.exported_symbols() and name in built, name
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_BAM\s+0x4000u", hdr)
    mask = re.search(r"#define\s+GSMVI_PATH_GENERIC_MASK\s+\(([^)]*)\)", hdr).group(1)
    assert "0x4000" not in mask
    assert "#define GSMVI_ABI_VERSION 1" in hdr
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_bam"] == 0x4000 and not HipEngine.PATH_GENERIC_MASK & 0x4000


def test_abi_checks_arguments_before_the_context_and_names_overlapping_arrays():
    """every bad argument is reported with a NULL context (no device work can have started); valid ones end at the context;
    an overlap is reported with the names of both arrays"""
    lib = _lib.load_library()
    buf = (C.c_double * 4096)()
    p = C.cast(buf, C.c_void_p).value
    q = p + 8 * 2048
    err = lambda: (lib.gsmvi_last_error() or b"").decode()

    def upd(K, D, B, X=p, mu=q, reg_dev=None):
        return lib.gsmvi_bam_update_batched_f64(None, None, K, D, B, X, X, X, X, 1.0, reg_dev, 0.0, mu, mu + 8 * 64, None)

    def step(K, D, B, X=p, Xout=None, seeds=None, R=None):
        return lib.gsmvi_bam_fit_step_batched_f64(None, None, K, D, B, X, q, q + 8 * 128, q + 8 * 256, R, 1.0, None, 0.0,
                                                  None, None, seeds, 0, Xout)

    assert upd(1, 65, 2) == 1 and "D must be" in err()
    assert upd(1, 0, 2) == 1 and "D must be" in err()
    assert upd(1, 4, 33) == 1 and "B must be" in err()
    assert upd(0, 4, 2) == 1 and "K must be" in err()
    assert upd(1, 4, 2, X=None) == 1 and "NULL array" in err()
    assert upd(1, 4, 2, mu=p) == 1 and "overlap" in err()
    assert upd(1, 4, 2) == 1 and "ctx is NULL" in err()
    assert step(1, 65, 2) == 1 and "D must be" in err()
    assert step(2, 4, 2, seeds=p) == 1 and "sampling factor" in err()
    assert step(2, 4, 2, Xout=q) == 1 and "overlaps" in err()
    assert step(2, 4, 2, Xout=p) == 1 and "ctx is NULL" in err()     # Xout may equal X
    assert step(2, 4, 2) == 1 and "ctx is NULL" in err()
    # the int outputs and the read-only key / regulariser arrays are checked too
    ib, ib2 = (C.c_int * 64)(), (C.c_int * 64)()
    i1, i2 = C.cast(ib, C.c_void_p).value, C.cast(ib2, C.c_void_p).value

    def step2(info=None, nrev=None, seeds=None, reg_dev=None, R=None, Xout=None):
        return lib.gsmvi_bam_fit_step_batched_f64(None, None, 2, 4, 2, p, q, q + 8 * 128, q + 8 * 256, R, 1.0, reg_dev, 0.0,
                                                  info, nrev, seeds, 0, Xout)

    assert step2(info=i1, nrev=i2) == 1 and "ctx is NULL" in err()
    assert step2(info=q + 8 * 128) == 1 and "info_dev overlaps mean" in err()                # info inside mean
    assert step2(nrev=q + 8 * 256) == 1 and "n_reverts_dev overlaps cov" in err()            # n_reverts inside cov
    assert step2(info=i1, nrev=i1 + 4) == 1 and "n_reverts_dev overlaps info_dev" in err()   # the two counters overlap
    assert step2(reg_dev=q + 8 * 128) == 1 and "overlap" in err()
    assert step2(seeds=q + 8 * 256, R=q + 8 * 1024, Xout=p) == 1 and "cov overlaps seeds_dev" in err()
    assert upd(1, 4, 2) == 1
    assert lib.gsmvi_bam_update_batched_f64(None, None, 1, 4, 2, p, p, p, p, 1.0, None, 0.0, q, q + 8 * 64, p) == 1 \
        and "overlap" in err()                                          # info over an input


def _targets(K, D, seed=0):
    ms, Ps = [], []
    for k in range(K):
        m, _, P = orc.make_gaussian_target(D, 100 * seed + k)
        ms.append(m)
        Ps.append(P)
    return np.array(ms), np.array(Ps)


def _batched_score(ms, Ps):
    def lp_g(X):
        return np.stack([orc.gaussian_score(X[k], ms[k], Ps[k]) for k in range(X.shape[0])])
    return lp_g


@pytest.mark.parametrize("D,B", [(4, 2), (5, 2), (3, 5)])
def test_draws_are_each_problems_device_stream(D, B):
    """problem k draws call i of seed_of(keys[k], last=True) at iteration i (BaM.fit's seed), the padded layout for odd D"""
    K, niter = 3, 6
    keys = [7, 2 ** 40 + 3, 12345]
    ms, Ps = _targets(K, D)
    eng = OracleBatchedBaMEngine()
    BaMBatch(K, D, None, _batched_score(ms, Ps), engine=eng).fit(keys, lambda i: 5.0, batch_size=B, niter=niter,
                                                                verbose=False)
    assert len(eng.draws) == K * (niter + 1)
    Dz = D + (D & 1)
    for n, (seed, call, Z) in enumerate(eng.draws):
        k, i = n % K, n // K
        assert seed == seed_of(keys[k], last=True) and call == i
        assert np.array_equal(Z, orc.philox_randn(seed_of(keys[k], last=True), i, B * Dz).reshape(B, Dz)[:, :D])
    steps = [c for c in eng.calls if isinstance(c, tuple)]
    assert steps == [("step", i + 1, i < niter) for i in range(niter + 1)]


@pytest.mark.parametrize("D,B", [(6, 3), (5, 2), (3, 6)])
def test_each_problem_is_the_reference_loop_on_its_samples(D, B):
    """problem k equals bam_oracle.bam_fit (default update, jitter 1e-6) forced with the samples it was given, bit for bit"""
    K, niter = 4, 15
    keys = np.array([3, 99, 1000, 5])
    ms, Ps = _targets(K, D, seed=1)
    mean0 = np.random.RandomState(0).standard_normal((K, D))
    eng = OracleBatchedBaMEngine()
    mb, cb = BaMBatch(K, D, None, _batched_score(ms, Ps), engine=eng).fit(
        keys, Regularizers().custom(lambda c: 100.0 / c), mean=mean0, batch_size=B, niter=niter, verbose=False)
    seen = np.array(eng.seen)
    assert seen.shape == (niter + 1, K, B, D)
    for k in range(K):
        mo, co = borc.bam_fit(D, None, lambda x, k=k: orc.gaussian_score(x, ms[k], Ps[k]), 0,
                              borc.Regularizers().custom(lambda c: 100.0 / c), mean=mean0[k], batch_size=B, niter=niter,
                              forced_samples=seen[:, k], jitter=1e-6)
        assert np.array_equal(mb[k], mo) and np.array_equal(cb[k], co), k


def test_regf_is_called_once_per_iteration_and_may_give_one_value_per_problem():
    K, D, B, niter = 3, 4, 2, 7
    ms, Ps = _targets(K, D, seed=4)
    calls = []

    def regf(i):
        calls.append(i)
        return np.array([1.0, 10.0, 100.0]) / (1 + i)

    eng = OracleBatchedBaMEngine()
    m, c = BaMBatch(K, D, None, _batched_score(ms, Ps), engine=eng).fit(range(K), regf, batch_size=B, niter=niter,
                                                                       verbose=False)
    assert calls == list(range(niter + 1))
    assert all(np.array_equal(r, np.array([1.0, 10.0, 100.0]) / (1 + i)) for i, r in enumerate(eng.regs))
    # each problem is its own reference loop with its own schedule
    seen = np.array(eng.seen)
    for k in range(K):
        mo, co = borc.bam_fit(D, None, lambda x, k=k: orc.gaussian_score(x, ms[k], Ps[k]), 0,
                              lambda i, k=k: [1.0, 10.0, 100.0][k] / (1 + i), batch_size=B, niter=niter,
                              forced_samples=seen[:, k], jitter=1e-6)
        assert np.array_equal(m[k], mo) and np.array_equal(c[k], co), k
    # a schedule of Regularizers counts calls: one per iteration, as in a single fit without retries
    r = Regularizers()
    eng = OracleBatchedBaMEngine()
    BaMBatch(K, D, None, _batched_score(ms, Ps), engine=eng).fit(range(K), r.linear(8.0), batch_size=B, niter=niter,
                                                                verbose=False)
    assert r.counter == niter + 1 and eng.regs == [8.0 / (i + 1) for i in range(niter + 1)]
    with pytest.raises(ValueError, match="2 values"):
        BaMBatch(K, D, None, _batched_score(ms, Ps), engine=OracleBatchedBaMEngine()).fit(
            range(K), lambda i: [1.0, 2.0], batch_size=B, niter=2, verbose=False)


def test_nan_score_reverts_one_problem_alone(capsys):
    K, D, B, niter, bad = 4, 5, 2, 12, 2
    keys = [11, 12, 13, 14]
    ms, Ps = _targets(K, D, seed=2)
    cov0 = np.stack([np.eye(D) * (1.0 + 0.1 * k) for k in range(K)])
    mean0 = np.arange(K * D, dtype=np.float64).reshape(K, D) / 10.0
    clean = _batched_score(ms, Ps)

    def poisoned(X):
        G = clean(X)
        G[bad] = np.nan
        return G

    ref = BaMBatch(K, D, None, clean, engine=OracleBatchedBaMEngine())
    m_ref, c_ref = ref.fit(keys, lambda i: 20.0, mean=mean0, cov=cov0, batch_size=B, niter=niter, verbose=False)
    fit = BaMBatch(K, D, None, poisoned, engine=OracleBatchedBaMEngine())
    m, c = fit.fit(keys, lambda i: 20.0, mean=mean0, cov=cov0, batch_size=B, niter=niter, nprint=3, verbose=True)
    assert fit.n_reverts.tolist() == [0 if k != bad else niter + 1 for k in range(K)]
    assert ref.n_reverts.tolist() == [0] * K
    assert np.array_equal(m[bad], mean0[bad]) and np.array_equal(c[bad], cov0[bad])
    others = [k for k in range(K) if k != bad]
    assert np.array_equal(m[others], m_ref[others]) and np.array_equal(c[others], c_ref[others])
    out = capsys.readouterr().out
    counts = [int(n) for n in re.findall(r"Revert \((\d+) since last print\)", out)]
    assert sum(counts) == niter + 1 and out.count("Iteration ") == 4


def test_score_and_regf_exceptions_propagate():
    K, D = 2, 3
    eng = OracleBatchedBaMEngine()

    def boom(X):
        raise RuntimeError("score failed")

    with pytest.raises(RuntimeError, match="score failed"):
        BaMBatch(K, D, None, boom, engine=eng).fit([1, 2], lambda i: 1.0, niter=3, verbose=False)

    def bad_reg(i):
        raise KeyError("no reg")

    with pytest.raises(KeyError):
        BaMBatch(K, D, None, lambda X: -X, engine=OracleBatchedBaMEngine()).fit([1, 2], bad_reg, niter=3, verbose=False)


def test_non_pd_initial_covariance_names_the_problem():
    K, D = 5, 3
    cov = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    cov[1, 0, 0] = -1.0
    cov[3] = np.nan
    with pytest.raises(ValueError, match=r"\[1, 3\]"):
        BaMBatch(K, D, None, lambda X: -X, engine=OracleBatchedBaMEngine()).fit(range(K), lambda i: 1.0, cov=cov, niter=3,
                                                                                verbose=False)


def test_bound_and_shape_errors_come_before_any_engine_call():
    eng = OracleBatchedBaMEngine()
    with pytest.raises(ValueError, match="D = 65"):
        BaMBatch(2, 65, None, lambda X: -X, engine=eng)
    with pytest.raises(ValueError, match="D = 0"):
        BaMBatch(2, 0, None, lambda X: -X, engine=eng)
    with pytest.raises(ValueError, match="K = 0"):
        BaMBatch(0, 4, None, lambda X: -X, engine=eng)
    fit = BaMBatch(2, 4, None, lambda X: -X, engine=eng)
    rf = lambda i: 1.0
    with pytest.raises(ValueError, match="B = 33"):
        fit.fit([1, 2], rf, batch_size=33, niter=2, verbose=False)
    with pytest.raises(ValueError, match="B = 0"):
        fit.fit([1, 2], rf, batch_size=0, niter=2, verbose=False)
    with pytest.raises(ValueError, match="3 keys"):
        fit.fit([1, 2, 3], rf, niter=2, verbose=False)
    with pytest.raises(AssertionError):
        fit.fit([1, 2], rf, mean=np.zeros((2, 5)), niter=2, verbose=False)
    with pytest.raises(AssertionError):
        fit.fit([1, 2], rf, cov=np.zeros((2, 4, 3)), niter=2, verbose=False)
    with pytest.raises(AssertionError):
        fit.fit([1, 2], rf, niter=2, batch_size=2, forced_samples=np.zeros((2, 2, 2, 4)), verbose=False)
    with pytest.raises(TypeError, match="monitor"):
        fit.fit([1, 2], rf, niter=2, verbose=False, monitor=object())
    z = np.zeros
    with pytest.raises(ValueError, match="D = 65"):
        bam_update_batched(z((2, 2, 65)), z((2, 2, 65)), z((2, 65)), z((2, 65, 65)), 1.0, engine=eng)
    with pytest.raises(ValueError, match="B = 40"):
        bam_update_batched(z((2, 40, 4)), z((2, 40, 4)), z((2, 4)), z((2, 4, 4)), 1.0, engine=eng)
    with pytest.raises(ValueError, match="3 values"):
        bam_update_batched(z((2, 3, 4)), z((2, 3, 4)), z((2, 4)), z((2, 4, 4)), np.ones(3), engine=eng)
    with pytest.raises(AssertionError):
        bam_update_batched(z((2, 3, 4)), z((2, 3, 4)), z((3, 4)), z((2, 4, 4)), 1.0, engine=eng)
    with pytest.raises(AssertionError):
        bam_lowrank_update_batched(z((3, 4)), z((3, 4)), z(4), z((4, 4)), 1.0, engine=eng)
    assert eng.calls == []


def test_one_shot_is_the_per_problem_update():
    K, D, B = 3, 5, 7
    rs = np.random.RandomState(0)
    X, G, mu0 = rs.standard_normal((K, B, D)), rs.standard_normal((K, B, D)), rs.standard_normal((K, D))
    S0 = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    regs = np.array([0.5, 2.0, 9.0])
    for fn in (bam_update_batched, bam_lowrank_update_batched):
        mu, S = fn(X, G, mu0, S0, regs, jitter=1e-6, engine=OracleBatchedBaMEngine())
        for k in range(K):
            mo, So = borc.bam_lowrank_update_exact(X[k], G[k], mu0[k], S0[k], regs[k])
            assert np.array_equal(mu[k], mo) and np.array_equal(S[k], 0.5 * (So + So.T) + 1e-6 * np.eye(D))


def test_lds_budget_fits_every_in_bounds_shape():
    """the dynamic LDS every batched BaM launch requests (the library's own host arithmetic, read through the debug build's
    query in a child process) fits in 160 KiB for every (D, B) in bounds, with and without the padded strides; four problems
    share a workgroup only for D <= 16"""
    import json
    import sys
    code = (
        "import ctypes as C, json, sys\n"
        "lib = C.CDLL(sys.argv[1])\n"
        "f = lib.gsmvi_debug_bam_batched_lds\n"
        "f.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]\n"
        "out = {}\n"
        "for D in range(0, 66):\n"
        "    for B in range(0, 34):\n"
        "        for pad in (0, 1):\n"
        "            n, p = C.c_size_t(0), C.c_int(0)\n"
        "            st = f(D, B, pad, C.byref(n), C.byref(p))\n"
        "            out[f'{D},{B},{pad}'] = [st, n.value, p.value]\n"
        "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.library_path(debug=True)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for key, (st, nbytes, ppw) in got.items():
        D, B, pad = (int(x) for x in key.split(","))
        if not (1 <= D <= 64 and 1 <= B <= 32):
            assert st == 1, key                                  # GSMVI_ERR_BAD_ARG outside the bounds
            continue
        assert st == 0 and 0 < nbytes <= 160 * 1024, key
        assert ppw in (1, 4) and (ppw == 1 or D <= 16), key
        assert nbytes % (8 * ppw) == 0
        if pad == 0:
            assert nbytes <= got[f"{D},{B},1"][1] and ppw == got[f"{D},{B},1"][2], key
    assert got["64,32,1"][2] == 1 and got["10,2,1"][2] == 4 and got["16,32,1"][2] == 1
    assert max(v[1] for k, v in got.items() if v[0] == 0 and v[2] == 1) == got["64,32,1"][1]     # one problem: (64, 32)
