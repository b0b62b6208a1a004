"""Batched KL monitor without a GPU: the C ABI declarations and argument checks, and the host logic of BatchedKLMonitor and of
the batched fits' monitor cadence, driven by an oracle-backed batched engine defined here that restates the two monitor
entry points in numpy (Cholesky, the device draw stream through oracle.gsm_oracle.philox_randn, the whitening)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gsmvi_amd import _lib
from gsmvi_amd.batched import BaMBatch, GSMBatch
from gsmvi_amd.monitors import BatchedKLMonitor, DeviceKLMonitor, KLMonitor, mvn_logpdf
from oracle import gsm_oracle as orc
from test_batched_cpu import OracleBatchedEngine, _batched_score, _targets
from test_bam_batched_cpu import OracleBatchedBaMEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gsmvi_kl_draw_batched_f64", "gsmvi_logq_batched_f64"]
LOG2PI = np.log(2 * np.pi)


def test_batched_kl_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        for mp in ("exports.map", "exports_debug.map"):
            assert re.search(r"^\s*" + name + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), (mp, name)
        assert name in _lib.exported_symbols() and name in built, name
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED_KL\s+0x8000u", hdr)
    mask = re.search(r"#define\s+GSMVI_PATH_GENERIC_MASK\s+\(([^)]*)\)", hdr).group(1)
    assert "0x8000" not in mask
    assert "#define GSMVI_ABI_VERSION 1" in hdr
    from gsmvi_amd.engine import HipEngine
    assert HipEngine.PATH_BITS["batched_kl"] == 0x8000 and not HipEngine.PATH_GENERIC_MASK & 0x8000


def test_abi_checks_arguments_before_the_context():
    """every bad argument is reported with a NULL context (no device work can have started); valid ones end at the context"""
    lib = _lib.load_library()
    buf = (C.c_double * 8192)()
    p = C.cast(buf, C.c_void_p).value
    mean, cov, seeds, X, lq, info = p, p + 8 * 256, p + 8 * 2048, p + 8 * 2304, p + 8 * 6400, p + 8 * 6656
    err = lambda: (lib.gsmvi_last_error() or b"").decode()

    def draw(K=2, D=4, nc=3, s0=0, mean=mean, cov=cov, seeds=seeds, X=X, lq=lq, info=info):
        return lib.gsmvi_kl_draw_batched_f64(None, None, K, D, nc, s0, mean, cov, seeds, 0, X, lq, info)

    def evalq(K=2, D=4, nc=3, mean=mean, cov=cov, Y=X, lq=lq, info=info):
        return lib.gsmvi_logq_batched_f64(None, None, K, D, nc, mean, cov, Y, lq, info)

    for f in (draw, evalq):
        assert f(D=0) == 1 and "D must be" in err()
        assert f(D=65) == 1 and "D must be" in err()
        assert f(K=0) == 1 and "K must be" in err()
        assert f(nc=0) == 1 and "nc must be" in err()
        assert f(mean=None) == 1 and "NULL array" in err()
        assert f(cov=None) == 1 and "NULL array" in err()
        assert f(lq=None) == 1 and "NULL array" in err()
        assert f(info=None) == 1 and "NULL array" in err()
        assert f(lq=mean) == 1 and "overlap" in err()                 # an output over an input
        assert f(info=lq + 8) == 1 and "overlap" in err()              # the outputs over each other
        assert f(info=cov + 8) == 1 and "overlap" in err()
        assert f() == 1 and "ctx is NULL" in err()
    assert draw(seeds=None) == 1 and "NULL array" in err()
    assert draw(X=None) == 1 and "NULL array" in err()
    assert draw(X=cov) == 1 and "overlap" in err()
    assert draw(X=seeds - 8) == 1 and "overlap" in err()              # X over the keys
    assert draw(lq=X + 8) == 1 and "overlap" in err()                 # logq inside X
    assert draw(s0=-1) == 1 and "s0" in err()
    assert evalq(Y=None) == 1 and "NULL array" in err()
    assert evalq(lq=X + 8) == 1 and "overlap" in err()                # logq inside Y


class KLEngineMixin:
    """The two monitor entry points restated in numpy: R_k = chol(cov_k)^T (upper); DRAW rows s0 .. s0 + nc - 1 of
    philox_randn(seed_k, call, .) in the plain layout (element s D + j), x = mean_k + z R_k; EVAL w = (y - mean_k) R_k^-1;
    logq_k = sum over the rows of -|z|^2 / 2 - sum log R_ii - D / 2 log 2 pi; a cov_k that is not positive definite gives NaN
    rows, NaN logq and info = 1.  ``chunks`` records every DRAW / EVAL call as (kind, call, s0, nc)."""

    def _kl_init(self):
        if not hasattr(self, "chunks"):
            self.chunks = []

    def _factor(self, cov):
        return np.linalg.cholesky(cov).T if orc.cov_is_good(cov) else None

    def kl_draw_batched(self, mean, cov, seeds, call, s0, nc, out=None, info=None):
        self._kl_init()
        self.chunks.append(("draw", call, s0, nc))
        K, D = mean.shape
        X, logq, inf = np.empty((K, nc, D)), np.empty(K), np.zeros(K, dtype=np.int64)
        for k in range(K):
            R = self._factor(np.asarray(cov[k]))
            if R is None:
                X[k], logq[k], inf[k] = np.nan, np.nan, 1
                continue
            Z = orc.philox_randn(int(seeds[k]), call, (s0 + nc) * D)[s0 * D:].reshape(nc, D)
            X[k] = mean[k][None, :] + Z @ R
            logq[k] = -0.5 * np.sum(Z * Z) - nc * (np.sum(np.log(np.diag(R))) + 0.5 * D * LOG2PI)
        return X, logq, inf

    def logq_batched(self, mean, cov, Y, out=None, info=None):
        self._kl_init()
        self.chunks.append(("eval", None, None, Y.shape[1]))
        K, nc, D = Y.shape
        logq, inf = np.empty(K), np.zeros(K, dtype=np.int64)
        for k in range(K):
            R = self._factor(np.asarray(cov[k]))
            if R is None:
                logq[k], inf[k] = np.nan, 1
                continue
            W = np.linalg.solve(R.T, (Y[k] - mean[k][None, :]).T)
            logq[k] = -0.5 * np.sum(W * W) - nc * (np.sum(np.log(np.diag(R))) + 0.5 * D * LOG2PI)
        return logq, inf

    def take_rows(self, A, idx):
        return np.ascontiguousarray(A[:, idx])


class KLEngine(KLEngineMixin, OracleBatchedEngine):
    name = "oracle-batched-kl(test-only)"


class KLBaMEngine(KLEngineMixin, OracleBatchedBaMEngine):
    name = "oracle-batched-bam-kl(test-only)"


def _gauss_lp(ms, covs):
    """normalised log N(x; m_k, cov_k), (K, rows) values"""
    def lp(X):
        X = np.asarray(X)
        return np.stack([mvn_logpdf(X[k], ms[k], covs[k]) for k in range(X.shape[0])])
    return lp


def _state(K, D, seed=0):
    rs = np.random.RandomState(seed)
    mean = rs.standard_normal((K, D))
    A = rs.standard_normal((K, D, D))
    cov = A @ np.swapaxes(A, 1, 2) + D * np.eye(D)
    return mean, cov


def _expected(mean, cov, lp, keys, n, call, ref=None, idx=None):
    """rkl_k, fkl_k restated from the definitions (DeviceKLMonitor's stream and seed rule per problem)"""
    K, D = mean.shape
    X = np.stack([mean[k] + orc.philox_randn((int(keys[k]) % 2 ** 32) ^ 0x5DEECE66D, call, n * D).reshape(n, D)
                  @ np.linalg.cholesky(cov[k]).T for k in range(K)])
    rkl = np.array([np.mean(mvn_logpdf(X[k], mean[k], cov[k])) for k in range(K)]) - np.mean(lp(X), axis=1)
    if ref is None:
        return rkl, np.full(K, np.nan)
    Y = ref[:, idx]
    return rkl, np.mean(lp(Y), axis=1) - np.array([np.mean(mvn_logpdf(Y[k], mean[k], cov[k])) for k in range(K)])


def test_monitor_restates_the_device_monitor_per_problem():
    K, D, n, N = 3, 5, 24, 50
    mean, cov = _state(K, D)
    ms, covs = _state(K, D, seed=1)
    lp = _gauss_lp(ms, covs)
    keys = [7, 2 ** 40 + 3, 12345]
    ref = np.random.RandomState(2).standard_normal((K, N, D))
    mon = BatchedKLMonitor(batch_size_kl=n, checkpoint=1, ref_samples=ref, engine=KLEngine())
    assert mon.batched and mon.device_native
    rs = np.random.RandomState(keys[0] % 2 ** 32)
    for c in range(2):
        assert mon(c, [mean, cov], lp, keys, nevals=4) is keys
        idx = rs.permutation(N)[:n]
        rkl, fkl = _expected(mean, cov, lp, keys, n, c, ref, idx)
        assert mon.rkl[c].shape == (K,) and mon.fkl[c].shape == (K,) and mon.rkl[c].dtype == np.float64
        np.testing.assert_allclose(mon.rkl[c], rkl, rtol=0, atol=1e-11)
        np.testing.assert_allclose(mon.fkl[c], fkl, rtol=0, atol=1e-11)
    assert mon.nevals == [4, 8]
    assert [ch[1] for ch in mon.engine.chunks if ch[0] == "draw"] == [0, 1]      # call number = the monitor's call count


def test_seeds_from_int_list_range_array_and_torch_keys():
    import torch
    K, D, n = 4, 3, 10
    mean, cov = _state(K, D)
    lp = _gauss_lp(*_state(K, D, seed=1))
    res = []
    for keys in ([5, 6, 7, 8], range(5, 9), np.array([5, 6, 7, 8]), torch.tensor([5, 6, 7, 8])):
        mon = BatchedKLMonitor(batch_size_kl=n, engine=KLEngine())
        mon(0, [mean, cov], lp, keys)
        res.append(mon.rkl[0])
        assert np.isnan(mon.fkl[0]).all() and mon.fkl[0].shape == (K,)
    for r in res[1:]:
        assert np.array_equal(r, res[0])
    np.testing.assert_allclose(res[0], _expected(mean, cov, lp, [5, 6, 7, 8], n, 0)[0], rtol=0, atol=1e-11)
    # the seed rule of DeviceKLMonitor: (key % 2^32) ^ 0x5DEECE66D -- keys equal modulo 2^32 draw the same rows
    mon = BatchedKLMonitor(batch_size_kl=n, engine=KLEngine())
    mon(0, [mean, cov], lp, [5 + 2 ** 32, 6, 7 + 2 ** 33, 8])
    assert np.array_equal(mon.rkl[0], res[0])


@pytest.mark.parametrize("chunk", [1, 7, 24, 128])
def test_chunks_cover_batch_size_kl_exactly(chunk):
    K, D, n, N = 2, 4, 24, 40
    mean, cov = _state(K, D)
    lp = _gauss_lp(*_state(K, D, seed=1))
    ref = np.random.RandomState(2).standard_normal((K, N, D))
    eng = KLEngine()
    mon = BatchedKLMonitor(batch_size_kl=n, ref_samples=ref, engine=eng)
    mon._CHUNK = chunk
    mon(0, [mean, cov], lp, [1, 2])
    draws = [(s0, nc) for kind, _, s0, nc in eng.chunks if kind == "draw"]
    assert draws == [(s, min(chunk, n - s)) for s in range(0, n, chunk)]
    assert sum(nc for kind, _, _, nc in eng.chunks if kind == "eval") == n
    assert max(nc for *_, nc in eng.chunks) <= chunk
    whole = BatchedKLMonitor(batch_size_kl=n, ref_samples=ref, engine=KLEngine())
    whole(0, [mean, cov], lp, [1, 2])
    np.testing.assert_allclose(mon.rkl[0], whole.rkl[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(mon.fkl[0], whole.fkl[0], rtol=0, atol=1e-12)


def test_lp_may_return_sums_or_values_per_row():
    K, D, n = 3, 4, 9
    mean, cov = _state(K, D)
    lp_rows = _gauss_lp(*_state(K, D, seed=1))
    lp_sums = lambda X: lp_rows(X).sum(axis=1)                  # noqa: E731
    ref = np.random.RandomState(2).standard_normal((K, 30, D))
    a = BatchedKLMonitor(batch_size_kl=n, ref_samples=ref, engine=KLEngine())
    b = BatchedKLMonitor(batch_size_kl=n, ref_samples=ref, engine=KLEngine())
    a(0, [mean, cov], lp_rows, [1, 2, 3])
    b(0, [mean, cov], lp_sums, [1, 2, 3])
    np.testing.assert_allclose(a.rkl[0], b.rkl[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(a.fkl[0], b.fkl[0], rtol=0, atol=1e-12)


def test_non_pd_covariance_gives_nan_for_its_problem_alone():
    K, D, n = 3, 4, 9
    mean, cov = _state(K, D)
    lp = _gauss_lp(*_state(K, D, seed=1))
    ref = np.random.RandomState(2).standard_normal((K, 30, D))
    bad = cov.copy()
    bad[1] = -np.eye(D)
    a = BatchedKLMonitor(batch_size_kl=n, ref_samples=ref, engine=KLEngine())
    b = BatchedKLMonitor(batch_size_kl=n, ref_samples=ref, engine=KLEngine())
    with np.errstate(invalid="ignore"):
        a(0, [mean, bad], lambda X: np.nan_to_num(lp(X)), [1, 2, 3])
    b(0, [mean, cov], lp, [1, 2, 3])
    assert np.isnan(a.rkl[0][1]) and np.isnan(a.fkl[0][1])
    assert np.array_equal(a.rkl[0][[0, 2]], b.rkl[0][[0, 2]]) and np.array_equal(a.fkl[0][[0, 2]], b.fkl[0][[0, 2]])


def test_shape_and_bound_errors_come_before_any_engine_call():
    eng = KLEngine()
    mean, cov = _state(2, 4)
    lp = lambda X: np.zeros(X.shape[:2])                        # noqa: E731
    mon = BatchedKLMonitor(engine=eng)
    with pytest.raises(ValueError, match="D = 65"):
        mon(0, [np.zeros((2, 65)), np.zeros((2, 65, 65))], lp, [1, 2])
    with pytest.raises(ValueError, match="D = 0"):
        mon(0, [np.zeros((2, 0)), np.zeros((2, 0, 0))], lp, [1, 2])
    with pytest.raises(ValueError, match="keys"):
        mon(0, [mean, cov], lp, [1, 2, 3])
    with pytest.raises(ValueError, match="cov"):
        mon(0, [mean, cov[:, :3]], lp, [1, 2])
    with pytest.raises(ValueError, match="ref_samples"):
        BatchedKLMonitor(ref_samples=np.zeros((3, 10, 4)), engine=eng)(0, [mean, cov], lp, [1, 2])
    with pytest.raises(ValueError, match="ref_samples"):
        BatchedKLMonitor(ref_samples=np.zeros((2, 10)), engine=eng)(0, [mean, cov], lp, [1, 2])
    assert eng.calls == [] and getattr(eng, "chunks", []) == [] and mon.rkl == [] and mon.nevals == []


class _Recording(BatchedKLMonitor):
    def __call__(self, i, params, lp, keys, nevals=1):
        self.__dict__.setdefault("iters", []).append(i)
        return super().__call__(i, params, lp, keys, nevals=nevals)


def _gsm_setup(K=3, D=4):
    ms, Ps = _targets(K, D)
    covs = np.linalg.inv(Ps)
    return ms, Ps, _gauss_lp(ms, covs)


@pytest.mark.parametrize("offset", [0, 100])
def test_cadence_and_nevals_in_the_gsm_fit(offset):
    K, D, B, niter, ck = 3, 4, 2, 7, 3
    ms, Ps, lp = _gsm_setup(K, D)
    mon = _Recording(batch_size_kl=6, checkpoint=ck, offset_evals=offset, engine=KLEngine())
    GSMBatch(K, D, lp, _batched_score(ms, Ps), engine=mon.engine).fit([4, 5, 6], batch_size=B, niter=niter, verbose=False,
                                                                      monitor=mon)
    assert mon.iters == [0, 3, 6, 7]                            # i % checkpoint == 0 before the score, then once after the loop
    assert mon.nevals == [offset + n for n in (1, 1 + 3 * B, 1 + 6 * B, 1 + 8 * B)]
    assert len(mon.rkl) == 4 and all(r.shape == (K,) and np.isfinite(r).all() for r in mon.rkl)
    mon.reset()
    assert mon.rkl == [] and mon.fkl == [] and mon.nevals == [] and mon.offset_evals == offset + 1 + 8 * B
    mon.reset(offset_evals=5, checkpoint=2)
    mon(0, [ms, np.linalg.inv(Ps)], lp, [4, 5, 6], nevals=3)
    assert mon.nevals == [8] and mon.checkpoint == 2


def test_cadence_in_the_bam_fit():
    K, D, B, niter, ck = 2, 4, 3, 5, 2
    ms, Ps, lp = _gsm_setup(K, D)
    mon = _Recording(batch_size_kl=4, checkpoint=ck, engine=KLBaMEngine())
    BaMBatch(K, D, lp, _batched_score(ms, Ps), engine=mon.engine).fit([1, 2], lambda i: 2.0, batch_size=B, niter=niter,
                                                                      verbose=False, monitor=mon)
    assert mon.iters == [0, 2, 4, 5]
    assert mon.nevals == [1, 1 + 2 * B, 1 + 4 * B, 1 + 6 * B]


@pytest.mark.parametrize("which", ["gsm", "bam"])
def test_the_monitor_leaves_the_fit_alone(which):
    K, D, B, niter = 3, 4, 2, 9
    ms, Ps, lp = _gsm_setup(K, D)
    ref = np.random.RandomState(2).standard_normal((K, 20, D))

    def run(monitor):
        if which == "gsm":
            eng = KLEngine()
            return GSMBatch(K, D, lp, _batched_score(ms, Ps), engine=eng).fit([4, 5, 6], batch_size=B, niter=niter,
                                                                              verbose=False, monitor=monitor)
        eng = KLBaMEngine()
        return BaMBatch(K, D, lp, _batched_score(ms, Ps), engine=eng).fit([4, 5, 6], lambda i: 3.0, batch_size=B,
                                                                          niter=niter, verbose=False, monitor=monitor)
    m0, c0 = run(None)
    m1, c1 = run(BatchedKLMonitor(batch_size_kl=5, checkpoint=2, ref_samples=ref, engine=KLEngine()))
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)


def test_lp_exception_appends_nan_and_the_fit_goes_on(capsys):
    K, D, B, niter = 3, 4, 2, 6
    ms, Ps, lp = _gsm_setup(K, D)
    n_calls = []

    def flaky(X):
        n_calls.append(1)
        if len(n_calls) == 2:
            raise ZeroDivisionError("boom")
        return lp(X)
    mon = BatchedKLMonitor(batch_size_kl=4, checkpoint=3, engine=KLEngine())
    m, c = GSMBatch(K, D, flaky, _batched_score(ms, Ps), engine=mon.engine).fit([4, 5, 6], batch_size=B, niter=niter,
                                                                                verbose=False, monitor=mon)
    assert "Exception occured in monitor : boom" in capsys.readouterr().out
    assert len(mon.rkl) == 4 and np.isnan(mon.rkl[1]).all() and np.isnan(mon.fkl[1]).all()
    assert all(np.isfinite(mon.rkl[j]).all() for j in (0, 2, 3))
    assert mon.nevals == [1, 1 + 3 * B, 1 + 6 * B, 1 + 7 * B] and np.isfinite(m).all()


@pytest.mark.parametrize("monitor", [object(), KLMonitor(), DeviceKLMonitor()], ids=["object", "KLMonitor", "DeviceKLMonitor"])
def test_single_problem_monitors_are_refused_by_both_fits(monitor):
    K, D = 2, 4
    eng = KLEngine()
    with pytest.raises(TypeError, match="monitor.*BatchedKLMonitor"):
        GSMBatch(K, D, None, lambda X: -X, engine=eng).fit([1, 2], niter=2, verbose=False, monitor=monitor)
    beng = KLBaMEngine()
    with pytest.raises(TypeError, match="monitor.*BatchedKLMonitor"):
        BaMBatch(K, D, None, lambda X: -X, engine=beng).fit([1, 2], lambda i: 1.0, niter=2, verbose=False, monitor=monitor)
    assert eng.calls == [] and beng.calls == []
