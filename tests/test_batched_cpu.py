"""Batched GSM without a GPU: the C ABI declarations, and the host logic of GSMBatch.fit driven by the oracle-backed batched
engine of tests/engines.py: seeds and draw calls, per-problem reverts, bounds and shape errors."""
import os
import re

import numpy as np
import pytest

from gsmvi_amd.batched import GSMBatch, gsm_update_batched
from gsmvi_amd.gsm import GSM
from gsmvi_amd._fitloop import seed_of
from gsmvi_amd import _lib
from oracle import gsm_oracle as orc
from engines import OracleBatchedEngine, OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gsmvi_gsm_update_batched_f64", "gsmvi_gsm_fit_init_batched_f64", "gsmvi_gsm_fit_step_batched_f64",
       "gsmvi_gaussian_score_batched_f64"]


def test_batched_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        for mp in ("exports.map", "exports_debug.map"):
            assert re.search(r"^\s*" + name + r";", open(os.path.join(ROOT, "gsm-vi_amd", "csrc", mp)).read(), re.M), (mp, name)
        assert name in _lib.exported_symbols()
    assert re.search(r"#define\s+GSMVI_PATH_BATCHED\s+0x2000u", hdr)
    assert "#define GSMVI_ABI_VERSION 1" in hdr


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


@pytest.mark.parametrize("D,B", [(4, 2), (5, 2), (3, 3)])
def test_draws_are_each_problems_device_stream(D, B):
    K, niter = 3, 6
    keys = [7, 2 ** 40 + 3, 12345]
    ms, Ps = _targets(K, D)
    eng = OracleBatchedEngine()
    GSMBatch(K, D, None, _batched_score(ms, Ps), engine=eng).fit(keys, batch_size=B, niter=niter, verbose=False)
    assert len(eng.draws) == K * (niter + 1)             # call 0 at the start, call i + 1 after iteration i, none after the last
    Dz = D + (D & 1)
    for n, (seed, call, Z) in enumerate(eng.draws):
        k, i = n % K, n // K
        assert seed == seed_of(keys[k], last=False) and call == i
        assert np.array_equal(Z, orc.philox_randn(seed_of(keys[k], last=False), i, B * Dz).reshape(B, Dz)[:, :D])
    steps = [c for c in eng.calls if isinstance(c, tuple)]
    assert steps == [("step", i + 1, i < niter) for i in range(niter + 1)]


def test_each_problem_equals_the_single_dense_fit():
    """even D (the single fit pads odd D only on the HIP engine): problem k is GSM.fit(keys[k], method="dense", rng="device")"""
    K, D, B, niter = 4, 6, 3, 20
    keys = np.array([3, 99, 1000, 5])
    ms, Ps = _targets(K, D, seed=1)
    mean0 = np.random.RandomState(0).standard_normal((K, D))
    mb, cb = GSMBatch(K, D, None, _batched_score(ms, Ps), engine=OracleBatchedEngine()).fit(
        keys, mean=mean0, batch_size=B, niter=niter, verbose=False)
    for k in range(K):
        g = GSM(D, None, lambda x, k=k: orc.gaussian_score(x, ms[k], Ps[k]), engine=OracleEngine())
        m1, c1 = g.fit(int(keys[k]), mean=mean0[k], batch_size=B, niter=niter, verbose=False, method="dense", rng="device")
        assert np.array_equal(mb[k], m1) and np.array_equal(cb[k], c1)


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

    ref = GSMBatch(K, D, None, clean, engine=OracleBatchedEngine())
    m_ref, c_ref = ref.fit(keys, mean=mean0, cov=cov0, batch_size=B, niter=niter, verbose=False)
    fit = GSMBatch(K, D, None, poisoned, engine=OracleBatchedEngine())
    m, c = fit.fit(keys, mean=mean0, cov=cov0, batch_size=B, niter=niter, nprint=3, verbose=True)
    assert fit.n_reverts.tolist() == [0 if k != bad else niter + 1 for k in range(K)]
    assert ref.n_reverts.tolist() == [0] * K
    assert np.array_equal(m[bad], mean0[bad]) and np.array_equal(c[bad], cov0[bad])
    others = [k for k in range(K) if k != bad]
    assert np.array_equal(m[others], m_ref[others]) and np.array_equal(c[others], c_ref[others])
    out = capsys.readouterr().out
    counts = [int(n) for n in re.findall(r"Revert \((\d+) since last print\)", out)]
    assert sum(counts) == niter + 1 and out.count("Iteration ") == 4


def _poisoned_at(score, iterations, rows=None):
    """``score`` with NaN (in ``rows`` of its leading axis, or everywhere) on the calls numbered in ``iterations``: a fit calls
    its score once per iteration"""
    count = [0]

    def lp_g(X):
        G = np.array(score(X), copy=True)
        if count[0] in iterations:
            G[slice(None) if rows is None else rows] = np.nan
        count[0] += 1
        return G
    return lp_g


def test_problem_reverts_and_recovers_like_the_single_fit():
    """The score of problem j is NaN at iterations 3, 4 and 10 only: each time it keeps its state and draws the next samples
    from the kept mean and factor, so it continues as the single dense fit with the same poisoned schedule does, bit for bit;
    the other problems never notice."""
    K, D, B, niter, j, when = 4, 6, 3, 20, 1, {3, 4, 10}
    keys = np.array([3, 99, 1000, 5])
    ms, Ps = _targets(K, D, seed=1)
    mean0 = np.random.RandomState(0).standard_normal((K, D))
    clean = _batched_score(ms, Ps)
    ref = GSMBatch(K, D, None, clean, engine=OracleBatchedEngine())
    m_ref, c_ref = ref.fit(keys, mean=mean0, batch_size=B, niter=niter, verbose=False)
    fit = GSMBatch(K, D, None, _poisoned_at(clean, when, rows=j), engine=OracleBatchedEngine())
    m, c = fit.fit(keys, mean=mean0, batch_size=B, niter=niter, verbose=False)
    assert ref.n_reverts.tolist() == [0] * K and fit.n_reverts.tolist() == [3 if k == j else 0 for k in range(K)]
    g = GSM(D, None, _poisoned_at(lambda x: orc.gaussian_score(x, ms[j], Ps[j]), when), engine=OracleEngine())
    m1, c1 = g.fit(int(keys[j]), mean=mean0[j], batch_size=B, niter=niter, verbose=False, method="dense", rng="device")
    assert g.n_reverts == 3
    assert np.array_equal(m[j], m1) and np.array_equal(c[j], c1)
    assert not np.array_equal(m[j], m_ref[j])                 # the schedule changed the problem's trajectory
    others = [k for k in range(K) if k != j]
    assert np.array_equal(m[others], m_ref[others]) and np.array_equal(c[others], c_ref[others])


def test_forced_samples_take_no_draws():
    K, D, B, niter = 2, 5, 2, 4
    ms, Ps = _targets(K, D, seed=3)
    forced = np.random.RandomState(1).standard_normal((niter + 1, K, B, D))
    eng = OracleBatchedEngine()
    m, c = GSMBatch(K, D, None, _batched_score(ms, Ps), engine=eng).fit([1, 2], batch_size=B, niter=niter, verbose=False,
                                                                       forced_samples=forced)
    assert eng.draws == [] and all(c_[2] is False for c_ in eng.calls if isinstance(c_, tuple))
    for k in range(K):
        mo, co = orc.gsm_fit(D, None, lambda x, k=k: orc.gaussian_score(x, ms[k], Ps[k]), 0, batch_size=B, niter=niter,
                             forced_samples=forced[:, k], update=orc.gsm_update_batched)
        assert np.array_equal(m[k], mo) and np.array_equal(c[k], co)


def test_non_pd_initial_covariance_names_the_problem():
    K, D = 5, 3
    cov = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    cov[1, 0, 0] = -1.0
    cov[3] = np.nan
    with pytest.raises(ValueError, match=r"\[1, 3\]"):
        GSMBatch(K, D, None, lambda X: -X, engine=OracleBatchedEngine()).fit(range(K), cov=cov, niter=3, verbose=False)


def test_bound_and_shape_errors_come_before_any_engine_call():
    eng = OracleBatchedEngine()
    with pytest.raises(ValueError, match="D = 65"):
        GSMBatch(2, 65, None, lambda X: -X, engine=eng)
    with pytest.raises(ValueError, match="D = 0"):
        GSMBatch(2, 0, None, lambda X: -X, engine=eng)
    with pytest.raises(ValueError, match="K = 0"):
        GSMBatch(0, 4, None, lambda X: -X, engine=eng)
    fit = GSMBatch(2, 4, None, lambda X: -X, engine=eng)
    with pytest.raises(ValueError, match="B = 33"):
        fit.fit([1, 2], batch_size=33, niter=2, verbose=False)
    with pytest.raises(ValueError, match="B = 0"):
        fit.fit([1, 2], batch_size=0, niter=2, verbose=False)
    with pytest.raises(ValueError, match="3 keys"):
        fit.fit([1, 2, 3], niter=2, verbose=False)
    with pytest.raises(AssertionError):
        fit.fit([1, 2], mean=np.zeros((2, 5)), niter=2, verbose=False)
    with pytest.raises(AssertionError):
        fit.fit([1, 2], cov=np.zeros((2, 4, 3)), niter=2, verbose=False)
    with pytest.raises(AssertionError):
        fit.fit([1, 2], niter=2, batch_size=2, forced_samples=np.zeros((2, 2, 2, 4)), verbose=False)
    with pytest.raises(TypeError, match="monitor"):
        fit.fit([1, 2], niter=2, verbose=False, monitor=object())
    with pytest.raises(ValueError, match="D = 65"):
        gsm_update_batched(np.zeros((2, 2, 65)), np.zeros((2, 2, 65)), np.zeros((2, 65)), np.zeros((2, 65, 65)), engine=eng)
    with pytest.raises(ValueError, match="B = 40"):
        gsm_update_batched(np.zeros((2, 40, 4)), np.zeros((2, 40, 4)), np.zeros((2, 4)), np.zeros((2, 4, 4)), engine=eng)
    with pytest.raises(AssertionError):
        gsm_update_batched(np.zeros((2, 3, 4)), np.zeros((2, 3, 4)), np.zeros((3, 4)), np.zeros((2, 4, 4)), engine=eng)
    with pytest.raises(AssertionError):
        gsm_update_batched(np.zeros((3, 4)), np.zeros((3, 4)), np.zeros(4), np.zeros((4, 4)), engine=eng)
    assert eng.calls == []


def test_keys_as_tensor_and_array():
    import torch
    K, D = 3, 2
    for keys in ([5, 6, 7], np.array([5, 6, 7]), torch.tensor([5, 6, 7])):
        eng = OracleBatchedEngine()
        GSMBatch(K, D, None, lambda X: -X, engine=eng).fit(keys, niter=1, verbose=False)
        assert [s for s, c, _ in eng.draws[:K]] == [5, 6, 7]
