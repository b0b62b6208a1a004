"""The column-sharded factor-form BaM fit (BaM.fit(shard="cols"), dist.col_sharded_bam_factor_update) on CPU: two gloo
ranks with an oracle-backed engine whose two column-block calls restate bam.py:72-114 in whitened coordinates; the policy of
the shard keyword; argument validation of the two C entry points without a GPU."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from scipy import linalg as sla

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
from engines import Flag, OracleEngine        # noqa: E402


def _helmert_qt(G, reg):
    """Qt (B x D): the B - 1 orthonormal (Helmert) combinations of the centred scores, scaled by sqrt(reg / B), and
    sqrt(reg / (1 + reg)) gbar -- U = Qt^T Qt (bam.py:59)."""
    B = G.shape[0]
    gbar = G.mean(axis=0)
    H = np.zeros((B - 1, B))
    for k in range(1, B):
        H[k - 1, :k] = 1.0
        H[k - 1, k] = -k
        H[k - 1] /= np.sqrt(k * (k + 1.0))
    return np.vstack([np.sqrt(reg / B) * (H @ (G - gbar)), np.sqrt(reg / (1.0 + reg)) * gbar[None, :]])


class ColsOracleEngine(OracleEngine):
    """The two column-block calls in numpy, from the whitened quantities alone (Sigma0 = F0^T F0, x_b = mu0 + z_b F0):
    Mv = I + Vw^T Vw, P = Mv Wq^T, BB = (I/2 + sqrtm(Wq P + I/4))^2, M = Mv - P BB^-1 P^T = I + Vw^T Vw - Zw^T Zw,
    F'[:, C] = chol(M)^T F0[:, C], mu'[C] = mu0[C] / (1 + reg) + r1 (F0[:, C]^T M wg + xbar[C]), wg = F0 gbar = Wq's last row
    / sqrt(r1).  ``bam_factor_update`` is the same with C = all columns, so the replicated factor fit and the sharded one
    sample with the same factor."""

    def bam_factor_wq_partial(self, G, col0, F0cols, reg, out=None):
        nc = F0cols.shape[1]
        Wp = _helmert_qt(G, reg)[:, col0:col0 + nc] @ F0cols.T
        if out is not None:
            out[...] = Wp
            return out
        return Wp

    def bam_factor_apply_cols(self, Z, X, G, Wq, mu0, F0cols, col0, reg, out=None, flag=None, n_reverts=None):
        flag = Flag() if flag is None else flag
        B, D = Z.shape
        nc = F0cols.shape[1]
        r1 = reg / (1.0 + reg)
        zbar = Z.mean(axis=0)
        Vw = np.vstack([np.sqrt(reg / B) * (Z - zbar), -np.sqrt(r1) * zbar[None, :]])
        Mv = np.eye(D) + Vw.T @ Vw
        P = Mv @ Wq.T
        BB = 0.5 * np.eye(B) + np.real(sla.sqrtm(Wq @ P + 0.25 * np.eye(B)))
        M = Mv - P @ np.linalg.solve(BB @ BB, P.T)
        mu = np.array(mu0, copy=True)
        try:
            L = np.linalg.cholesky(0.5 * (M + M.T))
            ok = bool(np.isfinite(L).all())
        except np.linalg.LinAlgError:
            ok = False
        if ok:
            wg = Wq[-1] / np.sqrt(r1)
            Fn, flag.v = L.T @ F0cols, 0
            mu[col0:col0 + nc] = mu0[col0:col0 + nc] / (1.0 + reg) + r1 * (F0cols.T @ (M @ wg) + X[:, col0:col0 + nc].mean(axis=0))
        else:
            Fn, flag.v = F0cols.copy(), 1
            if n_reverts is not None:
                n_reverts.v += 1
        if out is not None:
            out[0][...] = mu
            out[1][...] = Fn
            return out[0], out[1], flag
        return mu, Fn, flag

    def bam_factor_update(self, Z, X, G, mu0, F0, reg, out=None, flag=None, n_reverts=None):
        Wq = self.bam_factor_wq_partial(G, 0, F0, reg)
        return self.bam_factor_apply_cols(Z, X, G, Wq, mu0, F0, 0, reg, out=out, flag=flag, n_reverts=n_reverts)


def _port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _init(rank, world, port):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _gather_cols(Fc, mu, lo, hi, world):
    t = torch.from_numpy(np.ascontiguousarray(Fc))
    blocks = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(blocks, t)
    mt = torch.from_numpy(np.ascontiguousarray(mu[lo:hi]))
    parts = [torch.empty_like(mt) for _ in range(world)]
    dist.all_gather(parts, mt)
    return np.concatenate([b.numpy() for b in blocks], axis=1), np.concatenate([p.numpy() for p in parts])


def _cols_worker(rank, world, port, q):
    _init(rank, world, port)
    out = {}
    try:
        from oracle import gsm_oracle as orc
        from test_bam_cols_cpu import ColsOracleEngine
        from gsmvi_amd.bam import BaM, Regularizers
        from gsmvi_amd.dist import col_bounds, col_gather_samples, col_sharded_bam_factor_update
        eng = ColsOracleEngine()
        D, B, reg = 128, 8, 1.7
        st = orc.make_update_state(D, B, 5)
        F0 = st["L"].T.copy()                                     # Sigma0 = F0^T F0, x = mu0 + z F0
        lo, hi = col_bounds(D, world, rank)
        mu0 = st["mu0"].copy()
        mu0[:lo] = np.nan                                          # entries a rank does not own are never read
        mu0[hi:] = np.nan
        stats = {}
        X = col_gather_samples(eng, eng.sample_cols(st["Z"], mu0[lo:hi], F0[:, lo:hi]), stats=stats)
        mu, Fc, fl = col_sharded_bam_factor_update(eng, st["Z"], X, st["vs"], mu0, F0[:, lo:hi].copy(), reg, stats=stats)
        F, mu_full = _gather_cols(Fc, mu, lo, hi, world)
        mu_o, F_o, fo = OracleEngine().bam_factor_update(st["Z"], st["samples"], st["vs"], st["mu0"], F0, reg)
        S_o = F_o.T @ F_o
        out["upd_err"] = float(max(np.abs(F.T @ F - S_o).max() / np.abs(S_o).max(),
                                   np.abs(mu_full - mu_o).max() / np.abs(mu_o).max()))
        out["flags"] = (fl.v, fo.v)
        out["stats"] = stats
        # the FIT: column-sharded against the replicated factor fit, same key, same draws
        m, cov_t, P = orc.make_gaussian_target(D, 4)
        seen = []

        def lp_g(x):
            seen.append(x.shape)
            return orc.gaussian_score(x, m, P)

        b = BaM(D, None, lp_g, engine=ColsOracleEngine())
        mean_c, cov_c = b.fit(7, Regularizers().linear(20.0), niter=40, batch_size=B, verbose=False, shard="cols", jitter=0)
        b1 = BaM(D, None, lambda x: orc.gaussian_score(x, m, P), engine=ColsOracleEngine())
        mean_1, cov_1 = b1.fit(7, Regularizers().linear(20.0), niter=40, batch_size=B, verbose=False, method="factor", jitter=0)
        out["fit_err"] = float(max(np.abs(mean_c - mean_1).max() / np.abs(mean_1).max(),
                                   np.abs(cov_c - cov_1).max() / np.abs(cov_1).max()))
        out["seen"] = sorted(set(seen))
        out["fit_stats"] = b.shard_stats
        out["method"] = (b.method_used, b1.method_used)
        out["reverts"] = (b.n_reverts, b1.n_reverts)
        t = torch.from_numpy(np.concatenate([mean_c, cov_c.ravel()]))
        gathered = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(gathered, t)
        out["same"] = all(torch.equal(gathered[0], x) for x in gathered)
        out["ok"] = True
    except Exception:                                            # noqa: BLE001
        import traceback
        out["ok"] = False
        out["exc"] = traceback.format_exc()
    q.put((rank, out))
    dist.destroy_process_group()


def _run(target, world=2, timeout=300):
    port = _port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=timeout) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def test_column_sharded_bam_world2_gloo():
    """Two gloo ranks: the one-shot update assembled from the two blocks is the dense restatement of bam.py:72-114 (FtF and
    the mean), the exchange is one all-gather of B D / P and one all-reduce of B D doubles, and a 40-iteration
    fit(shard="cols") walks the replicated factor fit's path with identical replicas."""
    D, B = 128, 8
    res = _run(_cols_worker)
    for r in range(2):
        o = res[r]
        assert o["ok"], o.get("exc")
        assert o["flags"] == (0, 0) and o["upd_err"] < 1e-10, o
        assert o["stats"] == {"all_gather_bytes_per_rank": B * (D // 2) * 8, "all_reduce_bytes": B * D * 8, "collectives": 2}
        assert o["fit_err"] < 1e-9 and o["same"] and o["method"] == ("factor", "factor"), o
        assert o["reverts"] == (0, 0)
        assert o["seen"] == [(B, D)]                              # every rank scores all B samples
        assert o["fit_stats"] == {"all_gather_bytes_per_rank": B * (D // 2) * 8, "all_reduce_bytes": B * D * 8,
                                  "collectives": 2, "block_bytes": D * (D // 2) * 8}


def _retry_worker(rank, world, port, q):
    _init(rank, world, port)
    out = {}
    try:
        from oracle import gsm_oracle as orc
        from test_bam_cols_cpu import ColsOracleEngine
        from gsmvi_amd.bam import BaM, Regularizers
        D, B = 128, 4
        m, cov_t, P = orc.make_gaussian_target(D, 4)
        calls = [0]

        def lp_g(x):
            calls[0] += 1
            if rank == 1 and calls[0] in (3, 4, 9):               # fails on ONE rank only, twice in a row once
                raise FloatingPointError("synthetic score failure")
            return orc.gaussian_score(x, m, P)

        reg = Regularizers()
        mean, cov = BaM(D, None, lp_g, engine=ColsOracleEngine()).fit(5, reg.linear(10.0), niter=12, batch_size=B,
                                                                       verbose=False, shard="cols", retries=3, jitter=0)
        t = torch.from_numpy(np.concatenate([mean, cov.ravel(), [float(reg.counter), float(calls[0])]]))
        gathered = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(gathered, t)
        out.update(same=all(torch.equal(gathered[0], x) for x in gathered), counter=reg.counter, calls=calls[0],
                   finite=bool(np.isfinite(cov).all()), ok=True)
    except Exception:                                            # noqa: BLE001
        import traceback
        out["ok"] = False
        out["exc"] = traceback.format_exc()
    q.put((rank, out))
    dist.destroy_process_group()


def test_column_sharded_bam_retries_are_collective():
    """A score failure on ONE rank makes EVERY rank retry (the fail bit is all-reduced before the update's all-reduce):
    the regularisers advance equally, the replicas stay identical, and the run ends (no rank waits in a collective alone)."""
    res = _run(_retry_worker, timeout=180)
    for r in range(2):
        o = res[r]
        assert o["ok"], o.get("exc")
        assert o["same"] and o["finite"], o
        assert o["counter"] == 13                 # niter + 1 successful updates; failed attempts never reached regf
        assert o["calls"] == 13 + 3               # three collective retries: every rank redrew and re-scored


class _NoCollectives(ColsOracleEngine):
    def sample_cols(self, *a, **k):               # the first thing an iteration does: the policy must refuse before it
        raise AssertionError("an iteration was entered")


def _target(D):
    from oracle import gsm_oracle as orc
    m, cov_t, P = orc.make_gaussian_target(D, 4)
    return lambda x: orc.gaussian_score(x, m, P)


def test_cols_policy_default_jitter_is_refused_before_any_collective():
    from gsmvi_amd.bam import BaM, Regularizers
    b = BaM(128, None, _target(128), engine=_NoCollectives())
    with pytest.raises(ValueError, match="jitter=0.*jitter_every=0"):
        b.fit(3, Regularizers().constant(5.0), niter=4, batch_size=4, verbose=False, shard="cols")
    with pytest.raises(ValueError, match="jitter"):
        b.fit(3, Regularizers().constant(5.0), niter=4, batch_size=4, verbose=False, shard="cols", jitter=1e-6,
              jitter_every=4)


def test_cols_policy_jitter_every_zero_drops_the_jitter():
    from gsmvi_amd.bam import BaM, Regularizers
    f = _target(128)
    b = BaM(128, None, f, engine=ColsOracleEngine())
    m_c, c_c = b.fit(3, Regularizers().constant(5.0), niter=6, batch_size=4, verbose=False, shard="cols", jitter=1e-6,
                     jitter_every=0)
    b0 = BaM(128, None, f, engine=ColsOracleEngine())
    m_0, c_0 = b0.fit(3, Regularizers().constant(5.0), niter=6, batch_size=4, verbose=False, shard="cols", jitter=0)
    assert b.jitter_every_used == 0 and b.method_used == "factor"
    assert np.array_equal(m_c, m_0) and np.array_equal(c_c, c_0)          # dropped, not applied
    assert b.shard_stats == {"block_bytes": 128 * 128 * 8}                 # one rank: no collective at all


def test_cols_policy_geometry_and_keyword():
    from gsmvi_amd.bam import BaM, Regularizers
    with pytest.raises(ValueError, match="multiple of 64"):
        BaM(96, None, _target(96), engine=_NoCollectives()).fit(3, Regularizers().constant(5.0), niter=2, batch_size=4,
                                                                 verbose=False, shard="cols", jitter=0)
    with pytest.raises(ValueError, match="2\\*batch_size"):
        BaM(128, None, _target(128), engine=_NoCollectives()).fit(3, Regularizers().constant(5.0), niter=2, batch_size=80,
                                                                   verbose=False, shard="cols", jitter=0)
    with pytest.raises(ValueError, match="FACTOR"):
        BaM(128, None, _target(128), engine=_NoCollectives()).fit(3, Regularizers().constant(5.0), niter=2, batch_size=4,
                                                                   verbose=False, shard="cols", jitter=0, method="dense")
    with pytest.raises(ValueError, match="bogus"):
        BaM(128, None, _target(128), engine=_NoCollectives()).fit(3, Regularizers().constant(5.0), niter=2, batch_size=4,
                                                                   verbose=False, shard="bogus")


def test_cols_policy_batch_is_a_synonym_of_true():
    from gsmvi_amd.bam import BaM, Regularizers
    f = _target(16)
    b1 = BaM(16, None, f, engine=OracleEngine())
    m1, c1 = b1.fit(3, Regularizers().constant(5.0), niter=5, batch_size=4, verbose=False, shard=True)
    b2 = BaM(16, None, f, engine=OracleEngine())
    m2, c2 = b2.fit(3, Regularizers().constant(5.0), niter=5, batch_size=4, verbose=False, shard="batch")
    assert np.array_equal(m1, m2) and np.array_equal(c1, c2) and b1.method_used == b2.method_used


def test_bam_cols_entry_points_reject_bad_arguments_without_a_gpu():
    """Argument validation of gsmvi_bam_factor_wq_partial_f64 / gsmvi_bam_factor_apply_cols_f64 runs before the context is
    used and before any HIP call, so it is checkable on a machine without a GPU."""
    import ctypes as C
    from gsmvi_amd import _lib
    lib = _lib.load_library()
    a = (C.c_double * 4096)()
    b = (C.c_double * 4096)()
    c = (C.c_double * 4096)()
    d = (C.c_double * 64)()
    e = (C.c_double * 64)()
    flag = (C.c_int * 2)()
    p = lambda x: C.cast(x, C.POINTER(C.c_double))             # noqa: E731

    def partial(col0=0, ncols=64, D=128, B=4, reg=1.0, G=a, F=b, W=c):
        return lib.gsmvi_bam_factor_wq_partial_f64(None, None, D, B, col0, ncols, p(G), D, p(F), ncols, reg, p(W))

    def apply(col0=0, ncols=64, D=128, B=4, reg=1.0, F0=b, F=c, mu0=d, mu=e):
        return lib.gsmvi_bam_factor_apply_cols_f64(None, None, D, B, col0, ncols, p(a), D, p(a), D, p(a), D, p(a), p(mu0),
                                                   p(F0), ncols, reg, p(mu), p(F), ncols,
                                                   C.cast(flag, C.POINTER(C.c_int)), None)

    for fn in (partial, apply):
        assert fn() == 1 and b"ctx" in lib.gsmvi_last_error()             # valid geometry: only the NULL context is left
        assert fn(col0=32) == 1 and b"tile aligned" in lib.gsmvi_last_error()
        assert fn(ncols=96) == 1 and b"tile aligned" in lib.gsmvi_last_error()
        assert fn(col0=64, ncols=128) == 1 and b"out of range" in lib.gsmvi_last_error()
        assert fn(reg=0.0) == 1 and b"reg" in lib.gsmvi_last_error()
        assert fn(reg=-1.0) == 1 and b"reg" in lib.gsmvi_last_error()
        assert fn(D=1024, B=129, ncols=1024) == 5 and b"2B <= 256" in lib.gsmvi_last_error()
        assert fn(D=128, B=65) == 5 and b"2B <= D" in lib.gsmvi_last_error()
    assert partial(W=a) == 1 and b"alias" in lib.gsmvi_last_error()
    assert partial(W=b) == 1 and b"alias" in lib.gsmvi_last_error()
    assert apply(F=b) == 1 and b"alias" in lib.gsmvi_last_error()
    assert apply(mu=d) == 1 and b"alias" in lib.gsmvi_last_error()
    assert lib.gsmvi_bam_factor_apply_cols_f64(None, None, 128, 4, 0, 64, None, 128, p(a), 128, p(a), 128, p(a), p(d), p(b),
                                               64, 1.0, p(e), p(c), 64, C.cast(flag, C.POINTER(C.c_int)), None) == 1
    assert b"NULL" in lib.gsmvi_last_error()
