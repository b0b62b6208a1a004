"""The column-sharded factor-form BaM update on the GPU (gsmvi_bam_factor_wq_partial_f64 + gsmvi_bam_factor_apply_cols_f64,
dist.col_sharded_bam_factor_update, BaM.fit(shard="cols")): the blocks assemble to the single-rank update at every chain
branch, the outputs stay inside the owned block, a revert keeps the block, a captured apply replays bit-identically, and
eight HIP ranks on one GPU follow the replicated factor fit."""
import os
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _state(eng, D, B, seed):
    """A dense, non-triangular square factor F0 (Sigma0 = F0^T F0), x = mu0 + z F0 and the scores of a Gaussian target."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    kw = dict(dtype=torch.float64, device="cuda", generator=g)
    F0 = (torch.randn(D, D, **kw) / D ** 0.5 + 0.7 * torch.eye(D, dtype=torch.float64, device="cuda")).contiguous()
    mu0 = torch.randn(D, **kw)
    Z = torch.randn(B, D, **kw)
    X = eng.sample(Z, mu0, F0)
    pd = 0.5 + torch.rand(D, **kw)
    m = torch.rand(D, **kw)
    G = (-(X - m) * pd).contiguous()
    return Z, X, G, mu0, F0


def _blocks(D, P):
    per = D // P
    return [(r * per, (r + 1) * per) for r in range(P)]


def _sharded(eng, Z, X, G, mu0, F0, reg, blocks):
    """The ranks' work in one process: partial Wq summed in a fixed order, one apply per block, blocks assembled."""
    B, D = Z.shape
    Wq = torch.zeros(B, D, dtype=torch.float64, device="cuda")
    for lo, hi in blocks:
        Wq += eng.bam_factor_wq_partial(G, lo, F0[:, lo:hi].contiguous(), reg)
    F = torch.empty(D, D, dtype=torch.float64, device="cuda")
    mu = torch.full((D,), float("nan"), dtype=torch.float64, device="cuda")
    flags = []
    for lo, hi in blocks:
        mu_b, F_b, fl = eng.bam_factor_apply_cols(Z, X, G, Wq, mu0, F0[:, lo:hi].contiguous(), lo, reg)
        F[:, lo:hi] = F_b
        mu[lo:hi] = mu_b[lo:hi]
        flags.append(eng.read_flag(fl))
    return mu, F, flags


# (1024, 128): BASELINE config 4 (2B = 256: the big 2B x 2B chain); 96 / 64: the 128-row chain, 64 at the fork threshold shape;
# 48 / 32: the one-launch B x B chain and the mean riding in the update kernel; (512, 8): the smallest; (4096, 64): the side-stream
# fork of Rt F0
@pytest.mark.parametrize("D,B", [(1024, 128), (4096, 64), (1024, 96), (1024, 64), (1024, 48), (1024, 32), (512, 8)])
def test_blocks_assemble_to_the_single_rank_update(D, B):
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    reg = 3.0
    Z, X, G, mu0, F0 = _state(eng, D, B, 11)
    mu_1, F_1, f1 = eng.bam_factor_update(Z, X, G, mu0, F0, reg)
    assert eng.read_flag(f1) == 0
    S_1 = eng.gram(F_1)
    mu_p, F_p, flags = _sharded(eng, Z, X, G, mu0, F0, reg, [(0, D)])
    assert flags == [0]
    assert _rel(F_p, F_1) <= 1e-13 and _rel(mu_p, mu_1) <= 1e-13
    for P in (2, 8):
        mu_p, F_p, flags = _sharded(eng, Z, X, G, mu0, F0, reg, _blocks(D, P))
        assert flags == [0] * P
        e = (_rel(eng.gram(F_p), S_1), _rel(mu_p, mu_1), _rel(F_p, F_1))
        assert e[0] <= 1e-12 and e[1] <= 1e-12 and e[2] <= 1e-11, (P, e)


def test_ragged_last_block():
    """D = 1000: blocks of 320, 320, 320 and a ragged 40 (the edge tiles of the update kernels inside a window)."""
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    D, B, reg = 1000, 24, 2.0
    Z, X, G, mu0, F0 = _state(eng, D, B, 12)
    mu_1, F_1, f1 = eng.bam_factor_update(Z, X, G, mu0, F0, reg)
    assert eng.read_flag(f1) == 0
    mu_p, F_p, flags = _sharded(eng, Z, X, G, mu0, F0, reg, [(0, 320), (320, 640), (640, 960), (960, 1000)])
    assert flags == [0] * 4
    e = (_rel(eng.gram(F_p), eng.gram(F_1)), _rel(mu_p, mu_1), _rel(F_p, F_1))
    assert e[0] <= 1e-12 and e[1] <= 1e-12 and e[2] <= 1e-11, e


@pytest.mark.parametrize("B", [32, 96])      # the mean written by the update kernel (2B <= 64) / by k_bamf_commit
def test_outputs_are_confined_to_the_owned_block(B):
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    D, reg = 1024, 3.0
    Z, X, G, mu0, F0 = _state(eng, D, B, 13)
    blocks = _blocks(D, 4)
    Wq = sum(eng.bam_factor_wq_partial(G, lo, F0[:, lo:hi].contiguous(), reg) for lo, hi in blocks)
    for lo, hi in (blocks[1], blocks[3]):
        nc = hi - lo
        F0c = F0[:, lo:hi].contiguous()
        mu_ref, F_ref, fl = eng.bam_factor_apply_cols(Z, X, G, Wq, mu0, F0c, lo, reg)
        assert eng.read_flag(fl) == 0
        mu0s = torch.full_like(mu0, float("nan"))              # the entries a rank does not own are stale: never read
        mu0s[lo:hi] = mu0[lo:hi]
        mu = torch.full_like(mu0, 7.25)                        # ... and never written
        Fbuf = torch.full((D, nc + 64), -3.5, dtype=torch.float64, device="cuda")   # ldf > ncols: padding untouched
        mu_o, F_o, fl = eng.bam_factor_apply_cols(Z, X, G, Wq, mu0s, F0c, lo, reg, out=(mu, Fbuf[:, :nc]))
        assert eng.read_flag(fl) == 0
        assert torch.equal(F_o, F_ref) and torch.equal(mu[lo:hi], mu_ref[lo:hi]) and bool(torch.isfinite(F_o).all())
        assert bool((mu[:lo] == 7.25).all()) and bool((mu[hi:] == 7.25).all())
        assert bool((Fbuf[:, nc:] == -3.5).all())


def test_revert_keeps_every_block():
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    D, B, reg = 1024, 64, 3.0
    Z, X, G, mu0, F0 = _state(eng, D, B, 14)
    G = G.clone()
    G[3, 5] = float("nan")
    blocks = _blocks(D, 4)
    Wq = sum(eng.bam_factor_wq_partial(G, lo, F0[:, lo:hi].contiguous(), reg) for lo, hi in blocks)
    eng.last_path()
    for lo, hi in blocks:
        n_rev = eng.new_flag()
        F0c = F0[:, lo:hi].contiguous()
        mu, Fc, fl = eng.bam_factor_apply_cols(Z, X, G, Wq, mu0, F0c, lo, reg, n_reverts=n_rev)
        assert eng.read_flag(fl) != 0 and eng.read_flag(n_rev) == 1
        assert torch.equal(Fc, F0c) and torch.equal(mu[lo:hi], mu0[lo:hi])
    path = eng.last_path()
    assert not [k for k in path if k.endswith("_generic") and k != "panel_t_generic"], path


def test_captured_apply_replays_bit_identically():
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    D, B, reg = 1024, 64, 3.0
    Z, X, G, mu0, F0 = _state(eng, D, B, 15)
    lo, hi = _blocks(D, 4)[2]
    F0c = F0[:, lo:hi].contiguous()
    Wq = eng.bam_factor_wq_partial(G, 0, F0, reg)
    out = (eng.empty(D), eng.empty(D, hi - lo))
    flag = eng.new_flag()
    eng.bam_factor_apply_cols(Z, X, G, Wq, mu0, F0c, lo, reg, out=out, flag=flag)
    torch.cuda.synchronize()
    mu_e, F_e = out[0][lo:hi].clone(), out[1].clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.bam_factor_apply_cols(Z, X, G, Wq, mu0, F0c, lo, reg, out=out, flag=flag)
    out[0].zero_()
    out[1].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[1], F_e) and torch.equal(out[0][lo:hi], mu_e) and eng.read_flag(flag) == 0


def _worker_bam_cols(rank, world, port, q):
    """Column-sharded factor-form BaM on HIP: 8 processes, 8 engine contexts on cuda:0 (gloo rendezvous), each owning D / 8
    columns of the square factor, at BASELINE config 4's shape."""
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    try:
        import gsmvi_amd
        from gsmvi_amd.dist import col_bounds, col_gather_samples, col_sharded_bam_factor_update
        torch.cuda.set_device(0)
        eng = gsmvi_amd.HipEngine(0)
        D, B, reg = 1024, 128, 3.0
        Z, X1, G, mu0, F0 = _state(eng, D, B, 21)                   # same state on every rank
        lo, hi = col_bounds(D, world, rank)
        stats = {}
        Fc = F0[:, lo:hi].contiguous()
        X = col_gather_samples(eng, eng.sample_cols(Z, mu0[lo:hi].contiguous(), Fc), stats=stats)
        mu_1, F_1, f1 = eng.bam_factor_update(Z, X1, G, mu0, F0, reg)
        mu_c, Fc_new, fc = col_sharded_bam_factor_update(eng, Z, X, G, mu0, Fc, reg, stats=stats)
        assert eng.read_flag(f1) == 0 and eng.read_flag(fc) == 0
        blocks = [torch.empty(D, hi - lo, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(blocks, Fc_new.cpu())
        F_c = torch.cat(blocks, dim=1).cuda()
        mparts = [torch.empty(hi - lo, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(mparts, mu_c[lo:hi].cpu())
        out["upd"] = max(_rel(eng.gram(F_c), eng.gram(F_1)), _rel(torch.cat(mparts).cuda(), mu_1))
        out["stats"] = stats
        # the FIT, column-sharded against the replicated factor fit (same key, same draws)
        from oracle import gsm_oracle as orc
        mt, cov_t, Pt = orc.make_gaussian_target(D, 4)
        tgt = gsmvi_amd.GaussianTarget(mt, precision=Pt, engine=eng)
        bc = gsmvi_amd.BaM(D, None, tgt.lp_g, engine=eng)
        mean_c, cov_c = bc.fit(7, gsmvi_amd.Regularizers().constant(10.0), niter=40, batch_size=B, verbose=False,
                               shard="cols", jitter=0, as_torch=True)
        b1 = gsmvi_amd.BaM(D, None, tgt.lp_g, engine=eng)
        mean_1, cov_1 = b1.fit(7, gsmvi_amd.Regularizers().constant(10.0), niter=40, batch_size=B, verbose=False,
                               method="factor", jitter=0, as_torch=True, graph=False)
        out["fit"] = max(_rel(mean_c, mean_1), _rel(cov_c, cov_1))
        out["fit_stats"] = bc.shard_stats
        out["reverts"] = (bc.n_reverts, b1.n_reverts)
        out["method"] = bc.method_used
        t = torch.cat([mean_c, cov_c.reshape(-1)]).cpu()
        gathered = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(gathered, t)
        out["replicas_identical"] = all(torch.equal(gathered[0], x) for x in gathered)
        out["ok"] = True
    except Exception:                                            # noqa: BLE001
        import traceback
        out["ok"] = False
        out["exc"] = traceback.format_exc()
    q.put((rank, out))
    dist.destroy_process_group()


def test_column_sharded_bam_eight_ranks_on_one_gpu():
    """BASELINE config 4's shape (D = 1024, B = 128), 128 columns per rank, eight HIP-backed ranks on one GPU: the blocks
    assemble to the single-rank update, each rank sends B D / P doubles into one all-gather and B D into one all-reduce, and a
    40-iteration fit(shard="cols") follows the replicated factor fit with identical replicas and no reverts."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    world = 8
    procs = [ctx.Process(target=_worker_bam_cols, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
    D, B = 1024, 128
    for r in range(world):
        o = res[r]
        assert o["ok"], o.get("exc")
        assert o["upd"] <= 1e-12, o
        assert o["stats"] == {"all_gather_bytes_per_rank": B * (D // 8) * 8, "collectives": 2, "all_reduce_bytes": B * D * 8}
        assert o["fit"] <= 1e-9 and o["reverts"] == (0, 0) and o["replicas_identical"] and o["method"] == "factor", o
        assert o["fit_stats"] == {"all_gather_bytes_per_rank": B * (D // 8) * 8, "collectives": 2, "all_reduce_bytes": B * D * 8,
                                  "block_bytes": D * (D // 8) * 8}
