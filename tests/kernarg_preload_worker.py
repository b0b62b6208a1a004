"""Run by tests/test_gpu_gsm_kernarg_preload.py in a CHILD process (knob "kernarg_preload").
usage: kernarg_preload_worker.py debug D B  -- with GSMVI_HIP_DEBUG_LIB=1: slabs, Qg and Qm read back from the workspace are the same
                                               bytes at knob 0 and 1; with the timeline on and the knob at 1 every stamp word of every
                                               workgroup of both launches is nonzero and, at D = 1024, the product's words keep the order
                                               that tests/panel_stream_worker.py checks.
       kernarg_preload_worker.py tail D B   -- one update with the knob at 1 and every array at the END of a freshly mapped
                                               allocation (as tests/panel_stream_worker.py): a read or write past an array is a
                                               fault that kills this process."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import gsmvi_amd  # noqa: E402
from oracle import gsm_oracle as orc  # noqa: E402

KNOB = "kernarg_preload"
mode, D, B = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
eng = gsmvi_amd.get_engine()
st = orc.make_update_state(D, B, 3 * D + B)
host = [st[k] for k in ("samples", "vs", "mu0", "S0")]


def debug():
    args = tuple(eng.asarray(a) for a in host)
    strips = D // 16
    two_slab = D == 1024                                        # two 512-row slabs, grid (strips, 2, B / 16); else D / 256 slabs, grid (strips, kc, 1)
    kc = 2 if two_slab else D // 256
    nwg_p = strips * kc * (B // 16 if two_slab else 1)
    nt = D // 32                                                # covariance launch: the quad / pair map at D = 1024, else one workgroup per
    nwg_c = (nt // 2) ** 2 if two_slab else sum((nt - ti + 1) // 2 for ti in range(nt))   # tile pair and diagonal leftover
    cw = 7 if two_slab else 6                                   # its stamp words: 0 - 6 (S0 last: 6 = "S0 landed"), else 0 - 5
    assert nwg_p <= 512 and nwg_c <= 512

    def run(knob):
        eng.set_tuning(KNOB, knob)
        eng.last_path()
        mu, S = eng.gsm_update(*args)
        path = eng.last_path()
        slabs = (C.c_double * (kc * B * D))()
        eng.lib.gsmvi_debug_read_workspace(eng._ctx, 0, 0, slabs, kc * B * D)
        nq = (kc + 1) * B * strips                              # Qg [B][kc strips], then Qm [B][strips]
        q = (C.c_double * nq)()
        eng.lib.gsmvi_debug_read_workspace(eng._ctx, 1, 0, q, nq)
        buf = (C.c_ulonglong * (3 * 4096))()                    # [kernel][512 workgroups][8 words]: product, -, covariance
        eng.lib.gsmvi_debug_read_stamps(eng._ctx, buf, 3 * 4096)
        w = np.array(buf, dtype=np.uint64).reshape(3, 512, 8).astype(np.int64)
        return mu.cpu().numpy(), S.cpu().numpy(), np.array(slabs), np.array(q), path, w

    eng.gsm_update(*args)
    eng.set_tuning("timeline", 1)
    try:
        r1, r0 = run(1), run(0)                                 # the knob at 1 first: the stamp buffer is zero from its allocation
    finally:
        eng.set_tuning("timeline", 0)
        eng.set_tuning(KNOB, 1)
    assert {"gsm_two_launch", "panel_fast", "cov_sym"} <= r0[4], r0[4]
    assert r1[4] == r0[4], (r1[4], r0[4])
    for k in range(4):
        assert r1[k].tobytes() == r0[k].tobytes(), k            # mu, S, slabs, Qg | Qm
    assert np.isfinite(r0[2]).all() and np.isfinite(r0[3]).all() and np.abs(r0[2]).max() > 0
    for name, r in (("knob 0", r0), ("knob 1", r1)):
        wp, wc = r[5][0, :nwg_p], r[5][2, :nwg_c]
        assert (wc[:, :cw] > 0).all(), (name, (wc == 0).sum(axis=0))
        assert (wc[:, 0:1] <= wc[:, 1:cw]).all(), name          # word 0 = the kernel's first instruction
        if two_slab:                                            # the streamed product: all eight words, the order of panel_stream_worker.py
            assert (wp > 0).all(), name
            seq = wp[:, [0, 4, 5, 6, 7, 2, 3]]
            assert (np.diff(seq, axis=1) >= 0).all(), (name, seq[(np.diff(seq, axis=1) < 0).any(axis=1)][:4])
            assert (wp[:, 1] == wp[:, 6]).all() and (wp[:, 7] > wp[:, 4]).all(), name
        else:                                                   # 256-row chunks: words 0 - 3
            assert (wp[:, :4] > 0).all() and (np.diff(wp[:, :4], axis=1) >= 0).all(), name
    print("kernarg preload debug ok", D, B)


def tail():
    keep = []

    def at_end(shape, src=None):
        n = int(np.prod(shape))
        seg = -(-8 * n // (2 * 2 ** 20)) * 2 * 2 ** 20          # whole 2 MiB granules; the array ends the allocation
        big = torch.empty(seg // 8, dtype=torch.float64, device=eng.device)
        keep.append(big)
        t = big[big.numel() - n:].view(*shape)
        if src is not None:
            t.copy_(torch.as_tensor(np.ascontiguousarray(src), dtype=torch.float64))
        return t

    eng.set_tuning(KNOB, 1)
    torch.cuda.empty_cache()
    X, G, mu0, S0 = at_end((B, D), host[0]), at_end((B, D), host[1]), at_end((D,), host[2]), at_end((D, D), host[3])
    eng.last_path()
    mu, S = eng.gsm_update(X, G, mu0, S0, out=(at_end((D,)), at_end((D, D))))
    torch.cuda.synchronize()
    assert "gsm_two_launch" in eng.last_path()
    mu_o, S_o = orc.gsm_update_batched(*host)
    assert np.abs(S.cpu().numpy() - S_o).max() <= 1e-8 * np.abs(S_o).max()      # (parity proper is in the test file: this is about faults)
    assert np.abs(mu.cpu().numpy() - mu_o).max() <= 1e-8 * np.abs(mu_o).max()
    print("kernarg preload tail ok", D, B)


{"debug": debug, "tail": tail}[mode]()
