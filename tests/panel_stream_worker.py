"""Run by tests/test_gpu_gsm_panel_stream.py in a CHILD process (knob "panel_stream", D = 1024).
usage: panel_stream_worker.py debug D B   -- with GSMVI_HIP_DEBUG_LIB=1: slabs, Qg and Qm read back from the workspace are the same
                                             bytes at knob 0, 1, 2 and 4; the timeline's stamp words of the product tell the instances
                                             apart; the path bits do not.
       panel_stream_worker.py tail D B    -- one update with the knob at 1 and every array at the END of a freshly mapped
                                             allocation (as tests/tail_guard_worker.py): a read or write past an array is a
                                             fault that kills this process."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import gsmvi_amd  # noqa: E402
from oracle import gsm_oracle as orc  # noqa: E402

mode, D, B = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
eng = gsmvi_amd.get_engine()
st = orc.make_update_state(D, B, 3 * D + B)
host = [st[k] for k in ("samples", "vs", "mu0", "S0")]


def debug():
    args = tuple(eng.asarray(a) for a in host)
    strips = D // 16
    nwg = strips * 2 * (B // 16)

    def run(knob):
        eng.set_tuning("panel_stream", knob)
        eng.last_path()
        mu, S = eng.gsm_update(*args)
        path = eng.last_path()
        slabs = (C.c_double * (2 * B * D))()
        eng.lib.gsmvi_debug_read_workspace(eng._ctx, 0, 0, slabs, 2 * B * D)
        q = (C.c_double * (3 * B * strips))()                   # Qg [B][2 strips], then Qm [B][strips]
        eng.lib.gsmvi_debug_read_workspace(eng._ctx, 1, 0, q, 3 * B * strips)
        buf = (C.c_ulonglong * (nwg * 8))()
        eng.lib.gsmvi_debug_read_stamps(eng._ctx, buf, nwg * 8)
        return mu.cpu().numpy(), S.cpu().numpy(), np.array(slabs), np.array(q), path, np.array(buf, dtype=np.uint64).reshape(nwg, 8).astype(np.int64)

    eng.gsm_update(*args)
    eng.set_tuning("timeline", 1)
    try:
        r0, r1, r2, r4 = run(0), run(1), run(2), run(4)
    finally:
        eng.set_tuning("timeline", 0)
        eng.set_tuning("panel_stream", 1)
    assert {"gsm_two_launch", "panel_chunk512", "panel_fast", "cov_sym"} <= r0[4], r0[4]
    for r in (r1, r2, r4):
        assert r[4] == r0[4], (r[4], r0[4])                     # the same set of path bits
        for k in range(4):
            assert r[k].tobytes() == r0[k].tobytes(), k        # mu, S, slabs, Qg | Qm
    assert np.isfinite(r0[2]).all() and np.isfinite(r0[3]).all() and np.abs(r0[2]).max() > 0
    for name, r in (("knob 1", r1), ("knob 2", r2), ("knob 4", r4)):
        w = r[5]
        assert (w > 0).all(), name                              # every word of every workgroup was written
        # start <= stage 0 staged <= first MFMA issued <= last stage staged <= last MFMA done <= reduction barrier <= end
        seq = w[:, [0, 4, 5, 6, 7, 2, 3]]
        assert (np.diff(seq, axis=1) >= 0).all(), (name, seq[(np.diff(seq, axis=1) < 0).any(axis=1)][:4])
        assert (w[:, 1] == w[:, 6]).all(), name                 # "left operand staged" = the last stage of the streamed form
        assert (w[:, 7] > w[:, 4]).all(), name
    assert np.median(r4[5][:, 6] - r4[5][:, 4]) > 0                # four stages: the last one is staged behind stage 0's MFMAs
    w = r0[5]                                                   # knob 0: the unstreamed code (its words 4 - 7 are a landing profile)
    assert (w[:, :4] > 0).all() and (np.diff(w[:, :4], axis=1) >= 0).all()
    assert (w[:, 6] != w[:, 1]).any()
    print("panel stream debug ok", D, B)


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

    eng.set_tuning("panel_stream", 1)
    torch.cuda.empty_cache()
    X, G, mu0, S0 = at_end((B, D), host[0]), at_end((B, D), host[1]), at_end((D,), host[2]), at_end((D, D), host[3])
    eng.last_path()
    mu, S = eng.gsm_update(X, G, mu0, S0, out=(at_end((D,)), at_end((D, D))))
    torch.cuda.synchronize()
    assert {"gsm_two_launch", "panel_chunk512"} <= eng.last_path()
    mu_o, S_o = orc.gsm_update_batched(*host)
    assert np.abs(S.cpu().numpy() - S_o).max() <= 1e-8 * np.abs(S_o).max()      # (parity proper is in the test file: this is about faults)
    assert np.abs(mu.cpu().numpy() - mu_o).max() <= 1e-8 * np.abs(mu_o).max()
    print("panel stream tail ok", D, B)


{"debug": debug, "tail": tail}[mode]()
