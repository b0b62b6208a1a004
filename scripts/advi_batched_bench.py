"""Batched ADVI benchmark (ADVIBatch.fit, csrc/gsmvi_advi_batched.hip) against the single-problem ADVI harness.

Writes one JSON object with
  fits[]   ADVIBatch.fit with BatchedGaussianTarget at (K, D, B) = (1024, 10, 8), (8192, 64, 8), (8192, 64, 32), with and
           without the losses: a device-synchronised host clock around --niter (>= 1000) iterations after a warm-up fit;
           problem_iters_per_s = K (niter + 1) / seconds
  single   one ``ADVI(D, tgt.lp, device="cuda").fit`` with torch.optim.Adam at (10, 8) (torch autograd, a torch optimiser, one
           host read of the loss per iteration), timed the same way in the same run: it_per_s
  speedup_vs_single  problem_iters_per_s of the (1024, 10, 8) fit without losses / single it_per_s   (acceptance: >= 50)
  step     the step kernel alone at K = 8192, D = 64, B = 8 (device events over --reps launches after warm-up): ms, the
           algorithmic bytes 8 K (6 (D (D + 1) / 2 + D) + 2 B D) (three triangles and three vectors read and written, G read,
           X written), and that rate as a fraction of 8 TB/s and of the library's own streaming copy
           (gsmvi_debug_stream_copy_f64 of the debug build) measured in the same run
Usage: python scripts/advi_batched_bench.py [--out FILE] [--niter N] [--quick] [--step-only]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gsmvi_amd  # noqa: E402
from gsmvi_amd import _lib  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def _problems(K, D, seed):
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((K, D, D))
    cov = A @ np.swapaxes(A, 1, 2) / D + np.eye(D)
    return rs.standard_normal((K, D)), np.linalg.inv(cov)


def _timed(run, niter):
    run(20)                                      # warm-up (kernels loaded, allocator warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(niter)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def fit_entry(K, D, B, niter, track_loss):
    m, P = _problems(K, D, 3)
    tgt = gsmvi_amd.BatchedGaussianTarget(m, precision=P)
    fit = gsmvi_amd.ADVIBatch(K, D, tgt.lp, tgt.lp_g)
    keys = np.arange(K)
    s = _timed(lambda n: fit.fit(keys, gsmvi_amd.Adam(1e-2), batch_size=B, niter=n, verbose=False, track_loss=track_loss,
                                 as_torch=True), niter)
    return {"K": K, "D": D, "B": B, "niter": niter, "track_loss": track_loss, "seconds": s, "iter_ms": s / (niter + 1) * 1e3,
            "problem_iters_per_s": K * (niter + 1) / s}


def single_entry(D, B, niter):
    m, P = _problems(1, D, 4)
    tgt = gsmvi_amd.GaussianTarget(m[0], precision=P[0])
    advi = gsmvi_amd.ADVI(D, tgt.lp, device="cuda")
    s = _timed(lambda n: advi.fit(7, lambda p: torch.optim.Adam(p, lr=1e-2), batch_size=B, niter=n, nprint=0), niter)
    return {"D": D, "B": B, "niter": niter, "seconds": s, "it_per_s": (niter + 1) / s}


def _events(fn, reps):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def copy_rate(reps):
    """bytes / s (read + write) of the library's streaming copy on 1 GiB"""
    dbg = C.CDLL(_lib.library_path(debug=True))
    dbg.gsmvi_debug_stream_copy_f64.restype = C.c_int
    dbg.gsmvi_debug_stream_copy_f64.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    big = torch.empty(2, 2 ** 27, dtype=torch.float64, device="cuda")
    big[0].fill_(1.0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def go():
        assert dbg.gsmvi_debug_stream_copy_f64(st, C.c_void_p(big[1].data_ptr()), C.c_void_p(big[0].data_ptr()), big[0].numel()) == 0

    ms = _events(go, reps)
    return 2 * 8 * big[0].numel() / (ms * 1e-3)


def step_entry(K, D, B, reps):
    eng = gsmvi_amd.get_engine()
    P = D * (D + 1) // 2
    rs = np.random.RandomState(5)
    scales = 0.1 * rs.standard_normal((K, P))
    scales[:, np.cumsum(np.arange(1, D + 1)) - 1] = 1.0
    d_sc, d_loc, d_G = eng.asarray(scales), eng.zeros(K, D), eng.asarray(rs.standard_normal((K, B, D)))
    mom = tuple(eng.zeros(K, n) for n in (D, D, P, P))
    X, logq, seeds = eng.empty(K, B, D), eng.empty(K), eng.batched_seeds(range(K))
    call = [0]

    def go():
        call[0] += 1
        eng.advi_step_batched(d_G, d_loc, d_sc, mom, call[0], 1e-4, seeds=seeds, call=call[0], Xout=X, logq=logq)

    ms = _events(go, reps)
    nbytes = 8 * K * (6 * (P + D) + 2 * B * D)
    return {"K": K, "D": D, "B": B, "step_ms": ms, "bytes": nbytes, "bytes_per_s": nbytes / (ms * 1e-3),
            "hbm_fraction": nbytes / (ms * 1e-3) / HBM_BYTES_PER_S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--niter", type=int, default=1000)
    ap.add_argument("--quick", action="store_true", help="few iterations and repetitions")
    ap.add_argument("--step-only", action="store_true", help="only the step kernel at K = 8192, D = 64, B = 8 and the copy "
                    "(the profiler run: its kernel statistics are then this one shape's)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    niter, reps = (60, 5) if args.quick else (max(args.niter, 1000), 30)
    res = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S, "fits": []}
    if args.step_only:
        res["copy_bytes_per_s"] = copy_rate(reps)
        res["step"] = step_entry(8192, 64, 8, reps)
        print(json.dumps(res), flush=True)
        return
    res["single"] = single_entry(10, 8, niter)
    print(json.dumps(res["single"]), flush=True)
    for K, D, B, n in ((1024, 10, 8, niter), (8192, 64, 8, niter), (8192, 64, 32, niter)):
        for track in (False, True):
            e = fit_entry(K, D, B, n, track)
            res["fits"].append(e)
            print(json.dumps(e), flush=True)
    res["speedup_vs_single"] = res["fits"][0]["problem_iters_per_s"] / res["single"]["it_per_s"]
    res["copy_bytes_per_s"] = copy_rate(reps)
    res["step"] = step_entry(8192, 64, 8, reps)
    res["step"]["copy_fraction"] = res["step"]["bytes_per_s"] / res["copy_bytes_per_s"]
    print(json.dumps({k: res[k] for k in ("speedup_vs_single", "copy_bytes_per_s", "step")}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
