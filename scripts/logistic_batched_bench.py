"""Batched logistic target benchmark (BatchedLogisticTarget, csrc/gsmvi_logistic_batched.hip) against the same score written as
torch ops -- how this target had to be scored before the kernel existed.

Writes one JSON object with
  calls[]  at K in {1024, 8192} x (N, D, B) in {(64, 10, 2), (256, 16, 8), (1024, 64, 8)}: the score call alone, the HIP launch
           (hip_ms) and the torch expression (torch_ms: torch.bmm for eta, the overflow-safe sigmoid, torch.baddbmm back; marked
           device_score), alternated in one process; per call one pair of device events, --reps (>= 30) calls after a warm-up,
           median and range; ratio = torch median / hip median (acceptance: >= 1.0).  Also the log-density call (lp_ms) and both
           (both_ms).  bytes = 8 K (N D + N + 2 B D + B) (A and y read once, X read, G and lp written), bytes_per_s over the hip
           median and its fraction of 8 TB/s (hbm_fraction) and of the library's streaming copy measured in the same run
           (copy_fraction); flops = 4 K N B D
  fits[]   GSMBatch.fit with the target's lp_g and with the torch score at the same shapes: a device-synchronised host clock
           around niter iterations after a warm-up fit; problem_iters_per_s = K (niter + 1) / seconds and their ratio
  advi     ADVIBatch.fit at K = 1024, N = 64, D = 10, B = 8 with track_loss=False and with track_loss=True (lp = the target's
           device lp): problem_iters_per_s of each
Usage: python scripts/logistic_batched_bench.py [--out FILE] [--reps R] [--quick] [--kernel-only]
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
SHAPES = [(64, 10, 2), (256, 16, 8), (1024, 64, 8)]
LAM = 0.5


def problems(K, N, D, seed):
    """K synthetic data sets on the device: A ~ N(0, 1) / sqrt(D), y ~ Bernoulli(sigmoid(A theta*)), theta* ~ N(0, 1)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(K, N, D, dtype=torch.float64, device="cuda", generator=g) / np.sqrt(D)
    theta = torch.randn(K, D, 1, dtype=torch.float64, device="cuda", generator=g)
    y = (torch.rand(K, N, dtype=torch.float64, device="cuda", generator=g) < torch.sigmoid(torch.bmm(A, theta)[:, :, 0])).double()
    return A, y


def torch_score(A, y, lam):
    """the same score as torch ops on the device"""
    At = A.transpose(1, 2)

    @gsmvi_amd.device_score
    def lp_g(x):
        eta = torch.bmm(x, At)
        e = torch.exp(-eta.abs())
        sig = torch.where(eta >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        return torch.baddbmm(x, y[:, None, :] - sig, A, beta=-lam)
    return lp_g


def _each(fns, reps):
    """per-call device-event times (ms) of the callables, alternated: {name: [ms] * reps}"""
    for _ in range(3):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def _stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


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

    ms = _each({"copy": go}, reps)["copy"]
    return 2 * 8 * big[0].numel() / (float(np.median(ms)) * 1e-3)


def call_entry(K, N, D, B, reps, kernel_only=False):
    A, y = problems(K, N, D, 11)
    tgt = gsmvi_amd.BatchedLogisticTarget(A, y, LAM)
    eng = tgt.engine
    x = torch.randn(K, B, D, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    G, lpo = eng.empty(K, B, D), eng.empty(K, B)
    fns = {"hip": lambda: tgt.lp_g(x, out=G)}
    if not kernel_only:
        tscore = torch_score(A, y, LAM)
        err = float((tscore(x) - tgt.lp_g(x)).abs().max() / tscore(x).abs().max())
        assert err < 1e-10, err
        fns["torch"] = lambda: tscore(x)
        fns["lp"] = lambda: eng.logistic_batched(x, tgt.A, tgt.y, None, LAM, lp_out=lpo, want="lp")
        fns["both"] = lambda: eng.logistic_batched(x, tgt.A, tgt.y, None, LAM, out=G, lp_out=lpo, want="both")
    t = _each(fns, reps)
    nbytes, flops = 8 * K * (N * D + N + 2 * B * D + B), 4 * K * N * B * D
    e = {"K": K, "N": N, "D": D, "B": B, "reps": reps, "bytes": nbytes, "flops": flops, "hip_ms": _stats(t["hip"])}
    e["bytes_per_s"] = nbytes / (e["hip_ms"]["median"] * 1e-3)
    e["hbm_fraction"] = e["bytes_per_s"] / HBM_BYTES_PER_S
    e["flops_per_s"] = flops / (e["hip_ms"]["median"] * 1e-3)
    if not kernel_only:
        e.update(torch_ms=_stats(t["torch"]), lp_ms=_stats(t["lp"]), both_ms=_stats(t["both"]), max_rel_diff_vs_torch=err)
        e["ratio"] = e["torch_ms"]["median"] / e["hip_ms"]["median"]
    return e


def _timed(run, niter):
    run(10)                                      # warm-up (kernels loaded, allocator warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(niter)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def fit_entry(K, N, D, B, niter):
    A, y = problems(K, N, D, 11)
    tgt = gsmvi_amd.BatchedLogisticTarget(A, y, LAM)
    keys = np.arange(K)
    e = {"K": K, "N": N, "D": D, "B": B, "niter": niter}
    for name, score in (("hip", tgt.lp_g), ("torch", torch_score(A, y, LAM))):
        fit = gsmvi_amd.GSMBatch(K, D, None, score)
        s = _timed(lambda n: fit.fit(keys, batch_size=B, niter=n, verbose=False, as_torch=True), niter)
        e[name] = {"seconds": s, "iter_ms": s / (niter + 1) * 1e3, "problem_iters_per_s": K * (niter + 1) / s}
    e["ratio"] = e["hip"]["problem_iters_per_s"] / e["torch"]["problem_iters_per_s"]
    return e


def advi_entry(K, N, D, B, niter):
    A, y = problems(K, N, D, 11)
    tgt = gsmvi_amd.BatchedLogisticTarget(A, y, LAM)
    fit = gsmvi_amd.ADVIBatch(K, D, tgt.lp, tgt.lp_g)
    keys = np.arange(K)
    e = {"K": K, "N": N, "D": D, "B": B, "niter": niter}
    for track in (False, True):
        s = _timed(lambda n: fit.fit(keys, gsmvi_amd.Adam(1e-2), batch_size=B, niter=n, verbose=False, track_loss=track,
                                     as_torch=True), niter)
        e["track_loss" if track else "no_loss"] = {"seconds": s, "problem_iters_per_s": K * (niter + 1) / s}
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--quick", action="store_true", help="few repetitions and iterations, K = 1024 only")
    ap.add_argument("--kernel-only", action="store_true", help="only the HIP score call at K = 8192 for the three shapes and the "
                    "copy (the profiler run: its kernel statistics are then these launches')")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 5 if args.quick else max(args.reps, 30)
    res = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S, "prior_precision": LAM, "calls": [],
           "fits": []}
    res["copy_bytes_per_s"] = copy_rate(reps)
    print(json.dumps({"copy_bytes_per_s": res["copy_bytes_per_s"]}), flush=True)
    Ks = (8192,) if args.kernel_only else (1024,) if args.quick else (1024, 8192)
    for K in Ks:
        for N, D, B in SHAPES:
            e = call_entry(K, N, D, B, reps, args.kernel_only)
            e["copy_fraction"] = e["bytes_per_s"] / res["copy_bytes_per_s"]
            res["calls"].append(e)
            print(json.dumps(e), flush=True)
    if not args.kernel_only:
        for K in Ks:
            for N, D, B in SHAPES:
                niter = 30 if args.quick else (1000 if N * D * K <= 2 ** 25 else 300 if N * D * K <= 2 ** 28 else 100)
                e = fit_entry(K, N, D, B, niter)
                res["fits"].append(e)
                print(json.dumps(e), flush=True)
        res["advi"] = advi_entry(1024, 64, 10, 8, 30 if args.quick else 1000)
        print(json.dumps(res["advi"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
