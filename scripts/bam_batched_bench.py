"""Batched BaM benchmark (bam_update_batched / BaMBatch.fit, csrc/gsmvi_bam_batched.hip) against the single dense BaM fit.

For K in {1, 64, 1024, 8192} x (D, B) in {(10, 2), (32, 8), (64, 8), (64, 32)} it writes one JSON object with, per entry:
  update_ms          one-shot bam_update_batched, device events (mean over --reps launches after warm-up)
  update_ms_unpadded the same with the knob "bam_batched_pad" = 0 (LDS row strides D and B instead of D | 1 and B | 1)
  fit_iter_ms        one BaMBatch.fit iteration with BatchedGaussianTarget (score launch + fit-step launch), wall clock over
                     the loop: (fit of n2 iterations - fit of n1 iterations) / (n2 - n1), so start-up and the final copy cancel
  problem_iters_per_s  K / fit_iter_ms
  single_dense_it_per_s  BaM.fit(method="dense", rng="device") at the same (D, B) with GaussianTarget, measured the same way in
                     the same run
  speedup_vs_single_dense  problem_iters_per_s / single_dense_it_per_s
  update_hbm_fraction  algorithmic bytes of the one-shot update (S0 read + S written + X, G, mu0 read + mu written) / time / 8 TB/s
Usage: python scripts/bam_batched_bench.py [--out FILE] [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gsmvi_amd  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
SHAPES = ((10, 2), (32, 8), (64, 8), (64, 32))


def _problems(K, D, seed):
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((K, D, D))
    cov = A @ np.swapaxes(A, 1, 2) / D + np.eye(D)
    return rs.standard_normal((K, D)), cov, np.linalg.inv(cov)


def update_ms(K, D, B, reps, pad=1):
    rs = np.random.RandomState(1)
    m, S0, _ = _problems(K, D, 2)
    dev = lambda a: torch.tensor(a, device="cuda")     # noqa: E731
    X = dev(m[:, None, :] + rs.standard_normal((K, B, D)))
    V = dev(-rs.standard_normal((K, B, D)))
    mu0, S0 = dev(m), dev(S0)
    eng = gsmvi_amd.get_engine()
    eng.set_tuning("bam_batched_pad", pad)
    out = (eng.empty(K, D), eng.empty(K, D, D))
    try:
        for _ in range(3):
            eng.bam_update_batched(X, V, mu0, S0, 2.0, 0.0, out=out)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            eng.bam_update_batched(X, V, mu0, S0, 2.0, 0.0, out=out)
        b.record()
        b.synchronize()
    finally:
        eng.set_tuning("bam_batched_pad", 1)
    return a.elapsed_time(b) / reps


def _fit_wall(run, n1, n2):
    run(2)                                       # warm-up (kernels loaded, buffers cached)
    torch.cuda.synchronize()
    t = []
    for n in (n1, n2):
        t0 = time.perf_counter()
        run(n)
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return (t[1] - t[0]) / (n2 - n1)


def fit_iter_s(K, D, B, n1, n2):
    m, cov, P = _problems(K, D, 3)
    tgt = gsmvi_amd.BatchedGaussianTarget(m, precision=P)
    fit = gsmvi_amd.BaMBatch(K, D, tgt.lp, tgt.lp_g)
    keys = np.arange(K)
    return _fit_wall(lambda n: fit.fit(keys, lambda i: 100.0 / (1 + i), batch_size=B, niter=n, verbose=False, as_torch=True),
                     n1, n2)


def single_iter_s(D, B, n1, n2):
    m, cov, P = _problems(1, D, 4)
    tgt = gsmvi_amd.GaussianTarget(m[0], precision=P[0])
    bam = gsmvi_amd.BaM(D, tgt.lp, tgt.lp_g)
    return _fit_wall(lambda n: bam.fit(7, lambda i: 100.0 / (1 + i), batch_size=B, niter=n, verbose=False, as_torch=True,
                                       method="dense", rng="device"), n1, n2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions (profiling runs)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps, n1, n2 = (5, 5, 15) if args.quick else (20, 20, 120)
    res = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S, "entries": []}
    for D, B in SHAPES:
        single = 1.0 / single_iter_s(D, B, n1, n2)
        for K in (1, 64, 1024, 8192):
            u = update_ms(K, D, B, reps)
            u0 = update_ms(K, D, B, reps, pad=0)
            it = fit_iter_s(K, D, B, n1, n2)
            nbytes = K * 8 * (2 * D * D + 2 * B * D + 2 * D)
            e = {"K": K, "D": D, "B": B, "update_ms": u, "update_ms_unpadded": u0, "fit_iter_ms": it * 1e3,
                 "problem_iters_per_s": K / it, "single_dense_it_per_s": single, "speedup_vs_single_dense": (K / it) / single,
                 "update_bytes": nbytes, "update_hbm_fraction": nbytes / (u * 1e-3) / HBM_BYTES_PER_S}
            res["entries"].append(e)
            print(json.dumps(e), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
