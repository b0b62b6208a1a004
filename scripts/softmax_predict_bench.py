"""Batched softmax posterior predictive benchmark (gsmvi_softmax_predict_batched_f64, csrc/gsmvi_softmax_predict_batched.hip).

Writes one JSON object with, at K = 1024, S = 1024 and (M, C, P) in {(64, 3, 5), (256, 5, 4), (1024, 9, 8)}, all in one process:
  predict[]  the launch alone (one call of the engine method on fixed draws, uniform weights, labels given),
             ``predict_softmax_batched`` end to end on a BatchedSoftmaxTarget (the draw launch, the predictive launch and the torch
             reductions, with the host-side check and upload of the labels; device tensors out, so no copy to the host is timed), and the same computation as torch ops, alternated:
             ``einsum`` for the (k, S, M, C - 1) linear predictors, ``softmax`` / ``log_softmax`` with the zero column appended,
             the mean over the draws and ``logsumexp``, in chunks of problems small enough to fit (``chunk``); the peak extra
             device memory of both; the largest difference between the two per output; the ratio torch / launch.  Times are
             device-event times around the calls (launch gaps included), medians of ``reps`` alternated calls after three warm-up
             calls of each, not profiler kernel time.  Reported, not gated.
Usage: python scripts/softmax_predict_bench.py [--out FILE] [--reps R] [--quick] [--launch-only]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gsmvi_amd  # noqa: E402

SHAPES = [(1024, 64, 3, 5, 1024), (1024, 256, 5, 4, 1024), (1024, 1024, 9, 8, 1024)]     # (K, M, C, P, S)
N_TRAIN = 64
CHUNK_BYTES = 2 ** 31                # the torch form's (k, S, M, C) block per chunk of problems


def problem(K, M, C, P, seed):
    """K multinomial logit regressions, their Laplace posteriors and M new rows with labels: (target, mean, cov, A_new, y_new)"""
    rs = np.random.RandomState(seed)
    A = 1.5 * rs.standard_normal((K, N_TRAIN + M, P)) / math.sqrt(P)
    W = rs.standard_normal((K, C - 1, P))
    eta = np.concatenate([np.einsum("knp,kcp->knc", A, W), np.zeros((K, N_TRAIN + M, 1))], axis=2)
    prob = np.exp(eta - eta.max(axis=2, keepdims=True))
    cdf = np.cumsum(prob / prob.sum(axis=2, keepdims=True), axis=2)
    y = np.minimum((rs.random_sample((K, N_TRAIN + M, 1)) > cdf).sum(axis=2), C - 1)
    tgt = gsmvi_amd.BatchedSoftmaxTarget(A[:, :N_TRAIN], y[:, :N_TRAIN], C, prior_precision=1.0)
    mean, cov, _ = gsmvi_amd.laplace_init_softmax_batched(tgt, as_torch=True)
    return tgt, mean, cov, A[:, N_TRAIN:], y[:, N_TRAIN:]


def _stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def _each(fns, reps):
    """per-call device-event times (ms) of the callables, alternated, after three warm-up calls of each"""
    out = {k: [] for k in fns}
    for r in range(reps + 3):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            if r >= 3:
                out[k].append(a.elapsed_time(b))
    return out


def torch_ops(X, A, y, C, chunk):
    """the launch's computation as torch ops, ``chunk`` problems at a time: (prob (K, M, C), lpd (K, M))"""
    K, S, _ = X.shape
    M, P = A.shape[1], A.shape[2]
    prob, lpd = X.new_empty(K, M, C), X.new_empty(K, M)
    for k0 in range(0, K, chunk):
        k1 = min(K, k0 + chunk)
        eta = torch.einsum("kmp,kscp->ksmc", A[k0:k1], X[k0:k1].view(k1 - k0, S, C - 1, P))
        eta = torch.cat([eta, eta.new_zeros(k1 - k0, S, M, 1)], dim=3)
        prob[k0:k1] = torch.softmax(eta, dim=3).mean(1)
        idx = y[k0:k1].long()[:, None, :, None].expand(k1 - k0, S, M, 1)
        lpd[k0:k1] = torch.logsumexp(torch.log_softmax(eta, dim=3).gather(3, idx)[..., 0], 1) - math.log(S)
        del eta
    return prob, lpd


def entry(K, M, C, P, S, reps, launch_only):
    eng = gsmvi_amd.get_engine()
    tgt, mean, cov, A_new, y_new = problem(K, M, C, P, 11)
    keys = list(range(K))
    seeds = eng.batched_seeds(tuple((k % (2 ** 32)) ^ 0x5DEECE66D for k in keys))
    X, _, _ = eng.kl_draw_batched(mean, cov, seeds, 0, 0, S)
    A, y = eng.asarray(A_new), eng.batched_labels(y_new)
    chunk = max(1, min(K, CHUNK_BYTES // (S * M * C * 8)))
    hip = lambda: eng.softmax_predict_batched(X, None, A, C, labels=y)                                                # noqa: E731
    whole = lambda: gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A, keys, y=y_new, num_draws=S, as_torch=True)   # noqa: E731
    old = lambda: torch_ops(X, A, y, C, chunk)                                                                        # noqa: E731
    e = {"K": K, "M": M, "C": C, "P": P, "D": (C - 1) * P, "S": S, "reps": reps, "chunk": chunk,
         "lds_bytes": eng.softmax_predict_lds_bytes(C, P), "library": os.path.basename(gsmvi_amd.library_path()),
         "rows": K * M}
    fns = {"hip": hip}
    if not launch_only:
        fns.update(whole=whole, torch=old)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        got = hip()
        torch.cuda.synchronize()
        e["launch_peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        want = old()
        torch.cuda.synchronize()
        e["torch_peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base)
        e["max_rel_diff"] = {n: float(((a - b).abs() / b.abs().clamp_min(1.0)).max().item())
                             for n, a, b in zip(("prob", "lpd"), got, want)}
        del want, got
    tm = _each(fns, reps)
    e["launch_ms"] = _stats(tm["hip"])
    e["launch_ns_per_row_draw"] = 1e6 * e["launch_ms"]["median"] / (K * M * S)
    if not launch_only:
        e["end_to_end_ms"] = _stats(tm["whole"])
        e["torch_ms"] = _stats(tm["torch"])
        e["torch_over_launch"] = e["torch_ms"]["median"] / e["launch_ms"]["median"]
    e["launch_output_bytes"] = 8 * K * M * (C + 1)
    e["time_source"] = "device events around the calls (not profiler kernel time)"
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="three repetitions, K = 64")
    ap.add_argument("--launch-only", action="store_true", help="time the launch alone")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 3 if args.quick else max(args.reps, 5)
    res = {"device": torch.cuda.get_device_name(0), "predict": []}
    for K, M, C, P, S in SHAPES:
        e = entry(64 if args.quick else K, M, C, P, S, reps, args.launch_only)
        res["predict"].append(e)
        print(json.dumps(e), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
