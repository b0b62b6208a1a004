"""Shared-design PSIS leave-one-out benchmark (gsmvi_psis_loo_shared_batched_f64, csrc/gsmvi_psis_loo_batched.hip, SHARED).

Writes one JSON object with, at (K, N, D, S) in {(1024, 64, 10, 1024), (1024, 256, 16, 1024)}, all in one process:
  loo[]  the launch alone and ``psis_loo_shared_batched`` end to end on a SharedDesignGLMTarget (logistic, K prior precisions on
         one design, no weights) against the same two of ``psis_loo_batched`` on the K-fold replicated BatchedGLMTarget, on the
         same draws, ratios and weights.  The two are alternated in one process and the order is swapped every repetition; times
         are device-event times around the calls (launch gaps included), medians of ``reps`` calls after three warm-up calls of
         each, not profiler kernel time.  Also the launch with observation weights (U(0, 2), a quarter exact zeros), which the
         replicated target cannot express; whether the two launches' outputs are equal bit for bit; and the device memory of the
         design: N D 8 bytes against K N D 8.  Everything is recorded, nothing is required: the per-observation sort dominates both
         launches, so the times are expected level; the gain is the memory and the weights.
Usage: python scripts/psis_loo_shared_bench.py [--out FILE] [--reps R] [--quick]
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

SHAPES = [(1024, 64, 10, 1024), (1024, 256, 16, 1024)]
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batched",
                           "psis_loo_shared_bench.json")


def problem(K, N, D, seed):
    """one logistic data set under K prior precisions: (shared target, replicated target, weights, mean, cov)"""
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((N, D)) / math.sqrt(D)
    y1 = (rs.random_sample(N) < 1.0 / (1.0 + np.exp(-A @ (2.0 * rs.standard_normal(D))))).astype(np.float64)
    y = np.ascontiguousarray(np.broadcast_to(y1, (K, N)))
    lam = 10.0 ** rs.uniform(-1.0, 1.0, K)
    w = 2.0 * rs.random_sample((K, N))
    w[rs.random_sample((K, N)) < 0.25] = 0.0
    shared = gsmvi_amd.SharedDesignGLMTarget(A, y, "logistic", prior_precision=lam)
    rep = gsmvi_amd.BatchedGLMTarget(np.ascontiguousarray(np.broadcast_to(A[None], (K, N, D))), y, "logistic", prior_precision=lam)
    mean, cov, _ = gsmvi_amd.laplace_init_shared_batched(shared, as_torch=True)
    return shared, rep, shared.engine.asarray(w), mean, cov


def _stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def _each(fns, reps):
    """per-call device-event times (ms) of the callables, alternated, the order swapped every repetition, after three warm-up
    calls of each"""
    out = {k: [] for k in fns}
    names = list(fns)
    for r in range(reps + 3):
        for k in (names if r % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fns[k]()
            b.record()
            b.synchronize()
            if r >= 3:
                out[k].append(a.elapsed_time(b))
    return out


def entry(K, N, D, S, reps):
    eng = gsmvi_amd.get_engine()
    shared, rep, w, mean, cov = problem(K, N, D, 11)
    keys = list(range(K))
    first = gsmvi_amd.psis_batched(shared.lp, mean, cov, keys, num_draws=S, moments=False, as_torch=True)
    X, logr, lw = first.samples, first.log_ratios, first.log_weights
    fns = {
        "shared": lambda: eng.psis_loo_shared_batched(X, logr, lw, shared.A, shared.y, "logistic"),
        "replicated": lambda: eng.psis_loo_batched(X, logr, lw, rep.A, rep.y, "logistic"),
        "shared_weighted": lambda: eng.psis_loo_shared_batched(X, logr, lw, shared.A, shared.y, "logistic", weights=w),
        "shared_whole": lambda: gsmvi_amd.psis_loo_shared_batched(shared, mean, cov, keys, num_draws=S, as_torch=True),
        "replicated_whole": lambda: gsmvi_amd.psis_loo_batched(rep, mean, cov, keys, num_draws=S, as_torch=True),
    }
    a, b = fns["shared"](), fns["replicated"]()
    torch.cuda.synchronize()
    e = {"K": K, "N": N, "D": D, "S": S, "reps": reps, "family": "logistic", "tile": eng.psis_loo_tile(D, S),
         "library": os.path.basename(gsmvi_amd.library_path()), "pareto_fits": K * N,
         "same_bits_as_replicated": bool(all(torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u,
                                                         v.view(torch.int64) if v.dtype == torch.float64 else v)
                                             for u, v in zip(a[:5], b[:5]))),
         "design_bytes_shared": int(shared.A.numel() * 8), "design_bytes_replicated": int(rep.A.numel() * 8),
         "valid_rows_weighted": int((w > 0).sum().item())}
    del a, b
    tm = _each(fns, reps)
    for k in fns:
        e[k + "_ms"] = _stats(tm[k])
    e["launch_replicated_over_shared"] = e["replicated_ms"]["median"] / e["shared_ms"]["median"]
    e["call_replicated_over_shared"] = e["replicated_whole_ms"]["median"] / e["shared_whole_ms"]["median"]
    e["time_source"] = "device events around the calls (not profiler kernel time)"
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="three repetitions, K = 64")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 3 if args.quick else max(args.reps, 5)
    res = {"device": torch.cuda.get_device_name(0), "loo": []}
    for K, N, D, S in SHAPES:
        e = entry(64 if args.quick else K, N, D, S, reps)
        res["loo"].append(e)
        print(json.dumps(e), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
