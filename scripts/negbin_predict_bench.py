"""Batched negative binomial posterior predictive benchmark (gsmvi_negbin_predict_batched_f64, csrc/gsmvi_negbin_predict_batched.hip).

Writes one JSON object with, at K = 1024, S = 1024 and (M, D) in {(64, 10), (256, 16), (1024, 64)}, D = P + 1, all in one process:
  predict[]  the launch alone (one call of the engine method on fixed draws, uniform weights, counts given),
             ``predict_negbin_batched`` end to end on a BatchedNegBinomialTarget (the draw launch, the predictive launch and the
             torch composition of mean, var and elpd, with the host-side check and upload of y; device tensors out, so no copy to
             the host is timed), and the same computation as torch ops, alternated: ``einsum`` for the (k, S, M) linear predictors,
             ``lgamma`` and ``softplus`` for the density and ``logsumexp`` over the draws, in chunks of problems small enough to fit
             (``chunk``); the peak extra device memory of both; the largest difference between the two per output; the ratio torch /
             launch.  Times are device-event times around the calls (launch gaps included), medians of ``reps`` alternated calls
             after three warm-up calls of each, not profiler kernel time.  Reported, not gated.
Usage: python scripts/negbin_predict_bench.py [--out FILE] [--reps R] [--quick] [--launch-only]
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

SHAPES = [(1024, 64, 10, 1024), (1024, 256, 16, 1024), (1024, 1024, 64, 1024)]     # (K, M, D, S)
N_TRAIN = 64
CHUNK_BYTES = 2 ** 30                # the torch form's (k, S, M) block per chunk of problems (it holds several at once)


def problem(K, M, P, seed):
    """K negative binomial regressions, their Laplace posteriors and M new rows with counts: (target, mean, cov, A_new, y_new)"""
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((K, N_TRAIN + M, P)) / math.sqrt(P)
    beta = 0.7 * rs.standard_normal((K, P))
    size = np.exp(rs.uniform(0.5, 2.5, K))
    mu = np.exp(np.einsum("knp,kp->kn", A, beta) + 1.0)
    y = rs.poisson(rs.gamma(size[:, None], mu / size[:, None])).astype(np.float64)
    tgt = gsmvi_amd.BatchedNegBinomialTarget(A[:, :N_TRAIN], y[:, :N_TRAIN], 1.0, log_size_mean=1.5, log_size_precision=1.0)
    mean, cov, _ = gsmvi_amd.laplace_init_negbin_batched(tgt, as_torch=True)
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


def torch_ops(X, A, y, chunk):
    """the launch's computation as torch ops, ``chunk`` problems at a time: (lmom (K, M, 3), lpd (K, M))"""
    K, S, D = X.shape
    M, P = A.shape[1], D - 1
    lmom, lpd = X.new_empty(K, M, 3), X.new_empty(K, M)
    sp = torch.nn.functional.softplus
    for k0 in range(0, K, chunk):
        k1 = min(K, k0 + chunk)
        eta = torch.einsum("kmp,ksp->ksm", A[k0:k1], X[k0:k1, :, :P])
        th = X[k0:k1, :, P, None]
        r, yy = torch.exp(th), y[k0:k1, None, :]
        lmom[k0:k1, :, 0] = torch.logsumexp(eta, 1)
        lmom[k0:k1, :, 1] = torch.logsumexp(2.0 * eta, 1)
        lmom[k0:k1, :, 2] = torch.logsumexp(2.0 * eta - th, 1)
        d = eta - th
        ell = torch.lgamma(yy + r) - torch.lgamma(r) - r * sp(d) - yy * sp(-d) - torch.lgamma(yy + 1.0)
        lpd[k0:k1] = torch.logsumexp(ell, 1)
        del eta, d, ell
    lmom -= math.log(S)
    lpd -= math.log(S)
    return lmom, lpd


def entry(K, M, D, S, reps, launch_only):
    eng = gsmvi_amd.get_engine()
    P = D - 1
    tgt, mean, cov, A_new, y_new = problem(K, M, P, 11)
    keys = list(range(K))
    seeds = eng.batched_seeds(tuple((k % (2 ** 32)) ^ 0x5DEECE66D for k in keys))
    X, _, _ = eng.kl_draw_batched(mean, cov, seeds, 0, 0, S)
    A, y = eng.asarray(A_new), eng.asarray(y_new)
    chunk = max(1, min(K, CHUNK_BYTES // (S * M * 8)))
    hip = lambda: eng.negbin_predict_batched(X, None, A, y=y)                                                        # noqa: E731
    whole = lambda: gsmvi_amd.predict_negbin_batched(tgt, mean, cov, A, keys, y=y_new, num_draws=S, as_torch=True)   # noqa: E731
    old = lambda: torch_ops(X, A, y, chunk)                                                                          # noqa: E731
    e = {"K": K, "M": M, "P": P, "D": D, "S": S, "reps": reps, "chunk": chunk,
         "lds_bytes": 8 * (80 * (4 * ((P + 3) // 4) + 1) + 824), "library": os.path.basename(gsmvi_amd.library_path()),
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
                             for n, a, b in zip(("lmom", "lpd"), got, want)}
        del want, got
    tm = _each(fns, reps)
    e["launch_ms"] = _stats(tm["hip"])
    e["launch_ns_per_row_draw"] = 1e6 * e["launch_ms"]["median"] / (K * M * S)
    if not launch_only:
        e["end_to_end_ms"] = _stats(tm["whole"])
        e["torch_ms"] = _stats(tm["torch"])
        e["torch_over_launch"] = e["torch_ms"]["median"] / e["launch_ms"]["median"]
    e["launch_output_bytes"] = 8 * K * M * 4
    e["time_source"] = "device events around the calls (not profiler kernel time)"
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="three repetitions, K = 64")
    ap.add_argument("--launch-only", action="store_true", help="time the launch alone")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 3 if args.quick else max(args.reps, 5)
    res = {"device": torch.cuda.get_device_name(0), "predict": []}
    for K, M, D, S in SHAPES:
        e = entry(64 if args.quick else K, M, D, S, reps, args.launch_only)
        res["predict"].append(e)
        print(json.dumps(e), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
