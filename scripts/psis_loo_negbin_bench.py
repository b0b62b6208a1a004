"""Batched negative binomial PSIS leave-one-out benchmark (gsmvi_psis_loo_negbin_batched_f64,
csrc/gsmvi_psis_loo_negbin_batched.hip).

Writes one JSON object with, at (K, N, D, S) in {(1024, 64, 10, 1024), (1024, 256, 16, 1024)} (D = P + 1), all in one process:
  loo[]  the launch alone (one call of the engine method on fixed draws, ratios and weights), ``psis_loo_negbin_batched`` end to
         end on a BatchedNegBinomialTarget (the draw launch, ``lp``, the PSIS launch, the leave-one-out launch and the torch
         reductions; device tensors out, so no copy to the host is timed), and the same computation from existing pieces,
         alternated: the (K, N, S) linear predictors, the log-likelihood block from torch ``lgamma`` and ``softplus``, the ratios
         logr - l, ``psis_weights_batched`` on them reshaped to (K N, S), and the two ``logsumexp``; the peak extra device memory of
         both; the largest difference between the two per output; the ratio pieces / launch.  Also the Poisson launch
         (``psis_loo_batched``, family "poisson") on the beta part of the same draws with the same (N, S), ratios and weights:
         what the negative binomial link costs over the Poisson one.  Everything is recorded, nothing is required.  Times are
         device-event times around the calls (launch gaps included), medians of ``reps`` alternated calls after three warm-up
         calls of each, not profiler kernel time.  ``tile`` is gsmvi_psis_loo_negbin_tile(P, S) of the library that ran.
Usage: python scripts/psis_loo_negbin_bench.py [--out FILE] [--reps R] [--quick] [--launch-only]
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
                           "psis_loo_negbin_bench.json")


def problem(K, N, P, seed):
    """K negative binomial regressions (log size about U(0.5, 2.5)) and their L-BFGS Gaussians: (target, mean, cov)"""
    rs = np.random.RandomState(seed)
    A = np.concatenate([np.ones((K, N, 1)), rs.standard_normal((K, N, P - 1)) / math.sqrt(P)], axis=2)
    beta = np.concatenate([1.0 + 0.3 * rs.standard_normal((K, 1)), 0.5 * rs.standard_normal((K, P - 1))], axis=1)
    offset = 0.3 * rs.standard_normal((K, N))
    size = np.exp(rs.uniform(0.5, 2.5, K))
    mu = np.exp(np.einsum("knp,kp->kn", A, beta) + offset)
    y = rs.poisson(rs.gamma(size[:, None], mu / size[:, None])).astype(np.float64)
    tgt = gsmvi_amd.BatchedNegBinomialTarget(A, y, prior_precision=1.0, offset=offset, log_size_mean=1.5, log_size_precision=1.0)
    mean, cov, _ = gsmvi_amd.lbfgs_init_batched(np.zeros((K, P + 1)), tgt.lp, tgt.lp_g, as_torch=True)
    return tgt, mean, cov


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


def pieces(eng, tgt, X, logr, lw):
    """the launch's computation from what existed before it: (elpd, lpd, khat, ess) as (K, N) tensors"""
    K, S, _ = X.shape
    N, P = tgt.N, tgt.P
    sp = torch.nn.functional.softplus
    d = torch.einsum("knp,ksp->kns", tgt.A, X[:, :, :P]) + tgt.offset[:, :, None] - X[:, None, :, P]      # eta - theta, (K, N, S)
    r = torch.exp(X[:, None, :, P])
    yv = tgt.y[:, :, None]
    ell = torch.lgamma(yv + r) - torch.lgamma(r) - torch.lgamma(yv + 1.0) - r * sp(d) - yv * sp(-d)
    del d
    w, khat, ess, _, _ = eng.psis_weights_batched((logr[:, None, :] - ell).reshape(K * N, S))
    elpd = torch.logsumexp(w.view(K, N, S) + ell, 2)
    lpd = torch.logsumexp(lw[:, None, :] + ell, 2)
    return elpd, lpd, khat.view(K, N), ess.view(K, N)


def entry(K, N, D, S, reps, launch_only):
    eng = gsmvi_amd.get_engine()
    P = D - 1
    tgt, mean, cov = problem(K, N, P, 11)
    keys = list(range(K))
    first = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, moments=False, as_torch=True)
    X, logr, lw = first.samples, first.log_ratios, first.log_weights
    Xb = X[:, :, :P].contiguous()
    hip = lambda: eng.psis_loo_negbin_batched(X, logr, lw, tgt.A, tgt.y, offset=tgt.offset)                   # noqa: E731
    whole = lambda: gsmvi_amd.psis_loo_negbin_batched(tgt, mean, cov, keys, num_draws=S, as_torch=True)       # noqa: E731
    old = lambda: pieces(eng, tgt, X, logr, lw)                                                               # noqa: E731
    pois = lambda: eng.psis_loo_batched(Xb, logr, lw, tgt.A, tgt.y, "poisson", offset=tgt.offset)             # noqa: E731
    e = {"K": K, "N": N, "P": P, "D": D, "S": S, "reps": reps, "tile": eng.psis_loo_negbin_tile(P, S),
         "poisson_tile": eng.psis_loo_tile(P, S), "library": os.path.basename(gsmvi_amd.library_path()), "pareto_fits": K * N,
         "share_draws_below_r_10": float((X[:, :, P] < math.log(10.0)).double().mean().item())}
    fns = {"hip": hip, "poisson": pois}
    if not launch_only:
        fns.update(whole=whole, pieces=old)
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
        e["pieces_peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base)
        e["max_rel_diff"] = {n: float(((a - b).abs() / b.abs().clamp_min(1.0)).max().item())
                             for n, a, b in zip(("elpd", "lpd", "khat", "ess"), got[:4], want)}
        del want, got
        r = whole()
        e["share_ok"] = float(r.ok.double().mean().item())
        e["khat_median"] = float(r.khat.median().item())
    tm = _each(fns, reps)
    e["launch_ms"] = _stats(tm["hip"])
    e["launch_us_per_fit"] = 1e3 * e["launch_ms"]["median"] / (K * N)
    e["poisson_launch_ms"] = _stats(tm["poisson"])
    e["negbin_over_poisson"] = e["launch_ms"]["median"] / e["poisson_launch_ms"]["median"]
    if not launch_only:
        e["end_to_end_ms"] = _stats(tm["whole"])
        e["pieces_ms"] = _stats(tm["pieces"])
        e["pieces_over_launch"] = e["pieces_ms"]["median"] / e["launch_ms"]["median"]
    e["launch_output_bytes"] = (4 * 8 + 4) * K * N
    e["time_source"] = "device events around the calls (not profiler kernel time)"
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="three repetitions, K = 64")
    ap.add_argument("--launch-only", action="store_true", help="time the launch alone")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 3 if args.quick else max(args.reps, 5)
    res = {"device": torch.cuda.get_device_name(0), "loo": []}
    for K, N, D, S in SHAPES:
        e = entry(64 if args.quick else K, N, D, S, reps, args.launch_only)
        res["loo"].append(e)
        print(json.dumps(e), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
