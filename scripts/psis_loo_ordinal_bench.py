"""Batched ordinal PSIS leave-one-out benchmark (gsmvi_psis_loo_ordinal_batched_f64, csrc/gsmvi_psis_loo_ordinal_batched.hip).

Writes one JSON object with, at (K, N, P, C, S) in {(1024, 64, 6, 5, 1024), (1024, 256, 12, 5, 1024), (1024, 64, 1, 64, 1024)}
(D = P + C - 1 = 10, 16 and 64: the negative binomial bench's shapes with C = 5, and the widest C), all in one process:
  loo[]  the launch alone (one call of the engine method on fixed draws, ratios and weights), ``psis_loo_ordinal_batched`` end to
         end on a BatchedOrdinalTarget (the draw launch, ``lp``, the PSIS launch, the leave-one-out launch and the torch
         reductions; device tensors out, so no copy to the host is timed), and the same computation from existing pieces,
         alternated: the cutpoints by ``cumsum``, the (K, N, S) linear predictors, the log-likelihood block from the two
         ``softplus`` terms and log1mexp of the label's gap, the ratios logr - l, ``psis_weights_batched`` on them reshaped to
         (K N, S), and the two ``logsumexp``; the peak extra device memory of both; the largest difference between the two per
         output; the ratio pieces / launch.  Also the negative binomial launch (``psis_loo_negbin_batched``) at the same
         (D, N, S) -- P + 1 = D, the same design width up to one column, the same ratios and weights, the same stage -- : what the
         ordinal step (1) costs against the nearest sibling's.  Everything is recorded, nothing is required.  Times are
         device-event times around the calls (launch gaps included), medians of ``reps`` alternated calls after three warm-up
         calls of each, not profiler kernel time.  ``tile`` is gsmvi_psis_loo_ordinal_tile(P, C, S) of the library that ran.
Usage: python scripts/psis_loo_ordinal_bench.py [--out FILE] [--reps R] [--quick] [--launch-only]
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

SHAPES = [(1024, 64, 6, 5, 1024), (1024, 256, 12, 5, 1024), (1024, 64, 1, 64, 1024)]
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batched",
                           "psis_loo_ordinal_bench.json")
LOG2 = math.log(2.0)


def problem(K, N, P, C, seed):
    """K cumulative-logit regressions (labels from the model at C - 1 cutpoints evenly over [-1.2, 1.2]) and their L-BFGS
    Gaussians: (target, mean, cov)"""
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((K, N, P)) / math.sqrt(P)
    offset = 0.3 * rs.standard_normal((K, N))
    eta = np.einsum("knp,kp->kn", A, rs.standard_normal((K, P))) + offset
    cuts = np.linspace(-1.2, 1.2, C - 1)
    cdf = 1.0 / (1.0 + np.exp(-(cuts[None, None, :] - eta[:, :, None])))
    y = (rs.random_sample((K, N))[:, :, None] > cdf).sum(2)
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, C, prior_precision=1.0, cut_precision=1.0, offset=offset)
    mean, cov, _ = gsmvi_amd.lbfgs_init_batched(np.zeros((K, P + C - 1)), tgt.lp, tgt.lp_g, as_torch=True)
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
    N, P, C = tgt.N, tgt.P, tgt.C
    sp = torch.nn.functional.softplus
    inf = torch.full((K, S, 1), float("inf"), dtype=X.dtype, device=X.device)
    w = torch.exp(X[:, :, P + 1:])                                                                      # (K, S, C - 2)
    cut = torch.cumsum(torch.cat([X[:, :, P:P + 1], w], 2), 2)                                          # (K, S, C - 1)
    edges = torch.cat([-inf, cut, inf], 2).transpose(1, 2).contiguous()                                 # (K, C + 1, S): cut_{y-1} at y
    lm = torch.where(w < LOG2, torch.log(-torch.expm1(-w)), torch.log1p(-torch.exp(-w)))
    zero = torch.zeros((K, S, 1), dtype=X.dtype, device=X.device)
    lm = torch.cat([zero, lm, zero], 2).transpose(1, 2).contiguous()                                    # (K, C, S): 0 at the ends
    yi = tgt.y.long()[:, :, None].expand(K, N, S)
    eta = torch.einsum("knp,ksp->kns", tgt.A, X[:, :, :P]) + tgt.offset[:, :, None]
    ell = -sp(eta - torch.gather(edges, 1, yi + 1)) - sp(torch.gather(edges, 1, yi) - eta) + torch.gather(lm, 1, yi)
    del eta
    wq, khat, ess, _, _ = eng.psis_weights_batched((logr[:, None, :] - ell).reshape(K * N, S))
    elpd = torch.logsumexp(wq.view(K, N, S) + ell, 2)
    lpd = torch.logsumexp(lw[:, None, :] + ell, 2)
    return elpd, lpd, khat.view(K, N), ess.view(K, N)


def sibling(eng, K, N, D, X, seed):
    """inputs of the negative binomial launch at the same (D, N, S): P' = D - 1 columns, counts, the same draws with the last
    column as a log size about N(1.5, 0.5^2)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    A = eng.asarray((torch.randn((K, N, D - 1), generator=g, dtype=torch.float64) / math.sqrt(D - 1)).numpy())
    y = eng.asarray(torch.poisson(torch.full((K, N), 3.0, dtype=torch.float64), generator=g).numpy())
    Xn = X.clone()
    Xn[:, :, D - 1] = 1.5 + 0.5 * eng.asarray(torch.randn(X.shape[:2], generator=g, dtype=torch.float64).numpy())
    return A, y, Xn


def entry(K, N, P, C, S, reps, launch_only):
    eng = gsmvi_amd.get_engine()
    D = P + C - 1
    tgt, mean, cov = problem(K, N, P, C, 11)
    keys = list(range(K))
    first = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=S, moments=False, as_torch=True)
    X, logr, lw = first.samples, first.log_ratios, first.log_weights
    An, yn, Xn = sibling(eng, K, N, D, X, 5)
    hip = lambda: eng.psis_loo_ordinal_batched(X, logr, lw, tgt.A, tgt.y, C, offset=tgt.offset)                # noqa: E731
    whole = lambda: gsmvi_amd.psis_loo_ordinal_batched(tgt, mean, cov, keys, num_draws=S, as_torch=True)      # noqa: E731
    old = lambda: pieces(eng, tgt, X, logr, lw)                                                               # noqa: E731
    negb = lambda: eng.psis_loo_negbin_batched(Xn, logr, lw, An, yn, offset=tgt.offset)                       # noqa: E731
    e = {"K": K, "N": N, "P": P, "C": C, "D": D, "S": S, "reps": reps, "tile": eng.psis_loo_ordinal_tile(P, C, S),
         "negbin_tile": eng.psis_loo_negbin_tile(D - 1, S), "library": os.path.basename(gsmvi_amd.library_path()),
         "pareto_fits": K * N,
         "share_gaps_below_log_2": float((X[:, :, P + 1:] < math.log(LOG2)).double().mean().item())}
    fns = {"hip": hip, "negbin": negb}
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
    e["negbin_launch_ms"] = _stats(tm["negbin"])
    e["ordinal_over_negbin"] = e["launch_ms"]["median"] / e["negbin_launch_ms"]["median"]
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
    for K, N, P, C, S in SHAPES:
        e = entry(64 if args.quick else K, N, P, C, S, reps, args.launch_only)
        res["loo"].append(e)
        print(json.dumps(e), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
