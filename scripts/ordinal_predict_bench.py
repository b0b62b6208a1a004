"""Batched ordinal posterior predictive benchmark (gsmvi_ordinal_predict_batched_f64, csrc/gsmvi_ordinal_predict_batched.hip).

Writes one JSON object with, at (K, M, P, C, S) in {(1024, 64, 6, 5, 1024), (1024, 256, 12, 5, 1024), (1024, 64, 1, 64, 1024)}
(D = P + C - 1 = 10, 16 and 64: the shapes of the ordinal leave-one-out bench), all in one process:
  predict[]  the launch alone (one call of the engine method on fixed draws, with labels, offsets and uniform weights),
             ``predict_ordinal_batched`` end to end on a BatchedOrdinalTarget (the draw launch, the predictive launch and the torch
             summaries; device tensors out, so no copy to the host is timed), and the same result from torch pieces, alternated:
             the cutpoints by ``cumsum``, the (K, M, S) linear predictors, class by class the difference of two ``sigmoid`` blocks
             averaged over the draws (no (K, M, S, C) block is formed there either), the log-likelihood block from the two
             ``softplus`` terms and log1mexp of the label's gap, and its ``logsumexp``; the peak extra device memory of both; the
             largest difference between the two per output; the ratio pieces / launch.  Also the softmax predictive launch
             (``softmax_predict_batched``) at the same (D, M, S), (C', P') = (3, 5), (5, 4) and (65, 1), on draws of the same
             spread: the nearest sibling.  Everything is recorded, nothing is required.  Times are device-event times around the
             calls (launch gaps included), medians of ``reps`` alternated calls after three warm-up calls of each, not profiler
             kernel time.  ``lds_bytes`` is gsmvi_ordinal_predict_lds_bytes(P, C) of the library that ran.
Usage: python scripts/ordinal_predict_bench.py [--out FILE] [--reps R] [--quick] [--launch-only]
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
SOFTMAX_SIBLING = {10: (3, 5), 16: (5, 4), 64: (65, 1)}        # (C', P') with (C' - 1) P' = D
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batched",
                           "ordinal_predict_bench.json")
LOG2 = math.log(2.0)


def problem(K, N, M, P, C, seed):
    """K cumulative-logit regressions (labels from the model at C - 1 cutpoints evenly over [-1.2, 1.2]) with N training and M
    held-out rows, and their L-BFGS Gaussians: (target, mean, cov, A_new, offset_new, y_new)"""
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((K, N + M, P)) / math.sqrt(P)
    offset = 0.3 * rs.standard_normal((K, N + M))
    eta = np.einsum("knp,kp->kn", A, rs.standard_normal((K, P))) + offset
    cuts = np.linspace(-1.2, 1.2, C - 1)
    cdf = 1.0 / (1.0 + np.exp(-(cuts[None, None, :] - eta[:, :, None])))
    y = (rs.random_sample((K, N + M))[:, :, None] > cdf).sum(2)
    tgt = gsmvi_amd.BatchedOrdinalTarget(A[:, :N], y[:, :N], C, prior_precision=1.0, cut_precision=1.0, offset=offset[:, :N])
    mean, cov, _ = gsmvi_amd.lbfgs_init_batched(np.zeros((K, P + C - 1)), tgt.lp, tgt.lp_g, as_torch=True)
    return tgt, mean, cov, A[:, N:], offset[:, N:], y[:, N:]


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


def pieces(X, A, o, y, P, C):
    """the launch's computation (uniform weights) from torch pieces: (prob (K, M, C), lpd (K, M))"""
    K, S, _ = X.shape
    M = A.shape[1]
    sp = torch.nn.functional.softplus
    inf = torch.full((K, S, 1), float("inf"), dtype=X.dtype, device=X.device)
    w = torch.exp(X[:, :, P + 1:])                                                                      # (K, S, C - 2)
    cut = torch.cumsum(torch.cat([X[:, :, P:P + 1], w], 2), 2)                                          # (K, S, C - 1)
    eta = torch.einsum("kmp,ksp->kms", A, X[:, :, :P]) + o[:, :, None]                                  # (K, M, S)
    prob = torch.empty((K, M, C), dtype=X.dtype, device=X.device)
    prev = None
    for c in range(C - 1):
        cdf = torch.sigmoid(cut[:, None, :, c] - eta)
        prob[:, :, c] = (cdf if prev is None else cdf - prev).mean(2)
        prev = cdf
    prob[:, :, C - 1] = (1.0 - prev).mean(2)
    del prev, cdf
    edges = torch.cat([-inf, cut, inf], 2).transpose(1, 2).contiguous()                                 # (K, C + 1, S): cut_{y-1} at y
    lm = torch.where(w < LOG2, torch.log(-torch.expm1(-w)), torch.log1p(-torch.exp(-w)))
    zero = torch.zeros((K, S, 1), dtype=X.dtype, device=X.device)
    lm = torch.cat([zero, lm, zero], 2).transpose(1, 2).contiguous()                                    # (K, C, S): 0 at the ends
    yi = y.long()[:, :, None].expand(K, M, S)
    ell = -sp(eta - torch.gather(edges, 1, yi + 1)) - sp(torch.gather(edges, 1, yi) - eta) + torch.gather(lm, 1, yi)
    del eta
    lpd = torch.logsumexp(ell, 2) - math.log(S)
    return prob, lpd


def sibling(eng, K, M, D, S, seed):
    """inputs of the softmax predictive launch at the same (D, M, S): rows, labels and draws of unit spread"""
    Cs, Ps = SOFTMAX_SIBLING[D]
    g = torch.Generator(device="cpu").manual_seed(seed)
    A = eng.asarray((torch.randn((K, M, Ps), generator=g, dtype=torch.float64) / math.sqrt(Ps)).numpy())
    y = eng.batched_labels(torch.randint(0, Cs, (K, M), generator=g).numpy().astype(np.int32))
    X = eng.asarray(torch.randn((K, S, D), generator=g, dtype=torch.float64).numpy())
    return Cs, Ps, A, y, X


def entry(K, M, P, C, S, reps, launch_only):
    eng = gsmvi_amd.get_engine()
    D = P + C - 1
    tgt, mean, cov, A_new, o_new, y_new = problem(K, 64, M, P, C, 11)
    keys = list(range(K))
    seeds = eng.batched_seeds(tuple((k % (2 ** 32)) ^ 0x5DEECE66D for k in keys))
    X, _, _ = eng.kl_draw_batched(mean, cov, seeds, 0, 0, S)
    A, o, y = eng.asarray(A_new), eng.asarray(o_new), eng.batched_labels(y_new.astype(np.int32))
    Cs, Ps, As, ys, Xs = sibling(eng, K, M, D, S, 5)
    hip = lambda: eng.ordinal_predict_batched(X, None, A, C, y=y, offset=o)                                   # noqa: E731
    whole = lambda: gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, offset=o_new, y=y_new, num_draws=S,      # noqa: E731
                                                      as_torch=True)
    old = lambda: pieces(X, A, o, y, P, C)                                                                    # noqa: E731
    soft = lambda: eng.softmax_predict_batched(Xs, None, As, Cs, labels=ys)                                   # noqa: E731
    e = {"K": K, "M": M, "P": P, "C": C, "D": D, "S": S, "reps": reps, "lds_bytes": eng.ordinal_predict_lds_bytes(P, C),
         "softmax_sibling": {"C": Cs, "P": Ps, "lds_bytes": eng.softmax_predict_lds_bytes(Cs, Ps)},
         "library": os.path.basename(gsmvi_amd.library_path()), "rows": K * M,
         "share_gaps_below_log_2": float((X[:, :, P + 1:] < math.log(LOG2)).double().mean().item()) if C > 2 else None}
    fns = {"hip": hip, "softmax": soft}
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
                             for n, a, b in zip(("prob", "lpd"), got, want)}
        e["max_row_sum_gap"] = float((got[0].sum(2) - 1.0).abs().max().item())
        del want, got
        r = whole()
        e["accuracy_of_median"] = float((r.median.cpu() == torch.as_tensor(y_new)).double().mean().item())
        e["elpd_per_row"] = float(r.elpd.sum().item()) / (K * M)
    tm = _each(fns, reps)
    e["launch_ms"] = _stats(tm["hip"])
    e["launch_ns_per_row_draw"] = 1e6 * e["launch_ms"]["median"] / (K * M * S)
    e["softmax_launch_ms"] = _stats(tm["softmax"])
    e["ordinal_over_softmax"] = e["launch_ms"]["median"] / e["softmax_launch_ms"]["median"]
    if not launch_only:
        e["end_to_end_ms"] = _stats(tm["whole"])
        e["pieces_ms"] = _stats(tm["pieces"])
        e["pieces_over_launch"] = e["pieces_ms"]["median"] / e["launch_ms"]["median"]
    e["launch_output_bytes"] = 8 * K * M * (C + 1)
    e["time_source"] = "device events around the calls (not profiler kernel time)"
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="three repetitions, K = 64")
    ap.add_argument("--launch-only", action="store_true", help="time the launch and its sibling alone")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 3 if args.quick else max(args.reps, 5)
    res = {"device": torch.cuda.get_device_name(0), "predict": []}
    for K, M, P, C, S in SHAPES:
        e = entry(64 if args.quick else K, M, P, C, S, reps, args.launch_only)
        res["predict"].append(e)
        print(json.dumps(e), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
