"""Batched PSIS diagnostic benchmark (gsmvi_psis_batched_f64, csrc/gsmvi_psis_batched.hip).

Writes one JSON object with, at (K, D, S) in {(1024, 10, 1024), (8192, 64, 1024)}, with and without the moments, all in one process:
  psis[]  ``psis_batched`` end to end on a BatchedGaussianTarget (the draw launch, ``lp_rows``, the PSIS launch; device tensors
          out, so no copy to the host is timed), the PSIS launch alone (one call of the engine method on the same draws), and
          the launch's computation as torch ops in the same run, alternated: ``linalg.cholesky`` + ``solve_triangular`` for
          log q, ``torch.sort`` over the batch, the tail fit vectorised over K (every tail has the full M entries: the ratios
          are continuous), ``scatter_`` back to row order, an ``einsum`` for the moments; the largest difference between the
          two per output; the ratio torch / launch (recorded, not required).  Times are device-event times around the calls
          (launch gaps included), not profiler kernel time.
Usage: python scripts/psis_batched_bench.py [--out FILE] [--reps R] [--quick]
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

SHAPES = [(1024, 10, 1024), (8192, 64, 1024)]
LOG_DBL_MIN = math.log(np.finfo(np.float64).tiny)


def problems(K, D, seed):
    """K Gaussian targets and fitted Gaussians a little narrower than them (tail shape about 0.2): (target, mean, cov)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)      # noqa: E731
    mt = rn(K, D)
    G = rn(K, D, D) / math.sqrt(D)
    ct = 0.5 * torch.eye(D, dtype=torch.float64, device="cuda")[None] + torch.bmm(G, G.mT)
    tgt = gsmvi_amd.BatchedGaussianTarget(mt.cpu().numpy(), cov=ct.cpu().numpy())
    return tgt, mt + 0.05 * rn(K, D), ct / 1.25


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


def torch_psis(mean, cov, X, lp, moments):
    """the launch's computation as torch ops: (logr, lw, khat, ess, log_z, mean_is, cov_is)"""
    K, S, D = X.shape
    L = torch.linalg.cholesky(cov)
    d = X - mean[:, None, :]
    w = torch.linalg.solve_triangular(L, d.mT, upper=False)
    logq = -0.5 * (w * w).sum(1) - torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)[:, None] - 0.5 * D * math.log(2 * math.pi)
    logr = lp - logq
    mx = logr.max(1, keepdim=True).values
    srt, order = torch.sort(logr - mx, dim=1, stable=True)
    M = int(math.ceil(min(S / 5.0, 3.0 * math.sqrt(S))))
    cut = srt[:, S - M - 1].clamp_min(LOG_DBL_MIN)
    ec = torch.exp(cut)[:, None]
    x = torch.exp(srt[:, S - M:]) - ec
    m = 30 + int(math.floor(math.sqrt(M)))
    j = torch.arange(1, m + 1, dtype=torch.float64, device=X.device)
    b = (1.0 - torch.sqrt(m / (j - 0.5)))[None, :] / (3.0 * x[:, (M + 2) // 4 - 1])[:, None] + (1.0 / x[:, -1])[:, None]
    kap = torch.log1p(-b[:, :, None] * x[:, None, :]).mean(2)
    Lj = M * (torch.log(-b / kap) - kap - 1.0)
    om = 1.0 / torch.exp(Lj[:, None, :] - Lj[:, :, None]).sum(2)
    om = torch.where(om < 10 * np.finfo(np.float64).eps, torch.zeros_like(om), om)
    om = om / om.sum(1, keepdim=True)
    bb = (om * b).sum(1)
    kappa = torch.log1p(-bb[:, None] * x).mean(1)
    sigma, khat = -kappa / bb, (M * kappa + 5.0) / (M + 10.0)
    p = (torch.arange(M, dtype=torch.float64, device=X.device) + 0.5) / M
    q = sigma[:, None] * torch.expm1(-khat[:, None] * torch.log1p(-p)[None, :]) / khat[:, None]
    srt = torch.cat([srt[:, :S - M], torch.log(q + ec)], 1).clamp_max(0.0)
    lse = torch.logsumexp(srt, 1, keepdim=True)
    lw = torch.empty_like(srt).scatter_(1, order, srt - lse)
    ess = 1.0 / torch.exp(2.0 * (srt - lse)).sum(1)
    log_z = (lse + mx)[:, 0] - math.log(S)
    if not moments:
        return logr, lw, khat, ess, log_z, None, None
    wt = torch.exp(lw)
    m1 = (wt[:, :, None] * d).sum(1)
    C2 = torch.einsum("ks,ksi,ksj->kij", wt, d, d) - m1[:, :, None] * m1[:, None, :]
    return logr, lw, khat, ess, log_z, mean + m1, C2


def entry(K, D, S, moments, reps):
    eng = gsmvi_amd.get_engine()
    tgt, mean, cov = problems(K, D, 11)
    keys = list(range(K))
    first = gsmvi_amd.psis_batched(tgt.lp_rows, mean, cov, keys, num_draws=S, moments=moments, as_torch=True)
    X, lp = first.samples, tgt.lp_rows(first.samples)
    whole = lambda: gsmvi_amd.psis_batched(tgt.lp_rows, mean, cov, keys, num_draws=S, moments=moments, as_torch=True)   # noqa: E731
    hip = lambda: eng.psis_batched(mean, cov, X, lp, moments=moments)                   # noqa: E731
    ref = lambda: torch_psis(mean, cov, X, lp, moments)                                 # noqa: E731
    diffs = {}
    names = ("logr", "lw", "khat", "ess", "log_z", "mean_is", "cov_is")
    for name, a, b in zip(names, hip()[:7], ref()):
        if a is not None:
            diffs[name] = float(((a - b).abs() / b.abs().clamp_min(1.0)).max().item())
    tm = _each({"whole": whole, "hip": hip, "torch": ref}, reps)
    e = {"K": K, "D": D, "S": S, "moments": moments, "reps": reps, "end_to_end_ms": _stats(tm["whole"]),
         "launch_ms": _stats(tm["hip"]), "torch_ms": _stats(tm["torch"]), "max_rel_diff": diffs,
         "share_ok": float(first.ok.double().mean().item()), "khat_median": float(first.khat.median().item())}
    e["torch_over_launch"] = e["torch_ms"]["median"] / e["launch_ms"]["median"]
    e["sample_block_bytes"] = 8 * K * S * D
    e["time_source"] = "device events around the calls (not profiler kernel time)"
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="three repetitions, K = 256")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 3 if args.quick else max(args.reps, 5)
    res = {"device": torch.cuda.get_device_name(0), "psis": []}
    for K, D, S in SHAPES:
        for moments in (True, False):
            e = entry(256 if args.quick else K, D, S, moments, reps)
            res["psis"].append(e)
            print(json.dumps(e), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
