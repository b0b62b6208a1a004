"""Batched negative binomial target benchmark (BatchedNegBinomialTarget, gsmvi_negbin_batched_f64 in
csrc/gsmvi_negbin_batched.hip): the score launch against the same score written as torch ops and against the Poisson launch of
gsmvi_glm_batched_f64 at the same shape, and GSMBatch.fit scored by the target against the fit scored by the torch score.

Writes one JSON object with
  calls[]  at K in {8192, 1024} x (N, D, B) in {(64, 10, 2), (256, 16, 8), (1024, 64, 8)} (D = P + 1): hip_ms (the score launch),
           torch_ms (torch.baddbmm for eta, torch.digamma twice, softplus, sigmoid, torch.baddbmm back and a row sum for the last
           component), poisson_ms (glm_batched, family poisson, on the same A, y, offset at beta), lp_ms and both_ms of the
           target and torch_lp_ms (the density as torch ops: torch.baddbmm, torch.lgamma twice, softplus twice),
           alternated in one process; per call one pair of device events, the median of --reps (>= 20) calls after a warm-up,
           with the range; ratio = torch median / hip median, link_cost = hip median / poisson median.  Reported, not gated.
  fits[]   at K = 1024, (N, D, B) = (256, 16, 8): GSMBatch.fit over --niter iterations scored by the target and by the torch
           score (both device-native), wall-clock with a synchronise, the median of 5 alternated runs; ratio = torch / target
Usage: python scripts/negbin_batched_bench.py [--out FILE] [--reps R] [--niter T] [--quick]
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

SHAPES = [(64, 10, 2), (256, 16, 8), (1024, 64, 8)]
KS = (8192, 1024)
LAM, TM, TK = 0.5, 1.0, 0.3


def problems(K, N, P, seed):
    """K synthetic count data sets on the device: A ~ N(0, 1) / sqrt(P), offsets 0.3 N(0, 1), y negative binomial at beta* ~
    N(0, 1) with size e^U(0, 3)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)      # noqa: E731
    A = rn(K, N, P) / np.sqrt(P)
    o = 0.3 * rn(K, N)
    mu = torch.exp(torch.bmm(A, rn(K, P, 1))[:, :, 0] + o)
    size = torch.exp(3.0 * torch.rand(K, 1, dtype=torch.float64, device="cuda", generator=g))
    # gamma-Poisson mixture (drawn on the host generator of torch.distributions: the data, not the timing)
    lamb = torch.distributions.Gamma(size.expand_as(mu), size / mu).sample()
    y = torch.poisson(lamb, generator=g)
    return A, y, o


def torch_score(A, y, o, lam, tm, tk):
    """the same score as torch ops on the device, in the form a torch user would write"""
    At, ob, yb = A.transpose(1, 2), o[:, None, :], y[:, None, :]
    P = A.shape[2]

    @gsmvi_amd.device_score
    def lp_g(x):
        beta, th = x[:, :, :P], x[:, :, P:]
        r = torch.exp(th)
        d = torch.baddbmm(ob, beta, At) - th
        re = yb * torch.sigmoid(-d) - r * torch.sigmoid(d)
        rt = r * (torch.digamma(yb + r) - torch.digamma(r) - torch.nn.functional.softplus(d)) - re
        gb = torch.baddbmm(beta, re, A, beta=-lam)
        return torch.cat([gb, rt.sum(2, keepdim=True) - tk * (th - tm)], dim=2)
    return lp_g


def torch_lp(A, y, o, lam, tm, tk):
    At, ob, yb = A.transpose(1, 2), o[:, None, :], y[:, None, :]
    P = A.shape[2]

    def lp(x):
        beta, th = x[:, :, :P], x[:, :, P:]
        r = torch.exp(th)
        d = torch.baddbmm(ob, beta, At) - th
        sp = torch.nn.functional.softplus
        t = torch.lgamma(yb + r) - torch.lgamma(r) - r * sp(d) - yb * sp(-d)
        return t.sum(2) - 0.5 * lam * (beta * beta).sum(2) - 0.5 * tk * (th[:, :, 0] - tm) ** 2
    return lp


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


def call_entry(K, N, D, B, reps):
    eng = gsmvi_amd.get_engine()
    P = D - 1
    A, y, o = problems(K, N, P, 11)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.cat([0.5 * torch.randn(K, B, P, dtype=torch.float64, device="cuda", generator=g),
                   3.0 * torch.rand(K, B, 1, dtype=torch.float64, device="cuda", generator=g)], dim=2).contiguous()
    beta = x[:, :, :P].contiguous()
    G, lpo, Gp = eng.empty(K, B, D), eng.empty(K, B), eng.empty(K, B, P)
    tgt = gsmvi_amd.BatchedNegBinomialTarget(A, y, LAM, offset=o, log_size_mean=TM, log_size_precision=TK)
    tscore, tlp = torch_score(A, y, o, LAM, TM, TK), torch_lp(A, y, o, LAM, TM, TK)
    ref = tscore(x)
    err = float((ref - tgt.lp_g(x)).abs().max() / ref.abs().max())
    assert err < 1e-9, err
    lref = tlp(x)
    err_lp = float((lref - tgt.lp(x)).abs().max() / lref.abs().max())
    fns = {"hip": lambda: tgt.lp_g(x, out=G), "torch": lambda: tscore(x),
           "poisson": lambda: eng.glm_batched(beta, tgt.A, tgt.y, "poisson", offset=tgt.offset, prior_prec=LAM, out=Gp, want="g"),
           "lp": lambda: tgt._call(x, lp_out=lpo, want="lp"), "both": lambda: tgt._call(x, out=G, lp_out=lpo, want="both"),
           "torch_lp": lambda: tlp(x)}
    t = _each(fns, reps)
    e = {"K": K, "N": N, "D": D, "B": B, "reps": reps, "hip_ms": _stats(t["hip"]), "torch_ms": _stats(t["torch"]),
         "poisson_ms": _stats(t["poisson"]), "lp_ms": _stats(t["lp"]), "both_ms": _stats(t["both"]),
         "torch_lp_ms": _stats(t["torch_lp"]), "max_rel_diff_vs_torch": err, "max_rel_diff_lp_vs_torch": err_lp}
    e["ratio"] = e["torch_ms"]["median"] / e["hip_ms"]["median"]
    e["lp_ratio"] = e["torch_lp_ms"]["median"] / e["lp_ms"]["median"]
    e["link_cost"] = e["hip_ms"]["median"] / e["poisson_ms"]["median"]
    return e


def fit_entry(K, N, D, B, niter, runs=5):
    P = D - 1
    A, y, o = problems(K, N, P, 13)
    tgt = gsmvi_amd.BatchedNegBinomialTarget(A, y, LAM, offset=o, log_size_mean=TM, log_size_precision=TK)
    tscore, tlp = torch_score(A, y, o, LAM, TM, TK), torch_lp(A, y, o, LAM, TM, TK)
    keys = np.arange(K) + 3
    mean0 = np.zeros((K, D))
    mean0[:, -1] = 1.0
    sides = {"target": (tgt.lp, tgt.lp_g), "torch": (tlp, tscore)}
    times, out = {k: [] for k in sides}, {}
    for r in range(runs + 1):                                               # (the first round is the warm-up)
        for name, (lp, lpg) in sides.items():
            fit = gsmvi_amd.GSMBatch(K, D, lp, lpg)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m, c = fit.fit(keys, mean=mean0, batch_size=B, niter=niter, verbose=False, as_torch=True)
            torch.cuda.synchronize()
            if r:
                times[name].append(1e3 * (time.perf_counter() - t0))
            out[name] = m
    e = {"K": K, "N": N, "D": D, "B": B, "niter": niter, "runs": runs, "target_ms": _stats(times["target"]),
         "torch_ms": _stats(times["torch"]),
         "max_rel_diff_mean": float((out["target"] - out["torch"]).abs().max() / out["torch"].abs().max())}
    e["ratio"] = e["torch_ms"]["median"] / e["target_ms"]["median"]
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--niter", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="few repetitions, K = 256")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 5 if args.quick else max(args.reps, 20)
    res = {"device": torch.cuda.get_device_name(0), "prior_precision": LAM, "log_size_mean": TM, "log_size_precision": TK,
           "calls": [], "fits": []}
    for K in ((256,) if args.quick else KS):
        for N, D, B in SHAPES:
            e = call_entry(K, N, D, B, reps)
            res["calls"].append(e)
            print(json.dumps(e), flush=True)
    e = fit_entry(256 if args.quick else 1024, 256, 16, 8, 20 if args.quick else args.niter, runs=2 if args.quick else 5)
    res["fits"].append(e)
    print(json.dumps(e), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
