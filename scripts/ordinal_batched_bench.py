"""Batched ordinal target benchmark (BatchedOrdinalTarget, gsmvi_ordinal_batched_f64 in csrc/gsmvi_ordinal_batched.hip): the score,
density and both-output launches against the same score and density written as torch ops, against the softmax launch on the same
data where its (C - 1) P <= 64 allows it, and GSMBatch.fit scored by the target against the fit scored by the torch score.

Writes one JSON object with
  calls[]  at K in {8192, 1024} x (N, D, B) in {(64, 10, 2), (256, 16, 8), (1024, 64, 8)} with C = 5 classes (D = P + 4): hip_ms (the
           score launch), torch_ms (torch.baddbmm for eta, torch.gather of the padded cutpoints, sigmoid, torch.scatter_add_ into
           the cutpoints, a reversed cumsum, torch.baddbmm back), lp_ms and both_ms of the target, torch_lp_ms (the density as torch
           ops: torch.baddbmm, torch.gather, logsigmoid twice), softmax_ms (BatchedSoftmaxTarget's score launch on the same A and
           labels at its own (C - 1) P parameters; null where (C - 1) P > 64), alternated in one process; per call one pair of
           device events, the median of --reps (>= 20) calls after a warm-up, with the range; ratio = torch median / hip median,
           lp_ratio the same for the density, vs_softmax = softmax median / hip median.  Reported, not gated.
  fits[]   at K = 1024, (N, D, B) = (256, 16, 8): GSMBatch.fit over --niter iterations scored by the target and by the torch
           score (both device-native), wall-clock with a synchronise, the median of 5 alternated runs; ratio = torch / target
Usage: python scripts/ordinal_batched_bench.py [--out FILE] [--reps R] [--niter T] [--quick]
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
C = 5
LAM, KAP = 0.5, 0.3
BIG = 1e300                                     # stands in for the cutpoints -inf and +inf: every sigmoid and softplus saturates


def problems(K, N, P, seed):
    """K synthetic rating data sets on the device: A ~ N(0, 1) / sqrt(P), offsets 0.3 N(0, 1), labels drawn from the model at
    beta* ~ N(0, 1) and cutpoints (-1.5, -0.5, 0.5, 1.5)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)      # noqa: E731
    A = rn(K, N, P) / np.sqrt(P)
    o = 0.3 * rn(K, N)
    eta = torch.bmm(A, rn(K, P, 1))[:, :, 0] + o
    cuts = torch.linspace(-1.5, 1.5, C - 1, dtype=torch.float64, device="cuda")
    u = torch.rand(K, N, dtype=torch.float64, device="cuda", generator=g)
    y = (u[:, :, None] > torch.sigmoid(cuts[None, None, :] - eta[:, :, None])).sum(2)
    return A, y, o


def _pieces(A, y, o):
    return A.transpose(1, 2), o[:, None, :], y[:, None, :]


def _cuts(x, P):
    """(beta, delta, w = exp(delta_j) for j >= 1, the cutpoints padded with -BIG and BIG)"""
    beta, delta = x[:, :, :P], x[:, :, P:]
    w = torch.exp(delta[:, :, 1:])
    cut = torch.cumsum(torch.cat([delta[:, :, :1], w], dim=2), dim=2)
    pad = torch.full_like(cut[:, :, :1], BIG)
    return beta, delta, w, torch.cat([-pad, cut, pad], dim=2)


def torch_score(A, y, o, lam, kap):
    """the same score as torch ops on the device, in the form a torch user would write from the stable forms"""
    At, ob, yb = _pieces(A, y, o)
    P = A.shape[2]

    @gsmvi_amd.device_score
    def lp_g(x):
        beta, delta, w, cpad = _cuts(x, P)
        B = x.shape[1]
        ylo = yb.expand(-1, B, -1)
        eta = torch.baddbmm(ob, beta, At)
        a = torch.gather(cpad, 2, ylo) - eta
        nb = eta - torch.gather(cpad, 2, ylo + 1)
        z = torch.zeros_like(w[:, :, :1])
        q = torch.gather(torch.cat([z, 1.0 / torch.expm1(w), z], dim=2), 2, ylo)
        sa, sb = torch.sigmoid(a), torch.sigmoid(nb)
        gb = torch.baddbmm(beta, sa - sb, A, beta=-lam)
        gc = torch.zeros_like(cpad)
        gc.scatter_add_(2, ylo, -sa - q)
        gc.scatter_add_(2, ylo + 1, sb + q)
        sfx = torch.flip(torch.cumsum(torch.flip(gc[:, :, 1:C], dims=[2]), dim=2), dims=[2])
        gd = torch.cat([sfx[:, :, :1], w * sfx[:, :, 1:]], dim=2) - kap * delta
        return torch.cat([gb, gd], dim=2)
    return lp_g


def torch_lp(A, y, o, lam, kap):
    At, ob, yb = _pieces(A, y, o)
    P = A.shape[2]

    def lp(x):
        beta, delta, w, cpad = _cuts(x, P)
        ylo = yb.expand(-1, x.shape[1], -1)
        eta = torch.baddbmm(ob, beta, At)
        a = torch.gather(cpad, 2, ylo) - eta
        b = torch.gather(cpad, 2, ylo + 1) - eta
        z = torch.zeros_like(w[:, :, :1])
        lm = torch.where(w < 0.6931471805599453, torch.log(-torch.expm1(-w)), torch.log1p(-torch.exp(-w)))
        ls = torch.nn.functional.logsigmoid
        t = ls(b) + ls(-a) + torch.gather(torch.cat([z, lm, z], dim=2), 2, ylo)
        return t.sum(2) - 0.5 * lam * (beta * beta).sum(2) - 0.5 * kap * (delta * delta).sum(2)
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


def _start(K, B, P, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)      # noqa: E731
    return torch.cat([0.5 * rn(K, B, P), rn(K, B, 1), -0.5 + 0.7 * rn(K, B, C - 2)], dim=2).contiguous()


def call_entry(K, N, D, B, reps):
    eng = gsmvi_amd.get_engine()
    P = D - (C - 1)
    A, y, o = problems(K, N, P, 11)
    x = _start(K, B, P, 5)
    G, lpo = eng.empty(K, B, D), eng.empty(K, B)
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, C, LAM, KAP, offset=o)
    tscore, tlp = torch_score(A, y, o, LAM, KAP), torch_lp(A, y, o, LAM, KAP)
    ref = tscore(x)
    err = float((ref - tgt.lp_g(x)).abs().max() / ref.abs().max())
    assert err < 1e-9, err
    lref = tlp(x)
    err_lp = float((lref - tgt.lp(x)).abs().max() / lref.abs().max())
    assert err_lp < 1e-9, err_lp
    fns = {"hip": lambda: tgt.lp_g(x, out=G), "torch": lambda: tscore(x),
           "lp": lambda: tgt._call(x, lp_out=lpo, want="lp"), "both": lambda: tgt._call(x, out=G, lp_out=lpo, want="both"),
           "torch_lp": lambda: tlp(x)}
    if (C - 1) * P <= 64:                                                   # the unordered model on the same data, where it fits
        sm = gsmvi_amd.BatchedSoftmaxTarget(A, y, C, LAM)
        xs = 0.5 * torch.randn(K, B, (C - 1) * P, dtype=torch.float64, device="cuda")
        Gs = eng.empty(K, B, (C - 1) * P)
        fns["softmax"] = lambda: sm.lp_g(xs, out=Gs)
    t = _each(fns, reps)
    e = {"K": K, "N": N, "D": D, "P": P, "C": C, "B": B, "reps": reps, "hip_ms": _stats(t["hip"]), "torch_ms": _stats(t["torch"]),
         "lp_ms": _stats(t["lp"]), "both_ms": _stats(t["both"]), "torch_lp_ms": _stats(t["torch_lp"]),
         "softmax_ms": _stats(t["softmax"]) if "softmax" in t else None, "softmax_D": (C - 1) * P if "softmax" in t else None,
         "max_rel_diff_vs_torch": err, "max_rel_diff_lp_vs_torch": err_lp}
    e["ratio"] = e["torch_ms"]["median"] / e["hip_ms"]["median"]
    e["lp_ratio"] = e["torch_lp_ms"]["median"] / e["lp_ms"]["median"]
    e["vs_softmax"] = e["softmax_ms"]["median"] / e["hip_ms"]["median"] if e["softmax_ms"] else None
    return e


def fit_entry(K, N, D, B, niter, runs=5):
    P = D - (C - 1)
    A, y, o = problems(K, N, P, 13)
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, C, LAM, KAP, offset=o)
    tscore, tlp = torch_score(A, y, o, LAM, KAP), torch_lp(A, y, o, LAM, KAP)
    keys = np.arange(K) + 3
    mean0 = np.zeros((K, D))
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
    e = {"K": K, "N": N, "D": D, "P": P, "C": C, "B": B, "niter": niter, "runs": runs, "target_ms": _stats(times["target"]),
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
    res = {"device": torch.cuda.get_device_name(0), "num_classes": C, "prior_precision": LAM, "cut_precision": KAP, "calls": [],
           "fits": []}
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
