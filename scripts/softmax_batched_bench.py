"""Batched softmax target benchmark (BatchedSoftmaxTarget, gsmvi_softmax_batched_f64 in csrc/gsmvi_softmax_batched.hip): the score
of K multinomial logit posteriors against the same score written as torch ops, alone and inside GSMBatch.fit.

Writes one JSON object with
  calls[]   at K = 8192 x (N, C, P, B) in {(64, 3, 5, 2), (256, 5, 4, 8), (1024, 9, 8, 8)}: call_ms, the score call as a user
            makes it (``tgt.lp_g(x)``: the output allocated by the call); kernel_ms, the launch alone (``out=`` given); torch_ms, the
            same score as torch ops on the same device arrays (torch.bmm for eta, torch.softmax over the C classes with the
            reference class's zero appended -- exp(log_softmax), in one op --, the one-hot labels, torch.baddbmm back); lp_ms and
            both_ms, the density alone and both outputs.  All alternated in one process; per call one pair of device events,
            --reps (10) calls after a warm-up, median and range; ratio = torch median / kernel median, ratio_call = torch median /
            call median.  The speed is reported, not gated.
  fits[]    at the same shapes GSMBatch.fit of --niter iterations scored by the target and by the torch score, alternated,
            --reps fits each between device events (the fit's own host work included): hip_fit_ms, torch_fit_ms, ratio.
Usage: python scripts/softmax_batched_bench.py [--out FILE] [--reps R] [--niter T] [--quick]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gsmvi_amd  # noqa: E402

SHAPES = [(64, 3, 5, 2), (256, 5, 4, 8), (1024, 9, 8, 8)]
K_BENCH = 8192
LAM = 0.5
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batched",
                           "softmax_batched_bench.json")


def problems(K, N, Cc, P, seed):
    """K synthetic data sets on the device: A ~ N(0, 1) / sqrt(P), labels drawn from the model at W* ~ N(0, 1)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)      # noqa: E731
    A = rn(K, N, P) / np.sqrt(P)
    eta = torch.cat([torch.bmm(A, rn(K, P, Cc - 1)), torch.zeros(K, N, 1, dtype=torch.float64, device="cuda")], dim=2)
    y = torch.multinomial(torch.softmax(eta, 2).reshape(K * N, Cc), 1, generator=g).reshape(K, N)
    return A, y


def torch_score(A, y, Cc, lam):
    """the same score as torch ops on the device, in the form a torch user would write"""
    K, N, P = A.shape
    At = A.transpose(1, 2)
    hot = torch.nn.functional.one_hot(y, Cc)[:, :, :Cc - 1].to(torch.float64).transpose(1, 2).contiguous()[:, None]   # (K, 1, C-1, N)

    @gsmvi_amd.device_score
    def lp_g(x):
        B = x.shape[1]
        W = x.reshape(K, B * (Cc - 1), P)
        eta = torch.bmm(W, At).reshape(K, B, Cc - 1, N)
        full = torch.cat([eta, eta.new_zeros(K, B, 1, N)], dim=2)
        r = hot - torch.softmax(full, dim=2)[:, :, :Cc - 1]
        return torch.baddbmm(W, r.reshape(K, B * (Cc - 1), N), A, beta=-lam).reshape(K, B, (Cc - 1) * P)
    return lp_g


def _each(fns, reps, warm=3):
    """per-call device-event times (ms) of the callables, alternated: {name: [ms] * reps}"""
    for _ in range(warm):
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


def shape_entries(K, N, Cc, P, B, reps, niter):
    eng = gsmvi_amd.get_engine()
    D = (Cc - 1) * P
    A, y = problems(K, N, Cc, P, 11)
    tgt = gsmvi_amd.BatchedSoftmaxTarget(A, y, Cc, LAM)
    tscore = torch_score(A, y, Cc, LAM)
    x = torch.randn(K, B, D, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    G, lpo = eng.empty(K, B, D), eng.empty(K, B)
    ref = tscore(x)
    err = float((ref - tgt.lp_g(x)).abs().max() / ref.abs().max())
    assert err < 1e-9, err
    t = _each({"call": lambda: tgt.lp_g(x), "kernel": lambda: tgt.lp_g(x, out=G), "torch": lambda: tscore(x),
               "lp": lambda: tgt._call(x, lp_out=lpo, want="lp"), "both": lambda: tgt._call(x, out=G, lp_out=lpo, want="both")}, reps)
    e = {"K": K, "N": N, "C": Cc, "P": P, "D": D, "B": B, "reps": reps, "call_ms": _stats(t["call"]), "kernel_ms": _stats(t["kernel"]),
         "torch_ms": _stats(t["torch"]), "lp_ms": _stats(t["lp"]), "both_ms": _stats(t["both"]), "max_rel_diff_vs_torch": err}
    e["ratio"] = e["torch_ms"]["median"] / e["kernel_ms"]["median"]
    e["ratio_call"] = e["torch_ms"]["median"] / e["call_ms"]["median"]
    keys = np.arange(K) + 3
    fit = lambda lpg: gsmvi_amd.GSMBatch(K, D, tgt.lp, lpg).fit(keys, batch_size=B, niter=niter, verbose=False)    # noqa: E731
    tf = _each({"hip": lambda: fit(tgt.lp_g), "torch": lambda: fit(tscore)}, reps, warm=1)
    f = {"K": K, "N": N, "C": Cc, "P": P, "D": D, "B": B, "reps": reps, "niter": niter, "hip_fit_ms": _stats(tf["hip"]),
         "torch_fit_ms": _stats(tf["torch"])}
    f["ratio"] = f["torch_fit_ms"]["median"] / f["hip_fit_ms"]["median"]
    return e, f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--niter", type=int, default=50)
    ap.add_argument("--quick", action="store_true", help="3 repetitions, K = 512, 10 iterations")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps, niter, K = (3, 10, 512) if args.quick else (args.reps, args.niter, K_BENCH)
    res = {"device": torch.cuda.get_device_name(0), "K": K, "prior_precision": LAM, "calls": [], "fits": []}
    for N, Cc, P, B in SHAPES:
        e, f = shape_entries(K, N, Cc, P, B, reps, niter)
        res["calls"].append(e)
        res["fits"].append(f)
        print(json.dumps(e), flush=True)
        print(json.dumps(f), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
