"""Batched Laplace initialiser benchmark (laplace_init_batched, csrc/gsmvi_laplace_batched.hip) on logistic posteriors, x0 = 0.

Writes one JSON object with, at K in {1024, 8192} x (N, D) in {(64, 10), (256, 16), (1024, 64)}, all in one process:
  calls[]    laplace_init_batched (defaults: gtol 1e-8) against lbfgs_init_batched (defaults: gtol 1e-5) on the same posteriors:
             the wall time of one call (device-synchronised host clock, after a warm-up call, --reps >= 10 calls alternated,
             median and range), the rounds that ran (nlaunch), the kernel launches they cost (one per Newton round plus the
             final inverse; three per L-BFGS round plus the dense product), the largest nit / nfev, how many converged, and
             the largest |score| the existing score kernel finds at each answer
  hessian[]  entry point (a) alone (H only, device events, alternated with the torch version) against the same Hessian as
             torch ops: the link in torch (sigmoid), w = s (1 - s), torch.baddbmm(lam I, (w[..., None] * A).mT, A); the largest
             difference between the two; the Gram product's rate 2 K N D^2 flop / time as a fraction of 47 TF (the fp64 MFMA
             rate this chip sustains) and the rate on the bytes of A, 8 K N D / time, as a fraction of
             8 TB/s; ``binds`` names the larger fraction.  The time is device-event time around one launch (launch gap
             included), not profiler kernel time: the fractions are those of the launch as a caller sees it
  step[]     one Newton round on a state two rounds in (nobody stopped; restored outside the timed region), device events
Usage: python scripts/laplace_batched_bench.py [--out FILE] [--reps R] [--quick]
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

HBM_BYTES_PER_S = 8.0e12
MFMA_F64_FLOPS = 47.0e12
SHAPES = [(64, 10), (256, 16), (1024, 64)]
LAM = 0.5


def problems(K, N, D, seed):
    """K synthetic data sets on the device: A ~ N(0, 1) / sqrt(D), y ~ Bernoulli(sigmoid(A theta*)), theta* ~ N(0, 1)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(K, N, D, dtype=torch.float64, device="cuda", generator=g) / np.sqrt(D)
    theta = torch.randn(K, D, 1, dtype=torch.float64, device="cuda", generator=g)
    y = (torch.rand(K, N, dtype=torch.float64, device="cuda", generator=g) < torch.sigmoid(torch.bmm(A, theta)[:, :, 0])).double()
    return A, y


def _stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def _wall(fns, reps):
    """seconds of every fns[name]() by a device-synchronised host clock, alternated, after a warm-up call of each"""
    out, last = {k: [] for k in fns}, {}
    for r in range(reps + 1):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = f()
            torch.cuda.synchronize()
            if r >= 1:
                out[k].append(time.perf_counter() - t0)
    return out, last


def _each(fns, reps):
    """per-call device-event times (ms) of the callables, alternated; fns[name] = (prepare or None, launch)"""
    out = {k: [] for k in fns}
    for r in range(reps + 3):
        for k, (prep, f) in fns.items():
            if prep is not None:
                prep()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            if r >= 3:
                out[k].append(a.elapsed_time(b))
    return out


def call_entry(tgt, K, N, D, reps):
    x0 = torch.zeros(K, D, dtype=torch.float64, device="cuda")
    t, last = _wall({"laplace": lambda: gsmvi_amd.laplace_init_batched(tgt, x0, as_torch=True),
                     "lbfgs": lambda: gsmvi_amd.lbfgs_init_batched(x0, tgt.lp, tgt.lp_g, as_torch=True)}, reps)
    e = {"K": K, "N": N, "D": D, "reps": reps}
    for name in ("laplace", "lbfgs"):
        mean, _, res = last[name]
        score = tgt.lp_g(mean.reshape(K, 1, D))
        launches = res.nlaunch + 1 if name == "laplace" else 3 * res.nlaunch + 1
        e[name] = {"call_s": _stats(t[name]), "nlaunch": res.nlaunch, "kernel_launches": launches, "nit_max": int(res.nit.max()),
                   "nfev_max": int(res.nfev.max()), "converged": int(res.success.sum()),
                   "score_max": float(score.abs().max().item())}
    e["lbfgs_over_laplace"] = e["lbfgs"]["call_s"]["median"] / e["laplace"]["call_s"]["median"]
    return e


def hessian_entry(tgt, K, N, D, reps):
    eng = tgt.engine
    g = torch.Generator(device="cuda").manual_seed(5)
    X = 0.5 * torch.randn(K, D, dtype=torch.float64, device="cuda", generator=g)
    H = eng.empty(K, D, D)
    lamI = (LAM * torch.eye(D, dtype=torch.float64, device="cuda")).expand(K, D, D)

    def torch_hessian():
        s = torch.sigmoid(torch.bmm(tgt.A, X[:, :, None])[:, :, 0])
        w = s * (1.0 - s)
        return torch.baddbmm(lamI, (w[..., None] * tgt.A).mT, tgt.A)

    def hip_hessian():
        return eng.glm_hessian_batched(X, tgt.A, tgt.y, "logistic", prior_prec=LAM, want="h", out=H)

    diff = float((hip_hessian() - torch_hessian()).abs().max().item())
    t = _each({"hip": (None, hip_hessian), "torch": (None, torch_hessian)}, reps)
    e = {"K": K, "N": N, "D": D, "reps": reps, "hip_ms": _stats(t["hip"]), "torch_ms": _stats(t["torch"]), "max_abs_diff": diff}
    sec = e["hip_ms"]["median"] * 1e-3
    e["torch_over_hip"] = e["torch_ms"]["median"] / e["hip_ms"]["median"]
    e["gram_flops_per_s"] = 2.0 * K * N * D * D / sec
    e["mfma_fraction"] = e["gram_flops_per_s"] / MFMA_F64_FLOPS
    e["a_bytes_per_s"] = 8.0 * K * N * D / sec
    e["hbm_fraction"] = e["a_bytes_per_s"] / HBM_BYTES_PER_S
    e["time_source"] = "device events around one launch (not profiler kernel time)"
    e["binds"] = "hbm (the bytes of A)" if e["hbm_fraction"] >= e["mfma_fraction"] else "fp64 mfma"
    return e


def step_entry(tgt, K, N, D, reps):
    eng = tgt.engine
    st = eng.laplace_state_batched(eng.zeros(K, D))
    opt = dict(prior_prec=LAM, gtol=0.0)
    for r in range(2):
        eng.laplace_step_batched(st, tgt.A, tgt.y, "logistic", start=r == 0, **opt)
    saved = {k: v.clone() for k, v in st.items()}
    assert int(saved["ist"][:, 0].abs().max().item()) == 0

    def restore():
        for k, v in saved.items():
            st[k].copy_(v)

    t = _each({"step": (restore, lambda: eng.laplace_step_batched(st, tgt.A, tgt.y, "logistic", **opt))}, reps)
    e = {"K": K, "N": N, "D": D, "reps": reps, "step_ms": _stats(t["step"])}
    e["a_bytes_per_s"] = 8.0 * K * N * D / (e["step_ms"]["median"] * 1e-3)
    e["hbm_fraction"] = e["a_bytes_per_s"] / HBM_BYTES_PER_S
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="few repetitions, K = 1024 only")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 3 if args.quick else max(args.reps, 10)
    res = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S, "mfma_f64_flops_per_s": MFMA_F64_FLOPS,
           "prior_precision": LAM, "calls": [], "hessian": [], "step": []}
    for K in ((1024,) if args.quick else (1024, 8192)):
        for N, D in SHAPES:
            A, y = problems(K, N, D, 11)
            tgt = gsmvi_amd.BatchedLogisticTarget(A, y, LAM)
            for key, fn, n in (("calls", call_entry, reps), ("hessian", hessian_entry, 3 * reps), ("step", step_entry, 3 * reps)):
                e = fn(tgt, K, N, D, n)
                res[key].append(e)
                print(json.dumps({key: e}), flush=True)
            del tgt, A, y
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
