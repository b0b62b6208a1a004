"""Batched Pathfinder initialiser benchmark (pathfinder_init_batched, csrc/gsmvi_pathfinder_batched.hip) on logistic posteriors,
x0 = 0.

Writes one JSON object with, at K in {1024, 8192} x (N, D) in {(64, 10), (256, 16), (1024, 64)}, all in one process:
  calls[]    pathfinder_init_batched (defaults: 5 draws per path point, the pair base) against lbfgs_init_batched on the same
             posteriors: the wall time of one call (device-synchronised host clock, after a warm-up call, --reps >= 10 calls
             alternated, median and range), the rounds that ran (nlaunch), the path points tried, how many problems got a start
  propose[]  the propose launch alone on a state three rounds in (every problem fresh: ``seen`` is reset outside the timed
             region), device events; the bytes it must move (the L-BFGS state in, mu, cov and the draws out) over that time
             as a fraction of 8 TB/s
  starts[]   the quality of the three starts as a start: the ELBO estimate mean(lp - log q) from 256 fresh draws and the PSIS
             khat of lbfgs_init_batched, laplace_init_batched and pathfinder_init_batched (``psis_batched``, one set of keys):
             medians over the problems and the share of problems with khat below the threshold
Reported, not gated.
Usage: python scripts/pathfinder_batched_bench.py [--out FILE] [--reps R] [--quick]
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
SHAPES = [(64, 10), (256, 16), (1024, 64)]
LAM = 0.5
DRAWS = 5


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


def call_entry(tgt, K, N, D, reps):
    x0 = torch.zeros(K, D, dtype=torch.float64, device="cuda")
    t, last = _wall({"pathfinder": lambda: gsmvi_amd.pathfinder_init_batched(x0, tgt.lp, tgt.lp_g, num_elbo_draws=DRAWS, as_torch=True),
                     "lbfgs": lambda: gsmvi_amd.lbfgs_init_batched(x0, tgt.lp, tgt.lp_g, as_torch=True)}, reps)
    e = {"K": K, "N": N, "D": D, "reps": reps, "num_elbo_draws": DRAWS}
    for name in ("pathfinder", "lbfgs"):
        res = last[name][2]
        e[name] = {"call_s": _stats(t[name]), "nlaunch": res.nlaunch, "kernel_launches": (6 if name == "pathfinder" else 3) * res.nlaunch,
                   "nit_max": int(res.nit.max()), "nfev_max": int(res.nfev.max()), "with_a_start": int(res.success.sum())}
    r = last["pathfinder"][2]
    e["pathfinder"].update(points_max=int(r.n_points.max()), best_it_median=float(np.median(r.best_it)),
                           best_is_last=int((r.best_it == r.nit).sum()), nevals=r.nevals)
    e["pathfinder_over_lbfgs"] = e["pathfinder"]["call_s"]["median"] / e["lbfgs"]["call_s"]["median"]
    return e


def propose_entry(tgt, K, N, D, reps):
    from gsmvi_amd.monitors import lp_sums
    eng = tgt.engine
    st = eng.lbfgs_state_batched(eng.zeros(K, D))
    Xt = st["Xt"].reshape(K, 1, D)
    for r in range(3):
        eng.lbfgs_step_batched(lp_sums(tgt.lp, Xt, eng, K).contiguous(), tgt.lp_g(Xt).reshape(K, D), st, start=r == 0, sign=-1.0,
                               gtol=0.0, ftol=0.0)
    pf = eng.pathfinder_state_batched(st["x"], DRAWS)
    seeds = eng.batched_seeds(range(K))
    ms = []
    for r in range(reps + 3):
        pf["seen"].fill_(-1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.pathfinder_propose_batched(st, pf, seeds)
        b.record()
        b.synchronize()
        if r >= 3:
            ms.append(a.elapsed_time(b))
    assert bool(pf["fresh"].all().item())
    held = st["ist"][:, 4].double()
    e = {"K": K, "N": N, "D": D, "reps": reps, "num_elbo_draws": DRAWS, "propose_ms": _stats(ms), "pairs_held_median": float(held.median().item())}
    e["bytes"] = 8.0 * K * (2 * D + 2 * D * float(held.mean().item()) + 24 + D + D * D + DRAWS * D + 1)
    e["bytes_per_s"] = e["bytes"] / (e["propose_ms"]["median"] * 1e-3)
    e["hbm_fraction"] = e["bytes_per_s"] / HBM_BYTES_PER_S
    e["time_source"] = "device events around one launch (not profiler kernel time)"
    return e


def starts_entry(tgt, K, N, D):
    x0 = torch.zeros(K, D, dtype=torch.float64, device="cuda")
    keys = np.arange(K) + 7
    starts = {"lbfgs": gsmvi_amd.lbfgs_init_batched(x0, tgt.lp, tgt.lp_g, as_torch=True),
              "laplace": gsmvi_amd.laplace_init_batched(tgt, x0, as_torch=True),
              "pathfinder": gsmvi_amd.pathfinder_init_batched(x0, tgt.lp, tgt.lp_g, num_elbo_draws=DRAWS, as_torch=True)}
    e = {"K": K, "N": N, "D": D, "draws": 256}
    for name, (mean, cov, _) in starts.items():
        r = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=256, moments=False)
        fin = r.info == 0
        elbo = r.log_ratios.mean(1)
        e[name] = {"elbo_median": float(np.median(elbo[fin])), "khat_median": float(np.median(r.khat[fin])),
                   "khat_ok_share": float(r.ok.mean()), "psis_failed": int((~fin).sum())}
    e["elbo_gain_over_lbfgs_median"] = e["pathfinder"]["elbo_median"] - e["lbfgs"]["elbo_median"]
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="few repetitions, K = 1024 only")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 3 if args.quick else max(args.reps, 10)
    res = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S, "prior_precision": LAM, "calls": [],
           "propose": [], "starts": []}
    for K in ((1024,) if args.quick else (1024, 8192)):
        for N, D in SHAPES:
            A, y = problems(K, N, D, 11)
            tgt = gsmvi_amd.BatchedLogisticTarget(A, y, LAM)
            for key, fn, extra in (("calls", call_entry, (reps,)), ("propose", propose_entry, (3 * reps,)), ("starts", starts_entry, ())):
                e = fn(tgt, K, N, D, *extra)
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
