"""Batched L-BFGS initialiser benchmark (lbfgs_init_batched, csrc/gsmvi_lbfgs_batched.hip) on BatchedLogisticTarget, x0 = 0,
default tolerances.

Writes one JSON object with
  calls[]   at K in {1024, 8192} x (N, D) in {(64, 10), (256, 16), (1024, 64)}: the wall time of one lbfgs_init_batched call
            (device-synchronised host clock, after a warm-up call, --reps >= 10 calls, median and range), its nlaunch and the
            largest nfev, ms per round, and the same call with check_every = 1
  looped    K = 1024, (N, D) = (64, 10): the single-problem way in the same run -- lbfgs_init (scipy's L-BFGS-B on the host)
            looped over the problems, each through a K = 1 BatchedLogisticTarget of its own slice.  32 problems are timed and
            the time is scaled to 1024 (seconds_scaled = seconds_32 * 32); ratio = seconds_scaled / the batched call's median
            (acceptance: >= 50)
  rounds[]  per shape at K = 8192 (and 1024): device-event times of the three launches of a round, each alone -- lp_g, lp and
            the step launch on a mid-run state (six rounds in with gtol = ftol = 0, nobody stopped; the state is restored
            outside the timed region before every launch) -- with the step's algorithmic bytes counted for a full history,
            8 K (30 D + 58) (x, g, Xt and the evaluation read, ten held pairs read, x, g, d, Xt and the new pair written, the
            scalars both ways; pairs_held_median is what the median problem of the timed state holds: with n pairs the bytes
            are 8 K ((10 + 2 n) D + 58)), as a fraction of 8 TB/s and of the library's streaming copy measured in the same
            run; step_share = step / (lp_g + lp + step)
Usage: python scripts/lbfgs_batched_bench.py [--out FILE] [--reps R] [--quick] [--kernel-only]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gsmvi_amd  # noqa: E402
from gsmvi_amd import _lib  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
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


def _wall(fn, reps):
    """seconds of fn() by a device-synchronised host clock, after a warm-up call"""
    out = fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return t, out


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


def copy_rate(reps):
    """bytes / s (read + write) of the library's streaming copy on 1 GiB"""
    dbg = C.CDLL(_lib.library_path(debug=True))
    dbg.gsmvi_debug_stream_copy_f64.restype = C.c_int
    dbg.gsmvi_debug_stream_copy_f64.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    big = torch.empty(2, 2 ** 27, dtype=torch.float64, device="cuda")
    big[0].fill_(1.0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def go():
        assert dbg.gsmvi_debug_stream_copy_f64(st, C.c_void_p(big[1].data_ptr()), C.c_void_p(big[0].data_ptr()), big[0].numel()) == 0

    ms = _each({"copy": (None, go)}, reps)["copy"]
    return 2 * 8 * big[0].numel() / (float(np.median(ms)) * 1e-3)


def call_entry(K, N, D, reps):
    A, y = problems(K, N, D, 11)
    tgt = gsmvi_amd.BatchedLogisticTarget(A, y, LAM)
    x0 = torch.zeros(K, D, dtype=torch.float64, device="cuda")
    e = {"K": K, "N": N, "D": D, "reps": reps}
    for name, ce in (("call_s", 8), ("call_check_every_1_s", 1)):
        t, (_, _, res) = _wall(lambda: gsmvi_amd.lbfgs_init_batched(x0, tgt.lp, tgt.lp_g, check_every=ce, as_torch=True), reps)
        e[name] = _stats(t)
        if ce == 8:
            e.update(nlaunch=res.nlaunch, nfev_max=int(res.nfev.max()), nfev_median=float(np.median(res.nfev)),
                     converged=int(res.success.sum()), ms_per_round=1e3 * e[name]["median"] / res.nlaunch)
    return e, tgt


def looped_entry(K, N, D, n_timed, batched_median):
    """lbfgs_init over the first n_timed problems, each through a K = 1 target of its own slice"""
    A, y = problems(K, N, D, 11)
    tgts = [gsmvi_amd.BatchedLogisticTarget(A[k:k + 1].contiguous(), y[k:k + 1].contiguous(), LAM) for k in range(n_timed)]
    eng = tgts[0].engine

    def one(t):
        lp = lambda x: t.lp(eng.asarray(x[None, None, :]))                     # noqa: E731
        lp_g = lambda x: t.lp_g(eng.asarray(x[None, None, :]))                 # noqa: E731
        return gsmvi_amd.lbfgs_init(np.zeros(D), lp, lp_g)

    def run():
        return [one(t)[2].nfev for t in tgts]
    t, nfev = _wall(run, 3)
    sec = float(np.median(t))
    return {"K": K, "N": N, "D": D, "problems_timed": n_timed, "seconds_timed": sec, "scaled_by": K / n_timed,
            "seconds_scaled": sec * K / n_timed, "nfev_max": int(max(nfev)), "nfev_median": float(np.median(nfev)),
            "batched_call_s": batched_median, "ratio": sec * K / n_timed / batched_median,
            "note": f"{n_timed} problems timed (median of 3 passes after a warm-up pass), scaled to {K}"}


def round_entry(K, N, D, reps, copy_bps):
    A, y = problems(K, N, D, 11)
    tgt = gsmvi_amd.BatchedLogisticTarget(A, y, LAM)
    eng = tgt.engine
    st = eng.lbfgs_state_batched(eng.zeros(K, D))
    Xt = st["Xt"].reshape(K, 1, D)
    G, opt = eng.empty(K, 1, D), dict(gtol=0.0, ftol=0.0)
    for r in range(6):
        tgt.lp_g(Xt, out=G)
        eng.lbfgs_step_batched(tgt.lp(Xt).reshape(K), G.reshape(K, D), st, start=r == 0, **opt)
    tgt.lp_g(Xt, out=G)
    fv = tgt.lp(Xt).reshape(K).clone()
    saved = {k: v.clone() for k, v in st.items()}
    assert int(saved["ist"][:, 0].abs().max().item()) == 0

    def restore():
        for k, v in saved.items():
            st[k].copy_(v)

    lpo = eng.empty(K, 1)
    t = _each({"lp_g": (None, lambda: tgt.lp_g(Xt, out=G)),
               "lp": (None, lambda: eng.logistic_batched(Xt, tgt.A, tgt.y, None, LAM, lp_out=lpo, want="lp")),
               "step": (restore, lambda: eng.lbfgs_step_batched(fv, G.reshape(K, D), st, **opt))}, reps)
    nbytes = 8 * K * (30 * D + 58)
    e = {"K": K, "N": N, "D": D, "reps": reps, "pairs_held_median": float(saved["ist"][:, 4].double().median().item()),
         "step_bytes": nbytes, "lp_g_ms": _stats(t["lp_g"]), "lp_ms": _stats(t["lp"]), "step_ms": _stats(t["step"])}
    e["step_bytes_per_s"] = nbytes / (e["step_ms"]["median"] * 1e-3)
    e["hbm_fraction"] = e["step_bytes_per_s"] / HBM_BYTES_PER_S
    e["copy_fraction"] = e["step_bytes_per_s"] / copy_bps
    e["step_share"] = e["step_ms"]["median"] / (e["step_ms"]["median"] + e["lp_ms"]["median"] + e["lp_g_ms"]["median"])
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="few repetitions, K = 1024 only")
    ap.add_argument("--kernel-only", action="store_true", help="only the rounds at K = 8192 and the copy (the profiler run)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 3 if args.quick else max(args.reps, 10)
    res = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S, "prior_precision": LAM, "calls": [],
           "rounds": []}
    res["copy_bytes_per_s"] = copy_rate(max(reps, 10))
    print(json.dumps({"copy_bytes_per_s": res["copy_bytes_per_s"]}), flush=True)
    Ks = (8192,) if args.kernel_only else (1024,) if args.quick else (1024, 8192)
    if not args.kernel_only:
        for K in Ks:
            for N, D in SHAPES:
                e, _ = call_entry(K, N, D, reps)
                res["calls"].append(e)
                print(json.dumps(e), flush=True)
        head = res["calls"][0]
        res["looped"] = looped_entry(1024, 64, 10, 8 if args.quick else 32, head["call_s"]["median"])
        print(json.dumps(res["looped"]), flush=True)
    for K in Ks:
        for N, D in SHAPES:
            e = round_entry(K, N, D, max(reps, 30) if not args.quick else 5, res["copy_bytes_per_s"])
            res["rounds"].append(e)
            print(json.dumps(e), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
