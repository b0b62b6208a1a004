"""Batched GLM posterior predictive benchmark (gsmvi_glm_predict_batched_f64, csrc/gsmvi_glm_predict_batched.hip).

Writes one JSON object with, at K = 8192 x (M, D) in {(64, 10), (256, 16), (1024, 64)} x four families x with / without y, all in
one process:
  predict[]  the launch (device events around one call of the engine method, alternated with the torch version, median and
             range) against the same quantities as torch ops in the same run: ``bmm`` for m, an ``einsum`` for the quadratic
             forms, a broadcast over the Q = 32 nodes, the link, a ``logsumexp`` (and ``lgamma`` / ``erfc`` where the family
             needs them); the largest difference between the two per output; the rate on the bytes the launch must move (A_new,
             cov, mean, y and the outputs) as a fraction of 8 TB/s and of the rate of the library's streaming copy (gsmvi_debug_stream_copy_f64 of the debug
             build) measured in this run.  The time is device-event time around one launch (launch gap included), not profiler
             kernel time
Usage: python scripts/glm_predict_bench.py [--out FILE] [--reps R] [--quick]
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

HBM_BYTES_PER_S = 8.0e12
SHAPES = [(64, 10), (256, 16), (1024, 64)]
FAMILIES = ("logistic", "poisson", "probit", "gaussian")
Q = 32


def problems(family, K, M, D, seed):
    """K synthetic held-out sets and fitted Gaussians on the device: A ~ N(0, 1) / sqrt(D), mean ~ 0.5 N(0, 1), cov = G G^T / (4 D)
    (a^T cov a about 0.25), y drawn from the family at A mean"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)      # noqa: E731
    A = rn(K, M, D) / np.sqrt(D)
    mean = 0.5 * rn(K, D)
    G = rn(K, D, D)
    cov = torch.bmm(G, G.mT) / (4.0 * D)
    eta = torch.bmm(A, mean[:, :, None])[:, :, 0]
    u = torch.rand(K, M, dtype=torch.float64, device="cuda", generator=g)
    if family == "logistic":
        y = (u < torch.sigmoid(eta)).double()
    elif family == "probit":
        y = (u < torch.special.ndtr(eta)).double()
    elif family == "poisson":
        y = torch.poisson(torch.exp(eta), generator=g)
    else:
        y = eta + rn(K, M)
    return A, y, mean, cov


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


def torch_predict(family, A, y, mean, cov, t, lw, tau=1.0):
    """the same quantities as torch ops: (eta_mean, eta_var, pmean, lpd, elpd)"""
    m = torch.bmm(A, mean[:, :, None])[:, :, 0]
    v = torch.einsum("kmi,kij,kmj->km", A, cov, A)
    vp = v.clamp_min(0.0)
    need_nodes = family == "logistic" or (y is not None and family != "gaussian")
    eta = m[:, :, None] + torch.sqrt(2.0 * vp)[:, :, None] * t if need_nodes else None
    if family == "gaussian":
        pm = m
    elif family == "probit":
        pm = 0.5 * torch.erfc(-(m / torch.sqrt(1.0 + vp)) * math.sqrt(0.5))
    elif family == "poisson":
        pm = torch.exp(m + 0.5 * vp)
    else:
        pm = (torch.exp(lw) * torch.sigmoid(eta)).sum(-1) / math.sqrt(math.pi)
    if y is None:
        return m, v, pm, None, None
    if family == "gaussian":
        var = vp + 1.0 / tau
        lpd = -0.5 * torch.log(2.0 * math.pi * var) - (y - m) ** 2 / (2.0 * var)
    else:
        yy = y[:, :, None]
        if family == "logistic":
            tt = yy * eta - torch.nn.functional.softplus(eta)
        elif family == "poisson":
            tt = yy * eta - torch.exp(eta)
        else:
            tt = yy * torch.special.log_ndtr(eta) + (1.0 - yy) * torch.special.log_ndtr(-eta)
        lpd = torch.logsumexp(lw + tt, -1) - 0.5 * math.log(math.pi)
        if family == "poisson":
            lpd = lpd - torch.lgamma(y + 1.0)
    return m, v, pm, lpd, lpd.sum(1)


def copy_rate(reps):
    """bytes / s (read + write) of the library's streaming copy on 1 GiB (gsmvi_debug_stream_copy_f64 of the debug build)"""
    import ctypes as C
    dbg = C.CDLL(gsmvi_amd._lib.library_path(debug=True))
    dbg.gsmvi_debug_stream_copy_f64.restype = C.c_int
    dbg.gsmvi_debug_stream_copy_f64.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    big = torch.empty(2, 2 ** 27, dtype=torch.float64, device="cuda")
    big[0].fill_(1.0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def go():
        assert dbg.gsmvi_debug_stream_copy_f64(st, C.c_void_p(big[1].data_ptr()), C.c_void_p(big[0].data_ptr()), big[0].numel()) == 0

    ms = np.median(_each({"copy": go}, reps)["copy"])
    return 2 * 8 * big[0].numel() / (ms * 1e-3)


def entry(family, K, M, D, with_y, reps, copy_bps):
    eng = gsmvi_amd.get_engine()
    A, y, mean, cov = problems(family, K, M, D, 11)
    t, lw = (eng.asarray(x) for x in eng.gauss_hermite(Q))
    yy = y if with_y else None
    hip = lambda: eng.glm_predict_batched(mean, cov, A, family, y=yy, nodes=Q)          # noqa: E731
    ref = lambda: torch_predict(family, A, yy, mean, cov, t, lw)                        # noqa: E731
    diffs = {}
    for name, a, b in zip(("eta_mean", "eta_var", "mean", "lpd", "elpd"), hip(), ref()):
        if a is not None:
            diffs[name] = float(((a - b).abs() / b.abs().clamp_min(1.0)).max().item())
    tm = _each({"hip": hip, "torch": ref}, reps)
    e = {"family": family, "K": K, "M": M, "D": D, "Q": Q, "with_y": with_y, "reps": reps, "hip_ms": _stats(tm["hip"]),
         "torch_ms": _stats(tm["torch"]), "max_rel_diff": diffs}
    sec = e["hip_ms"]["median"] * 1e-3
    e["torch_over_hip"] = e["torch_ms"]["median"] / e["hip_ms"]["median"]
    nbytes = 8.0 * K * (M * D + D * D + D + M * (5 if with_y else 3))     # A_new, cov, mean; y and the outputs
    e["bytes_per_s"] = nbytes / sec
    e["hbm_fraction"] = e["bytes_per_s"] / HBM_BYTES_PER_S
    e["copy_fraction"] = e["bytes_per_s"] / copy_bps
    e["time_source"] = "device events around one launch (not profiler kernel time)"
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="few repetitions, K = 1024")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 3 if args.quick else max(args.reps, 10)
    K = 1024 if args.quick else 8192
    copy_bps = copy_rate(reps)
    res = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S, "copy_bytes_per_s": copy_bps,
           "predict": []}
    for M, D in SHAPES:
        for family in FAMILIES:
            for with_y in (True, False):
                e = entry(family, K, M, D, with_y, reps, copy_bps)
                res["predict"].append(e)
                print(json.dumps(e), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
