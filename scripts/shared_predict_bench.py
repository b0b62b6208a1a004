"""Shared-design GLM predictive benchmark (gsmvi_glm_shared_predict_batched_f64 in csrc/gsmvi_glm_shared_predict_batched.hip;
``predict_shared_batched``) against the existing way to get the same numbers: the per-problem launch (``glm_predict_batched``) on
the K-fold replicated rows, alternated call by call in the same process.  The replicated form cannot carry row weights, so the
comparison runs without them; the weighted launch is timed on its own.

Writes one JSON object with
  cases[]  K in {1024, 8192} x (M, D) in {(64, 10), (256, 16), (1024, 64)} x {logistic, poisson, gaussian}; for each of ``with_y``
           (eta_mean, eta_var, pmean, lpd, elpd) and ``without_y`` (the first three): shared_ms and replicated_ms, the median,
           minimum and maximum of --reps (>= 10, default 20) calls after a warm-up, one pair of device events per call, the two
           forms alternated and their order swapped every repetition; ratio = replicated median / shared median; noise_ms = the
           spread (max - min) of the replicated calls; slower_beyond_noise = the shared median exceeds the replicated median by
           more than that spread.
           weighted_ms: the shared launch with y and weights U(0, 2), a quarter of them zero (median, minimum, maximum).
           design_bytes: the device memory the rows take in each form; same_bits: every output of the two forms is equal bit for
           bit (weights None)
  library_sha256: of the library that ran
Every (K, M, D) runs in a child process under a time limit (--case-limit seconds), and in it every timed call under its own
(--call-limit seconds: the event is polled, never waited for without a deadline); after a child that fails or runs out of time
no further one is started.  Nothing is gated on the figures.
Usage: python scripts/shared_predict_bench.py [--out FILE] [--reps R] [--quick]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64, 10), (256, 16), (1024, 64)]
KS = (1024, 8192)
FAMILIES = ("logistic", "poisson", "gaussian")
NODES = 32


def one(torch, f, call_limit):
    """the device-event time (ms) of one call; a call that is not done after call_limit seconds ends the process (exit status
    3) without waiting for it"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    deadline = time.monotonic() + call_limit
    while not b.query():
        if time.monotonic() > deadline:
            print(json.dumps({"error": "a call ran past its time limit"}), flush=True)
            os._exit(3)
    return a.elapsed_time(b)


def timed_pair(torch, shared, replicated, reps, call_limit):
    """the two forms alternated call by call, the order within the pair swapped every repetition: a span between two events also
    holds the time the idle device takes to pick the launch up, which depends on what ran before it, so each form runs first in
    half of the repetitions.  Three warm-up rounds are not recorded."""
    out = {"shared": [], "replicated": []}
    fns = {"shared": shared, "replicated": replicated}
    for r in range(-3, reps):
        for k in ("shared", "replicated") if r % 2 == 0 else ("replicated", "shared"):
            ms = one(torch, fns[k], call_limit)
            if r >= 0:
                out[k].append(ms)
    return out


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def pair(t):
    s, r = stats(t["shared"]), stats(t["replicated"])
    noise = r["max"] - r["min"]
    return {"shared_ms": s, "replicated_ms": r, "ratio": r["median"] / s["median"], "noise_ms": noise,
            "slower_beyond_noise": bool(s["median"] > r["median"] + noise)}


def run_shape(K, M, D, reps, call_limit):
    import torch
    import gsmvi_amd
    torch.cuda.set_device(0)
    eng = gsmvi_amd.get_engine()
    g = torch.Generator(device="cuda").manual_seed(11)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)      # noqa: E731
    A = rn(M, D) / np.sqrt(D)
    rep = A[None].expand(K, M, D).contiguous()
    mean = 0.5 * rn(K, D)
    G = rn(K, D, D)
    cov = G @ G.transpose(1, 2) / (4.0 * D)
    vmax = torch.einsum("ni,kij,nj->kn", A, cov, A).amax(1)
    cov = (cov * torch.clamp(0.9 / vmax, max=1.0)[:, None, None]).contiguous()   # a^T Sigma a <= 0.9: the band of the tests
    eta = (mean + 0.5 * rn(K, D)) @ A.T
    u = torch.rand(K, M, dtype=torch.float64, device="cuda", generator=g)
    w = 2.0 * torch.rand(K, M, dtype=torch.float64, device="cuda", generator=g)
    w[torch.rand(K, M, dtype=torch.float64, device="cuda", generator=g) < 0.25] = 0.0
    out = []
    for family in FAMILIES:
        if family == "logistic":
            y = (u < torch.sigmoid(eta)).double()
        elif family == "poisson":
            y = torch.poisson(torch.exp(eta.clamp(max=10.0)), generator=g)
        else:
            y = eta + rn(K, M)
        e = {"family": family, "K": K, "M": M, "D": D, "reps": reps, "nodes": NODES,
             "design_bytes": {"shared": M * D * 8, "replicated": K * M * D * 8}}
        same = True
        for name, yy in (("with_y", y), ("without_y", None)):
            shared = lambda: eng.glm_shared_predict_batched(mean, cov, A, family, y=yy, nodes=NODES)       # noqa: E731
            replicated = lambda: eng.glm_predict_batched(mean, cov, rep, family, y=yy, nodes=NODES)          # noqa: E731
            a, b = shared(), replicated()
            torch.cuda.synchronize()
            same = same and all(torch.equal(x, z) for x, z in zip(a, b) if x is not None)
            del a, b
            e[name] = pair(timed_pair(torch, shared, replicated, reps, call_limit))
        weighted = lambda: eng.glm_shared_predict_batched(mean, cov, A, family, y=y, weights=w, nodes=NODES)  # noqa: E731
        for _ in range(3):
            weighted()
        e["weighted_ms"] = stats([one(torch, weighted, call_limit) for _ in range(reps)])
        e["same_bits"] = bool(same)
        out.append(e)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched", "shared_predict_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="K = 1024 only")
    ap.add_argument("--case-limit", type=float, default=180.0, help="seconds a (K, M, D) (a child process) may take")
    ap.add_argument("--call-limit", type=float, default=30.0, help="seconds one timed call may take")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)        # K,M,D: run it here and print its entries
    args = ap.parse_args()
    reps = max(args.reps, 10)
    if args.case:
        K, M, D = (int(v) for v in args.case.split(","))
        print(json.dumps(run_shape(K, M, D, reps, args.call_limit)), flush=True)
        return
    from gsmvi_amd import _lib
    res = {"library_sha256": hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest(), "reps": reps, "cases": [],
           "stopped": None}
    for K in KS[:1] if args.quick else KS:
        for M, D in SHAPES:
            case = f"{K},{M},{D}"
            cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(reps), "--call-limit",
                   str(args.call_limit)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.case_limit)
                rc, tail = r.returncode, (r.stdout.strip().splitlines() or [""])[-1]
            except subprocess.TimeoutExpired:
                rc, tail = 124, ""
            if rc != 0:                                                   # nothing more is started on the device after this
                res["stopped"] = {"case": case, "status": rc, "output": tail[-500:]}
                break
            for e in json.loads(tail):
                res["cases"].append(e)
                print(json.dumps(e), flush=True)
        if res["stopped"]:
            break
    if res["cases"]:
        import torch
        res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"stopped": res["stopped"], "cases": len(res["cases"])}), flush=True)
    sys.exit(1 if res["stopped"] else 0)


if __name__ == "__main__":
    main()
