"""Shared-design GLM target benchmark (SharedDesignGLMTarget, gsmvi_glm_shared_batched_f64 in csrc/gsmvi_glm_shared_batched.hip):
the score call of K problems on ONE design matrix against the two ways to get the same score without it, in the same process --
gsmvi_glm_batched_f64 on the K-fold replicated design, and torch ops (X @ A.T, the link, @ A).

Writes one JSON object with
  cases[]  K in {1024, 8192} x (N, D, nc) in {(64, 10, 2), (256, 16, 8), (1024, 64, 8)} x {logistic, poisson}: shared_ms (the new
           launch, score alone), replicated_ms (glm_batched on the copy), torch_ms (where the (K nc, N) intermediate fits), each
           the median, minimum and maximum of --reps (>= 10) calls after a warm-up, alternated call by call, one pair of device
           events per call; ratio_replicated / ratio_torch = that median / the shared median; extra_bytes: the device memory
           each alternative holds beyond y and X (shared: the one A; replicated: K copies; torch: A and the two (K nc, N)
           intermediates); max_rel_diff: the outputs against the new launch's
  library_sha256: of the library that ran
Every case runs in a child process under a time limit (--case-limit seconds), and in it every timed call under its own
(--call-limit seconds: the event is polled, never waited for without a deadline); after a case that fails or runs out of time
no further case is started.  Nothing is gated on the figures.
Usage: python scripts/shared_glm_bench.py [--out FILE] [--reps R] [--quick]
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

SHAPES = [(64, 10, 2), (256, 16, 8), (1024, 64, 8)]
KS = (1024, 8192)
FAMILIES = ("logistic", "poisson")
LAM = 0.5
TORCH_MAX_BYTES = 8 << 30          # the torch alternative is skipped when its two (K nc, N) intermediates exceed this


def torch_score(torch, family, A, y, lam, nc):
    """the same score as torch ops on the stacked rows, each link in the form a torch user would write to keep it finite"""
    K, N = y.shape
    At = A.T.contiguous()
    yb = y[:, None, :]

    def lp_g(x):
        eta = (x.reshape(K * nc, -1) @ At).reshape(K, nc, N)
        if family == "logistic":
            e = torch.exp(-eta.abs())
            r = yb - torch.where(eta >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        else:
            r = yb - torch.exp(eta)
        return (r.reshape(K * nc, N) @ A).reshape(K, nc, -1) - lam * x
    return lp_g


def timed(torch, fns, reps, call_limit):
    """per-call device-event times (ms) of the callables, alternated; a call that is not done after call_limit seconds ends
    the process (exit status 3) without waiting for it"""
    def one(f):
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
    for _ in range(3):
        for f in fns.values():
            one(f)
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            out[k].append(one(f))
    return out


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def run_case(K, N, D, nc, family, reps, call_limit):
    import torch
    import gsmvi_amd
    torch.cuda.set_device(0)
    eng = gsmvi_amd.get_engine()
    g = torch.Generator(device="cuda").manual_seed(11)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)      # noqa: E731
    A = rn(N, D) / np.sqrt(D)
    eta = rn(K, D) @ A.T
    u = torch.rand(K, N, dtype=torch.float64, device="cuda", generator=g)
    y = (u < torch.sigmoid(eta)).double() if family == "logistic" else torch.poisson(torch.exp(eta), generator=g)
    x = rn(K, nc, D)
    G, Gr = eng.empty(K, nc, D), eng.empty(K, nc, D)
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, family, LAM)
    Arep = A[None].expand(K, N, D).contiguous()
    fns = {"shared": lambda: tgt.lp_g(x, out=G),
           "replicated": lambda: eng.glm_batched(x, Arep, tgt.y, family, prior_prec=LAM, out=Gr, want="g")}
    ref = tgt.lp_g(x).clone()
    diffs = {"replicated": float((fns["replicated"]() - ref).abs().max() / ref.abs().max())}
    extra = {"shared": N * D * 8, "replicated": K * N * D * 8, "torch": N * D * 8 + 2 * K * nc * N * 8}
    if extra["torch"] <= TORCH_MAX_BYTES:
        ts = torch_score(torch, family, A, y, LAM, nc)
        fns["torch"] = lambda: ts(x)
        diffs["torch"] = float((ts(x) - ref).abs().max() / ref.abs().max())
    torch.cuda.synchronize()
    t = timed(torch, fns, reps, call_limit)
    e = {"family": family, "K": K, "N": N, "D": D, "nc": nc, "reps": reps, "extra_bytes": extra, "max_rel_diff": diffs}
    for k in fns:
        e[k + "_ms"] = stats(t[k])
        if k != "shared":
            e["ratio_" + k] = e[k + "_ms"]["median"] / e["shared_ms"]["median"]
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched", "shared_glm_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="K = 1024 only")
    ap.add_argument("--case-limit", type=float, default=120.0, help="seconds a case (a child process) may take")
    ap.add_argument("--call-limit", type=float, default=20.0, help="seconds one timed call may take")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)        # K,N,D,nc,family: run it here and print its entry
    args = ap.parse_args()
    reps = max(args.reps, 10)
    if args.case:
        K, N, D, nc, family = args.case.split(",")
        print(json.dumps(run_case(int(K), int(N), int(D), int(nc), family, reps, args.call_limit)), flush=True)
        return
    from gsmvi_amd import _lib
    res = {"library_sha256": hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest(), "prior_precision": LAM,
           "reps": reps, "cases": [], "stopped": None}
    for K in KS[:1] if args.quick else KS:
        for N, D, nc in SHAPES:
            for family in FAMILIES:
                case = f"{K},{N},{D},{nc},{family}"
                cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(reps), "--call-limit",
                       str(args.call_limit)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.case_limit)
                    rc, tail = r.returncode, (r.stdout.strip().splitlines() or [""])[-1]
                except subprocess.TimeoutExpired:
                    rc, tail = 124, ""
                if rc != 0:                                               # nothing more is started on the device after this
                    res["stopped"] = {"case": case, "status": rc, "output": tail[-500:]}
                    break
                e = json.loads(tail)
                res["cases"].append(e)
                print(json.dumps(e), flush=True)
            if res["stopped"]:
                break
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
