"""Shared-design Laplace initialiser benchmark (gsmvi_glm_shared_hessian_batched_f64, gsmvi_laplace_shared_step_batched_f64 in
csrc/gsmvi_laplace_shared_batched.hip; ``laplace_init_shared_batched``) against the existing way to get the same results: the
per-problem entry points (``glm_hessian_batched``, ``laplace_step_batched``, ``laplace_init_batched``) on the K-fold replicated
design, alternated call by call in the same process.  The replicated form cannot carry observation weights, so the comparison
runs without them.

Writes one JSON object with
  cases[]  K in {1024, 8192} x (N, D) in {(64, 10), (256, 16), (1024, 64)} x {logistic, poisson}; for each of ``hessian`` (one
           launch, H alone), ``step`` (the first launch of a run: f, g, H, the factorisation and the direction of every problem; the
           start point is restored outside the timed span) and ``init`` (``laplace_init_*`` end to end, host loop included):
           shared_ms and replicated_ms, the median, minimum and maximum of --reps (>= 10, default 20) calls after a warm-up, one
           pair of device events per call, the two forms alternated and their order swapped every repetition; ratio =
           replicated median / shared median; noise_ms = the spread (max - min) of the replicated calls; slower_beyond_noise =
           the shared median exceeds the replicated median by more than that spread.
           design_bytes: the device memory the design takes in each form; init_peak_bytes: the rise of
           torch.cuda.max_memory_allocated over one end-to-end call of each; max_rel_diff: H and the means against the
           replicated form's; rounds: launches of the end-to-end call
  library_sha256: of the library that ran
Every case runs in a child process under a time limit (--case-limit seconds), and in it every timed call under its own
(--call-limit seconds: the event is polled, never waited for without a deadline); after a case that fails or runs out of time
no further case is started.  Nothing is gated on the figures.
Usage: python scripts/shared_laplace_bench.py [--out FILE] [--reps R] [--quick]
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
FAMILIES = ("logistic", "poisson")
LAM = 0.5


def timed(torch, fns, reps, call_limit):
    """per-call device-event times (ms) of the (prepare, call) pairs; ``prepare`` runs outside the timed span.  The two forms of
    one quantity ("<name>_shared", "<name>_replicated") are timed as a group, alternated call by call, and the order within the
    pair is swapped every repetition: a span between two events also holds the time the idle device takes to pick the launch up,
    which depends on what ran before it, so each form runs first in half of the repetitions.  A call that is not done after
    call_limit seconds ends the process (exit status 3) without waiting for it"""
    def one(prep, f):
        if prep is not None:
            prep()
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
    out = {k: [] for k in fns}
    for name in dict.fromkeys(k.rsplit("_", 1)[0] for k in fns):
        both = [name + "_shared", name + "_replicated"]
        for r in range(-3, reps):                                       # three warm-up rounds, not recorded
            for k in both if r % 2 == 0 else both[::-1]:
                ms = one(*fns[k])
                if r >= 0:
                    out[k].append(ms)
    return out


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def pair(t, name):
    s, r = stats(t[name + "_shared"]), stats(t[name + "_replicated"])
    noise = r["max"] - r["min"]
    return {"shared_ms": s, "replicated_ms": r, "ratio": r["median"] / s["median"], "noise_ms": noise,
            "slower_beyond_noise": bool(s["median"] > r["median"] + noise)}


def run_case(K, N, D, family, reps, call_limit):
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
    x = 0.3 * rn(K, D)
    tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, family, LAM)
    rep = gsmvi_amd.BatchedGLMTarget(A[None].expand(K, N, D).contiguous(), y, family, LAM)
    Hs, Hr = eng.empty(K, D, D), eng.empty(K, D, D)
    opt = dict(maxiter=100, maxfun=200, gtol=1e-8)
    x0 = eng.zeros(K, D)
    sts, str_ = eng.laplace_state_batched(x0), eng.laplace_state_batched(x0)
    fns = {
        "hessian_shared": (None, lambda: eng.glm_shared_hessian_batched(x, tgt.A, tgt.y, family, prior_prec=LAM, want="h", out=Hs)),
        "hessian_replicated": (None, lambda: eng.glm_hessian_batched(x, rep.A, rep.y, family, prior_prec=LAM, want="h", out=Hr)),
        "step_shared": (lambda: sts["Xt"].copy_(x0),
                        lambda: eng.laplace_shared_step_batched(sts, tgt.A, tgt.y, family, prior_prec=LAM, start=True, **opt)),
        "step_replicated": (lambda: str_["Xt"].copy_(x0),
                            lambda: eng.laplace_step_batched(str_, rep.A, rep.y, family, prior_prec=LAM, start=True, **opt)),
        "init_shared": (None, lambda: gsmvi_amd.laplace_init_shared_batched(tgt, as_torch=True)),
        "init_replicated": (None, lambda: gsmvi_amd.laplace_init_batched(rep, as_torch=True)),
    }
    fns["hessian_shared"][1]()
    fns["hessian_replicated"][1]()
    peaks, means, rounds = {}, {}, {}
    for name, call in (("shared", fns["init_shared"][1]), ("replicated", fns["init_replicated"][1])):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m, _, res = call()
        torch.cuda.synchronize()
        peaks[name] = int(torch.cuda.max_memory_allocated() - base)
        means[name], rounds[name] = m.clone(), int(res.nlaunch)
        del m, _
    diffs = {"H": float((Hs - Hr).abs().max() / Hr.abs().max()),
             "mean": float((means["shared"] - means["replicated"]).abs().max() / means["replicated"].abs().max())}
    torch.cuda.synchronize()
    t = timed(torch, fns, reps, call_limit)
    e = {"family": family, "K": K, "N": N, "D": D, "reps": reps, "design_bytes": {"shared": N * D * 8, "replicated": K * N * D * 8},
         "init_peak_bytes": peaks, "rounds": rounds, "max_rel_diff": diffs}
    for name in ("hessian", "step", "init"):
        e[name] = pair(t, name)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched", "shared_laplace_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="K = 1024 only")
    ap.add_argument("--case-limit", type=float, default=180.0, help="seconds a case (a child process) may take")
    ap.add_argument("--call-limit", type=float, default=30.0, help="seconds one timed call may take")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)        # K,N,D,family: run it here and print its entry
    args = ap.parse_args()
    reps = max(args.reps, 10)
    if args.case:
        K, N, D, family = args.case.split(",")
        print(json.dumps(run_case(int(K), int(N), int(D), family, reps, args.call_limit)), flush=True)
        return
    from gsmvi_amd import _lib
    res = {"library_sha256": hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest(), "prior_precision": LAM,
           "reps": reps, "cases": [], "stopped": None}
    for K in KS[:1] if args.quick else KS:
        for N, D in SHAPES:
            for family in FAMILIES:
                case = f"{K},{N},{D},{family}"
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
