"""A/B of the five batched Laplace kernels between libraries ("The Laplace stage block"): the Hessian
launch, the Hessian launch with the inverse and one step launch (start = 1, x0 = 0) of the GLM (logistic), softmax, shared-design
(logistic), negative binomial and ordinal entries at K in {1024, 8192} and the three (N, D) points of each family's own
``*_laplace_bench.py``: 90 cases (``--families`` takes a subset).

One child process per load of a library (``GSMVI_HIP_LIB_VARIANT``; "" is the library the package loads), the libraries
alternated ``--rounds`` times with the order rotated; per case the median of 10 calls by device events after 10 warm-up calls.
The measure's own noise comes from the base library loaded a second time from a copy under another file name (``--null``) and
timed as if it were the candidate: the margin of a case is the larger of the spread of the base's medians and the difference
between the means of the base and of its copy, and a case passes if the mean of the candidate's medians is not above the base's
mean by more than that margin.  Every child runs under a time limit; after one that fails nothing more is started.

  python scripts/laplace_sweep_ab.py --base parent --null parentcopy --cand tree --out profiles/batched/laplace_sweep_ab_parent.txt
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1024, 8192)
GLM_SHAPES = ((64, 10), (256, 16), (1024, 64))              # (N, D): laplace_batched_bench.py, shared_laplace_bench.py
NEGBIN_SHAPES = ((64, 10), (256, 16), (1024, 64))           # (N, D = P + 1): negbin_laplace_bench.py
SOFTMAX_SHAPES = ((64, 3, 5), (256, 5, 4), (1024, 9, 8))    # (N, C, P): softmax_laplace_bench.py
ORDINAL_SHAPES = ((64, 6, 5), (256, 10, 7), (1024, 48, 17))  # (N, P, C): ordinal_laplace_bench.py
WARM, REPS = 10, 10


def family_calls(torch, eng, family, K, shape):
    """(D, hessian(x, want, outs), step(state)) of one family at one shape, on seeded inputs"""
    g = torch.Generator(device="cuda").manual_seed(11)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)      # noqa: E731
    ru = lambda *s: torch.rand(*s, dtype=torch.float64, device="cuda", generator=g)       # noqa: E731
    opt = dict(maxiter=100, maxfun=200, gtol=1e-8)
    if family in ("glm", "shared"):
        N, D = shape
        A = (rn(K, N, D) if family == "glm" else rn(N, D)) / np.sqrt(D)
        eta = torch.bmm(A, rn(K, D, 1))[:, :, 0] if family == "glm" else rn(K, D) @ A.T
        y = (ru(K, N) < torch.sigmoid(eta)).double()
        if family == "glm":
            return (D, lambda x, **kw: eng.glm_hessian_batched(x, A, y, "logistic", prior_prec=1.0, **kw),
                    lambda st: eng.laplace_step_batched(st, A, y, "logistic", prior_prec=1.0, start=True, **opt))
        return (D, lambda x, **kw: eng.glm_shared_hessian_batched(x, A, y, "logistic", prior_prec=1.0, **kw),
                lambda st: eng.laplace_shared_step_batched(st, A, y, "logistic", prior_prec=1.0, start=True, **opt))
    if family == "softmax":
        N, C, P = shape
        A = rn(K, N, P) / np.sqrt(P)
        y = torch.randint(0, C, (K, N), device="cuda", generator=g).to(torch.int32)
        return ((C - 1) * P, lambda x, **kw: eng.softmax_hessian_batched(x, A, y, C, prior_prec=1.0, **kw),
                lambda st: eng.softmax_laplace_step_batched(st, A, y, C, prior_prec=1.0, start=True, **opt))
    if family == "negbin":
        N, D = shape
        P = D - 1
        A = rn(K, N, P) / np.sqrt(P)
        o = 1.0 + 0.3 * rn(K, N)
        y = torch.poisson(torch.exp(torch.bmm(A, 0.7 * rn(K, P, 1))[:, :, 0] + o), generator=g)
        return (D, lambda x, **kw: eng.negbin_hessian_batched(x, A, y, offset=o, **kw),
                lambda st: eng.negbin_laplace_step_batched(st, A, y, offset=o, start=True, **opt))
    N, P, C = shape
    A = rn(K, N, P) / np.sqrt(P)
    o = 0.3 * rn(K, N)
    eta = torch.bmm(A, rn(K, P, 1))[:, :, 0] + o
    cuts = torch.sort(1.5 * rn(K, C - 1), dim=1).values
    y = (ru(K, N)[:, :, None] > torch.sigmoid(cuts[:, None, :] - eta[:, :, None])).sum(2).to(torch.int32)
    return (P + C - 1, lambda x, **kw: eng.ordinal_hessian_batched(x, A, y, C, offset=o, **kw),
            lambda st: eng.ordinal_laplace_step_batched(st, A, y, C, offset=o, start=True, **opt))


def cases(families):
    for family, shapes in (("glm", GLM_SHAPES), ("softmax", SOFTMAX_SHAPES), ("shared", GLM_SHAPES), ("negbin", NEGBIN_SHAPES),
                           ("ordinal", ORDINAL_SHAPES)):
        if family not in families:
            continue
        for K in KS:
            for shape in shapes:
                yield family, K, shape


def worker(families):
    """every case with the library this process loads: one JSON line per case, the medians in ms"""
    import torch
    import gsmvi_amd
    torch.cuda.set_device(0)
    eng = gsmvi_amd.get_engine()
    w = torch.randn(4096, 4096, device="cuda")
    for _ in range(50):                                     # the device clocked up first
        w = torch.tanh(w @ w * 1e-3)
    torch.cuda.synchronize()

    def median(prep, f):
        ts = []
        for r in range(-WARM, REPS):
            if prep is not None:
                prep()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            if r >= 0:
                ts.append(a.elapsed_time(b))
        return float(np.median(ts))

    for family, K, shape in cases(families):
        D, hess, step = family_calls(torch, eng, family, K, shape)
        x = 0.3 * torch.randn(K, D, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
        H, cov, info = eng.empty(K, D, D), eng.empty(K, D, D), eng.batched_ints(K)
        x0 = eng.zeros(K, D)
        st = eng.laplace_state_batched(x0)
        e = {"family": family, "K": K, "shape": list(shape),
             "hessian": median(None, lambda: hess(x, want="h", out=H)),
             "hessian_inverse": median(None, lambda: hess(x, want="both", out=H, cov_out=cov, info_out=info)),
             "step": median(lambda: st["Xt"].copy_(x0), lambda: step(st))}
        print(json.dumps(e), flush=True)
        del hess, step, H, cov, st
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--base", default="parent", help="variant name of the base library")
    ap.add_argument("--null", default="parentcopy", help="variant name of a copy of the base library under another file name")
    ap.add_argument("--cand", default="", help="variant name of the candidate ('': the library the package loads)")
    ap.add_argument("--families", default="glm,softmax,shared,negbin,ordinal", help="the families to time, comma-separated")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=170.0, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched", "laplace_sweep_ab_parent.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.families.split(","))
    libs = {"base": args.base, "null": args.null, "cand": args.cand}
    order = ["base", "cand", "null"]
    runs = {k: [] for k in libs}                            # role -> list (per round) of {case key: entry}
    lines = []
    for r in range(args.rounds):
        for role in order[r % 3:] + order[:r % 3]:
            env = dict(os.environ, GSMVI_HIP_LIB_VARIANT=libs[role])
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--families", args.families], env=env, capture_output=True, text=True,
                                   timeout=args.limit)
                rc = p.returncode
            except subprocess.TimeoutExpired:
                p, rc = None, 124
            if rc != 0:                                     # nothing more is started on the device after this
                print(f"round {r} {role} ({libs[role]!r}): exit status {rc}\n{(p.stderr if p else '')[-2000:]}", flush=True)
                sys.exit(1)
            got = {}
            for ln in p.stdout.splitlines():
                if ln.startswith("{"):
                    e = json.loads(ln)
                    got[(e["family"], e["K"], tuple(e["shape"]))] = e
                    lines.append(f"round {r} {role:4s} {libs[role] or '(default)':10s} {ln}")
            runs[role].append(got)
            print(f"round {r} {role}: {len(got)} cases", flush=True)
    report = [f"base {args.base!r}, its copy {args.null!r}, candidate {args.cand or '(the default library)'!r}; {args.rounds} rounds, "
              f"median of {REPS} calls after {WARM}; times in ms", ""]
    npass = ntot = 0
    for key in runs["base"][0]:
        for launch in ("hessian", "hessian_inverse", "step"):
            b, n, c = ([run[key][launch] for run in runs[role]] for role in ("base", "null", "cand"))
            spread, null = max(b) - min(b), abs(np.mean(n) - np.mean(b))
            margin = max(spread, null)
            ok = np.mean(c) <= np.mean(b) + margin
            npass, ntot = npass + ok, ntot + 1
            fmt = lambda v: " ".join(f"{t:.5f}" for t in v)  # noqa: E731
            report.append(f"{key[0]:8s} K={key[1]:5d} {str(key[2]):15s} {launch:16s} base {fmt(b)} | copy {fmt(n)} | cand {fmt(c)} | "
                          f"spread {spread:.5f} null {null:.5f} margin {margin:.5f} | cand - base {np.mean(c) - np.mean(b):+.5f} "
                          f"({100 * (np.mean(c) / np.mean(b) - 1):+.2f} %) {'pass' if ok else 'MISS'}")
    report.append("")
    report.append(f"{npass} of {ntot} cases pass")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(report) + "\n\nraw lines\n" + "\n".join(lines) + "\n")
    print("\n".join(report[-40:]), flush=True)


if __name__ == "__main__":
    main()
