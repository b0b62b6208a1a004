"""A/B of the three draw-based predictive launches between libraries ("The draw-predictive block"): the
launch of ``softmax_predict_bench.py``, ``negbin_predict_bench.py`` and ``ordinal_predict_bench.py`` (their ``problem`` and their
three shapes each, labels or counts given, uniform weights): 9 cases.

The method is ``laplace_sweep_ab.py``'s.  One child process per load of a library (``GSMVI_HIP_LIB_VARIANT``; "" is the library the
package loads), the libraries alternated ``--rounds`` times with the order rotated; per case the median of 10 calls by device
events after 10 warm-up calls.  The measure's own noise comes from the base library loaded a second time from a copy under
another file name (``--null``) and timed as if it were the candidate: the margin of a case is the larger of the spread of the
base's medians and the difference between the means of the base and of its copy, and a case passes if the mean of the candidate's
medians is not above the base's mean by more than that margin.  Every child runs under a time limit; after one that fails nothing
more is started.

  python scripts/predict_draws_ab.py --base parent --null parentcopy --out profiles/batched/predict_draws_ab_parent.txt
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
WARM, REPS = 10, 10


def launches(eng):
    """(family, shape, launch) of every case: the ``hip`` call of each bench script's ``entry`` on that script's inputs"""
    import negbin_predict_bench as nb
    import ordinal_predict_bench as ob
    import softmax_predict_bench as sb

    def draws(K, S, mean, cov):
        seeds = eng.batched_seeds(tuple((k % (2 ** 32)) ^ 0x5DEECE66D for k in range(K)))
        return eng.kl_draw_batched(mean, cov, seeds, 0, 0, S)[0]

    for K, M, C, P, S in sb.SHAPES:
        _, mean, cov, A_new, y_new = sb.problem(K, M, C, P, 11)
        X, A, y = draws(K, S, mean, cov), eng.asarray(A_new), eng.batched_labels(y_new)
        yield "softmax", (K, M, C, P, S), lambda X=X, A=A, y=y, C=C: eng.softmax_predict_batched(X, None, A, C, labels=y)
    for K, M, D, S in nb.SHAPES:
        _, mean, cov, A_new, y_new = nb.problem(K, M, D - 1, 11)
        X, A, y = draws(K, S, mean, cov), eng.asarray(A_new), eng.asarray(y_new)
        yield "negbin", (K, M, D, S), lambda X=X, A=A, y=y: eng.negbin_predict_batched(X, None, A, y=y)
    for K, M, P, C, S in ob.SHAPES:
        _, mean, cov, A_new, o_new, y_new = ob.problem(K, 64, M, P, C, 11)
        X, A, o, y = draws(K, S, mean, cov), eng.asarray(A_new), eng.asarray(o_new), eng.batched_labels(y_new.astype(np.int32))
        yield "ordinal", (K, M, P, C, S), lambda X=X, A=A, o=o, y=y, C=C: eng.ordinal_predict_batched(X, None, A, C, y=y, offset=o)


def worker():
    """every case with the library this process loads: one JSON line per case, the median in ms"""
    import torch
    import gsmvi_amd
    torch.cuda.set_device(0)
    eng = gsmvi_amd.get_engine()
    w = torch.randn(4096, 4096, device="cuda")
    for _ in range(50):                                     # the device clocked up first
        w = torch.tanh(w @ w * 1e-3)
    torch.cuda.synchronize()
    for family, shape, f in launches(eng):
        ts = []
        for r in range(-WARM, REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            if r >= 0:
                ts.append(a.elapsed_time(b))
        print(json.dumps({"family": family, "shape": list(shape), "launch": float(np.median(ts))}), flush=True)
        del f
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--base", default="parent", help="variant name of the base library")
    ap.add_argument("--null", default="parentcopy", help="variant name of a copy of the base library under another file name")
    ap.add_argument("--cand", default="", help="variant name of the candidate ('': the library the package loads)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched", "predict_draws_ab_parent.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker()
    libs = {"base": args.base, "null": args.null, "cand": args.cand}
    order = ["base", "cand", "null"]
    runs = {k: [] for k in libs}                            # role -> list (per round) of {case key: median}
    lines = []
    for r in range(args.rounds):
        for role in order[r % 3:] + order[:r % 3]:
            env = dict(os.environ, GSMVI_HIP_LIB_VARIANT=libs[role])
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=env, capture_output=True, text=True,
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
                    got[(e["family"], tuple(e["shape"]))] = e["launch"]
                    lines.append(f"round {r} {role:4s} {libs[role] or '(default)':10s} {ln}")
            runs[role].append(got)
            print(f"round {r} {role}: {len(got)} cases", flush=True)
    report = [f"base {args.base!r}, its copy {args.null!r}, candidate {args.cand or '(the default library)'!r}; {args.rounds} rounds, "
              f"median of {REPS} calls after {WARM}; times in ms", ""]
    npass = 0
    fmt = lambda v: " ".join(f"{t:.5f}" for t in v)         # noqa: E731
    for key in runs["base"][0]:
        b, n, c = ([run[key] for run in runs[role]] for role in ("base", "null", "cand"))
        spread, null = max(b) - min(b), abs(np.mean(n) - np.mean(b))
        margin = max(spread, null)
        ok = np.mean(c) <= np.mean(b) + margin
        npass += ok
        report.append(f"{key[0]:8s} {str(key[1]):28s} base {fmt(b)} | copy {fmt(n)} | cand {fmt(c)} | spread {spread:.5f} "
                      f"null {null:.5f} margin {margin:.5f} | cand - base {np.mean(c) - np.mean(b):+.5f} "
                      f"({100 * (np.mean(c) / np.mean(b) - 1):+.2f} %) {'pass' if ok else 'MISS'}")
    report += ["", f"{npass} of {len(runs['base'][0])} cases pass"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(report) + "\n\nraw lines\n" + "\n".join(lines) + "\n")
    print("\n".join(report), flush=True)


if __name__ == "__main__":
    main()
