"""Batched softmax Laplace benchmark (BatchedSoftmaxTarget.neg_hessian, laplace_init_softmax_batched;
csrc/gsmvi_softmax_laplace_batched.hip) on multinomial logit posteriors, x0 = 0, against the same computation as torch ops.

Writes one JSON object with, at K in {1024, 8192} x (N, C, P) in {(64, 3, 5), (256, 5, 4), (1024, 9, 8)} (the softmax target's
bench shapes), all in one process:
  hessian[]  one ``neg_hessian`` launch at a point of order one against the torch form (torch.bmm for eta, torch.softmax over the
             C classes with the reference class's zero appended, the Hessian by einsum: sum_n p_nc a_n a_n^T on the class
             blocks minus U^T U with u_nd = p_nc a_ni), alternated, one pair of device events per call, --reps (10) calls after
             a warm-up: median and range, and the ratio
  init[]     ``laplace_init_softmax_batched`` end to end against a Newton loop of torch ops with the same stopping rule (full
             step, Armijo backtracking with the same constants, max|g| <= 1e-8, per-problem freezing by masking, torch.linalg
             .cholesky / torch.cholesky_solve), and ``lbfgs_init_batched`` and ``pathfinder_init_batched`` on the same target:
             wall time of one call (device-synchronised host clock, alternated), rounds, problems with a start
  starts[]   the quality of the three starts as a start, as scripts/pathfinder_batched_bench.py reports it: the ELBO estimate
             mean(lp - log q) from 256 fresh draws and the PSIS khat (``psis_batched``, one set of keys): medians over the
             problems and the share of problems with khat below the threshold
Reported, not gated.
Usage: python scripts/softmax_laplace_bench.py [--out FILE] [--reps R] [--quick]
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

SHAPES = [(64, 3, 5), (256, 5, 4), (1024, 9, 8)]
LAM = 0.5
DRAWS = 5
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batched",
                           "softmax_laplace_bench.json")


def problems(K, N, Cc, P, seed):
    """K synthetic data sets on the device: A ~ N(0, 1) / sqrt(P), labels drawn from the model at W* ~ N(0, 1)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)      # noqa: E731
    A = rn(K, N, P) / np.sqrt(P)
    eta = torch.cat([torch.bmm(A, rn(K, P, Cc - 1)), torch.zeros(K, N, 1, dtype=torch.float64, device="cuda")], dim=2)
    y = torch.multinomial(torch.softmax(eta, 2).reshape(K * N, Cc), 1, generator=g).reshape(K, N)
    return A, y


class TorchSoftmax:
    """f = -lp, g = -score and H of the K posteriors as torch ops on the device, in the form a torch user would write"""

    def __init__(self, A, y, Cc, lam):
        self.A, self.C, self.lam = A, Cc, lam
        self.K, self.N, self.P = A.shape
        self.D = (Cc - 1) * self.P
        self.hot = torch.nn.functional.one_hot(y, Cc).to(torch.float64)                  # (K, N, C)
        self.eye = torch.eye(self.D, dtype=torch.float64, device=A.device)

    def probs(self, x):
        eta = torch.bmm(self.A, x.reshape(self.K, self.C - 1, self.P).transpose(1, 2))
        full = torch.cat([eta, eta.new_zeros(self.K, self.N, 1)], dim=2)
        return full, torch.softmax(full, dim=2)

    def f_g(self, x):
        full, p = self.probs(x)
        f = -((full * self.hot).sum(2) - torch.logsumexp(full, 2)).sum(1) + 0.5 * self.lam * (x * x).sum(1)
        r = (self.hot - p)[:, :, :self.C - 1]
        g = -(torch.bmm(r.transpose(1, 2), self.A).reshape(self.K, self.D) - self.lam * x)
        return f, g, p

    def hessian(self, x, p=None):
        if p is None:
            p = self.probs(x)[1]
        K, N, P, Cm = self.K, self.N, self.P, self.C - 1
        p = p[:, :, :Cm]
        U = (p[:, :, :, None] * self.A[:, :, None, :]).reshape(K, N, self.D)              # u_nd = p_nc a_ni
        H = (-torch.einsum("knd,kne->kde", U, U)).contiguous()
        blocks = torch.einsum("knc,kni,knj->kcij", p, self.A, self.A)                    # sum_n p_nc a_n a_n^T
        Hv = H.view(K, Cm, P, Cm, P)
        for c in range(Cm):
            Hv[:, c, :, c, :] += blocks[:, c]
        return H + self.lam * self.eye

    def newton(self, maxiter=100, maxfun=200, gtol=1e-8):
        """the damped Newton iteration of laplace_init_softmax_batched on whole-batch torch ops: the same constants, a problem
        that has stopped is masked out of every update; returns (mean, cov, rounds)"""
        K, D = self.K, self.D
        x = torch.zeros(K, D, dtype=torch.float64, device=self.A.device)
        f, g, p = self.f_g(x)
        done = g.abs().amax(1) <= gtol
        rounds = 1
        while rounds < maxfun and not bool(done.all().item()):
            L = torch.linalg.cholesky(self.hessian(x, p))
            d = -torch.cholesky_solve(g[:, :, None], L)[:, :, 0]
            gd = (g * d).sum(1)
            t = torch.ones(K, dtype=torch.float64, device=x.device)
            moved = done.clone()
            for _ in range(21):
                xt = x + t[:, None] * d
                ft, gt, pt = self.f_g(xt)
                rounds += 1
                ok = (ft <= f + 1e-4 * t * gd + 1e-10 * f.abs().clamp(min=1.0)) & ~moved
                x = torch.where(ok[:, None], xt, x)
                f, g = torch.where(ok, ft, f), torch.where(ok[:, None], gt, g)
                p = torch.where(ok[:, None, None], pt, p)
                moved |= ok
                if bool(moved.all().item()) or rounds >= maxfun:
                    break
                t = torch.where(moved, t, 0.5 * t)
            done |= (g.abs().amax(1) <= gtol) | ~moved
        cov = torch.cholesky_inverse(torch.linalg.cholesky(self.hessian(x, p)))
        return x, cov, rounds


def _stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def _events(fns, reps, warm=3):
    """per-call device-event times (ms) of the callables, alternated"""
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


def hessian_entry(tgt, ref, K, N, Cc, P, reps):
    g = torch.Generator(device="cuda").manual_seed(5)
    x = 0.5 * torch.randn(K, tgt.D, dtype=torch.float64, device="cuda", generator=g)
    out = tgt.engine.empty(K, tgt.D, tgt.D)
    ms = _events({"hip": lambda: tgt.engine.softmax_hessian_batched(x, tgt.A, tgt.y, Cc, counts=None, prior_prec=LAM, want="h", out=out),
                  "torch": lambda: ref.hessian(x)}, reps)
    err = float((out - ref.hessian(x)).abs().max().item())
    e = {"K": K, "N": N, "C": Cc, "P": P, "D": tgt.D, "reps": reps, "hip_ms": _stats(ms["hip"]), "torch_ms": _stats(ms["torch"]),
         "max_abs_difference": err}
    e["ratio"] = e["torch_ms"]["median"] / e["hip_ms"]["median"]
    e["time_source"] = "device events around one call (not profiler kernel time)"
    return e


def init_entry(tgt, ref, K, N, Cc, P, reps):
    x0 = torch.zeros(K, tgt.D, dtype=torch.float64, device="cuda")
    t, last = _wall({"laplace": lambda: gsmvi_amd.laplace_init_softmax_batched(tgt, as_torch=True),
                     "torch_newton": lambda: ref.newton(),
                     "lbfgs": lambda: gsmvi_amd.lbfgs_init_batched(x0, tgt.lp, tgt.lp_g, as_torch=True),
                     "pathfinder": lambda: gsmvi_amd.pathfinder_init_batched(x0, tgt.lp, tgt.lp_g, num_elbo_draws=DRAWS, as_torch=True)},
                    reps)
    e = {"K": K, "N": N, "C": Cc, "P": P, "D": tgt.D, "reps": reps}
    for name in ("laplace", "lbfgs", "pathfinder"):
        res = last[name][2]
        e[name] = {"call_s": _stats(t[name]), "nlaunch": res.nlaunch, "nit_max": int(res.nit.max()), "nfev_max": int(res.nfev.max()),
                   "with_a_start": int(res.success.sum())}
    e["torch_newton"] = {"call_s": _stats(t["torch_newton"]), "evaluations": last["torch_newton"][2],
                         "max_abs_mean_difference": float((last["torch_newton"][0] - last["laplace"][0]).abs().max().item())}
    e["torch_over_laplace"] = e["torch_newton"]["call_s"]["median"] / e["laplace"]["call_s"]["median"]
    return e, last


def starts_entry(tgt, last, K, N, Cc, P):
    keys = np.arange(K) + 7
    e = {"K": K, "N": N, "C": Cc, "P": P, "D": tgt.D, "draws": 256}
    for name in ("lbfgs", "laplace", "pathfinder"):
        mean, cov, _ = last[name]
        r = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=256, moments=False)
        fin = r.info == 0
        elbo = r.log_ratios.mean(1)
        e[name] = {"elbo_median": float(np.median(elbo[fin])), "khat_median": float(np.median(r.khat[fin])),
                   "khat_ok_share": float(r.ok.mean()), "psis_failed": int((~fin).sum())}
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="few repetitions, K = 1024 only")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 3 if args.quick else max(args.reps, 10)
    res = {"device": torch.cuda.get_device_name(0), "prior_precision": LAM, "hessian": [], "init": [], "starts": []}
    for K in ((1024,) if args.quick else (1024, 8192)):
        for N, Cc, P in SHAPES:
            A, y = problems(K, N, Cc, P, 11)
            tgt = gsmvi_amd.BatchedSoftmaxTarget(A, y, Cc, LAM)
            ref = TorchSoftmax(A, y, Cc, LAM)
            eh = hessian_entry(tgt, ref, K, N, Cc, P, reps)
            ei, last = init_entry(tgt, ref, K, N, Cc, P, max(reps // 3, 3))
            es = starts_entry(tgt, last, K, N, Cc, P)
            for key, e in (("hessian", eh), ("init", ei), ("starts", es)):
                res[key].append(e)
                print(json.dumps({key: e}), flush=True)
            del tgt, ref, A, y, last
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
