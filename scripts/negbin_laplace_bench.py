"""Negative binomial Laplace initialiser benchmark (gsmvi_negbin_hessian_batched_f64, gsmvi_negbin_laplace_step_batched_f64 in
csrc/gsmvi_negbin_laplace_batched.hip; ``laplace_init_negbin_batched``).

Writes one JSON object with
  cases[]  K in {1024, 8192} x (N, D) in {(64, 10), (256, 16), (1024, 64)}, D = P + 1:
           hessian, step: device-event times (ms; median, min, max of --reps >= 10, default 20, calls after a warm-up) of the
             Hessian launch and of the first step launch (f, g, H, the factorisation, the direction), alternated call by call
             with their comparisons: the same quantities as whole-batch torch ops (digamma, polygamma, bmm), and the Poisson
             launches of ``glm_hessian_batched`` / ``laplace_step_batched`` at the same (K, N, P) -- what the link costs
           init: host-clock seconds (device-synchronised) of ``laplace_init_negbin_batched`` end to end, of the same Newton loop
             with the same last-pivot rule as torch ops, of ``lbfgs_init_batched`` and of ``pathfinder_init_batched`` on the same
             problems, alternated in this process; rounds, iterations, problems with a start, problems with a modified pivot
           starts: per initialiser the median ELBO estimate from 256 fresh draws (``psis_batched``) and the share of problems
             with khat below the threshold
           ratio = comparison median / HIP median; slower = the HIP median is the larger one
  library_sha256: of the library that ran
Every case runs in a child process under a time limit (--case-limit seconds); after a case that fails or runs out of time no
further case is started.  Nothing is gated on the figures.
Usage: python scripts/negbin_laplace_bench.py [--out FILE] [--reps R] [--quick]
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
LAM, KAP = 0.5, 1.0


class TorchNegBin:
    """f = -lp, g, H and the Newton loop of the negative binomial target as whole-batch torch ops on the device"""

    def __init__(self, torch, A, y, o):
        self.t, self.A, self.y, self.o = torch, A, y, o
        self.K, self.N, self.P = A.shape

    def parts(self, x, second=True):
        t = self.t
        P = self.P
        beta, th = x[:, :P], x[:, P:]
        r = th.exp()
        d = t.bmm(self.A, beta[:, :, None])[:, :, 0] + self.o - th
        sg, sn, spd, spn = t.sigmoid(d), t.sigmoid(-d), t.nn.functional.softplus(d), t.nn.functional.softplus(-d)
        y = self.y
        dlg = t.lgamma(y + r) - t.lgamma(r)
        dps = t.special.digamma(y + r) - t.special.digamma(r)
        tt = dlg - r * spd - y * spn
        re = y * sn - r * sg
        rt = r * (dps - spd) - re
        f = -(tt.sum(1) - 0.5 * LAM * (beta * beta).sum(1) - 0.5 * KAP * (th[:, 0] ** 2))
        g = -t.cat([t.bmm(re[:, None, :], self.A)[:, 0, :] - LAM * beta, rt.sum(1, keepdim=True) - KAP * th], dim=1)
        if not second:
            return f, g, None
        dtg = t.special.polygamma(1, y + r) - t.special.polygamma(1, r)
        wee, wet = (y + r) * sg * sn, -sg * re
        wtt = -(r * (dps - spd) + r * r * dtg + r * sg - sg * re)
        H = x.new_zeros(self.K, P + 1, P + 1)
        H[:, :P, :P] = t.bmm((self.A * wee[:, :, None]).transpose(1, 2), self.A) + LAM * t.eye(P, dtype=x.dtype, device=x.device)
        c = t.bmm(wet[:, None, :], self.A)[:, 0, :]
        H[:, :P, P], H[:, P, :P] = c, c
        H[:, P, P] = wtt.sum(1) + KAP
        return f, g, H

    def direction(self, g, H):
        """d = -(modified H)^{-1} g by elimination of the border: the last pivot s replaced by |s|"""
        t, P = self.t, self.P
        L = t.linalg.cholesky(H[:, :P, :P])
        v = t.linalg.solve_triangular(L, H[:, :P, P:], upper=False)
        s = (H[:, P, P] - (v[:, :, 0] ** 2).sum(1)).abs()
        z = t.linalg.solve_triangular(L, g[:, :P, None], upper=False)
        zl = (g[:, P] - (v[:, :, 0] * z[:, :, 0]).sum(1)) / s.sqrt()
        dl = zl / s.sqrt()
        db = t.linalg.solve_triangular(L.transpose(1, 2), z - v * dl[:, None, None], upper=True)[:, :, 0]
        return -t.cat([db, dl[:, None]], dim=1)

    def newton(self, maxfun=200, gtol=1e-8):
        t = self.t
        K = self.K
        x = t.zeros(K, self.P + 1, dtype=t.float64, device=self.A.device)
        f, g, H = self.parts(x)
        done = g.abs().amax(1) <= gtol
        rounds = 1
        while rounds < maxfun and not bool(done.all().item()):
            d = self.direction(g, H)
            gd = (g * d).sum(1)
            step = t.ones(K, dtype=t.float64, device=x.device)
            moved = done.clone()
            for _ in range(21):
                xt = x + step[:, None] * d
                ft, gt, Ht = self.parts(xt)
                rounds += 1
                ok = (ft <= f + 1e-4 * step * gd + 1e-10 * f.abs().clamp(min=1.0)) & ~moved
                x = t.where(ok[:, None], xt, x)
                f, g, H = t.where(ok, ft, f), t.where(ok[:, None], gt, g), t.where(ok[:, None, None], Ht, H)
                moved |= ok
                if bool(moved.all().item()) or rounds >= maxfun:
                    break
                step = t.where(moved, step, 0.5 * step)
            done |= (g.abs().amax(1) <= gtol) | ~moved
        return x, t.linalg.inv(H), rounds


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def events(torch, fns, reps, warm=3):
    """per-call device-event times (ms) of the (prepare, call) pairs, alternated; ``prepare`` runs outside the timed span"""
    out = {k: [] for k in fns}
    for r in range(-warm, reps):
        for k, (prep, f) in fns.items():
            if prep is not None:
                prep()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            if r >= 0:
                out[k].append(a.elapsed_time(b))
    return out


def wall(torch, fns, reps):
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


def versus(t, hip, others):
    e = {"hip_ms": stats(t[hip])}
    for name in others:
        s = stats(t[name])
        e[name] = {"ms": s, "ratio": s["median"] / e["hip_ms"]["median"], "slower": bool(e["hip_ms"]["median"] > s["median"])}
    return e


def run_case(K, N, D, reps, init_reps):
    import torch
    import gsmvi_amd
    torch.cuda.set_device(0)
    eng = gsmvi_amd.get_engine()
    P = D - 1
    g = torch.Generator(device="cuda").manual_seed(11)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)      # noqa: E731
    A = rn(K, N, P) / np.sqrt(P)
    o = 1.0 + 0.3 * rn(K, N)
    mu = torch.exp(torch.bmm(A, 0.7 * rn(K, P, 1))[:, :, 0] + o)
    size = 3.0
    lamb = torch.distributions.Gamma(torch.full_like(mu, size), size / mu).sample()
    y = torch.poisson(lamb, generator=g)
    tgt = gsmvi_amd.BatchedNegBinomialTarget(A, y, prior_precision=LAM, offset=o, log_size_mean=0.0, log_size_precision=KAP)
    pois = gsmvi_amd.BatchedGLMTarget(A, y, "poisson", prior_precision=LAM, offset=o)
    ref = TorchNegBin(torch, tgt.A, tgt.y, tgt.offset)
    model = dict(offset=tgt.offset, prior_prec=LAM, log_size_mean=0.0, log_size_prec=KAP)
    x = torch.cat([0.3 * rn(K, P), 1.0 + 0.3 * rn(K, 1)], dim=1).contiguous()
    xp = x[:, :P].contiguous()
    Hn, Hp = eng.empty(K, D, D), eng.empty(K, P, P)
    opt = dict(maxiter=100, maxfun=200, gtol=1e-8)
    x0, x0p = eng.zeros(K, D), eng.zeros(K, P)
    stn, stp = eng.laplace_state_batched(x0), eng.laplace_state_batched(x0p)
    t = events(torch, {
        "hessian_hip": (None, lambda: eng.negbin_hessian_batched(x, tgt.A, tgt.y, want="h", out=Hn, **model)),
        "hessian_torch": (None, lambda: ref.parts(x)),
        "hessian_poisson": (None, lambda: eng.glm_hessian_batched(xp, pois.A, pois.y, "poisson", offset=pois.offset, prior_prec=LAM,
                                                                 want="h", out=Hp)),
        "step_hip": (lambda: stn["Xt"].copy_(x0), lambda: eng.negbin_laplace_step_batched(stn, tgt.A, tgt.y, start=True, **opt, **model)),
        "step_torch": (None, lambda: ref.direction(*ref.parts(x0)[1:])),
        "step_poisson": (lambda: stp["Xt"].copy_(x0p),
                         lambda: eng.laplace_step_batched(stp, pois.A, pois.y, "poisson", offset=pois.offset, prior_prec=LAM,
                                                          start=True, **opt)),
    }, reps)
    Ht = ref.parts(x)[2]
    e = {"K": K, "N": N, "D": D, "P": P, "reps": reps, "init_reps": init_reps,
         "hessian": versus(t, "hessian_hip", ("hessian_torch", "hessian_poisson")),
         "step": versus(t, "step_hip", ("step_torch", "step_poisson")),
         "max_rel_diff_H_vs_torch": float(((Hn - Ht).abs().amax((1, 2)) / Ht.abs().amax((1, 2))).max())}
    w, last = wall(torch, {
        "laplace": lambda: gsmvi_amd.laplace_init_negbin_batched(tgt, as_torch=True),
        "torch_newton": lambda: ref.newton(),
        "lbfgs": lambda: gsmvi_amd.lbfgs_init_batched(x0, tgt.lp, tgt.lp_g, as_torch=True),
        "pathfinder": lambda: gsmvi_amd.pathfinder_init_batched(x0, tgt.lp, tgt.lp_g, num_elbo_draws=256, as_torch=True)}, init_reps)
    init = {}
    for name in ("laplace", "lbfgs", "pathfinder"):
        res = last[name][2]
        init[name] = {"call_s": stats(w[name]), "nlaunch": int(res.nlaunch), "nit_max": int(res.nit.max()),
                      "nfev_max": int(res.nfev.max()), "with_a_start": int(res.success.sum())}
    init["laplace"]["modified_pivot_problems"] = int((last["laplace"][2].nmod > 0).sum())
    init["laplace"]["status_counts"] = np.bincount(last["laplace"][2].status, minlength=6).tolist()
    init["torch_newton"] = {"call_s": stats(w["torch_newton"]), "evaluations": int(last["torch_newton"][2]),
                            "max_abs_mean_difference": float((last["torch_newton"][0] - last["laplace"][0]).abs().max().item())}
    for name in ("torch_newton", "lbfgs", "pathfinder"):
        init[name]["ratio"] = init[name]["call_s"]["median"] / init["laplace"]["call_s"]["median"]
        init[name]["slower"] = bool(init["laplace"]["call_s"]["median"] > init[name]["call_s"]["median"])
    e["init"] = init
    keys = np.arange(K) + 7
    starts = {"draws": 256}
    for name in ("lbfgs", "laplace", "pathfinder"):
        mean, cov, _ = last[name]
        r = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=256, moments=False)
        fin = r.info == 0
        starts[name] = {"elbo_median": float(np.median(r.log_ratios.mean(1)[fin])) if fin.any() else None,
                        "khat_median": float(np.median(r.khat[fin])) if fin.any() else None,
                        "khat_ok_share": float(r.ok.mean()), "psis_failed": int((~fin).sum())}
    e["starts"] = starts
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched", "negbin_laplace_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--init-reps", type=int, default=3, help="repetitions of the end-to-end initialisers")
    ap.add_argument("--quick", action="store_true", help="K = 1024 only")
    ap.add_argument("--case-limit", type=float, default=240.0, help="seconds a case (a child process) may take")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)        # K,N,D: run it here and print its entry
    args = ap.parse_args()
    reps = max(args.reps, 10)
    if args.case:
        K, N, D = args.case.split(",")
        print(json.dumps(run_case(int(K), int(N), int(D), reps, max(args.init_reps, 1))), flush=True)
        return
    from gsmvi_amd import _lib
    res = {"library_sha256": hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest(), "prior_precision": LAM,
           "log_size_precision": KAP, "reps": reps, "cases": [], "stopped": None}
    for K in KS[:1] if args.quick else KS:
        for N, D in SHAPES:
            case = f"{K},{N},{D}"
            cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(reps), "--init-reps", str(args.init_reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.case_limit)
                rc, tail = r.returncode, (r.stdout.strip().splitlines() or [""])[-1]
                if rc != 0:
                    tail = (tail + " | " + r.stderr.strip()[-400:])
            except subprocess.TimeoutExpired:
                rc, tail = 124, ""
            if rc != 0:                                               # nothing more is started on the device after this
                res["stopped"] = {"case": case, "status": rc, "output": tail[-800:]}
                break
            e = json.loads(tail)
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
