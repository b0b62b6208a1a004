"""Ordinal Laplace initialiser benchmark (gsmvi_ordinal_hessian_batched_f64, gsmvi_ordinal_laplace_step_batched_f64 in
csrc/gsmvi_ordinal_laplace_batched.hip; ``laplace_init_ordinal_batched``).

Writes one JSON object with
  cases[]  K in {1024, 8192} x (N, P, C) in {(64, 6, 5), (256, 10, 7), (1024, 48, 17)}, D = P + C - 1:
           hessian, step: device-event times (ms; median, min, max of --reps >= 20 calls after a warm-up) of the Hessian launch
             and of the first step launch (f, g, H, the factorisation, the direction), alternated call by call with their
             comparisons: the same quantities as whole-batch torch ops (sigmoid, softplus, bmm, cholesky), and the logistic
             launches of ``glm_hessian_batched`` / ``laplace_step_batched`` at the same (K, N, D) -- what the link and the delta
             block cost
           init: host-clock seconds (device-synchronised) of ``laplace_init_ordinal_batched`` end to end, of the same Newton loop
             with the same retry rule as torch ops, of ``lbfgs_init_batched`` and of ``pathfinder_init_batched`` on the same
             problems, alternated in this process; rounds, iterations, problems with a start, problems with a retried round
           starts: per initialiser the median ELBO estimate from 256 fresh draws (``psis_batched``) and the share of problems
             with khat below the threshold
           ratio = comparison median / HIP median; slower = the HIP median is the larger one
  library_sha256: of the library that ran
Every case runs in a child process under a time limit (--case-limit seconds); after a case that fails or runs out of time no
further case is started.  Nothing is gated on the figures.
Usage: python scripts/ordinal_laplace_bench.py [--out FILE] [--reps R] [--quick]
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

SHAPES = [(64, 6, 5), (256, 10, 7), (1024, 48, 17)]
KS = (1024, 8192)
LAM, KAP = 1.0, 1.0


class TorchOrdinal:
    """f = -lp, g, H, the chain terms and the Newton loop of the ordinal target as whole-batch torch ops on the device"""

    def __init__(self, torch, A, y, o, C):
        self.t, self.A, self.y, self.o, self.C = torch, A, y.long(), o, C
        self.K, self.N, self.P = A.shape
        lc = C - 1
        i = torch.arange(lc, device=A.device)
        self.below = (i[None, None, :] < self.y[:, :, None]).to(A.dtype)
        self.at = (i[None, None, :] == self.y[:, :, None]).to(A.dtype)
        self.cnt = self.at.sum(1)
        self.cnt[:, 0] = 0.0
        self.mx = torch.maximum(i[:, None], i[None, :])
        self.lo, self.hi = (self.y >= 1).to(A.dtype), (self.y <= C - 2).to(A.dtype)
        self.ya, self.yb = (self.y - 1).clamp(min=0), self.y.clamp(max=lc - 1)

    def parts(self, x, second=True):
        t, P, lc = self.t, self.P, self.C - 1
        F = t.nn.functional
        beta, delta = x[:, :P], x[:, P:]
        w = t.cat([t.ones_like(delta[:, :1]), delta[:, 1:].exp()], dim=1)
        cut = t.cumsum(t.cat([delta[:, :1], w[:, 1:]], dim=1), dim=1)
        eta = t.bmm(self.A, beta[:, :, None])[:, :, 0] + self.o
        a, b = t.gather(cut, 1, self.ya) - eta, t.gather(cut, 1, self.yb) - eta
        lo, hi = self.lo, self.hi
        sga, sgb = t.sigmoid(a) * lo, t.sigmoid(-b) * hi
        lm = t.cat([t.zeros_like(w[:, :1]), t.log(-t.expm1(-w[:, 1:]))], dim=1)
        q = t.cat([t.zeros_like(w[:, :1]), 1.0 / t.expm1(w[:, 1:])], dim=1)
        tt = -F.softplus(a) * lo - F.softplus(-b) * hi + t.gather(lm, 1, self.yb) * lo * hi
        re = sga - sgb
        Sv = (self.below * (-re)[:, :, None] + self.at * sgb[:, :, None]).sum(1) + q * self.cnt
        f = -(tt.sum(1) - 0.5 * LAM * (beta * beta).sum(1) - 0.5 * KAP * (delta * delta).sum(1))
        g = -t.cat([t.bmm(re[:, None, :], self.A)[:, 0, :] - LAM * beta, w * Sv - KAP * delta], dim=1)
        if not second:
            return f, g, None, None
        fa, fb = sga * t.sigmoid(-a), t.sigmoid(b) * sgb
        fab = fa + fb
        E = self.below * fab[:, :, None] + self.at * fb[:, :, None]
        Fv = E.sum(1)
        c = -(w * Sv)
        c[:, 0] = 0.0
        wq = w * q
        H = x.new_zeros(self.K, P + lc, P + lc)
        H[:, :P, :P] = t.bmm((self.A * fab[:, :, None]).transpose(1, 2), self.A) + LAM * t.eye(P, dtype=x.dtype, device=x.device)
        bd = -t.bmm(self.A.transpose(1, 2), E) * w[:, None, :]
        H[:, :P, P:], H[:, P:, :P] = bd, bd.transpose(1, 2)
        dd = w[:, :, None] * w[:, None, :] * Fv[:, self.mx]
        H[:, P:, P:] = dd + t.diag_embed(wq * (w + wq) * self.cnt + c + KAP)
        return f, g, H, c

    def direction(self, g, H, c):
        """d = -H^{-1} g, or with the retried matrix H - diag(min(c, 0)) where H does not factor"""
        t, P = self.t, self.P
        L, info = t.linalg.cholesky_ex(H)
        Hm = H.clone()
        idx = t.arange(P, H.shape[1], device=H.device)
        Hm[:, idx, idx] = Hm[:, idx, idx] - c.clamp(max=0.0)
        L2, _ = t.linalg.cholesky_ex(Hm)
        L = t.where((info != 0)[:, None, None], L2, L)
        return -t.cholesky_solve(g[:, :, None], L)[:, :, 0]

    def newton(self, maxfun=200, gtol=1e-8):
        t = self.t
        K = self.K
        x = t.zeros(K, self.P + self.C - 1, dtype=t.float64, device=self.A.device)
        f, g, H, c = self.parts(x)
        done = g.abs().amax(1) <= gtol
        rounds = 1
        while rounds < maxfun and not bool(done.all().item()):
            d = self.direction(g, H, c)
            gd = (g * d).sum(1)
            step = t.ones(K, dtype=t.float64, device=x.device)
            moved = done.clone()
            for _ in range(21):
                xt = x + step[:, None] * d
                ft, gt, Ht, ct = self.parts(xt)
                rounds += 1
                ok = (ft <= f + 1e-4 * step * gd + 1e-10 * f.abs().clamp(min=1.0)) & ~moved
                x = t.where(ok[:, None], xt, x)
                f, g, H = t.where(ok, ft, f), t.where(ok[:, None], gt, g), t.where(ok[:, None, None], Ht, H)
                c = t.where(ok[:, None], ct, c)
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


def run_case(K, N, P, C, reps, init_reps):
    import torch
    import gsmvi_amd
    torch.cuda.set_device(0)
    eng = gsmvi_amd.get_engine()
    D = P + C - 1
    g = torch.Generator(device="cuda").manual_seed(11)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)      # noqa: E731
    A = rn(K, N, P) / np.sqrt(P)
    o = 0.3 * rn(K, N)
    eta = torch.bmm(A, rn(K, P, 1))[:, :, 0] + o
    cuts = torch.sort(1.5 * rn(K, C - 1), dim=1).values
    u = torch.rand(K, N, dtype=torch.float64, device="cuda", generator=g)
    y = (u[:, :, None] > torch.sigmoid(cuts[:, None, :] - eta[:, :, None])).sum(2).to(torch.int32)
    tgt = gsmvi_amd.BatchedOrdinalTarget(A, y, C, prior_precision=LAM, cut_precision=KAP, offset=o)
    Ad = rn(K, N, D) / np.sqrt(D)
    yb = (torch.rand(K, N, dtype=torch.float64, device="cuda", generator=g) < torch.sigmoid(torch.bmm(Ad, rn(K, D, 1))[:, :, 0])).double()
    logi = gsmvi_amd.BatchedGLMTarget(Ad, yb, "logistic", prior_precision=LAM)
    ref = TorchOrdinal(torch, tgt.A, tgt.y, tgt.offset, C)
    model = dict(offset=tgt.offset, prior_prec=LAM, cut_prec=KAP)
    x = torch.cat([0.3 * rn(K, P + 1), -0.5 + 0.3 * rn(K, C - 2)], dim=1).contiguous()
    Hn, Hl = eng.empty(K, D, D), eng.empty(K, D, D)
    opt = dict(maxiter=100, maxfun=200, gtol=1e-8)
    x0 = eng.zeros(K, D)
    stn, stl = eng.laplace_state_batched(x0), eng.laplace_state_batched(x0)
    t = events(torch, {
        "hessian_hip": (None, lambda: eng.ordinal_hessian_batched(x, tgt.A, tgt.y, C, want="h", out=Hn, **model)),
        "hessian_torch": (None, lambda: ref.parts(x)),
        "hessian_logistic": (None, lambda: eng.glm_hessian_batched(x, logi.A, logi.y, "logistic", prior_prec=LAM, want="h", out=Hl)),
        "step_hip": (lambda: stn["Xt"].copy_(x0), lambda: eng.ordinal_laplace_step_batched(stn, tgt.A, tgt.y, C, start=True, **opt, **model)),
        "step_torch": (None, lambda: ref.direction(*ref.parts(x0)[1:])),
        "step_logistic": (lambda: stl["Xt"].copy_(x0),
                          lambda: eng.laplace_step_batched(stl, logi.A, logi.y, "logistic", prior_prec=LAM, start=True, **opt)),
    }, reps)
    Ht = ref.parts(x)[2]
    e = {"K": K, "N": N, "P": P, "C": C, "D": D, "reps": reps, "init_reps": init_reps,
         "hessian": versus(t, "hessian_hip", ("hessian_torch", "hessian_logistic")),
         "step": versus(t, "step_hip", ("step_torch", "step_logistic")),
         "max_rel_diff_H_vs_torch": float(((Hn - Ht).abs().amax((1, 2)) / Ht.abs().amax((1, 2))).max())}
    w, last = wall(torch, {
        "laplace": lambda: gsmvi_amd.laplace_init_ordinal_batched(tgt, as_torch=True),
        "torch_newton": lambda: ref.newton(),
        "lbfgs": lambda: gsmvi_amd.lbfgs_init_batched(x0, tgt.lp, tgt.lp_g, as_torch=True),
        "pathfinder": lambda: gsmvi_amd.pathfinder_init_batched(x0, tgt.lp, tgt.lp_g, num_elbo_draws=256, as_torch=True)}, init_reps)
    init = {}
    for name in ("laplace", "lbfgs", "pathfinder"):
        res = last[name][2]
        init[name] = {"call_s": stats(w[name]), "nlaunch": int(res.nlaunch), "nit_max": int(res.nit.max()),
                      "nfev_max": int(res.nfev.max()), "with_a_start": int(res.success.sum())}
    init["laplace"]["retried_round_problems"] = int((last["laplace"][2].nmod > 0).sum())
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched", "ordinal_laplace_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--init-reps", type=int, default=3, help="repetitions of the end-to-end initialisers")
    ap.add_argument("--quick", action="store_true", help="K = 1024 only")
    ap.add_argument("--case-limit", type=float, default=240.0, help="seconds a case (a child process) may take")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)        # K,N,P,C: run it here and print its entry
    args = ap.parse_args()
    reps = max(args.reps, 20)
    if args.case:
        K, N, P, C = (int(v) for v in args.case.split(","))
        print(json.dumps(run_case(K, N, P, C, reps, max(args.init_reps, 1))), flush=True)
        return
    from gsmvi_amd import _lib
    res = {"library_sha256": hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest(), "prior_precision": LAM,
           "cut_precision": KAP, "reps": reps, "cases": [], "stopped": None}
    for K in KS[:1] if args.quick else KS:
        for N, P, C in SHAPES:
            case = f"{K},{N},{P},{C}"
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
