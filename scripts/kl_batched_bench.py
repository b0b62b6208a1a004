"""Batched KL monitor benchmark (BatchedKLMonitor, csrc/gsmvi_kl_batched.hip).

It writes one JSON object with:
  calls     one BatchedKLMonitor call (reverse KL on batch_size_kl draws + forward KL on as many reference rows, lp =
            BatchedGaussianTarget.lp, normalised) for K in {1024, 8192} x (D, batch_size_kl) in {(10, 32), (64, 32)}: call_ms
            by a synchronised host clock (median of --reps calls after warm-up), and the two kernels alone by device events:
            draw_ms, eval_ms, with the bytes each moves (mean, cov read; X written / Y read) and that over 8 TB/s
  device_loop  the same K = 1024 problems at (10, 32) through a loop of K DeviceKLMonitor calls: loop_ms and the ratio to one
            batched call
  fits      GSMBatch.fit and BaMBatch.fit at K = 1024, D = 10, B = 2, niter = 1000, with BatchedKLMonitor(checkpoint=10) and
            without a monitor: wall clock of the whole fit, problem-iterations/s, and the cost of one checkpoint
Usage: python scripts/kl_batched_bench.py [--out FILE] [--quick]
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

HBM_BYTES_PER_S = 8.0e12
LOG2PI = np.log(2 * np.pi)


def _problems(K, D, seed):
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((K, D, D))
    cov = A @ np.swapaxes(A, 1, 2) / D + np.eye(D)
    return rs.standard_normal((K, D)), cov


def _target(K, D, seed):
    m, cov = _problems(K, D, seed)
    tgt = gsmvi_amd.BatchedGaussianTarget(m, cov=cov)
    norms = tgt.mean.new_tensor(-0.5 * D * LOG2PI - 0.5 * np.linalg.slogdet(cov)[1])

    def lp(x):
        return tgt.lp(x) + norms * x.shape[1]
    return m, cov, tgt, lp


def _median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def _event_ms(fn, reps):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def call_entry(K, D, n, reps):
    eng = gsmvi_amd.get_engine()
    m, cov, tgt, lp = _target(K, D, 1)
    mq, Sq = _problems(K, D, 2)
    md, cd = eng.asarray(mq), eng.asarray(Sq)
    ref = np.random.RandomState(3).standard_normal((K, 2 * n, D))
    mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=n, ref_samples=ref)
    keys = list(range(K))
    call_ms = _median_ms(lambda: mon(0, [md, cd], lp, keys), reps)
    seeds = eng.batched_seeds(keys)
    X, lq, info = eng.kl_draw_batched(md, cd, seeds, 0, 0, n)
    draw_ms = _event_ms(lambda: eng.kl_draw_batched(md, cd, seeds, 0, 0, n, out=(X, lq), info=info), reps)
    eval_ms = _event_ms(lambda: eng.logq_batched(md, cd, X, out=lq, info=info), reps)
    mat = K * 8 * (D * D + D) + K * 8 * 2 + K * 4          # mean, cov read; seeds / logq, info
    rows = K * n * D * 8                                    # X written (draw) or Y read (eval)
    e = {"K": K, "D": D, "batch_size_kl": n, "call_ms": call_ms, "draw_ms": draw_ms, "eval_ms": eval_ms,
         "draw_bytes": mat + rows, "eval_bytes": mat + rows,
         "draw_hbm_fraction": (mat + rows) / (draw_ms * 1e-3) / HBM_BYTES_PER_S,
         "eval_hbm_fraction": (mat + rows) / (eval_ms * 1e-3) / HBM_BYTES_PER_S}
    return e, mon


def device_loop_entry(K, D, n, reps, batched_ms):
    eng = gsmvi_amd.get_engine()
    m, cov, tgt, lp = _target(K, D, 1)
    mq, Sq = _problems(K, D, 2)
    md, cd = eng.asarray(mq), eng.asarray(Sq)
    ref = np.random.RandomState(3).standard_normal((K, 2 * n, D))
    norms = -0.5 * D * LOG2PI - 0.5 * np.linalg.slogdet(cov)[1]
    P = tgt.P

    def lp_k(k):
        def f(x):
            r = tgt.mean[k][None, :] - x
            return -0.5 * torch.einsum("bi,ij,bj->", r, P[k], r) + float(norms[k]) * x.shape[0]
        return f
    lps = [lp_k(k) for k in range(K)]
    mons = [gsmvi_amd.DeviceKLMonitor(batch_size_kl=n, ref_samples=ref[k]) for k in range(K)]

    def loop():
        for k in range(K):
            mons[k](0, [md[k], cd[k]], lps[k], k)
    loop_ms = _median_ms(loop, max(1, reps // 5))
    return {"K": K, "D": D, "batch_size_kl": n, "loop_ms": loop_ms, "batched_call_ms": batched_ms,
            "speedup": loop_ms / batched_ms}


def fits_entry(K, D, B, niter, checkpoint):
    m, cov, tgt, lp = _target(K, D, 4)
    ref = np.random.RandomState(5).standard_normal((K, 64, D)) @ np.linalg.cholesky(cov).transpose(0, 2, 1) + m[:, None, :]
    keys = np.arange(K)
    out = {"K": K, "D": D, "B": B, "niter": niter, "checkpoint": checkpoint}
    for name, run in (("gsm", lambda mon: gsmvi_amd.GSMBatch(K, D, lp, tgt.lp_g).fit(
                          keys, batch_size=B, niter=niter, verbose=False, monitor=mon, as_torch=True)),
                      ("bam", lambda mon: gsmvi_amd.BaMBatch(K, D, lp, tgt.lp_g).fit(
                          keys, lambda i: 100.0 / (1 + i), batch_size=B, niter=niter, verbose=False, monitor=mon,
                          as_torch=True))):
        res = {}
        for label, mk in (("plain", lambda: None),
                          ("monitor", lambda: gsmvi_amd.BatchedKLMonitor(batch_size_kl=32, checkpoint=checkpoint,
                                                                         ref_samples=ref))):
            run(mk())                                   # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mon = mk()
            run(mon)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[label] = {"fit_s": dt, "problem_iters_per_s": K * (niter + 1) / dt,
                          "monitor_calls": 0 if mon is None else len(mon.rkl)}
        ncalls = res["monitor"]["monitor_calls"]
        res["checkpoint_ms"] = 1e3 * (res["monitor"]["fit_s"] - res["plain"]["fit_s"]) / ncalls
        res["iteration_ms"] = 1e3 * res["plain"]["fit_s"] / (niter + 1)
        res["checkpoint_over_iteration"] = res["checkpoint_ms"] / res["iteration_ms"]
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions (profiling runs)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 5 if args.quick else 20
    res = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S, "calls": []}
    for D, n in ((10, 32), (64, 32)):
        for K in (1024, 8192):
            e, _ = call_entry(K, D, n, reps)
            res["calls"].append(e)
            print(json.dumps(e), flush=True)
    base = next(e for e in res["calls"] if (e["K"], e["D"]) == (1024, 10))
    res["device_loop"] = device_loop_entry(1024, 10, 32, reps, base["call_ms"])
    print(json.dumps(res["device_loop"]), flush=True)
    res["fits"] = fits_entry(1024, 10, 2, 200 if args.quick else 1000, 10)
    print(json.dumps(res["fits"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
