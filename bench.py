#!/usr/bin/env python3
"""bench.py -- GSM updates/sec + achieved HBM GB/s at D=1024, B=32 (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one GSM update -- gsm_update(samples, vs, mu0, S0) -> (mu, S), reference
gsmvi/gsm_numpy.py:27-55 -- at configs[2] of BASELINE.json (D=1024, B=32, dense covariance,
synthetic Gaussian target, fp64), inputs resident in HBM before the timed region.  To keep the
Infinity Cache (256 MiB) from serving the covariance, the steps cycle over a ring of independent
problem instances whose footprint exceeds it; with --full the cache-resident rate (one instance,
what a real fit loop sees) is reported beside it as "value_cache_resident".

A plain run sets up, warms up, times K steps and prints the headline.  --full adds the secondary
figures (per-step device-time statistics, roofline and calibration, the D=4096 point, fit-iteration
and call-path rates, CPU baseline); the --no-* switches below trim that set.  --dump-outputs DIR
writes the last timed step's (mu, S) as DIR/mu.npy, DIR/S.npy (float64); the inputs are seeded, so
two builds can be compared output for output.

N > 1: the batch is sharded across ranks (B/N samples each), records are all-gathered over RCCL
and every replica applies the combined update (gsm-vi_amd/dist.py); total work is fixed ->
"scaling": "strong".  Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (guide: MI355X_MICROARCH.md, chip-level parameters)
DUMP_LIMIT_BYTES = 64 * 2 ** 20     # --dump-outputs: all files together


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=400)
    ap.add_argument("--D", type=int, default=1024)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--instances", type=int, default=0, help="ring size (0 = enough to exceed the Infinity Cache)")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of a captured hipGraph")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-large-point", action="store_true", help="skip the D=4096 roofline point of the covariance kernel")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-callpath", action="store_true", help="skip the host / autograd score call-path rates")
    ap.add_argument("--tune", action="append", default=[], help="name=value launch knob (experiments)")
    ap.add_argument("--in-flight", type=int, default=1,
                    help="also measure the throughput with this many independent updates in flight (one HIP stream "
                         "and one engine context each; compute of one overlaps the collective of another). Reported "
                         "as value_in_flight beside the sequential `value`; opt-in")
    ap.add_argument("--shard", choices=("batch", "rows"), default="batch",
                    help="N>1 decomposition: batch (north_star; records all-gathered) or covariance row blocks "
                         "(SURVEY 8(f)3; SG column slices all-gathered, D^2 passes divided by N)")
    ap.add_argument("--full", action="store_true",
                    help="also measure every secondary figure: per-step device-time statistics, cache-resident rate, "
                         "roofline and HBM calibration, the D=4096 point, fit-iteration and call-path rates, CPU baseline. "
                         "Without it a run times the headline steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the last timed step (mu, S; float64) as DIR/<name>.npy, "
                         f"at most {DUMP_LIMIT_BYTES >> 20} MB in all (a seeded sample of rows beyond that)")
    return ap.parse_args(argv)


def make_instances(eng, D, B, n_inst, seed0=0, ldpad=0):
    """Synthetic state per SURVEY 8(d): target m, P; per instance mu0, S0 = A A^T/D + 0.1 I,
    samples = mu0 + z chol(S0)^T, scores from the HIP Gaussian-score kernel.  Data generation
    uses torch (plumbing); the benchmarked path does not."""
    dev = eng.device
    g = torch.Generator(device=dev)
    g.manual_seed(1234 + seed0)
    m = torch.rand(D, dtype=torch.float64, device=dev, generator=g)
    L = torch.randn(D, D, dtype=torch.float64, device=dev, generator=g)
    cov_t = L @ L.T + 1e-3 * torch.eye(D, dtype=torch.float64, device=dev)
    P = torch.linalg.inv(cov_t)
    P = (0.5 * (P + P.T)).contiguous()
    inst = []
    for k in range(n_inst):
        mu0 = torch.randn(D, dtype=torch.float64, device=dev, generator=g)
        A = torch.randn(D, D, dtype=torch.float64, device=dev, generator=g)
        S0 = A @ A.T / D + 0.1 * torch.eye(D, dtype=torch.float64, device=dev)
        S0 = (0.5 * (S0 + S0.T)).contiguous()
        Lc = torch.linalg.cholesky(S0)
        Z = torch.randn(B, D, dtype=torch.float64, device=dev, generator=g)
        X = mu0[None, :] + Z @ Lc.T
        G = eng.gaussian_score(X, m, P)
        if ldpad:                                  # padded leading dimension (row stride != power of two)
            S0p = eng.empty(D, D + ldpad)[:, :D]
            S0p.copy_(S0)
            Sout = eng.empty(D, D + ldpad)[:, :D]
        else:
            S0p, Sout = S0.contiguous(), eng.empty(D, D)
        inst.append(dict(X=X.contiguous(), G=G, mu0=mu0, S0=S0p, mu=eng.empty(D), S=Sout))
    torch.cuda.synchronize()
    return inst, m, P


def dump_outputs(dirname, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: every (name, tensor) as float64 DIR/<name>.npy.  A matrix that would take the total past `limit` is
    written as a fixed, seeded sample of its rows instead (<name>_sample.npy, the row indices in <name>_sample_rows.npy), so
    that two runs with the same arguments write the same files."""
    os.makedirs(dirname, exist_ok=True)
    used = 0
    for name, t in arrays:
        a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float64)
        if used + a.nbytes > limit and a.ndim == 2:
            n = min(a.shape[0], (limit - used) // (a[0].nbytes + 8))          # each row and its index
            rows = np.sort(np.random.default_rng(0).choice(a.shape[0], size=max(n, 0), replace=False))
            np.save(os.path.join(dirname, f"{name}_sample_rows.npy"), rows.astype(np.float64))
            used += rows.nbytes
            a, name = a[rows], f"{name}_sample"
        if used + a.nbytes > limit or a.size == 0:
            raise ValueError(f"--dump-outputs: {name} does not fit in {limit} bytes")
        np.save(os.path.join(dirname, f"{name}.npy"), a)
        used += a.nbytes


def cpu_baseline(D, B, seconds):
    """The oracle's faithful restatement of gsm_numpy.gsm_update ("port") on the host cores."""
    from oracle import gsm_oracle as orc
    st = orc.make_update_state(D, B, 0)
    try:
        from threadpoolctl import threadpool_info
        threads = max([p.get("num_threads", 1) for p in threadpool_info()] or [1])
    except Exception:
        threads = os.cpu_count() or 1
    orc.gsm_update_faithful(st["samples"][:2], st["vs"][:2], st["mu0"], st["S0"])      # touch BLAS
    n, t0 = 0, time.perf_counter()
    while True:
        orc.gsm_update_faithful(st["samples"], st["vs"], st["mu0"], st["S0"])
        n += 1
        el = time.perf_counter() - t0
        if (el >= seconds and n >= 2) or n >= 200:
            break
    tb0 = time.perf_counter()
    nb = 0
    while time.perf_counter() - tb0 < min(2.0, seconds / 4) or nb < 3:
        orc.gsm_update_batched(st["samples"], st["vs"], st["mu0"], st["S0"])
        nb += 1
    tb = time.perf_counter() - tb0
    one_core = None
    try:                                         # the same port pinned to one BLAS thread
        from threadpoolctl import threadpool_limits
        with threadpool_limits(limits=1):
            n1, t1 = 0, time.perf_counter()
            while time.perf_counter() - t1 < min(4.0, seconds / 3) or n1 < 2:
                orc.gsm_update_faithful(st["samples"], st["vs"], st["mu0"], st["S0"])
                n1 += 1
            one_core = n1 / (time.perf_counter() - t1)
    except Exception:
        one_core = None
    # F on the CPU ("report U and F exactly as for the GPU"): the reference's own loop -- MT19937 + SVD sampler,
    # Gaussian score, faithful update, Cholesky accept test (gsm_numpy.py:105-125, restated as oracle.gsm_fit)
    fit_cpu = None
    try:
        mt, _, Pt = orc.make_gaussian_target(D, 0)
        lp_g = lambda x: orc.gaussian_score(x, mt, Pt)
        tf0 = time.perf_counter()
        nfit = 0
        while time.perf_counter() - tf0 < min(6.0, seconds / 2) or nfit < 2:
            orc.gsm_fit(D, None, lp_g, 1, batch_size=B, niter=1)     # niter + 1 = 2 iterations per call
            nfit += 2
        fit_cpu = nfit / (time.perf_counter() - tf0)
    except Exception as e:                       # a reported baseline, never fatal
        fit_cpu = f"failed: {type(e).__name__}: {e}"
    return {"value": n / el, "unit": "updates/s", "cores": int(threads), "kind": "port",
            "sample": f"{n} updates of D={D},B={B} (oracle/gsm_oracle.py:gsm_update_faithful, numpy fp64, "
                      f"{os.cpu_count()} host cpus)",
            "value_is": "the faithful port of gsm_numpy.gsm_update (its B x D x D temporaries included) with numpy's BLAS on all "
                        "host threads -- the reference's own operation sequence on this box; `value_1_core` is the same port "
                        "pinned to one BLAS thread (faster here: the port is memory-bound and oversubscribed threads hurt), "
                        "`best_effort_blas3_value` the O(B D^2) batched formulation the kernels implement.  All three are "
                        "reported; the GPU/CPU ratio is a reported baseline, not the optimisation target",
            "fit_iterations_per_s": fit_cpu,
            "value_1_core": one_core, "best_effort_blas3_value": nb / tb,
            "cpu_jax": "unavailable (jax/jaxlib are not installed on this image and there is no network; the "
                       "numpy port stands in for the north star's CPU-JAX baseline)"}


def _marginal_rate(run, n, timed=None):
    """marginal iterations/s from fits of n and 3n iterations (fixed costs cancel), after a full-length warm-up fit (lazy
    library initialisation inside the first long fit would inflate t(n) and with it the rate); best of two each.
    timed (a _TimedCallable, host scores): the callable's own time is taken from the SAME runs the rate is taken from
    (timed.marginal_fn_s = its marginal time per iteration), and "best" is the run with the least time OUTSIDE the callable:
    a many-threaded numpy GEMM swings between 0.9 and 2.7 ms per call from run to run, and a rate from one pair of runs minus a
    callable time from all of them once came out at 47 us per iteration for a 2.7 ms callable (overhead -2.7 ms)."""
    run(n - 1)
    ts, fs = {}, {}
    for k in (n, 3 * n):
        best = None
        for _ in range(2):
            torch.cuda.synchronize()
            f0 = timed.t if timed is not None else 0.0
            t0 = time.perf_counter()
            run(k - 1)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            ft = (timed.t - f0) if timed is not None else 0.0
            if best is None or t - ft < best[0] - best[1]:
                best = (t, ft)
        ts[k], fs[k] = best
    if timed is not None:
        timed.marginal_fn_s = (fs[3 * n] - fs[n]) / (2 * n)
    return 2 * n / (ts[3 * n] - ts[n])


class _TimedCallable:
    """wraps a host score callable and accumulates the time spent inside it"""

    def __init__(self, fn):
        self.fn, self.t, self.calls = fn, 0.0, 0

    def __call__(self, x):
        t0 = time.perf_counter()
        r = self.fn(x)
        self.t += time.perf_counter() - t0
        self.calls += 1
        return r


def callpath_rates(D, B, methods=("auto",), n_fast=300, n_host=60, loop_variant=False):
    """Fit-iteration rates through the DROP-IN call path (round-4 verdict, item 4): the score callables a user of the reference
    brings, beside the built-in device score every other rate uses.
      native                    GaussianTarget.lp_g (device kernel)
      host_lp_g                 a numpy callable as examples/example_gsm_numpy.py:24-29 (vectorised over the rows): samples go
                                device -> host and scores host -> device every iteration (gsm_numpy.py:117)
      autograd_lp_g             score_from_logp of a torch log-density (examples/example_gsm.py:34-35: jit(grad(sum lp)))
      autograd_lp_g_graph_safe  the same, marked capturable: forward + backward replay inside the fit's hipGraph blocks
      *_diag_target             a target with DIAGONAL precision, whose host score is an elementwise product: there the engine's
                                own share of a host iteration is not buried under numpy's GEMM (0.2 - 3 ms per call at c3)
    host_fn_us = mean time inside the host callable during the timed fits; overhead_us = iteration_us - host_fn_us -
    iteration_us of the native score on the same target."""
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    dev = eng.device
    g = torch.Generator(device=dev)
    g.manual_seed(100)
    kw = dict(dtype=torch.float64, device=dev, generator=g)
    m = torch.rand(D, **kw)
    L = torch.randn(D, D, **kw)
    cov = L @ L.T + 1e-3 * torch.eye(D, dtype=torch.float64, device=dev)
    P = torch.linalg.inv(cov)
    P = (0.5 * (P + P.T)).contiguous()
    mh, Ph = m.cpu().numpy(), P.cpu().numpy()
    tgt = gsmvi_amd.GaussianTarget(mh, precision=Ph)
    pdh = (0.5 + torch.rand(D, **kw)).cpu().numpy()
    tgt_d = gsmvi_amd.GaussianTarget(mh, precision=np.diag(pdh))

    def host_lp_g(x):                                   # examples/example_gsm_numpy.py:24-29, vectorised over the rows
        assert len(x.shape) == 2
        return -(x - mh) @ Ph

    def host_lp_g_loop(x):                              # the example's literal per-row loop
        assert len(x.shape) == 2
        return np.array([-1.0 * np.dot(Ph, x[i] - mh) for i in range(x.shape[0])])

    def host_lp_g_diag(x):
        assert len(x.shape) == 2
        return -(x - mh) * pdh

    def logp(x):                                        # torch log-density, one value per row
        r = x - m
        return -0.5 * ((r @ P) * r).sum(-1)

    spin = {"s": 0.0}

    @gsmvi_amd.device_score
    def native_behind_an_idle_gap(x):
        """the built-in device score behind a host synchronisation and a busy wait as long as the numpy score takes: the GPU
        sits idle for that long every iteration, exactly as it does while a host callable runs -- what is left of the host
        path's overhead here is the price of the idle gap (clocks, wake-up), not of the engine's round trip"""
        torch.cuda.current_stream().synchronize()
        t_end = time.perf_counter() + spin["s"]
        while time.perf_counter() < t_end:
            pass
        return tgt.lp_g(x)

    scores = {"native": (tgt, tgt.lp_g), "host_lp_g": (tgt, host_lp_g), "native_behind_an_idle_gap": (tgt, native_behind_an_idle_gap),
              "autograd_lp_g": (tgt, gsmvi_amd.score_from_logp(logp)),
              "autograd_lp_g_graph_safe": (tgt, gsmvi_amd.score_from_logp(logp, graph_safe=True)),
              "native_diag_target": (tgt_d, tgt_d.lp_g), "host_lp_g_diag_target": (tgt_d, host_lp_g_diag)}
    if loop_variant:
        scores["host_lp_g_loop"] = (tgt, host_lp_g_loop)
    # (round 6) the same numpy score with the BLAS pool limited: the worker threads of a many-threaded GEMM keep spinning after it
    # returns and compete with the host side of the NEXT iteration's launches and synchronisation -- the engine's own share
    # (d2h_and_sync - device time) shows up only when they do not
    blas_limits = {}
    try:
        import threadpoolctl
        for nthr in (1, 8):
            scores[f"host_lp_g_blas_{nthr}_threads"] = (tgt, host_lp_g)
            blas_limits[f"host_lp_g_blas_{nthr}_threads"] = nthr
    except ImportError:
        threadpoolctl = None
    ent = {"D": D, "B": B}
    for method in methods:
        r = {}
        for sname, (tg, fn) in scores.items():
            host = sname.startswith("host")
            f = _TimedCallable(fn) if host else fn
            if sname == "native_behind_an_idle_gap":
                if "host_fn_us" not in r.get("host_lp_g", {}):
                    continue
                spin["s"] = r["host_lp_g"]["host_fn_us"] * 1e-6
            eng.host_score_profile = {} if host else None
            gsm = gsmvi_amd.GSM(D, tg.lp, f)
            n = n_fast if method != "dense" else max(50, n_fast // 2)
            if sname == "host_lp_g" and D >= 1024:
                n = n_host
            fkw = {"graph": True} if (sname.endswith("graph_safe") and method != "dense") else {}
            if sname.startswith("host_lp_g_blas"):
                n = n_host
            try:
                if sname in blas_limits:
                    with threadpoolctl.threadpool_limits(limits=blas_limits[sname], user_api="blas"):
                        rate = _marginal_rate(lambda k: gsm.fit(1, niter=k, batch_size=B, verbose=False, method=method, **fkw), n,
                                              timed=f if host else None)
                else:
                    rate = _marginal_rate(lambda k: gsm.fit(1, niter=k, batch_size=B, verbose=False, method=method, **fkw), n,
                                          timed=f if host else None)
            except Exception as e:                      # reported, never hidden
                r[sname] = {"error": f"{type(e).__name__}: {e}"[:200]}
                continue
            r[sname] = {"it_per_s": rate, "iteration_us": 1e6 / rate}
            if host:
                r[sname]["host_fn_us"] = f.marginal_fn_s * 1e6        # (the runs the rate comes from: see _marginal_rate)
                r[sname]["host_fn_us_all_runs"] = f.t / max(f.calls, 1) * 1e6
                pr, eng.host_score_profile = eng.host_score_profile, None
                nc = max(pr.get("calls", 0), 1)
                # (round-5 verdict, item 7) the engine's round trip in three lines, all fits of the rate measurement included:
                # device -> host copy + the ONE stream synchronisation (it also waits for the device's share of the iteration
                # in front of the copy), the callable as timed INSIDE the loop, staging memcpy + host -> device enqueue
                r[sname]["breakdown_us"] = {"d2h_and_sync": pr.get("d2h_and_sync_s", 0.0) / nc * 1e6,
                                            "callable_in_loop": pr.get("callable_s", 0.0) / nc * 1e6,
                                            "stage_and_h2d_enqueue": pr.get("stage_and_h2d_enqueue_s", 0.0) / nc * 1e6}
            if sname == "native_behind_an_idle_gap":
                r[sname]["idle_gap_us"] = spin["s"] * 1e6
            if fkw:
                r[sname]["graph_replays"] = int(getattr(gsm, "graph_replays", 0))
        for sname, v in r.items():
            base = r.get("native_diag_target" if sname.endswith("diag_target") else "native", {}).get("iteration_us")
            if "iteration_us" not in v or base is None or (sname.startswith("native") and sname != "native_behind_an_idle_gap"):
                continue
            v["overhead_us"] = v["iteration_us"] - v.get("host_fn_us", v.get("idle_gap_us", 0.0)) - base
        ent[method] = r
    return ent


def launch_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves as a CHILD torch.distributed.run
    (never an exec of this process, and before this process has made any GPU call) and relay rank 0's JSON line."""
    import socket
    import subprocess
    ndev = torch.cuda.device_count()             # counting devices does not initialise the GPU
    if ndev < n:
        sys.stderr.write(f"bench.py: --gpus {n} requested but only {ndev} GPU(s) are visible; refusing to report a "
                         f"{n}-GPU number from fewer devices\n")
        sys.exit(2)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    for ln in p.stdout.splitlines():
        if not lines or ln != lines[-1]:
            sys.stderr.write(ln + "\n")           # whatever else the ranks printed
    if p.returncode != 0 or not lines:
        sys.stderr.write(f"bench.py: the {n}-rank run failed (exit code {p.returncode}, "
                         f"{'no' if not lines else 'a'} JSON line)\n")
        sys.exit(p.returncode or 1)
    print(lines[-1], flush=True)
    sys.exit(0)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        launch_ranks(args.gpus)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # before the first HIP call: dmabuf IPC for RCCL
    assert torch.cuda.is_available(), "bench.py needs a GPU (there is no CPU fallback)"
    torch.cuda.set_device(local_rank)
    use_dist = world > 1 or bool(os.environ.get("GSMVI_BENCH_FORCE_DIST"))   # the env knob exercises RCCL at N=1
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("NCCL_DEBUG", "WARN")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"

    import gsmvi_amd
    from gsmvi_amd.dist import sharded_gsm_update, shard_bounds, row_sharded_gsm_update, row_bounds
    eng = gsmvi_amd.get_engine(local_rank)
    for kv in args.tune:
        k, v = kv.split("=")
        eng.set_tuning(k, int(v))
    D, B = args.D, args.B
    per_inst = 2 * D * D * 8
    n_inst = args.instances or max(2, int(np.ceil(320 * 2 ** 20 / per_inst)) + 1)
    inst, m, P = make_instances(eng, D, B, n_inst)
    lo, hi = shard_bounds(B, world, rank)
    rec_all = eng.empty(B, eng.record_len(D)) if use_dist else None
    rows = use_dist and args.shard == "rows"
    if rows:                                 # every rank keeps only its row block of each covariance
        rlo, rhi = row_bounds(D, world, rank)
        for it in inst:
            it["S0r"] = it["S0"][rlo:rhi].contiguous()
            it["Sr"] = eng.empty(rhi - rlo, D)

    def step(k):
        it = inst[k % n_inst]
        if not use_dist:
            eng.gsm_update(it["X"], it["G"], it["mu0"], it["S0"], out=(it["mu"], it["S"]))
        elif rows:
            row_sharded_gsm_update(eng, it["X"], it["G"], it["mu0"], it["S0r"], out=(it["mu"], it["Sr"]))
        else:
            sharded_gsm_update(eng, it["X"][lo:hi], it["G"][lo:hi], it["mu0"], it["S0"], rec_all=rec_all,
                               out=(it["mu"], it["S"]), force_collective=True)

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- hipGraphs of the timed sequence (with RCCL: the all-gather is captured too).  The timed region is
    # `steps // gsize` replays of a graph of gsize = min(ring, steps) consecutive ring positions plus ONE replay
    # of a second graph holding the `steps % gsize` left over, so every timed step runs in the launch mode the
    # JSON line names, for any --steps.
    gsize = max(1, min(n_inst, args.steps))
    n_full, n_rem = args.steps // gsize, args.steps % gsize
    graph, graph_rem, launch = None, None, "eager"

    def capture(first, count):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for k in range(first, first + count):
                step(k)
        return g

    if not args.no_graph:
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for k in range(n_inst):
                    step(k)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = capture(0, gsize)
            if n_rem:
                graph_rem = capture(n_full * gsize, n_rem)
            launch = f"hipGraph({n_full} x {gsize} updates/replay" + (f" + 1 x {n_rem}" if n_rem else "") + ")"
        except Exception as e:           # capture unsupported -> stay on eager launches of the same kernels
            graph, graph_rem, launch = None, None, f"eager (graph capture failed: {type(e).__name__})"
            torch.cuda.synchronize()
        if use_dist:                     # every rank must take the same path
            ok = torch.tensor([1 if graph is not None else 0], device="cuda")
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok.item()) == 0:
                graph, graph_rem, launch = None, None, "eager (graph capture failed on some rank)"

    replay_ev = []                       # one torch event pair per full replay: median / min per step

    def run_timed():
        if graph is not None:
            for _ in range(n_full):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graph.replay()
                e1.record()
                replay_ev.append((e0, e1))
            if graph_rem is not None:
                graph_rem.replay()
        else:
            for k in range(args.steps):
                step(k)

    def run_warmup():
        """At least --warmup steps, in the timed region's own launch mode (whole replays, >= 1 of each graph)."""
        if graph is not None:
            for _ in range(max(1, -(-args.warmup // gsize))):
                graph.replay()
            if graph_rem is not None:
                graph_rem.replay()
            return max(1, -(-args.warmup // gsize)) * gsize + n_rem
        for k in range(args.warmup):
            step(k)
        return args.warmup

    warm_done = run_warmup()
    barrier()
    t0 = time.perf_counter()
    run_timed()
    barrier()
    el = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([el], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    ms_per_step = el / args.steps * 1e3
    value = args.steps / el
    # what the last timed step computed, before anything else writes to the instances (every step writes its own ring
    # position's outputs from fixed inputs, so the last step's position holds exactly that step's result)
    if args.dump_outputs and rank == 0:
        last = inst[(args.steps - 1) % n_inst]
        dump_outputs(args.dump_outputs, [("mu", last["mu"]), ("S_row_block", last["Sr"]) if rows else ("S", last["S"])])
    # statistics of the per-step device time need more than the one or two replays a small --steps gives: top the sample up
    # to >= 30 full replays OUTSIDE the timed region (`value`, `ms_per_step` and `steps` keep their contract meaning)
    if args.full and graph is not None and len(replay_ev) < 30:
        for _ in range(30 - len(replay_ev)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            replay_ev.append((e0, e1))
        torch.cuda.synchronize()
    per_replay_us = sorted(e0.elapsed_time(e1) * 1e3 / gsize for e0, e1 in replay_ev) if args.full and replay_ev else []
    step_us_stats = ({"median": per_replay_us[len(per_replay_us) // 2], "min": per_replay_us[0], "max": per_replay_us[-1],
                      "replays": len(per_replay_us), "replays_inside_timed_region": n_full if graph is not None else 0,
                      "note": "device time of each full graph replay / updates per replay (torch events on the replay "
                              "stream; topped up to >= 30 replays after the timed region); `value` itself is wall clock "
                              "over the timed steps only"}
                     if per_replay_us else None)

    # ---- opt-in: several independent updates in flight (throughput of independent chains, not of one fit) -----
    value_in_flight = None
    if args.in_flight > 1:
        from gsmvi_amd.engine import HipEngine
        nl = args.in_flight
        engs = [eng] + [HipEngine(local_rank) for _ in range(nl - 1)]        # one context (workspace) per stream
        recs = [rec_all] + [eng.empty(B, eng.record_len(D)) if use_dist else None for _ in range(nl - 1)]
        lanes = [torch.cuda.Stream() for _ in range(nl)]

        def lane_step(k, ln):
            it = inst[k % n_inst]
            if not use_dist:
                engs[ln].gsm_update(it["X"], it["G"], it["mu0"], it["S0"], out=(it["mu"], it["S"]))
            elif rows:
                row_sharded_gsm_update(engs[ln], it["X"], it["G"], it["mu0"], it["S0r"], out=(it["mu"], it["Sr"]))
            else:
                sharded_gsm_update(engs[ln], it["X"][lo:hi], it["G"][lo:hi], it["mu0"], it["S0"], rec_all=recs[ln],
                                   out=(it["mu"], it["S"]), force_collective=True)

        def issue():
            cur = torch.cuda.current_stream()
            for sl in lanes:
                sl.wait_stream(cur)
            for k in range(n_inst):
                with torch.cuda.stream(lanes[k % nl]):
                    lane_step(k, k % nl)
            for sl in lanes:
                cur.wait_stream(sl)

        issue()
        torch.cuda.synchronize()
        gfl = None
        if not args.no_graph:
            try:
                gfl = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gfl):
                    issue()
            except Exception:
                gfl = None
                torch.cuda.synchronize()
        if use_dist:
            okf = torch.tensor([1 if gfl is not None else 0], device="cuda")
            dist.all_reduce(okf, op=dist.ReduceOp.MIN)
            if int(okf.item()) == 0:
                gfl = None
        reps = max(1, args.steps // n_inst)
        for _ in range(2):
            gfl.replay() if gfl is not None else issue()
        barrier()
        tf0 = time.perf_counter()
        for _ in range(reps):
            gfl.replay() if gfl is not None else issue()
        barrier()
        elf = time.perf_counter() - tf0
        if use_dist:
            tt = torch.tensor([elf], dtype=torch.float64, device="cuda")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            elf = float(tt.item())
        value_in_flight = {"updates_per_s": reps * n_inst / elf, "in_flight": nl,
                           "launch": "hipGraph" if gfl is not None else "eager"}

    # ---- cache-resident rate: one instance, what a fit loop with a single covariance sees ------
    value_hot = None
    if args.full and not use_dist:
        it = inst[0]
        g1 = None
        try:
            if graph is not None:
                g1 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g1):
                    for _ in range(n_inst):
                        eng.gsm_update(it["X"], it["G"], it["mu0"], it["S0"], out=(it["mu"], it["S"]))
        except Exception:
            g1 = None
        reps = max(1, args.steps // n_inst)
        for _ in range(3):
            g1.replay() if g1 is not None else [step(0) for _ in range(n_inst)]
        torch.cuda.synchronize()
        th = time.perf_counter()
        for _ in range(reps):
            if g1 is not None:
                g1.replay()
            else:
                for _ in range(n_inst):
                    eng.gsm_update(it["X"], it["G"], it["mu0"], it["S0"], out=(it["mu"], it["S"]))
        torch.cuda.synchronize()
        value_hot = reps * n_inst / (time.perf_counter() - th)

    roofline = None
    if args.full:
        # ---- roofline of the dominant kernel (covariance update), dispatch-timestamp events --------
        # Each sample is the LAST of four back-to-back updates on consecutive (HBM-cold) instances: the durations are the kernels'
        # durations with the device busy, as in the timed region.  (Round 5: a sample per update timed from an idle device --
        # launch, read the events, launch -- read 10.8 us for the 6.3 us covariance kernel on one MI355X, whose clocks
        # drop between the synchronisations, while the replayed region and rocprofv3 of the same run were unchanged.)
        eng.set_profiling(True)
        kt = {"panel": [], "scalars": [], "cov_update": []}
        for k in range(2 * n_inst):
            for q in range(4):
                it = inst[(4 * k + q) % n_inst]
                eng.gsm_update(it["X"], it["G"], it["mu0"], it["S0"], out=(it["mu"], it["S"]))
            pr = eng.get_profile()
            if k >= n_inst // 2:
                for key in kt:
                    kt[key].append(pr[key])
        eng.set_profiling(False)
        avg_ms = {k: float(np.mean(v)) for k, v in kt.items()}
        alg_bytes_update = 16.0 * D * D + 16.0 * B * D                     # pass B
        alg_bytes_total = 24.0 * D * D + 72.0 * B * D                      # whole update
        achieved = alg_bytes_update / (avg_ms["cov_update"] * 1e-3) / 1e9
        traffic, mfma_util = None, None
        tpath = os.path.join(ROOT, "profiles", "traffic.json")
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                traffic = tj.get("k_gsm_cov_update_bytes_per_launch")
                mfma_util = next((v.get("util") for k, v in (tj.get("mfma_util") or {}).items() if "k_gsm_cov_sym" in k), None)
            except Exception:
                traffic = None
        # (round-5 verdict, item 8) the same kernel's average under `rocprofv3 --kernel-trace --stats` of this command, read from the
        # TRACKED summary of the latest published pass (profiles/rNN/kernel_stats.csv, scripts/collect_profiles.sh at the headline
        # shape): `frac` is computed from it so that the line's figure follows from what profiles/ holds; the live dispatch events
        # stay beside it.  Another shape than the profiled one: events only.
        rocprof_us, rocprof_src = None, None
        if (D, B) == (1024, 32):
            import csv as _csv
            import glob as _glob
            for ks in sorted(_glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]", "kernel_stats.csv")), reverse=True):
                try:
                    rows = [r for r in _csv.DictReader(open(ks)) if "k_gsm_cov_sym<" in r["Name"]]
                    if rows:
                        r = max(rows, key=lambda r_: int(r_["Calls"]))
                        rocprof_us, rocprof_src = float(r["AverageNs"]) / 1e3, os.path.relpath(ks, ROOT)
                        rocprof_calls, rocprof_min = int(r["Calls"]), float(r["MinNs"]) / 1e3
                        break
                except Exception:
                    continue
        sym = D % 2 == 0
        # bytes the selected kernel really moves: the symmetric kernel reads only the upper triangle of S0
        # (4 D^2 + the diagonal tiles) and writes all of S (8 D^2); the generic one reads and writes 8 D^2 each
        nt32 = (D + 31) // 32
        moved = ((nt32 * (nt32 + 1) // 2) * 32 * 32 * 8.0 + 8.0 * D * D + 16.0 * B * D) if sym else alg_bytes_update
        roofline = {"bound": "hbm", "kernel": "k_gsm_cov_sym" if sym else "k_gsm_cov_update",
                    "achieved": achieved if rocprof_us is None else alg_bytes_update / (rocprof_us * 1e-6) / 1e9, "peak": HBM_PEAK_GBS,
                    "unit": "GB/s",
                    "frac": (achieved if rocprof_us is None else alg_bytes_update / (rocprof_us * 1e-6) / 1e9) / HBM_PEAK_GBS,
                    "frac_basis": "events (live dispatch events; no published rocprofv3 summary for this shape)" if rocprof_us is None
                    else f"rocprofv3 average of {rocprof_src} ({rocprof_calls} launches, min {rocprof_min:.2f} us)",
                    "avg_kernel_us_events": avg_ms["cov_update"] * 1e3, "avg_kernel_us_rocprof": rocprof_us,
                    "achieved_events": achieved, "frac_events": achieved / HBM_PEAK_GBS, "traffic": traffic,
                    "traffic_source": "profiles/traffic.json (rocprofv3 PMC pass of an earlier run of this command; "
                                      "not a live counter)",
                    "algorithmic_bytes_per_launch": alg_bytes_update,
                    "moved_bytes_per_launch": moved, "achieved_moved": moved / (avg_ms["cov_update"] * 1e-3) / 1e9,
                    "frac_moved": moved / (avg_ms["cov_update"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "avg_kernel_us": {k: v * 1e3 for k, v in avg_ms.items()},
                    "whole_update_algorithmic_GBs": alg_bytes_total * value / 1e9,
                    "whole_update_frac": alg_bytes_total * value / 1e9 / HBM_PEAK_GBS,   # all launches of one update
                    "whole_update_frac_cache_resident": (alg_bytes_total * value_hot / 1e9 / HBM_PEAK_GBS)
                    if value_hot else None,
                    "mfma_pipe_util_profiled": mfma_util}     # SQ_VALU_MFMA_BUSY_CYCLES pass, profiles/traffic.json
        # ---- calibration: the attainable HBM rate on this device (device copy of 1 GiB, read + write
        # bytes) and what a plain copy of one covariance costs in the same cold ring (it moves 16 D^2 bytes, the
        # covariance kernel's algorithmic count) -- torch's copy kernel, plumbing, not the product path.
        if rank == 0:
            try:
                # the yardstick is this library's OWN streaming copy (16 B per lane, non-temporal: gsmvi_debug_stream_copy_f64 of the
                # debug build -- calibration, not the product path; until round 3 torch's copy_ kernel stood here and read 5.0 TB/s
                # where MI355X_MICROARCH.md's float4 copy reaches 6.29); torch's figure is kept beside it
                import ctypes as _C
                from gsmvi_amd import _lib as _gl
                dbg = _C.CDLL(_gl.library_path(debug=True))
                dbg.gsmvi_debug_stream_copy_f64.restype = _C.c_int
                dbg.gsmvi_debug_stream_copy_f64.argtypes = [_C.c_void_p, _C.c_void_p, _C.c_void_p, _C.c_size_t]
                big = torch.empty(2, 2 ** 27, dtype=torch.float64, device=eng.device)
                big[0].fill_(1.0)
                st_ = _C.c_void_p(torch.cuda.current_stream().cuda_stream)

                def own_copy():
                    rc_ = dbg.gsmvi_debug_stream_copy_f64(st_, _C.c_void_p(big[1].data_ptr()), _C.c_void_p(big[0].data_ptr()),
                                                          big[0].numel())
                    assert rc_ == 0

                rates = {}
                for name, fn in (("own", own_copy), ("torch", lambda: big[1].copy_(big[0]))):
                    for _ in range(2):
                        fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(5):
                        fn()
                    e1.record()
                    e1.synchronize()
                    rates[name] = 5 * 2.0 * big[0].numel() * 8 / (e0.elapsed_time(e1) * 1e-3) / 1e9
                assert torch.equal(big[1], big[0])
                attain = max(rates.values())
                roofline["attainable_peak_by_kernel"] = rates
                del big
                gcp = torch.cuda.CUDAGraph()
                for it in inst:
                    it["S"].copy_(it["S0"])
                torch.cuda.synchronize()
                with torch.cuda.graph(gcp):
                    for it in inst:
                        it["S"].copy_(it["S0"])
                gcp.replay()
                torch.cuda.synchronize()
                tc0 = time.perf_counter()
                for _ in range(20):
                    gcp.replay()
                torch.cuda.synchronize()
                copy_us = (time.perf_counter() - tc0) / (20 * n_inst) * 1e6
                roofline["attainable_peak"] = attain
                # moved bytes against a moved-bytes copy rate (round-4 verdict: the former algorithmic / moved ratio could exceed 1)
                roofline["frac_of_attainable_moved"] = roofline["achieved_moved"] / attain
                roofline["plain_copy_same_size_us"] = copy_us
            except Exception as e:                  # calibration only
                roofline["attainable_peak"] = f"failed: {type(e).__name__}"

        # ---- the same kernel where it is bandwidth- rather than latency-bound: D=4096, B=32, measured live (two cold
        # instances, hipExt dispatch events; rocprofv3 evidence: profiles/r02/d4096_b32_kernel_stats.csv) ----
        if rank == 0 and not use_dist and D == 1024 and not args.no_large_point:
            try:
                DL, BL = 4096, 32
                li, _, _ = make_instances(eng, DL, BL, 3, seed0=7)
                eng.set_profiling(True)
                tl = []
                for kk in range(12):
                    for q in range(3):                   # (the last of three back-to-back updates: device busy, see above)
                        it = li[(3 * kk + q) % 3]
                        eng.gsm_update(it["X"], it["G"], it["mu0"], it["S0"], out=(it["mu"], it["S"]))
                    if kk >= 3:
                        tl.append(eng.get_profile()["cov_update"])
                eng.set_profiling(False)
                tms = float(np.mean(tl))
                bl = 16.0 * DL * DL + 16.0 * BL * DL
                roofline["large_D_point"] = {"D": DL, "B": BL, "kernel": "k_gsm_cov_sym_p (persistent form of k_gsm_cov_sym)",
                                             "avg_kernel_us": tms * 1e3,
                                             "algorithmic_bytes_per_launch": bl, "achieved": bl / (tms * 1e-3) / 1e9,
                                             "frac": bl / (tms * 1e-3) / 1e9 / HBM_PEAK_GBS}
                ntl = DL // 32
                mvl = (ntl * (ntl + 1) // 2) * 32 * 32 * 8.0 + 8.0 * DL * DL + 16.0 * BL * DL      # upper triangle read, all of S written
                roofline["large_D_point"]["moved_bytes_per_launch"] = mvl
                roofline["large_D_point"]["achieved_moved"] = mvl / (tms * 1e-3) / 1e9
                if isinstance(roofline.get("attainable_peak"), float):
                    roofline["large_D_point"]["frac_of_attainable_moved"] = mvl / (tms * 1e-3) / 1e9 / roofline["attainable_peak"]
                del li
                torch.cuda.empty_cache()
            except Exception as e:                  # secondary figure only
                roofline["large_D_point"] = f"failed: {type(e).__name__}: {e}"

    # ---- fit-iteration rate F: sample -> score -> update -> Cholesky PD check -> commit ----
    fit_rate = None
    if args.full and not use_dist:
        fit_rate = {}
        tgt = gsmvi_amd.GaussianTarget(m.cpu().numpy(), precision=P.cpu().numpy())
        for method in ("dense", "factor", "auto"):
            try:
                gsm = gsmvi_amd.GSM(D, tgt.lp, tgt.lp_g)
                gsm.fit(1, niter=10, batch_size=B, verbose=False, rng="device", method=method)
                torch.cuda.synchronize()
                tf0 = time.perf_counter()
                nf = 150 if (method == "dense" or D > 1024) else 600     # enough iterations to amortise the one-off setup
                gsm.fit(1, niter=nf - 1, batch_size=B, verbose=False, rng="device", method=method)
                torch.cuda.synchronize()
                fit_rate[method] = nf / (time.perf_counter() - tf0)
            except Exception as e:      # reported, never hidden
                fit_rate[method] = f"failed: {type(e).__name__}: {e}"

    # ---- BASELINE config 4 beside the headline (round 6): BaM.fit at DEFAULT arguments (the reference's jitter => its own loop,
    # update + jitter + Cholesky accept test), D = 1024, B = 128, reg = 100 / (1 + i) (examples/example_bam.py:58); and the Cholesky
    # alone, the accept test of every reference-faithful loop ----
    if fit_rate is not None and rank == 0 and D == 1024 and not args.no_large_point:
        try:
            bam = gsmvi_amd.BaM(D, tgt.lp, tgt.lp_g)
            sched = lambda i: 100.0 / (1 + i)                                       # noqa: E731
            bam.fit(1, sched, niter=5, batch_size=128, verbose=False)
            torch.cuda.synchronize()
            tb0 = time.perf_counter()
            bam.fit(1, sched, niter=149, batch_size=128, verbose=False)
            torch.cuda.synchronize()
            fit_rate["bam_c4_default_args"] = {"it_per_s": 150 / (time.perf_counter() - tb0), "method_used": bam.method_used,
                                               "n_reverts": int(bam.n_reverts)}
            Sx, Rx, fx = inst[0]["S0"], eng.empty(D, D), eng.new_flag()
            for _ in range(3):
                eng.potrf(Sx, out=Rx, flag=fx)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                eng.potrf(Sx, out=Rx, flag=fx)
            e1.record()
            e1.synchronize()
            fit_rate["potrf_us"] = e0.elapsed_time(e1) * 1e2
        except Exception as e:                  # secondary figures only
            fit_rate["bam_c4_default_args"] = f"failed: {type(e).__name__}: {e}"

    # ---- the drop-in call path: host numpy score and torch-autograd score (round-4 verdict, item 4), c3 (this shape) and c2 ----
    if fit_rate is not None and rank == 0 and not args.no_callpath:
        try:
            cp = {"here": callpath_rates(D, B, methods=("auto",), n_fast=200, n_host=40)}
            if (D, B) != (256, 8):
                cp["c2"] = callpath_rates(256, 8, methods=("auto",), n_fast=300)
            for key in ("host_lp_g", "autograd_lp_g", "autograd_lp_g_graph_safe", "host_lp_g_diag_target"):
                v = cp["here"]["auto"].get(key, {})
                fit_rate[key] = v.get("it_per_s", v.get("error"))
            fit_rate["call_path"] = cp
        except Exception as e:                  # reported, never hidden
            fit_rate["call_path"] = f"failed: {type(e).__name__}: {e}"

    # roofline of the DEFAULT fit iteration (factor form): F is streamed four times and written once per iteration --
    # sampler 8 D^2, score 8 D^2 (the precision matrix), W = G F^T 8 D^2, V F 8 D^2, update 16 D^2 = 48 D^2 bytes
    fit_roofline = None
    if fit_rate and isinstance(fit_rate.get("factor"), float):
        fb = 48.0 * D * D
        fit_roofline = {"bound": "hbm", "algorithmic_bytes_per_iteration": fb, "iteration_us": 1e6 / fit_rate["factor"],
                        "achieved": fb * fit_rate["factor"] / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": fb * fit_rate["factor"] / 1e9 / HBM_PEAK_GBS,
                        "note": "whole iteration of GSM.fit(method='factor'), eager launches from Python, built-in Gaussian target"}
    out = {"metric": "GSM updates/sec at D=%d,B=%d (dense-cov gsm_update, fp64)" % (D, B),
           "value": value, "unit": "updates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "f64", "data": "synthetic",
           "config": {"workload": (("BASELINE configs[2]: " if (D, B) == (1024, 32) else
                                    "BASELINE configs[1]: " if (D, B) == (256, 8) else "not a BASELINE config: ") +
                                   f"D={D} dense-cov Gaussian target, B={B}, one GSM update per step"),
                      "D": D, "B": B, "instances": n_inst,
                      "ring_bytes": n_inst * per_inst, "launch": launch, "warmup_steps_run": warm_done,
                      "parallelism": "single GPU" if not use_dist else
                      (f"covariance row blocks x{world} + RCCL all-gather of SG column slices" if rows else
                       f"batch-sharded x{world} + RCCL all-gather")}}
    if args.full:
        out.update({"step_us": step_us_stats, "value_cache_resident": value_hot, "fit_iterations_per_s": fit_rate,
                    "fit_roofline": fit_roofline, "roofline": roofline})
    if value_in_flight is not None:
        out["value_in_flight"] = value_in_flight
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(D, B, args.cpu_seconds)
    if use_dist:
        dist.destroy_process_group()
    if rank == 0:
        try:                                   # RCCL prints a banner through C stdio: get it out first
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(json.dumps(out), flush=True)     # the ONE JSON line, last on stdout


if __name__ == "__main__":
    main()
