"""Batched GLM target benchmark (BatchedGLMTarget, gsmvi_glm_batched_f64 in csrc/gsmvi_logistic_batched.hip): the score call of
every family against the same score written as torch ops, and the logistic entry point against the library of another commit.

Writes one JSON object with
  calls[]   at K = 8192 x (N, D, B) in {(64, 10, 2), (256, 16, 8), (1024, 64, 8)}, per family, with an offset and without,
            all through gsmvi_glm_batched_f64: the score call alone, the HIP launch (hip_ms) and
            the torch expression (torch_ms: torch.baddbmm for eta, the link in its stable torch form, torch.baddbmm back),
            alternated in one process; per call one pair of device events, --reps (>= 30) calls after a warm-up, median and
            range; ratio = torch median / hip median (acceptance: > 1.0 for every new family).  logistic_entry_ms: the same
            logistic data through gsmvi_logistic_batched_f64, in the same alternation; link_cost = hip median / that median.
            Also lp_ms and both_ms of the family.
  parent[]  with --parent-lib FILE (libgsmvi_hip.so built from the parent commit, loaded beside this tree's library): at the
            same shapes gsmvi_logistic_batched_f64 of both libraries through the same ctypes call on the same device arrays,
            alternated call by call, in two passes over the three shapes (the two passes of a shape are separate loops on
            fresh allocations with the other shapes' work between them): the medians of each of the four series
            (parent_ms_pass1 / 2, new_ms_pass1 / 2) and of each library's two series pooled (parent_ms, new_ms); spread =
            |pass1 - pass2| of the parent's medians, its own run-to-run spread; slower_by = new_ms - parent_ms (acceptance:
            <= spread); same_bits = the outputs are equal
Usage: python scripts/glm_batched_bench.py [--out FILE] [--reps R] [--quick] [--parent-lib FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gsmvi_amd  # noqa: E402
from gsmvi_amd import _lib  # noqa: E402

SHAPES = [(64, 10, 2), (256, 16, 8), (1024, 64, 8)]
K_BENCH = 8192
LAM, TAU = 0.5, 1.7
FAMILIES = ("logistic", "poisson", "probit", "gaussian")
# (family, with an offset): every family with and without (the logistic family without one is what its own entry point runs)
VARIANTS = [(f, o) for o in (False, True) for f in FAMILIES]


def problems(family, K, N, D, seed, offset=False):
    """K synthetic data sets on the device: A ~ N(0, 1) / sqrt(D), offsets 0.3 N(0, 1) if asked, y drawn from the family at
    theta* ~ N(0, 1)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)      # noqa: E731
    A = rn(K, N, D) / np.sqrt(D)
    o = 0.3 * rn(K, N) if offset else None
    eta = torch.bmm(A, rn(K, D, 1))[:, :, 0] + (0.0 if o is None else o)
    u = torch.rand(K, N, dtype=torch.float64, device="cuda", generator=g)
    if family == "logistic":
        y = (u < torch.sigmoid(eta)).double()
    elif family == "probit":
        y = (u < torch.special.ndtr(eta)).double()
    elif family == "poisson":
        y = torch.poisson(torch.exp(eta), generator=g)
    else:
        y = eta + rn(K, N) / np.sqrt(TAU)
    return A, y, o


def torch_score(family, A, y, o, lam, tau):
    """the same score as torch ops on the device, each link in the form a torch user would write to keep it finite"""
    At = A.transpose(1, 2)
    ob = None if o is None else o[:, None, :]
    yb = y[:, None, :]

    @gsmvi_amd.device_score
    def lp_g(x):
        eta = torch.bmm(x, At) if ob is None else torch.baddbmm(ob, x, At)
        if family == "logistic":
            e = torch.exp(-eta.abs())
            r = yb - torch.where(eta >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        elif family == "poisson":
            r = yb - torch.exp(eta)
        elif family == "probit":
            lphi = -0.5 * eta * eta - 0.9189385332046727
            r = yb * torch.exp(lphi - torch.special.log_ndtr(eta)) - (1.0 - yb) * torch.exp(lphi - torch.special.log_ndtr(-eta))
        else:
            r = tau * (yb - eta)
        return torch.baddbmm(x, r, A, beta=-lam)
    return lp_g


def _each(fns, reps):
    """per-call device-event times (ms) of the callables, alternated: {name: [ms] * reps}"""
    for _ in range(3):
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


def _stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def call_entries(K, N, D, B, reps):
    """one entry per family at this shape, all callables of the shape alternated in one loop"""
    eng = gsmvi_amd.get_engine()
    x = torch.randn(K, B, D, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    G, lpo = eng.empty(K, B, D), eng.empty(K, B)
    fns, errs, keep = {}, {}, []
    for fam, off in VARIANTS:
        A, y, o = problems(fam, K, N, D, 11, off)
        name = fam + ("+offset" if off else "")
        tau = TAU if fam == "gaussian" else 1.0
        tgt = gsmvi_amd.BatchedGLMTarget(A, y, fam, LAM, offset=o, noise_precision=tau)
        tscore = torch_score(fam, A, y, o, LAM, tau)
        ref = tscore(x)
        errs[name] = float((ref - tgt.lp_g(x)).abs().max() / ref.abs().max())
        assert errs[name] < 1e-9, (name, errs[name])
        fns[name + ":hip"] = lambda t=tgt: t.lp_g(x, out=G)
        fns[name + ":torch"] = lambda s=tscore: s(x)
        fns[name + ":lp"] = lambda t=tgt: t._call(x, lp_out=lpo, want="lp")
        fns[name + ":both"] = lambda t=tgt: t._call(x, out=G, lp_out=lpo, want="both")
        if name == "logistic":
            fns["logistic:entry"] = lambda t=tgt: eng.logistic_batched(x, t.A, t.y, None, LAM, out=G, want="g")
        keep.append((tgt, tscore))
    t = _each(fns, reps)
    base = float(np.median(t["logistic:entry"]))
    out = []
    for fam, off in VARIANTS:
        name = fam + ("+offset" if off else "")
        e = {"family": fam, "K": K, "N": N, "D": D, "B": B, "reps": reps, "offset": off,
             "hip_ms": _stats(t[name + ":hip"]), "torch_ms": _stats(t[name + ":torch"]), "lp_ms": _stats(t[name + ":lp"]),
             "both_ms": _stats(t[name + ":both"]), "max_rel_diff_vs_torch": errs[name]}
        e["ratio"] = e["torch_ms"]["median"] / e["hip_ms"]["median"]
        e["link_cost"] = e["hip_ms"]["median"] / base
        if name == "logistic":
            e["logistic_entry_ms"] = _stats(t["logistic:entry"])
        out.append(e)
    return out


class OtherLibrary:
    """gsmvi_logistic_batched_f64 of one build of the library (with a context of its own), called through plain ctypes"""

    def __init__(self, path, device):
        self.lib = C.CDLL(path)                                         # RTLD_LOCAL: its symbols stay its own
        res, args = _lib._SIGS["gsmvi_logistic_batched_f64"]
        self.fn = self.lib.gsmvi_logistic_batched_f64
        self.fn.restype, self.fn.argtypes = res, args
        self.lib.gsmvi_create.restype, self.lib.gsmvi_create.argtypes = _lib._SIGS["gsmvi_create"]
        self.lib.gsmvi_destroy.restype, self.lib.gsmvi_destroy.argtypes = _lib._SIGS["gsmvi_destroy"]
        self.ctx = C.c_void_p()
        assert self.lib.gsmvi_create(C.byref(self.ctx), device, 64, 32) == 0

    def score(self, K, D, nc, N, A, y, lam, X, G):
        st = self.fn(self.ctx, C.c_void_p(torch.cuda.current_stream().cuda_stream), K, D, nc, N, C.c_void_p(A.data_ptr()),
                     C.c_void_p(y.data_ptr()), None, lam, None, C.c_void_p(X.data_ptr()), C.c_void_p(G.data_ptr()), None)
        assert st == 0, st

    def close(self):
        torch.cuda.synchronize()
        self.lib.gsmvi_destroy(self.ctx)


def parent_pass(new, other, K, N, D, B, reps):
    """one pass: both libraries on fresh copies of the same data, alternated call by call; the two series and whether the
    outputs are equal"""
    eng = gsmvi_amd.get_engine()
    A, y, _ = problems("logistic", K, N, D, 11)
    x = torch.randn(K, B, D, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    Gn, Gp = eng.empty(K, B, D), eng.empty(K, B, D)
    fn = lambda: new.score(K, D, B, N, A, y, LAM, x, Gn)                                   # noqa: E731  the same call path
    fo = lambda: other.score(K, D, B, N, A, y, LAM, x, Gp)                                 # noqa: E731  for both libraries
    t = _each({"parent": fo, "new": fn}, reps)
    torch.cuda.synchronize()
    return t["parent"], t["new"], bool(torch.equal(Gn, Gp))


def parent_entries(new, other, K, reps):
    """two passes over the three shapes (so the two passes of a shape are minutes of other work apart)"""
    got = {s: [] for s in SHAPES}
    for _ in range(2):
        for s in SHAPES:
            got[s].append(parent_pass(new, other, K, *s, reps))
    out = []
    for (N, D, B), ((p1, n1, b1), (p2, n2, b2)) in got.items():
        e = {"K": K, "N": N, "D": D, "B": B, "reps": reps, "parent_ms_pass1": _stats(p1), "parent_ms_pass2": _stats(p2),
             "new_ms_pass1": _stats(n1), "new_ms_pass2": _stats(n2), "same_bits": b1 and b2}
        e["parent_ms"], e["new_ms"] = float(np.median(p1 + p2)), float(np.median(n1 + n2))
        e["spread"] = abs(e["parent_ms_pass1"]["median"] - e["parent_ms_pass2"]["median"])
        e["slower_by"] = e["new_ms"] - e["parent_ms"]
        e["not_slower"] = bool(e["slower_by"] <= e["spread"])
        out.append(e)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--quick", action="store_true", help="few repetitions, K = 512")
    ap.add_argument("--parent-lib", default=None, help="libgsmvi_hip.so of the parent commit for the logistic A/B")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    reps = 5 if args.quick else max(args.reps, 30)
    K = 512 if args.quick else K_BENCH
    res = {"device": torch.cuda.get_device_name(0), "K": K, "prior_precision": LAM, "noise_precision": TAU, "calls": [],
           "parent": []}
    for N, D, B in SHAPES:
        for e in call_entries(K, N, D, B, reps):
            res["calls"].append(e)
            print(json.dumps(e), flush=True)
    if args.parent_lib:
        dev = torch.cuda.current_device()
        new, other = OtherLibrary(_lib.library_path(), dev), OtherLibrary(args.parent_lib, dev)
        for e in parent_entries(new, other, K, max(reps, 100) if not args.quick else reps):
            res["parent"].append(e)
            print(json.dumps(e), flush=True)
        new.close()
        other.close()
    res["new_families_beat_torch"] = all(e["ratio"] > 1.0 for e in res["calls"] if e["family"] != "logistic")
    res["logistic_not_slower_than_parent"] = all(e["not_slower"] for e in res["parent"]) if res["parent"] else None
    print(json.dumps({k: res[k] for k in ("new_families_beat_torch", "logistic_not_slower_than_parent")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
