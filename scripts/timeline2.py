#!/usr/bin/env python3
"""Diagnostic: timeline of ONE dense GSM update (all kernels) inside a replayed hipGraph, from in-kernel s_memrealtime stamps
(100 MHz, one clock for the whole chip).  usage: timeline2.py [cold|warm] [name=value tuning ...]"""
import os as _os; _os.environ.setdefault("GSMVI_HIP_DEBUG_LIB", "1")   # gsmvi_debug_* are exported by libgsmvi_hip_debug.so only
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, gsmvi_amd
from bench import make_instances
mode = sys.argv[1] if len(sys.argv) > 1 else "cold"
eng = gsmvi_amd.get_engine()
for kv in sys.argv[2:]:
    k, v = kv.split("=")
    eng.set_tuning(k, int(v))
D, B = 1024, 32
n_inst = 21 if mode == "cold" else 1
inst, m, P = make_instances(eng, D, B, n_inst)
eng.gsm_update(inst[0]["X"], inst[0]["G"], inst[0]["mu0"], inst[0]["S0"], out=(inst[0]["mu"], inst[0]["S"]))
eng.set_tuning("timeline", 1)
def step(k):
    it = inst[k % n_inst]
    eng.gsm_update(it["X"], it["G"], it["mu0"], it["S0"], out=(it["mu"], it["S"]))
for k in range(21): step(k)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    for k in range(21): step(k)
NW = 4 * 4096
names = {0: "panel", 1: "scalars", 2: "cov", 3: "k3"}
for trial in range(4):
    for _ in range(20): g.replay()
    torch.cuda.synchronize()
    buf = (C.c_ulonglong * NW)()
    eng.lib.gsmvi_debug_read_stamps(eng._ctx, buf, NW)
    st = np.array(buf, dtype=np.uint64).reshape(4, 512, 8).astype(np.int64)
    t0 = st[st > 0].min()
    print(f"--- trial {trial} ({mode}) ---")
    prev_end = None
    for k in range(4):
        a = st[k]
        live = a[:, 0] > 0
        if not live.any():
            continue
        a = a[live]
        us = np.where(a > 0, (a - t0) / 100.0, np.nan)
        cols = [c for c in range(8) if np.isfinite(us[:, c]).any()]
        s = f"{names[k]:8s} {live.sum():3d} WGs: "
        for c in cols:
            s += f"[{c}] {np.nanmin(us[:, c]):6.2f}/{np.nanmedian(us[:, c]):6.2f}/{np.nanmax(us[:, c]):6.2f}  "
        print(s)
        end_col = 3 if k == 0 else cols[-1]      # the product's words 4 - 7 lie inside its run: [3] is its end
        first, last = np.nanmin(us[:, cols[0]]), np.nanmax(us[:, end_col])
        if prev_end is not None:
            print(f"         gap from previous kernel's last stamp to this kernel's first start: {first - prev_end:.2f} us")
        print(f"         span {last - first:.2f} us")
        prev_end = last

# ---- who is in the tail of the covariance kernel (last trial)? ----
a = st[2]
live = a[:, 0] > 0
us = (a[live] - t0) / 100.0
end = us[:, 5]
order = np.argsort(-end)
print("cov kernel: slowest workgroups (blockIdx, start, loads, staged, mfma, mirror, drained):")
for i in order[:14]:
    print("   ", int(i), " ".join(f"{v:6.2f}" for v in us[i, :6]))
print("cov kernel: fastest:")
for i in order[-4:]:
    print("   ", int(i), " ".join(f"{v:6.2f}" for v in us[i, :6]))
ph = np.diff(us[:, :6], axis=1)
print("phase medians (loads, stage, mfma, mirror, drain):", np.round(np.median(ph, axis=0), 2), " p95:", np.round(np.percentile(ph, 95, axis=0), 2))
if (a[live][:, 6] > 0).all():    # "cov_s0_last": [1] = staged units landed (S0 still in flight), [6] = S0 landed, right before the W step
    s0 = us[:, 6]
    print("S0 landed: after start", np.round(np.median(s0 - us[:, 0]), 2), " after 'loads landed'", np.round(np.median(s0 - us[:, 1]), 2),
          " after the MFMAs", np.round(np.median(s0 - us[:, 3]), 2), " p95 of the last:", np.round(np.percentile(s0 - us[:, 3], 95), 2))
print("blocks >= 256 (single-tile): end median", np.median(end[256:]) if len(end) > 256 else None, " blocks < 256: end median", np.median(end[:256]), "p95", np.percentile(end[:256], 95))
# ---- the hosts of the folded diagonal tiles against the other workgroups (folded grid: the two-tile workgroups alone) ----
nt = D // 32
# ---- the quads against the pairs (round 13, "cov_diag_quad": the same grid size as the fold at D = 1024, so the knobs decide) ----
import re as _re
_ctx_h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsm-vi_amd", "csrc", "gsmvi_ctx.h")).read()
_knob = {k: int(_re.search(rf"int\s+tune_{k}\s*=\s*(\d+)\s*;", _ctx_h).group(1))
         for k in ("cov_diag_quad", "cov_wave_store", "cov_fold_diag", "cov_s0_last", "cov_store_wt", "panel_qm_whole", "panel_kc")}
_knob.update({kv.split("=")[0]: int(kv.split("=")[1]) for kv in sys.argv[2:]})
quad_on = (_knob["cov_diag_quad"] != 0 and _knob["cov_fold_diag"] != 0 and _knob["cov_s0_last"] != 0 and _knob["cov_store_wt"] != 0
           and _knob["panel_qm_whole"] == 0 and _knob["panel_kc"] <= 0 and len(end) == (nt >> 1) ** 2)
if quad_on:
    print(f"cov_wave_store = {_knob['cov_wave_store']} (round 14: 1 = per-wave store path; [4] stands behind a barrier in the stamped instance only)")
    quad = np.arange(len(end)) < (nt >> 1)
    for nm, sel in (("quads", quad), ("pairs", ~quad)):
        e, p = end[sel], ph[sel]
        print(f"{nm:6s} {sel.sum():3d} WGs: end min/median/max {e.min():.2f}/{np.median(e):.2f}/{e.max():.2f}  staged->MFMA done "
              f"{p[:, 2].min():.2f}/{np.median(p[:, 2]):.2f}/{p[:, 2].max():.2f}  MFMA done->last store issued "
              f"{p[:, 3].min():.2f}/{np.median(p[:, 3]):.2f}/{p[:, 3].max():.2f}  drain {np.median(p[:, 4]):.2f}")
    print(f"quads' last end - pairs' median end: {end[quad].max() - np.median(end[~quad]):.2f} us;  quads' last end - pairs' last end: "
          f"{end[quad].max() - end[~quad].max():.2f} us;  launch span {end.max() - us[:, 0].min():.2f} us")
elif len(end) == (nt >> 1) * ((nt + 1) >> 1):
    host = []
    for ti in range(nt):
        for rem in range((nt - ti) >> 1):
            host.append((((nt - ti) & 1) == 1 and rem == 0) or ti == nt - 2)
    host = np.array(host)
    for nm, sel in (("hosts", host), ("others", ~host)):
        e, p = end[sel], ph[sel]
        print(f"{nm:6s} {sel.sum():3d} WGs: end min/median/max {e.min():.2f}/{np.median(e):.2f}/{e.max():.2f}  staged->MFMA done "
              f"{p[:, 2].min():.2f}/{np.median(p[:, 2]):.2f}/{p[:, 2].max():.2f}  MFMA done->last store issued "
              f"{p[:, 3].min():.2f}/{np.median(p[:, 3]):.2f}/{p[:, 3].max():.2f}  drain {np.median(p[:, 4]):.2f}")
    print(f"hosts' last end - others' median end: {end[host].max() - np.median(end[~host]):.2f} us;  hosts' last end - others' last end: "
          f"{end[host].max() - end[~host].max():.2f} us;  launch span {end.max() - us[:, 0].min():.2f} us")
a = st[0]; live = a[:, 0] > 0; usp = (a[live] - t0) / 100.0
php = np.diff(usp[:, :4], axis=1)
print("panel phase medians (staged, mfma, end):", np.round(np.median(php, axis=0), 2), " p95:", np.round(np.percentile(php, 95, axis=0), 2))
# ---- the product's words 4 - 7 (round 12) ----
def _mp(x):
    return f"{np.median(x):.2f} (p95 {np.percentile(x, 95):.2f}, max {x.max():.2f})"
if (a[live][:, 4:8] > 0).all():
    t = usp - usp[:, :1]
    if (a[live][:, 1] == a[live][:, 6]).all():      # "panel_stream": [4] stage 0 staged, [5] first MFMA issued, [6] = [1] last stage staged, [7] last MFMA done
        print("panel (streamed), us after the workgroup's start, median (p95, max): stage 0 staged", _mp(t[:, 4]), " first MFMA issued", _mp(t[:, 5]),
              " last stage staged", _mp(t[:, 6]), " last MFMA done", _mp(t[:, 7]))
        print("panel (streamed) per stage: start -> stage 0 staged", _mp(t[:, 4]), " stage 0 -> last stage staged", _mp(t[:, 6] - t[:, 4]),
              " last stage staged -> last MFMA done", _mp(t[:, 7] - t[:, 6]), " -> reduction barrier", _mp(t[:, 2] - t[:, 7]), " -> end", _mp(t[:, 3] - t[:, 2]))
    else:                                           # "panel_stream" = 0: wave 0's [4] first G unit, [5] last G unit, [6] last S0 load landed; [7] wave 7's last G unit
        print("panel landing profile, us after the workgroup's start, median (p95, max): first G", _mp(t[:, 4]), " last G", _mp(t[:, 5]),
              " staged", _mp(t[:, 1]), " last S0", _mp(t[:, 6]))
        print("panel landing profile: first G -> last G", _mp(t[:, 5] - t[:, 4]), " last G -> staged", _mp(t[:, 1] - t[:, 5]),
              " last G -> last S0", _mp(t[:, 6] - t[:, 5]), " wave skew |wave 7 - wave 0| of the last G unit", _mp(np.abs(t[:, 7] - t[:, 5])),
              " staged - later wave's last G", _mp(t[:, 1] - np.maximum(t[:, 5], t[:, 7])))
