#!/usr/bin/env python3
"""Assembly checks of the preloaded entry points (gsm-vi_amd/csrc/gsmvi_fast_hot.hip).  No GPU needed.

Compiles every translation unit of the library to device assembly with the Makefile's flags (--offload-device-only -S) and checks:
  * the entry points of gsmvi_fast_hot.hip have .amdhsa_user_sgpr_kernarg_preload_length > 0, every other kernel has 0;
  * behind the compatibility prologue a preloaded entry point has no s_waitcnt lgkmcnt in front of its first global_load (the
    scalar loads issued there -- arguments that are needed later -- are listed);
  * no scratch; LDS, VGPRs, SGPRs and occupancy are printed beside those of the entry point of gsmvi_fast.hip with the same body.
usage: scripts/kernarg_asm_check.py [--jobs N] [--only-fast]     (exit status 1 when a check fails)"""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gsm-vi_amd", "csrc")
HOT = "gsmvi_fast_hot.hip"


def make_vars():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    get = lambda name: re.search(rf"^{name}\s*\??=\s*(.*)$", mk, re.M).group(1)
    flags = get("CXXFLAGS").replace("$(ARCH)", get("ARCH")).split()
    kflags = {m.group(1): m.group(2).split() for m in re.finditer(r"^KFLAGS_(\w+)\s*=\s*(.*)$", mk, re.M)}
    return get("HIPCC"), flags, get("SRCS").split(), kflags


def compile_s(hipcc, flags, kflags, src, outdir):
    out = os.path.join(outdir, src.replace(".hip", ".s"))
    cmd = [hipcc] + flags + kflags.get(src[:-4], []) + ["--offload-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
    return src, out


def kernels(path):
    """name -> dict(body lines, directives) of every kernel of one assembly file"""
    text = open(path).read()
    res = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.M | re.S):
        d = dict(re.findall(r"^\t\t\.amdhsa_(\w+) (\S+)$", m.group(2), re.M))
        res[m.group(1)] = {"dir": d}
    for name in res:
        b = re.search(rf"^{re.escape(name)}:.*?\n(.*?)^\ts_endpgm", text, re.M | re.S)
        res[name]["body"] = b.group(1).splitlines() if b else []
        o = re.search(rf"^{re.escape(name)}:.*?^; Occupancy: (\d+)", text, re.M | re.S)
        res[name]["occ"] = int(o.group(1)) if o else -1
    return res


def front(body):
    """instructions between the compatibility prologue (ends with s_branch to the aligned entry) and the first global_load"""
    ins = [l.strip() for l in body if l.startswith("\t") and not l.strip().startswith((";", "."))]
    start = next((i + 1 for i, l in enumerate(ins[:8]) if l.startswith("s_branch")), 0)
    end = next(i for i, l in enumerate(ins) if l.startswith("global_load") and i >= start)
    return ins[:start], ins[start:end]


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, p.stdout.splitlines()))


def twin(dem):
    """the entry point of gsmvi_fast.hip that runs the same body, as a demangled prefix"""
    m = re.match(r"void k_panel_part_hot<(-?\d+), (-?\d+), (-?\d+)>", dem)
    if m:
        mt, chw, ns = m.groups()
        return f"void k_panel_fast<{mt}, false, {chw}, false, false, false, true, false, {ns}>"
    m = re.match(r"void k_gsm_cov_slabs_hot<(\d+), (\d+), (\w+), (\w+), (\w+), (\w+), (\w+)>", dem)
    sb, kct, fold, s0l, wt, quad, wst = m.groups()
    return f"void k_gsm_cov_sym<{sb}, false, true, {kct}, {fold}, {s0l}, {wt}, false, {quad}, {wst}>"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only-fast", action="store_true", help="compile gsmvi_fast.hip and gsmvi_fast_hot.hip alone")
    a = ap.parse_args()
    hipcc, flags, srcs, kflags = make_vars()
    if a.only_fast:
        srcs = ["gsmvi_fast.hip", HOT]
    bad = 0
    with tempfile.TemporaryDirectory() as td:
        with cf.ThreadPoolExecutor(a.jobs) as ex:
            outs = dict(ex.map(lambda s: compile_s(hipcc, flags, kflags, s, td), srcs))
        ks = {src: kernels(path) for src, path in outs.items()}
    n_other = 0
    for src, kk in ks.items():
        for name, k in kk.items():
            pl = int(k["dir"].get("user_sgpr_kernarg_preload_length", "0"))
            if src == HOT:
                if pl <= 0:
                    print(f"FAIL {name}: preload length {pl}")
                    bad += 1
            else:
                n_other += 1
                if pl != 0:
                    print(f"FAIL {src} {name}: preload length {pl} outside {HOT}")
                    bad += 1
    print(f"kernels outside {HOT}: {n_other}, all with kernarg preload length 0" if not bad else "preload lengths: see above")
    dem = demangle(list(ks[HOT]) + list(ks["gsmvi_fast.hip"]))
    fast_by_dem = {dem[n]: k for n, k in ks["gsmvi_fast.hip"].items()}
    cols = ("user_sgpr_kernarg_preload_length", "user_sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
            "next_free_vgpr", "accum_offset", "next_free_sgpr")
    print("\nentry point | " + " | ".join(c.replace("user_sgpr_", "").replace("_fixed_size", "") for c in cols) + " | occupancy")
    for name, k in ks[HOT].items():
        d = dem[name].split("(")[0]
        pro, fr = front(k["body"])
        sl = [l for l in fr if l.startswith("s_load")]
        wt = [l for l in fr if l.startswith("s_waitcnt") and "lgkmcnt" in l]
        row = lambda kk: " | ".join(kk["dir"].get(c, "?") for c in cols) + f" | {kk['occ']}"
        print(f"{d}\n    hot  | {row(k)}")
        tw = next((v for dn, v in fast_by_dem.items() if dn.startswith(twin(dem[name]) + "(")), None)
        if tw is None:
            print("    twin | (not instantiated in gsmvi_fast.hip)")
        else:
            print(f"    twin | {row(tw)}")
            for c in ("group_segment_fixed_size", "private_segment_fixed_size"):
                if tw["dir"].get(c) != k["dir"].get(c):
                    print(f"FAIL {d}: {c} differs from the twin's")
                    bad += 1
            if tw["occ"] != k["occ"]:
                print(f"FAIL {d}: occupancy {k['occ']} against the twin's {tw['occ']}")
                bad += 1
            _, tfr = front(tw["body"])
            print(f"    twin's front: {sum(l.startswith('s_load') for l in tfr)} s_load, "
                  f"{sum(l.startswith('s_waitcnt') and 'lgkmcnt' in l for l in tfr)} s_waitcnt lgkmcnt before the first global_load")
        print(f"    prologue: {'; '.join(pro)}")
        print(f"    front: {len(fr)} instructions, {len(wt)} s_waitcnt lgkmcnt, s_load issued (not waited for): {sl if sl else 'none'}")
        if wt and d.endswith("k_panel_part_hot<1, 512, -1>"):
            print("    (launched with the timeline diagnostic on only: its landing profile tests `stamps` in front of the loads)")
        elif wt:
            print(f"FAIL {d}: {wt} in front of the first global_load")
            bad += 1
        if k["dir"].get("private_segment_fixed_size") != "0":
            print(f"FAIL {d}: scratch")
            bad += 1
    print("\n" + ("FAILED: %d" % bad if bad else "all checks passed"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
