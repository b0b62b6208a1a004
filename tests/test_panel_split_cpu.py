"""csrc/gsmvi_panel_split.h (the one split-K function of the panel products) against a restatement of the three code blocks it
replaced in csrc/gsmvi_abi.hip -- gsmvi_panel_product_nc, gsmvi_panel_product_out and gsm_two_launch_gate --, each written out
below from those blocks as they stood, not from the function.  tests/abi_c/panel_split_table.cpp prints the function's table."""
import os
import subprocess

import pytest

from conftest import ROOT

MAX_KC = 8                        # GSMVI_MAX_KC (csrc/gsmvi_ctx.h)
ITEMS = (1, 2, 3, 16, 32, 48, 64, 128, 256, 257, 512, 1024)


def site_nc(items, nchunks, tune, num_cu):
    """gsmvi_panel_product_nc: clamps to nchunks, to GSMVI_MAX_KC and to at least 1"""
    kc = tune if tune > 0 else (2 * num_cu + items - 1) // items
    if kc > nchunks:
        kc = nchunks
    if kc > MAX_KC:
        kc = MAX_KC
    if kc < 1:
        kc = 1
    cpw = (nchunks + kc - 1) // kc
    kc = (nchunks + cpw - 1) // cpw
    return kc, cpw


def site_out(items, nchunks, tune, num_cu):
    """gsmvi_panel_product_out: the same two upper clamps, then ``if (kc >= 1)`` around the rest (None: the branch not taken)"""
    kc = tune if tune > 0 else (2 * num_cu + items - 1) // items
    if kc > nchunks:
        kc = nchunks
    if kc > MAX_KC:
        kc = MAX_KC
    if kc >= 1:
        cpw = (nchunks + kc - 1) // kc
        kc = (nchunks + cpw - 1) // cpw
        return kc, cpw
    return None


def site_gate(items, nchunks, tune, num_cu):
    """gsm_two_launch_gate (items = strips): clamps to nchunks and to at least 1, NO GSMVI_MAX_KC clamp; then the route is taken
    only with kc <= 4 slabs of whole chunks.  Returns (kc, cpw, taken)."""
    kc = tune if tune > 0 else (2 * num_cu + items - 1) // items
    if kc > nchunks:
        kc = nchunks
    if kc < 1:
        kc = 1
    cpw = (nchunks + kc - 1) // kc
    kc = (nchunks + cpw - 1) // cpw
    return kc, cpw, not (kc > 4 or kc * cpw != nchunks)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("split") / "panel_split_table")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "gsm-vi_amd", "csrc"),
           os.path.join(ROOT, "tests", "abi_c", "panel_split_table.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    out = {}
    for ln in p.stdout.splitlines():
        it, n, t, cu, kc, cpw = (int(x) for x in ln.split())
        out[(it, n, t, cu)] = (kc, cpw)
    assert sorted(out) == sorted((it, n, t, cu) for it in ITEMS for n in range(1, 65) for t in range(10) for cu in (256, 64))
    return out


def test_split_is_the_plain_products(table):
    for key, got in table.items():
        assert got == site_nc(*key), key


def test_split_is_the_finished_output_products_and_its_guard_never_fails(table):
    for key, got in table.items():
        assert site_out(*key) is not None and got == site_out(*key), key


def test_split_is_the_two_launch_gates(table):
    """The gate never clamped to GSMVI_MAX_KC.  Its nchunks is D / 256 <= 4, where that clamp cannot bind: there the pair is the
    gate's.  Beyond (the gate never gets there) the pairs may differ, but never the decision, nor the pair of a taken route."""
    for key, got in table.items():
        kc, cpw, taken = site_gate(*key)
        if key[1] <= 4:
            assert got == (kc, cpw), key
        assert (not (got[0] > 4 or got[0] * got[1] != key[1])) == taken, key
        if taken:
            assert got == (kc, cpw), key
