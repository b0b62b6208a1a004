"""The unit map of the streamed left operand of the two-slab product (k_panel_fast<.., PART, .., STREAM>, knob "panel_stream"),
restated in numpy from the comment in front of panel_stream_chunk (gsm-vi_amd/csrc/gsmvi_fast.hip) for NSTAGE = 2 and 4: the
staged chunk is 16 sample rows x 512 columns of doubles (256 16-byte units per row, LDS row stride 514 doubles); wave w of 8
multiplies columns 64 w .. 64 w + 63 (MFMA step s, k-slot ks = column 64 w + 4 s + ks), and loads exactly those itself, stage q =
steps q * 16 / NSTAGE .. (q + 1) * 16 / NSTAGE - 1."""
import os
import re

import numpy as np
import pytest

ROWS, CHW, LDG, WAVES, LANES, STEPS = 16, 512, 514, 8, 64, 16
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsm-vi_amd", "csrc")


def unit_map(ns):
    """(wave, stage, instruction, lane) -> (row, first column in doubles) of the 16-byte unit that lane loads and stages."""
    upr = 32 // ns              # units per row and stage
    rpi = LANES // upr          # rows per wave-instruction
    ips = ROWS // rpi           # wave-instructions per stage
    w, q, i, l = np.meshgrid(np.arange(WAVES), np.arange(ns), np.arange(ips), np.arange(LANES), indexing="ij")
    row = i * rpi + l // upr
    col = 64 * w + 2 * (l % upr) + q * (64 // ns)
    return row, col


def operand_columns(w, steps):
    """columns of the staged chunk that wave w's operand reads of these MFMA steps touch (every row c = 0 .. 15)"""
    return {64 * w + 4 * s + ks for s in steps for ks in range(4)}


@pytest.mark.parametrize("ns", [2, 4])
def test_every_unit_is_loaded_exactly_once(ns):
    row, col = unit_map(ns)
    assert row.size == ROWS * CHW // 2 and row.shape[2] * ns == 8          # 8 units per lane, as without the flag
    assert (col % 2 == 0).all() and row.min() == 0 and row.max() == ROWS - 1 and col.min() == 0 and col.max() == CHW - 2
    hits = np.zeros((ROWS, CHW // 2), dtype=int)
    np.add.at(hits, (row.ravel(), col.ravel() // 2), 1)
    assert (hits == 1).all()


@pytest.mark.parametrize("ns", [2, 4])
def test_a_wave_loads_what_it_multiplies_stage_by_stage(ns):
    row, col = unit_map(ns)
    sps = STEPS // ns
    for w in range(WAVES):
        mine = operand_columns(w, range(STEPS))
        assert mine == set(range(64 * w, 64 * w + 64))
        for q in range(ns):
            loaded = {(int(r), int(c) + h) for r, c in zip(row[w, q].ravel(), col[w, q].ravel()) for h in (0, 1)}
            want = {(r, c) for r in range(ROWS) for c in operand_columns(w, range(q * sps, (q + 1) * sps))}
            assert loaded == want, (ns, w, q)
            assert {c for _, c in loaded} <= mine


@pytest.mark.parametrize("ns", [2, 4])
def test_staging_writes_are_conflict_free_and_loads_are_whole_segments(ns):
    """ds_write_b128 is served in groups of 8 consecutive lanes, bank = (byte address / 4) mod 32, four banks per lane: a group must
    cover the 32 banks once.  The eight lanes of a group read 128 contiguous bytes of one row of G."""
    row, col = unit_map(ns)
    addr = (row * LDG + col) * 8
    assert (addr % 16 == 0).all()
    g = addr.reshape(-1, 8)                                                   # groups of 8 consecutive lanes
    banks = ((g[:, :, None] // 4 + np.arange(4)) % 32).reshape(len(g), 32)
    assert (np.sort(banks, axis=1) == np.arange(32)).all()
    rg, cg = row.reshape(-1, 8), col.reshape(-1, 8)
    assert (rg == rg[:, :1]).all() and (cg == cg[:, :1] + 2 * np.arange(8)).all() and (cg[:, 0] % 16 == 0).all()


@pytest.mark.parametrize("ns", [2, 4])
def test_waits_leave_the_later_stages_in_flight(ns):
    """Issue order: per stage its G units, then its S0 loads; the three partial-dot loads last.  vmcnt counts in issue order, so
    waiting for a load leaves exactly the loads issued behind it outstanding."""
    ips, sps = 8 // ns, STEPS // ns
    order = []
    for q in range(ns):
        order += [("g", q)] * ips + [("m", q)] * sps
    order += [("pq", None)] * 3
    assert len(order) == 27
    for q in range(ns):
        last_g = max(k for k, o in enumerate(order) if o == ("g", q))
        first_m = min(k for k, o in enumerate(order) if o == ("m", q))
        later = [o for o in order[first_m + 1:]]
        assert first_m == last_g + 1
        assert all(o[1] is None or o[1] >= q for o in later)
        assert sum(1 for o in later if o[1] is not None and o[1] > q) == (ns - 1 - q) * (ips + sps)     # all of them still in flight
    first_mfma_vmcnt = len(order) - 1 - order.index(("m", 0))
    assert first_mfma_vmcnt == 27 - ips - 1


def test_knob_and_instances_in_the_sources():
    with open(os.path.join(_CSRC, "gsmvi_ctx.h")) as f:
        m = re.search(r"int\s+tune_panel_stream\s*=\s*(\d+)\s*;", f.read())
    assert m and int(m.group(1)) in (0, 1)
    with open(os.path.join(_CSRC, "gsmvi_abi.hip")) as f:
        abi = f.read()
    assert '"panel_stream"' in abi
    with open(os.path.join(os.path.dirname(_CSRC), "..", "include", "gsmvi_hip.h")) as f:
        hdr = f.read()
    assert '"panel_stream"' in hdr
    bits = [int(v, 16) for v in re.findall(r"#define\s+GSMVI_PATH_\w+\s+(0x[0-9a-fA-F]+)u", hdr)]
    assert len(bits) == len(set(bits)) and max(bits) == 0x80000000          # no new path bit: the word is full
