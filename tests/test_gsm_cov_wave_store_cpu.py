"""The lane maps of the per-wave store path of the covariance launch (k_gsm_cov_sym<.., QUAD, WST>, knob "cov_wave_store"), restated
in numpy with the index arithmetic of gsm_cov_wave_direct / gsm_cov_wave_mirror and of the WST branches of k_gsm_cov_sym and
gsm_cov_quad (gsm-vi_amd/csrc/gsmvi_fast.hip), for SB in {16, 32}.

A wave w of 8 holds block (wr, wc) = ((w >> 1) & 1, w & 1) of tile t = w >> 2 in MFMA accumulator layout: lane l = (c = l & 15,
ks = l >> 4) holds u[r] = U[ks + 4 r][c], r = 0 .. 3.  Direct units: (row ks + 4 (c & 1) + 8 q, columns c & ~1, + 1), q = 0, 1.  Mirror
units: lane (j = (l >> 3) + 8 q, i2 = l & 7) stores (W[2 i2][j], W[2 i2 + 1][j]) at row j, columns 2 i2, + 1 of the transposed block,
read from a wave-private [16][COV_WST_RS] buffer."""
import os
import re

import numpy as np
import pytest

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsm-vi_amd", "csrc")
with open(os.path.join(_CSRC, "gsmvi_fast.hip")) as _f:
    _SRC = _f.read()
RS = int(re.search(r"constexpr int COV_WST_RS = (\d+), COV_WST_PB = 16 \* COV_WST_RS;", _SRC).group(1))
PB = 16 * RS
LANES = np.arange(64)
C, KS = LANES & 15, LANES >> 4


def direct_units(q):
    """(row, first column) inside the 16 x 16 block of the q-th direct unit of every lane"""
    return KS + 4 * (C & 1) + 8 * q, C & ~1


def mirror_units(q):
    """(row j, first column 2 i2) inside the TRANSPOSED block of the q-th mirror unit of every lane"""
    return (LANES >> 3) + 8 * q, 2 * (LANES & 7)


def segments_are_128_bytes(row, col):
    """a wave instruction: every group of 8 consecutive lanes writes one row's 128 contiguous, 128-byte aligned bytes"""
    r, c = row.reshape(-1, 8), col.reshape(-1, 8)
    srt = np.sort(c, axis=1)
    return bool((r == r[:, :1]).all() and (srt == srt[:, :1] + 2 * np.arange(8)).all() and (srt[:, 0] % 16 == 0).all())


def test_direct_units_of_a_pair_cover_both_tiles_once_in_128_byte_segments():
    hits = np.zeros((32, 64), dtype=int)                     # the pair's two tiles side by side
    for w in range(8):
        t, wr, wc = w >> 2, (w >> 1) & 1, w & 1
        for q in range(2):
            row, col = direct_units(q)
            assert (col % 2 == 0).all()                       # 16-byte aligned (tile columns and leading dimensions are even)
            # lanes 2k, 2k + 1 hold the same column pair in rows ks, ks + 4: a row's eight units sit on the even (odd) lanes of a DPP row
            for par in (0, 1):
                sel = (C & 1) == par
                assert segments_are_128_bytes(row[sel], col[sel])
            for h in (0, 1):
                np.add.at(hits, (16 * wr + row, 32 * t + 16 * wc + col + h), 1)
    assert (hits == 1).all()


def test_mirror_units_of_a_pair_cover_both_transposed_tiles_once_in_128_byte_segments():
    hits = np.zeros((64, 32), dtype=int)                     # S[J0 .. J0 + 63][I0 .. I0 + 31]
    for w in range(8):
        t, wr, wc = w >> 2, (w >> 1) & 1, w & 1
        for q in range(2):
            j, i = mirror_units(q)
            assert (i % 2 == 0).all() and segments_are_128_bytes(j, i)
            for h in (0, 1):
                np.add.at(hits, (32 * t + 16 * wc + j, 16 * wr + i + h), 1)
    assert (hits == 1).all()


def _exchange(U):
    """gsm_cov_wave_direct's exchange on one block: the two units (ua, ub) of every lane"""
    u = np.stack([U[KS + 4 * r, C] for r in range(4)])        # accumulator layout
    odd = (C & 1) == 1
    swap = LANES ^ 1                                          # quad_perm [1, 0, 3, 2]
    send0, send1 = np.where(odd, u[0], u[1]), np.where(odd, u[2], u[3])
    x0, x1 = send0[swap], send1[swap]
    ua = np.stack([np.where(odd, x0, u[0]), np.where(odd, u[1], x0)], axis=1)
    ub = np.stack([np.where(odd, x1, u[2]), np.where(odd, u[3], x1)], axis=1)
    return ua, ub


def test_dpp_exchange_reproduces_the_block_and_the_buffer_transposes_it():
    rng = np.random.default_rng(14)
    U, S0 = rng.standard_normal((16, 16)), rng.standard_normal((16, 16))
    ua, ub = _exchange(U)
    W, buf = np.full((16, 16), np.nan), np.full(PB, np.nan)
    for q, un in enumerate((ua, ub)):
        row, col = direct_units(q)
        assert (un[:, 0] == U[row, col]).all() and (un[:, 1] == U[row, col + 1]).all()
        w2 = np.stack([S0[row, col], S0[row, col + 1]], axis=1) + un      # S0 units in the same layout: s0 + u
        W[row, col], W[row, col + 1] = w2[:, 0], w2[:, 1]
        buf[row * RS + col], buf[row * RS + col + 1] = w2[:, 0], w2[:, 1]
    assert (W == S0 + U).all()
    M = np.full((16, 16), np.nan)
    for q in range(2):
        j, i = mirror_units(q)
        M[j, i], M[j, i + 1] = buf[i * RS + j], buf[(i + 1) * RS + j]
    assert (M == W.T).all()


def test_private_buffer_writes_and_column_reads_are_bank_conflict_free():
    """ds_write_b128: groups of 8 consecutive lanes, bank = (byte address / 4) mod 32, four banks per lane -- a group covers the 32
    banks once (the rule of tests/test_gsm_panel_stream_cpu.py).  ds_read_b64: the two 32-lane halves, bank = (byte address / 4) mod
    64, two banks per lane -- a half covers the 64 banks once."""
    for q in range(2):
        row, col = direct_units(q)
        addr = (row * RS + col) * 8
        assert (addr % 16 == 0).all()
        g = addr.reshape(-1, 8)
        banks = ((g[:, :, None] // 4 + np.arange(4)) % 32).reshape(len(g), 32)
        assert (np.sort(banks, axis=1) == np.arange(32)).all()
        j, i = mirror_units(q)
        for h in (0, 1):                                       # rows 2 i2 and 2 i2 + 1: one ds_read_b64 each
            a = (((i + h) * RS + j) * 8).reshape(2, 32)
            banks = ((a[:, :, None] // 4 + np.arange(2)) % 64).reshape(2, 64)
            assert (np.sort(banks, axis=1) == np.arange(64)).all()
        assert max(int((row * RS + col + 1).max()), int(((i + 1) * RS + j).max())) < PB


def _lds(SB):
    """the kernel's LDS map in doubles: staged tile, a quad's LDS, the private buffers' offset, the total"""
    tile = SB * 48
    scr = max(3 * 32 * 33 + 2 * SB * 32 + 512, 4 * SB * 48)
    qlds = scr + 512
    pbo = max(6 * tile, qlds, 2 * 32 * 33)
    return tile, scr, qlds, pbo, pbo + 8 * PB


@pytest.mark.parametrize("SB", [16, 32])
def test_private_buffers_overlap_nothing_and_the_total_fits(SB):
    tile, scr, qlds, pbo, total = _lds(SB)
    assert pbo % 2 == 0 and PB % 2 == 0                        # 16-byte aligned units
    assert pbo >= 6 * tile and pbo >= qlds                     # behind the pairs' six staged tiles and behind a quad's LDS
    spans = [(pbo + w * PB, pbo + (w + 1) * PB) for w in range(8)]
    assert all(a1 <= b0 for (_, a1), (b0, _) in zip(spans, spans[1:])) and spans[-1][1] == total
    assert total * 8 < 160 * 1024
    assert total * 8 == {16: 41728, 32: 73728}[SB] + 8 * PB * 8
    # a quad's means with the flag: dmu tiles and partial sums outside the four staged tiles, the hand-over and the buffers
    muo = 3 * 32 * 33
    muw = muo if muo >= 4 * tile else qlds
    paw = muw + 2 * SB * 32
    assert muw >= 4 * tile and paw + 512 <= (scr if muo >= 4 * tile else pbo)
    assert 256 <= PB                                           # a handed-over e-chain (4 x 64 doubles) fits a private buffer (waves 0, 3)


def test_a_quad_writes_every_element_of_its_three_tiles_and_both_transposes_once():
    """gsm_cov_quad with the flag, the diagonal 64 x 64 block [A; B] x [A; B]: waves 4-7 block (wr, wc) of tile (A, B) and its
    mirror; wave 0 (A, A) (0, 0) and (B, B) (0, 1); wave 1 (A, A) (0, 1) and its transpose (A, A) (1, 0); wave 2 (A, A) (1, 1) and
    the transpose (B, B) (1, 0); wave 3 (B, B) (0, 0) and (B, B) (1, 1)."""
    A0, B0 = 0, 32
    hits = np.zeros((64, 64), dtype=int)

    def direct(r0, c0):
        for q in range(2):
            row, col = direct_units(q)
            for h in (0, 1):
                np.add.at(hits, (r0 + row, c0 + col + h), 1)

    def mirror(r0, c0):
        for q in range(2):
            j, i = mirror_units(q)
            for h in (0, 1):
                np.add.at(hits, (r0 + j, c0 + i + h), 1)

    for w in range(4, 8):
        wr, wc = (w >> 1) & 1, w & 1
        direct(A0 + 16 * wr, B0 + 16 * wc)
        mirror(B0 + 16 * wc, A0 + 16 * wr)
    direct(A0, A0), direct(B0, B0 + 16)                        # wave 0
    direct(A0, A0 + 16), mirror(A0 + 16, A0)                   # wave 1
    direct(A0 + 16, A0 + 16), mirror(B0 + 16, B0)              # wave 2
    direct(B0, B0), direct(B0 + 16, B0 + 16)                   # wave 3
    assert (hits == 1).all()


def test_s0_units_of_a_quad_are_those_of_the_blocks_its_waves_store():
    """load_s0 of gsm_cov_quad with the flag: four units per lane on every wave; s0w[0 .. 1] in the direct layout of the wave's whole
    block, s0w[2 .. 3] in the layout of its second block (the mirror's on waves 1 and 2)."""
    A0, B0 = 0, 32
    first = {0: (A0, A0), 1: (A0, A0 + 16), 2: (A0 + 16, A0 + 16), 3: (B0, B0)}
    second = {0: (B0, B0 + 16, False), 1: (A0 + 16, A0, True), 2: (B0 + 16, B0, True), 3: (B0 + 16, B0 + 16, False)}
    for w in range(8):
        wr, wc = (w >> 1) & 1, w & 1
        r0 = A0 + 16 * wr if w >= 4 else (B0 if w == 3 else (A0 + 16 if w == 2 else A0))
        c0 = B0 + 16 * wc if w >= 4 else (B0 if w == 3 else (A0 if w == 0 else A0 + 16))
        r1 = r0 if w >= 4 else (B0 if w == 0 else (A0 + 16 if w == 1 else B0 + 16))
        c1 = c0 if w >= 4 else (A0 if w == 1 else (B0 if w == 2 else B0 + 16))
        mir = w in (1, 2)
        if w < 4:
            assert (r0, c0) == first[w] and (r1, c1, mir) == second[w]
        else:
            assert (r0, c0) == (A0 + 16 * wr, B0 + 16 * wc) == (r1, c1) and not mir


def test_knob_and_instances_in_the_sources():
    with open(os.path.join(_CSRC, "gsmvi_ctx.h")) as f:
        m = re.search(r"int\s+tune_cov_wave_store\s*=\s*(\d+)\s*;", f.read())
    assert m and int(m.group(1)) in (0, 1)
    with open(os.path.join(_CSRC, "gsmvi_abi.hip")) as f:
        assert '"cov_wave_store"' in f.read()
    with open(os.path.join(os.path.dirname(_CSRC), "..", "include", "gsmvi_hip.h")) as f:
        hdr = f.read()
    assert '"cov_wave_store"' in hdr
    bits = [int(v, 16) for v in re.findall(r"#define\s+GSMVI_PATH_\w+\s+(0x[0-9a-fA-F]+)u", hdr)]
    assert len(bits) == len(set(bits)) and max(bits) == 0x80000000          # no new path bit: the word is full
    # the flag is instantiated on the QUAD instances alone (one launch macro, SB in {16, 32} x {KCT = 2 S0L WT, KCT = 4})
    assert len(re.findall(r"k_gsm_cov_sym<SBV, false, true, KV, false, LV, WV, false, true, SV>", _SRC)) == 1
    assert 'static_assert(!WST || QUAD' in _SRC
