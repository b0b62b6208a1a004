"""CPU: the quad / pair item map of k_gsm_cov_sym<.., FROM_SLABS, .., QUAD> and the chain assignment of a quad (gsm_cov_quad in
csrc/gsmvi_fast.hip), restated with the kernel's index arithmetic.  For nt in {8, 16, 24, 32} (D = 256 .. 1024): every
upper-triangle tile and every mu block exactly once, (nt/2)^2 workgroups with the quads at the first nt/2 ids, every quad stages
exactly the two column blocks its three tiles need, and the twenty chains of a quad are each assigned once, five per SIMD.  Also the
knob's default, the fold knob's, and the number of path bits (the quad route adds none)."""
import os
import re

import pytest

from conftest import ROOT

NTS = [8, 16, 24, 32]


def item(nt, bid):
    """(kind, tiles, mu blocks, staged column blocks) of workgroup `bid`, as the kernel computes them."""
    h = nt >> 1
    if bid < h:                                         # quad p: blocks A = 2p, B = 2p + 1
        a, b = 2 * bid, 2 * bid + 1
        return "quad", [(a, a), (a, b), (b, b)], [a, b], {a, b}
    rem, ti = bid - h, 0
    while True:
        inrow = h - (ti >> 1) - 1
        if rem < inrow:
            break
        rem -= inrow
        ti += 1
    tj0 = 2 * ((ti >> 1) + 1) + 2 * rem
    return "pair", [(ti, tj0), (ti, tj0 + 1)], [], {ti, tj0, tj0 + 1}


def quad_chains():
    """[(wave, tile, block row, block column, chain)] of a quad: a whole block per wave, then one chain of a split block on waves 0-3.
    Tiles: 0 = (A, A), 1 = (A, B), 2 = (B, B)."""
    out = []
    for w in range(8):
        if w >= 4:
            tile, br, bc = 1, (w >> 1) & 1, w & 1
        else:
            tile = 2 if w == 3 else 0                   # ta = (w == 3) ? 2 : 0, tb = (w >= 3) ? 2 : 0: both operands of one block
            br = 1 if w == 2 else 0
            bc = 1 if w in (1, 2) else 0
        out += [(w, tile, br, bc, "d"), (w, tile, br, bc, "e")]
        if w < 4:                                       # (B, B) block (w >> 1, 1): d on the even wave, e on the odd one
            out.append((w, 2, w >> 1, 1, "e" if w & 1 else "d"))
    return out


@pytest.mark.parametrize("nt", NTS)
def test_every_tile_and_every_mu_block_exactly_once(nt):
    tiles, mus = [], []
    for bid in range((nt // 2) ** 2):
        _, t, m, _ = item(nt, bid)
        tiles += t
        mus += m
    assert sorted(tiles) == [(i, j) for i in range(nt) for j in range(i, nt)]
    assert sorted(mus) == list(range(nt))


@pytest.mark.parametrize("nt", NTS)
def test_grid_and_quads_first(nt):
    h = nt // 2
    kinds = [item(nt, bid)[0] for bid in range(h * h)]
    assert kinds == ["quad"] * h + ["pair"] * (h * (h - 1))
    assert h + sum(h - (i >> 1) - 1 for i in range(nt)) == h * h
    for bid in range(h, h * h):                         # pairs: never diagonal, right of their row's quad, inside the matrix
        _, t, m, _ = item(nt, bid)
        (i, j0), (_, j1) = t
        assert not m and j0 % 2 == 0 and j1 == j0 + 1 and j0 // 2 > i // 2 and j1 < nt
    if nt == 32:
        assert h * h == 256


@pytest.mark.parametrize("nt", NTS)
def test_quads_stage_the_two_blocks_their_tiles_need(nt):
    for p in range(nt // 2):
        _, tiles, mus, staged = item(nt, p)
        assert staged == {i for t in tiles for i in t} == {2 * p, 2 * p + 1} and len(staged) == 2
        assert mus == [2 * p, 2 * p + 1]


def test_twenty_chains_five_per_simd():
    ch = quad_chains()
    # the blocks the result needs: block (1, 0) of a diagonal tile is written as the transpose of block (0, 1), not computed
    need = [(t, r, c) for t in (0, 2) for (r, c) in ((0, 0), (0, 1), (1, 1))] + [(1, r, c) for r in (0, 1) for c in (0, 1)]
    assert len(need) == 10
    assert sorted((t, r, c, k) for _, t, r, c, k in ch) == sorted((t, r, c, k) for (t, r, c) in need for k in "de")
    per_simd = [sum(1 for w, *_ in ch if w & 3 == s) for s in range(4)]
    assert per_simd == [5, 5, 5, 5]
    split = {}
    for w, t, r, c, k in ch:
        split.setdefault((t, r, c), set()).add(w)
    halves = [b for b, ws in split.items() if len(ws) == 2]
    assert sorted(halves) == [(2, 0, 1), (2, 1, 1)]     # a split block's chains on different waves (and different SIMDs)
    for b in halves:
        assert len({w & 3 for w in split[b]}) == 2 and max(split[b]) < 4


def test_quad_lds():
    for sb, want in ((16, 41728), (32, 6 * 32 * 48 * 8)):
        scr = max(3 * 32 * 33 + 2 * sb * 32 + 512, 4 * sb * 48)     # COV_QUAD_SCR: behind the store path's LDS and the staged tiles
        assert max(scr + 512, 6 * sb * 48) * 8 == want


def test_knob_defaults_and_path_bits():
    from gsmvi_amd.engine import HipEngine
    ctx = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_ctx.h")).read()
    abi = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_abi.hip")).read()
    assert int(re.search(r"int\s+tune_cov_diag_quad\s*=\s*(\d+)\s*;", ctx).group(1)) == 1
    assert int(re.search(r"int\s+tune_cov_fold_diag\s*=\s*(\d+)\s*;", ctx).group(1)) == 1
    assert '"cov_diag_quad"' in abi
    assert len(HipEngine.PATH_BITS) == 32
    assert HipEngine.PATH_BITS["cov_fold_diag"] == 0x8000000 and "cov_diag_quad" not in HipEngine.PATH_BITS
