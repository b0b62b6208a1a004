"""CPU: the item map of k_gsm_cov_sym<.., FROM_SLABS, .., FOLD> (csrc/gsmvi_fast.hip), restated with the kernel's index arithmetic.
With the diagonal leftovers folded the grid is the n_two two-tile workgroups alone; for nt in {8, 16, 24, 32} (D = 256 .. 1024)
the map covers every upper-triangle tile exactly once, writes every mu block exactly once, and names for every leftover a host
that has staged the leftover's column block.  Also: the path bit and the knob's default in the header, engine and context."""
import os
import re

import pytest

from conftest import ROOT

NTS = [8, 16, 24, 32]


def n_two(nt):
    return (nt >> 1) * ((nt + 1) >> 1)


def item(nt, bid, fold_on):
    """(tiles, mu blocks, staged blocks, fold kind, folded block) of workgroup `bid`, as the kernel computes them."""
    fold = 0
    if fold_on or bid < n_two(nt):
        rem, ti = bid, 0
        while True:
            inrow = (nt - ti) >> 1
            if rem < inrow:
                break
            rem -= inrow
            ti += 1
        tj0 = ti + ((nt - ti) & 1) + 2 * rem
        two = True
        if fold_on:
            fold = 1 if (((nt - ti) & 1) and rem == 0) else (2 if ti == nt - 2 else 0)
    else:
        k = bid - n_two(nt)
        ti = (0 if nt & 1 else 1) + 2 * k
        tj0 = ti
        two = False
    diag = tj0 == ti
    tiles = [(ti, tj0)] + ([(ti, tj0 + 1)] if two else [])
    staged = {ti, tj0} | ({tj0 + 1} if two else set())
    mus = [ti] if diag else []
    x = None
    if fold:
        x = tj0 + 1 if fold == 2 else ti        # X0 = (fold == 2) ? J0 + 32 : I0
        tiles.append((x, x))
        mus.append(x)
    return tiles, mus, staged, fold, x


def grid(nt, fold_on):
    return n_two(nt) if fold_on else sum((nt - ti + 1) // 2 for ti in range(nt))


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("fold_on", [False, True])
def test_every_tile_and_every_mu_block_exactly_once(nt, fold_on):
    tiles, mus = [], []
    for bid in range(grid(nt, fold_on)):
        t, m, _, _, _ = item(nt, bid, fold_on)
        tiles += t
        mus += m
    upper = [(i, j) for i in range(nt) for j in range(i, nt)]
    assert sorted(tiles) == upper
    assert sorted(mus) == list(range(nt))


@pytest.mark.parametrize("nt", NTS)
def test_hosts_hold_the_leftover_block(nt):
    assert grid(nt, True) == n_two(nt) and grid(nt, False) - grid(nt, True) == nt // 2
    leftovers = {ti for ti in range(nt) if (nt - ti) & 1}
    hosted = {}
    for bid in range(n_two(nt)):
        tiles, _, staged, fold, x = item(nt, bid, True)
        if not fold:
            continue
        assert x in staged and x not in hosted
        hosted[x] = bid
        ti, tj0 = tiles[0]
        if fold == 1:                               # rows with >= 3 tiles: the first pair of the row, operands = the I tiles
            assert x == ti and nt - ti >= 3 and tiles[:2] == [(ti, ti + 1), (ti, ti + 2)]
        else:                                       # the last row: the pair of row nt - 2, operands = its J1 tiles
            assert x == nt - 1 == tj0 + 1 and tiles[:2] == [(nt - 2, nt - 2), (nt - 2, nt - 1)]
    assert set(hosted) == leftovers
    if nt == 8:
        assert sorted(hosted) == [1, 3, 5, 7]


def test_third_update_buffer_fits_the_staged_tiles():
    for sb in (16, 32):
        assert 3 * 32 * 33 <= 6 * sb * 48


def test_path_bit_and_knob_default():
    from gsmvi_amd.engine import HipEngine
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    ctx = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_ctx.h")).read()
    assert HipEngine.PATH_BITS["cov_fold_diag"] == 0x8000000
    assert re.search(r"#define\s+GSMVI_PATH_COV_FOLD_DIAG\s+0x8000000u", hdr)
    assert not HipEngine.PATH_GENERIC_MASK & 0x8000000
    assert len(set(HipEngine.PATH_BITS.values())) == len(HipEngine.PATH_BITS)
    assert int(re.search(r"int\s+tune_cov_fold_diag\s*=\s*(\d+)\s*;", ctx).group(1)) == 1
    assert "#define GSMVI_ABI_VERSION 1" in hdr
