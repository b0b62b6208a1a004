"""CPU: the path bit of the 512-row product of the two-launch dense GSM update (two slabs at D = 1024) is the same number in the
header and in HipEngine.PATH_BITS, lies outside the generic mask, collides with no other bit; the two-launch knob still
defaults to 1 and the ABI version did not move."""
import os
import re

from conftest import ROOT


def test_panel_chunk512_path_bit_header_and_engine_agree():
    from gsmvi_amd.engine import HipEngine
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    assert HipEngine.PATH_BITS["panel_chunk512"] == 0x2000000
    m = re.search(r"#define\s+GSMVI_PATH_PANEL_CHUNK512\s+(0x[0-9a-fA-F]+)u", hdr)
    assert m and int(m.group(1), 16) == HipEngine.PATH_BITS["panel_chunk512"]
    assert len(set(HipEngine.PATH_BITS.values())) == len(HipEngine.PATH_BITS)
    assert "#define GSMVI_ABI_VERSION 1" in hdr


def test_panel_chunk512_is_outside_the_generic_mask():
    from gsmvi_amd.engine import HipEngine
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    assert not HipEngine.PATH_GENERIC_MASK & 0x2000000
    mask = re.search(r"#define\s+GSMVI_PATH_GENERIC_MASK\s+\(([^)]*)\)", hdr).group(1)
    assert not eval(mask.replace("u", "")) & 0x2000000
    assert eval(mask.replace("u", "")) == HipEngine.PATH_GENERIC_MASK


def test_two_launch_knob_still_defaults_to_one():
    ctx = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_ctx.h")).read()
    assert int(re.search(r"int\s+tune_gsm_two_launch\s*=\s*(\d+)\s*;", ctx).group(1)) == 1
