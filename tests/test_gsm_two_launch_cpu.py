"""CPU: the path bit of the two-launch dense GSM update is the same number in the header and in HipEngine.PATH_BITS, lies
outside the generic mask, collides with no other bit, and the ABI version did not move."""
import os
import re

from conftest import ROOT


def test_two_launch_path_bit_header_and_engine_agree():
    from gsmvi_amd.engine import HipEngine
    hdr = open(os.path.join(ROOT, "include", "gsmvi_hip.h")).read()
    assert HipEngine.PATH_BITS["gsm_two_launch"] == 0x800000
    assert not HipEngine.PATH_GENERIC_MASK & 0x800000
    assert len(set(HipEngine.PATH_BITS.values())) == len(HipEngine.PATH_BITS)
    assert re.search(r"#define\s+GSMVI_PATH_GSM_TWO_LAUNCH\s+0x800000u", hdr)
    mask = re.search(r"#define\s+GSMVI_PATH_GENERIC_MASK\s+\(([^)]*)\)", hdr).group(1)
    assert "0x800000" not in mask
    assert eval(mask.replace("u", "")) == HipEngine.PATH_GENERIC_MASK
    assert "#define GSMVI_ABI_VERSION 1" in hdr


def test_knob_default_the_gpu_tests_restore_is_the_shipped_one():
    """tests/test_gpu_gsm_two_launch.py forces the knob on and puts KNOB_DEFAULT back: that constant is the context's default."""
    import ast
    ctx = open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_ctx.h")).read()
    shipped = int(re.search(r"int\s+tune_gsm_two_launch\s*=\s*(\d+)\s*;", ctx).group(1))
    src = open(os.path.join(ROOT, "tests", "test_gpu_gsm_two_launch.py")).read()
    mirrored = int(re.search(r"^KNOB_DEFAULT\s*=\s*(\d+)", src, re.M).group(1))
    assert ast.parse(src) is not None and mirrored == shipped
