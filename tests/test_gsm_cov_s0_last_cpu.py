"""Host-side facts of the round-10 forms of the two-slab covariance launch (knobs "cov_s0_last", "cov_store_wt", "panel_qm_whole"): the new path
bits agree between include/gsmvi_hip.h and HipEngine.PATH_BITS and lie outside the generic mask, and the knob defaults of
csrc/gsmvi_ctx.h are the ones DESIGN.md states."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = {"cov_s0_last": ("GSMVI_PATH_COV_S0_LAST", 0x20000000), "cov_store_wt": ("GSMVI_PATH_COV_STORE_WT", 0x40000000),
        "panel_qm_whole": ("GSMVI_PATH_PANEL_QM_WHOLE", 0x80000000)}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_path_bits_agree_and_lie_outside_the_generic_mask():
    from gsmvi_amd.engine import HipEngine
    hdr = _read("include", "gsmvi_hip.h")
    mask = re.search(r"#define\s+GSMVI_PATH_GENERIC_MASK\s+\(([^)]*)\)", hdr).group(1)
    hdr_mask = 0
    for term in mask.split("|"):
        hdr_mask |= int(term.strip().rstrip("u"), 16)
    assert hdr_mask == HipEngine.PATH_GENERIC_MASK
    for name, (macro, bit) in BITS.items():
        assert HipEngine.PATH_BITS[name] == bit
        m = re.search(rf"#define\s+{macro}\s+(0x[0-9a-fA-F]+)u", hdr)
        assert m and int(m.group(1), 16) == bit, name
        assert not hdr_mask & bit and not HipEngine.PATH_GENERIC_MASK & bit
    assert len(set(HipEngine.PATH_BITS.values())) == len(HipEngine.PATH_BITS)
    # every path bit of the header is one the engine names, and the other way round
    hdr_bits = {int(v, 16) for v in re.findall(r"#define\s+GSMVI_PATH_(?!GENERIC_MASK)\w+\s+(0x[0-9a-fA-F]+)u", hdr)}
    assert hdr_bits == set(HipEngine.PATH_BITS.values())


def test_knob_defaults_match_design():
    ctx = _read("gsm-vi_amd", "csrc", "gsmvi_ctx.h")
    design = _read("DESIGN.md")
    abi = _read("gsm-vi_amd", "csrc", "gsmvi_abi.hip")
    for name in BITS:
        default = int(re.search(rf"int\s+tune_{name}\s*=\s*(\d+)\s*;", ctx).group(1))
        stated = re.search(rf"`{name}`\s*\(default\s+(\d+)\b", design)
        assert stated, f"DESIGN.md does not state the default of {name}"
        assert int(stated.group(1)) == default, name
        assert f'"{name}"' in abi                                # gsmvi_set_tuning knows the name
