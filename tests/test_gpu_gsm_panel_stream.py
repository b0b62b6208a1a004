"""The streamed left operand of the two-slab product of the two-launch dense GSM update (k_panel_fast<.., 512, .., PART, .., STREAM>,
knob "panel_stream"; D = 1024, B in {16, 32} -- the only shapes that reach the instance): every wave loads the part of G that it
multiplies, in stages along K, and starts a stage's MFMAs behind that stage's loads, with no workgroup barrier in front.  The same
products enter the same accumulators in the same order, so everything the launch writes is the same BYTES as with the knob at 0
(1 and 2 = two stages, 4 = four).  Bound against the pinned oracle: rel_err < 1e-11, the bar of tests/test_gpu_gsm_two_slab.py."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-11
SHAPES = [(1024, 32), (1024, 16)]
KNOB = "panel_stream"
_CACHE = {}
with open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_ctx.h")) as _f:
    KNOB_DEFAULT = int(re.search(rf"int\s+tune_{KNOB}\s*=\s*(\d+)\s*;", _f.read()).group(1))
OTHER = {"panel_kc": 0, "panel_qm_whole": 0, "gsm_two_launch": 1}


@pytest.fixture(scope="module")
def eng():
    import gsmvi_amd
    e = gsmvi_amd.get_engine()
    for k, v in OTHER.items():
        e.set_tuning(k, v)
    yield e
    e.set_tuning(KNOB, KNOB_DEFAULT)
    for k, v in OTHER.items():
        e.set_tuning(k, v)


def _case(D, B):
    """Inputs and oracle result of one shape (as tests/test_gpu_gsm_two_slab.py::_case), computed once and never modified."""
    key = (D, B)
    if key not in _CACHE:
        from oracle import gsm_oracle as orc
        st = orc.make_update_state(D, B, 3 * D + B)
        mu_o, S_o = orc.gsm_update_batched(st["samples"], st["vs"], st["mu0"], st["S0"])
        _CACHE[key] = dict(X=st["samples"], G=st["vs"], mu0=st["mu0"], S0=st["S0"], mu_o=mu_o, S_o=S_o)
    return _CACHE[key]


def _dev(eng, c):
    return tuple(eng.asarray(c[k]) for k in ("X", "G", "mu0", "S0"))


def _run(eng, args, knob, out=None, **other):
    try:
        eng.set_tuning(KNOB, knob)
        for k, v in other.items():
            eng.set_tuning(k, v)
        eng.last_path()
        mu, S = eng.gsm_update(*args, out=out)
        return mu, S, eng.last_path()
    finally:
        eng.set_tuning(KNOB, KNOB_DEFAULT)
        for k, v in OTHER.items():
            eng.set_tuning(k, v)


def _wide(t, ld):
    import torch
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=torch.float64, device="cuda")
    v = buf[:, :t.shape[1]]
    v.copy_(t)
    return v


@pytest.mark.parametrize("pad", [0, 2, 6])
@pytest.mark.parametrize("D,B", SHAPES)
def test_same_bytes_as_knob_0_and_oracle_parity(eng, D, B, pad):
    """(a), (b): contiguous arrays and padded even leading dimensions (ldx, ldg, lds0, lds = D + pad)."""
    import torch
    c = _case(D, B)
    X, G, mu0, S0 = _dev(eng, c)
    if pad:
        X, G, S0 = _wide(X, D + pad), _wide(G, D + pad), _wide(S0, D + pad)

    def out():
        return (eng.empty(D), _wide(eng.zeros(D, D), D + pad) if pad else eng.empty(D, D))

    mu_0, S_0, p0 = _run(eng, (X, G, mu0, S0), 0, out=out())
    assert {"gsm_two_launch", "panel_chunk512", "cov_sym"} <= p0 and "scalars_fast" not in p0, p0
    for knob in (1, 2, 4):
        mu_k, S_k, pk = _run(eng, (X, G, mu0, S0), knob, out=out())
        assert pk == p0, (pk, p0)
        assert torch.equal(mu_k, mu_0) and torch.equal(S_k, S_0), knob
    e_mu, e_S = rel_err(mu_k.cpu().numpy(), c["mu_o"]), rel_err(S_k.cpu().numpy(), c["S_o"])
    print(f"({D}, {B}) ld + {pad}: rel_err mu {e_mu:.3e} S {e_S:.3e}")
    assert e_mu < TOL and e_S < TOL, (e_mu, e_S)
    assert torch.equal(S_k, S_k.T)


@pytest.mark.parametrize("D,B", SHAPES)
def test_graph_replay_equals_eager(eng, D, B):
    """(c)"""
    import torch
    args = _dev(eng, _case(D, B))
    out = (eng.empty(D), eng.empty(D, D))
    try:
        eng.set_tuning(KNOB, 1)
        mu, S = eng.gsm_update(*args, out=out)
        eager = (mu.clone(), S.clone())
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.gsm_update(*args, out=out)
    finally:
        eng.set_tuning(KNOB, KNOB_DEFAULT)
    for _ in range(3):
        out[0].zero_()
        out[1].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


def _worker(mode, D, B, debug_lib):
    env = dict(os.environ)
    env["GSMVI_HIP_DEBUG_LIB"] = "1" if debug_lib else "0"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "panel_stream_worker.py"), mode, str(D), str(B)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and f"panel stream {mode} ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-1500:])


@pytest.mark.parametrize("D,B", SHAPES)
def test_workspace_bytes_stamps_and_path_bits(D, B):
    """(a) for the slabs, Qg and Qm read back from the workspace, and (d): with the timeline diagnostic on, the product's stamp words
    4 - 7 are nonzero and ordered with the knob at 1; the path bits are the same set at 0 and 1.  Through the debug library, which a
    process selects when it loads the package: a child process (tests/panel_stream_worker.py)."""
    _worker("debug", D, B, True)


def test_routes_the_knob_does_not_reach(eng):
    """(e): panel_kc=4 (256-row chunks), D = 768 and panel_qm_whole=1 give the same bytes with the knob at 0 and at 1."""
    import torch
    from oracle import gsm_oracle as orc
    args = _dev(eng, _case(1024, 32))
    st = orc.make_update_state(768, 32, 5)
    args768 = tuple(eng.asarray(st[k]) for k in ("samples", "vs", "mu0", "S0"))
    for a, other, want, miss in ((args, dict(panel_kc=4), "gsm_two_launch", "panel_chunk512"),
                                 (args768, {}, "gsm_two_launch", "panel_chunk512"),
                                 (args, dict(panel_qm_whole=1), "panel_qm_whole", None)):
        mu_0, S_0, p0 = _run(eng, a, 0, **other)
        mu_1, S_1, p1 = _run(eng, a, 1, **other)
        assert want in p0 and (miss is None or miss not in p0) and p1 == p0, (other, p0, p1)
        assert torch.equal(mu_1, mu_0) and torch.equal(S_1, S_0), other


@pytest.mark.parametrize("D,B", SHAPES)
def test_arrays_at_the_end_of_their_mapping(D, B):
    """(f): one update with the knob at 1, every input and output array at the end of a freshly mapped allocation."""
    _worker("tail", D, B, False)
