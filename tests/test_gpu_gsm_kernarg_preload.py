"""The preloaded entry points of the two-launch dense GSM update (gsmvi_fast_hot.hip, knob "kernarg_preload"): both launches take
what their first load batch needs from SGPRs that arrive with the wave, the rest of the argument block behind the first vector
loads.  The bodies are the ones of the other entry points, one copy, so everything the two launches write is the same BYTES with
the knob at 0 and at 1.  Shapes: the smallest and the largest that the gate passes, the two instance families of the covariance
launch (four slabs at D = 256, two at D = 1024).  Bound against the pinned oracle: rel_err < 1e-11, the bar of
tests/test_gpu_gsm_two_slab.py."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-11
SHAPES = [(256, 16), (256, 32), (1024, 16), (1024, 32)]
KNOB = "kernarg_preload"
_CACHE = {}
with open(os.path.join(ROOT, "gsm-vi_amd", "csrc", "gsmvi_ctx.h")) as _f:
    _CTX = _f.read()


def _default(knob):
    return int(re.search(rf"int\s+tune_{knob}\s*=\s*(\d+)\s*;", _CTX).group(1))


KNOB_DEFAULT = _default(KNOB)
OTHER = {k: _default(k) for k in ("panel_stream", "cov_wave_store", "panel_kc", "panel_qm_whole", "gsm_two_launch")}


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


@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("D,B", SHAPES)
def test_same_bytes_as_knob_0_and_oracle_parity(eng, D, B, pad):
    """Contiguous arrays and leading dimensions D + 2, with "panel_stream" at 0, 1, 4 and "cov_wave_store" at 0, 1."""
    import torch
    c = _case(D, B)
    X, G, mu0, S0 = _dev(eng, c)
    if pad:
        X, G, S0 = _wide(X, D + pad), _wide(G, D + pad), _wide(S0, D + pad)

    def out():
        return (eng.empty(D), _wide(eng.zeros(D, D), D + pad) if pad else eng.empty(D, D))

    for ps in (0, 1, 4):
        for ws in (0, 1):
            mu_0, S_0, p0 = _run(eng, (X, G, mu0, S0), 0, out=out(), panel_stream=ps, cov_wave_store=ws)
            mu_1, S_1, p1 = _run(eng, (X, G, mu0, S0), 1, out=out(), panel_stream=ps, cov_wave_store=ws)
            assert {"gsm_two_launch", "panel_fast", "cov_sym"} <= p0 and "scalars_fast" not in p0, p0
            assert p1 == p0, (p1, p0)
            assert torch.equal(mu_1, mu_0) and torch.equal(S_1, S_0), (ps, ws)
            assert torch.equal(S_1, S_1.T), (ps, ws)
    e_mu, e_S = rel_err(mu_1.cpu().numpy(), c["mu_o"]), rel_err(S_1.cpu().numpy(), c["S_o"])
    print(f"({D}, {B}) ld + {pad}: rel_err mu {e_mu:.3e} S {e_S:.3e}")
    assert e_mu < TOL and e_S < TOL, (e_mu, e_S)


@pytest.mark.parametrize("D,B", SHAPES)
def test_graph_replay_equals_eager(eng, D, B):
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
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kernarg_preload_worker.py"), mode, str(D), str(B)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and f"kernarg preload {mode} ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-1500:])


@pytest.mark.parametrize("D,B", SHAPES)
def test_workspace_bytes_and_stamps(D, B):
    """Slabs, Qg and Qm read back from the workspace hold the same bytes at knob 0 and 1; with the timeline diagnostic on, every stamp
    word of every workgroup of both launches is nonzero and ordered.  Through the debug library, which a process selects when it
    loads the package: a child process (tests/kernarg_preload_worker.py)."""
    _worker("debug", D, B, True)


def test_a_shape_the_gate_refuses(eng):
    """D = 320, B = 32 takes three launches: the same bytes and the same path set with the knob at 0 and at 1."""
    import torch
    from oracle import gsm_oracle as orc
    st = orc.make_update_state(320, 32, 5)
    args = tuple(eng.asarray(st[k]) for k in ("samples", "vs", "mu0", "S0"))
    mu_0, S_0, p0 = _run(eng, args, 0)
    mu_1, S_1, p1 = _run(eng, args, 1)
    assert "gsm_two_launch" not in p0 and p1 == p0, (p0, p1)
    assert torch.equal(mu_1, mu_0) and torch.equal(S_1, S_0)


@pytest.mark.parametrize("D,B", SHAPES)
def test_arrays_at_the_end_of_their_mapping(D, B):
    """One update with the knob at 1, every input and output array at the end of a freshly mapped allocation."""
    _worker("tail", D, B, False)
