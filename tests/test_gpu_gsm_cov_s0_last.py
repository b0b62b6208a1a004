"""The two-slab covariance launch of the two-launch dense GSM update (D = 1024, B in {16, 32}; k_gsm_cov_sym<.., FROM_SLABS, 2, ..>)
with its Sigma0 tile issued and waited for LAST (knob "cov_s0_last") and with write-through stores of Sigma' (knob
"cov_store_wt").  Both forms run the same operations on the same values in the same order, so knob 1 must equal knob 0 of
the same build BIT FOR BIT (torch.equal on mu and S), with the fold knob at 0, 1 and 2; S must equal its transpose exactly and
stay within 1e-11 of the pinned oracle (the bound of tests/test_gpu_gsm_two_launch.py for this route).  A wait placed too early
costs time only; a wait placed too LATE reads a register before its load has landed, which shows as soon as Sigma0 really comes
from HBM: the cold case runs 20 independent instances (about 320 MB of Sigma0 and Sigma) round-robin.  KCT = 2 runs nowhere
below D = 1024, so these are the smallest shapes."""
import os
import re

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-11
SHAPES = [(1024, 32), (1024, 16)]
KNOBS = ["cov_s0_last", "cov_store_wt"]
_CACHE = {}
_CTX_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsm-vi_amd", "csrc", "gsmvi_ctx.h")


def _default(name):
    """The shipped default of a knob: `int tune_<name> = <n>;` in csrc/gsmvi_ctx.h (tests/test_gsm_cov_s0_last_cpu.py holds
    those against DESIGN.md)."""
    with open(_CTX_H) as f:
        return int(re.search(rf"int\s+tune_{name}\s*=\s*(\d+)\s*;", f.read()).group(1))


DEFAULTS = {k: _default(k) for k in KNOBS + ["cov_fold_diag"]}


@pytest.fixture(scope="module")
def eng():
    import gsmvi_amd
    e = gsmvi_amd.get_engine()
    e.set_tuning("gsm_two_launch", 1)
    e.set_tuning("panel_kc", 0)
    yield e
    for k, v in DEFAULTS.items():
        e.set_tuning(k, v)


def _case(D, B, seed=0):
    """Inputs and oracle result of one shape (as tests/test_gpu_gsm_two_launch.py::_case), computed once and never modified."""
    key = (D, B, seed)
    if key not in _CACHE:
        from oracle import gsm_oracle as orc
        st = orc.make_update_state(D, B, seed + 3 * D + B)
        mu_o, S_o = orc.gsm_update_batched(st["samples"], st["vs"], st["mu0"], st["S0"])
        _CACHE[key] = dict(X=st["samples"], G=st["vs"], mu0=st["mu0"], S0=st["S0"], mu_o=mu_o, S_o=S_o)
    return _CACHE[key]


def _dev(eng, c):
    return tuple(eng.asarray(c[k]) for k in ("X", "G", "mu0", "S0"))


def _run(eng, args, knobs, out=None):
    """One update with the given knobs (the others at 0), every knob restored to its default afterwards."""
    try:
        for k in KNOBS:
            eng.set_tuning(k, 0)
        for k, v in knobs.items():
            eng.set_tuning(k, v)
        eng.last_path()
        mu, S = eng.gsm_update(*args, out=out)
        return mu, S, eng.last_path()
    finally:
        for k, v in DEFAULTS.items():
            eng.set_tuning(k, v)
        eng.set_tuning("panel_kc", 0)


@pytest.mark.parametrize("fold", [0, 1, 2])
@pytest.mark.parametrize("D,B", SHAPES)
@pytest.mark.parametrize("knob", KNOBS + ["both"])
def test_knob_on_equals_knob_off_bit_for_bit(eng, knob, D, B, fold):
    import torch
    c = _case(D, B)
    args = _dev(eng, c)
    on = {k: 1 for k in KNOBS} if knob == "both" else {knob: 1}
    mu0, S0, p0 = _run(eng, args, {"cov_fold_diag": fold})
    mu1, S1, p1 = _run(eng, args, {"cov_fold_diag": fold, **on})
    assert "gsm_two_launch" in p0 and not (set(KNOBS) & p0), p0
    assert {"gsm_two_launch", "cov_sym", "panel_chunk512"} <= p1 and set(KNOBS) & p1 == set(on), p1
    assert ("cov_fold_diag" in p1) == (fold > 0), p1
    print(f"({D}, {B}) {knob} fold {fold}: max |dmu| {float((mu1 - mu0).abs().max()):.3e} max |dS| {float((S1 - S0).abs().max()):.3e}")
    assert torch.equal(mu1, mu0)
    assert torch.equal(S1, S0)
    assert torch.equal(S1, S1.T)
    e_mu, e_S = rel_err(mu1.cpu().numpy(), c["mu_o"]), rel_err(S1.cpu().numpy(), c["S_o"])
    print(f"rel_err mu {e_mu:.3e} S {e_S:.3e}")
    assert e_mu < TOL and e_S < TOL, (e_mu, e_S)


def test_path_bits_only_where_the_form_ran(eng):
    from oracle import gsm_oracle as orc
    on = {k: 1 for k in KNOBS}
    _, _, path = _run(eng, _dev(eng, _case(1024, 32)), on)
    assert set(KNOBS) <= path, path
    for D, B in ((512, 32), (1024, 64)):                       # KCT = 4 instance; three launches
        st = orc.make_update_state(D, B, 5)
        _, _, path = _run(eng, tuple(eng.asarray(st[k]) for k in ("samples", "vs", "mu0", "S0")), on)
        assert not (set(KNOBS) & path), (D, B, path)
    _, _, path = _run(eng, _dev(eng, _case(1024, 32)), {"panel_kc": 4, **on})   # 256-row chunks: the KCT = 4 instance
    assert "gsm_two_launch" in path and "panel_chunk512" not in path and not (set(KNOBS) & path), path


@pytest.mark.parametrize("knob", KNOBS)
def test_padded_leading_dimensions(eng, knob):
    """Sigma0 and Sigma with leading dimension D + 2 (NaN in the padding): the late loads use lds0, the write-through stores lds."""
    import torch
    D, B = 1024, 32
    c = _case(D, B)
    X, G, mu0, S0 = _dev(eng, c)

    def wide(t, ld):
        buf = torch.full((t.shape[0], ld), float("nan"), dtype=torch.float64, device="cuda")
        v = buf[:, :t.shape[1]]
        v.copy_(t)
        return v, buf

    ref_mu, ref_S, _ = _run(eng, (X, G, mu0, S0), {})
    Sv, Sbuf = wide(eng.zeros(D, D), D + 2)
    mu, S, path = _run(eng, (X, G, mu0, wide(S0, D + 2)[0]), {knob: 1}, out=(eng.empty(D), Sv))
    assert {"gsm_two_launch", knob} <= path, path
    assert S.data_ptr() == Sv.data_ptr()
    assert torch.equal(mu, ref_mu) and torch.equal(S, ref_S) and torch.equal(S, S.T)
    assert bool(torch.isnan(Sbuf[:, D:]).all())               # nothing was written beyond column D
    assert rel_err(S.cpu().numpy(), c["S_o"]) < TOL


@pytest.mark.parametrize("knob", KNOBS)
def test_repeats_and_graph_replay(eng, knob):
    """The same call 8 times, and a captured graph replayed 3 times into zeroed outputs: every result equals the first."""
    import torch
    args = _dev(eng, _case(1024, 32))
    out = (eng.empty(1024), eng.empty(1024, 1024))
    try:
        eng.set_tuning(knob, 1)
        mu, S = eng.gsm_update(*args, out=out)
        first = (mu.clone(), S.clone())
        for _ in range(7):
            out[0].zero_(), out[1].zero_()
            eng.gsm_update(*args, out=out)
            assert torch.equal(out[0], first[0]) and torch.equal(out[1], first[1])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.gsm_update(*args, out=out)
        for _ in range(3):
            out[0].zero_(), out[1].zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out[0], first[0]) and torch.equal(out[1], first[1])
    finally:
        eng.set_tuning(knob, DEFAULTS[knob])
    ref_mu, ref_S, _ = _run(eng, args, {})
    assert torch.equal(first[0], ref_mu) and torch.equal(first[1], ref_S)


@pytest.mark.parametrize("knob", KNOBS)
def test_cold_sigma0(eng, knob):
    """20 instances, each with its own Sigma0 and Sigma (about 320 MB, beyond the Infinity Cache), round-robin twice: Sigma0
    comes from HBM, where a wait that does not cover its load would show."""
    import torch
    D, B, n = 1024, 32, 20
    X, G, mu0, S0 = _dev(eng, _case(D, B))
    S0s = [S0 * (1.0 + k / 64.0) for k in range(n)]            # symmetric positive definite, all different
    outs = [(eng.empty(D), eng.empty(D, D)) for _ in range(n)]
    ref = []
    for k in range(n):
        mu, S, _ = _run(eng, (X, G, mu0, S0s[k]), {}, out=outs[k])
        ref.append((mu.clone(), S.clone()))
    for mu, S in outs:
        mu.zero_(), S.zero_()
    try:
        eng.set_tuning(knob, 1)
        for rnd in range(2):
            for k in range(n):
                eng.gsm_update(X, G, mu0, S0s[k], out=outs[k])
            torch.cuda.synchronize()
            for k in range(n):
                assert torch.equal(outs[k][0], ref[k][0]) and torch.equal(outs[k][1], ref[k][1]), (rnd, k)
    finally:
        eng.set_tuning(knob, DEFAULTS[knob])
    assert not torch.equal(ref[0][1], ref[1][1])              # the instances do differ
