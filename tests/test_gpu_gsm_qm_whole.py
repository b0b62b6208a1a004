"""Whole-sample Qm on the two-slab route of the two-launch dense GSM update (knob "panel_qm_whole"; D = 1024, B in {16, 32}): the
product's idle slab-1 workgroups write ONE (mu0 - x_b).g_b per sample (k_panel_fast<.., PART, QMW>) and every covariance
workgroup loads that value instead of re-summing D / 16 pieces (k_gsm_cov_sym<.., QMW>).  The sum is ordered differently, so mu
and S differ from knob 0 at rounding level: there is no threshold between the two (the difference is printed), each is held
against the pinned oracle at the route's bound (rel_err < 1e-11), S must equal its transpose exactly, the result must repeat
bit for bit, and it must not depend on what other routes left in the workspace."""
import os
import re

import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-11
SHAPES = [(1024, 32), (1024, 16)]
KNOB = "panel_qm_whole"
_CACHE = {}
_CTX_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsm-vi_amd", "csrc", "gsmvi_ctx.h")
with open(_CTX_H) as _f:
    KNOB_DEFAULT = int(re.search(rf"int\s+tune_{KNOB}\s*=\s*(\d+)\s*;", _f.read()).group(1))


@pytest.fixture(scope="module")
def eng():
    import gsmvi_amd
    e = gsmvi_amd.get_engine()
    e.set_tuning("gsm_two_launch", 1)
    e.set_tuning("panel_kc", 0)
    yield e
    e.set_tuning(KNOB, KNOB_DEFAULT)
    e.set_tuning("panel_kc", 0)
    e.set_tuning("gsm_two_launch", 1)


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


def _run(eng, args, knob, **other):
    try:
        eng.set_tuning(KNOB, knob)
        for k, v in other.items():
            eng.set_tuning(k, v)
        eng.last_path()
        mu, S = eng.gsm_update(*args)
        return mu, S, eng.last_path()
    finally:
        eng.set_tuning(KNOB, KNOB_DEFAULT)
        eng.set_tuning("panel_kc", 0)
        eng.set_tuning("gsm_two_launch", 1)


@pytest.mark.parametrize("D,B", SHAPES)
def test_knob_on_against_the_oracle_and_knob_off(eng, D, B):
    import torch
    c = _case(D, B)
    args = _dev(eng, c)
    mu0, S0, p0 = _run(eng, args, 0)
    mu1, S1, p1 = _run(eng, args, 1)
    assert "gsm_two_launch" in p0 and KNOB not in p0, p0
    assert {"gsm_two_launch", "panel_chunk512", "cov_sym", KNOB} <= p1, p1
    print(f"({D}, {B}) knob 1 against knob 0: max |dmu| {float((mu1 - mu0).abs().max()):.3e} max |dS| {float((S1 - S0).abs().max()):.3e} "
          f"(max |mu| {float(mu0.abs().max()):.3e} max |S| {float(S0.abs().max()):.3e})")
    e_mu, e_S = rel_err(mu1.cpu().numpy(), c["mu_o"]), rel_err(S1.cpu().numpy(), c["S_o"])
    print(f"rel_err mu {e_mu:.3e} S {e_S:.3e}")
    assert e_mu < TOL and e_S < TOL, (e_mu, e_S)
    assert torch.equal(S1, S1.T)
    assert bool(torch.isfinite(S1).all()) and bool(torch.isfinite(mu1).all())


@pytest.mark.parametrize("D,B", SHAPES)
def test_repeats_bit_for_bit(eng, D, B):
    import torch
    args = _dev(eng, _case(D, B))
    mu, S, _ = _run(eng, args, 1)
    first = (mu.clone(), S.clone())
    for _ in range(7):
        mu, S, _ = _run(eng, args, 1)
        assert torch.equal(mu, first[0]) and torch.equal(S, first[1])


def test_workspace_layout_between_routes(eng):
    """A three-launch call, a 256-row-chunk call (per-strip Qm) and a knob-0 call over the same workspace in between: the
    knob-1 result is unchanged."""
    import torch
    args = _dev(eng, _case(1024, 32))
    mu, S, path = _run(eng, args, 1)
    assert KNOB in path, path
    first = (mu.clone(), S.clone())
    _, _, p3 = _run(eng, args, 1, gsm_two_launch=0)
    assert "gsm_two_launch" not in p3 and KNOB not in p3, p3
    _, _, p4 = _run(eng, args, 1, panel_kc=4)
    assert "gsm_two_launch" in p4 and "panel_chunk512" not in p4 and KNOB not in p4, p4
    _, _, p0 = _run(eng, args, 0)
    assert "panel_chunk512" in p0 and KNOB not in p0, p0
    mu, S, path = _run(eng, args, 1)
    assert KNOB in path, path
    assert torch.equal(mu, first[0]) and torch.equal(S, first[1])


def test_gated_out_shapes_never_carry_the_bit(eng):
    from oracle import gsm_oracle as orc
    for D, B in ((512, 32), (1024, 64)):
        st = orc.make_update_state(D, B, 5)
        _, _, path = _run(eng, tuple(eng.asarray(st[k]) for k in ("samples", "vs", "mu0", "S0")), 1)
        assert KNOB not in path, (D, B, path)
