"""The dense GSM update in TWO launches (B in {16, 32}, D % 256 == 0, D <= 1024, aligned operands): the product launch leaves
partial dots beside its split-K slabs (k_panel_fast<.., PART>) and the covariance launch forms its factor tiles from samples, slabs
and partials (k_gsm_cov_sym<.., FROM_SLABS>) -- no per-sample launch, no records, no in-launch hand-off.  Every other shape, layout
or knob setting keeps the three launches.  Bound: rel_err < 1e-11 against the pinned oracle, the bar of every dense-update test
(tests/test_gpu_gsm_update.py, tests/test_gpu_offgrid.py); the two routes are NOT compared against each other with a threshold
(their gSg sums are ordered differently: last-bit differences are expected), the largest difference is printed."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-11
# KC = 1, 2, 3, 4 slabs; even and odd tile counts per row (two-tile and single-tile workgroups); SB = 16 and 32
SHAPES = [(256, 16), (256, 32), (512, 32), (768, 32), (1024, 16), (1024, 32)]
GATED_OUT = [(1024, 20), (1000, 32), (1024, 64), (2048, 32)]
_CACHE = {}


KNOB_DEFAULT = 1          # `int tune_gsm_two_launch = 1;` in csrc/gsmvi_ctx.h (tests/test_gsm_two_launch_cpu.py holds the two together)


@pytest.fixture(scope="module")
def eng():
    """The shared engine with the knob forced on for this module (whatever the shipped default), restored afterwards."""
    import gsmvi_amd
    e = gsmvi_amd.get_engine()
    e.set_tuning("gsm_two_launch", 1)
    yield e
    e.set_tuning("gsm_two_launch", KNOB_DEFAULT)


def _case(D, B, seed=0):
    """Inputs and oracle result of one shape, computed once per module and never modified."""
    key = (D, B, seed)
    if key not in _CACHE:
        from oracle import gsm_oracle as orc
        st = orc.make_update_state(D, B, seed + 3 * D + B)
        mu_o, S_o = orc.gsm_update_batched(st["samples"], st["vs"], st["mu0"], st["S0"])
        _CACHE[key] = dict(X=st["samples"], G=st["vs"], mu0=st["mu0"], S0=st["S0"], mu_o=mu_o, S_o=S_o)
    return _CACHE[key]


def _dev(eng, c):
    return tuple(eng.asarray(c[k]) for k in ("X", "G", "mu0", "S0"))


def _run(eng, args, out=None):
    eng.last_path()
    mu, S = eng.gsm_update(*args, out=out)
    return mu, S, eng.last_path()


def _check(c, mu, S):
    mun, Sn = mu.cpu().numpy(), S.cpu().numpy()
    e_mu, e_S = rel_err(mun, c["mu_o"]), rel_err(Sn, c["S_o"])
    print(f"rel_err mu {e_mu:.3e} S {e_S:.3e}")
    assert e_mu < TOL and e_S < TOL, (e_mu, e_S)
    return mun, Sn


@pytest.mark.parametrize("D,B", SHAPES)
def test_parity_and_route(eng, D, B):
    c = _case(D, B)
    mu, S, path = _run(eng, _dev(eng, c))
    _, Sn = _check(c, mu, S)
    assert np.array_equal(Sn, Sn.T)
    assert {"gsm_two_launch", "panel_fast", "cov_sym"} <= path and "scalars_fast" not in path, path


@pytest.mark.parametrize("D,B", SHAPES)
def test_knob_off_runs_three_launches(eng, D, B):
    c = _case(D, B)
    args = _dev(eng, c)
    mu2, S2, path2 = _run(eng, args)
    try:
        eng.set_tuning("gsm_two_launch", 0)
        mu3, S3, path3 = _run(eng, args)
    finally:
        eng.set_tuning("gsm_two_launch", 1)                      # (the module runs with the knob on: fixture `eng`)
    assert "gsm_two_launch" in path2 and "gsm_two_launch" not in path3 and "scalars_fast" in path3, (path2, path3)
    _check(c, mu3, S3)
    _check(c, mu2, S2)
    d_mu = float((mu2 - mu3).abs().max())
    d_S = float((S2 - S3).abs().max())
    print(f"two-launch vs three-launch at ({D}, {B}): max |dmu| {d_mu:.3e}, max |dS| {d_S:.3e} "
          f"(max |S| {float(S3.abs().max()):.3e})")


def test_no_stale_workspace(eng):
    import torch
    big, mid, small, off = _case(1024, 32), _case(512, 32), _case(256, 16), _case(320, 12)
    a_big = _dev(eng, big)
    mu0_, S0_, p0 = _run(eng, a_big)
    first = (mu0_.clone(), S0_.clone())
    mu1, S1, _ = _run(eng, a_big)
    assert torch.equal(mu1, first[0]) and torch.equal(S1, first[1])              # the same call twice
    for c in (mid, small):
        mu, S, path = _run(eng, _dev(eng, c))
        assert "gsm_two_launch" in path, path
        _check(c, mu, S)
    mu_o3, S_o3, path = _run(eng, _dev(eng, off))                               # a three-launch call in between
    assert "gsm_two_launch" not in path and "scalars_fast" in path, path
    _check(off, mu_o3, S_o3)
    mu2, S2, path = _run(eng, a_big)
    assert "gsm_two_launch" in path and "gsm_two_launch" in p0
    assert torch.equal(mu2, first[0]) and torch.equal(S2, first[1])


def test_graph_capture(eng):
    import torch
    ring = [_dev(eng, _case(1024, 32, seed=s)) for s in (0, 1)]
    outs = [(eng.empty(1024), eng.empty(1024, 1024)) for _ in range(2)]
    eager = []
    for k in range(3):
        mu, S, path = _run(eng, ring[k % 2], out=outs[k % 2])
        assert "gsm_two_launch" in path, path
        eager.append((mu.clone(), S.clone()))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(3):
            eng.gsm_update(*ring[k % 2], out=outs[k % 2])
    for _ in range(2):
        for mu, S in outs:
            mu.zero_()
            S.zero_()
        g.replay()
        torch.cuda.synchronize()
        # instance 0 was written by updates 0 and 2 (same inputs), instance 1 by update 1
        assert torch.equal(outs[0][0], eager[2][0]) and torch.equal(outs[0][1], eager[2][1])
        assert torch.equal(outs[1][0], eager[1][0]) and torch.equal(outs[1][1], eager[1][1])
    assert torch.equal(eager[0][0], eager[2][0]) and torch.equal(eager[0][1], eager[2][1])


def test_layouts(eng):
    import torch
    D, B = 512, 32
    c = _case(D, B)
    X, G, mu0, S0 = _dev(eng, c)

    def wide(t, ld, off=0):
        buf = torch.full((t.shape[0], ld), float("nan"), dtype=torch.float64, device="cuda")
        v = buf[:, off:off + t.shape[1]]
        v.copy_(t)
        return v

    # padded leading dimensions (even) and row slices of wider arrays: still two launches
    out = (eng.empty(D), wide(eng.zeros(D, D), D + 2))
    mu, S, path = _run(eng, (wide(X, D + 6), wide(G, D + 4), mu0, wide(S0, D + 2)), out=out)
    assert "gsm_two_launch" in path and "scalars_fast" not in path, path
    _, Sn = _check(c, mu, S)
    assert np.array_equal(Sn, Sn.T)
    # an odd leading dimension, or a pointer offset by 8 bytes: three launches
    for args in ((wide(X, D + 3), G, mu0, S0), (X, wide(G, D + 2, off=1), mu0, S0), (X, G, mu0, wide(S0, D + 1)),
                 (wide(X, D + 2, off=1), G, mu0, S0)):
        mu, S, path = _run(eng, args)
        assert "gsm_two_launch" not in path, path
        _check(c, mu, S)
    out = (eng.empty(D), wide(eng.zeros(D, D), D + 2, off=1))
    mu, S, path = _run(eng, (X, G, mu0, S0), out=out)
    assert "gsm_two_launch" not in path, path
    _check(c, mu, S)


@pytest.mark.parametrize("D,B", GATED_OUT)
def test_gate_keeps_other_shapes_on_three_launches(eng, D, B):
    c = _case(D, B)
    mu, S, path = _run(eng, _dev(eng, c))
    assert "scalars_fast" in path and "gsm_two_launch" not in path, path
    _check(c, mu, S)


def test_profile_slots(eng):
    big, off = _dev(eng, _case(1024, 32)), _dev(eng, _case(320, 12))
    eng.set_profiling(True)
    try:
        eng.gsm_update(*big)
        p2 = eng.get_profile()
        eng.gsm_update(*off)                      # three launches: leaves slot 1 valid
        p3 = eng.get_profile()
        eng.gsm_update(*big)
        p2b = eng.get_profile()
    finally:
        eng.set_profiling(False)
    print(p2, p3, p2b)
    for p in (p2, p2b):
        assert 0 < p["panel"] < 50 and 0 < p["cov_update"] < 50 and p["scalars"] == -1, p
    assert all(0 < v < 50 for v in p3.values()), p3
