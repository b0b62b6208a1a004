"""The two-launch dense GSM update at D = 1024 with TWO 512-row slabs (k_panel_fast<.., 512, .., PART> and
k_gsm_cov_sym<.., FROM_SLABS, 2>): the default route of (1024, 16) and (1024, 32) when "panel_kc" is not set.  An explicit
"panel_kc" keeps the 256-row chunks with that split (panel_kc=4: four slabs, the earlier route); D = 256, 512, 768 keep their
256-row chunks; everything the two-launch gate refuses keeps three launches.  Bound: rel_err < 1e-11 against the pinned oracle,
the bar of every dense-update test (inputs and oracle as tests/test_gpu_gsm_two_launch.py::_case).  The two splits are not
compared against each other with a threshold (their sums are ordered differently); the largest difference is printed."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-11
NEW = [(1024, 32), (1024, 16)]
OTHER_TWO_LAUNCH = [(256, 16), (512, 32), (768, 32)]
THREE_LAUNCH = [(1024, 20), (1024, 64)]
_CACHE = {}


@pytest.fixture(scope="module")
def eng():
    """The shared engine with the two-launch knob on and no explicit split, as shipped; left that way afterwards."""
    import gsmvi_amd
    e = gsmvi_amd.get_engine()
    e.set_tuning("gsm_two_launch", 1)
    e.set_tuning("panel_kc", 0)
    yield e
    e.set_tuning("panel_kc", 0)
    e.set_tuning("gsm_two_launch", 1)


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


def _run_forced(eng, args, kc=4):
    """The same call with an explicit split: 256-row chunks, kc slabs.  The knob goes back in a finally."""
    try:
        eng.set_tuning("panel_kc", kc)
        return _run(eng, args)
    finally:
        eng.set_tuning("panel_kc", 0)


def _check(c, mu, S):
    mun, Sn = mu.cpu().numpy(), S.cpu().numpy()
    e_mu, e_S = rel_err(mun, c["mu_o"]), rel_err(Sn, c["S_o"])
    print(f"rel_err mu {e_mu:.3e} S {e_S:.3e}")
    assert e_mu < TOL and e_S < TOL, (e_mu, e_S)
    return mun, Sn


@pytest.mark.parametrize("D,B", NEW)
def test_parity_and_route(eng, D, B):
    c = _case(D, B)
    mu, S, path = _run(eng, _dev(eng, c))
    _, Sn = _check(c, mu, S)
    assert np.array_equal(Sn, Sn.T)
    assert {"gsm_two_launch", "panel_chunk512", "cov_sym"} <= path and "scalars_fast" not in path, path


@pytest.mark.parametrize("D,B", NEW)
def test_forced_four_slab_route(eng, D, B):
    c = _case(D, B)
    args = _dev(eng, c)
    mu2, S2, path2 = _run(eng, args)
    mu4, S4, path4 = _run_forced(eng, args, 4)
    assert "panel_chunk512" in path2, path2
    assert "panel_chunk512" not in path4 and "gsm_two_launch" in path4 and "scalars_fast" not in path4, path4
    _check(c, mu4, S4)
    _check(c, mu2, S2)
    print(f"two slabs vs four slabs at ({D}, {B}): max |dmu| {float((mu2 - mu4).abs().max()):.3e}, "
          f"max |dS| {float((S2 - S4).abs().max()):.3e} (max |S| {float(S4.abs().max()):.3e})")
    _, _, path = _run(eng, args)                     # the knob is back: the default route again
    assert "panel_chunk512" in path, path


@pytest.mark.parametrize("D,B", OTHER_TWO_LAUNCH)
def test_other_two_launch_shapes_keep_256_row_chunks(eng, D, B):
    c = _case(D, B)
    mu, S, path = _run(eng, _dev(eng, c))
    assert "gsm_two_launch" in path and "panel_chunk512" not in path and "scalars_fast" not in path, path
    _check(c, mu, S)


@pytest.mark.parametrize("D,B", THREE_LAUNCH)
def test_gated_out_shapes_keep_three_launches(eng, D, B):
    c = _case(D, B)
    mu, S, path = _run(eng, _dev(eng, c))
    assert "scalars_fast" in path and "gsm_two_launch" not in path and "panel_chunk512" not in path, path
    _check(c, mu, S)


def test_workspace_layout_between_routes(eng):
    """Qm starts at Qg + B * 2 * strips on the new route and at Qg + B * 4 * strips on the four-slab one, in the same record
    area, and the slab count differs: nothing one route (or a three-launch call's records) leaves may reach the other."""
    import torch
    cP, cQ, off = _case(1024, 32, seed=0), _case(1024, 32, seed=1), _case(320, 12)
    P, Q = _dev(eng, cP), _dev(eng, cQ)

    def keep(r):
        return r[0].clone(), r[1].clone(), r[2]

    fresh_forced_P = keep(_run_forced(eng, P, 4))
    _run(eng, _dev(eng, off))                                   # records of a three-launch call over the same area
    fresh_new_P = keep(_run(eng, P))
    _run(eng, _dev(eng, off))
    fresh_new_Q = keep(_run(eng, Q))
    assert "panel_chunk512" not in fresh_forced_P[2] and "panel_chunk512" in fresh_new_P[2] and "panel_chunk512" in fresh_new_Q[2]
    _check(cP, *fresh_forced_P[:2])
    _check(cP, *fresh_new_P[:2])
    _check(cQ, *fresh_new_Q[:2])

    mu, S, path = _run_forced(eng, P, 4)
    assert "panel_chunk512" not in path and torch.equal(mu, fresh_forced_P[0]) and torch.equal(S, fresh_forced_P[1])
    mu, S, path = _run(eng, Q)
    assert "panel_chunk512" in path and torch.equal(mu, fresh_new_Q[0]) and torch.equal(S, fresh_new_Q[1])
    mu, S, path = _run(eng, P)
    assert "panel_chunk512" in path and torch.equal(mu, fresh_new_P[0]) and torch.equal(S, fresh_new_P[1])
    for _ in range(8):
        mu, S, path = _run(eng, Q)
        assert "panel_chunk512" in path and torch.equal(mu, fresh_new_Q[0]) and torch.equal(S, fresh_new_Q[1])


def test_graph_capture(eng):
    import torch
    args = _dev(eng, _case(1024, 32))
    out = (eng.empty(1024), eng.empty(1024, 1024))
    mu, S, path = _run(eng, args, out=out)
    assert "panel_chunk512" in path, path
    eager = (mu.clone(), S.clone())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.gsm_update(*args, out=out)
    for _ in range(3):
        out[0].zero_()
        out[1].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


def test_layouts(eng):
    import torch
    D, B = 1024, 32
    c = _case(D, B)
    X, G, mu0, S0 = _dev(eng, c)

    def wide(t, ld, off=0):
        buf = torch.full((t.shape[0], ld), float("nan"), dtype=torch.float64, device="cuda")
        v = buf[:, off:off + t.shape[1]]
        v.copy_(t)
        return v

    # leading dimension D + 2 for X, G, S0 and S: still the new route
    out = (eng.empty(D), wide(eng.zeros(D, D), D + 2))
    mu, S, path = _run(eng, (wide(X, D + 2), wide(G, D + 2), mu0, wide(S0, D + 2)), out=out)
    assert {"gsm_two_launch", "panel_chunk512"} <= path and "scalars_fast" not in path, path
    assert S.data_ptr() == out[1].data_ptr() and mu.data_ptr() == out[0].data_ptr()
    _, Sn = _check(c, mu, S)
    assert np.array_equal(Sn, Sn.T)
    # a base pointer offset by 8 bytes: three launches
    for args in ((wide(X, D + 2, off=1), G, mu0, S0), (X, wide(G, D + 2, off=1), mu0, S0), (X, G, mu0, wide(S0, D + 2, off=1))):
        mu, S, path = _run(eng, args)
        assert "gsm_two_launch" not in path and "panel_chunk512" not in path and "scalars_fast" in path, path
        _check(c, mu, S)
    out = (eng.empty(D), wide(eng.zeros(D, D), D + 2, off=1))
    mu, S, path = _run(eng, (X, G, mu0, S0), out=out)
    assert "gsm_two_launch" not in path and "panel_chunk512" not in path, path
    _check(c, mu, S)
