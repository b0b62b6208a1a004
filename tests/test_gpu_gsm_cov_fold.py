"""The covariance launch of the two-launch dense GSM update with the diagonal leftover tiles folded into two-tile workgroups
(k_gsm_cov_sym<.., FROM_SLABS, .., FOLD>, knob "cov_fold_diag": 0 = the leftovers are workgroups of their own, 1 = folded where
the two-tile workgroups alone fill the device (D = 1024), 2 = folded at every two-launch shape).  The folded tile runs the same
MFMA chains on the same staged values, so every result must equal the knob = 0 result of the same build BIT FOR BIT
(torch.equal on mu and S), S must equal its transpose exactly, and last_path() carries "cov_fold_diag" only when folding ran.
D = 256 (nt = 8: 16 workgroups instead of 20) has both kinds of host: rows 1, 3, 5 fold into the first pair of their row, row 7
into the pair of row 6.  One case is also held against the pinned oracle at the bound of tests/test_gpu_gsm_two_slab.py for
this route (rel_err < 1e-11)."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-11
KNOB_DEFAULT = 1          # `int tune_cov_fold_diag = 1;` in csrc/gsmvi_ctx.h (tests/test_gsm_cov_fold_cpu.py checks it)
# (D, B, knob, folds)
CASES = [(256, 16, 2, True), (256, 32, 2, True), (512, 32, 2, True), (1024, 32, KNOB_DEFAULT, True), (1024, 16, KNOB_DEFAULT, True)]
_CACHE = {}


@pytest.fixture(scope="module")
def eng():
    import gsmvi_amd
    e = gsmvi_amd.get_engine()
    e.set_tuning("gsm_two_launch", 1)
    e.set_tuning("panel_kc", 0)
    e.set_tuning("cov_fold_diag", KNOB_DEFAULT)
    yield e
    e.set_tuning("cov_fold_diag", KNOB_DEFAULT)


def _case(D, B):
    """Inputs and oracle result of one shape, computed once per module and never modified."""
    if (D, B) not in _CACHE:
        from oracle import gsm_oracle as orc
        st = orc.make_update_state(D, B, 7 + 3 * D + B)
        mu_o, S_o = orc.gsm_update_batched(st["samples"], st["vs"], st["mu0"], st["S0"])
        _CACHE[(D, B)] = dict(X=st["samples"], G=st["vs"], mu0=st["mu0"], S0=st["S0"], mu_o=mu_o, S_o=S_o)
    return _CACHE[(D, B)]


def _run(eng, args, knob, out=None):
    try:
        eng.set_tuning("cov_fold_diag", knob)
        eng.last_path()
        mu, S = eng.gsm_update(*args, out=out)
        return mu, S, eng.last_path()
    finally:
        eng.set_tuning("cov_fold_diag", KNOB_DEFAULT)


@pytest.mark.parametrize("D,B,knob,folds", CASES)
def test_folded_equals_unfolded_bit_for_bit(eng, D, B, knob, folds):
    import torch
    c = _case(D, B)
    args = tuple(eng.asarray(c[k]) for k in ("X", "G", "mu0", "S0"))
    mu0, S0, p0 = _run(eng, args, 0)
    mu1, S1, p1 = _run(eng, args, knob)
    assert "gsm_two_launch" in p0 and "cov_fold_diag" not in p0, p0
    assert {"gsm_two_launch", "cov_sym"} <= p1 and ("cov_fold_diag" in p1) == folds, p1
    print(f"({D}, {B}) knob {knob}: max |dmu| {float((mu1 - mu0).abs().max()):.3e} max |dS| {float((S1 - S0).abs().max()):.3e}")
    assert torch.equal(mu1, mu0)
    assert torch.equal(S1, S0)
    assert torch.equal(S1, S1.T) and torch.equal(S0, S0.T)
    assert bool(torch.isfinite(S1).all()) and bool(torch.isfinite(mu1).all())


def test_default_knob_folds_only_where_the_pairs_fill_the_device(eng):
    for D, B in ((256, 16), (512, 32)):
        c = _case(D, B)
        _, _, path = _run(eng, tuple(eng.asarray(c[k]) for k in ("X", "G", "mu0", "S0")), KNOB_DEFAULT)
        assert "gsm_two_launch" in path and "cov_fold_diag" not in path, path


def test_gated_out_shape_never_carries_the_bit(eng):
    from oracle import gsm_oracle as orc
    st = orc.make_update_state(256, 20, 5)                     # B = 20: three launches
    args = tuple(eng.asarray(st[k]) for k in ("samples", "vs", "mu0", "S0"))
    _, _, path = _run(eng, args, 2)
    assert "gsm_two_launch" not in path and "cov_fold_diag" not in path, path


def test_against_the_oracle(eng):
    D, B = 256, 32
    c = _case(D, B)
    mu, S, path = _run(eng, tuple(eng.asarray(c[k]) for k in ("X", "G", "mu0", "S0")), 2)
    assert "cov_fold_diag" in path, path
    e_mu, e_S = rel_err(mu.cpu().numpy(), c["mu_o"]), rel_err(S.cpu().numpy(), c["S_o"])
    print(f"rel_err mu {e_mu:.3e} S {e_S:.3e}")
    assert e_mu < TOL and e_S < TOL, (e_mu, e_S)


def test_padded_leading_dimensions(eng):
    """Leading dimension D + 2 for X, G, S0 and S (NaN in the padding): the folded tile's loads and its store use lds0 / lds."""
    import torch
    D, B = 256, 32
    c = _case(D, B)
    X, G, mu0, S0 = (eng.asarray(c[k]) for k in ("X", "G", "mu0", "S0"))

    def wide(t, ld):
        buf = torch.full((t.shape[0], ld), float("nan"), dtype=torch.float64, device="cuda")
        v = buf[:, :t.shape[1]]
        v.copy_(t)
        return v, buf

    args = (wide(X, D + 2)[0], wide(G, D + 2)[0], mu0, wide(S0, D + 2)[0])
    ref_mu, ref_S, _ = _run(eng, (X, G, mu0, S0), 0)
    Sv, Sbuf = wide(eng.zeros(D, D), D + 2)
    mu, S, path = _run(eng, args, 2, out=(eng.empty(D), Sv))
    assert {"gsm_two_launch", "cov_fold_diag"} <= path, path
    assert S.data_ptr() == Sv.data_ptr()
    assert torch.equal(mu, ref_mu) and torch.equal(S, ref_S) and torch.equal(S, S.T)
    assert bool(torch.isnan(Sbuf[:, D:]).all())              # nothing was written beyond column D
    e_S = rel_err(S.cpu().numpy(), c["S_o"])
    assert e_S < TOL, e_S
