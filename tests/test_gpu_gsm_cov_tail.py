"""The hosts of the covariance launch of the two-launch dense GSM update (k_gsm_cov_sym<.., FROM_SLABS, .., FOLD>) after round 11:
mu0 of the mean epilogues is loaded with the first load batch (block X in a host, block I in a diagonal workgroup, both in the
workgroup that is both), and a host stores its folded tile in front of the mean of that tile's block.  Loads and stores moved;
no operation, value or order of a sum did.  So for every case
  * mu and S with the fold equal the "cov_fold_diag" = 0 result of the same build BIT FOR BIT (torch.equal),
  * S equals its transpose exactly,
  * mu and S are within the route's bound of the pinned oracle (rel_err < 1e-11, as tests/test_gpu_gsm_cov_fold.py),
  * mu is compared block by block, 32 entries each, so that a mu0 value taken from the wrong block names the block.
The inputs come from oracle.make_update_state, whose mu0 is drawn at random per case: a mu0 loaded from the wrong block cannot
pass the oracle bound by coincidence.
Shapes: (256, 16) and (256, 32) with knob 2 -- nt = 8, both kinds of host and the workgroup that is diagonal and host at once,
the KCT = 4 instances at SB = 16 and 32; (512, 32) with knob 2; (1024, 32) and (1024, 16) at every combination of "cov_s0_last"
and "cov_store_wt" -- the KCT = 2 instances.  (256, 32) and (1024, 32) run once more on views: S0 and S with leading dimension
D + 2, mu0 a 16-byte aligned view at a non-zero offset into a buffer that is NaN elsewhere."""
import os
import re

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-11
KNOBS = ["cov_s0_last", "cov_store_wt"]
_CACHE = {}
_CTX_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsm-vi_amd", "csrc", "gsmvi_ctx.h")


def _default(name):
    with open(_CTX_H) as f:
        return int(re.search(rf"int\s+tune_{name}\s*=\s*(\d+)\s*;", f.read()).group(1))


DEFAULTS = {k: _default(k) for k in KNOBS + ["cov_fold_diag"]}
# (D, B, fold knob, {knob: value}): the KCT = 4 instances take neither "cov_s0_last" nor "cov_store_wt"
CASES = [(256, 16, 2, {}), (256, 32, 2, {}), (512, 32, 2, {})]
CASES += [(1024, B, DEFAULTS["cov_fold_diag"] or 1, {"cov_s0_last": s, "cov_store_wt": w}) for B in (32, 16) for s in (0, 1) for w in (0, 1)]
VIEW_CASES = [(256, 32, 2, {}), (1024, 32, DEFAULTS["cov_fold_diag"] or 1, {k: DEFAULTS[k] for k in KNOBS})]


def _id(case):
    D, B, fold, knobs = case
    return f"{D}-{B}-fold{fold}" + "".join(f"-{k[4:]}{v}" for k, v in knobs.items())


@pytest.fixture(scope="module")
def eng():
    import gsmvi_amd
    e = gsmvi_amd.get_engine()
    e.set_tuning("gsm_two_launch", 1)
    e.set_tuning("panel_kc", 0)
    yield e
    for k, v in DEFAULTS.items():
        e.set_tuning(k, v)


def _case(D, B):
    """Inputs (random mu0) and oracle result of one shape, computed once per module and never modified."""
    if (D, B) not in _CACHE:
        from oracle import gsm_oracle as orc
        st = orc.make_update_state(D, B, 11 + 3 * D + B)
        mu_o, S_o = orc.gsm_update_batched(st["samples"], st["vs"], st["mu0"], st["S0"])
        assert np.unique(np.round(st["mu0"].reshape(-1, 32), 6), axis=0).shape[0] == D // 32    # every block of mu0 differs
        _CACHE[(D, B)] = dict(X=st["samples"], G=st["vs"], mu0=st["mu0"], S0=st["S0"], mu_o=mu_o, S_o=S_o)
    return _CACHE[(D, B)]


def _dev(eng, c):
    return tuple(eng.asarray(c[k]) for k in ("X", "G", "mu0", "S0"))


def _run(eng, args, fold, knobs, out=None):
    """One update with the given fold knob and knobs, every knob restored to its default afterwards."""
    try:
        eng.set_tuning("cov_fold_diag", fold)
        for k, v in knobs.items():
            eng.set_tuning(k, v)
        eng.last_path()
        mu, S = eng.gsm_update(*args, out=out)
        return mu, S, eng.last_path()
    finally:
        for k, v in DEFAULTS.items():
            eng.set_tuning(k, v)


def _assert_mu_blocks(mu, ref, what):
    """mu against ref, 32 entries at a time: the message names the blocks that differ."""
    import torch
    bad = [k for k in range(mu.numel() // 32) if not torch.equal(mu[32 * k:32 * k + 32], ref[32 * k:32 * k + 32])]
    assert not bad, f"mu differs from {what} in blocks {bad} (32 entries each) of {mu.numel() // 32}"


def _assert_mu_blocks_oracle(mu, mu_o):
    scale = np.abs(mu_o).max()
    err = np.abs(mu - mu_o).reshape(-1, 32).max(axis=1) / scale
    bad = [(k, float(e)) for k, e in enumerate(err) if not e < TOL]
    assert not bad, f"mu beyond {TOL} of the oracle in blocks (block, rel_err): {bad}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_folded_hosts_equal_unfolded_bit_for_bit_and_the_oracle(eng, case):
    import torch
    D, B, fold, knobs = case
    c = _case(D, B)
    args = _dev(eng, c)
    mu0, S0, p0 = _run(eng, args, 0, knobs)
    mu1, S1, p1 = _run(eng, args, fold, knobs)
    assert "gsm_two_launch" in p0 and "cov_fold_diag" not in p0, p0
    assert {"gsm_two_launch", "cov_sym", "cov_fold_diag"} <= p1, p1
    assert set(KNOBS) & p1 == {k for k, v in knobs.items() if v}, p1
    assert ("panel_chunk512" in p1) == (D == 1024), p1              # KCT = 2 at D = 1024, KCT = 4 below
    mu_n, S_n = mu1.cpu().numpy(), S1.cpu().numpy()
    e_mu, e_S = rel_err(mu_n, c["mu_o"]), rel_err(S_n, c["S_o"])
    print(f"{_id(case)}: max |dmu| {float((mu1 - mu0).abs().max()):.3e} max |dS| {float((S1 - S0).abs().max()):.3e} "
          f"rel_err mu {e_mu:.3e} S {e_S:.3e}")
    _assert_mu_blocks(mu1, mu0, "the unfolded result")
    assert torch.equal(mu1, mu0)
    assert torch.equal(S1, S0)
    assert torch.equal(S1, S1.T) and torch.equal(S0, S0.T)
    _assert_mu_blocks_oracle(mu_n, c["mu_o"])
    _assert_mu_blocks_oracle(mu0.cpu().numpy(), c["mu_o"])          # the diagonal workgroups of the unfolded grid prefetch too
    assert e_mu < TOL and e_S < TOL, (e_mu, e_S)
    assert rel_err(S0.cpu().numpy(), c["S_o"]) < TOL


@pytest.mark.parametrize("case", VIEW_CASES, ids=_id)
def test_views_equal_packed_arrays_bit_for_bit(eng, case):
    """S0 and S with leading dimension D + 2, mu0 a 16-byte aligned view at a non-zero offset into a larger buffer, NaN everywhere
    else: a prefetch indexed from the wrong base reads NaN, a store outside the extent overwrites one."""
    import torch
    D, B, fold, knobs = case
    c = _case(D, B)
    X, G, mu0, S0 = _dev(eng, c)

    def wide(t, ld):
        buf = torch.full((t.shape[0], ld), float("nan"), dtype=torch.float64, device="cuda")
        v = buf[:, :t.shape[1]]
        v.copy_(t)
        return v, buf

    mbuf = torch.full((D + 64,), float("nan"), dtype=torch.float64, device="cuda")
    mu0v = mbuf[6:6 + D]                                            # 48 bytes into the buffer
    mu0v.copy_(mu0)
    assert mu0v.data_ptr() % 16 == 0 and mu0v.data_ptr() != mbuf.data_ptr()
    ref_mu, ref_S, _ = _run(eng, (X, G, mu0, S0), fold, knobs)
    Sv, Sbuf = wide(eng.zeros(D, D), D + 2)
    obuf = torch.full((D + 64,), float("nan"), dtype=torch.float64, device="cuda")
    mu, S, path = _run(eng, (X, G, mu0v, wide(S0, D + 2)[0]), fold, knobs, out=(obuf[6:6 + D], Sv))
    assert {"gsm_two_launch", "cov_fold_diag"} <= path, path
    assert S.data_ptr() == Sv.data_ptr()
    _assert_mu_blocks(mu, ref_mu, "the packed-array result")
    assert torch.equal(mu, ref_mu) and torch.equal(S, ref_S) and torch.equal(S, S.T)
    assert bool(torch.isnan(Sbuf[:, D:]).all())                     # nothing was written beyond column D
    assert bool(torch.isnan(obuf[:6]).all()) and bool(torch.isnan(obuf[6 + D:]).all())   # nor outside mu
    assert bool(torch.isnan(mbuf[:6]).all()) and bool(torch.isnan(mbuf[6 + D:]).all())
    assert rel_err(S.cpu().numpy(), c["S_o"]) < TOL and rel_err(mu.cpu().numpy(), c["mu_o"]) < TOL
