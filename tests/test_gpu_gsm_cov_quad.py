"""The quad / pair item map of the covariance launch of the two-launch dense GSM update (k_gsm_cov_sym<.., FROM_SLABS, .., QUAD>,
knob "cov_diag_quad": 0 = the fold as it was, 1 = where the fold runs by default on the shipped two-slab form, 2 = wherever the
fold knob is not 0).  A quad computes the same chains on the same staged values as a host or a diagonal workgroup, so for every shape
  * mu and S equal the results of "cov_diag_quad" = 0 both with "cov_fold_diag" = 0 and with the fold BIT FOR BIT (torch.equal),
  * S equals its transpose exactly,
  * mu and S are within the route's bound of the pinned oracle (rel_err < 1e-11, as tests/test_gpu_gsm_cov_fold.py),
  * padded leading dimensions (D + 2) with S and mu ending at the end of their allocations give the packed result,
  * a captured graph replays to the eager result,
  * Sigma0 with the strictly lower 16 x 16 block of every diagonal tile moved by one ulp still gives the bits of knob 0 (W = S0 + U
    reads that block although block (1, 0) of U is written as a transpose),
  * the path set equals what knob 0 with the fold reports (the quad route has no bit of its own).
Shapes: (256, 16), (256, 32) with knob 2 -- nt = 8, four quads and twelve pairs on the KCT = 4 instances; (1024, 16), (1024, 32) at
the default -- the shipped KCT = 2 instances."""
import os
import re

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-11
_CACHE = {}
_CTX_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsm-vi_amd", "csrc", "gsmvi_ctx.h")


def _default(name):
    with open(_CTX_H) as f:
        return int(re.search(rf"int\s+tune_{name}\s*=\s*(\d+)\s*;", f.read()).group(1))


DEFAULTS = {k: _default(k) for k in ("cov_diag_quad", "cov_fold_diag", "cov_s0_last", "cov_store_wt", "panel_qm_whole")}
# (D, B, quad knob, fold knob of the folded reference)
CASES = [(256, 16, 2, 2), (256, 32, 2, 2), (1024, 16, 1, 1), (1024, 32, 1, 1)]


def _id(case):
    return f"{case[0]}-{case[1]}-quad{case[2]}"


@pytest.fixture(scope="module")
def eng():
    import gsmvi_amd
    e = gsmvi_amd.get_engine()
    e.set_tuning("gsm_two_launch", 1)
    e.set_tuning("panel_kc", 0)
    for k, v in DEFAULTS.items():
        e.set_tuning(k, v)
    yield e
    for k, v in DEFAULTS.items():
        e.set_tuning(k, v)


def _case(D, B):
    """Inputs, the oracle result and the three results of one shape (quads, knob 0 unfolded, knob 0 folded), computed once."""
    if (D, B) not in _CACHE:
        from oracle import gsm_oracle as orc
        st = orc.make_update_state(D, B, 13 + 5 * D + B)
        mu_o, S_o = orc.gsm_update_batched(st["samples"], st["vs"], st["mu0"], st["S0"])
        _CACHE[(D, B)] = dict(X=st["samples"], G=st["vs"], mu0=st["mu0"], S0=st["S0"], mu_o=mu_o, S_o=S_o)
    return _CACHE[(D, B)]


def _dev(eng, c):
    return tuple(eng.asarray(c[k]) for k in ("X", "G", "mu0", "S0"))


def _run(eng, args, quad, fold, out=None):
    try:
        eng.set_tuning("cov_diag_quad", quad)
        eng.set_tuning("cov_fold_diag", fold)
        eng.last_path()
        mu, S = eng.gsm_update(*args, out=out)
        return mu, S, eng.last_path()
    finally:
        eng.set_tuning("cov_diag_quad", DEFAULTS["cov_diag_quad"])
        eng.set_tuning("cov_fold_diag", DEFAULTS["cov_fold_diag"])


def _refs(eng, case):
    """(mu, S, path) of the quads, of knob 0 without the fold and of knob 0 with it: once per shape, never modified."""
    D, B, quad, fold = case
    c = _case(D, B)
    if "res" not in c:
        args = _dev(eng, c)
        q = _run(eng, args, quad, fold if quad == 2 else DEFAULTS["cov_fold_diag"])
        c["res"] = (q, _run(eng, args, 0, 0), _run(eng, args, 0, fold))
    return c["res"]


def _tail_flat(rows, cols, ld, fill=float("nan")):
    """A rows x cols view with leading dimension ld whose last element is the last of its allocation."""
    import torch
    buf = torch.full(((rows - 1) * ld + cols,), fill, dtype=torch.float64, device="cuda")
    return buf.as_strided((rows, cols), (ld, 1)), buf


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_quads_equal_knob_0_bit_for_bit_and_the_oracle(eng, case):
    import torch
    D, B, quad, fold = case
    c = _case(D, B)
    (mu, S, p), (mu_u, S_u, p_u), (mu_f, S_f, p_f) = _refs(eng, case)
    e_mu, e_S = rel_err(mu.cpu().numpy(), c["mu_o"]), rel_err(S.cpu().numpy(), c["S_o"])
    print(f"{_id(case)}: rel_err mu {e_mu:.3e} S {e_S:.3e}; max |dS| against unfolded {float((S - S_u).abs().max()):.3e}, "
          f"folded {float((S - S_f).abs().max()):.3e}; max |dmu| {float((mu - mu_u).abs().max()):.3e}")
    assert "cov_fold_diag" not in p_u and "cov_fold_diag" in p_f, (p_u, p_f)
    assert ("panel_chunk512" in p) == (D == 1024), p                 # KCT = 2 at D = 1024, KCT = 4 below
    bad = [k for k in range(D // 32) if not torch.equal(mu[32 * k:32 * k + 32], mu_u[32 * k:32 * k + 32])]
    assert not bad, f"mu differs from the unfolded result in blocks {bad}"
    assert torch.equal(mu, mu_u) and torch.equal(S, S_u)
    assert torch.equal(mu, mu_f) and torch.equal(S, S_f)
    assert torch.equal(S, S.T)
    assert e_mu < TOL and e_S < TOL, (e_mu, e_S)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_path_set_is_that_of_the_fold(eng, case):
    (_, _, p), _, (_, _, p_f) = _refs(eng, case)
    assert p == p_f and {"gsm_two_launch", "cov_sym", "cov_fold_diag"} <= p, (p, p_f)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_padded_leading_dimensions_at_the_end_of_the_allocation(eng, case):
    import torch
    D, B, quad, fold = case
    c = _case(D, B)
    X, G, mu0, S0 = _dev(eng, c)
    (mu_r, S_r, _), _, _ = _refs(eng, case)
    S0v, _ = _tail_flat(D, D, D + 2)
    S0v.copy_(S0)
    Sv, Sbuf = _tail_flat(D, D, D + 2)
    mubuf = torch.full((D + 6,), float("nan"), dtype=torch.float64, device="cuda")
    muv = mubuf[6:]                                                  # 48 bytes in, ends with the allocation
    mu, S, p = _run(eng, (X, G, mu0, S0v), quad, fold if quad == 2 else DEFAULTS["cov_fold_diag"], out=(muv, Sv))
    assert {"gsm_two_launch", "cov_fold_diag"} <= p, p
    assert S.data_ptr() == Sv.data_ptr() and mu.data_ptr() == muv.data_ptr()
    assert torch.equal(mu, mu_r) and torch.equal(S, S_r) and torch.equal(S, S.T)
    pad = Sbuf[:(D - 1) * (D + 2)].view(D - 1, D + 2)[:, D:]
    assert bool(torch.isnan(pad).all()) and bool(torch.isnan(mubuf[:6]).all())   # nothing outside the views was written


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_graph_replay_equals_eager(eng, case):
    import torch
    D, B, quad, fold = case
    args = _dev(eng, _case(D, B))
    (mu_r, S_r, _), _, _ = _refs(eng, case)
    out = (eng.empty(D), eng.empty(D, D))
    try:
        eng.set_tuning("cov_diag_quad", quad)
        eng.set_tuning("cov_fold_diag", fold if quad == 2 else DEFAULTS["cov_fold_diag"])
        eng.gsm_update(*args, out=out)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.gsm_update(*args, out=out)
        for _ in range(2):
            out[0].zero_(), out[1].zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out[0], mu_r) and torch.equal(out[1], S_r)
    finally:
        eng.set_tuning("cov_diag_quad", DEFAULTS["cov_diag_quad"])
        eng.set_tuning("cov_fold_diag", DEFAULTS["cov_fold_diag"])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_lower_block_of_sigma0_diagonal_tiles_is_read(eng, case):
    """Sigma0 whose strictly lower 16 x 16 block of every diagonal 32 x 32 tile is one ulp up: not symmetric inside those tiles.  Every
    form reads each diagonal tile whole (no mirror store), so the quads still give the bits of knob 0, and S carries the moved block."""
    import torch
    D, B, quad, fold = case
    c = _case(D, B)
    S0 = c["S0"].copy()
    for k in range(D // 32):
        blk = S0[32 * k + 16:32 * k + 32, 32 * k:32 * k + 16]
        blk[...] = np.nextafter(blk, np.inf)
    X, G, mu0, _ = _dev(eng, c)
    args = (X, G, mu0, eng.asarray(S0))
    mu, S, _ = _run(eng, args, quad, fold if quad == 2 else DEFAULTS["cov_fold_diag"])
    mu_u, S_u, _ = _run(eng, args, 0, 0)
    mu_f, S_f, _ = _run(eng, args, 0, fold)
    assert torch.equal(mu, mu_u) and torch.equal(S, S_u)
    assert torch.equal(mu, mu_f) and torch.equal(S, S_f)
    k = D // 32 - 1                                                  # W = S0 + U took the moved block: S is not symmetric there
    assert not torch.equal(S[32 * k + 16:32 * k + 32, 32 * k:32 * k + 16], S[32 * k:32 * k + 16, 32 * k + 16:32 * k + 32].T)
