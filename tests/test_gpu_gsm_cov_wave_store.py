"""The per-wave store path of the covariance launch of the two-launch dense GSM update (k_gsm_cov_sym<.., QUAD, WST>, knob
"cov_wave_store": 1 = wherever the quads run, every wave forms W = S0 + U for the 16 x 16 block it computed, stores it and mirrors
it through a wave-private LDS buffer; 0 = the store path through the shared LW buffers and three workgroup barriers).  The new form
runs the same chains, the same (acc_d - acc_e) * invB and the same S0 + U, and copies for the mirror, so for every shape
  * mu and S equal the results of "cov_wave_store" = 0 BIT FOR BIT (torch.equal),
  * S equals its transpose exactly,
  * mu and S are within the route's bound of the pinned oracle (rel_err < 1e-11, as tests/test_gpu_gsm_cov_quad.py),
  * padded leading dimensions (D + 2) with S and mu ending at the end of their allocations give the packed result (the
    write-through descriptor's extent is exact: a store at a wrong offset is dropped and the comparison shows it),
  * a captured graph replays to the eager result,
  * the path set equals knob 0's (the knob has no path bit).
Shapes, those of tests/test_gpu_gsm_cov_quad.py: (256, 16), (256, 32) with "cov_diag_quad" = 2 -- four quads and twelve pairs on the
KCT = 4 instances, plain stores; (1024, 16), (1024, 32) at the defaults -- the shipped KCT = 2 instances, S0 last, write-through."""
import os
import re

import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-11
_CACHE = {}
_CTX_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsm-vi_amd", "csrc", "gsmvi_ctx.h")


def _default(name):
    with open(_CTX_H) as f:
        return int(re.search(rf"int\s+tune_{name}\s*=\s*(\d+)\s*;", f.read()).group(1))


DEFAULTS = {k: _default(k) for k in ("cov_wave_store", "cov_diag_quad", "cov_fold_diag", "cov_s0_last", "cov_store_wt", "panel_qm_whole")}
# (D, B, quad knob, fold knob)
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
    """Inputs and the oracle result of one shape, computed once."""
    if (D, B) not in _CACHE:
        from oracle import gsm_oracle as orc
        st = orc.make_update_state(D, B, 13 + 5 * D + B)
        mu_o, S_o = orc.gsm_update_batched(st["samples"], st["vs"], st["mu0"], st["S0"])
        _CACHE[(D, B)] = dict(X=st["samples"], G=st["vs"], mu0=st["mu0"], S0=st["S0"], mu_o=mu_o, S_o=S_o)
    return _CACHE[(D, B)]


def _dev(eng, c):
    return tuple(eng.asarray(c[k]) for k in ("X", "G", "mu0", "S0"))


def _set(eng, case, wave_store):
    D, B, quad, fold = case
    eng.set_tuning("cov_wave_store", wave_store)
    eng.set_tuning("cov_diag_quad", quad)
    eng.set_tuning("cov_fold_diag", fold if quad == 2 else DEFAULTS["cov_fold_diag"])


def _restore(eng):
    for k in ("cov_wave_store", "cov_diag_quad", "cov_fold_diag"):
        eng.set_tuning(k, DEFAULTS[k])


def _run(eng, case, args, wave_store, out=None):
    try:
        _set(eng, case, wave_store)
        eng.last_path()
        mu, S = eng.gsm_update(*args, out=out)
        return mu, S, eng.last_path()
    finally:
        _restore(eng)


def _refs(eng, case):
    """(mu, S, path) with the knob at 1 and at 0: once per shape, never modified."""
    c = _case(case[0], case[1])
    if "res" not in c:
        args = _dev(eng, c)
        c["res"] = (_run(eng, case, args, 1), _run(eng, case, args, 0))
    return c["res"]


def _tail_flat(rows, cols, ld, fill=float("nan")):
    """A rows x cols view with leading dimension ld whose last element is the last of its allocation."""
    import torch
    buf = torch.full(((rows - 1) * ld + cols,), fill, dtype=torch.float64, device="cuda")
    return buf.as_strided((rows, cols), (ld, 1)), buf


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_wave_store_equals_knob_0_bit_for_bit_and_the_oracle(eng, case):
    import torch
    D, B, _, _ = case
    c = _case(D, B)
    (mu, S, p), (mu_0, S_0, p_0) = _refs(eng, case)
    e_mu, e_S = rel_err(mu.cpu().numpy(), c["mu_o"]), rel_err(S.cpu().numpy(), c["S_o"])
    print(f"{_id(case)}: rel_err mu {e_mu:.3e} S {e_S:.3e}; max |dS| against knob 0 {float((S - S_0).abs().max()):.3e}, "
          f"max |dmu| {float((mu - mu_0).abs().max()):.3e}")
    assert ("panel_chunk512" in p) == (D == 1024), p                 # KCT = 2 at D = 1024, KCT = 4 below
    bad = [(i, j) for i in range(D // 32) for j in range(D // 32) if not torch.equal(S[32 * i:32 * i + 32, 32 * j:32 * j + 32],
                                                                                      S_0[32 * i:32 * i + 32, 32 * j:32 * j + 32])]
    assert not bad, f"S differs from knob 0 in tiles {bad[:12]} ({len(bad)} in all)"
    assert torch.equal(mu, mu_0) and torch.equal(S, S_0)
    assert torch.equal(S, S.T)
    assert e_mu < TOL and e_S < TOL, (e_mu, e_S)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_path_set_is_that_of_knob_0(eng, case):
    (_, _, p), (_, _, p_0) = _refs(eng, case)
    assert p == p_0 and {"gsm_two_launch", "cov_sym", "cov_fold_diag"} <= p, (p, p_0)
    assert ("cov_store_wt" in p) == (case[0] == 1024), p


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_padded_leading_dimensions_at_the_end_of_the_allocation(eng, case):
    import torch
    D, B, _, _ = case
    c = _case(D, B)
    X, G, mu0, S0 = _dev(eng, c)
    _, (mu_r, S_r, _) = _refs(eng, case)
    S0v, _ = _tail_flat(D, D, D + 2)
    S0v.copy_(S0)
    Sv, Sbuf = _tail_flat(D, D, D + 2)
    mubuf = torch.full((D + 6,), float("nan"), dtype=torch.float64, device="cuda")
    muv = mubuf[6:]                                                  # 48 bytes in, ends with the allocation
    mu, S, p = _run(eng, case, (X, G, mu0, S0v), 1, out=(muv, Sv))
    assert {"gsm_two_launch", "cov_fold_diag"} <= p, p
    assert S.data_ptr() == Sv.data_ptr() and mu.data_ptr() == muv.data_ptr()
    assert torch.equal(mu, mu_r) and torch.equal(S, S_r) and torch.equal(S, S.T)
    pad = Sbuf[:(D - 1) * (D + 2)].view(D - 1, D + 2)[:, D:]
    assert bool(torch.isnan(pad).all()) and bool(torch.isnan(mubuf[:6]).all())   # nothing outside the views was written


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_graph_replay_equals_eager(eng, case):
    import torch
    D, B, _, _ = case
    args = _dev(eng, _case(D, B))
    (mu_r, S_r, _), _ = _refs(eng, case)
    out = (eng.empty(D), eng.empty(D, D))
    try:
        _set(eng, case, 1)
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
        _restore(eng)
