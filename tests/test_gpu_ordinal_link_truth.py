"""The ordinal link on the GPU, element by element, against the committed mpmath table (tests/golden/ordinal_link_truth.npz;
tests/ordinal_link_truth.py has the grid and the metric).  No kernel of its own: with C = 3, P = 1, N = 1, A = 1, beta = 0, eta given
as the offset and lam = kap = 0, lp of gsmvi_ordinal_batched_f64 is t and G is (dt / d eta, dt / d delta_0, dt / d delta_1).  The
bound is the project's rule max(16, 4 C_CPU) eps of the scale per quantity, C_CPU from tests/test_ordinal_batched_cpu.py and never
from the device.  No mpmath is needed here."""
import numpy as np
import pytest
import torch

import ordinal_batched_ref as ref
import ordinal_link_truth as truth

pytestmark = pytest.mark.gpu


def _probe(eta, d0, d1, y, want="both"):
    """one problem per point: (t, re, d0, d1) of the launch, host arrays (None for what was not asked)"""
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    A, yy, o, X = ref.link3_problems(eta, d0, d1, y)
    out = eng.ordinal_batched(eng.asarray(X), eng.asarray(A), eng.batched_labels(yy), 3, offset=eng.asarray(o), prior_prec=0.0,
                              cut_prec=0.0, want=want)
    torch.cuda.synchronize()
    G, lp = (out, None) if want == "g" else (None, out) if want == "lp" else out
    G = None if G is None else G.cpu().numpy()
    t = None if lp is None else lp.cpu().numpy()[:, 0]
    return (t,) + ((None,) * 3 if G is None else (G[:, 0, 0], G[:, 0, 1], G[:, 0, 2]))


def test_ordinal_batched_is_the_link_element_by_element():
    tab = truth.load_table()
    eta, d0, d1, y = truth.grid()
    got = _probe(eta, d0, d1, y)
    for q, g in zip(truth.QUANTITIES, got):
        worst = truth.ratio(g, tab, q)
        i = int(np.argmax(worst))
        print(f"ordinal {q} on the device: worst ratio {worst[i]:.3f} at eta = {eta[i]!r}, delta = ({d0[i]!r}, {d1[i]!r}), y = {y[i]} "
              f"(bound {truth.c_gpu(q)}, C_CPU {truth.C_CPU[q]})")
        assert worst[i] <= truth.c_gpu(q), (q, worst[i], eta[i], d0[i], d1[i], y[i])
    # the launches with one output give the bits of the one with both
    g1 = _probe(eta, d0, d1, y, want="g")
    t1 = _probe(eta, d0, d1, y, want="lp")[0]
    assert np.array_equal(t1, got[0]) and all(np.array_equal(a, b) for a, b in zip(g1[1:], got[1:]))


def test_beyond_the_grid_no_nan_the_sign_and_inf_only_where_the_truth_overflows():
    """|eta| = 1e160 and 1e300: no NaN, the sign of r_eta, and an infinity only where the float64 rounding of the truth is one"""
    far = truth.load_table()["beyond"]
    eta, d0, d1, y = (np.ascontiguousarray(far[:, i]) for i in range(4))
    assert set(np.abs(eta)) == set(truth.BEYOND)
    got = _probe(eta, d0, d1, y.astype(np.int64))
    for i, (name, g) in enumerate(zip(truth.QUANTITIES, got)):
        tru = far[:, 4 + i]
        assert not np.isnan(g).any(), name
        inf = np.isinf(g)
        assert np.array_equal(g[inf], tru[inf]), (name, far[inf & (g != tru)][:4])          # inf only where the truth is, same sign
    re, re0 = got[1], far[:, 5]
    nz = re0 != 0.0
    assert nz.any() and np.array_equal(np.sign(re[nz]), np.sign(re0[nz]))
