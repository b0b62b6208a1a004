"""The negative binomial link on the GPU, element by element, against the committed mpmath table (tests/golden/
negbin_link_truth.npz; tests/negbin_link_truth.py has the grid and the metric).  No kernel of its own: with P = 1, N = 1, A = 1,
beta = 0, eta given as the offset and lam = kap = 0, lp of gsmvi_negbin_batched_f64 is t and G is (r_eta, r_theta).  The bound is
the project's rule max(16, 4 C_CPU) eps of the scale per quantity, C_CPU from tests/test_negbin_batched_cpu.py and never from the
device.  No mpmath is needed here."""
import numpy as np
import pytest
import torch

import negbin_link_truth as truth

pytestmark = pytest.mark.gpu


def _probe(eta, theta, y, want="both"):
    """one problem per point: (r_eta, r_theta, t) of the launch, host arrays"""
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    K = eta.size
    X = np.stack([np.zeros(K), theta], axis=1).reshape(K, 1, 2)
    A, yy, o = np.ones((K, 1, 1)), y.reshape(K, 1).copy(), eta.reshape(K, 1).copy()
    out = eng.negbin_batched(eng.asarray(X), eng.asarray(A), eng.asarray(yy), offset=eng.asarray(o), prior_prec=0.0,
                             log_size_mean=0.0, log_size_prec=0.0, want=want)
    torch.cuda.synchronize()
    if want == "g":
        G = out.cpu().numpy()
        return G[:, 0, 0], G[:, 0, 1], None
    if want == "lp":
        return None, None, out.cpu().numpy()[:, 0]
    G, lp = out[0].cpu().numpy(), out[1].cpu().numpy()
    return G[:, 0, 0], G[:, 0, 1], lp[:, 0]


def test_negbin_batched_is_the_link_element_by_element():
    tab = truth.load_table()
    eta, theta, y = truth.grid()
    re, rt, t = _probe(eta, theta, y)
    for q, got in (("t", t), ("re", re), ("rt", rt)):
        worst = truth.ratio(got, tab, q)
        i = int(np.argmax(worst))
        print(f"negbin {q} on the device: worst ratio {worst[i]:.3f} at eta = {eta[i]!r}, theta = {theta[i]!r}, y = {y[i]!r} "
              f"(bound {truth.c_gpu(q)}, C_CPU {truth.C_CPU[q]})")
        assert worst[i] <= truth.c_gpu(q), (q, worst[i], eta[i], theta[i], y[i])
    # the launches with one output give the bits of the one with both
    re1, rt1, _ = _probe(eta, theta, y, want="g")
    _, _, t1 = _probe(eta, theta, y, want="lp")
    assert np.array_equal(re1, re) and np.array_equal(rt1, rt) and np.array_equal(t1, t)


def test_beyond_the_grid_no_nan_the_sign_and_inf_only_where_the_truth_overflows():
    """|eta| = 1e160 and 1e300: no NaN, the sign of r_eta, and an infinity only where the float64 rounding of the truth is one"""
    far = truth.load_table()["beyond"]
    eta, theta, y, t0, re0, rt0 = (np.ascontiguousarray(far[:, i]) for i in range(6))
    assert set(np.abs(eta)) == set(truth.BEYOND)
    re, rt, t = _probe(eta, theta, y)
    for name, got, tru in (("t", t, t0), ("re", re, re0), ("rt", rt, rt0)):
        assert not np.isnan(got).any(), name
        inf = np.isinf(got)
        assert np.array_equal(got[inf], tru[inf]), (name, far[inf & (got != tru)][:4])      # inf only where the truth is, same sign
    nz = re0 != 0.0
    assert np.array_equal(np.sign(re[nz]), np.sign(re0[nz]))
