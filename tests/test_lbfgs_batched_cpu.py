"""The batched L-BFGS initialiser without a GPU: the numpy restatement (tests/lbfgs_batched_ref.py) is pinned to scipy's dense
inverse-Hessian product and to the Newton MAP of the logistic problems, the inputs of the GPU tests are shown to visit every
branch, and the argument checks of ``lbfgs_init_batched`` and of the C ABI run before any device work."""
import collections
import ctypes

import numpy as np
import pytest
from scipy.optimize import LbfgsInvHessProduct

import lbfgs_batched_ref as ref
import logistic_batched_ref as lref


def _scipy_dense(st):
    idx = ref.held(st)
    return LbfgsInvHessProduct(st["S"][idx], st["Y"][idx]).todense()


def _logistic_runs(N, D, **opt):
    A, y, counts, lam, _ = lref.make_inputs(13, N, D, 1)
    for k in range(1, 13):
        st = ref.run(ref.logistic_fun(A[k], y[k], counts[k], lam[k]), np.zeros(D), **opt)
        yield k, st, lref.newton_map(A[k], y[k], lam[k], n=counts[k]), lam[k]


@pytest.mark.parametrize("N,D", ref.LOGISTIC_SHAPES)
def test_hess_inv_is_scipys_dense_product_on_the_logistic_runs(N, D):
    worst = 0.0
    for k, st, _, _ in _logistic_runs(N, D):
        H, Hs = ref.hess_inv(st), _scipy_dense(st)
        worst = max(worst, np.abs(H - Hs).max() / np.abs(Hs).max())
        assert np.array_equal(H, H.T) or np.abs(H - H.T).max() <= 1e-14 * np.abs(H).max()
    print(f"(N, D) = {(N, D)}: hess_inv against LbfgsInvHessProduct.todense(), worst relative {worst:.2e}")
    assert worst <= 1e-12


def test_hess_inv_is_scipys_dense_product_after_the_ring_buffer_wrapped():
    """the D = 16 Gaussian of the reference's example: more than ten accepted steps, the oldest pair sits mid-array"""
    st = ref.run(ref.gaussian_fun(16), np.ones(16))
    assert st["status"] == 1 and st["visits"]["wrapped"] > 0 and st["npairs"] == ref.M and st["head"] not in (0,)
    H, Hs = ref.hess_inv(st), _scipy_dense(st)
    err = np.abs(H - Hs).max() / np.abs(Hs).max()
    print(f"D = 16 Gaussian, {st['nfev']} evaluations, {st['nit']} iterations: worst relative {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("N,D", ref.LOGISTIC_SHAPES)
def test_ftol_zero_converges_within_the_derived_bound(N, D):
    """-grad^2 lp >= lam_k I, so |x - x*|_2 <= |g|_2 / lam_k <= sqrt(D) max|g| / lam_k <= sqrt(D) gtol / lam_k at status 1"""
    worst = 0.0
    for k, st, xs, lam in _logistic_runs(N, D, ftol=0.0):
        assert st["status"] == 1, (k, st["status"])
        assert np.abs(st["g"]).max() <= 1e-5
        frac = np.linalg.norm(st["x"] - xs) / (np.sqrt(D) * 1e-5 / lam)
        worst = max(worst, frac)
        assert frac <= 1.0, (k, frac)
    print(f"(N, D) = {(N, D)}: worst share of the bound used {worst:.3f}")


@pytest.mark.parametrize("N,D", ref.LOGISTIC_SHAPES)
def test_default_tolerances_converge_within_the_bound_of_the_final_gradient(N, D):
    for k, st, xs, lam in _logistic_runs(N, D):
        assert st["status"] == 1, (k, st["status"])
        assert np.linalg.norm(st["x"] - xs) <= np.sqrt(D) * np.abs(st["g"]).max() / lam, k
        assert st["nfev"] <= 20 and st["visits"]["rejected"] <= 2


def test_the_gpu_inputs_visit_every_branch():
    """what tests/test_gpu_lbfgs_batched.py walks step by step: the visit counts are asserted here, so the GPU test cannot
    silently cover less; and the two decisions that go through a sum formed on the device are exact zeros on both sides or clear
    of their thresholds by 1e-6 of the sum of the absolute products"""
    total = collections.Counter()
    for D in ref.GPU_DS:
        per_d = collections.Counter()
        for name, fun, x0, opt in ref.gpu_cases(D):
            st, rec = ref.run(fun, x0, record=True, **opt)
            assert len(rec) == st["nfev"]
            per_d += st["visits"]
            for kind, a, b, scale in st["margins"]:
                assert (a == 0.0 and b == 0.0) or abs(a - b) >= 1e-6 * scale, (D, name, kind, a, b, scale)
        for branch in ("accepted", "accepted_unit", "rejected", "stored", "skipped", "maxiter", "status1", "status2", "status3",
                       "status4"):
            assert per_d[branch] > 0, (D, branch)
        total += per_d
    assert total["wrapped"] > 0 and total["maxfun"] > 0 and total["not_descent"] == 0
    for D in (5, 10, 16, 17, 33, 64):                                   # (D <= 2 converges before ten pairs exist)
        assert sum(ref.run(f, x0, **o)["visits"]["wrapped"] for _, f, x0, o in ref.gpu_cases(D)) > 0, D
    print(dict(total))


def test_a_stopped_state_is_frozen_and_pack_round_trips():
    st = ref.run(ref.gaussian_fun(5), np.ones(5))
    again = ref.step(st, 0.0, np.zeros(5))
    for key in ("x", "g", "d", "xt", "S", "Y", "sy", "yy"):
        assert np.array_equal(st[key], again[key])
    assert [st[k] for k in ("f", "t", "gd", "nls", "npairs", "head", "nit", "nfev", "status")] == \
        [again[k] for k in ("f", "t", "gd", "nls", "npairs", "head", "nit", "nfev", "status")]
    p = ref.pack([st, again])
    assert p["ist"].dtype == np.int32 and p["sc"].shape == (2, ref.NSC) and np.array_equal(p["S"][0], st["S"])
    assert p["ist"][0].tolist() == [st["status"], st["nit"], st["nfev"], st["nls"], st["npairs"], st["head"], 0, 0]


def test_argument_errors_need_no_gpu():
    import gsmvi_amd
    lp = lambda x: np.zeros(x.shape[0])                                 # noqa: E731
    lp_g = lambda x: np.zeros_like(x)                                   # noqa: E731
    with pytest.raises(ValueError, match="outside 1 <= D <= 64"):
        gsmvi_amd.lbfgs_init_batched(np.zeros((3, 0)), lp, lp_g)
    with pytest.raises(ValueError, match="outside 1 <= D <= 64"):
        gsmvi_amd.lbfgs_init_batched(np.zeros((3, 65)), lp, lp_g)
    with pytest.raises(ValueError, match=r"\(K, D\) or \(D,\)"):
        gsmvi_amd.lbfgs_init_batched(np.zeros((3, 1, 4)), lp, lp_g)
    with pytest.raises(ValueError, match="K = 0"):
        gsmvi_amd.lbfgs_init_batched(np.zeros((0, 4)), lp, lp_g)
    with pytest.raises(ValueError, match="both required"):
        gsmvi_amd.lbfgs_init_batched(np.zeros((3, 4)), None, lp_g)
    with pytest.raises(ValueError, match="both required"):
        gsmvi_amd.lbfgs_init_batched(np.zeros((3, 4)), lp, None)
    with pytest.raises(ValueError, match="maxfun at least 2"):
        gsmvi_amd.lbfgs_init_batched(np.zeros((3, 4)), lp, lp_g, maxfun=1)
    with pytest.raises(ValueError, match="gtol and ftol"):
        gsmvi_amd.lbfgs_init_batched(np.zeros((3, 4)), lp, lp_g, gtol=-1.0)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """the C ABI checks shapes, NULL arrays and overlaps before it looks at the context: GSMVI_ERR_BAD_ARG with a NULL context"""
    from gsmvi_amd import _lib
    lib = _lib.load_library()
    buf = (ctypes.c_double * 4096)()
    p = lambda off: ctypes.c_void_p(ctypes.addressof(buf) + 8 * off)    # noqa: E731
    K, D = 2, 4
    arrs = dict(fv=p(0), gv=p(8), x=p(16), g=p(24), d=p(32), S=p(40), Y=p(120), sc=p(200), ist=p(248), Xt=p(256), stopped=p(264))

    def step(K=K, D=D, sign=-1.0, maxiter=10, maxfun=10, gtol=1e-5, ftol=0.0, **over):
        a = dict(arrs, **over)
        return lib.gsmvi_lbfgs_step_batched_f64(None, None, K, D, 0, a["fv"], a["gv"], sign, a["x"], a["g"], a["d"], a["S"], a["Y"],
                                                a["sc"], a["ist"], a["Xt"], a["stopped"], maxiter, maxfun, gtol, ftol)

    assert step() == 1 and b"ctx is NULL" in lib.gsmvi_last_error()      # everything else is in order
    assert step(D=0) == 1 and b"D must be" in lib.gsmvi_last_error()
    assert step(D=65) == 1 and b"D must be" in lib.gsmvi_last_error()
    assert step(K=0) == 1 and b"K must be" in lib.gsmvi_last_error()
    assert step(x=None) == 1 and b"NULL array" in lib.gsmvi_last_error()
    assert step(sign=0.5) == 1 and b"sign" in lib.gsmvi_last_error()
    assert step(maxfun=1) == 1 and b"maxfun" in lib.gsmvi_last_error()
    assert step(maxiter=0) == 1 and b"maxiter" in lib.gsmvi_last_error()
    assert step(gtol=float("nan")) == 1 and b"gtol" in lib.gsmvi_last_error()
    assert step(Xt=p(17)) == 1 and b"overlaps" in lib.gsmvi_last_error()
    assert step(gv=p(41)) == 1 and b"S overlaps gv" in lib.gsmvi_last_error()
    assert step(stopped=None) == 1 and b"ctx is NULL" in lib.gsmvi_last_error()      # the counter is optional

    hess = lambda K=K, D=D, S=p(40), Y=p(120), ist=p(248), cov=p(300): \
        lib.gsmvi_lbfgs_hess_inv_batched_f64(None, None, K, D, S, Y, ist, cov)       # noqa: E731
    assert hess() == 1 and b"ctx is NULL" in lib.gsmvi_last_error()
    assert hess(D=65) == 1 and b"D must be" in lib.gsmvi_last_error()
    assert hess(cov=None) == 1 and b"NULL array" in lib.gsmvi_last_error()
    assert hess(cov=p(100)) == 1 and b"cov overlaps" in lib.gsmvi_last_error()


def test_lds_of_every_dimension_fits_the_default_limit():
    """the debug query walks every D: a step holds the ring buffers and their twenty sums (2 m D + 2 m doubles per problem),
    the finish also the D x (D | 1) matrix, a vector and ten sums; four problems per workgroup for D <= 16; never above 64 KB, so
    no kernel attribute is set"""
    from gsmvi_amd import _lib
    lib = ctypes.CDLL(_lib.library_path(debug=True))
    fn = lib.gsmvi_debug_lbfgs_batched_lds
    fn.restype, fn.argtypes = _lib._DEBUG_SIGS["gsmvi_debug_lbfgs_batched_lds"]
    worst = 0
    for D in range(1, 65):
        for mode in (0, 1):
            nbytes, ppw = ctypes.c_size_t(0), ctypes.c_int(0)
            assert fn(D, mode, ctypes.byref(nbytes), ctypes.byref(ppw)) == 0
            assert ppw.value == (4 if D <= 16 else 1)
            per = 20 * D + 20 if mode == 0 else D * (D | 1) + 20 * D + D + 10
            assert nbytes.value == 8 * per * ppw.value
            assert nbytes.value <= 64 * 1024
            worst = max(worst, nbytes.value)
    assert worst == 8 * (64 * 65 + 20 * 64 + 64 + 10)
    nbytes, ppw = ctypes.c_size_t(0), ctypes.c_int(0)
    assert fn(65, 0, ctypes.byref(nbytes), ctypes.byref(ppw)) == 1 and fn(4, 2, ctypes.byref(nbytes), ctypes.byref(ppw)) == 1
    assert fn(4, 0, None, ctypes.byref(ppw)) == 1
