"""Numpy restatement of the shared-design Laplace initialiser (gsmvi_glm_shared_hessian_batched_f64,
gsmvi_laplace_shared_step_batched_f64, csrc/gsmvi_laplace_shared_batched.hip) and a stand-in engine for the host logic of
``laplace_init_shared_batched`` and ``neg_hessian_shared_batched``.  Test-only.  All K problems have the rows a_n of ONE design
matrix A (N, D); problem k has responses y_k, offsets o_k, observation weights v_k >= 0, lam_k and (gaussian) tau_k.  With
eta = A x + o_k, the link (r, t) of glm_batched_ref.link and the weight w = -dr / d eta of laplace_batched_ref.weights:

    f_k(x) = -( sum_n v_kn t_n - lam_k |x|^2 / 2 ),   g_k(x) = -( sum_n v_kn r_n a_n - lam_k x ),   H_k(x) = sum_n v_kn w_n a_n a_n^T + lam_k I

An observation whose weight is not > 0 is dropped before anything is computed (its y, offset and eta are never looked at), as the
kernel removes it by selection.  The sums are formed as laplace_batched_ref.evaluate forms them, so that v = 1 is that function on
the K-fold replicated design bit for bit; every summed quantity comes with its scale, the sum of the absolute values of its terms.
The step is the state machine of include/gsmvi_hip.h (gsmvi_laplace_step_batched_f64) on this evaluation, built from
laplace_batched_ref's pieces.  Pinned in tests/test_shared_laplace_cpu.py."""
import functools

import numpy as np

import glm_batched_ref as gref
import laplace_batched_ref as lref
import shared_glm_ref as sref
from laplace_batched_ref import _direction, chol_info, inverse, new_state, pack      # noqa: F401
from shared_glm_ref import make_inputs, replicate                                   # noqa: F401

FAMILIES = gref.FAMILIES
# (N, D) of the GPU tests: each padded width (16, 32, 48, 64 columns), the four-problem packing (D <= 16) and the one-problem
# packing, N one past one and two row tiles of 32, the largest D
SHAPES = ((40, 3), (70, 10), (33, 16), (65, 17), (70, 33), (150, 64))
STEP_K = 5                                  # problems per trajectory batch of the step test
STEP_GTOL = lref.STEP_GTOL
# make_inputs seeds of the step test's trajectories where the default one (N + D) puts a decision on its threshold or leaves the
# flat-prior problem 0 without a mode (tests/test_shared_laplace_cpu.py asserts the margins for every entry, default or not):
# (family, (N, D)) -> seed
SEEDS = {("logistic", (40, 3)): 1, ("logistic", (33, 16)): 7, ("logistic", (70, 33)): 53, ("logistic", (150, 64)): 8,
         ("poisson", (40, 3)): 2, ("poisson", (70, 10)): 1, ("poisson", (33, 16)): 2, ("probit", (33, 16)): 74,
         ("probit", (65, 17)): 1, ("probit", (70, 33)): 47}


def problem(family, A, y, offset, weights, lam, tau, k):
    """problem k of a batch as the restatement takes it: its selected observations only (weight > 0; all of them without weights)"""
    A = np.asarray(A, dtype=np.float64)
    K, N = np.shape(y)
    if weights is None:
        sel, v = np.arange(N), np.ones(N)
    else:
        w = np.asarray(weights, dtype=np.float64)[k]
        with np.errstate(invalid="ignore"):
            sel = np.flatnonzero(w > 0.0)
        v = w[sel]
    return {"family": family, "A": A[sel], "y": np.asarray(y, dtype=np.float64)[k, sel], "v": v,
            "o": np.zeros(len(sel)) if offset is None else np.asarray(offset, dtype=np.float64)[k, sel],
            "lam": float(np.broadcast_to(lam, (K,))[k]), "tau": float(np.broadcast_to(tau, (K,))[k])}


def evaluate(p, x):
    """f, g, H at x and the scales of the three sums; non-finite x or a flagged selected observation: f = NaN, g = H = NaN"""
    A, lam, v = p["A"], p["lam"], p["v"]
    D = A.shape[1]
    with np.errstate(all="ignore"):
        eta = A @ x + p["o"]
        r, t, flag = gref.link(p["family"], eta, p["y"], p["tau"])
        w, flag2 = lref.weights(p["family"], eta, p["y"], p["tau"])
        r, t, w = v * r, v * t, v * w
        f = -(t.sum() - 0.5 * lam * (x * x).sum())
        g = -(r @ A - lam * x)
        H = (A * w[:, None]).T @ A + lam * np.eye(D)
        sf = np.abs(t).sum() + 0.5 * lam * (x * x).sum()
        sg = np.abs(r) @ np.abs(A) + lam * np.abs(x)
        sH = (np.abs(A) * np.abs(w)[:, None]).T @ np.abs(A) + lam * np.eye(D)
    H = 0.5 * (H + H.T)
    if not np.isfinite(x).all() or flag.any() or flag2.any():
        f, g, H = np.nan, np.full(D, np.nan), np.full((D, D), np.nan)
    return f, g, H, {"f": sf, "g": sg, "H": sH}


def neg_hessian(family, A, y, offset, weights, lam, tau, X):
    """(K, D, D) at the rows of X (K, D)"""
    X = np.asarray(X, dtype=np.float64)
    return np.stack([evaluate(problem(family, A, y, offset, weights, lam, tau, k), X[k])[2] for k in range(X.shape[0])])


def step(p, before, start, maxiter=100, maxfun=200, gtol=1e-8):
    """one launch for one problem: (state after, notes), as laplace_batched_ref.step, on this module's ``evaluate``; notes also
    carries ``pivot``: the smallest pivot / (64 eps H_jj) of a factorisation that was made"""
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in before.items()}
    notes = {}
    if not start and s["status"] != 0:
        return s, notes                                                 # frozen
    ft, gt, H, sc = evaluate(p, s["Xt"])
    notes["scale_f"], notes["scale_g"] = sc["f"], sc["g"]
    fin = bool(np.isfinite(ft) and np.isfinite(gt).all())

    def direction():
        _direction(s, gt, H, sc, notes)
        notes["pivot"] = pivot_margin(H)

    if start:
        s.update(x=s["Xt"].copy(), f=ft, g=gt, d=np.zeros_like(gt), t=0.0, gd=0.0, nfev=1, nit=0, nls=0, status=0)
        if not fin:
            s["status"] = 4
        else:
            notes["gmax"] = float(np.abs(gt).max())
            if notes["gmax"] <= gtol:
                s["status"] = 1
            else:
                direction()
        return s, notes
    s["nfev"] += 1
    f, t, gd = s["f"], s["t"], s["gd"]
    rhs = (f + (1e-4 * t) * gd) + 1e-10 * max(1.0, abs(f))
    ok = fin and ft <= rhs
    if fin:
        notes["armijo"] = abs(rhs - ft) / max(1.0, abs(f))
    if not ok:
        s["t"] = 0.5 * t
        s["nls"] += 1
        if s["nls"] > 20:
            s["status"] = 3
        elif s["nfev"] >= maxfun:
            s["status"] = 2
        else:
            s["Xt"] = s["x"] + s["t"] * s["d"]
        return s, notes
    s.update(x=s["Xt"].copy(), f=ft, g=gt)
    s["nit"] += 1
    notes["gmax"] = float(np.abs(gt).max())
    if notes["gmax"] <= gtol:
        s["status"] = 1
    elif s["nit"] >= maxiter or s["nfev"] >= maxfun:
        s["status"] = 2
    else:
        direction()
    return s, notes


def pivot_margin(H):
    """the smallest pivot / (64 eps H_jj) of the right-looking factorisation of H (0 where a pivot is not finite or not positive)"""
    S = np.array(H, dtype=np.float64)
    dg = np.diag(S).copy()
    low = np.inf
    with np.errstate(all="ignore"):
        for c in range(S.shape[0]):
            a = S[c, c]
            if not (a > 0.0 and a < np.inf and dg[c] > 0.0):
                return 0.0
            low = min(low, a / (lref.PIVOT_REL * dg[c]))
            v = S[c, c + 1:] / np.sqrt(a)
            S[c + 1:, c + 1:] -= np.outer(v, v)
    return float(low)


def run(p, x0, record=False, maxiter=100, maxfun=200, gtol=1e-8):
    """the whole iteration of one problem: the final state, and with ``record`` the list of (before, after, notes) per launch"""
    s = new_state(x0)
    rec = []
    for r in range(maxfun):
        after, notes = step(p, s, r == 0, maxiter, maxfun, gtol)
        rec.append((s, after, notes))
        s = after
        if s["status"] != 0:
            break
    return (s, rec) if record else s


def inputs(family, shape, seed=None, K=STEP_K):
    """make_inputs at (N, D) = ``shape`` with the seed of SEEDS: A, y, offset, weights, lam, tau, X"""
    N, D = shape
    return make_inputs(family, K, N, D, 1, seed=SEEDS.get((family, shape)) if seed is None else seed)


def _trajectories(family, shape, full, seed):
    A, y, offset, weights, lam, tau, _ = inputs(family, shape, seed)
    out = []
    for k in range(STEP_K):
        p = problem(family, A, y, offset if full else None, weights if full else None, lam, tau, k)
        s, rec = run(p, np.zeros(shape[1]), record=True, gtol=STEP_GTOL, maxiter=30, maxfun=60)
        out.append((k, s, rec))
    return out


@functools.lru_cache(maxsize=None)
def trajectories(family, shape, full):
    """the step test's runs at (N, D) = ``shape``: the STEP_K problems of ``inputs`` from x0 = 0 at gtol = STEP_GTOL, with offsets
    and weights (``full``) or with neither, as [(problem index, final state, [(before, after, notes), ...]), ...]; computed once
    and shared (do not modify)"""
    return _trajectories(family, shape, full, None)


def margins_hold(traj):
    """what tests/test_laplace_batched_cpu.py demands of the per-problem trajectories: every run converged, no max|g| within a
    factor 1.5 of gtol, every Armijo decision by at least 1e-11 max(1, |f|), no failed factorisation -- and, since a pivot is a
    decision too, every pivot at least 1e3 times its threshold 64 eps H_jj.  Returns (ok, smallest Armijo margin, smallest pivot
    ratio)."""
    ok, low, piv = True, 1.0, np.inf
    for _, st, rec in traj:
        ok = ok and st["status"] == 1
        for _, _, notes in rec:
            if "gmax" in notes:
                ok = ok and not STEP_GTOL / 1.5 <= notes["gmax"] <= 1.5 * STEP_GTOL
            if "armijo" in notes:
                low = min(low, notes["armijo"])
            if "pivot" in notes:
                piv = min(piv, notes["pivot"])
            ok = ok and notes.get("info", 0) == 0
    return bool(ok and low >= 1e-11 and piv >= 1e3), low, piv


class StandInEngine(sref.RestatementEngine, lref.StandInEngine):
    """the engine calls of ``laplace_init_shared_batched`` and ``neg_hessian_shared_batched`` on numpy and the restatement (the
    state, ``read_flag`` and ``read_ints`` are laplace_batched_ref.StandInEngine's)"""
    name = "restatement-shared-laplace(test-only)"

    def glm_shared_hessian_batched(self, X, A, y, family, offset=None, weights=None, prior_prec=1.0, noise_prec=1.0, want="h",
                                   out=None, cov_out=None, info_out=None):
        self.calls.append(("shared_hessian", family, want))
        assert A.ndim == 2 and A.dtype == np.float64 and y.dtype == np.float64
        H = neg_hessian(family, A, y, offset, weights, prior_prec, noise_prec, X)
        if want == "h":
            return H
        ci = [inverse(h) for h in H]
        cov, info = np.stack([c for c, _ in ci]), np.array([i for _, i in ci], dtype=np.int32)
        return (cov, info) if want == "cov" else (H, cov, info)

    def laplace_shared_step_batched(self, state, A, y, family, offset=None, weights=None, prior_prec=1.0, noise_prec=1.0,
                                    start=False, maxiter=100, maxfun=200, gtol=1e-8):
        self.calls.append(("laplace_shared_step", family, bool(start)))
        assert A.ndim == 2
        for k in range(y.shape[0]):
            p = problem(family, A, y, offset, weights, prior_prec, noise_prec, k)
            i = state["ist"][k]
            s = {"x": state["x"][k], "g": state["g"][k], "d": state["d"][k], "Xt": state["Xt"][k], "f": state["sc"][k, 0],
                 "t": state["sc"][k, 1], "gd": state["sc"][k, 2], "status": int(i[0]), "nit": int(i[1]), "nfev": int(i[2]),
                 "nls": int(i[3])}
            was = 0 if start else s["status"]
            a, _ = step(p, s, bool(start), maxiter, maxfun, gtol)
            one = pack([a])
            for name in ("x", "g", "d", "Xt", "sc", "ist"):
                state[name][k] = one[name][0]
            if was == 0 and a["status"] != 0:
                state["stopped"][0] += 1


NAMES = ("gsmvi_glm_shared_hessian_batched_f64", "gsmvi_laplace_shared_step_batched_f64")


def check_bad_arguments(lib):
    """both entry points through the C ABI with a NULL context, in the pattern of laplace_batched_ref.check_bad_arguments: every
    bad argument returns GSMVI_ERR_BAD_ARG (1) with its own message, so nothing can have been enqueued; valid calls end at the
    context"""
    import ctypes as C
    buf = (C.c_double * 8192)()
    p = C.cast(buf, C.c_void_p).value
    a = lambda n: p + 8 * 512 * n                                   # noqa: E731  sixteen disjoint 4 KB arrays
    err = lambda: (lib.gsmvi_last_error() or b"").decode()           # noqa: E731

    def hess(K=2, D=4, N=5, family=1, A=a(0), y=a(1), offset=a(2), weights=a(3), tau=1.0, tau_dev=None, lam=1.0, lam_dev=None,
             X=a(4), H=a(5), cov=a(6), info=a(7)):
        return lib.gsmvi_glm_shared_hessian_batched_f64(None, None, K, D, N, family, A, y, offset, weights, tau, tau_dev, lam,
                                                        lam_dev, X, H, cov, info)

    def step_(K=2, D=4, N=5, family=1, A=a(0), y=a(1), offset=a(2), weights=a(3), tau=1.0, tau_dev=None, lam=1.0, lam_dev=None,
              start=0, x=a(4), g=a(5), d=a(6), sc=a(7), ist=a(8), Xt=a(9), stopped=a(10), maxiter=10, maxfun=20, gtol=1e-8):
        return lib.gsmvi_laplace_shared_step_batched_f64(None, None, K, D, N, family, A, y, offset, weights, tau, tau_dev, lam,
                                                         lam_dev, start, x, g, d, sc, ist, Xt, stopped, maxiter, maxfun, gtol)

    for call, name in ((hess, NAMES[0]), (step_, NAMES[1])):
        assert call(D=0) == 1 and "D must be" in err() and name in err()
        assert call(D=65) == 1 and "D must be" in err()
        assert call(K=0) == 1 and "K must be" in err()
        assert call(K=2 ** 26) == 1 and "K must be" in err()
        assert call(N=0) == 1 and "N must be" in err()
        assert call(K=2 ** 20, N=2 ** 40) == 1 and "too large" in err()
        for fam in (-1, 4):
            assert call(family=fam) == 1 and "family" in err(), fam
        for arr in ("A", "y"):
            assert call(**{arr: None}) == 1 and "NULL array" in err(), arr
        assert call(lam=-1.0) == 1 and "prior_prec" in err()
        assert call(lam=float("inf")) == 1 and "prior_prec" in err()
        assert call(tau=2.0) == 1 and "noise_prec" in err()
        assert call(tau_dev=a(11)) == 1 and "noise_prec" in err()
        assert call(family=3, tau=0.0) == 1 and "noise_prec" in err()
        for fam in (0, 1, 2, 3):
            assert call(family=fam) == 1 and "ctx is NULL" in err(), fam
        assert call(family=3, tau_dev=a(11)) == 1 and "ctx is NULL" in err()
        assert call(offset=None, weights=None, lam_dev=a(11)) == 1 and "ctx is NULL" in err()
        assert call(y=a(0), offset=a(0), weights=a(0)) == 1 and "ctx is NULL" in err()      # read-only arrays may overlap
    assert hess(X=None) == 1 and "NULL array" in err()
    assert hess(H=None, cov=None, info=None) == 1 and "H or cov" in err()
    assert hess(info=None) == 1 and "info_dev is required" in err()                         # cov without info_dev
    assert hess(cov=None) == 1 and "info_dev is required" in err()                          # and info_dev without cov
    assert hess(cov=None, info=None) == 1 and "ctx is NULL" in err()
    assert hess(H=None) == 1 and "ctx is NULL" in err()
    for w in ("H", "cov", "info"):
        for arr, where in (("A", a(0)), ("y", a(1)), ("offset", a(2)), ("weights", a(3)), ("X", a(4))):
            assert hess(**{w: where}) == 1 and f"{w if w != 'info' else 'info_dev'} overlaps {arr}" in err(), (w, arr)
    assert hess(cov=a(5)) == 1 and "cov overlaps H" in err()
    assert hess(lam_dev=a(5)) == 1 and "H overlaps prior_prec_dev" in err()
    assert hess(family=3, tau_dev=a(6)) == 1 and "cov overlaps noise_prec_dev" in err()
    assert hess(H=a(4) + 8 * (2 * 4 - 1)) == 1 and "H overlaps X" in err()                  # the last element of X
    assert hess(H=a(4) + 8 * 2 * 4) == 1 and "ctx is NULL" in err()                         # adjacent is not overlapping
    # A is ONE (N, D) matrix: N D doubles, not K N D
    assert hess(H=a(0) + 8 * (5 * 4 - 1)) == 1 and "H overlaps A" in err()
    assert hess(H=a(0) + 8 * 5 * 4) == 1 and "ctx is NULL" in err()
    for arr in ("x", "g", "d", "sc", "ist", "Xt"):
        assert step_(**{arr: None}) == 1 and "NULL array" in err(), arr
        assert step_(**{arr: a(0)}) == 1 and f"{arr} overlaps A" in err(), arr
        assert step_(**{arr: a(3)}) == 1 and f"{arr} overlaps weights" in err(), arr
        assert step_(**{arr: a(10)}) == 1 and "overlaps" in err() and "stopped_dev" in err(), arr
    assert step_(g=a(4)) == 1 and "g overlaps x" in err()
    assert step_(stopped=None) == 1 and "ctx is NULL" in err()
    assert step_(maxfun=1) == 1 and "maxfun at least 2" in err()
    assert step_(maxiter=0) == 1 and "maxiter must be at least 1" in err()
    assert step_(gtol=-1.0) == 1 and "gtol" in err()
    assert step_(gtol=float("nan")) == 1 and "gtol" in err()
    assert step_(start=1) == 1 and "ctx is NULL" in err()
