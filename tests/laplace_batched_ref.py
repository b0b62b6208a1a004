"""Numpy restatement of the batched Laplace initialiser (gsmvi_glm_hessian_batched_f64, gsmvi_laplace_step_batched_f64,
csrc/gsmvi_laplace_batched.hip), built on ``glm_batched_ref.link``, and a stand-in engine for the host logic of
``laplace_init_batched`` and ``neg_hessian``.  Test-only.  For problem k (glm_batched_ref's model):

    w = -dr / d eta,   H_k(x) = sum_{n < n_k} w(eta_n, y_n) a_n a_n^T + lam_k I,   phi = -lp,   d = -H^{-1} grad phi

The weights are in the kernel's forms, the step is the state machine of include/gsmvi_hip.h word for word (with the slack of
the Armijo test), ``run`` records the state after every launch, and every summed quantity comes with its scale, the sum of the
absolute values of its terms: what an error bound of a sum in another order is proportional to.  It is pinned to torch autograd
of the written densities and to scipy's Newton methods in tests/test_laplace_batched_cpu.py."""
import functools

import numpy as np
from scipy.special import erfcx

import glm_batched_ref as gref

FAMILIES = gref.FAMILIES
# (K, N, D) of the GPU tests: the four-problem packing; D = 10; one full MFMA block with N one past a row tile; the first padded
# D with N one past two tiles; three blocks per side; the largest D
SHAPES = ((5, 40, 3), (6, 70, 10), (5, 33, 16), (5, 65, 17), (5, 70, 33), (4, 150, 64))
STEP_GTOL = 1e-6
PIVOT_REL = 64 * 2.220446049250313e-16
PROBIT_S0, PROBIT_CF = 4.0, 40             # LB_PROBIT_S0, LB_PROBIT_CF of csrc/gsmvi_glm_link.h
# make_inputs seeds of the step test's trajectories where the default one (N + D) puts a decision on its threshold
# (tests/test_laplace_batched_cpu.py asserts the margins for every entry, default or not): (family, (K, N, D)) -> seed
SEEDS = {("logistic", (5, 40, 3)): 1, ("logistic", (6, 70, 10)): 1, ("logistic", (5, 33, 16)): 13, ("logistic", (5, 65, 17)): 1,
         ("logistic", (5, 70, 33)): 2, ("logistic", (4, 150, 64)): 1, ("poisson", (5, 40, 3)): 1, ("poisson", (6, 70, 10)): 5,
         ("poisson", (5, 33, 16)): 3, ("poisson", (5, 65, 17)): 3, ("poisson", (5, 70, 33)): 1, ("probit", (5, 40, 3)): 1,
         ("probit", (6, 70, 10)): 5, ("probit", (5, 33, 16)): 15, ("probit", (5, 70, 33)): 31, ("probit", (4, 150, 64)): 15}


def weights(family, eta, y, tau=1.0):
    """w = -dr / d eta in the kernel's forms, and the mask of the entries that flag their problem (poisson: exp(eta) not finite)"""
    none = np.zeros(np.shape(eta), dtype=bool)
    if family == "logistic":
        e = np.exp(-np.abs(eta))
        d = 1.0 + e
        return e / (d * d), none
    if family == "poisson":
        m = np.exp(eta)
        bad = ~(m < np.inf)
        return np.where(bad, 0.0, m), bad
    if family == "probit":
        s = np.abs(eta)
        u, hs = erfcx(s * 0.70710678118654752440), 0.5 * (s * s)
        e = np.exp(-hs)
        q = 0.5 * (u * e)
        rt, rc = 0.79788456080286535588 / u, e * 0.39894228040143267794 / (1.0 - q)
        # the central side h (h + s), and the tail side h (h - s): from s = PROBIT_S0 on g (1 + z g) with z = 1 / s^2 and
        # g = 1 / (1 + 2 z / (1 + 3 z / ..)) (Laplace's continued fraction of the Mills ratio) as one ratio of its forward recurrence
        wc = rc * (rc + s)
        z = 1.0 / np.maximum(s, PROBIT_S0)
        z = z * z
        a0, a1, b0, b1 = 0.0, 1.0, 1.0, 1.0
        for k in range(2, PROBIT_CF + 1):
            a0, a1, b0, b1 = a1, a1 + (k * z) * a0, b1, b1 + (k * z) * b0
        g = a1 / b1
        wt = np.where(s >= PROBIT_S0, g * (1.0 + z * g), rt * (rt - s))
        return np.where(eta >= 0.0, y * wc + (1.0 - y) * wt, y * wt + (1.0 - y) * wc), none
    if family == "gaussian":
        return np.broadcast_to(np.asarray(tau, dtype=np.float64), np.shape(eta)).copy(), none
    raise ValueError(family)


def problem(family, A, y, offset, counts, lam, tau, k):
    """problem k of a batch as the restatement takes it: its valid rows only"""
    N = A.shape[1]
    n = N if counts is None else int(min(max(int(counts[k]), 0), N))
    return {"family": family, "A": np.asarray(A[k, :n], dtype=np.float64), "y": np.asarray(y[k, :n], dtype=np.float64),
            "o": np.zeros(n) if offset is None else np.asarray(offset[k, :n], dtype=np.float64),
            "lam": float(np.broadcast_to(lam, (A.shape[0],))[k]), "tau": float(np.broadcast_to(tau, (A.shape[0],))[k])}


def evaluate(p, x):
    """f = -lp, g = -score, H at x and the scales of the three sums; non-finite x or a flagged row: f = NaN, g = H = NaN"""
    A, lam = p["A"], p["lam"]
    D = A.shape[1]
    with np.errstate(all="ignore"):
        eta = A @ x + p["o"]
        r, t, flag = gref.link(p["family"], eta, p["y"], p["tau"])
        w, flag2 = weights(p["family"], eta, p["y"], p["tau"])
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


def neg_hessian(family, A, y, offset, counts, lam, tau, X):
    """(K, D, D) at the rows of X (K, D)"""
    X = np.asarray(X, dtype=np.float64)
    return np.stack([evaluate(problem(family, A, y, offset, counts, lam, tau, k), X[k])[2] for k in range(A.shape[0])])


def chol_info(H):
    """the kernel's factorisation verdict: 0, or 1 + the first pivot that is not finite or not > 64 eps H_jj (right-looking)"""
    S = np.array(H, dtype=np.float64)
    D = S.shape[0]
    dg = np.diag(S).copy()
    with np.errstate(all="ignore"):
        for c in range(D):
            a = S[c, c]
            if not (a > PIVOT_REL * dg[c] and a < np.inf):
                return c + 1
            v = S[c, c + 1:] / np.sqrt(a)
            S[c + 1:, c + 1:] -= np.outer(v, v)
    return 0


def inverse(H):
    """(cov, info) of gsmvi_glm_hessian_batched_f64: the identity where the factorisation fails"""
    info = chol_info(H) if np.isfinite(H).all() else 1
    return (np.linalg.inv(H) if info == 0 else np.eye(H.shape[0])), info


def new_state(x0):
    D = len(x0)
    x0 = np.array(x0, dtype=np.float64)
    return {"x": x0.copy(), "g": np.zeros(D), "d": np.zeros(D), "Xt": x0.copy(), "f": 0.0, "t": 0.0, "gd": 0.0, "status": 0,
            "nit": 0, "nfev": 0, "nls": 0}


def _direction(s, g, H, sc, notes):
    """factor H; d = -H^{-1} g, t = 1, g.d, Xt = x + d, or status 5"""
    info = chol_info(H)
    notes["info"] = info
    if info != 0:
        s["status"] = 5
        return
    Hi = np.linalg.inv(H)
    d = -np.linalg.solve(H, g)
    s["d"], s["t"], s["gd"], s["nls"] = d, 1.0, float(g @ d), 0
    s["Xt"] = s["x"] + d
    sd = np.abs(Hi).sum(1).max() * sc["g"].max() + np.abs(d).max()
    notes["scale_d"] = sd
    notes["scale_gd"] = float(np.abs(g) @ np.abs(d) + sc["g"] @ np.abs(d) + np.abs(g).sum() * sd)


def step(p, before, start, maxiter=100, maxfun=200, gtol=1e-8):
    """one launch for one problem: (state after, notes); notes: the scales of what was written and the margins of the decisions
    (``armijo``: |rhs - ft| / max(1, |f|); ``gmax``: max|g| where it was tested against gtol)"""
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in before.items()}
    notes = {}
    if not start and s["status"] != 0:
        return s, notes                                                 # frozen
    ft, gt, H, sc = evaluate(p, s["Xt"])
    notes["scale_f"], notes["scale_g"] = sc["f"], sc["g"]
    fin = bool(np.isfinite(ft) and np.isfinite(gt).all())
    if start:
        s.update(x=s["Xt"].copy(), f=ft, g=gt, d=np.zeros_like(gt), t=0.0, gd=0.0, nfev=1, nit=0, nls=0, status=0)
        if not fin:
            s["status"] = 4
        else:
            notes["gmax"] = float(np.abs(gt).max())
            if notes["gmax"] <= gtol:
                s["status"] = 1
            else:
                _direction(s, gt, H, sc, notes)
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
        _direction(s, gt, H, sc, notes)
    return s, notes


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


def pack(states):
    """states -> the packed arrays of include/gsmvi_hip.h: x, g, d, Xt (K, D), sc (K, 4), ist (K, 8) int32"""
    out = {k: np.stack([s[k] for s in states]) for k in ("x", "g", "d", "Xt")}
    out["sc"] = np.array([[s["f"], s["t"], s["gd"], 0.0] for s in states], dtype=np.float64)
    out["ist"] = np.array([[s["status"], s["nit"], s["nfev"], s["nls"], 0, 0, 0, 0] for s in states], dtype=np.int32)
    return out


def inputs(family, shape, seed=None):
    K, N, D = shape
    return gref.make_inputs(family, K, N, D, 1, seed=SEEDS.get((family, shape)) if seed is None else seed)


@functools.lru_cache(maxsize=None)
def trajectories(family, shape, with_offset):
    """the step test's runs at ``shape``: every problem of make_inputs from x0 = 0 at gtol = STEP_GTOL, as
    [(problem index, final state, [(before, after, notes), ...]), ...]; computed once and shared (do not modify)"""
    A, y, offset, counts, lam, tau, _ = inputs(family, shape)
    out = []
    for k in range(shape[0]):
        p = problem(family, A, y, offset if with_offset else None, counts, lam, tau, k)
        s, rec = run(p, np.zeros(shape[2]), record=True, gtol=STEP_GTOL, maxiter=30, maxfun=60)
        out.append((k, s, rec))
    return out


class StandInEngine(gref.RestatementEngine):
    """the engine calls of ``laplace_init_batched`` and ``neg_hessian`` on numpy and the restatement"""
    name = "restatement-laplace(test-only)"

    def _problems(self, A, y, family, offset, counts, prior_prec, noise_prec):
        return [problem(family, A, y, offset, counts, prior_prec, noise_prec, k) for k in range(A.shape[0])]

    def glm_hessian_batched(self, X, A, y, family, offset=None, counts=None, prior_prec=1.0, noise_prec=1.0, want="h", out=None,
                            cov_out=None, info_out=None):
        self.calls.append(("hessian", family, want))
        H = neg_hessian(family, A, y, offset, counts, prior_prec, noise_prec, X)
        if want == "h":
            return H
        ci = [inverse(h) for h in H]
        cov, info = np.stack([c for c, _ in ci]), np.array([i for _, i in ci], dtype=np.int32)
        return (cov, info) if want == "cov" else (H, cov, info)

    def laplace_state_batched(self, x0):
        self.calls.append("laplace_state")
        st = pack([new_state(x) for x in np.asarray(x0, dtype=np.float64)])
        st["stopped"] = np.zeros(1, dtype=np.int32)
        return st

    def laplace_step_batched(self, state, A, y, family, offset=None, counts=None, prior_prec=1.0, noise_prec=1.0, start=False,
                             maxiter=100, maxfun=200, gtol=1e-8):
        self.calls.append(("laplace_step", family, bool(start)))
        ps = self._problems(A, y, family, offset, counts, prior_prec, noise_prec)
        for k, p in enumerate(ps):
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

    def read_flag(self, flag):
        self.calls.append("read_flag")
        return int(flag[0])

    def read_ints(self, t):
        return np.asarray(t).astype(np.int64)



def check_bad_arguments(lib):
    """both entry points through the C ABI with a NULL context: every bad argument returns GSMVI_ERR_BAD_ARG (1) with its own
    message, so nothing can have been enqueued; valid calls end at the context"""
    import ctypes as C
    buf = (C.c_double * 8192)()
    p = C.cast(buf, C.c_void_p).value
    a = lambda n: p + 8 * 512 * n                                   # noqa: E731  sixteen disjoint 4 KB arrays
    err = lambda: (lib.gsmvi_last_error() or b"").decode()           # noqa: E731

    def hess(K=2, D=4, N=5, family=1, A=a(0), y=a(1), offset=a(2), counts=a(3), tau=1.0, tau_dev=None, lam=1.0, lam_dev=None,
             X=a(4), H=a(5), cov=a(6), info=a(7)):
        return lib.gsmvi_glm_hessian_batched_f64(None, None, K, D, N, family, A, y, offset, counts, tau, tau_dev, lam, lam_dev, X,
                                                 H, cov, info)

    def step(K=2, D=4, N=5, family=1, A=a(0), y=a(1), offset=a(2), counts=a(3), tau=1.0, tau_dev=None, lam=1.0, lam_dev=None,
             start=0, x=a(4), g=a(5), d=a(6), sc=a(7), ist=a(8), Xt=a(9), stopped=a(10), maxiter=10, maxfun=20, gtol=1e-8):
        return lib.gsmvi_laplace_step_batched_f64(None, None, K, D, N, family, A, y, offset, counts, tau, tau_dev, lam, lam_dev,
                                                  start, x, g, d, sc, ist, Xt, stopped, maxiter, maxfun, gtol)

    for call, name in ((hess, "gsmvi_glm_hessian_batched_f64"), (step, "gsmvi_laplace_step_batched_f64")):
        assert call(D=0) == 1 and "D must be" in err() and name in err()
        assert call(D=65) == 1 and "D must be" in err()
        assert call(K=0) == 1 and "K must be" in err()
        assert call(N=0) == 1 and "N must be" in err()
        assert call(K=2 ** 20, N=2 ** 40) == 1 and "too large" in err()
        for fam in (-1, 4):
            assert call(family=fam) == 1 and "family" in err(), fam
        for arr in ("A", "y"):
            assert call(**{arr: None}) == 1 and "NULL array" in err(), arr
        assert call(lam=-1.0) == 1 and "prior_prec" in err()
        assert call(tau=2.0) == 1 and "noise_prec" in err()
        assert call(family=3, tau=0.0) == 1 and "noise_prec" in err()
        for fam in (0, 1, 2, 3):
            assert call(family=fam) == 1 and "ctx is NULL" in err(), fam
        assert call(offset=None, counts=None, lam_dev=a(11)) == 1 and "ctx is NULL" in err()
        assert call(y=a(0), offset=a(0), counts=a(0)) == 1 and "ctx is NULL" in err()       # read-only arrays may overlap
    assert hess(X=None) == 1 and "NULL array" in err()
    assert hess(H=None, cov=None, info=None) == 1 and "H or cov" in err()
    assert hess(info=None) == 1 and "info_dev is required" in err()                         # cov without info_dev
    assert hess(cov=None) == 1 and "info_dev is required" in err()                          # and info_dev without cov
    assert hess(cov=None, info=None) == 1 and "ctx is NULL" in err()
    assert hess(H=None) == 1 and "ctx is NULL" in err()
    for w in ("H", "cov", "info"):
        for arr, where in (("A", a(0)), ("y", a(1)), ("offset", a(2)), ("counts_dev", a(3)), ("X", a(4))):
            assert hess(**{w: where}) == 1 and f"{w if w != 'info' else 'info_dev'} overlaps {arr}" in err(), (w, arr)
    assert hess(cov=a(5)) == 1 and "cov overlaps H" in err()
    assert hess(H=a(4) + 8 * (2 * 4 - 1)) == 1 and "H overlaps X" in err()                  # the last element of X
    assert hess(H=a(4) + 8 * 2 * 4) == 1 and "ctx is NULL" in err()                         # adjacent is not overlapping
    for arr in ("x", "g", "d", "sc", "ist", "Xt"):
        assert step(**{arr: None}) == 1 and "NULL array" in err(), arr
        assert step(**{arr: a(0)}) == 1 and f"{arr} overlaps A" in err(), arr
        assert step(**{arr: a(10)}) == 1 and "overlaps" in err() and "stopped_dev" in err(), arr
    assert step(g=a(4)) == 1 and "g overlaps x" in err()
    assert step(stopped=None) == 1 and "ctx is NULL" in err()
    assert step(maxfun=1) == 1 and "maxfun at least 2" in err()
    assert step(maxiter=0) == 1 and "maxiter must be at least 1" in err()
    assert step(gtol=-1.0) == 1 and "gtol" in err()
    assert step(gtol=float("nan")) == 1 and "gtol" in err()
    assert step(start=1) == 1 and "ctx is NULL" in err()
