"""Numpy restatement of the batched softmax Laplace initialiser (gsmvi_softmax_hessian_batched_f64,
gsmvi_softmax_laplace_step_batched_f64, csrc/gsmvi_softmax_laplace_batched.hip) and a stand-in engine for the host logic of
``laplace_init_softmax_batched`` and ``BatchedSoftmaxTarget.neg_hessian``.  Test-only.  For problem k (softmax_batched_ref's
model: class C - 1 the reference class, x[c P + j] = W_cj), with p_nc = exp(eta_nc - m_n) / s_n, d = c P + i, d' = c' P + j:

    H_k(x)[d, d'] = sum_{n < n_k} w_n,cc' a_ni a_nj + lam_k [d = d'],   w_n,cc = p_nc (1 - p_nc),   w_n,cc' = -p_nc p_nc'
    phi = -lp,   g = -score,   d_newton = -H^{-1} g

1 - p is in the kernel's form, a sum over the other classes: c* the first class that attains m (e_c* = 1 exactly), s_rest =
sum_{c != c*} e_c, s = 1 + s_rest, 1 - p_c* = s_rest / s and 1 - p_c = (s - e_c) / s elsewhere; the residual is 1 - p_nc where
y_n = c and -p_nc elsewhere.  The step is the state machine of include/gsmvi_hip.h word for word (laplace_batched_ref's, on this
module's ``evaluate``), ``run`` records the state after every launch, and every summed quantity comes with its scale, the sum of
the absolute values of its terms.  It is pinned to torch autograd of the written density, to softmax_batched_ref and to scipy in
tests/test_softmax_laplace_cpu.py."""
import functools

import numpy as np

import softmax_batched_ref as sref
from laplace_batched_ref import chol_info, inverse, new_state, pack            # noqa: F401  (shared with the GLM restatement)

# (K, N, C, P) of the GPU tests: the four-problem packing; D = 10; four classes inside one MFMA block with N one past two tiles;
# C = 2 with N one past a tile; the first padded D, every entry its own class; class boundaries that straddle blocks; a class
# block of two MFMA blocks; and the other corners of D = 64
SHAPES = ((5, 40, 3, 2), (6, 70, 3, 5), (5, 65, 5, 4), (5, 33, 2, 16), (5, 65, 18, 1), (5, 70, 4, 11), (4, 70, 3, 32),
          (4, 150, 9, 8), (4, 40, 65, 1), (4, 150, 2, 64))
SATURATED = ((70, 3, 5), (65, 5, 4), (33, 2, 16), (40, 9, 8), (40, 17, 1))
STEP_GTOL = 1e-6
# ``inputs`` seeds of the step test's trajectories where the default one puts a decision on its threshold
# (tests/test_softmax_laplace_cpu.py asserts the margins for every shape, listed or not): (K, N, C, P) -> seed
SEEDS = {(4, 70, 3, 32): 1, (4, 40, 65, 1): 1, (4, 150, 2, 64): 1}


def problem(A, y, C, counts, lam, k):
    """problem k of a batch as the restatement takes it: its valid rows only"""
    N = A.shape[1]
    n = N if counts is None else int(min(max(int(counts[k]), 0), N))
    return {"A": np.asarray(A[k, :n], dtype=np.float64), "y": np.asarray(y[k, :n]).astype(np.int64), "C": int(C),
            "lam": float(np.broadcast_to(lam, (A.shape[0],))[k])}


def probabilities(A, x, C):
    """eta (n, C), m, s_rest, p and the accurate 1 - p (n, C) in the kernel's forms, in the dtype of A and x"""
    n, P = A.shape
    dt = np.result_type(A.dtype, x.dtype)
    eta = np.concatenate([A @ x.reshape(C - 1, P).T, np.zeros((n, 1), dtype=dt)], axis=1)
    rows = np.arange(n)
    cs = np.argmax(eta, axis=1) if n else np.zeros(0, dtype=np.int64)           # the first class that attains the maximum
    m = eta[rows, cs]
    e = np.exp(eta - m[:, None])
    e[rows, cs] = 1.0
    others = e.copy()
    others[rows, cs] = 0.0
    rest = others.sum(axis=1)
    s = 1.0 + rest
    p = e / s[:, None]
    q = (s[:, None] - e) / s[:, None]
    q[rows, cs] = rest / s
    return eta, m, rest, p, q


def evaluate(p, x):
    """f = -lp, g = -score, H at x and the scales of the three sums; a non-finite x or eta: f = NaN, g = H = NaN.  The arithmetic
    runs in the dtype of x (float64, or np.longdouble for the accuracy tests)."""
    x = np.asarray(x)
    dt = x.dtype
    A, y, C, lam = p["A"].astype(dt), p["y"], p["C"], dt.type(p["lam"])
    n, P = A.shape
    Cm = C - 1
    D = Cm * P
    with np.errstate(all="ignore"):
        eta, m, rest, pr, q = probabilities(A, x, C)
        hot = y[:, None] == np.arange(C)[None, :]
        t = (eta * hot).sum(axis=1) - m - sref.log_s(rest, 1 + rest)    # (log(s) is 0 where s_rest < eps / 2)
        r = np.where(hot, q, -pr)[:, :Cm]
        f = -(t.sum() - 0.5 * lam * (x * x).sum())
        g = -((r.T @ A).reshape(D) - lam * x)
        sf = np.abs(t).sum() + 0.5 * lam * (x * x).sum()
        sg = (np.abs(r).T @ np.abs(A)).reshape(D) + lam * np.abs(x)
        H, sH = np.zeros((D, D), dtype=dt), np.zeros((D, D), dtype=dt)
        aA = np.abs(A)
        for c in range(Cm):
            for c2 in range(Cm):
                w = pr[:, c] * q[:, c] if c == c2 else -(pr[:, c] * pr[:, c2])
                H[c * P:(c + 1) * P, c2 * P:(c2 + 1) * P] = (A * w[:, None]).T @ A
                sH[c * P:(c + 1) * P, c2 * P:(c2 + 1) * P] = (aA * np.abs(w)[:, None]).T @ aA
        H, sH = H + lam * np.eye(D, dtype=dt), sH + lam * np.eye(D, dtype=dt)
    H = 0.5 * (H + H.T)
    if not np.isfinite(x).all() or not np.isfinite(eta).all():
        f, g, H = dt.type(np.nan), np.full(D, np.nan, dtype=dt), np.full((D, D), np.nan, dtype=dt)
    return f, g, H, {"f": sf, "g": sg, "H": sH}


def hessian_difference_of_grams(p, x):
    """H as sum p a a^T - sum p^2 a a^T on the diagonal class blocks: the form the specification rules out (the accuracy test
    shows that it misses the bar)"""
    x = np.asarray(x, dtype=np.float64)
    A, C, lam = p["A"], p["C"], p["lam"]
    P = A.shape[1]
    Cm = C - 1
    _, _, _, pr, _ = probabilities(A, x, C)
    H = np.zeros((Cm * P, Cm * P))
    for c in range(Cm):
        for c2 in range(Cm):
            if c == c2:
                blk = (A * pr[:, c][:, None]).T @ A - (A * (pr[:, c] * pr[:, c])[:, None]).T @ A
            else:
                blk = -((A * (pr[:, c] * pr[:, c2])[:, None]).T @ A)
            H[c * P:(c + 1) * P, c2 * P:(c2 + 1) * P] = blk
    return H + lam * np.eye(Cm * P)


def neg_hessian(A, y, C, counts, lam, X):
    """(K, D, D) at the rows of X (K, D)"""
    X = np.asarray(X, dtype=np.float64)
    return np.stack([evaluate(problem(A, y, C, counts, lam, k), X[k])[2] for k in range(A.shape[0])])


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
    ft = float(ft)
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


def inputs(shape, seed=None, flat0=True):
    """softmax_batched_ref.make_inputs at (K, N, C, P) with one row of X, problem 1 given a count of 0, and (``flat0`` false)
    a proper prior for problem 0 too: A, y, counts, lam, X (K, D)"""
    K, N, C, P = shape
    A, y, counts, lam, X = sref.make_inputs(K, N, C, P, 1, seed=SEEDS.get(shape) if seed is None else seed)
    counts[1] = 0
    if not flat0:
        lam[0] = 0.05
    return A, y, counts, lam, X[:, 0]


def saturated_inputs(N, C, P, top=25.0):
    """the inputs that saturate one class: intercept column 1, the other columns 0.3 N(0, 1), W = 0.5 N(0, 1) with W_00 = ``top``
    (25 .. 30), lam = 0: a problem dict and its x"""
    rs = np.random.RandomState(1000 + N + 64 * C + P)
    A = 0.3 * rs.standard_normal((N, P))
    A[:, 0] = 1.0
    W = 0.5 * rs.standard_normal((C - 1, P))
    W[0, 0] = top
    y = rs.randint(0, C, size=N)
    return {"A": A, "y": y.astype(np.int64), "C": C, "lam": 0.0}, W.reshape(-1)


@functools.lru_cache(maxsize=None)
def trajectories(shape):
    """the step test's runs at ``shape``: every problem of ``inputs`` (proper priors) from x0 = 0 at gtol = STEP_GTOL, as
    [(problem index, final state, [(before, after, notes), ...]), ...]; computed once and shared (do not modify)"""
    A, y, counts, lam, _ = inputs(shape, flat0=False)
    K, _, C, P = shape
    out = []
    for k in range(K):
        s, rec = run(problem(A, y, C, counts, lam, k), np.zeros((C - 1) * P), record=True, gtol=STEP_GTOL, maxiter=30, maxfun=60)
        out.append((k, s, rec))
    return out


class StandInEngine(sref.RestatementEngine):
    """the engine calls of ``laplace_init_softmax_batched`` and ``neg_hessian`` on numpy and the restatement"""
    name = "restatement-softmax-laplace(test-only)"

    def softmax_hessian_batched(self, X, A, labels, num_classes, counts=None, prior_prec=1.0, want="h", out=None, cov_out=None,
                                info_out=None):
        self.calls.append(("softmax_hessian", num_classes, want))
        H = neg_hessian(A, labels, num_classes, counts, prior_prec, X)
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

    def softmax_laplace_step_batched(self, state, A, labels, num_classes, counts=None, prior_prec=1.0, start=False, maxiter=100,
                                     maxfun=200, gtol=1e-8):
        self.calls.append(("softmax_laplace_step", num_classes, bool(start)))
        for k in range(A.shape[0]):
            p = problem(A, labels, num_classes, counts, prior_prec, k)
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

    def hess(K=2, Cc=3, P=2, N=5, A=a(0), labels=a(1), counts=a(3), lam=1.0, lam_dev=None, X=a(4), H=a(5), cov=a(6), info=a(7)):
        return lib.gsmvi_softmax_hessian_batched_f64(None, None, K, Cc, P, N, A, labels, counts, lam, lam_dev, X, H, cov, info)

    def step(K=2, Cc=3, P=2, N=5, A=a(0), labels=a(1), counts=a(3), lam=1.0, lam_dev=None, start=0, x=a(4), g=a(5), d=a(6),
             sc=a(7), ist=a(8), Xt=a(9), stopped=a(10), maxiter=10, maxfun=20, gtol=1e-8):
        return lib.gsmvi_softmax_laplace_step_batched_f64(None, None, K, Cc, P, N, A, labels, counts, lam, lam_dev, start, x, g, d,
                                                          sc, ist, Xt, stopped, maxiter, maxfun, gtol)

    for call, name in ((hess, "gsmvi_softmax_hessian_batched_f64"), (step, "gsmvi_softmax_laplace_step_batched_f64")):
        assert call(Cc=1) == 1 and "C must be" in err() and name in err()
        assert call(P=0) == 1 and "P must be" in err()
        assert call(Cc=3, P=33) == 1 and "D = (C - 1) P" in err()
        assert call(Cc=66, P=1) == 1 and "D = (C - 1) P" in err()
        assert call(Cc=2 ** 30, P=2 ** 30) == 1 and "D = (C - 1) P" in err()
        assert call(K=0) == 1 and "K must be" in err()
        assert call(N=0) == 1 and "N must be" in err()
        assert call(K=2 ** 20, N=2 ** 40) == 1 and "too large" in err()
        for arr in ("A", "labels"):
            assert call(**{arr: None}) == 1 and "NULL array" in err(), arr
        assert call(lam=-1.0) == 1 and "prior_prec" in err()
        assert call(lam=float("inf")) == 1 and "prior_prec" in err()
        assert call(lam=float("nan")) == 1 and "prior_prec" in err()
        for Cc, P in ((2, 1), (3, 2), (2, 16), (18, 1)):                # (H and cov of K = 1 fit the 4 KB arrays up to D = 22)
            assert call(Cc=Cc, P=P, K=1, N=1) == 1 and "ctx is NULL" in err(), (Cc, P)
        assert call(counts=None, lam=-1.0, lam_dev=a(11)) == 1 and "ctx is NULL" in err()   # (the scalar is unused with K values)
        assert call(labels=a(0), counts=a(0)) == 1 and "ctx is NULL" in err()               # read-only arrays may overlap
    assert hess(X=None) == 1 and "NULL array" in err()
    assert hess(H=None, cov=None, info=None) == 1 and "H or cov" in err()
    assert hess(info=None) == 1 and "info_dev is required" in err()                         # cov without info_dev
    assert hess(cov=None) == 1 and "info_dev is required" in err()                          # and info_dev without cov
    assert hess(cov=None, info=None) == 1 and "ctx is NULL" in err()
    assert hess(H=None) == 1 and "ctx is NULL" in err()
    for w in ("H", "cov", "info"):
        for arr, where in (("A", a(0)), ("labels", a(1)), ("counts_dev", a(3)), ("X", a(4))):
            assert hess(**{w: where}) == 1 and f"{w if w != 'info' else 'info_dev'} overlaps {arr}" in err(), (w, arr)
        assert hess(lam_dev=a(11), **{w: a(11)}) == 1 and "overlaps prior_prec_dev" in err(), w
    assert hess(cov=a(5)) == 1 and "cov overlaps H" in err()
    assert hess(H=a(4) + 8 * (2 * 4 - 1)) == 1 and "H overlaps X" in err()                  # the last element of X
    assert hess(H=a(4) + 8 * 2 * 4) == 1 and "ctx is NULL" in err()                         # adjacent is not overlapping
    for arr in ("x", "g", "d", "sc", "ist", "Xt"):
        assert step(**{arr: None}) == 1 and "NULL array" in err(), arr
        assert step(**{arr: a(0)}) == 1 and f"{arr} overlaps A" in err(), arr
        assert step(**{arr: a(1)}) == 1 and f"{arr} overlaps labels" in err(), arr
        assert step(**{arr: a(10)}) == 1 and "overlaps" in err() and "stopped_dev" in err(), arr
    assert step(g=a(4)) == 1 and "g overlaps x" in err()
    assert step(stopped=None) == 1 and "ctx is NULL" in err()
    assert step(maxfun=1) == 1 and "maxfun at least 2" in err()
    assert step(maxiter=0) == 1 and "maxiter must be at least 1" in err()
    assert step(gtol=-1.0) == 1 and "gtol" in err()
    assert step(gtol=float("nan")) == 1 and "gtol" in err()
    assert step(start=1) == 1 and "ctx is NULL" in err()
