"""Numpy restatements of the ordinal Laplace initialiser (gsmvi_ordinal_hessian_batched_f64,
gsmvi_ordinal_laplace_step_batched_f64, csrc/gsmvi_ordinal_laplace_batched.hip, the curvature of csrc/gsmvi_ordinal_link.h) and a
stand-in engine for the host logic of ``laplace_init_ordinal_batched`` and ``neg_hessian_ordinal_batched``.  Test-only.  The model is
ordinal_batched_ref's; at x = (beta, delta), w_0 = 1, w_i = e^{delta_i}, q_i = 1 / expm1(w_i), fa = sigma(a) sigma(-a) (0 for
y = 0), fb = sigma(b) sigma(-b) (0 for y = C - 1) and per (row n, cutpoint i)

    e_ni = fa + fb (i < y_n), fb (i = y_n), 0 (i > y_n)          s_ni = -r_eta,n (i < y_n), sigma(-b_n) (i = y_n), 0 (i > y_n)
    F(i) = sum_n e_ni,   S_i = sum_n s_ni + q_i cnt_i,   cnt_i = #{n : y_n = i} (1 <= i <= C - 2),   c_i = -w_i S_i (i >= 1), c_0 = 0
    f = -lp,   g = -score = -(sum_n r_eta a_n - lam beta,  w_i S_i - kap delta_i)
    H[:P, :P] = sum_n (fa + fb) a a^T + lam I,   H[:P, P + i] = -w_i sum_n e_ni a_n,   H[P + i, P + i'] = w_i w_i' F(max(i, i'))
    H[P + i, P + i] = w_i^2 F(i) + (w_i q_i)(w_i + w_i q_i) cnt_i + c_i + kap

``evaluate`` is the restatement of the kernel's forms in float64 or, with L = np.longdouble, in long double (the reference of the
GPU tests), with the scale of every entry (the sum of the magnitudes of its terms, plus the prior) and the chain terms c.
``factor`` is the kernel's right-looking factorisation with the relative pivot rule and, with ``rule``, the retry rule of
include/gsmvi_hip.h: a failed factorisation with some c_i < 0 is repeated once on H - diag(min(c, 0)); ``step`` is the state
machine of gsmvi_laplace_step_batched_f64 on these, ``run`` the whole iteration.  Pinned in tests/test_ordinal_laplace_cpu.py."""
import functools

import numpy as np

import laplace_batched_ref as lref
import ordinal_batched_ref as oref
from laplace_batched_ref import new_state, PIVOT_REL                        # noqa: F401
from ordinal_batched_ref import make_inputs, W_MIN                          # noqa: F401

STEP_GTOL = lref.STEP_GTOL
STEP_K = 5
MOD_MARGIN = 1e-6                       # every replayed pivot test: |pivot| >= MOD_MARGIN m, m the magnitudes it is the difference of
# (N, P, C) of the GPU tests: D = P + C - 1 in {2, 3, 16, 17, 32, 33, 48, 49, 64}; C = 2, small C with large P and large C with
# P = 1 among them; P = 15 and P = 16 (delta_0 the last column of an MFMA block and the first of the next); N in {1, 31, 32, 33, 70}
SHAPES = ((33, 1, 2), (70, 2, 2), (31, 15, 2), (70, 16, 2), (32, 15, 18), (70, 16, 18), (33, 40, 9), (70, 1, 49), (70, 63, 2),
          (70, 62, 3), (70, 1, 64))
SMALL_N = ((1, 9, 4), (31, 9, 4), (32, 9, 4), (33, 9, 4), (1, 16, 5), (33, 16, 5))
# the step test's sets: (N, P, C); from x0 = 0 the retry rule fires on those with C >= 8 (RETRY_SHAPES; on
# some of the others too), from near the mode on none
STEP_SHAPES = ((33, 1, 3), (70, 2, 5), (70, 9, 8), (40, 15, 2), (70, 16, 4), (120, 3, 30), (90, 40, 17))
RETRY_SHAPES = tuple(s for s in STEP_SHAPES if s[2] >= 8)
# ((N, P, C), with_offset, near) -> seed where the default 0 puts a decision on its threshold (tests/test_ordinal_laplace_cpu.py
# asserts the margins of every entry, default or not)
SEEDS = {((70, 2, 5), True, False): 1, ((70, 2, 5), False, False): 2, ((70, 9, 8), False, False): 1, ((40, 15, 2), True, False): 1,
         ((40, 15, 2), False, False): 1, ((70, 16, 4), True, True): 1, ((70, 16, 4), False, True): 1,
         ((120, 3, 30), False, False): 1, ((120, 3, 30), True, True): 1, ((120, 3, 30), False, True): 2}


def problem(A, y, offset, counts, lam, kap, C, k):
    """problem k of a batch as the restatement takes it: its valid rows only, the labels clamped as the kernel stages them"""
    K, N = np.shape(y)
    n = N if counts is None else int(min(max(int(counts[k]), 0), N))
    bc = lambda v: float(np.broadcast_to(np.asarray(v, dtype=np.float64), (K,))[k])          # noqa: E731
    return {"A": np.asarray(A[k, :n], dtype=np.float64), "y": np.clip(np.asarray(y[k, :n]).astype(np.int64), 0, C - 1),
            "o": np.zeros(n) if offset is None else np.asarray(offset[k, :n], dtype=np.float64), "lam": bc(lam), "kap": bc(kap),
            "C": int(C)}


def flagged(x, P):
    """the kernel's flag: a non-finite x, or some e^{delta_j}, j >= 1, that is not a positive normal number"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        w = np.exp(x[P + 1:])
    return not np.isfinite(x).all() or not ((w >= W_MIN) & (w < np.inf)).all()


def _spsf(z):
    """softplus(z), sigma(z), sigma(z) sigma(-z) from one exponential: ord_spsf"""
    e = np.exp(-np.abs(z))
    q = 1 + e
    big, small = 1 / q, e / q
    return np.where(z > 0, z, 0) + np.log1p(e), np.where(z >= 0, big, small), big * small


def curv(eta, y, cut, lm):
    """(r_eta, sigma(-b), fa + fb, fb, t) per row and the magnitudes (|terms of r_eta|, |terms of t|): ord_link_curv, in eta's
    precision; y (n,) in 0 .. C - 1, cut and lm (C - 1,)"""
    lc = cut.shape[0]
    Z = eta.dtype.type(0)
    lo, hi = y >= 1, y <= lc - 1
    inn = lo & hi
    ya, yb = np.clip(y - 1, 0, lc - 1), np.clip(y, 0, lc - 1)
    spa, sga, fa = (np.where(lo, v, Z) for v in _spsf(cut[ya] - eta))
    spb, sgb, fb = (np.where(hi, v, Z) for v in _spsf(-(cut[yb] - eta)))
    lmy = np.where(inn, lm[yb], Z)
    t = (-spb - spa) + lmy
    return sga - sgb, sgb, fa + fb, fb, t, sga + sgb, spb + spa + np.abs(lmy)


def evaluate(p, x, L=np.float64):
    """f = -lp, g = -score, H at x = (beta, delta), and {"f", "g", "H"}: the scales of the sums, {"c"}: the chain terms (C - 1,);
    a flagged x: f = NaN, g = H = NaN.  L = np.longdouble: the high-precision restatement (results rounded to float64)."""
    A, o = np.asarray(p["A"], dtype=L), np.asarray(p["o"], dtype=L)
    y, C = p["y"], p["C"]
    lam, kap = L(p["lam"]), L(p["kap"])
    n, P = A.shape
    lc = C - 1
    D = P + lc
    x = np.asarray(x, dtype=L)
    beta, delta = x[:P], x[P:]
    with np.errstate(all="ignore"):
        w = np.exp(delta)
        w[0] = 1
        cut = np.empty(lc, dtype=L)
        cut[0] = delta[0]
        for j in range(1, lc):
            cut[j] = cut[j - 1] + w[j]
        lm, qe = oref.gap(w)
        lm[0], qe[0] = 0, 0
        eta = A @ beta + o
        re, sb, fab, fb, t, are, at_ = curv(eta, y, cut, lm)
        ii, yy = np.arange(lc)[None, :], y[:, None]
        below, at = ii < yy, ii == yy
        Z = L(0)
        E = np.where(below, fab[:, None], np.where(at, fb[:, None], Z))
        Sm = np.where(below, -re[:, None], np.where(at, sb[:, None], Z))
        aS = np.where(below, are[:, None], np.where(at, sb[:, None], Z))
        gapc = np.arange(lc) >= 1
        cnt = np.where(gapc, at.sum(0), 0).astype(L)
        F = E.sum(0)
        Sv = Sm.sum(0) + qe * cnt
        aSv = aS.sum(0) + qe * cnt
        c = np.where(gapc, -(w * Sv), Z)
        wq = w * qe
        gapt = (wq * (w + wq)) * cnt
        bb, dd = (beta * beta).sum(), (delta * delta).sum()
        f = -((t.sum() - L(0.5) * lam * bb) - L(0.5) * kap * dd)
        g = np.empty(D, dtype=L)
        g[:P] = -(re @ A - lam * beta)
        g[P:] = -(w * Sv - kap * delta)
        H = np.empty((D, D), dtype=L)
        Hbb = (A * fab[:, None]).T @ A + lam * np.eye(P, dtype=L)
        H[:P, :P] = L(0.5) * (Hbb + Hbb.T)
        H[:P, P:] = (A.T @ (-E)) * w[None, :]
        H[P:, :P] = H[:P, P:].T
        mx = np.maximum(ii, ii.T)
        Hdd = np.zeros((lc, lc), dtype=L)
        iu = np.triu_indices(lc, 1)
        Hdd[iu] = w[iu[0]] * (w[iu[1]] * F[iu[1]])
        Hdd = Hdd + Hdd.T
        Hdd[np.arange(lc), np.arange(lc)] = w * (w * F) + ((gapt + c) + kap)
        H[P:, P:] = Hdd
        aA = np.abs(A)
        sf = at_.sum() + L(0.5) * lam * bb + L(0.5) * kap * dd
        sg = np.empty(D, dtype=L)
        sg[:P] = are @ aA + lam * np.abs(beta)
        sg[P:] = w * aSv + kap * np.abs(delta)
        sH = np.empty((D, D), dtype=L)
        sH[:P, :P] = (aA * fab[:, None]).T @ aA + lam * np.eye(P, dtype=L)
        sH[:P, P:] = (aA.T @ E) * w[None, :]
        sH[P:, :P] = sH[:P, P:].T
        sdd = w[:, None] * (w[None, :] * F[mx])
        sdd[np.arange(lc), np.arange(lc)] = w * (w * F) + gapt + np.where(gapc, w * aSv, Z) + kap
        sH[P:, P:] = sdd
    f, g, H, c = float(f), g.astype(np.float64), H.astype(np.float64), c.astype(np.float64)
    if flagged(x.astype(np.float64), P):
        f, g, H = np.nan, np.full(D, np.nan), np.full((D, D), np.nan)
    return f, g, H, {"f": float(sf), "g": sg.astype(np.float64), "H": sH.astype(np.float64), "c": c}


def neg_hessian(A, y, offset, counts, lam, kap, C, X, L=np.float64):
    """(K, D, D) at the rows of X (K, D), and the scales (K, D, D)"""
    X = np.asarray(X, dtype=np.float64)
    out = [evaluate(problem(A, y, offset, counts, lam, kap, C, k), X[k], L) for k in range(X.shape[0])]
    return np.stack([o[2] for o in out]), np.stack([o[3]["H"] for o in out])


def _chol(H):
    """the kernel's right-looking factorisation with the pivot rule 64 eps H_jj: (info, R, margins); margins: |pivot| / m for every
    pivot tested up to and including the first that fails, m = |H_cc| + sum_{c' < c} R[c', c]^2"""
    S = np.array(H, dtype=np.float64)
    D = S.shape[0]
    dg = np.diag(S).copy()
    pv = np.zeros(D)
    info = 0
    margins = []
    with np.errstate(all="ignore"):
        for c in range(D):
            a = S[c, c]
            if info == 0:
                m = abs(dg[c]) + (abs(dg[c] - a) if np.isfinite(a) else 0.0)
                margins.append(abs(a) / m if m > 0 and np.isfinite(a) else 0.0)
                if not (a > PIVOT_REL * dg[c] and a < np.inf):
                    info = c + 1
            pv[c] = np.sqrt(a)
            v = S[c, c + 1:] * (1.0 / pv[c])
            S[c + 1:, c + 1:] -= np.outer(v, v)
        R = np.zeros((D, D))
        for i in range(D):
            R[i, i + 1:] = S[i, i + 1:] / pv[i]
            R[i, i] = pv[i]
    return info, R, margins


def retried(H, c):
    """the retried matrix: H with min(c_i, 0) taken off the diagonal of the delta block"""
    H2 = np.array(H, dtype=np.float64)
    lc = len(c)
    P = H2.shape[0] - lc
    idx = P + np.arange(lc)
    H2[idx, idx] = H2[idx, idx] - np.minimum(c, 0.0)
    return H2


def factor(H, c=None, rule=False):
    """(info, R, notes) of the factorisation for a new direction.  info: 0, or 1 + the first failing pivot.  With ``rule``, a
    failure with some c_i < 0 is repeated once on ``retried(H, c)``: success gives info = 0 and notes["mod"] = True, failure the
    second info.  notes["margin"]: the smallest |pivot| / m of every pivot test made."""
    info, R, mar = _chol(H)
    notes = {"mod": False, "margin": min(mar)}
    if info != 0 and rule and c is not None and (np.asarray(c) < 0).any():
        info, R, mar2 = _chol(retried(H, c))
        notes["margin"] = min(mar + mar2)
        notes["mod"] = info == 0
    return info, R, notes


def inverse(H):
    """(cov, info) of gsmvi_ordinal_hessian_batched_f64: never modified; the identity where the factorisation fails"""
    info = _chol(H)[0] if np.isfinite(H).all() else 1
    return (np.linalg.inv(H) if info == 0 else np.eye(H.shape[0])), info


def _direction(s, g, H, sc, notes, rule):
    """factor H (with the retry rule when ``rule``); d = -(R^T R)^{-1} g, t = 1, g.d, Xt = x + d, or status 5"""
    info, R, fn = factor(H, sc["c"], rule)
    notes["info"], notes["mod"], notes["margin"] = info, fn["mod"], fn["margin"]
    if info != 0:
        s["status"] = 5
        return
    Hm = retried(H, sc["c"]) if fn["mod"] else H
    Hi = np.linalg.inv(Hm)
    d = -np.linalg.solve(Hm, g)
    s["d"], s["t"], s["gd"], s["nls"] = d, 1.0, float(g @ d), 0
    s["Xt"] = s["x"] + d
    s["nmod"] = s.get("nmod", 0) + int(fn["mod"])
    sd = np.abs(Hi).sum(1).max() * sc["g"].max() + np.abs(d).max()
    notes["scale_d"] = sd
    notes["scale_gd"] = float(np.abs(g) @ np.abs(d) + sc["g"] @ np.abs(d) + np.abs(g).sum() * sd)


def step(p, before, start, maxiter=100, maxfun=200, gtol=1e-8, rule=True, L=np.float64):
    """one launch for one problem: (state after, notes), laplace_batched_ref.step on this module's ``evaluate`` and ``factor``; the
    state carries ``nmod`` (ist[4]); notes: ``mod``, ``margin`` of the pivot tests, and lref.step's"""
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in before.items()}
    s.setdefault("nmod", 0)
    notes = {}
    if not start and s["status"] != 0:
        return s, notes                                                 # frozen
    ft, gt, H, sc = evaluate(p, s["Xt"], L)
    notes["scale_f"], notes["scale_g"] = sc["f"], sc["g"]
    fin = bool(np.isfinite(ft) and np.isfinite(gt).all())
    if start:
        s.update(x=s["Xt"].copy(), f=ft, g=gt, d=np.zeros_like(gt), t=0.0, gd=0.0, nfev=1, nit=0, nls=0, status=0, nmod=0)
        if not fin:
            s["status"] = 4
        else:
            notes["gmax"] = float(np.abs(gt).max())
            if notes["gmax"] <= gtol:
                s["status"] = 1
            else:
                _direction(s, gt, H, sc, notes, rule)
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
        _direction(s, gt, H, sc, notes, rule)
    return s, notes


def run(p, x0, record=False, maxiter=100, maxfun=200, gtol=1e-8, rule=True):
    """the whole iteration of one problem: the final state, and with ``record`` the list of (before, after, notes) per launch"""
    s = new_state(x0)
    s["nmod"] = 0
    rec = []
    for r in range(maxfun):
        after, notes = step(p, s, r == 0, maxiter, maxfun, gtol, rule)
        rec.append((s, after, notes))
        s = after
        if s["status"] != 0:
            break
    return (s, rec) if record else s


def pack(states):
    """states -> the packed arrays of include/gsmvi_hip.h, ist[4] = nmod"""
    out = lref.pack(states)
    out["ist"][:, 4] = [s.get("nmod", 0) for s in states]
    return out


# ---- the named test sets of the convergence tests (16 problems each) -------------------------------------------------------------
SETS = {"c3": (33, 1, 3), "c5": (64, 6, 5), "c8": (70, 9, 8), "c17": (256, 10, 17), "c30": (200, 3, 30)}
SET_K = 16
# what tests/test_ordinal_laplace_cpu.py asserts on these sets at the defaults (lam = kap = 1, x0 = 0): plain Newton (rule off) ends
# at least this many problems of the set with status 5; with the rule every problem converges
SET_PLAIN_STATUS5_MIN = {"c3": 0, "c5": 0, "c8": 1, "c17": 1, "c30": 1}


def make_problems(N, P, C, K=SET_K, seed=0, lam=1.0, kap=1.0):
    """K well-posed problems: ordinal_batched_ref.make_inputs(seed = 5 + seed, no poison) with every row valid and the priors
    lam, kap.  Returns A, y, offset, None, lam, kap, C."""
    A, y, offset = make_inputs(K, N, P, C, 1, seed=5 + seed, poison=False)[:3]
    return A, y, offset, None, lam, kap, C


@functools.lru_cache(maxsize=None)
def set_runs(name, rule):
    """the final states of the SET_K problems of SETS[name] from x0 = 0 at the defaults; computed once and shared"""
    N, P, C = SETS[name]
    inp = make_problems(N, P, C)
    return [run(problem(*inp, k), np.zeros(P + C - 1), rule=rule) for k in range(SET_K)]


# ---- the step test's trajectories ------------------------------------------------------------------------------------------------
def step_inputs(shape, with_offset=True, near=False, seed=None):
    """the STEP_K problems of the step test at (N, P, C) = ``shape`` (make_problems with the seed of SEEDS)"""
    N, P, C = shape
    inp = list(make_problems(N, P, C, K=STEP_K, seed=SEEDS.get((shape, with_offset, near), 0) if seed is None else seed))
    if not with_offset:
        inp[2] = None
    return tuple(inp)


@functools.lru_cache(maxsize=None)
def trajectories(shape, near, with_offset=True, seed=None):
    """the step test's runs at (N, P, C) = ``shape``: the STEP_K problems of ``step_inputs`` at gtol = STEP_GTOL from x0 = 0 (the
    retry rule fires at C >= 8) or, with ``near``, from the mode of a first run plus 0.05 N(0, 1) (it does not), as [(problem
    index, final state, [(before, after, notes), ...], x0), ...]; computed once and shared (do not modify)"""
    inp = step_inputs(shape, with_offset, near, seed)
    D = shape[1] + shape[2] - 1
    rs = np.random.RandomState(17)
    out = []
    for k in range(STEP_K):
        p = problem(*inp, k)
        x0 = np.zeros(D)
        if near:
            x0 = run(p, x0)["x"] + 0.05 * rs.standard_normal(D)
        s, rec = run(p, x0, record=True, gtol=STEP_GTOL, maxiter=40, maxfun=80)
        out.append((k, s, rec, x0))
    return out


def margins_hold(traj):
    """every run converged, no max|g| within a factor 1.5 of gtol, every Armijo decision by at least 1e-11 max(1, |f|), and every
    pivot test of every factorisation (first and retried) with |pivot| >= MOD_MARGIN m.  Returns (ok, smallest Armijo margin,
    smallest |pivot| / m, rounds whose direction came from the retried matrix)."""
    ok, low, mar, nmod = True, 1.0, np.inf, 0
    for _, st, rec, _ in traj:
        ok = ok and st["status"] == 1
        for _, _, notes in rec:
            if "gmax" in notes:
                ok = ok and not STEP_GTOL / 1.5 <= notes["gmax"] <= 1.5 * STEP_GTOL
            if "armijo" in notes:
                low = min(low, notes["armijo"])
            if "margin" in notes:
                mar = min(mar, notes["margin"])
            nmod += int(notes.get("mod", False))
            ok = ok and notes.get("info", 0) == 0
    return bool(ok and low >= 1e-11 and mar >= MOD_MARGIN), low, mar, nmod


class StandInEngine(oref.RestatementEngine, lref.StandInEngine):
    """the engine calls of ``laplace_init_ordinal_batched`` and ``neg_hessian_ordinal_batched`` on numpy and the restatement (the
    state, ``read_flag`` and ``read_ints`` are laplace_batched_ref.StandInEngine's); ``rule``: the retry rule on or off"""
    name = "restatement-ordinal-laplace(test-only)"

    def __init__(self, rule=True):
        super().__init__()
        self.rule = rule

    def ordinal_hessian_batched(self, X, A, y, C, offset=None, counts=None, prior_prec=1.0, cut_prec=1.0, want="h", out=None,
                                cov_out=None, info_out=None):
        self.calls.append(("ordinal_hessian", want))
        assert A.dtype == np.float64 and y.dtype == np.int32 and X.shape[1] == A.shape[2] + C - 1
        H = neg_hessian(A, y, offset, counts, prior_prec, cut_prec, C, X)[0]
        if want == "h":
            return H
        ci = [inverse(h) for h in H]
        cov, info = np.stack([c for c, _ in ci]), np.array([i for _, i in ci], dtype=np.int32)
        return (cov, info) if want == "cov" else (H, cov, info)

    def ordinal_laplace_step_batched(self, state, A, y, C, offset=None, counts=None, prior_prec=1.0, cut_prec=1.0, start=False,
                                     maxiter=100, maxfun=200, gtol=1e-8):
        self.calls.append(("ordinal_laplace_step", bool(start)))
        for k in range(y.shape[0]):
            p = problem(A, y, offset, counts, prior_prec, cut_prec, C, k)
            i = state["ist"][k]
            s = {"x": state["x"][k], "g": state["g"][k], "d": state["d"][k], "Xt": state["Xt"][k], "f": state["sc"][k, 0],
                 "t": state["sc"][k, 1], "gd": state["sc"][k, 2], "status": int(i[0]), "nit": int(i[1]), "nfev": int(i[2]),
                 "nls": int(i[3]), "nmod": int(i[4])}
            was = 0 if start else s["status"]
            a, _ = step(p, s, bool(start), maxiter, maxfun, gtol, self.rule)
            one = pack([a])
            for name in ("x", "g", "d", "Xt", "sc", "ist"):
                state[name][k] = one[name][0]
            if was == 0 and a["status"] != 0:
                state["stopped"][0] += 1


NAMES = ("gsmvi_ordinal_hessian_batched_f64", "gsmvi_ordinal_laplace_step_batched_f64")


def check_bad_arguments(lib):
    """both entry points through the C ABI with a NULL context, in the pattern of laplace_batched_ref.check_bad_arguments: every
    bad argument returns GSMVI_ERR_BAD_ARG (1) with its own message, so nothing can have been enqueued; valid calls end at the
    context.  The order of the checks: shape, priors, NULL arrays, overlaps, the context last."""
    import ctypes as C
    buf = (C.c_double * 8192)()
    p = C.cast(buf, C.c_void_p).value
    a = lambda n: p + 8 * 512 * n                                   # noqa: E731  sixteen disjoint 4 KB arrays
    err = lambda: (lib.gsmvi_last_error() or b"").decode()           # noqa: E731

    def hess(K=2, P=3, Cc=3, N=5, A=a(0), y=a(1), offset=a(2), counts=a(3), lam=1.0, lam_dev=None, kap=1.0, kap_dev=None, X=a(4),
             H=a(5), cov=a(6), info=a(7)):
        return lib.gsmvi_ordinal_hessian_batched_f64(None, None, K, P, Cc, N, A, y, offset, counts, lam, lam_dev, kap, kap_dev, X, H,
                                                     cov, info)

    def step_(K=2, P=3, Cc=3, N=5, A=a(0), y=a(1), offset=a(2), counts=a(3), lam=1.0, lam_dev=None, kap=1.0, kap_dev=None, start=0,
              x=a(4), g=a(5), d=a(6), sc=a(7), ist=a(8), Xt=a(9), stopped=a(10), maxiter=10, maxfun=20, gtol=1e-8):
        return lib.gsmvi_ordinal_laplace_step_batched_f64(None, None, K, P, Cc, N, A, y, offset, counts, lam, lam_dev, kap, kap_dev,
                                                          start, x, g, d, sc, ist, Xt, stopped, maxiter, maxfun, gtol)

    for call, name in ((hess, NAMES[0]), (step_, NAMES[1])):
        assert call(Cc=1) == 1 and "C must be" in err() and name in err()
        assert call(Cc=65) == 1 and "C must be" in err()
        assert call(P=0) == 1 and "P must be" in err()
        assert call(P=63) == 1 and "P must be" in err()                                     # D = 65
        big = dict(N=1, H=a(8), cov=None, info=None) if call is hess else dict(N=1)         # (H is 64 KB: beyond the other arrays)
        assert call(P=62, **big) == 1 and "ctx is NULL" in err()                            # D = 64
        assert call(P=1, Cc=64, **big) == 1 and "ctx is NULL" in err()
        assert call(K=0) == 1 and "K must be" in err()
        assert call(K=2 ** 26) == 1 and "K must be" in err()
        assert call(N=0) == 1 and "N must be" in err()
        assert call(K=2 ** 20, N=2 ** 40) == 1 and "too large" in err()
        assert call(lam=-1.0) == 1 and "prior_prec" in err()
        assert call(lam=float("inf")) == 1 and "prior_prec" in err()
        assert call(kap=-1.0) == 1 and "cut_prec" in err()
        assert call(kap=float("nan")) == 1 and "cut_prec" in err()
        assert call(kap=-1.0, A=None) == 1 and "cut_prec" in err()                          # priors before NULL arrays
        assert call(N=0, lam=-1.0) == 1 and "N must be" in err()                            # shape before priors
        for arr in ("A", "y"):
            assert call(**{arr: None}) == 1 and "NULL array" in err(), arr
        assert call() == 1 and "ctx is NULL" in err()
        assert call(kap=0.0, lam=0.0) == 1 and "ctx is NULL" in err()
        assert call(kap=-1.0, kap_dev=a(12), lam=-1.0, lam_dev=a(13)) == 1 and "ctx is NULL" in err()
        assert call(offset=None, counts=None) == 1 and "ctx is NULL" in err()
        assert call(y=a(0), offset=a(0), counts=a(0), lam_dev=a(0), kap_dev=a(0)) == 1 and "ctx is NULL" in err()   # read-only
    assert hess(X=None) == 1 and "NULL array" in err()
    assert hess(H=None, cov=None, info=None) == 1 and "H or cov" in err()
    assert hess(info=None) == 1 and "info_dev is required" in err()                         # cov without info_dev
    assert hess(cov=None) == 1 and "info_dev is required" in err()                          # and info_dev without cov
    assert hess(cov=None, info=None) == 1 and "ctx is NULL" in err()
    assert hess(H=None) == 1 and "ctx is NULL" in err()
    assert hess(X=None, H=a(0)) == 1 and "NULL array" in err()                              # NULL arrays before overlaps
    for w in ("H", "cov", "info"):
        for arr, where in (("A", a(0)), ("y", a(1)), ("offset", a(2)), ("counts_dev", a(3)), ("X", a(4))):
            assert hess(**{w: where}) == 1 and f"{w if w != 'info' else 'info_dev'} overlaps {arr}" in err(), (w, arr)
    assert hess(cov=a(5)) == 1 and "cov overlaps H" in err()
    assert hess(kap_dev=a(6)) == 1 and "cov overlaps cut_prec_dev" in err()
    assert hess(lam_dev=a(5)) == 1 and "H overlaps prior_prec_dev" in err()
    assert hess(H=a(4) + 8 * (2 * 5 - 1)) == 1 and "H overlaps X" in err()                  # the last element of X (K D = 10)
    assert hess(H=a(4) + 8 * 2 * 5) == 1 and "ctx is NULL" in err()                         # adjacent is not overlapping
    assert hess(H=a(1) + 4 * (2 * 5 - 1)) == 1 and "H overlaps y" in err()                  # y is K N ints
    assert hess(H=a(1) + 4 * 2 * 5) == 1 and "ctx is NULL" in err()
    for arr in ("x", "g", "d", "sc", "ist", "Xt"):
        assert step_(**{arr: None}) == 1 and "NULL array" in err(), arr
        assert step_(**{arr: a(0)}) == 1 and f"{arr} overlaps A" in err(), arr
        assert step_(**{arr: a(10)}) == 1 and "overlaps" in err() and "stopped_dev" in err(), arr
    assert step_(g=a(4)) == 1 and "g overlaps x" in err()
    assert step_(stopped=None) == 1 and "ctx is NULL" in err()
    assert step_(maxfun=1) == 1 and "maxfun at least 2" in err()
    assert step_(maxiter=0) == 1 and "maxiter must be at least 1" in err()
    assert step_(gtol=-1.0) == 1 and "gtol" in err()
    assert step_(gtol=float("nan")) == 1 and "gtol" in err()
    assert step_(start=1) == 1 and "ctx is NULL" in err()
