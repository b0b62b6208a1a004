"""Numpy restatements of the negative binomial Laplace initialiser (gsmvi_negbin_hessian_batched_f64,
gsmvi_negbin_laplace_step_batched_f64, csrc/gsmvi_negbin_laplace_batched.hip, the curvature of csrc/gsmvi_negbin_link.h) and a
stand-in engine for the host logic of ``laplace_init_negbin_batched`` and ``neg_hessian_negbin_batched``.  Test-only.  The model is
negbin_batched_ref's; at x = (beta, theta), r = e^theta, d = eta - theta, sigma = sigma(d):

    w_ee = (y + r) sigma sigma(-d),   w_et = -sigma r_eta,   w_tt = -[ r (dps - softplus(d)) + r^2 dtg + r sigma - sigma r_eta ]
    f = -lp,   g = -score,   H[:P, :P] = sum_n w_ee a a^T + lam I,   H[:P, P] = sum_n w_et a,   H[P, P] = sum_n w_tt + kap

``curv`` is the float64 restatement: the kernel's forms operation by operation (dtg = psi'(y + r) - psi'(r) as a shifted Stirling
difference, r^2 dtg as r (r [..]) with the term j = 0 kept apart).  ``curv_ld`` is the same model in np.longdouble with the
differences shifted to z >= 40, where the tails leave less than 1e-20: the reference of the GPU tests, by the same means as
negbin_batched_ref.link_ld.  ``evaluate`` forms f, g and H with the scale of every sum (the sum of the absolute values of its
terms); ``factor`` is the kernel's right-looking factorisation with the relative pivot rule and, with ``rule``, the last-pivot rule
of include/gsmvi_hip.h; ``step`` is the state machine of gsmvi_laplace_step_batched_f64 on these, ``run`` the whole iteration.
Pinned in tests/test_negbin_laplace_cpu.py."""
import functools

import numpy as np

import laplace_batched_ref as lref
import negbin_batched_ref as nref
from laplace_batched_ref import new_state, PIVOT_REL                        # noqa: F401
from negbin_batched_ref import make_inputs, R_MIN, SHIFT, SHIFT_BELOW       # noqa: F401

TG = (43867.0 / 798.0, -3617.0 / 510.0, 7.0 / 6.0, -691.0 / 2730.0, 5.0 / 66.0, -1.0 / 30.0, 1.0 / 42.0, -1.0 / 30.0, 1.0 / 6.0)
STEP_GTOL = lref.STEP_GTOL
STEP_K = 5
MOD_MARGIN = 1e-6                       # every replayed last-pivot decision: |s| >= MOD_MARGIN m (asserted on the CPU)
# (N, P) of the GPU tests: D = P + 1 in {2, 3, 16, 17, 32, 33, 48, 49, 64} (at 16 the border column is the last of an MFMA block,
# at 17 it is alone in one), N in {1, 31, 32, 33, 70} around one and two row tiles
SHAPES = ((33, 1), (70, 2), (31, 15), (70, 16), (32, 31), (70, 32), (33, 47), (70, 48), (70, 63))
SMALL_N = ((1, 9), (31, 9), (32, 9), (33, 9), (1, 20), (33, 20))
# the step test's sets: (N, P) -> make_problems seed for the trajectories from x0 = 0 (the rule fires) and from a start near the
# mode (it does not); tests/test_negbin_laplace_cpu.py asserts the margins of every entry
STEP_SHAPES = ((33, 1), (70, 2), (70, 9), (40, 15), (70, 16), (70, 32), (80, 63))
# ((N, P), with_offset) -> seed where the default 0 puts a decision on its threshold or leaves the set from x0 = 0 without a
# modified pivot
SEEDS = {((33, 1), False): 3, ((70, 2), False): 1, ((70, 9), False): 1, ((40, 15), True): 1, ((70, 16), True): 1,
         ((70, 32), True): 1, ((70, 32), False): 1}


def _tg_tail(z, L=np.float64):
    """T(z) = sum_{k=1..9} B_2k / z^(2k + 1), Horner in 1 / z^2 as the kernel"""
    x = L(1.0) / z
    w = x * x
    if L is np.float64:
        c = TG
    else:
        c = [L(43867) / 798, L(-3617) / 510, L(7) / 6, L(-691) / 2730, L(5) / 66, L(-1) / 30, L(1) / 42, L(-1) / 30, L(1) / 6]
    p = c[0]
    for a in c[1:]:
        p = p * w + a
    return (p * w) * x


def curv(eta, theta, y, r=None):
    """(r_eta, r_theta, t, w_ee, w_et, w_tt) in float64, the kernel's forms (nb_link_core<true, true, true>); eta, theta, y
    broadcast; r = exp(theta) unless given"""
    with np.errstate(all="ignore"):
        eta, theta, y = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (eta, theta, y)))
        r = np.exp(theta) if r is None else np.broadcast_to(np.asarray(r, dtype=np.float64), eta.shape)
        d = eta - theta
        e = np.exp(-np.abs(d))
        q, l1 = 1.0 + e, np.log1p(e)
        spd, spn = np.where(d > 0.0, d, 0.0) + l1, np.where(d < 0.0, -d, 0.0) + l1
        small = r < SHIFT_BELOW
        u = y / r
        sl = np.where(u < 1e300, np.log1p(u), np.log(y) - theta)
        sp = (y / (r + y)) / r
        ry = r + y
        tg0 = -((y / ry) * (1.0 + r / ry))
        st = np.zeros(eta.shape)
        for j in range(1, SHIFT):
            a = r + float(j)
            m = a * (a + y)
            qj = y / m
            sl = sl + np.log1p(y / a)
            sp = sp + qj
            st = st - qj * ((a + (a + y)) / m)
        sl, sp, st, tg0 = (np.where(small, v, 0.0) for v in (sl, sp, st, tg0))
        z = np.where(small, r + float(SHIFT), r)
        zy, lu = z + y, np.log1p(y / z)
        (s1, p1), (s0, p0) = nref._tails(zy), nref._tails(z)
        dlg = ((z - 0.5) * lu + y * (np.log(zy) - 1.0)) + (s1 - s0) - sl
        t = dlg - r * spd - y * spn
        sg, sn = np.where(d >= 0.0, 1.0 / q, e / q), np.where(d >= 0.0, e / q, 1.0 / q)
        dps = lu + y / (2.0 * z * zy) + (p1 - p0) + sp
        re = y * sn - r * sg
        rt = r * (dps - spd) - re
        x1 = -((y / zy) / z)
        x2 = x1 * ((0.5 * (z / zy + 1.0)) / z)
        dtz = ((x1 + x2) + (_tg_tail(zy) - _tg_tail(z))) + st
        r2dtg = r * (r * dtz) + tg0
        sre = sg * re
        wee = ((y + r) * sg) * sn
        wet = -sre
        wtt = -(((r * (dps - spd) + r2dtg) + r * sg) - sre)
    return re, rt, t, wee, wet, wtt


def curv_ld(eta, theta, y, zmin=40.0):
    """the same six in np.longdouble: the same model, the differences shifted until z >= zmin (tails below 1e-20), and the
    magnitudes a_ee, a_et, a_tt of the terms of the three weights as written (dps and dtg as primitives)"""
    L = np.longdouble
    with np.errstate(all="ignore"):
        eta, theta, y = np.broadcast_arrays(*(np.asarray(v, dtype=L) for v in (eta, theta, y)))
        re, rt, t = nref.link_ld(eta, theta, y, zmin)
        r = np.exp(theta)
        d = eta - theta
        e = np.exp(-np.abs(d))
        q, l1 = 1 + e, np.log1p(e)
        spd = np.where(d > 0, d, L(0)) + l1
        sg, sn = np.where(d >= 0, 1 / q, e / q), np.where(d >= 0, e / q, 1 / q)
        on = r < zmin
        ry = r + y
        tg0 = np.where(on, -((y / ry) * (1 + r / ry)), L(0))
        sp = np.where(on, (y / ry) / r, L(0))                            # (dps again, as link_ld forms it: rt + re would cancel)
        st = np.zeros(r.shape, dtype=L)
        for j in range(1, int(zmin)):
            a = r + j
            ay = a + y
            sp = sp + np.where(on, (y / ay) / a, L(0))
            st = st - np.where(on, ((y / ay) / a) * (1 / a + 1 / ay), L(0))
        z = np.where(on, r + int(zmin), r)
        zy = z + y
        dps = np.log1p(y / z) + y / (2 * z * zy) + (nref._tails(zy, L)[1] - nref._tails(z, L)[1]) + sp
        x1 = -((y / zy) / z)
        x2 = x1 * ((L(0.5) * (z / zy + 1)) / z)
        dtz = ((x1 + x2) + (_tg_tail(zy, L) - _tg_tail(z, L))) + st
        r2dtg = r * (r * dtz) + tg0
        rdp = r * (dps - spd)
        wee = (y + r) * sg * sn
        wet = -(sg * re)
        wtt = -(rdp + r2dtg + r * sg - sg * re)
        a_et = sg * (y * sn + r * sg)
        a_tt = r * np.abs(dps) + r * spd + np.abs(r2dtg) + r * sg + a_et
    return re, rt, t, wee, wet, wtt, (wee, a_et, a_tt)


def problem(A, y, offset, counts, lam, tm, tk, k):
    """problem k of a batch as the restatement takes it: its valid rows only"""
    K, N = np.shape(y)
    n = N if counts is None else int(min(max(int(counts[k]), 0), N))
    bc = lambda v: float(np.broadcast_to(np.asarray(v, dtype=np.float64), (K,))[k])          # noqa: E731
    return {"A": np.asarray(A[k, :n], dtype=np.float64), "y": np.asarray(y[k, :n], dtype=np.float64),
            "o": np.zeros(n) if offset is None else np.asarray(offset[k, :n], dtype=np.float64),
            "lam": bc(lam), "tm": bc(tm), "tk": bc(tk)}


def flagged(x):
    """the kernel's flag: a non-finite x, or an e^theta that is not a positive normal number"""
    with np.errstate(all="ignore"):
        r = np.exp(np.float64(x[-1]))
    return not np.isfinite(np.asarray(x, dtype=np.float64)).all() or not (r >= R_MIN and r < np.inf)


def evaluate(p, x, L=np.float64):
    """f = -lp, g = -score, H at x = (beta, theta) and the scales of the sums ({"f", "g", "H"}); a flagged x: f = NaN, g = H = NaN.
    L = np.longdouble: the high-precision restatement (results rounded to float64)."""
    A, yv, o = (np.asarray(p[k], dtype=L) for k in ("A", "y", "o"))
    lam, tm, tk = L(p["lam"]), L(p["tm"]), L(p["tk"])
    n, P = A.shape
    D = P + 1
    x = np.asarray(x, dtype=L)
    beta, theta = x[:P], x[P]
    with np.errstate(all="ignore"):
        eta = A @ beta + o
        if L is np.float64:
            re, rt, t, wee, wet, wtt = curv(eta, theta, yv)
            _, _, _, _, _, _, (a_ee, a_et, a_tt) = curv_ld(eta, theta, yv)
        else:
            re, rt, t, wee, wet, wtt, (a_ee, a_et, a_tt) = curv_ld(eta, theta, yv)
        dm = theta - tm
        f = -(t.sum() - L(0.5) * lam * (beta * beta).sum() - L(0.5) * tk * (dm * dm))
        g = np.empty(D, dtype=L)
        g[:P] = -(re @ A - lam * beta)
        g[P] = -(rt.sum() - tk * dm)
        H = np.empty((D, D), dtype=L)
        H[:P, :P] = (A * wee[:, None]).T @ A + lam * np.eye(P, dtype=L)
        H[:P, :P] = L(0.5) * (H[:P, :P] + H[:P, :P].T)
        H[:P, P] = H[P, :P] = wet @ A
        H[P, P] = wtt.sum() + tk
        aA = np.abs(A)
        sf = np.abs(t).sum() + L(0.5) * lam * (beta * beta).sum() + L(0.5) * tk * (dm * dm)
        sg = np.empty(D, dtype=L)
        sg[:P] = np.abs(re) @ aA + lam * np.abs(beta)
        sg[P] = np.abs(rt).sum() + tk * np.abs(dm)
        sH = np.empty((D, D), dtype=L)
        sH[:P, :P] = (aA * np.asarray(a_ee, dtype=L)[:, None]).T @ aA + lam * np.eye(P, dtype=L)
        sH[:P, P] = sH[P, :P] = np.asarray(a_et, dtype=L) @ aA
        sH[P, P] = np.asarray(a_tt, dtype=L).sum() + tk
    f, g, H = float(f), g.astype(np.float64), H.astype(np.float64)
    if flagged(x.astype(np.float64)):
        f, g, H = np.nan, np.full(D, np.nan), np.full((D, D), np.nan)
    return f, g, H, {"f": float(sf), "g": sg.astype(np.float64), "H": sH.astype(np.float64)}


def neg_hessian(A, y, offset, counts, lam, tm, tk, X, L=np.float64):
    """(K, D, D) at the rows of X (K, D), and the scales (K, D, D)"""
    X = np.asarray(X, dtype=np.float64)
    out = [evaluate(problem(A, y, offset, counts, lam, tm, tk, k), X[k], L) for k in range(X.shape[0])]
    return np.stack([o[2] for o in out]), np.stack([o[3]["H"] for o in out])


def factor(H, rule=False):
    """the kernel's right-looking factorisation H = R^T R with the pivot rule 64 eps H_jj: (info, R, notes).  info: 0, or 1 + the
    first failing pivot.  With ``rule``, when exactly the last pivot fails: s = H[P, P] - sum_c R[c, P]^2 and m = |H[P, P]| +
    sum_c R[c, P]^2 in c order; |s| finite and > 64 eps m: R[P, P] = sqrt|s|, info = 0, notes["mod"] = True; notes["margin"] =
    |s| / m whenever the last pivot failed."""
    S = np.array(H, dtype=np.float64)
    D = S.shape[0]
    dg = np.diag(S).copy()
    pv = np.zeros(D)
    info = 0
    notes = {"mod": False}
    with np.errstate(all="ignore"):
        for c in range(D):
            a = S[c, c]
            if info == 0 and not (a > PIVOT_REL * dg[c] and a < np.inf):
                info = c + 1
            pv[c] = np.sqrt(a)
            v = S[c, c + 1:] * (1.0 / pv[c])
            S[c + 1:, c + 1:] -= np.outer(v, v)
        R = np.zeros((D, D))
        for i in range(D):
            R[i, i + 1:] = S[i, i + 1:] / pv[i]
            R[i, i] = pv[i]
        if info == D:
            s2, s = 0.0, dg[D - 1]
            for c in range(D - 1):
                s2 += R[c, D - 1] * R[c, D - 1]
            for c in range(D - 1):
                s -= R[c, D - 1] * R[c, D - 1]
            m = abs(dg[D - 1]) + s2
            notes["margin"] = abs(s) / m if m > 0 and np.isfinite(s) else 0.0
            if rule and abs(s) < np.inf and abs(s) > PIVOT_REL * m:
                R[D - 1, D - 1] = np.sqrt(abs(s))
                info, notes["mod"] = 0, True
    return info, R, notes


def inverse(H):
    """(cov, info) of gsmvi_negbin_hessian_batched_f64: never modified; the identity where the factorisation fails"""
    info = factor(H)[0] if np.isfinite(H).all() else 1
    return (np.linalg.inv(H) if info == 0 else np.eye(H.shape[0])), info


def _direction(s, g, H, sc, notes, rule):
    """factor H (with the last-pivot rule when ``rule``); d = -(R^T R)^{-1} g, t = 1, g.d, Xt = x + d, or status 5"""
    info, R, fn = factor(H, rule)
    notes["info"], notes["mod"] = info, fn["mod"]
    if "margin" in fn:
        notes["margin"] = fn["margin"]
    if info != 0:
        s["status"] = 5
        return
    Hm = R.T @ R if fn["mod"] else H
    Hi = np.linalg.inv(Hm)
    z = np.linalg.solve(R.T, g)
    d = -np.linalg.solve(R, z)
    s["d"], s["t"], s["gd"], s["nls"] = d, 1.0, float(g @ d), 0
    s["Xt"] = s["x"] + d
    s["nmod"] = s.get("nmod", 0) + int(fn["mod"])
    sd = np.abs(Hi).sum(1).max() * sc["g"].max() + np.abs(d).max()
    notes["scale_d"] = sd
    notes["scale_gd"] = float(np.abs(g) @ np.abs(d) + sc["g"] @ np.abs(d) + np.abs(g).sum() * sd)
    notes["pivot"] = float(np.min(np.diag(R) ** 2 / (PIVOT_REL * np.abs(np.diag(H)))))


def step(p, before, start, maxiter=100, maxfun=200, gtol=1e-8, rule=True, L=np.float64):
    """one launch for one problem: (state after, notes), laplace_batched_ref.step on this module's ``evaluate`` and ``factor``; the
    state carries ``nmod`` (ist[4]); notes: ``mod``, ``margin`` of a last-pivot decision, ``pivot``, and lref.step's"""
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


# ---- the named test sets of the convergence tests (the issue's five settings; 64 problems each) ----------------------------------
SETS = {"r2": (64, 9, 2.0), "r50": (64, 9, 50.0), "r0.3": (256, 15, 0.3), "p1": (33, 1, 5.0), "poisson": (64, 9, None)}
SET_K = 64
# what tests/test_negbin_laplace_cpu.py found and asserts on these sets at the defaults (kap = 1): plain Newton (rule off) ends
# this many problems with status 5; with the rule every problem converges within these many iterations and evaluations
SET_PLAIN_STATUS5_MIN = 1
SET_MAX_NIT, SET_MAX_NFEV = 11, 23


def make_problems(N, P, size, K=SET_K, seed=0, kap=1.0, lam=1.0):
    """K well-posed problems: A = N(0, 1) / sqrt(P), beta* ~ 0.7 N(0, 1), intercept offsets 1 + 0.3 N(0, 1), y negative binomial
    at mu = exp(A beta* + o) with size ``size`` (None: Poisson data), priors lam, kap, m = 0.  Returns A, y, offset, None, lam, 0.0, kap."""
    rs = np.random.RandomState(1000 * N + 10 * P + seed)
    A = rs.standard_normal((K, N, P)) / np.sqrt(P)
    beta = 0.7 * rs.standard_normal((K, P))
    offset = 1.0 + 0.3 * rs.standard_normal((K, N))
    mu = np.exp(np.einsum("knp,kp->kn", A, beta) + offset)
    y = rs.poisson(mu if size is None else rs.gamma(size, mu / size)).astype(np.float64)
    return A, y, offset, None, lam, 0.0, kap


@functools.lru_cache(maxsize=None)
def set_runs(name, rule, kap=1.0):
    """the final states of the SET_K problems of SETS[name] from x0 = 0 at the defaults; computed once and shared"""
    N, P, size = SETS[name]
    inp = make_problems(N, P, size, kap=kap)
    return [run(problem(*inp, k), np.zeros(P + 1), rule=rule) for k in range(SET_K)]


# ---- the step test's trajectories ------------------------------------------------------------------------------------------------
def step_inputs(shape, with_offset=True, seed=None):
    """the STEP_K problems of the step test at (N, P) = ``shape`` (make_problems at size 3 with the seed of SEEDS)"""
    N, P = shape
    inp = list(make_problems(N, P, 3.0, K=STEP_K, seed=SEEDS.get((shape, with_offset), 0) if seed is None else seed))
    if not with_offset:
        inp[2] = None
    return tuple(inp)


@functools.lru_cache(maxsize=None)
def trajectories(shape, near, with_offset=True, seed=None):
    """the step test's runs at (N, P) = ``shape``: the STEP_K problems of ``step_inputs`` at gtol = STEP_GTOL from x0 = 0 (the
    last-pivot rule fires on some) or, with ``near``, from the mode of a first run plus 0.05 (it does not), as [(problem index,
    final state, [(before, after, notes), ...]), ...]; computed once and shared (do not modify)"""
    inp = step_inputs(shape, with_offset, seed)
    out = []
    for k in range(STEP_K):
        p = problem(*inp, k)
        x0 = np.zeros(shape[1] + 1)
        if near:
            x0 = run(p, x0)["x"] + 0.05
        s, rec = run(p, x0, record=True, gtol=STEP_GTOL, maxiter=30, maxfun=60)
        out.append((k, s, rec, x0))
    return out


def margins_hold(traj):
    """every run converged, no max|g| within a factor 1.5 of gtol, every Armijo decision by at least 1e-11 max(1, |f|), every
    pivot that passed at least 1e3 times its threshold, and every last-pivot decision with |s| >= MOD_MARGIN m.  Returns (ok,
    smallest Armijo margin, smallest pivot ratio, smallest |s| / m, rounds with a modified pivot)."""
    ok, low, piv, mar, nmod = True, 1.0, np.inf, np.inf, 0
    for _, st, rec, _ in traj:
        ok = ok and st["status"] == 1
        for _, _, notes in rec:
            if "gmax" in notes:
                ok = ok and not STEP_GTOL / 1.5 <= notes["gmax"] <= 1.5 * STEP_GTOL
            if "armijo" in notes:
                low = min(low, notes["armijo"])
            if "pivot" in notes:
                piv = min(piv, notes["pivot"])
            if "margin" in notes:
                mar = min(mar, notes["margin"])
            nmod += int(notes.get("mod", False))
            ok = ok and notes.get("info", 0) == 0
    return bool(ok and low >= 1e-11 and piv >= 1e3 and mar >= MOD_MARGIN), low, piv, mar, nmod


class StandInEngine(nref.RestatementEngine, lref.StandInEngine):
    """the engine calls of ``laplace_init_negbin_batched`` and ``neg_hessian_negbin_batched`` on numpy and the restatement (the
    state, ``read_flag`` and ``read_ints`` are laplace_batched_ref.StandInEngine's); ``rule``: the last-pivot rule on or off"""
    name = "restatement-negbin-laplace(test-only)"

    def __init__(self, rule=True):
        super().__init__()
        self.rule = rule

    def negbin_hessian_batched(self, X, A, y, offset=None, counts=None, prior_prec=1.0, log_size_mean=0.0, log_size_prec=1.0,
                               want="h", out=None, cov_out=None, info_out=None):
        self.calls.append(("negbin_hessian", want))
        assert A.dtype == np.float64 and y.dtype == np.float64 and X.shape[1] == A.shape[2] + 1
        H = neg_hessian(A, y, offset, counts, prior_prec, log_size_mean, log_size_prec, X)[0]
        if want == "h":
            return H
        ci = [inverse(h) for h in H]
        cov, info = np.stack([c for c, _ in ci]), np.array([i for _, i in ci], dtype=np.int32)
        return (cov, info) if want == "cov" else (H, cov, info)

    def negbin_laplace_step_batched(self, state, A, y, offset=None, counts=None, prior_prec=1.0, log_size_mean=0.0,
                                    log_size_prec=1.0, start=False, maxiter=100, maxfun=200, gtol=1e-8):
        self.calls.append(("negbin_laplace_step", bool(start)))
        for k in range(y.shape[0]):
            p = problem(A, y, offset, counts, prior_prec, log_size_mean, log_size_prec, k)
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


NAMES = ("gsmvi_negbin_hessian_batched_f64", "gsmvi_negbin_laplace_step_batched_f64")


def check_bad_arguments(lib):
    """both entry points through the C ABI with a NULL context, in the pattern of laplace_batched_ref.check_bad_arguments: every
    bad argument returns GSMVI_ERR_BAD_ARG (1) with its own message, so nothing can have been enqueued; valid calls end at the
    context"""
    import ctypes as C
    buf = (C.c_double * 8192)()
    p = C.cast(buf, C.c_void_p).value
    a = lambda n: p + 8 * 512 * n                                   # noqa: E731  sixteen disjoint 4 KB arrays
    err = lambda: (lib.gsmvi_last_error() or b"").decode()           # noqa: E731

    def hess(K=2, P=3, N=5, A=a(0), y=a(1), offset=a(2), counts=a(3), tm=0.0, tm_dev=None, tk=1.0, tk_dev=None, lam=1.0,
             lam_dev=None, X=a(4), H=a(5), cov=a(6), info=a(7)):
        return lib.gsmvi_negbin_hessian_batched_f64(None, None, K, P, N, A, y, offset, counts, tm, tm_dev, tk, tk_dev, lam, lam_dev,
                                                    X, H, cov, info)

    def step_(K=2, P=3, N=5, A=a(0), y=a(1), offset=a(2), counts=a(3), tm=0.0, tm_dev=None, tk=1.0, tk_dev=None, lam=1.0,
              lam_dev=None, start=0, x=a(4), g=a(5), d=a(6), sc=a(7), ist=a(8), Xt=a(9), stopped=a(10), maxiter=10, maxfun=20,
              gtol=1e-8):
        return lib.gsmvi_negbin_laplace_step_batched_f64(None, None, K, P, N, A, y, offset, counts, tm, tm_dev, tk, tk_dev, lam,
                                                         lam_dev, start, x, g, d, sc, ist, Xt, stopped, maxiter, maxfun, gtol)

    for call, name in ((hess, NAMES[0]), (step_, NAMES[1])):
        assert call(P=0) == 1 and "P must be" in err() and name in err()
        assert call(P=64) == 1 and "P must be" in err()
        assert call(K=0) == 1 and "K must be" in err()
        assert call(K=2 ** 26) == 1 and "K must be" in err()
        assert call(N=0) == 1 and "N must be" in err()
        assert call(K=2 ** 20, N=2 ** 40) == 1 and "too large" in err()
        for arr in ("A", "y"):
            assert call(**{arr: None}) == 1 and "NULL array" in err(), arr
        assert call(lam=-1.0) == 1 and "prior_prec" in err()
        assert call(lam=float("inf")) == 1 and "prior_prec" in err()
        assert call(tk=-1.0) == 1 and "theta_prec" in err()
        assert call(tk=float("nan")) == 1 and "theta_prec" in err()
        assert call(tm=float("inf")) == 1 and "theta_mean" in err()
        assert call() == 1 and "ctx is NULL" in err()
        assert call(tk=0.0, lam=0.0) == 1 and "ctx is NULL" in err()
        assert call(tm=float("nan"), tm_dev=a(11), tk=-1.0, tk_dev=a(12), lam=-1.0, lam_dev=a(13)) == 1 and "ctx is NULL" in err()
        assert call(offset=None, counts=None) == 1 and "ctx is NULL" in err()
        assert call(y=a(0), offset=a(0), counts=a(0), tm_dev=a(0), tk_dev=a(0)) == 1 and "ctx is NULL" in err()   # read-only
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
    assert hess(tm_dev=a(5)) == 1 and "H overlaps theta_mean_dev" in err()
    assert hess(tk_dev=a(6)) == 1 and "cov overlaps theta_prec_dev" in err()
    assert hess(lam_dev=a(5)) == 1 and "H overlaps prior_prec_dev" in err()
    assert hess(H=a(4) + 8 * (2 * 4 - 1)) == 1 and "H overlaps X" in err()                  # the last element of X (K D = 8)
    assert hess(H=a(4) + 8 * 2 * 4) == 1 and "ctx is NULL" in err()                         # adjacent is not overlapping
    assert hess(H=a(0) + 8 * (2 * 5 * 3 - 1)) == 1 and "H overlaps A" in err()              # A is K N P doubles
    assert hess(H=a(0) + 8 * 2 * 5 * 3) == 1 and "ctx is NULL" in err()
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
