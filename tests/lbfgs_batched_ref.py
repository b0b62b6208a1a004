"""Numpy restatement of the batched L-BFGS initialiser (csrc/gsmvi_lbfgs_batched.hip), one problem at a time, and the inputs of
its tests.  Test-only.  phi = -lp is minimised by plain L-BFGS (history 10) with an Armijo backtracking search:

    start(x0, f, g)      the state after the first evaluation
    step(state, ft, gt)  the state after the evaluation at the trial point state["xt"]
    hess_inv(state)      the dense BFGS inverse-Hessian product of the held pairs on an identity base
    run(fun, x0)         the driver: fun(x) -> (phi, grad phi)

A state is a dict: x, f, g, d, t, gd, nls, the ring buffers S, Y (10, D) with sy, yy (10), npairs, head (the held pairs are the
slots head - npairs .. head - 1 mod 10, oldest first), nit, nfev, status (0 running, 1 converged, 2 maxiter / maxfun, 3 line
search failed, 4 non-finite start), the trial point xt, and the options.  ``visits`` counts the branches taken and ``margins``
records how far the two decisions that depend on a dot product were from their thresholds, relative to the sum of the absolute
products (what the rounding of such a sum scales with); both are bookkeeping of the tests, not part of the algorithm."""
import collections
import copy

import numpy as np

M = 10
FTOL = 2.220446049250313e-09
NSC, NIS = 24, 8          # the device layout: doubles per problem in sc, ints per problem in ist


def _steepest(st):
    g = st["g"]
    st["d"] = -g
    st["t"] = min(1.0, 1.0 / np.sqrt(np.dot(g, g)))
    st["gd"] = float(np.dot(g, st["d"]))
    st["nls"] = 0
    st["xt"] = st["x"] + st["t"] * st["d"]


def _count_stop(st):
    if st["status"] != 0:
        st["visits"]["status%d" % st["status"]] += 1


def start(x0, f, g, gtol=1e-5, ftol=FTOL, maxiter=1000, maxfun=1000):
    x0, g = np.array(x0, dtype=np.float64), np.array(g, dtype=np.float64)
    D = x0.shape[0]
    st = dict(x=x0.copy(), f=float(f), g=g.copy(), d=np.zeros(D), t=0.0, gd=0.0, nls=0, S=np.zeros((M, D)), Y=np.zeros((M, D)),
              sy=np.zeros(M), yy=np.zeros(M), npairs=0, head=0, nit=0, nfev=1, status=0, xt=x0.copy(),
              opt=dict(gtol=gtol, ftol=ftol, maxiter=maxiter, maxfun=maxfun), visits=collections.Counter(), margins=[])
    if not (np.isfinite(f) and np.isfinite(g).all()):
        st["status"] = 4
    elif np.abs(g).max() <= gtol:
        st["status"] = 1
    else:
        _steepest(st)
    _count_stop(st)
    return st


def held(st):
    """ring-buffer slots of the held pairs, oldest first"""
    return [(st["head"] - st["npairs"] + p) % M for p in range(st["npairs"])]


def step(st, ft, gt):
    """the state after (ft, gt) at st["xt"]; a stopped state comes back unchanged (a copy)"""
    st = copy.deepcopy(st)
    if st["status"] != 0:
        return st
    o, v = st["opt"], st["visits"]
    ft, gt = float(ft), np.array(gt, dtype=np.float64)
    st["nfev"] += 1
    ok = bool(np.isfinite(ft) and np.isfinite(gt).all() and ft <= st["f"] + (1e-4 * st["t"]) * st["gd"])
    if not ok:
        v["rejected"] += 1
        st["t"] = 0.5 * st["t"]
        st["nls"] += 1
        if st["nls"] > 20:
            st["status"] = 3
        elif st["nfev"] >= o["maxfun"]:
            st["status"] = 2
            v["maxfun"] += 1
        else:
            st["xt"] = st["x"] + st["t"] * st["d"]
        _count_stop(st)
        return st
    v["accepted"] += 1
    v["accepted_unit"] += st["t"] == 1.0
    s, y = st["xt"] - st["x"], gt - st["g"]
    fprev = st["f"]
    st["x"], st["f"], st["g"] = st["xt"].copy(), ft, gt
    st["nit"] += 1
    sy, yy = float(np.dot(s, y)), float(np.dot(y, y))
    st["margins"].append(("pair", sy, 2.2e-16 * yy, float(np.abs(s * y).sum())))
    if sy > 2.2e-16 * yy:
        h = st["head"]
        v["stored"] += 1
        v["wrapped"] += st["npairs"] == M
        st["S"][h], st["Y"][h], st["sy"][h], st["yy"][h] = s, y, sy, yy
        st["head"] = (h + 1) % M
        st["npairs"] = min(st["npairs"] + 1, M)
    else:
        v["skipped"] += 1
    if np.abs(gt).max() <= o["gtol"] or (fprev - ft) <= o["ftol"] * max(abs(fprev), abs(ft), 1.0):
        st["status"] = 1
    elif st["nit"] >= o["maxiter"] or st["nfev"] >= o["maxfun"]:
        st["status"] = 2
        v["maxiter" if st["nit"] >= o["maxiter"] else "maxfun"] += 1
    elif st["npairs"] == 0:
        _steepest(st)
    else:
        idx = held(st)[::-1]                         # newest to oldest
        q, al = gt.copy(), []
        for i in idx:
            a = (1.0 / st["sy"][i]) * np.dot(st["S"][i], q)
            al.append(a)
            q = q - a * st["Y"][i]
        r = (st["sy"][idx[0]] / st["yy"][idx[0]]) * q
        for i, a in zip(idx[::-1], al[::-1]):        # oldest to newest
            b = (1.0 / st["sy"][i]) * np.dot(st["Y"][i], r)
            r = r + st["S"][i] * (a - b)
        st["d"], st["t"], st["nls"] = -r, 1.0, 0
        st["gd"] = float(np.dot(gt, st["d"]))
        st["margins"].append(("descent", st["gd"], 0.0, float(np.abs(gt * st["d"]).sum())))
        if not st["gd"] < 0.0:
            v["not_descent"] += 1
            st["npairs"], st["head"] = 0, 0
            _steepest(st)
        else:
            st["xt"] = st["x"] + st["t"] * st["d"]
    _count_stop(st)
    return st


def hess_inv(st):
    D = st["x"].shape[0]
    H, I = np.eye(D), np.eye(D)
    for i in held(st):
        s, y = st["S"][i], st["Y"][i]
        rho = 1.0 / np.dot(s, y)
        H = (I - rho * np.outer(s, y)) @ H @ (I - rho * np.outer(y, s)) + rho * np.outer(s, s)
    return H


def run(fun, x0, record=False, **opt):
    """the driver: returns the final state, and with ``record`` the list of (state before, ft, gt, state after) of every step
    (the first entry's state before is None: the start)"""
    x0 = np.array(x0, dtype=np.float64)
    f, g = fun(x0)
    st = start(x0, f, g, **opt)
    rec = [(None, f, np.array(g, dtype=np.float64), st)]
    while st["status"] == 0:
        ft, gt = fun(st["xt"])
        new = step(st, ft, gt)
        rec.append((st, ft, np.array(gt, dtype=np.float64), new))
        st = new
    return (st, rec) if record else st


# ---- the device layout ----------------------------------------------------------------------------------------------------
def pack(states):
    """the states of K problems of one D as the arrays the engine takes: x, g, d, Xt (K, D), S, Y (K, 10, D), sc (K, 24), ist
    (K, 8) int32"""
    K, D = len(states), states[0]["x"].shape[0]
    out = dict(x=np.zeros((K, D)), g=np.zeros((K, D)), d=np.zeros((K, D)), Xt=np.zeros((K, D)), S=np.zeros((K, M, D)),
               Y=np.zeros((K, M, D)), sc=np.zeros((K, NSC)), ist=np.zeros((K, NIS), dtype=np.int32))
    for k, st in enumerate(states):
        out["x"][k], out["g"][k], out["d"][k], out["Xt"][k], out["S"][k], out["Y"][k] = st["x"], st["g"], st["d"], st["xt"], st["S"], st["Y"]
        out["sc"][k, :3] = st["f"], st["t"], st["gd"]
        out["sc"][k, 4:14], out["sc"][k, 14:24] = st["sy"], st["yy"]
        out["ist"][k, :6] = st["status"], st["nit"], st["nfev"], st["nls"], st["npairs"], st["head"]
    return out


# ---- the inputs of the tests ------------------------------------------------------------------------------------------------
LOGISTIC_SHAPES = [(200, 5), (200, 10), (257, 33), (1000, 64), (64, 64), (7, 16)]
GPU_DS = [1, 2, 5, 10, 16, 17, 33, 64]


def logistic_fun(A, y, count, lam):
    """phi = -lp and its gradient of one logistic problem (tests/logistic_batched_ref.py)"""
    import logistic_batched_ref as lref

    def fun(x):
        G, lp = lref.score_and_lp(A[None], y[None], np.array([count]), np.array([lam]), x[None, None, :])
        return -float(lp[0, 0]), -G[0, 0]
    return fun


def gaussian_fun(D, seed=0):
    """the reference example's target (examples/example_initializers.py:29-36): mean ~ U(0, 1), cov = L L^T + 1e-3 I"""
    rs = np.random.RandomState(1000 + 7 * D + seed)
    mean = rs.random_sample(D)
    L = rs.standard_normal((D, D))
    P = np.linalg.inv(L @ L.T + 1e-3 * np.eye(D))
    P = 0.5 * (P + P.T)

    def fun(x):
        r = x - mean
        return 0.5 * float(r @ P @ r), P @ r
    fun.mean, fun.P = mean, P
    return fun


def huber_fun(D):
    """sum_i h(x_i), h = x^2 / 2 inside |x| <= 1 and |x| - 1 / 2 outside: the gradient is constant on the linear piece, so steps
    that stay on it give y = 0 exactly (a skipped pair)"""
    def fun(x):
        inside = np.abs(x) <= 1.0
        return float(np.where(inside, 0.5 * x * x, np.abs(x) - 0.5).sum()), np.where(inside, x, np.sign(x))
    return fun


def wall_fun(x0):
    """finite at x0 alone (lp = -inf off the start point): every trial is rejected"""
    x0 = np.array(x0, dtype=np.float64)

    def fun(x):
        if np.array_equal(x, x0):
            return 1.0, np.ones_like(x0)
        return np.inf, np.zeros_like(x0)
    return fun


def gpu_cases(D):
    """(name, fun, x0, options) of the trajectories the GPU step test walks at dimension D"""
    import logistic_batched_ref as lref
    N = {1: 9, 2: 12, 5: 200, 10: 200, 16: 7, 17: 40, 33: 257, 64: 64}[D]
    A, y, counts, lam, _ = lref.make_inputs(3, N, D, 1)
    g = gaussian_fun(D)
    cases = [("logistic%d" % k, logistic_fun(A[k], y[k], counts[k], lam[k]), np.zeros(D), {}) for k in (1, 2)]
    cases += [("logistic_ftol0", logistic_fun(A[1], y[1], counts[1], lam[1]), np.zeros(D), dict(ftol=0.0)),
              ("gaussian", g, np.ones(D), dict(maxfun=60)),
              ("gaussian_maxfun", g, np.ones(D), dict(maxfun=4)),
              ("gaussian_maxiter", g, np.ones(D), dict(maxiter=2)),
              ("gaussian_at_optimum", g, g.mean.copy(), {}),
              ("huber", huber_fun(D), np.full(D, 6.5), {}),
              ("huber_maxiter", huber_fun(D), np.full(D, 40.0), dict(maxiter=3)),
              ("far_logistic", logistic_fun(A[1], 1.0 - y[1], counts[1], lam[1]), np.full(D, 30.0), dict(maxfun=40)),
              ("wall", wall_fun(np.ones(D)), np.ones(D), {}),
              ("nan_start", lambda x: (np.nan, np.zeros(D)), np.ones(D), {}),
              ("nan_gradient_start", lambda x: (1.0, np.full(D, np.nan)), np.ones(D), {})]
    return cases
