"""Numpy restatement of the batched Pathfinder initialiser (gsmvi_pathfinder_propose_batched_f64 and
gsmvi_pathfinder_select_batched_f64, csrc/gsmvi_pathfinder_batched.hip), in np.longdouble (``dtype=np.float64`` is the switch
that measures the float64 noise floor of the same arithmetic, and what the stand-in engine runs).  Test-only.  Written from the
definition in include/gsmvi_hip.h on the device layout of the L-BFGS state (tests/lbfgs_batched_ref.py: ``pack``):

    base(sc, ist, h0)               gamma: h0 if h0 > 0, else s.y / y.y of the newest held pair, 1 without a pair
    sigma(S, Y, sc, ist, h0)        H after H_0 = gamma I and the BFGS recursion over the held pairs, oldest to newest
    propose(state, seen, normals, M, h0)   one launch for K problems: fresh, seen, mu, cov, X, logq, info
    select(lpsum, prop, nit, best, M)      one launch: elbo_last, npts and the best state

The normals are handed in (``normals(k, nit)`` -> (M, D) float64): the rows of the engine's ``normal`` stream on the GPU, the
oracle's Philox on the CPU.  ``select`` is copies and one subtract-divide in float64, as the kernel.  The stand-in engine at the
end serves the host-logic tests of ``pathfinder_init_batched``; it steps the L-BFGS states with tests/lbfgs_batched_ref.py."""
import collections

import numpy as np

import glm_batched_ref as gref
import lbfgs_batched_ref as lref
import softmax_batched_ref as sref
from engines import OracleBatchedEngine
from oracle import gsm_oracle as orc
from psis_batched_ref import chol_upper

LD = np.longdouble
HIST = lref.M
MAX_DRAWS = 4096
PATH_BIT = 0x4000000


def held(ist):
    """ring-buffer slots of the held pairs, oldest first, from the clamped words ist[4] (pairs held) and ist[5] (next slot)"""
    n, head = min(max(int(ist[4]), 0), HIST), int(ist[5]) % HIST
    return [(head - n + p) % HIST for p in range(n)]


def base(sc, ist, h0=0.0):
    if h0 > 0.0:
        return float(h0)
    idx = held(ist)
    if not idx:
        return 1.0
    with np.errstate(all="ignore"):
        return float(np.float64(sc[4 + idx[-1]]) / np.float64(sc[14 + idx[-1]]))


def sigma(S, Y, sc, ist, h0=0.0, dtype=LD):
    """(D, D): H <- H - rho (s u^T + u s^T) + (rho^2 y.u + rho) s s^T with u = H y, rho = 1 / s.y: the expanded form of
    (I - rho s y^T) H (I - rho y s^T) + rho s s^T, symmetric by construction"""
    D = S.shape[1]
    H = dtype(base(sc, ist, h0)) * np.eye(D, dtype=dtype)
    with np.errstate(all="ignore"):
        for i in held(ist):
            s, y = S[i].astype(dtype), Y[i].astype(dtype)
            rho = dtype(1) / np.dot(s, y)
            u = H @ y
            H = (H - rho * (np.outer(s, u) + np.outer(u, s))) + (rho * rho * np.dot(y, u) + rho) * np.outer(s, s)
    return H


def log_2pi(dtype):
    return np.log(dtype(8) * np.arctan(dtype(1)))


def propose(state, seen, normals, M, h0=0.0, dtype=LD):
    """state: the arrays x, g (K, D), S, Y (K, 10, D), sc (K, 24), ist (K, 8); seen (K) ints.  Returns a dict: fresh, seen, info
    (K) int64, logq (K), X (K, M, D), and mu (K, D), cov (K, D, D) whose rows of the problems that are not fresh are NaN
    markers (the launch leaves those untouched: the caller keeps what it had)."""
    K, D = state["x"].shape
    out = dict(fresh=np.zeros(K, dtype=np.int64), seen=np.array(seen, dtype=np.int64), info=np.zeros(K, dtype=np.int64),
               logq=np.full(K, np.nan, dtype=dtype), X=np.empty((K, M, D), dtype=dtype), mu=np.full((K, D), np.nan, dtype=dtype),
               cov=np.full((K, D, D), np.nan, dtype=dtype))
    for k in range(K):
        ist = state["ist"][k]
        nit = int(ist[1])
        if nit == int(seen[k]):
            out["X"][k] = state["x"][k][None, :]
            continue
        out["fresh"][k], out["seen"][k] = 1, nit
        H = sigma(state["S"][k], state["Y"][k], state["sc"][k], ist, h0, dtype)
        with np.errstate(all="ignore"):
            mu = state["x"][k].astype(dtype) - H @ state["g"][k].astype(dtype)
        out["mu"][k], out["cov"][k] = mu, H
        R, info = chol_upper_of(H, dtype)
        out["info"][k] = info
        if info or not np.isfinite(mu.astype(np.float64)).all():
            out["X"][k] = np.nan
            continue
        Z = np.asarray(normals(k, nit), dtype=np.float64).reshape(M, D).astype(dtype)
        out["X"][k] = mu[None, :] + Z @ R
        out["logq"][k] = -(Z * Z).sum() / dtype(2) - dtype(M) * (np.log(np.diag(R)).sum() + dtype(D) / dtype(2) * log_2pi(dtype))
    return out


def chol_upper_of(H, dtype):
    """psis_batched_ref.chol_upper on a matrix that is already in ``dtype`` (that function rounds its input to float64 first)"""
    if dtype is np.float64:
        return chol_upper(H, dtype)
    A = np.array(H, dtype=dtype)
    D = A.shape[0]
    R = np.zeros((D, D), dtype=dtype)
    with np.errstate(all="ignore"):
        for c in range(D):
            if not (A[c, c] > 0 and np.isfinite(A[c, c])):
                return None, c + 1
            R[c, c] = np.sqrt(A[c, c])
            R[c, c + 1:] = A[c, c + 1:] / R[c, c]
            for i in range(c + 1, D):
                A[i, i:] -= R[c, i] * R[c, i:]
    return R, 0


def new_best(x0):
    """the best state as ``pathfinder_state_batched`` starts it"""
    x0 = np.array(x0, dtype=np.float64)
    K, D = x0.shape
    return dict(best_elbo=np.full(K, -np.inf), best_mean=x0.copy(), best_cov=np.broadcast_to(np.eye(D), (K, D, D)).copy(),
                best_it=np.full(K, -1, dtype=np.int64), npts=np.zeros(K, dtype=np.int64), elbo_last=np.full(K, np.nan))


def select(lpsum, logq, fresh, info, nit, mu, cov, best, M):
    """the state after one select launch (a copy): float64 throughout, as the kernel"""
    out = {k: np.array(v, copy=True) for k, v in best.items()}
    lpsum, logq = np.asarray(lpsum, dtype=np.float64), np.asarray(logq, dtype=np.float64)
    for k in range(lpsum.shape[0]):
        e = np.float64(np.nan)
        if fresh[k] and info[k] == 0:
            with np.errstate(all="ignore"):
                e = (lpsum[k] - logq[k]) / np.float64(M)
        out["elbo_last"][k] = e
        out["npts"][k] += 1 if fresh[k] else 0
        if fresh[k] and np.isfinite(e) and e > out["best_elbo"][k]:
            out["best_elbo"][k], out["best_it"][k] = e, nit[k]
            out["best_mean"][k], out["best_cov"][k] = mu[k], cov[k]
    return out


def rel_gap(a, b):
    """max |a - b| / max(1, max |b|) over the finite entries of b, after the non-finite ones are checked to sit in the same places"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    fa, fb = np.isfinite(a.astype(np.float64)), np.isfinite(b.astype(np.float64))
    assert np.array_equal(fa, fb), "non-finite entries in different places"
    if not fb.any():
        return 0.0
    return float(np.abs(a[fb] - b[fb]).max() / max(LD(1), np.abs(b[fb]).max()))


def rel_err(a, b):
    """the same relative to max |b| alone (conftest.rel_err in longdouble): the metric of the matrices and vectors"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    fa, fb = np.isfinite(a.astype(np.float64)), np.isfinite(b.astype(np.float64))
    assert np.array_equal(fa, fb), "non-finite entries in different places"
    if not fb.any():
        return 0.0
    return float(np.abs(a[fb] - b[fb]).max() / max(np.abs(b[fb]).max(), LD(1e-300)))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
GPU_DS = [1, 2, 7, 16, 17, 33, 64]
GPU_MS = [1, 5, 32]
GPU_KS = [1, 3, 130]


def quadratic(D, seed=0):
    """lbfgs_batched_ref.gaussian_fun rescaled to condition <= 100: the same eigenvectors, the spectrum of the precision mapped
    log-uniformly onto [1, min(cond, 100)]"""
    f = lref.gaussian_fun(D, seed)
    w, V = np.linalg.eigh(f.P)
    if w[-1] / w[0] > 100.0:
        w = np.exp(np.log(w / w[0]) * (np.log(100.0) / np.log(w[-1] / w[0])))
    else:
        w = w / w[0]
    P = (V * w) @ V.T
    P = 0.5 * (P + P.T)
    mean = f.mean

    def fun(x):
        r = x - mean
        return 0.5 * float(r @ P @ r), P @ r
    fun.mean, fun.P = mean, P
    return fun


def isotropic(K, D, var, seed=0):
    """N(m_k, var I): means (K, D), the start points at distance 3 from them (so the first steepest-descent trial, of length
    min(|g|, 1), passes the Armijo test for every var >= 0.25), phi and its gradient"""
    rs = np.random.RandomState(100 * D + seed)
    means = rs.standard_normal((K, D))
    u = rs.standard_normal((K, D))
    x0 = means + 3.0 * u / np.linalg.norm(u, axis=1, keepdims=True)
    return means, x0


def isotropic_elbo(D, var, lp_at_mean=0.0):
    """lp - log q is this constant at every draw when q = N(m, var I) and lp = lp(m) - |x - m|^2 / (2 var)"""
    return lp_at_mean + 0.5 * D * np.log(2.0 * np.pi * var)


# ---- the stand-in engine of the host-logic tests ---------------------------------------------------------------------------
def unpack(state, k, opt):
    """problem k of a packed L-BFGS state as the dict tests/lbfgs_batched_ref.py steps"""
    i, sc = state["ist"][k], state["sc"][k]
    return dict(x=state["x"][k].copy(), f=float(sc[0]), g=state["g"][k].copy(), d=state["d"][k].copy(), t=float(sc[1]),
                gd=float(sc[2]), nls=int(i[3]), S=state["S"][k].copy(), Y=state["Y"][k].copy(), sy=sc[4:14].copy(),
                yy=sc[14:24].copy(), npairs=int(i[4]), head=int(i[5]), nit=int(i[1]), nfev=int(i[2]), status=int(i[0]),
                xt=state["Xt"][k].copy(), opt=dict(opt), visits=collections.Counter(), margins=[])


class StandInEngine(OracleBatchedEngine, sref.RestatementEngine, gref.RestatementEngine):
    """tests/engines.py's OracleBatchedEngine (so ``GSMBatch.fit`` runs on it) with the target launches of the GLM and softmax
    restatements, the L-BFGS launch stepped by tests/lbfgs_batched_ref.py and the two Pathfinder launches restated in float64
    (this file).  ``calls`` records every engine call; the launches as tuples."""
    name = "restatement-pathfinder(test-only)"

    def new_flag(self):
        return np.zeros(1, dtype=np.int32)

    def read_flag(self, flag):
        self._rec("read_flag")
        return int(flag[0])

    def logistic_batched(self, X, A, y, counts=None, prior_prec=1.0, out=None, lp_out=None, want="g"):
        """BatchedLogisticTarget's own entry: the GLM restatement's logistic family, no offset"""
        return self.glm_batched(X, A, y, "logistic", counts=counts, prior_prec=prior_prec, out=out, lp_out=lp_out, want=want)

    def lbfgs_state_batched(self, x0):
        self._rec("lbfgs_state")
        x0 = np.array(x0, dtype=np.float64)
        K, D = x0.shape
        return dict(x=x0.copy(), g=np.zeros((K, D)), d=np.zeros((K, D)), Xt=x0.copy(), S=np.zeros((K, HIST, D)),
                    Y=np.zeros((K, HIST, D)), sc=np.zeros((K, lref.NSC)), ist=np.zeros((K, lref.NIS), dtype=np.int32),
                    stopped=self.new_flag())

    def lbfgs_step_batched(self, fv, gv, state, start=False, sign=-1.0, maxiter=1000, maxfun=1000, gtol=1e-5, ftol=lref.FTOL):
        self._rec(("lbfgs_step", bool(start)))
        opt = dict(gtol=gtol, ftol=ftol, maxiter=maxiter, maxfun=maxfun)
        for k in range(state["x"].shape[0]):
            if start:
                new, was = lref.start(state["x"][k], sign * fv[k], sign * np.asarray(gv[k]), **opt), 0
            else:
                old = unpack(state, k, opt)
                was = old["status"]
                new = lref.step(old, sign * fv[k], sign * np.asarray(gv[k]))
            one = lref.pack([new])
            for name in ("x", "g", "d", "Xt", "S", "Y", "sc", "ist"):
                state[name][k] = one[name][0]                               # in place: the caller holds views
            if was == 0 and new["status"] != 0:
                state["stopped"][0] += 1

    def pathfinder_state_batched(self, x0, M):
        self._rec(("pathfinder_state", int(M)))
        x0 = np.array(x0, dtype=np.float64)
        K, D = x0.shape
        pf = dict(seen=np.full(K, -1, dtype=np.int64), fresh=np.zeros(K, dtype=np.int64), mu=np.zeros((K, D)),
                  cov=np.zeros((K, D, D)), X=np.zeros((K, int(M), D)), logq=np.zeros(K), info=np.zeros(K, dtype=np.int64))
        pf.update(new_best(x0))
        return pf

    def pathfinder_propose_batched(self, lbfgs_state, pf_state, seeds, h0=0.0):
        K, M, D = pf_state["X"].shape
        self._rec(("propose", float(h0)))
        normals = lambda k, nit: orc.philox_randn(int(seeds[k]), nit, M * D).reshape(M, D)      # noqa: E731
        p = propose(lbfgs_state, pf_state["seen"], normals, M, h0, dtype=np.float64)
        fr = p["fresh"] != 0
        for name in ("fresh", "seen", "X", "logq"):
            pf_state[name][...] = p[name]
        for name in ("mu", "cov", "info"):
            pf_state[name][fr] = p[name][fr]

    def pathfinder_select_batched(self, lpsum, lbfgs_state, pf_state):
        K, M, D = pf_state["X"].shape
        self._rec("select")
        new = select(lpsum, pf_state["logq"], pf_state["fresh"], pf_state["info"], lbfgs_state["ist"][:, 1], pf_state["mu"],
                     pf_state["cov"], {k: pf_state[k] for k in new_best(np.zeros((K, D)))}, M)
        for name, v in new.items():
            pf_state[name][...] = v


# ---- the C ABI's argument checks (NULL context) ------------------------------------------------------------------------------
def check_bad_arguments(lib):
    """both entry points with a NULL context: every bad argument returns GSMVI_ERR_BAD_ARG (1) with its own message, so nothing can
    have been enqueued; valid calls end at the context"""
    import ctypes as C
    err = lambda: (lib.gsmvi_last_error() or b"").decode()          # noqa: E731
    buf = (C.c_double * (1024 * 24))()
    p = C.cast(buf, C.c_void_p).value
    at = lambda i: p + 8 * 1024 * i                                   # noqa: E731  (slots of 8 KB: K = 2, D = 4, M = 8 fit)
    P = dict(x=at(0), g=at(1), S=at(2), Y=at(3), sc=at(4), ist=at(5), seeds=at(6), seen=at(7), fresh=at(8), mu=at(9), cov=at(10),
             X=at(11), logq=at(12), info=at(13))
    Q = dict(lpsum=at(14), logq=at(12), fresh=at(8), info=at(13), ist=at(5), mu=at(9), cov=at(10), elbo_last=at(15), npts=at(16),
             best_elbo=at(17), best_mean=at(18), best_cov=at(19), best_it=at(20))

    def prop(K=2, D=4, M=8, h0=0.0, **kw):
        a = dict(P, **kw)
        return lib.gsmvi_pathfinder_propose_batched_f64(None, None, K, D, M, a["x"], a["g"], a["S"], a["Y"], a["sc"], a["ist"],
                                                        a["seeds"], a["seen"], h0, a["fresh"], a["mu"], a["cov"], a["X"], a["logq"],
                                                        a["info"])

    def sel(K=2, D=4, M=8, **kw):
        a = dict(Q, **kw)
        return lib.gsmvi_pathfinder_select_batched_f64(None, None, K, D, M, a["lpsum"], a["logq"], a["fresh"], a["info"], a["ist"],
                                                       a["mu"], a["cov"], a["elbo_last"], a["npts"], a["best_elbo"], a["best_mean"],
                                                       a["best_cov"], a["best_it"])

    for f, names, fname in ((prop, P, "gsmvi_pathfinder_propose_batched_f64"), (sel, Q, "gsmvi_pathfinder_select_batched_f64")):
        assert f() == 1 and "ctx is NULL" in err() and fname in err()          # everything else is in order
        assert f(D=0) == 1 and "D must be" in err()
        assert f(D=65) == 1 and "D must be" in err()
        assert f(K=0) == 1 and "K must be" in err()
        assert f(K=2 ** 26) == 1 and "K must be" in err()                      # (D = 4: four problems per workgroup)
        assert f(M=0) == 1 and "M must be" in err()
        assert f(M=4097) == 1 and "M must be" in err()
        for name in names:
            assert f(**{name: None}) == 1 and "NULL array" in err(), name
    assert prop(h0=-1.0) == 1 and "h0" in err()
    assert prop(h0=float("nan")) == 1 and "h0" in err()
    assert prop(h0=float("inf")) == 1 and "h0" in err()
    assert prop(h0=2.5) == 1 and "ctx is NULL" in err()
    assert prop(mu=P["x"]) == 1 and "mu overlaps x" in err()
    assert prop(X=P["S"] + 8) == 1 and "X overlaps S" in err()
    assert prop(seen=P["ist"] + 4) == 1 and "seen overlaps ist" in err()
    assert prop(g=P["x"]) == 1 and "ctx is NULL" in err()                     # read-only arrays may overlap
    assert sel(best_cov=Q["cov"]) == 1 and "best_cov overlaps cov" in err()
    assert sel(best_elbo=Q["elbo_last"]) == 1 and "overlaps" in err()
    assert sel(npts=Q["fresh"]) == 1 and "npts overlaps fresh" in err()
    assert sel(lpsum=Q["logq"]) == 1 and "ctx is NULL" in err()
