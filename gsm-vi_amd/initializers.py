"""Initialisers for the fit drivers (off the hot path, host side).

``lbfgs_init`` follows gsmvi/initializers.py:5-17: maximise ``lp`` with scipy's L-BFGS-B and hand back the
optimum together with the optimiser's dense inverse-Hessian estimate as the starting (mean, cov) of
``GSM.fit`` / ``BaM.fit``, plus the scipy result object.  Additions: ``lp`` / ``lp_g`` may be the
device-native callables of this package (they are fed a (1, D) CUDA tensor then), and ``lp`` may return a
one-element array instead of a scalar.

``lbfgs_init_batched`` is the same initialiser for the K problems of a batched fit (``GSMBatch``, ``BaMBatch``, ``ADVIBatch``):
plain L-BFGS with a backtracking line search in HIP (csrc/gsmvi_lbfgs_batched.hip), one launch per function evaluation after
the score and ``lp``, whatever K is.

``pathfinder_init_batched`` walks the same L-BFGS path and picks the start by how well it fits: every accepted iterate
defines a Gaussian from the pairs held at that moment, a few draws estimate its ELBO, and the best is returned (single-path
Pathfinder; csrc/gsmvi_pathfinder_batched.hip).  Any target with ``lp`` and ``lp_g``.

``laplace_init_batched`` is the second-order start for the built-in GLM targets (``BatchedGLMTarget``,
``BatchedLogisticTarget``): a damped Newton (IRLS) iteration in HIP (csrc/gsmvi_laplace_batched.hip), one launch per round, and
the Laplace covariance (A^T W A + lam I)^-1 at the mode.  ``laplace_init_softmax_batched`` is the same start for
``BatchedSoftmaxTarget``, on the class-coupled Hessian of the multinomial logit (csrc/gsmvi_softmax_laplace_batched.hip), and
``laplace_init_shared_batched`` for ``SharedDesignGLMTarget``, K problems with observation weights on one design matrix that is
never replicated (csrc/gsmvi_laplace_shared_batched.hip); the three share one host loop.
"""
from dataclasses import dataclass

import numpy as np
from scipy.optimize import minimize


def _host_callable(fn, D, vector):
    """Wrap ``fn`` (numpy or device-native, taking (D,) or (1, D)) as a float64 numpy function of a (D,) point."""
    native = getattr(fn, "device_native", False)

    def call(x):
        x = np.asarray(x, dtype=np.float64)
        if native:
            import torch
            out = fn(torch.as_tensor(x[None, :], device="cuda"))
            out = out.detach().to("cpu").numpy()
        else:
            out = fn(x)
            if hasattr(out, "detach"):
                out = out.detach().to("cpu").numpy()
            out = np.asarray(out, dtype=np.float64)
        return out.reshape(D) if vector else float(out.reshape(-1)[0])
    return call


def lbfgs_init(x0, lp, lp_g=None, maxiter=1000, maxfun=1000):
    """Returns ``(mu, cov, res)``: the L-BFGS-B maximiser of ``lp`` started at ``x0``, the dense inverse
    Hessian approximation at it, and the ``scipy.optimize.OptimizeResult`` (gsmvi/initializers.py:5-17).
    Without ``lp_g`` scipy differentiates numerically, as the reference does."""
    x0 = np.asarray(x0, dtype=np.float64)
    D = x0.shape[0]
    value = _host_callable(lp, D, vector=False)
    neg = lambda x: -value(x)
    jac = None
    if lp_g is not None:
        score = _host_callable(lp_g, D, vector=True)
        jac = lambda x: -score(x)
    res = minimize(neg, x0, method="L-BFGS-B", jac=jac, options={"maxiter": maxiter, "maxfun": maxfun})
    return res.x, res.hess_inv.todense(), res


@dataclass
class LbfgsBatchedResult:
    """What ``lbfgs_init_batched`` found, per problem (arrays of length K, or (K, D)): the minimiser ``x`` of -lp, ``fun`` = -lp
    and ``jac`` = -score at it, iterations ``nit`` and evaluations ``nfev`` the problem used before it stopped, ``status``
    (1 converged, 2 ``maxiter`` or ``maxfun`` reached, 3 line search failed, 4 non-finite start; 0 still running: only when the
    loop was cut short) and ``success`` = ``status == 1``.  ``nlaunch`` is shared: the evaluation rounds that ran.  Every
    problem is scored in every round, so it is the ``offset_evals`` of a ``BatchedKLMonitor`` that follows the fits."""
    x: np.ndarray
    fun: np.ndarray
    jac: np.ndarray
    nit: np.ndarray
    nfev: np.ndarray
    status: np.ndarray
    success: np.ndarray
    nlaunch: int


def lbfgs_init_batched(x0, lp, lp_g, maxiter=1000, maxfun=1000, *, gtol=1e-5, ftol=2.220446049250313e-09, check_every=8,
                       as_torch=False, engine=None):
    """``lbfgs_init`` (gsmvi/initializers.py:5-17) for K problems of one D at once: returns ``(mean (K, D), cov (K, D, D), res)``,
    the L-BFGS maximisers of ``lp_k``, the dense BFGS inverse-Hessian products of the stored pairs on an identity base (what
    ``res.hess_inv.todense()`` is in scipy: ``LbfgsInvHessProduct(S, Y).todense()``) and a ``LbfgsBatchedResult``.

    ``x0``: (K, D), or (D,): the same start for every problem (K is then the ``K`` of the target whose method ``lp`` is, 1 if it
    has none).  1 <= D <= 64, K >= 1.  ``lp_g``: (K, 1, D) -> (K, 1, D), ``lp``: (K, 1, D) -> (K,) or
    (K, 1): the batched callables of the fits and of ``BatchedKLMonitor`` (``device_native`` ones stay on the GPU; any other
    score goes through the host round trip of the fits).  Both are required: the line search needs the value, and the
    reference's numerical-gradient fallback (scipy's, without ``lp_g``) is not carried over.

    This is plain L-BFGS (history 10, scipy's ``maxcor``) with an Armijo backtracking search (c1 = 1e-4, halving, 20 rejected
    trials at most), not a port of L-BFGS-B: no bounds, no Cauchy point, no More-Thuente search, so the evaluation counts differ
    from scipy's (on well-conditioned posteriors by one or two, on ill-conditioned quadratics of D <= 10 by more: L-BFGS-B's
    subspace step is missing).  ``maxiter``, ``maxfun``, ``gtol``, ``ftol`` are scipy's L-BFGS-B options at scipy's defaults as
    the reference passes them.  A round is: ``lp_g`` and ``lp`` at the K trial points, then one launch that accepts or rejects
    every problem's trial, updates its state and writes the next trial points.  A problem that has stopped is frozen, bit for
    bit, while the others go on.  The loop does not synchronise per round: it reads the device's count of stopped problems
    every ``check_every`` rounds and leaves when it equals K, so the result does not depend on ``check_every``; only
    ``res.nlaunch`` does.  Prints nothing."""
    from ._fitloop import scorer, takes_out
    from .batched import MAX_D
    from .monitors import lp_sums
    if lp is None or lp_g is None:
        raise ValueError("lbfgs_init_batched: lp and lp_g are both required (no numerical gradient)")
    if not hasattr(x0, "shape"):
        x0 = np.asarray(x0, dtype=np.float64)
    shape = tuple(int(n) for n in x0.shape)
    if len(shape) == 1:                                 # one start for every problem of the target that owns lp
        shape = (int(getattr(getattr(lp, "__self__", None), "K", 1)),) + shape
    elif len(shape) != 2:
        raise ValueError(f"lbfgs_init_batched: x0 must be (K, D) or (D,), got {tuple(x0.shape)}")
    K, D = shape
    if not 1 <= D <= MAX_D:
        raise ValueError(f"lbfgs_init_batched: D = {D} is outside 1 <= D <= {MAX_D}")
    if K < 1:
        raise ValueError(f"lbfgs_init_batched: K = {K} must be at least 1")
    maxiter, maxfun, check_every = int(maxiter), int(maxfun), int(check_every)
    if maxiter < 1 or maxfun < 2 or check_every < 1:
        raise ValueError("lbfgs_init_batched: maxiter and check_every must be at least 1, maxfun at least 2")
    if not (gtol >= 0.0 and ftol >= 0.0):
        raise ValueError("lbfgs_init_batched: gtol and ftol must be >= 0")
    if engine is None:
        from .engine import get_engine
        engine = get_engine()
    eng = engine
    x0 = eng.asarray(x0)
    st = eng.lbfgs_state_batched(x0.reshape(K, D) if x0.dim() == 2 else x0.expand(K, D))
    Xt = st["Xt"].reshape(K, 1, D)                      # the trial points where the callables read them (a view)
    score = scorer(eng, lp_g)
    Gbuf = eng.empty(K, 1, D) if not getattr(lp_g, "device_native", False) or takes_out(lp_g) else None
    nlaunch = 0
    for r in range(1, maxfun + 1):
        G = score(Xt, out=Gbuf) if Gbuf is not None else score(Xt)
        v = lp_sums(lp, Xt, eng, K)
        eng.lbfgs_step_batched(v.contiguous(), G.reshape(K, D), st, start=r == 1, sign=-1.0, maxiter=maxiter, maxfun=maxfun,
                               gtol=gtol, ftol=ftol)
        nlaunch = r
        if r % check_every == 0 and eng.read_flag(st["stopped"]) == K:
            break
    cov = eng.lbfgs_hess_inv_batched(st)
    ist = eng.read_ints(st["ist"])
    status = ist[:, 0]
    res = LbfgsBatchedResult(x=eng.to_numpy(st["x"]), fun=eng.to_numpy(st["sc"][:, 0]).copy(), jac=eng.to_numpy(st["g"]),
                             nit=ist[:, 1].copy(), nfev=ist[:, 2].copy(), status=status.copy(), success=status == 1,
                             nlaunch=nlaunch)
    return (st["x"], cov, res) if as_torch else (res.x.copy(), eng.to_numpy(cov), res)


@dataclass
class PathfinderBatchedResult:
    """What ``pathfinder_init_batched`` found, per problem (arrays of length K, or (K, D)).  The L-BFGS fields are those of
    ``LbfgsBatchedResult``, bit for bit what ``lbfgs_init_batched`` reports with the same options: ``x``, ``fun``, ``jac``, ``nit``,
    ``nfev``, ``status`` and the shared ``nlaunch``.  ``elbo`` is the best ELBO estimate along the path (-inf: no path point had
    a finite one), ``best_it`` the L-BFGS iteration whose Gaussian was returned (0: the start point; -1: none), ``n_points`` the
    path points that were tried, ``success`` = ``best_it >= 0``.  ``nevals`` = ``nlaunch`` (1 + M) is shared: every round
    evaluates ``lp`` at the trial point and at the M draws of every problem, so it is the ``offset_evals`` of a
    ``BatchedKLMonitor`` that follows the fits."""
    x: np.ndarray
    fun: np.ndarray
    jac: np.ndarray
    nit: np.ndarray
    nfev: np.ndarray
    status: np.ndarray
    success: np.ndarray
    nlaunch: int
    elbo: np.ndarray
    best_it: np.ndarray
    n_points: np.ndarray
    nevals: int


def pathfinder_init_batched(x0, lp, lp_g, maxiter=1000, maxfun=1000, *, num_elbo_draws=5, h0="pair", seed=0, gtol=1e-5,
                            ftol=2.220446049250313e-09, check_every=8, as_torch=False, engine=None):
    """Single-path Pathfinder (Zhang, Carpenter, Gelman, Vehtari 2022) for K problems of one D at once: returns ``(mean (K, D),
    cov (K, D, D), res)``, the Gaussian along the L-BFGS path of ``lbfgs_init_batched`` with the best ELBO estimate and a
    ``PathfinderBatchedResult``.  It fills the role of ``lbfgs_init`` (gsmvi/initializers.py:5-17) with a start that is chosen by
    how well it fits, for any target with ``lp`` and ``lp_g``.

    ``x0``, ``lp``, ``lp_g``, ``maxiter``, ``maxfun``, ``gtol``, ``ftol``, ``check_every``: as in ``lbfgs_init_batched``; the
    L-BFGS trajectory is the same, bit for bit.  Every accepted iterate x (the start point included) defines N(mu, Sigma):
    Sigma = the BFGS inverse-Hessian product of the pairs held at that moment on the base gamma I, mu = x + Sigma score(x).
    ``h0`` = "pair": gamma = s.y / y.y of the newest pair, the scale the two-loop recursion uses (1 before the first pair); a
    positive float fixes gamma (1.0 gives ``lbfgs_init_batched``'s covariance at every point).  The paper's diagonal base alpha
    is replaced by gamma I: a stated simplification.  ``num_elbo_draws`` = M in 1 .. 4096 draws per path
    point, from the counter-based stream of key ``engine.batched_seeds``(seed + k) and draw number = the iteration, estimate
    ELBO = mean(lp(x_s) - log q(x_s)); the first maximum over the path wins.  A round is six launches against
    ``lbfgs_init_batched``'s three: score and lp at the trial points, the L-BFGS step, the proposal, lp at the (K, M, D) draws,
    the selection.  A problem whose path has no finite ELBO keeps its last x, the identity covariance and ``elbo`` = -inf
    (what ``laplace_init_batched`` does for a lost problem).  The result does not depend on ``check_every``; only ``res.nlaunch``
    and ``res.nevals`` do.  Prints nothing."""
    from ._fitloop import scorer, takes_out
    from .batched import MAX_D
    from .monitors import lp_sums
    if lp is None or lp_g is None:
        raise ValueError("pathfinder_init_batched: lp and lp_g are both required (no numerical gradient)")
    if not hasattr(x0, "shape"):
        x0 = np.asarray(x0, dtype=np.float64)
    shape = tuple(int(n) for n in x0.shape)
    if len(shape) == 1:                                 # one start for every problem of the target that owns lp
        shape = (int(getattr(getattr(lp, "__self__", None), "K", 1)),) + shape
    elif len(shape) != 2:
        raise ValueError(f"pathfinder_init_batched: x0 must be (K, D) or (D,), got {tuple(x0.shape)}")
    K, D = shape
    if not 1 <= D <= MAX_D:
        raise ValueError(f"pathfinder_init_batched: D = {D} is outside 1 <= D <= {MAX_D}")
    if K < 1:
        raise ValueError(f"pathfinder_init_batched: K = {K} must be at least 1")
    maxiter, maxfun, check_every = int(maxiter), int(maxfun), int(check_every)
    if maxiter < 1 or maxfun < 2 or check_every < 1:
        raise ValueError("pathfinder_init_batched: maxiter and check_every must be at least 1, maxfun at least 2")
    if not (gtol >= 0.0 and ftol >= 0.0):
        raise ValueError("pathfinder_init_batched: gtol and ftol must be >= 0")
    M = int(num_elbo_draws)
    if M != num_elbo_draws or not 1 <= M <= 4096:
        raise ValueError(f"pathfinder_init_batched: num_elbo_draws = {num_elbo_draws} is outside 1 <= num_elbo_draws <= 4096")
    if isinstance(h0, str):
        if h0 != "pair":
            raise ValueError(f"pathfinder_init_batched: h0 must be \"pair\" or a positive float, got {h0!r}")
        base = 0.0
    else:
        base = float(h0)
        if not (base > 0.0 and base < float("inf")):
            raise ValueError(f"pathfinder_init_batched: h0 must be \"pair\" or a positive float, got {h0!r}")
    if engine is None:
        from .engine import get_engine
        engine = get_engine()
    eng = engine
    x0 = eng.asarray(x0)
    x0 = x0.reshape(K, D) if len(x0.shape) == 2 else (x0.expand(K, D) if hasattr(x0, "expand") else np.broadcast_to(x0, (K, D)))
    st = eng.lbfgs_state_batched(x0)
    pf = eng.pathfinder_state_batched(st["x"], M)
    seeds = eng.batched_seeds([int(seed) + k for k in range(K)])
    Xt = st["Xt"].reshape(K, 1, D)                      # the trial points where the callables read them (a view)
    score = scorer(eng, lp_g)
    Gbuf = eng.empty(K, 1, D) if not getattr(lp_g, "device_native", False) or takes_out(lp_g) else None
    packed = lambda v: v.contiguous() if hasattr(v, "contiguous") else np.ascontiguousarray(v)      # noqa: E731
    nlaunch = 0
    for r in range(1, maxfun + 1):
        G = score(Xt, out=Gbuf) if Gbuf is not None else score(Xt)
        v = lp_sums(lp, Xt, eng, K)
        eng.lbfgs_step_batched(packed(v), G.reshape(K, D), st, start=r == 1, sign=-1.0, maxiter=maxiter, maxfun=maxfun,
                               gtol=gtol, ftol=ftol)
        eng.pathfinder_propose_batched(st, pf, seeds, h0=base)
        eng.pathfinder_select_batched(packed(lp_sums(lp, pf["X"], eng, K)), st, pf)
        nlaunch = r
        if r % check_every == 0 and eng.read_flag(st["stopped"]) == K:
            break
    ist = eng.read_ints(st["ist"])
    status = ist[:, 0]
    best_it = eng.read_ints(pf["best_it"])
    mean, cov = pf["best_mean"], pf["best_cov"]
    lost = np.flatnonzero(best_it < 0)
    if lost.size:                                       # no finite ELBO on the path: the last x (the covariance is still I)
        if isinstance(mean, np.ndarray):
            mean[lost] = st["x"][lost]
        else:
            import torch
            idx = torch.as_tensor(lost, device=mean.device)
            mean[idx] = st["x"][idx]
    res = PathfinderBatchedResult(x=eng.to_numpy(st["x"]), fun=eng.to_numpy(st["sc"][:, 0]).copy(), jac=eng.to_numpy(st["g"]),
                                  nit=ist[:, 1].copy(), nfev=ist[:, 2].copy(), status=status.copy(), success=best_it >= 0,
                                  nlaunch=nlaunch, elbo=eng.to_numpy(pf["best_elbo"]).copy(), best_it=best_it.copy(),
                                  n_points=eng.read_ints(pf["npts"]).copy(), nevals=nlaunch * (1 + M))
    return (mean, cov, res) if as_torch else (eng.to_numpy(mean).copy(), eng.to_numpy(cov).copy(), res)


@dataclass
class LaplaceBatchedResult:
    """What ``laplace_init_batched`` found, per problem (arrays of length K, or (K, D)): the minimiser ``x`` of -lp, ``fun`` = -lp
    and ``jac`` = -score at it, Newton iterations ``nit`` and evaluations ``nfev`` the problem used before it stopped, ``status``
    (1 converged, 2 ``maxiter`` or ``maxfun`` reached, 3 line search failed, 4 non-finite start, 5 Hessian not positive definite;
    0 still running: only when the loop was cut short), ``info`` of the final factorisation (0, or 1 + the first failing pivot)
    and ``success`` = ``status == 1`` and ``info == 0``.  A problem without success returns its last ``x`` and the identity
    covariance (nothing is known: what ``lbfgs_init_batched`` gives without a pair), which keeps a following fit alive.
    ``nlaunch`` is shared: the rounds that ran, the ``offset_evals`` of a ``BatchedKLMonitor`` that follows the fits (a stopped
    problem is not evaluated again, so this is an upper bound per problem)."""
    x: np.ndarray
    fun: np.ndarray
    jac: np.ndarray
    nit: np.ndarray
    nfev: np.ndarray
    status: np.ndarray
    success: np.ndarray
    info: np.ndarray
    nlaunch: int


def laplace_init_batched(target, x0=None, maxiter=100, maxfun=200, *, gtol=1e-8, check_every=4, as_torch=False, engine=None):
    """The Laplace start of K GLM posteriors at once: returns ``(mean (K, D), cov (K, D, D), res)``, the Newton modes of
    ``lp_k``, the inverses of the negative Hessians A_k^T W A_k + lam_k I there and a ``LaplaceBatchedResult``.  It fills the
    role of ``lbfgs_init`` (gsmvi/initializers.py:5-17) for the models whose second derivative is closed-form.

    ``target``: a ``BatchedGLMTarget`` or a ``BatchedLogisticTarget`` (anything else: TypeError).  ``x0``: None (zeros), (D,)
    (the same start for every problem) or (K, D).  All four families are log-concave, so the damped Newton iteration (full
    step, Armijo backtracking with c1 = 1e-4 and a slack of 1e-10 max(1, |f|), halving, at most 20 rejected trials) converges
    from any start when the prior is proper; with a flat prior on separable data there is no mode, and the problem ends with
    ``status`` 2 or 5 and is reported, not hidden.  A round is ONE launch: f, g and H at the K trial points in one sweep over the
    data, the accept / reject decision, the stopping test max|g| <= ``gtol``, the factorisation and the next trial point.  A
    problem that has stopped is frozen, bit for bit, and its data are not read again.  The loop does not synchronise per round:
    it reads the device's count of stopped problems every ``check_every`` rounds and leaves when it equals K, so the result
    does not depend on ``check_every``; only ``res.nlaunch`` does.  One more launch gives the covariance at the final points.
    Prints nothing."""
    from .targets import BatchedGLMTarget, SharedDesignGLMTarget
    if not isinstance(target, BatchedGLMTarget):
        hint = "; call laplace_init_shared_batched(target, ...) for it" if isinstance(target, SharedDesignGLMTarget) else ""
        raise TypeError(f"laplace_init_batched: target must be a BatchedGLMTarget or a BatchedLogisticTarget, "
                        f"got {type(target).__name__}{hint}")
    model = dict(offset=target.offset, counts=target.counts, prior_prec=target.prior_precision,
                 noise_prec=target.noise_precision)
    eng = engine if engine is not None else target.engine
    return _laplace_run("laplace_init_batched", target, x0, maxiter, maxfun, gtol, check_every, as_torch, eng,
                        lambda st, **kw: eng.laplace_step_batched(st, target.A, target.y, target.family, **kw, **model),
                        lambda x: eng.glm_hessian_batched(x, target.A, target.y, target.family, want="cov", **model))


def _laplace_run(name, target, x0, maxiter, maxfun, gtol, check_every, as_torch, eng, step, cov_at):
    """The host loop of the Laplace initialisers, once: the argument checks (errors carry ``name``), the state, one ``step(state,
    start=, maxiter=, maxfun=, gtol=)`` launch per round until the device's count of stopped problems equals K, then
    ``cov_at(x)`` -> (cov, info) at the final points, the identity for every problem without success, and the result."""
    K, D = target.K, target.D
    maxiter, maxfun, check_every = int(maxiter), int(maxfun), int(check_every)
    if maxiter < 1 or maxfun < 2 or check_every < 1:
        raise ValueError(f"{name}: maxiter and check_every must be at least 1, maxfun at least 2")
    if not gtol >= 0.0:
        raise ValueError(f"{name}: gtol must be >= 0")
    if x0 is None:
        x0 = np.zeros((K, D))
    elif not hasattr(x0, "shape"):
        x0 = np.asarray(x0, dtype=np.float64)
    shape = tuple(int(n) for n in x0.shape)
    if shape not in ((D,), (K, D)):
        raise ValueError(f"{name}: x0 must be None, (D,) = {(D,)} or (K, D) = {(K, D)}, got {shape}")
    x0 = eng.asarray(x0)
    if len(shape) == 1:
        x0 = x0.reshape(1, D).repeat(K, 0) if isinstance(x0, np.ndarray) else x0.reshape(1, D).expand(K, D)
    st = eng.laplace_state_batched(x0)
    nlaunch = 0
    for r in range(1, maxfun + 1):
        step(st, start=r == 1, maxiter=maxiter, maxfun=maxfun, gtol=gtol)
        nlaunch = r
        if r % check_every == 0 and eng.read_flag(st["stopped"]) == K:
            break
    cov, info = cov_at(st["x"])
    ist = eng.read_ints(st["ist"])
    status, info = ist[:, 0].copy(), eng.read_ints(info)
    success = (status == 1) & (info == 0)
    lost = np.flatnonzero(~success)
    if lost.size:                                       # (info != 0 already gave the identity; status != 1 does here)
        if isinstance(cov, np.ndarray):
            cov[lost] = np.eye(D)
        else:
            import torch
            cov[torch.as_tensor(lost, device=cov.device)] = torch.eye(D, dtype=cov.dtype, device=cov.device)
    res = LaplaceBatchedResult(x=eng.to_numpy(st["x"]), fun=eng.to_numpy(st["sc"][:, 0]).copy(), jac=eng.to_numpy(st["g"]),
                               nit=ist[:, 1].copy(), nfev=ist[:, 2].copy(), status=status, success=success, info=info,
                               nlaunch=nlaunch)
    return (st["x"], cov, res) if as_torch else (res.x.copy(), eng.to_numpy(cov), res)


def laplace_init_softmax_batched(target, x0=None, maxiter=100, maxfun=200, *, gtol=1e-8, check_every=4, as_torch=False, engine=None):
    """The Laplace start of K multinomial logit posteriors at once: returns ``(mean (K, D), cov (K, D, D), res)``, the Newton
    modes of ``lp_k``, the inverses of the negative Hessians there (``BatchedSoftmaxTarget.neg_hessian``: block (c, c') is
    sum_n w_n,cc' a_n a_n^T + lam_k [c = c'] I) and a ``LaplaceBatchedResult``.  It fills the role of ``lbfgs_init``
    (gsmvi/initializers.py:5-17) for the softmax target.

    ``target``: a ``BatchedSoftmaxTarget`` (anything else: TypeError).  The posterior is log-concave, and everything else --
    ``x0``, the damped Newton iteration and its line search, the stopping rule, ``check_every``, one launch per round
    (csrc/gsmvi_softmax_laplace_batched.hip), the frozen problems, the failure policy (a problem without success returns its
    last ``x`` and the identity) and the defaults -- is ``laplace_init_batched``'s, word for word.  Prints nothing."""
    from .targets import BatchedSoftmaxTarget
    if not isinstance(target, BatchedSoftmaxTarget):
        raise TypeError(f"laplace_init_softmax_batched: target must be a BatchedSoftmaxTarget, got {type(target).__name__}")
    model = dict(counts=target.counts, prior_prec=target.prior_precision)
    eng = engine if engine is not None else target.engine
    return _laplace_run("laplace_init_softmax_batched", target, x0, maxiter, maxfun, gtol, check_every, as_torch, eng,
                        lambda st, **kw: eng.softmax_laplace_step_batched(st, target.A, target.y, target.C, **kw, **model),
                        lambda x: eng.softmax_hessian_batched(x, target.A, target.y, target.C, want="cov", **model))


def laplace_init_shared_batched(target, x0=None, maxiter=100, maxfun=200, *, gtol=1e-8, check_every=4, as_torch=False, engine=None):
    """The Laplace start of K GLM posteriors on ONE design matrix at once: returns ``(mean (K, D), cov (K, D, D), res)``, the
    Newton modes of ``lp_k``, the inverses of the negative Hessians A^T diag(v_k w_k) A + lam_k I there
    (``neg_hessian_shared_batched``) and a ``LaplaceBatchedResult``.  It fills the role of ``lbfgs_init``
    (gsmvi/initializers.py:5-17) for the shared-design target: responses, offsets, observation weights and precisions per
    problem, the design held once and never replicated.

    ``target``: a ``SharedDesignGLMTarget`` (anything else: TypeError).  Weights >= 0 keep all four families log-concave, and
    everything else -- ``x0``, the damped Newton iteration and its line search, the stopping rule, ``check_every``, one launch
    per round (csrc/gsmvi_laplace_shared_batched.hip), the frozen problems, the failure policy (a problem without success
    returns its last ``x`` and the identity) and the defaults -- is ``laplace_init_batched``'s, word for word.  A problem whose
    weights are all zero is its prior: with lam_k > 0 it converges at once at x = 0 with cov = I / lam_k; with lam_k = 0 both its
    gradient and its Hessian are zero.  One thing is this function's own: a problem that the launches stopped by the gradient
    test (the device's status word 1: that test comes before the factorisation) but whose Hessian at that point fails the
    final factorisation (``info`` != 0) is reported with ``res.status`` 5, Hessian not positive definite, not 1: a stationary
    point without a positive definite Hessian is no mode to expand around.  It has no ``success`` and gets the identity, as
    before; the all-zero-weights problem with lam_k = 0 is the plain case (``status`` 5, ``info`` 1).  Prints nothing."""
    from .targets import SharedDesignGLMTarget
    if not isinstance(target, SharedDesignGLMTarget):
        raise TypeError(f"laplace_init_shared_batched: target must be a SharedDesignGLMTarget, got {type(target).__name__}")
    model = dict(offset=target.offset, weights=target.weights, prior_prec=target.prior_precision,
                 noise_prec=target.noise_precision)
    eng = engine if engine is not None else target.engine
    mean, cov, res = _laplace_run(
        "laplace_init_shared_batched", target, x0, maxiter, maxfun, gtol, check_every, as_torch, eng,
        lambda st, **kw: eng.laplace_shared_step_batched(st, target.A, target.y, target.family, **kw, **model),
        lambda x: eng.glm_shared_hessian_batched(x, target.A, target.y, target.family, want="cov", **model))
    res.status = np.where((res.status == 1) & (res.info != 0), 5, res.status)     # stationary, but H is not positive definite
    return mean, cov, res


@dataclass
class LaplaceNegBinBatchedResult(LaplaceBatchedResult):
    """``LaplaceBatchedResult`` of ``laplace_init_negbin_batched`` with ``nmod`` (K,): the Newton rounds of each problem whose
    direction came from a factorisation with a modified last pivot (0: plain Newton throughout)."""
    nmod: np.ndarray = None


def laplace_init_negbin_batched(target, x0=None, maxiter=100, maxfun=200, *, gtol=1e-8, check_every=4, as_torch=False, engine=None):
    """The Laplace start of K negative binomial posteriors at once: returns ``(mean (K, D), cov (K, D, D), res)``, the Newton
    modes of ``lp_k`` in x = (beta, theta), the inverses of the negative Hessians there (``neg_hessian_negbin_batched``) and a
    ``LaplaceNegBinBatchedResult``.  It fills the role of ``lbfgs_init`` (gsmvi/initializers.py:5-17) for the negative binomial
    target.

    ``target``: a ``BatchedNegBinomialTarget`` (anything else: TypeError).  ``x0``, the line search, the stopping rule,
    ``check_every``, one launch per round (csrc/gsmvi_negbin_laplace_batched.hip), the frozen problems, the failure policy (a
    problem without success returns its last ``x`` and the identity) and the defaults are ``laplace_init_batched``'s.  Two things
    are this function's own, because the posterior is not log-concave in theta = log r and the negative Hessian away from the
    mode is often indefinite in that direction (at x0 = 0 for about half of well-posed problems).  First, the last-pivot rule:
    when the factorisation of a round fails at exactly its last pivot -- theta's, given beta -- that pivot is replaced by its
    absolute value (if it is not within 64 eps of the sizes it is the difference of); the modified matrix is positive definite,
    the direction a descent direction, and the Armijo search does the rest.  ``res.nmod`` counts such rounds per problem.  A
    pivot failing before the last still ends the problem with ``status`` 5.  The covariance is never modified: second, as in
    ``laplace_init_shared_batched``, a problem that stopped by the gradient test but whose Hessian at that point is not positive
    definite (``info`` != 0) is reported with ``status`` 5, has no ``success`` and gets the identity.  With a flat prior on theta
    (``log_size_precision`` = 0) and data without overdispersion the mode is at theta = inf: such a problem ends with ``status``
    2, 3 or 5 and is reported, not hidden.  Prints nothing."""
    from .targets import BatchedNegBinomialTarget
    if not isinstance(target, BatchedNegBinomialTarget):
        raise TypeError(f"laplace_init_negbin_batched: target must be a BatchedNegBinomialTarget, got {type(target).__name__}")
    model = dict(offset=target.offset, counts=target.counts, prior_prec=target.prior_precision,
                 log_size_mean=target.log_size_mean, log_size_prec=target.log_size_precision)
    eng = engine if engine is not None else target.engine
    kept = {}

    def step(st, **kw):
        kept["ist"] = st["ist"]
        eng.negbin_laplace_step_batched(st, target.A, target.y, **kw, **model)

    mean, cov, res = _laplace_run(
        "laplace_init_negbin_batched", target, x0, maxiter, maxfun, gtol, check_every, as_torch, eng, step,
        lambda x: eng.negbin_hessian_batched(x, target.A, target.y, want="cov", **model))
    status = np.where((res.status == 1) & (res.info != 0), 5, res.status)         # stationary, but H is not positive definite
    fields = {f: getattr(res, f) for f in ("x", "fun", "jac", "nit", "nfev", "success", "info", "nlaunch")}
    return mean, cov, LaplaceNegBinBatchedResult(status=status, nmod=eng.read_ints(kept["ist"])[:, 4].copy(), **fields)


@dataclass
class LaplaceOrdinalBatchedResult(LaplaceBatchedResult):
    """``LaplaceBatchedResult`` of ``laplace_init_ordinal_batched`` with ``nmod`` (K,): the Newton rounds of each problem whose
    direction came from the retried matrix (0: plain Newton throughout)."""
    nmod: np.ndarray = None


def laplace_init_ordinal_batched(target, x0=None, maxiter=100, maxfun=200, *, gtol=1e-8, check_every=4, as_torch=False, engine=None):
    """The Laplace start of K cumulative-logit posteriors at once: returns ``(mean (K, D), cov (K, D, D), res)``, the Newton
    modes of ``lp_k`` in x = (beta, delta), the inverses of the negative Hessians there (``neg_hessian_ordinal_batched``) and a
    ``LaplaceOrdinalBatchedResult``.  It fills the role of ``lbfgs_init`` (gsmvi/initializers.py:5-17) for the ordinal target.

    ``target``: a ``BatchedOrdinalTarget`` (anything else: TypeError).  ``x0``, the line search, the stopping rule,
    ``check_every``, one launch per round (csrc/gsmvi_ordinal_laplace_batched.hip), the frozen problems, the failure policy (a
    problem without success returns its last ``x`` and the identity) and the defaults are ``laplace_init_batched``'s.  Two things
    are this function's own, because the posterior is not log-concave in delta: the gaps are exp(delta_i), and the chain terms
    c_i = -exp(delta_i) d lp_lik / d gap_i on the diagonal make the negative Hessian indefinite away from the mode (from x0 = 0
    for most problems with 8 or more classes).  First, the retry rule: when the factorisation of a round fails and some c_i is
    negative, those c_i are taken off the diagonal and the matrix is factored once more; the retried matrix is positive
    semi-definite plus the priors, the direction a descent direction, and the Armijo search does the rest.  ``res.nmod``
    counts such rounds per problem.  No negative c_i, or a second failure, ends the problem with ``status`` 5.  The
    covariance is never modified: second, as in ``laplace_init_shared_batched``, a problem that stopped by the gradient test but
    whose Hessian at that point is not positive definite (``info`` != 0) is reported with ``status`` 5, has no ``success`` and
    gets the identity (a problem without valid rows and a flat prior on delta is the plain case).  With a flat prior on
    separable data there is no mode: such a problem ends with ``status`` 2, 3 or 5 and is reported, not hidden.  Prints
    nothing."""
    from .targets import BatchedOrdinalTarget
    if not isinstance(target, BatchedOrdinalTarget):
        raise TypeError(f"laplace_init_ordinal_batched: target must be a BatchedOrdinalTarget, got {type(target).__name__}")
    model = dict(offset=target.offset, counts=target.counts, prior_prec=target.prior_precision, cut_prec=target.cut_precision)
    eng = engine if engine is not None else target.engine
    kept = {}

    def step(st, **kw):
        kept["ist"] = st["ist"]
        eng.ordinal_laplace_step_batched(st, target.A, target.y, target.C, **kw, **model)

    mean, cov, res = _laplace_run(
        "laplace_init_ordinal_batched", target, x0, maxiter, maxfun, gtol, check_every, as_torch, eng, step,
        lambda x: eng.ordinal_hessian_batched(x, target.A, target.y, target.C, want="cov", **model))
    status = np.where((res.status == 1) & (res.info != 0), 5, res.status)         # stationary, but H is not positive definite
    fields = {f: getattr(res, f) for f in ("x", "fun", "jac", "nit", "nfev", "success", "info", "nlaunch")}
    return mean, cov, LaplaceOrdinalBatchedResult(status=status, nmod=eng.read_ints(kept["ist"])[:, 4].copy(), **fields)
