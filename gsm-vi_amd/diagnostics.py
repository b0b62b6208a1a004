"""Diagnostics of fitted batched posteriors: the Pareto-smoothed importance sampling (PSIS) check of K Gaussians q_k = N(mean_k,
cov_k) against their targets, one launch after the target's ``lp`` (csrc/gsmvi_psis_batched.hip; Vehtari, Simpson, Gelman, Yao,
Gabry, "Pareto smoothed importance sampling", JMLR 2024).  ``BatchedKLMonitor`` traces a reverse KL up to each target's unknown
constant; this says per problem, on one scale, whether q_k can be trusted: the shape khat of the importance ratios' tail, the
effective sample size, an estimate of the log normalising constant, and importance-corrected moments.  ``psis_loo_batched`` takes
the same draws one step further for the GLM targets: the PSIS leave-one-out log predictive density of every observation
(csrc/gsmvi_psis_loo_batched.hip; Vehtari, Gelman, Gabry 2017; Magnusson, Andersen, Jonasson, Vehtari 2019), the number by which
fitted models are compared; ``psis_loo_softmax_batched`` is the same for ``BatchedSoftmaxTarget``
(csrc/gsmvi_psis_loo_softmax_batched.hip), ``psis_loo_negbin_batched`` for ``BatchedNegBinomialTarget``
(csrc/gsmvi_psis_loo_negbin_batched.hip), ``psis_loo_ordinal_batched`` for ``BatchedOrdinalTarget``
(csrc/gsmvi_psis_loo_ordinal_batched.hip) and ``psis_loo_shared_batched`` for ``SharedDesignGLMTarget``, observation weights
honoured (the other form of the kernel in csrc/gsmvi_psis_loo_batched.hip)."""
from dataclasses import dataclass

import numpy as np

from .monitors import _to_numpy

MIN_DRAWS, MAX_DRAWS = 5, 4096


def khat_threshold(S):
    """min(1 - 1 / log10(S), 0.7): the khat below which S draws give a usable importance estimate"""
    return min(1.0 - 1.0 / np.log10(S), 0.7)


@dataclass
class PSISBatchedResult:
    """What ``psis_batched`` / ``psis_weights_batched`` return (numpy arrays, or the engine's tensors with ``as_torch``):
    ``khat`` (K,) the tail shape (+inf: the tail had fewer than 5 entries), ``ess`` (K,) the effective sample size of the
    smoothed weights, ``log_z`` (K,) the estimate of log of the integral of exp(lp_k), ``log_weights`` (K, S) the normalised smoothed log
    weights, ``log_ratios`` (K, S) lp_k - log q_k, ``samples`` (K, S, D) the draws, ``mean`` (K, D) and ``cov`` (K, D, D) the
    importance-weighted moments (None without ``moments``), ``info`` (K,): 0, -1 = non-finite ratios, -2 = tail too short,
    1 + the first bad pivot of cov_k (outputs NaN for -1 and the pivot codes), ``threshold`` = min(1 - 1 / log10(S), 0.7),
    ``ok`` (K,) = (info == 0) & (khat < threshold), ``nlaunch`` the kernel launches made.  ``psis_weights_batched`` leaves the
    fields that need q (``samples``, ``mean``, ``cov``) None; its ``log_ratios`` are the caller's."""
    khat: object
    ess: object
    log_z: object
    log_weights: object
    log_ratios: object
    samples: object
    mean: object
    cov: object
    info: object
    threshold: float
    ok: object
    nlaunch: int


def _shape(a):
    return tuple(int(n) for n in a.shape)


def _result(eng, as_torch, S, nlaunch, khat, ess, log_z, lw, logr, X, mean_is, cov_is, info):
    thr = khat_threshold(S)
    ok = (info == 0) & (khat < thr)
    if not as_torch:
        conv = lambda t: None if t is None else np.asarray(eng.to_numpy(t))      # noqa: E731
        khat, ess, log_z, lw, logr, X, mean_is, cov_is, ok = (conv(t) for t in (khat, ess, log_z, lw, logr, X, mean_is, cov_is, ok))
        info = np.asarray(eng.read_ints(info))
    return PSISBatchedResult(khat=khat, ess=ess, log_z=log_z, log_weights=lw, log_ratios=logr, samples=X, mean=mean_is,
                             cov=cov_is, info=info, threshold=thr, ok=ok, nlaunch=nlaunch)


def psis_batched(lp, mean, cov, keys, num_draws=1024, *, call=0, moments=True, as_torch=False, engine=None):
    """The PSIS diagnostic of K fitted Gaussians q_k = N(mean_k, cov_k) against their targets: returns a ``PSISBatchedResult``.

    ``lp`` maps a (K, S, D) block of points to the (K, S) values lp_k(x_ks), unnormalised or not (``BatchedGLMTarget.lp``,
    ``BatchedLogisticTarget.lp``, ``BatchedGaussianTarget.lp_rows``); mean (K, D) and cov (K, D, D) are device tensors or numpy;
    ``keys`` are K per-problem keys.  Two launches and one call of ``lp``: S = ``num_draws`` draws of every q_k (one call of
    ``kl_draw_batched``, the stream of ``BatchedKLMonitor``: seed (keys[k] % 2**32) ^ 0x5DEECE66D, draw number ``call``), then
    ``lp`` once, with the device tensor first and numpy if it refuses it, then ``gsmvi_psis_batched_f64``: log q_k per row, the
    Pareto fit to the largest ratios, the smoothed weights and, with ``moments``, the importance-weighted mean and covariance.
    mean and cov are only read, so a running fit is left bit for bit alone.  The sample block takes K * S * D * 8 bytes of
    device memory (512 MB at K = 8192, S = 1024, D = 8; 4 GB at D = 64), the ratios and weights 2 * K * S * 8 more.
    D outside 1..64, ``num_draws`` outside 5..4096, keys of another length than K or a cov that is not (K, D, D) raise ValueError
    before any device work; so does an ``lp`` that returns (K,) sums -- give ``lp_rows``."""
    from .batched import MAX_D
    if len(_shape(mean)) != 2:
        raise ValueError(f"psis_batched: mean must be (K, D), got {_shape(mean)}")
    K, D = _shape(mean)
    if not 1 <= D <= MAX_D:
        raise ValueError(f"psis_batched: D = {D} is outside 1 <= D <= {MAX_D}")
    if _shape(cov) != (K, D, D):
        raise ValueError(f"psis_batched: cov must be {(K, D, D)}, got {_shape(cov)}")
    S = int(num_draws)
    if S != num_draws or not MIN_DRAWS <= S <= MAX_DRAWS:
        raise ValueError(f"psis_batched: num_draws = {num_draws} is outside {MIN_DRAWS} <= num_draws <= {MAX_DRAWS}")
    keys_l = [int(k) for k in np.asarray(list(keys) if isinstance(keys, (list, tuple, range)) else _to_numpy(keys)).reshape(-1)]
    if len(keys_l) != K:
        raise ValueError(f"psis_batched: {len(keys_l)} keys for K = {K} problems")
    if engine is None:
        from .engine import get_engine
        engine = get_engine()
    eng = engine
    seeds = eng.batched_seeds(tuple((k % (2 ** 32)) ^ 0x5DEECE66D for k in keys_l))
    mu, cv = eng.asarray(mean), eng.asarray(cov)
    X, _, _ = eng.kl_draw_batched(mu, cv, seeds, int(call), 0, S)
    try:
        v = lp(X)
    except (TypeError, AttributeError, RuntimeError, ValueError):
        v = lp(eng.to_numpy(X))
    v = eng.asarray(v)
    if _shape(v) == (K,):
        raise ValueError(f"psis_batched: lp returned ({K},) sums: PSIS needs the ({K}, {S}) values per row -- give lp_rows "
                         "(BatchedGaussianTarget.lp_rows) or a log-density that returns (K, rows)")
    if _shape(v) != (K, S):
        raise ValueError(f"psis_batched: lp returned shape {_shape(v)}: expected ({K}, {S}) values")
    logr, lw, khat, ess, log_z, mean_is, cov_is, info = eng.psis_batched(mu, cv, X, v, moments=bool(moments))
    return _result(eng, as_torch, S, 2, khat, ess, log_z, lw, logr, X, mean_is, cov_is, info)


def psis_weights_batched(log_ratios, *, as_torch=False, engine=None):
    """The PSIS stage alone on the caller's own log ratios (K, S), 5 <= S <= 4096, one launch (gsmvi_psis_weights_batched_f64):
    returns a ``PSISBatchedResult`` whose ``samples``, ``mean`` and ``cov`` are None.  A shape that is not (K, S) or S out of
    bounds raises ValueError before any device work."""
    sh = _shape(log_ratios)
    if len(sh) != 2 or sh[0] < 1:
        raise ValueError(f"psis_weights_batched: log_ratios must be (K, S), got {sh}")
    K, S = sh
    if not MIN_DRAWS <= S <= MAX_DRAWS:
        raise ValueError(f"psis_weights_batched: S = {S} is outside {MIN_DRAWS} <= S <= {MAX_DRAWS}")
    if engine is None:
        from .engine import get_engine
        engine = get_engine()
    eng = engine
    logr = eng.asarray(log_ratios)
    lw, khat, ess, log_z, info = eng.psis_weights_batched(logr)
    return _result(eng, as_torch, S, 1, khat, ess, log_z, lw, logr, None, None, None, info)


@dataclass
class LOOBatchedResult:
    """What ``psis_loo_batched`` returns (numpy arrays, or the engine's tensors with ``as_torch``).  Pointwise, (K, N) each:
    ``elpd_i`` the leave-one-out log predictive density of observation i, ``lpd_i`` the importance-corrected in-sample density,
    ``khat`` and ``ess`` of the leave-one-out ratios, ``info``: 0, -1 = non-finite ratios (the row's outputs are NaN), -2 = tail
    too short (khat = +inf, plain weights), -3 = not a valid row (NaN).  Per problem, (K,) each: ``elpd_loo`` = the sum of
    ``elpd_i`` over the valid rows, ``p_loo`` = the sum of ``lpd_i - elpd_i`` (the effective number of parameters), ``se`` =
    sqrt(n_k var(elpd_i)) with the unbiased variance over the n_k valid rows (NaN for n_k < 2), ``n_bad`` = the valid rows with
    ``info`` != 0 or ``khat`` >= ``threshold``, ``ok`` = ``psis.ok`` & (``n_bad`` == 0).  ``loglik`` (K, N, S) the pointwise log
    likelihood of every draw, or None; ``psis`` the problem-level ``PSISBatchedResult`` (device tensors: hand it back as
    ``psis=`` to reuse its draws); ``threshold`` = min(1 - 1 / log10(S), 0.7); ``nlaunch`` the kernel launches made.
    From ``psis_loo_shared_batched`` with observation weights v_ki the valid rows are those with v_ki > 0, ``elpd_i`` and ``lpd_i``
    are densities of ONE unit observation (unweighted), and the sums are weighted: with c_i = v_ki ``elpd_i``, ``elpd_loo`` = sum
    c_i, ``p_loo`` = sum v_ki (``lpd_i`` - ``elpd_i``), ``se`` = sqrt(n_k var(c_i)) over the n_k valid rows."""
    elpd_loo: object
    p_loo: object
    se: object
    elpd_i: object
    lpd_i: object
    khat: object
    ess: object
    info: object
    n_bad: object
    ok: object
    loglik: object
    psis: object
    threshold: float
    nlaunch: int


def _reusable(psis, K, D, eng, fn="psis_loo_batched"):
    """(X, logr, lw) of a ``PSISBatchedResult`` that still holds its device tensors, else ValueError naming what is missing (a
    field that is None, or a host copy where the engine works on device tensors)"""
    import torch
    on_device = isinstance(getattr(eng, "device", None), torch.device)
    if not isinstance(psis, PSISBatchedResult):
        raise ValueError(f"{fn}: psis must be a PSISBatchedResult of psis_batched(..., as_torch=True), got {type(psis).__name__}")
    parts = (("samples", psis.samples), ("log_ratios", psis.log_ratios), ("log_weights", psis.log_weights))
    missing = [n for n, t in parts if t is None or (on_device and not isinstance(t, torch.Tensor))]
    if missing:
        raise ValueError(f"{fn}: psis holds no device tensor for {', '.join(missing)}: give the result of "
                         "psis_batched(..., as_torch=True)")
    X, logr, lw = (t for _, t in parts)
    if len(_shape(X)) != 3 or _shape(X)[0] != K or _shape(X)[2] != D:
        raise ValueError(f"{fn}: psis.samples must be ({K}, S, {D}), got {_shape(X)}")
    S = _shape(X)[1]
    if _shape(logr) != (K, S) or _shape(lw) != (K, S):
        raise ValueError(f"{fn}: psis.log_ratios and psis.log_weights must be {(K, S)}, got {_shape(logr)} and {_shape(lw)}")
    return X, logr, lw


def _loo_result(eng, target, psis, S, nlaunch, as_torch, elpd_i, lpd_i, khat, ess, info, loglik, weights=None, by_weights=False):
    """The ``LOOBatchedResult`` of the pointwise outputs of a leave-one-out launch (``psis_loo_batched``,
    ``psis_loo_softmax_batched``, ``psis_loo_negbin_batched``, ``psis_loo_ordinal_batched`` and ``psis_loo_shared_batched``): the per-problem summaries are torch
    reductions under the mask of the valid rows (a stand-in engine's numpy arrays: on the host).  The valid rows are the first
    ``target.counts[k]``, or with ``by_weights`` (the shared design, which has no counts) the rows whose weight in ``weights``
    (K, N) is > 0, every row for None; the sums are then weighted: c_i = v_i elpd_i, p_loo = sum v_i (lpd_i - elpd_i).  Weights
    of 0 and 1 give the unweighted sums bit for bit."""
    import torch
    K, N = target.K, target.N
    thr = khat_threshold(S)
    ten = lambda a: a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))      # noqa: E731
    e, lp_, kh, inf = ten(elpd_i), ten(lpd_i), ten(khat), ten(info)
    c, d = e, lp_ - e
    if by_weights and weights is not None:
        v = ten(weights).to(e.device)
        mask = v > 0.0
        nk = mask.sum(1)
        c, d = v * c, v * d
    elif by_weights:
        nk = torch.full((K,), N, device=e.device)
        mask = torch.ones((K, N), dtype=torch.bool, device=e.device)
    else:
        nk = ten(target.counts).to(e.device).clamp(0, N) if target.counts is not None else torch.full((K,), N, device=e.device)
        mask = torch.arange(N, device=e.device)[None, :] < nk[:, None]
    zero = torch.zeros((), dtype=e.dtype, device=e.device)
    nf = nk.to(e.dtype)
    elpd_loo = torch.where(mask, c, zero).sum(1)
    p_loo = torch.where(mask, d, zero).sum(1)
    dev = torch.where(mask, c - (elpd_loo / nf)[:, None], zero)
    se = torch.sqrt(nf * ((dev * dev).sum(1) / (nf - 1.0)))
    se = torch.where(nk >= 2, se, torch.full_like(se, float("nan")))
    n_bad = (mask & ((inf != 0) | (kh >= thr))).sum(1)
    ok = ten(psis.ok).to(e.device) & (n_bad == 0)
    out = dict(elpd_loo=elpd_loo, p_loo=p_loo, se=se, elpd_i=elpd_i, lpd_i=lpd_i, khat=khat, ess=ess, info=info, n_bad=n_bad,
               ok=ok, loglik=loglik)
    if not as_torch:
        out = {n: None if t is None else np.asarray(eng.to_numpy(t)) for n, t in out.items()}
        out["info"] = out["info"].astype(np.int64)
    return LOOBatchedResult(psis=psis, threshold=thr, nlaunch=nlaunch, **out)


def _loo_draws(fn, target, mean, cov, keys, num_draws, call, psis, engine):
    """The argument checks and the problem-level run shared by the five leave-one-out functions: (eng, psis, nlaunch, X, logr, lw)"""
    K, D = target.K, target.D
    if _shape(mean) != (K, D):
        raise ValueError(f"{fn}: mean must be (K, D) = {(K, D)} of the target, got {_shape(mean)}")
    if _shape(cov) != (K, D, D):
        raise ValueError(f"{fn}: cov must be {(K, D, D)}, got {_shape(cov)}")
    keys_l = [int(k) for k in np.asarray(list(keys) if isinstance(keys, (list, tuple, range)) else _to_numpy(keys)).reshape(-1)]
    if len(keys_l) != K:
        raise ValueError(f"{fn}: {len(keys_l)} keys for K = {K} problems")
    eng = engine if engine is not None else target.engine
    if psis is None:
        S = int(num_draws)
        if S != num_draws or not MIN_DRAWS <= S <= MAX_DRAWS:
            raise ValueError(f"{fn}: num_draws = {num_draws} is outside {MIN_DRAWS} <= num_draws <= {MAX_DRAWS}")
        psis = psis_batched(target.lp, mean, cov, keys_l, S, call=call, moments=False, as_torch=True, engine=eng)
        nlaunch = psis.nlaunch + 1
    else:
        nlaunch = 1
    X, logr, lw = _reusable(psis, K, D, eng, fn)
    return eng, psis, nlaunch, X, logr, lw


def psis_loo_batched(target, mean, cov, keys, num_draws=1024, *, call=0, psis=None, pointwise_loglik=False, as_torch=False,
                     engine=None):
    """PSIS leave-one-out of K fitted GLM posteriors q_k = N(mean_k, cov_k): returns a ``LOOBatchedResult``.

    ``target`` is the ``BatchedGLMTarget`` or ``BatchedLogisticTarget`` the posteriors were fitted to (its A, y, offset, counts
    and noise precision are the model; anything else raises TypeError); mean (K, D), cov (K, D, D) and ``keys`` are
    ``psis_batched``'s.  Without ``psis`` it first runs ``psis_batched(target.lp, mean, cov, keys, num_draws, call=call,
    moments=False, as_torch=True)`` (two launches and one call of ``target.lp``); with ``psis``, the result of such a call, its
    draws, ratios and weights are reused (``num_draws`` and ``call`` are then not used).  Then one launch,
    gsmvi_psis_loo_batched_f64: the pointwise log likelihood l_si of every draw on the fp64 MFMA, and per observation the PSIS
    stage on the ratios logr_s - l_si and the two log-sum-exps (the definition is in include/gsmvi_hip.h).  The per-problem
    sums are torch reductions of the (K, N) outputs under the mask of ``target.counts``.  ``pointwise_loglik`` also returns the
    (K, N, S) block l_si (K * N * S * 8 bytes).  mean and cov are only read.
    A mean that is not (K, D) of the target, a cov that is not (K, D, D), ``num_draws`` outside 5..4096, keys of another length
    than K, or a ``psis`` that is not a ``PSISBatchedResult`` holding device tensors of the right shapes raise ValueError before
    any device work."""
    from .targets import BatchedGLMTarget, SharedDesignGLMTarget
    if not isinstance(target, BatchedGLMTarget):
        hint = "; call psis_loo_shared_batched(target, ...) for it" if isinstance(target, SharedDesignGLMTarget) else ""
        raise TypeError(f"psis_loo_batched: target must be a BatchedGLMTarget or BatchedLogisticTarget, got "
                        f"{type(target).__name__}{hint}")
    eng, psis, nlaunch, X, logr, lw = _loo_draws("psis_loo_batched", target, mean, cov, keys, num_draws, call, psis, engine)
    S = _shape(X)[1]
    elpd_i, lpd_i, khat, ess, info, loglik = eng.psis_loo_batched(
        X, logr, lw, target.A, target.y, target.family, offset=target.offset, counts=target.counts,
        noise_prec=target.noise_precision, pointwise_loglik=bool(pointwise_loglik))
    return _loo_result(eng, target, psis, S, nlaunch, as_torch, elpd_i, lpd_i, khat, ess, info, loglik)


def psis_loo_softmax_batched(target, mean, cov, keys, num_draws=1024, *, call=0, psis=None, pointwise_loglik=False, as_torch=False,
                             engine=None):
    """PSIS leave-one-out of K fitted multinomial logit posteriors q_k = N(mean_k, cov_k): returns a ``LOOBatchedResult``, the
    twin of ``psis_loo_batched`` for the class-coupled likelihood.

    ``target`` is the ``BatchedSoftmaxTarget`` the posteriors were fitted to (its A, labels, number of classes and counts are the
    model; anything else raises TypeError); mean (K, D), D = (C - 1) P, cov (K, D, D) and ``keys`` are ``psis_batched``'s.
    Without ``psis`` it first runs ``psis_batched(target.lp, mean, cov, keys, num_draws, call=call, moments=False,
    as_torch=True)`` (two launches and one call of ``target.lp``); with ``psis``, the result of such a call, its draws, ratios
    and weights are reused (``num_draws`` and ``call`` are then not used).  Then one launch,
    gsmvi_psis_loo_softmax_batched_f64: per class the linear predictors of every draw on the fp64 MFMA, the pointwise log
    likelihood l_si = eta_y - m - log sum_c exp(eta_c - m), and per observation the PSIS stage on the ratios logr_s - l_si and the
    two log-sum-exps (the definition is in include/gsmvi_hip.h).  No (K, N, S) block of log likelihoods and no (K, S, N, C) block
    of probabilities is formed unless ``pointwise_loglik`` asks for the first (K * N * S * 8 bytes).  The per-problem sums are
    those of ``psis_loo_batched``.  mean and cov are only read.
    A mean that is not (K, D) of the target, a cov that is not (K, D, D), ``num_draws`` outside 5..4096, keys of another length
    than K, or a ``psis`` that is not a ``PSISBatchedResult`` holding device tensors of the right shapes raise ValueError before
    any device work."""
    from .targets import BatchedSoftmaxTarget
    fn = "psis_loo_softmax_batched"
    if not isinstance(target, BatchedSoftmaxTarget):
        raise TypeError(f"{fn}: target must be a BatchedSoftmaxTarget, got {type(target).__name__}")
    eng, psis, nlaunch, X, logr, lw = _loo_draws(fn, target, mean, cov, keys, num_draws, call, psis, engine)
    S = _shape(X)[1]
    elpd_i, lpd_i, khat, ess, info, loglik = eng.psis_loo_softmax_batched(
        X, logr, lw, target.A, target.y, target.C, counts=target.counts, pointwise_loglik=bool(pointwise_loglik))
    return _loo_result(eng, target, psis, S, nlaunch, as_torch, elpd_i, lpd_i, khat, ess, info, loglik)


def psis_loo_negbin_batched(target, mean, cov, keys, num_draws=1024, *, call=0, psis=None, pointwise_loglik=False, as_torch=False,
                            engine=None):
    """PSIS leave-one-out of K fitted negative binomial posteriors q_k = N(mean_k, cov_k) over (beta, log size): returns a
    ``LOOBatchedResult``, the twin of ``psis_loo_batched`` for the likelihood whose draws carry a shape parameter.

    ``target`` is the ``BatchedNegBinomialTarget`` the posteriors were fitted to (its A, y, offset and counts are the model;
    anything else raises TypeError); mean (K, D), D = P + 1, cov (K, D, D) and ``keys`` are ``psis_batched``'s.  Without ``psis``
    it first runs ``psis_batched(target.lp, mean, cov, keys, num_draws, call=call, moments=False, as_torch=True)`` (two launches
    and one call of ``target.lp``); with ``psis``, the result of such a call, its draws, ratios and weights are reused
    (``num_draws`` and ``call`` are then not used).  Then one launch, gsmvi_psis_loo_negbin_batched_f64: the linear predictors of
    every draw on the fp64 MFMA, the pointwise log likelihood l_si = t(eta_si, theta_s, y_i) - lgamma(y_i + 1) through the
    target's own link, and per observation the PSIS stage on the ratios logr_s - l_si and the two log-sum-exps (the definition is
    in include/gsmvi_hip.h).  The term -lgamma(y + 1), which ``target.lp`` drops, is INCLUDED: l_si is the normalised log
    probability of the count, as in ``psis_loo_batched`` of a poisson ``BatchedGLMTarget``, so ``elpd_loo`` of the two models are
    on one scale and their difference says whether the shape parameter earns its place.  No (K, N, S) block of log likelihoods is
    formed unless ``pointwise_loglik`` asks for it (K * N * S * 8 bytes).  The per-problem sums are those of
    ``psis_loo_batched``.  mean and cov are only read.
    A mean that is not (K, D) of the target, a cov that is not (K, D, D), ``num_draws`` outside 5..4096, keys of another length
    than K, or a ``psis`` that is not a ``PSISBatchedResult`` holding device tensors of the right shapes raise ValueError before
    any device work."""
    from .targets import BatchedNegBinomialTarget
    fn = "psis_loo_negbin_batched"
    if not isinstance(target, BatchedNegBinomialTarget):
        raise TypeError(f"{fn}: target must be a BatchedNegBinomialTarget, got {type(target).__name__}")
    eng, psis, nlaunch, X, logr, lw = _loo_draws(fn, target, mean, cov, keys, num_draws, call, psis, engine)
    S = _shape(X)[1]
    elpd_i, lpd_i, khat, ess, info, loglik = eng.psis_loo_negbin_batched(
        X, logr, lw, target.A, target.y, offset=target.offset, counts=target.counts, pointwise_loglik=bool(pointwise_loglik))
    return _loo_result(eng, target, psis, S, nlaunch, as_torch, elpd_i, lpd_i, khat, ess, info, loglik)


def psis_loo_ordinal_batched(target, mean, cov, keys, num_draws=1024, *, call=0, psis=None, pointwise_loglik=False, as_torch=False,
                             engine=None):
    """PSIS leave-one-out of K fitted cumulative-logit (proportional odds) posteriors q_k = N(mean_k, cov_k) over (beta, delta):
    returns a ``LOOBatchedResult``, the twin of ``psis_loo_batched`` for the likelihood whose draws carry the cutpoints.

    ``target`` is the ``BatchedOrdinalTarget`` the posteriors were fitted to (its A, labels, number of classes, offset and counts
    are the model; anything else raises TypeError); mean (K, D), D = P + C - 1, cov (K, D, D) and ``keys`` are ``psis_batched``'s.
    Without ``psis`` it first runs ``psis_batched(target.lp, mean, cov, keys, num_draws, call=call, moments=False,
    as_torch=True)`` (two launches and one call of ``target.lp``); with ``psis``, the result of such a call, its draws, ratios
    and weights are reused (``num_draws`` and ``call`` are then not used).  Then one launch, gsmvi_psis_loo_ordinal_batched_f64:
    the linear predictors of every draw on the fp64 MFMA, the cutpoints of every draw, the pointwise log likelihood l_si =
    log P(y_i | eta_si, cut_s) through the target's own link (no two probabilities are subtracted), and per observation the PSIS
    stage on the ratios logr_s - l_si and the two log-sum-exps (the definition is in include/gsmvi_hip.h).  l_si is the log of a
    normalised categorical probability and no constant is added, so ``elpd_loo`` is on the scale of
    ``psis_loo_softmax_batched`` on the same labels -- does proportional odds beat a multinomial logit? -- and of another
    ordinal fit -- does a covariate earn its place?  No (K, N, S) block of log likelihoods is formed unless
    ``pointwise_loglik`` asks for it (K * N * S * 8 bytes).  The per-problem sums are those of ``psis_loo_batched``.  mean and
    cov are only read.
    A mean that is not (K, D) of the target, a cov that is not (K, D, D), ``num_draws`` outside 5..4096, keys of another length
    than K, or a ``psis`` that is not a ``PSISBatchedResult`` holding device tensors of the right shapes raise ValueError before
    any device work."""
    from .targets import BatchedOrdinalTarget
    fn = "psis_loo_ordinal_batched"
    if not isinstance(target, BatchedOrdinalTarget):
        raise TypeError(f"{fn}: target must be a BatchedOrdinalTarget, got {type(target).__name__}")
    eng, psis, nlaunch, X, logr, lw = _loo_draws(fn, target, mean, cov, keys, num_draws, call, psis, engine)
    S = _shape(X)[1]
    elpd_i, lpd_i, khat, ess, info, loglik = eng.psis_loo_ordinal_batched(
        X, logr, lw, target.A, target.y, target.C, offset=target.offset, counts=target.counts,
        pointwise_loglik=bool(pointwise_loglik))
    return _loo_result(eng, target, psis, S, nlaunch, as_torch, elpd_i, lpd_i, khat, ess, info, loglik)


def psis_loo_shared_batched(target, mean, cov, keys, num_draws=1024, *, call=0, psis=None, pointwise_loglik=False, as_torch=False,
                            engine=None):
    """PSIS leave-one-out of K fitted GLM posteriors q_k = N(mean_k, cov_k) on ONE design matrix: returns a ``LOOBatchedResult``,
    the twin of ``psis_loo_batched`` for ``SharedDesignGLMTarget`` -- which lambda of a sweep, which response, which bootstrap
    replicate predicts best -- with no copy of A per problem and the observation weights honoured.

    ``target`` is the ``SharedDesignGLMTarget`` the posteriors were fitted to (its A, y, offset, weights and noise precision are
    the model; anything else raises TypeError); mean (K, D), cov (K, D, D) and ``keys`` are ``psis_batched``'s.  Without ``psis``
    it first runs ``psis_batched(target.lp, mean, cov, keys, num_draws, call=call, moments=False, as_torch=True)`` (two launches
    and one call of ``target.lp``, the weighted density); with ``psis``, the result of such a call, its draws, ratios and weights
    are reused (``num_draws`` and ``call`` are then not used).  Then one launch, gsmvi_psis_loo_shared_batched_f64 (the
    definition is in include/gsmvi_hip.h).  Row i of problem k is valid iff its weight v_ki is > 0 (no weights: every row): any
    subset of the rows, and what y and the offset hold at the others is never looked at; those rows get ``info`` = -3 and NaN.
    The pointwise log likelihood l_si is that of ONE unit observation at row i, normalised as ``psis_loo_batched`` does and
    unweighted; leaving row i out removes its whole weighted term, so the PSIS stage runs on logr_s - v_ki l_si.  The sums are
    weighted, over the n_k valid rows with c_i = v_ki elpd_i: ``elpd_loo`` = sum c_i, ``p_loo`` = sum v_ki (lpd_i - elpd_i),
    ``se`` = sqrt(n_k var(c_i)).  With weights None, all ones, or 0 / 1 these are ``psis_loo_batched``'s numbers on the replicated
    design, bit for bit.  A row of weight 0 is NOT scored as a held-out row: K-fold cross-validation through the weights is not
    what this computes.  ``pointwise_loglik`` also returns the (K, N, S) block l_si.  mean and cov are only read.
    A mean that is not (K, D) of the target, a cov that is not (K, D, D), ``num_draws`` outside 5..4096, keys of another length
    than K, or a ``psis`` that is not a ``PSISBatchedResult`` holding device tensors of the right shapes raise ValueError before
    any device work."""
    from .targets import SharedDesignGLMTarget
    fn = "psis_loo_shared_batched"
    if not isinstance(target, SharedDesignGLMTarget):
        raise TypeError(f"{fn}: target must be a SharedDesignGLMTarget, got {type(target).__name__}")
    eng, psis, nlaunch, X, logr, lw = _loo_draws(fn, target, mean, cov, keys, num_draws, call, psis, engine)
    S = _shape(X)[1]
    elpd_i, lpd_i, khat, ess, info, loglik = eng.psis_loo_shared_batched(
        X, logr, lw, target.A, target.y, target.family, offset=target.offset, weights=target.weights,
        noise_prec=target.noise_precision, pointwise_loglik=bool(pointwise_loglik))
    return _loo_result(eng, target, psis, S, nlaunch, as_torch, elpd_i, lpd_i, khat, ess, info, loglik, weights=target.weights,
                       by_weights=True)
