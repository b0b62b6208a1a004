"""Score providers for the fit drivers.

``GaussianTarget`` is the benchmark target of the reference's examples
(examples/example_gsm_numpy.py:8-31: ``lp_g(x) = -icov (x - mean)``) evaluated by the HIP panel
kernel.  ``device_score`` marks a user callable as taking/returning CUDA tensors;
``score_from_logp`` is the sum-then-autograd helper matching the JAX examples
(examples/example_gsm.py:34-35: ``lp_g = jit(grad(lambda x: sum(lp(x))))``).
``BatchedLogisticTarget`` is the first non-Gaussian device target of the batched fits: K Bayesian logistic
regressions, score and log-density from one HIP launch.  ``BatchedGLMTarget`` is the same launch for a family of generalised
linear models: Poisson, probit, Gaussian and logistic, with offsets; the logistic class is its ``family="logistic"`` case.  They have ``predict``: the posterior predictive of the
fitted Gaussians on new rows (``GLMPrediction``), one HIP launch.  ``BatchedSoftmaxTarget`` is the multiclass response: K
multinomial logit regressions (C classes, C - 1 linear predictors per row), a launch and a class of its own.

    target                    response                        entry point                    laplace / predict / loo
    BatchedGaussianTarget     (a Gaussian density)            gsmvi_gaussian_score_batched_f64   no
    BatchedLogisticTarget     y in [0, 1]                     gsmvi_logistic_batched_f64         yes
    BatchedGLMTarget          poisson, probit, gaussian, ...  gsmvi_glm_batched_f64              yes
    SharedDesignGLMTarget     the same four, ONE A (N, D),    gsmvi_glm_shared_batched_f64       laplace_init_shared_batched and
                              observation weights                                                neg_hessian_shared_batched (free
                                                                                                 functions); predict, loo: no (not a
                                                                                                 BatchedGLMTarget: the isinstance
                                                                                                 checks refuse it)
    BatchedNegBinomialTarget  counts y >= 0, a fitted size    gsmvi_negbin_batched_f64           no (not a BatchedGLMTarget: the Hessian
                              (x = (beta, log r))                                                has a 2 x 2 block per row)
    BatchedOrdinalTarget      ordered labels in 0 .. C - 1,   gsmvi_ordinal_batched_f64          laplace_init_ordinal_batched and
                              x = (beta, C - 1 cutpoints)                                        neg_hessian_ordinal_batched; predict, loo:
                                                                                                 no method (TypeError from the others):
                                                                                                 predict_ordinal_batched,
                                                                                                 psis_loo_ordinal_batched
    BatchedSoftmaxTarget      integer labels in 0 .. C - 1    gsmvi_softmax_batched_f64          laplace_init_softmax_batched and
                                                                                                 neg_hessian; predict, loo: no (TypeError):
                                                                                                 predict_softmax_batched,
                                                                                                 psis_loo_softmax_batched

``predict_softmax_batched`` is the softmax target's posterior predictive (``SoftmaxPrediction``): class probabilities and the
held-out score of new rows from draws of the fitted Gaussians, one HIP launch after the draws.  ``predict_ordinal_batched`` is
the same for the ordinal target (``OrdinalPrediction``): the probabilities of the C ordered classes, their first maximum and their
median class, and the held-out score, one HIP launch after the draws.
"""
from dataclasses import dataclass
from typing import Any

import numpy as np
import torch

from .engine import get_engine


def device_score(fn=None, *, graph_safe=False):
    """Decorator: ``fn`` maps a float64 CUDA tensor (B,D) to a float64 CUDA tensor (B,D).
    ``@device_score(graph_safe=True)`` additionally promises that a call is capturable into a hipGraph (only stream-ordered
    device work on the current stream, no host synchronisation, deterministic launch sequence): the factor-form fit then
    replays blocks of iterations as one graph instead of issuing every launch from Python."""
    def mark(f):
        f.device_native = True
        f.graph_safe = bool(graph_safe)
        return f
    return mark(fn) if fn is not None else mark


def score_from_logp(logp, graph_safe=False):
    """Score via torch autograd of a *summed* log-probability (examples/example_gsm.py:34-35: jit(grad(sum lp))).
    ``graph_safe=True`` promises that ``logp`` is capturable (stream-ordered torch ops of fixed shapes, no host
    synchronisation, no data-dependent control flow): the factor-form fit then records forward AND backward of every
    iteration of a block into its hipGraph -- the ~12 torch dispatches per score evaluation (90 - 160 us of host time at
    D = 1024) replay as part of one graph launch, which is what jit does for the reference's JAX score."""
    def lp_g(x):
        xg = x.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            total = logp(xg).sum()
            (g,) = torch.autograd.grad(total, xg)
        return g.detach()
    lp_g.device_native = True
    lp_g.graph_safe = bool(graph_safe)
    return lp_g


class GaussianTarget:
    """N(mean, cov) with device-resident precision matrix; ``lp`` / ``lp_g`` follow
    examples/example_gsm_numpy.py:17-29."""

    def __init__(self, mean, cov=None, precision=None, engine=None):
        self.engine = engine if engine is not None else get_engine()
        eng = self.engine
        if precision is None:
            precision = np.linalg.inv(np.asarray(cov, dtype=np.float64))
        P = np.asarray(precision, dtype=np.float64)
        self.mean = eng.asarray(np.asarray(mean, dtype=np.float64))
        self.P = eng.asarray(0.5 * (P + P.T))
        self.D = int(self.mean.shape[0])

        def lp_g(x, out=None):
            return eng.gaussian_score(x, self.mean, self.P, out=out)
        lp_g.device_native = True
        lp_g.graph_safe = True          # one capturable kernel launch, no allocation when `out` is given, no host work

        def padded(Dp):
            """the score of the same target with (Dp - D) inert coordinates appended (zero rows / columns in the precision
            matrix: g' = [g, 0] for x' = [x, anything]) -- what the fit loops use for odd D (gsm-vi_amd/_oddpad.py)"""
            if getattr(self, "_padded", None) is None or self._padded[0] != Dp:
                mp, Pp = eng.zeros(Dp), eng.zeros(Dp, Dp)
                mp[:self.D] = self.mean
                Pp[:self.D, :self.D] = self.P

                def lp_g_p(x, out=None):
                    return eng.gaussian_score(x, mp, Pp, out=out)
                lp_g_p.device_native = True
                lp_g_p.graph_safe = True
                self._padded = (Dp, lp_g_p)
            return self._padded[1]
        lp_g.padded = padded
        self.lp_g = lp_g

    def lp(self, x):
        """sum_b -1/2 (m - x_b)^T P (m - x_b); monitor-only, so plain torch is fine here."""
        x = self.engine.asarray(x)
        r = self.mean[None, :] - x
        return -0.5 * torch.einsum("bi,ij,bj->", r, self.P, r)


class BatchedGaussianTarget:
    """K Gaussian targets N(means[k], cov[k]) of one dimension D for ``GSMBatch``: ``lp_g`` maps (K,B,D) samples to (K,B,D)
    scores g_kb = -P_k (x_kb - m_k) with the batched score kernel (gsmvi_gaussian_score_batched_f64; one capturable launch,
    marked ``graph_safe``); ``lp`` is the plain batched log-density, one sum over the batch per problem (example_gsm_numpy.py:17-29
    per target).  Give ``cov`` (K,D,D) or ``precision`` (K,D,D)."""

    def __init__(self, means, cov=None, precision=None, engine=None):
        self.engine = engine if engine is not None else get_engine()
        eng = self.engine
        m = np.asarray(means, dtype=np.float64)
        assert m.ndim == 2, "means: expected shape (K, D)"
        if precision is None:
            assert cov is not None, "give cov or precision"
            precision = np.linalg.inv(np.asarray(cov, dtype=np.float64))
        P = np.asarray(precision, dtype=np.float64)
        assert P.shape == (m.shape[0], m.shape[1], m.shape[1]), "precision / cov: expected shape (K, D, D)"
        self.K, self.D = int(m.shape[0]), int(m.shape[1])
        self.mean = eng.asarray(m)
        self.P = eng.asarray(0.5 * (P + np.swapaxes(P, 1, 2)))

        def lp_g(x, out=None):
            return eng.gaussian_score_batched(x, self.mean, self.P, out=out)
        lp_g.device_native = True
        lp_g.graph_safe = True          # one capturable kernel launch, no allocation when `out` is given, no host work
        self.lp_g = lp_g

    def lp(self, x):
        """(K,) sums over the batch of -1/2 (m_k - x_kb)^T P_k (m_k - x_kb); plain torch (off the hot path)."""
        x = self.engine.asarray(x)
        r = self.mean[:, None, :] - x
        return -0.5 * torch.einsum("kbi,kij,kbj->k", r, self.P, r)

    def lp_rows(self, x):
        """(K, rows) values -1/2 (m_k - x_kr)^T P_k (m_k - x_kr) at the rows of x (K, rows, D): what ``psis_batched`` needs (``lp``
        returns their sums); plain torch (off the hot path)."""
        x = self.engine.asarray(x)
        r = self.mean[:, None, :] - x
        return -0.5 * torch.einsum("kbi,kij,kbj->kb", r, self.P, r)


def _host_array(x):
    """numpy view or copy of a host array or of a tensor on any device (validation only)"""
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _shape(x):
    """the shape of an array, a tensor or nested lists as a tuple of ints"""
    return tuple(int(n) for n in x.shape) if hasattr(x, "shape") else np.shape(x)


def _check_per_problem(x, name, K, positive=False, fixed=None):
    """``x``, a number or K values, as a host float64 array: finite and >= 0, or (``positive``) > 0 with the offending problems
    listed; ``fixed``: the message for an ``x`` that must stay at 1.0 and does not; else ValueError"""
    v = np.asarray(_host_array(x), dtype=np.float64)
    if v.shape not in ((), (K,)):
        raise ValueError(f"{name}: expected a number or {K} values, got shape {v.shape}")
    if fixed is not None and not (v == 1.0).all():
        raise ValueError(f"{name}: {fixed}")
    good = np.isfinite(v) & (v > 0.0 if positive else v >= 0.0)
    if not good.all():
        where = f" (problems {np.flatnonzero(~good).tolist()})" if positive and v.shape != () else ""
        raise ValueError(f"{name}: expected finite values {'> 0' if positive else '>= 0'}{where}")
    return v


def _check_counts(counts, K, N, rows="N"):
    """``counts`` of K problems of N rows each as a host integer array (None stays None), else ValueError"""
    if counts is None:
        return None
    cnt = np.asarray(_host_array(counts))
    if cnt.shape != (K,) or not np.issubdtype(cnt.dtype, np.integer):
        raise ValueError(f"counts: expected {K} integers, got shape {cnt.shape}, dtype {cnt.dtype}")
    if (cnt < 0).any() or (cnt > N).any():
        raise ValueError(f"counts: values outside 0 .. {rows} = {N} for problems {np.flatnonzero((cnt < 0) | (cnt > N)).tolist()}")
    return cnt


def _live_rows(cnt, N):
    """(K, N) or (1, N) mask of the rows that count"""
    return np.arange(N)[None, :] < (cnt[:, None] if cnt is not None else N)


def _check_responses(y, family, live, name_family=True):
    """the responses as a host float64 array, their range per family checked in the valid rows, else ValueError"""
    yh = np.asarray(_host_array(y), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        if family in ("logistic", "probit"):
            good, what = (yh >= 0.0) & (yh <= 1.0), "outside [0, 1] or non-finite"     # (a NaN fails both comparisons)
        elif family == "poisson":
            good, what = (yh >= 0.0) & np.isfinite(yh), "negative or non-finite"
        else:
            good, what = np.isfinite(yh), "non-finite"
    bad = live & ~good
    if bad.any():
        raise ValueError(f"y: values {what} in the valid rows of problems {np.flatnonzero(bad.any(1)).tolist()}"
                         + (f" (family {family!r})" if name_family else ""))
    return yh


def _check_offset(offset, K, N, live, rows="N"):
    """the offsets as a host float64 array (None stays None), shape and finiteness in the valid rows checked, else ValueError"""
    if offset is None:
        return None
    so = _shape(offset)
    if so != (K, N):
        raise ValueError(f"offset: expected shape (K, {rows}) = {(K, N)}, got {so}")
    oh = np.asarray(_host_array(offset), dtype=np.float64)
    bad = live & ~np.isfinite(oh)
    if bad.any():
        raise ValueError(f"offset: non-finite values in the valid rows of problems {np.flatnonzero(bad.any(1)).tolist()}")
    return oh


@dataclass
class GLMPrediction:
    """What ``BatchedGLMTarget.predict`` and ``BatchedLogisticTarget.predict`` return for M new rows of each of K problems under
    the fitted q_k = N(mean_k, cov_k): ``eta_mean`` = a . mean_k + o and ``eta_var`` = a^T cov_k a (the raw value: negative
    where cov_k is not positive semi-definite), the Gaussian of the linear predictor; ``mean`` = E[E[y | eta]], the predictive
    mean of the response; with ``y``, ``lpd`` = log E[p(y | eta)] (normalised) per row and ``elpd`` (K,), its sum over the valid
    rows: the held-out score by which fits of one model are compared.  (K, M) each; rows beyond ``counts[k]`` are NaN; ``lpd`` and
    ``elpd`` are None without ``y``.  numpy arrays or device tensors, as the call's ``mean`` was.
    [examples/example_gsm.py:34-35, the use of the fit; no reference twin]"""
    eta_mean: Any
    eta_var: Any
    mean: Any
    lpd: Any
    elpd: Any


class BatchedGLMTarget:
    """K Bayesian generalised linear models with their own data sets, for ``GSMBatch``, ``BaMBatch``, ``ADVIBatch``,
    ``BatchedKLMonitor`` and ``lbfgs_init_batched``: ``BatchedLogisticTarget``'s protocol for a family of links.  Problem k has
    the design matrix A[k] (N, D), responses y[k] (N,), an optional ``offset[k]`` (N,) added to the linear predictor (a log
    exposure, say), ``counts[k]`` <= N valid rows (None: all N; the rows beyond are ignored whatever they hold) and the prior
    N(0, I / lam_k), ``prior_precision`` = lam a float or K values, 0 = flat.  With eta = A[k] x + offset[k]:

        lp_k(x) = sum_n t(eta_n, y_n) - lam_k |x|^2 / 2,      grad lp_k(x) = sum_n r(eta_n, y_n) a_n - lam_k x

        family       y                  r                                          t
        "logistic"   in [0, 1]          y - sigmoid(eta)                           y eta - softplus(eta)
        "poisson"    >= 0, finite       y - exp(eta)                               y eta - exp(eta)      (log link; -log y! dropped)
        "probit"     in [0, 1]          y phi/Phi(eta) - (1 - y) phi/Phi(-eta)     y log Phi(eta) + (1 - y) log Phi(-eta)
        "gaussian"   finite             tau_k (y - eta)                            -tau_k (y - eta)^2 / 2   (identity link)

    evaluated by gsmvi_glm_batched_f64: what examples/example_gsm.py:34-35 gets from a model's log_prob and jit(grad(...)).
    ``noise_precision`` = tau, a float or K values > 0, is the Gaussian family's alone.  A Poisson point whose exp(eta) overflows
    in a valid row gets NaN outputs (the fits then revert that step).  numpy arrays or tensors in; everything is kept on the
    device as float64 / int32.  Arguments are validated on the host before any device work (ValueError naming the argument and
    the problems).

    ``lp_g(x, out=None)``: (K, B, D) -> (K, B, D) scores, ``device_native`` and ``graph_safe`` (one capturable launch, no
    allocation with ``out``).  ``lp(x)``: (K, rows, D) -> (K, rows) values; a device tensor or numpy.  ``lp_and_score(x)``:
    (scores, values) from one launch."""

    FAMILIES = ("logistic", "poisson", "probit", "gaussian")
    _y_names_family = True              # the ``y:`` messages end with the family

    def __init__(self, A, y, family, prior_precision=1.0, counts=None, offset=None, noise_precision=1.0, engine=None):
        if family not in self.FAMILIES:
            raise ValueError(f"family: expected one of {self.FAMILIES}, got {family!r}")
        sa = _shape(A)
        if len(sa) != 3 or min(sa) < 1:
            raise ValueError(f"A: expected shape (K, N, D) with K, N, D >= 1, got {sa}")
        K, N, D = sa
        if not 1 <= D <= 64:
            raise ValueError(f"A: D = {D} is outside 1 <= D <= 64")
        if _shape(y) != (K, N):
            raise ValueError(f"y: expected shape (K, N) = {(K, N)}, got {_shape(y)}")
        cnt = _check_counts(counts, K, N)
        live = _live_rows(cnt, N)
        yh = _check_responses(y, family, live, name_family=self._y_names_family)
        oh = _check_offset(offset, K, N, live)
        lam = _check_per_problem(prior_precision, "prior_precision", K)
        tau = _check_per_problem(noise_precision, "noise_precision", K, positive=True, fixed=None if family == "gaussian" else
                                 f"only family 'gaussian' has one (family {family!r}: leave it at 1.0)")
        self.engine = engine if engine is not None else get_engine()
        eng = self.engine
        self.family = family
        self.K, self.N, self.D = K, N, D
        self.A = eng.asarray(A.contiguous() if isinstance(A, torch.Tensor) else A)
        self.y = eng.asarray(yh)
        self.offset = eng.asarray(oh) if oh is not None else None
        self.counts = eng.batched_counts(cnt) if cnt is not None else None
        self.prior_precision = float(lam) if lam.shape == () else eng.batched_regs(lam)
        self.noise_precision = 1.0 if family != "gaussian" else float(tau) if tau.shape == () else eng.batched_regs(tau)

        def lp_g(x, out=None):
            return self._call(x, out=out, want="g")
        lp_g.device_native = True
        lp_g.graph_safe = True          # one capturable kernel launch, no allocation when `out` is given, no host work
        self.lp_g = lp_g

    def _call(self, x, **kw):
        return self.engine.glm_batched(x, self.A, self.y, self.family, offset=self.offset, counts=self.counts,
                                       prior_prec=self.prior_precision, noise_prec=self.noise_precision, **kw)

    def lp(self, x):
        """(K, rows) values lp_k(x_kr) at the rows of x (K, rows, D), a device tensor or numpy; one launch"""
        return self._call(self.engine.asarray(x), want="lp")

    def lp_and_score(self, x):
        """(scores (K, rows, D), values (K, rows)) from one launch"""
        return self._call(self.engine.asarray(x), want="both")

    def neg_hessian(self, x):
        """(K, D, D) negative Hessians A_k^T W A_k + lam_k I of lp_k at the rows of x (K, D), W = diag(-dr / d eta) (logistic:
        sigmoid (1 - sigmoid); poisson: exp(eta); probit: y hp (hp + eta) + (1 - y) hm (hm - eta) with hp = phi / Phi(eta), hm =
        phi / Phi(-eta); gaussian: tau_k), exactly symmetric; a device tensor or numpy; one launch"""
        eng = self.engine
        return eng.glm_hessian_batched(eng.asarray(x), self.A, self.y, self.family, offset=self.offset, counts=self.counts,
                                       prior_prec=self.prior_precision, noise_prec=self.noise_precision, want="h")

    def predict(self, mean, cov, A_new, offset=None, y=None, counts=None, nodes=32):
        """The posterior predictive of the K fitted problems on new rows: ``mean`` (K, D) and ``cov`` (K, D, D) are the
        fitted Gaussians (of GSMBatch, BaMBatch, ADVIBatch or ``laplace_init_batched``), ``A_new`` (K, M, D) the new rows,
        ``offset`` (K, M) their offsets (None: none, whether or not the target was built with one: the new rows are new data),
        ``y`` (K, M) their responses (None: no ``lpd`` / ``elpd``), ``counts`` (K,) the valid rows per problem (None: all M),
        ``nodes`` = Q the Gauss-Hermite nodes, 1 .. 64.  Returns a ``GLMPrediction``; numpy in gives numpy out, CUDA tensors in
        give tensors out.  ``y``, ``offset`` and ``counts`` are validated as the constructor validates its own (ValueError
        naming the argument and the problems), the shapes and ``nodes`` too, before any device work.  The quadrature is
        accurate for modest eta_var; the gaussian family is closed-form.  One launch."""
        K, D, family = self.K, self.D, self.family
        if isinstance(nodes, bool) or not isinstance(nodes, (int, np.integer)) or not 1 <= nodes <= 64:
            raise ValueError(f"nodes: expected an integer in 1 .. 64, got {nodes!r}")
        sa = _shape(A_new)
        if len(sa) != 3 or min(sa) < 1 or sa[0] != K or sa[2] != D:
            raise ValueError(f"A_new: expected shape (K, M, D) with K = {K}, D = {D} and M >= 1, got {sa}")
        M = sa[1]
        if _shape(mean) != (K, D):
            raise ValueError(f"mean: expected shape (K, D) = {(K, D)}, got {_shape(mean)}")
        if _shape(cov) != (K, D, D):
            raise ValueError(f"cov: expected shape (K, D, D) = {(K, D, D)}, got {_shape(cov)}")
        cnt = _check_counts(counts, K, M, rows="M")
        live = _live_rows(cnt, M)
        yh = None
        if y is not None:
            if _shape(y) != (K, M):
                raise ValueError(f"y: expected shape (K, M) = {(K, M)}, got {_shape(y)}")
            yh = _check_responses(y, family, live, name_family=self._y_names_family)
        oh = _check_offset(offset, K, M, live, rows="M")
        eng = self.engine
        as_tensor = isinstance(mean, torch.Tensor)
        dev = lambda x: eng.asarray(x.contiguous() if isinstance(x, torch.Tensor) else x)      # noqa: E731
        out = eng.glm_predict_batched(dev(mean), dev(cov), dev(A_new), family, offset=eng.asarray(oh) if oh is not None else None,
                                      y=eng.asarray(yh) if yh is not None else None,
                                      counts=eng.batched_counts(cnt) if cnt is not None else None,
                                      noise_prec=self.noise_precision, nodes=int(nodes))
        if not as_tensor:
            out = tuple(eng.to_numpy(t) if t is not None else None for t in out)
        return GLMPrediction(*out)

    def loo(self, mean, cov, keys, **kw):
        """``psis_loo_batched(self, mean, cov, keys, **kw)``: the PSIS leave-one-out density of every observation under the fitted
        q_k = N(mean_k, cov_k) (a ``LOOBatchedResult``: ``elpd_loo``, ``p_loo``, ``se`` per problem, the pointwise values and
        their khat)"""
        from .diagnostics import psis_loo_batched
        return psis_loo_batched(self, mean, cov, keys, **kw)


class BatchedLogisticTarget(BatchedGLMTarget):
    """K Bayesian logistic regressions with their own data sets, for ``GSMBatch``, ``BaMBatch``, ``ADVIBatch`` and
    ``BatchedKLMonitor``.  Problem k has the design matrix A[k] (N, D), labels y[k] (N,) in [0, 1] (soft labels allowed),
    ``counts[k]`` <= N valid rows (None: all N; the rows beyond are ignored whatever they hold) and the prior N(0, I / lam_k),
    ``prior_precision`` = lam a float or K values, 0 = flat.  With eta = A[k] x:

        lp_k(x)      = sum_n [ y_n eta_n - softplus(eta_n) ] - lam_k |x|^2 / 2          (unnormalised log posterior)
        grad lp_k(x) = sum_n ( y_n - sigmoid(eta_n) ) a_n - lam_k x

    in the overflow-safe forms (e = exp(-|eta|); sigmoid = 1 / (1 + e) for eta >= 0, e / (1 + e) otherwise; softplus =
    max(eta, 0) + log1p(e)), evaluated by gsmvi_logistic_batched_f64: what examples/example_gsm.py:34-35 gets from a model's
    log_prob and jit(grad(...)).  numpy arrays or tensors in; everything is kept on the device as float64 / int32.  Arguments
    are validated on the host before any device work (ValueError naming the argument).

    ``lp_g(x, out=None)``: (K, B, D) -> (K, B, D) scores, ``device_native`` and ``graph_safe`` (one capturable launch, no
    allocation with ``out``).  ``lp(x)``: (K, rows, D) -> (K, rows) values (what ADVIBatch's losses and BatchedKLMonitor sum per
    problem); a device tensor or numpy.  ``lp_and_score(x)``: (scores, values) from one launch."""

    _y_names_family = False

    def __init__(self, A, y, prior_precision=1.0, counts=None, engine=None):
        super().__init__(A, y, "logistic", prior_precision, counts, engine=engine)

    def _call(self, x, **kw):           # the logistic entry point of its own: the model is the GLM's with no offset and tau = 1
        return self.engine.logistic_batched(x, self.A, self.y, self.counts, self.prior_precision, **kw)


def _check_weights(weights, K, N, rows="N"):
    """the observation weights as a host float64 array (None stays None): shape (K, N), finite and >= 0, else ValueError
    (``rows`` names the row count in the message: "N", or "M" for the new rows of a predictive)"""
    if weights is None:
        return None
    sw = _shape(weights)
    if sw != (K, N):
        raise ValueError(f"weights: expected shape (K, {rows}) = {(K, N)}, got {sw}")
    wh = np.asarray(_host_array(weights), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        bad = ~(np.isfinite(wh) & (wh >= 0.0))
    if bad.any():
        raise ValueError(f"weights: negative or non-finite values for problems {np.flatnonzero(bad.any(1)).tolist()}")
    return wh


class SharedDesignGLMTarget:
    """K Bayesian generalised linear models on ONE design matrix, for ``GSMBatch``, ``BaMBatch``, ``ADVIBatch``,
    ``BatchedKLMonitor``, ``lbfgs_init_batched``, ``pathfinder_init_batched`` and ``psis_batched``: ``BatchedGLMTarget``'s protocol
    (attributes ``K``, ``N``, ``D``, ``family``; ``lp_g``, ``lp``, ``lp_and_score``) for the case where every problem has the same
    covariates -- many responses regressed on one design, a sweep over the prior or noise precision, the Bayesian or case
    bootstrap and tempered likelihoods.  ``A`` (N, D) is shared and held once; problem k has responses ``y[k]`` (N,), an optional
    ``offset[k]`` (N,) added to the linear predictor, optional observation weights ``weights[k]`` (N,), finite and >= 0, and the
    prior N(0, I / lam_k), ``prior_precision`` = lam a float or K values, 0 = flat.  With eta = A x + offset[k] and the link
    (r, t) of ``family`` (the table of ``BatchedGLMTarget``):

        lp_k(x) = sum_n w_kn t(eta_n, y_kn) - lam_k |x|^2 / 2,      grad lp_k(x) = sum_n w_kn r(eta_n, y_kn) a_n - lam_k x

    evaluated by gsmvi_glm_shared_batched_f64: what examples/example_gsm.py:34-35 gets from a model's log_prob and
    jit(grad(...)), with both sums on the fp64 MFMA and no copy of A per problem.  There is no ``counts``: a weight of 0 removes
    an observation, and ``y`` and ``offset`` are validated only where the weight is > 0 (elsewhere anything goes, NaN included).
    ``noise_precision`` = tau, a float or K values > 0, is the Gaussian family's alone.  A Poisson point whose exp(eta) overflows
    at an observation with w > 0 gets NaN outputs (the fits then revert that step).  numpy arrays or tensors in; everything is
    kept on the device as float64.  Arguments are validated on the host before any device work (ValueError naming the argument
    and the problems).

    ``lp_g(x, out=None)``: (K, B, D) -> (K, B, D) scores, ``device_native`` and ``graph_safe`` (one capturable launch, no
    allocation with ``out``).  ``lp(x)``: (K, rows, D) -> (K, rows) values.  ``lp_and_score(x)``: (scores, values) from one launch.
    Not a ``BatchedGLMTarget``: it has no ``neg_hessian``, ``predict`` or ``loo``, and ``laplace_init_batched``,
    ``psis_loo_batched`` refuse it.  Its negative Hessian is ``neg_hessian_shared_batched(target, x)``, its second-order start
    ``laplace_init_shared_batched(target, ...)`` and its PSIS leave-one-out ``psis_loo_shared_batched(target, mean, cov, keys,
    ...)`` (weighted sums over the rows of weight > 0) and its posterior predictive ``predict_shared_batched(target, mean, cov,
    A_new, ...)`` (one shared set of new rows with per-problem row weights: the held-out score of K-fold cross-validation
    through the weights), all on the shared design without a copy per problem."""

    FAMILIES = BatchedGLMTarget.FAMILIES

    def __init__(self, A, y, family, prior_precision=1.0, offset=None, weights=None, noise_precision=1.0, engine=None):
        if family not in self.FAMILIES:
            raise ValueError(f"family: expected one of {self.FAMILIES}, got {family!r}")
        sa = _shape(A)
        if len(sa) != 2 or min(sa) < 1:
            raise ValueError(f"A: expected shape (N, D) with N, D >= 1 (one design matrix for all problems), got {sa}")
        N, D = sa
        if not 1 <= D <= 64:
            raise ValueError(f"A: D = {D} is outside 1 <= D <= 64")
        sy = _shape(y)
        if len(sy) != 2 or sy[0] < 1 or sy[1] != N:
            raise ValueError(f"y: expected shape (K, N) with K >= 1 and N = {N}, got {sy}")
        K = sy[0]
        wh = _check_weights(weights, K, N)
        live = wh > 0.0 if wh is not None else np.ones((1, N), dtype=bool)
        yh = _check_responses(y, family, live)
        oh = _check_offset(offset, K, N, live)
        lam = _check_per_problem(prior_precision, "prior_precision", K)
        tau = _check_per_problem(noise_precision, "noise_precision", K, positive=True, fixed=None if family == "gaussian" else
                                 f"only family 'gaussian' has one (family {family!r}: leave it at 1.0)")
        self.engine = engine if engine is not None else get_engine()
        eng = self.engine
        self.family = family
        self.K, self.N, self.D = K, N, D
        self.A = eng.asarray(A.contiguous() if isinstance(A, torch.Tensor) else A)
        self.y = eng.asarray(yh)
        self.offset = eng.asarray(oh) if oh is not None else None
        self.weights = eng.asarray(wh) if wh is not None else None
        self.prior_precision = float(lam) if lam.shape == () else eng.batched_regs(lam)
        self.noise_precision = 1.0 if family != "gaussian" else float(tau) if tau.shape == () else eng.batched_regs(tau)

        def lp_g(x, out=None):
            return self._call(x, out=out, want="g")
        lp_g.device_native = True
        lp_g.graph_safe = True          # one capturable kernel launch, no allocation when `out` is given, no host work
        self.lp_g = lp_g

    def _call(self, x, **kw):
        return self.engine.glm_shared_batched(x, self.A, self.y, self.family, offset=self.offset, weights=self.weights,
                                              prior_prec=self.prior_precision, noise_prec=self.noise_precision, **kw)

    def lp(self, x):
        """(K, rows) values lp_k(x_kr) at the rows of x (K, rows, D), a device tensor or numpy; one launch"""
        return self._call(self.engine.asarray(x), want="lp")

    def lp_and_score(self, x):
        """(scores (K, rows, D), values (K, rows)) from one launch"""
        return self._call(self.engine.asarray(x), want="both")


def neg_hessian_shared_batched(target, x, *, engine=None):
    """(K, D, D) negative Hessians A^T diag(v_k w_k) A + lam_k I of lp_k of a ``SharedDesignGLMTarget`` at the rows of x (K, D):
    w = -dr / d eta of the family (the table of ``BatchedGLMTarget.neg_hessian``), v_k the observation weights; an observation
    whose weight is 0 contributes exactly nothing, whatever its y and offset hold.  Exactly symmetric; a device tensor or numpy
    in; one launch (gsmvi_glm_shared_hessian_batched_f64), no copy of the design per problem.  Anything that is not a
    ``SharedDesignGLMTarget`` raises TypeError."""
    if not isinstance(target, SharedDesignGLMTarget):
        raise TypeError(f"neg_hessian_shared_batched: target must be a SharedDesignGLMTarget, got {type(target).__name__}")
    K, D = target.K, target.D
    if _shape(x) != (K, D):
        raise ValueError(f"neg_hessian_shared_batched: x must be (K, D) = {(K, D)} of the target, got {_shape(x)}")
    eng = engine if engine is not None else target.engine
    return eng.glm_shared_hessian_batched(eng.asarray(x), target.A, target.y, target.family, offset=target.offset,
                                          weights=target.weights, prior_prec=target.prior_precision,
                                          noise_prec=target.noise_precision, want="h")


def predict_shared_batched(target, mean, cov, A_new, offset=None, y=None, weights=None, nodes=32, *, engine=None):
    """The posterior predictive of the K fitted problems of a ``SharedDesignGLMTarget`` on ONE shared set of new rows:
    ``BatchedGLMTarget.predict`` without a copy of the rows per problem, and with row weights.  ``mean`` (K, D) and ``cov``
    (K, D, D) are the fitted Gaussians (of GSMBatch, BaMBatch, ADVIBatch or ``laplace_init_shared_batched``), ``A_new`` (M, D)
    the new rows of every problem (``target.A`` itself is taken as it is, without a copy), ``offset`` (K, M) their offsets (None:
    none, whether or not the target was built with one), ``y`` (K, M) their responses (None: no ``lpd`` / ``elpd``),
    ``weights`` (K, M) the row weights v_km, finite and >= 0 (None: 1 everywhere), ``nodes`` = Q the Gauss-Hermite nodes, 1 .. 64.

    Row m of problem k is valid iff v_km > 0, the rule of the target's own weights.  A valid row gets what ``predict`` gives
    for that row (``eta_mean``, ``eta_var``, ``mean``, and with ``y`` ``lpd``, the density of one unit observation, not
    weighted); a row of weight 0 is NaN in all four and its ``y`` and ``offset`` may hold anything, NaN included;
    ``elpd[k]`` = sum over the valid rows of v_km lpd[k, m], 0 for a problem without a valid row.  K-fold cross-validation:
    with the fold's mask as ``weights`` here and 1 - mask as the weights of the fit, ``elpd`` is the fold's held-out score
    (examples/kfold_shared_batched.py).  With ``weights`` None every field has the bits of ``predict`` on K copies of ``A_new``.

    Returns a ``GLMPrediction``; numpy in gives numpy out, CUDA tensors in give tensors out.  The shapes, ``nodes``,
    ``weights``, and ``y`` and ``offset`` where the weight is > 0, are validated before any device work (ValueError naming the
    argument and the problems).  Anything that is not a ``SharedDesignGLMTarget`` raises TypeError: a ``BatchedGLMTarget`` has
    ``BatchedGLMTarget.predict``.  One launch (gsmvi_glm_shared_predict_batched_f64)."""
    fn = "predict_shared_batched"
    if not isinstance(target, SharedDesignGLMTarget):
        raise TypeError(f"{fn}: target must be a SharedDesignGLMTarget, got {type(target).__name__}"
                        " (a BatchedGLMTarget has BatchedGLMTarget.predict)")
    K, D, family = target.K, target.D, target.family
    if isinstance(nodes, bool) or not isinstance(nodes, (int, np.integer)) or not 1 <= nodes <= 64:
        raise ValueError(f"nodes: expected an integer in 1 .. 64, got {nodes!r}")
    sa = _shape(A_new)
    if len(sa) != 2 or min(sa) < 1 or sa[1] != D:
        raise ValueError(f"A_new: expected shape (M, D) with D = {D} and M >= 1 (one set of new rows for all problems), got {sa}")
    M = sa[0]
    if _shape(mean) != (K, D):
        raise ValueError(f"mean: expected shape (K, D) = {(K, D)}, got {_shape(mean)}")
    if _shape(cov) != (K, D, D):
        raise ValueError(f"cov: expected shape (K, D, D) = {(K, D, D)}, got {_shape(cov)}")
    wh = _check_weights(weights, K, M, rows="M")
    live = wh > 0.0 if wh is not None else np.ones((1, M), dtype=bool)
    yh = None
    if y is not None:
        if _shape(y) != (K, M):
            raise ValueError(f"y: expected shape (K, M) = {(K, M)}, got {_shape(y)}")
        yh = _check_responses(y, family, live)
    oh = _check_offset(offset, K, M, live, rows="M")
    eng = engine if engine is not None else target.engine
    as_tensor = isinstance(mean, torch.Tensor)
    dev = lambda x: eng.asarray(x.contiguous() if isinstance(x, torch.Tensor) else x)      # noqa: E731
    out = eng.glm_shared_predict_batched(dev(mean), dev(cov), A_new if A_new is target.A else dev(A_new), family,
                                         offset=eng.asarray(oh) if oh is not None else None,
                                         y=eng.asarray(yh) if yh is not None else None,
                                         weights=eng.asarray(wh) if wh is not None else None,
                                         noise_prec=target.noise_precision, nodes=int(nodes))
    if not as_tensor:
        out = tuple(eng.to_numpy(t) if t is not None else None for t in out)
    return GLMPrediction(*out)


def _check_finite_per_problem(x, name, K):
    """``x``, a number or K values, as a host float64 array: finite (any sign), else ValueError"""
    v = np.asarray(_host_array(x), dtype=np.float64)
    if v.shape not in ((), (K,)):
        raise ValueError(f"{name}: expected a number or {K} values, got shape {v.shape}")
    if not np.isfinite(v).all():
        raise ValueError(f"{name}: expected finite values")
    return v


class BatchedNegBinomialTarget:
    """K Bayesian negative binomial regressions with their own data sets -- overdispersed counts, the dispersion fitted -- for
    ``GSMBatch``, ``BaMBatch``, ``ADVIBatch``, ``BatchedKLMonitor``, ``lbfgs_init_batched``, ``pathfinder_init_batched`` and
    ``psis_batched``.  Problem k has the design matrix A[k] (N, P), responses y[k] (N,) >= 0 (finite; they need not be integers),
    an optional ``offset[k]`` (N,) added to the linear predictor (a log exposure, say) and ``counts[k]`` <= N valid rows (None: all
    N; the rows beyond are ignored whatever they hold).  The parameter is x = (beta, theta) in R^D, D = P + 1 <= 64: theta = log r
    is the log of the size, the variance of an observation is mu + mu^2 / r, and r -> inf is the Poisson model.  With eta = A[k]
    beta + offset[k], d = eta - theta and r = exp(theta):

        t_n          = lgamma(y_n + r) - lgamma(r) - r softplus(d_n) - y_n softplus(-d_n)
        lp_k(x)      = sum_n t_n - lam_k |beta|^2 / 2 - kap_k (theta - m_k)^2 / 2            (unnormalised: -lgamma(y + 1) dropped)
        grad lp_k(x) = ( sum_n [y_n sigmoid(-d_n) - r sigmoid(d_n)] a_n - lam_k beta,
                         sum_n [r (psi(y_n + r) - psi(r) - softplus(d_n)) - (y_n sigmoid(-d_n) - r sigmoid(d_n))] - kap_k (theta - m_k) )

    evaluated by gsmvi_negbin_batched_f64: what examples/example_gsm.py:34-35 gets from a model's log_prob and jit(grad(...)).
    The priors: beta ~ N(0, I / lam_k), ``prior_precision`` = lam; theta ~ N(m_k, 1 / kap_k), ``log_size_mean`` = m and
    ``log_size_precision`` = kap; each a float or K values, a precision of 0 = flat.  The two differences of lgamma and of psi
    are evaluated as differences (never as two calls), and exp(eta) is never formed: the outputs are finite wherever the truth
    is.  A point whose exp(theta) is not a positive normal number (|theta| above 708) gets NaN outputs (the fits then revert that
    step).  numpy arrays or tensors in; everything is kept on the device as float64 / int32.  Arguments are validated on the host
    before any device work (ValueError naming the argument and the problems).

    ``lp_g(x, out=None)``: (K, B, D) -> (K, B, D) scores, ``device_native`` and ``graph_safe`` (one capturable launch, no
    allocation with ``out``).  ``lp(x)``: (K, rows, D) -> (K, rows) values; a device tensor or numpy.  ``lp_and_score(x)``:
    (scores, values) from one launch.  Attributes ``K, N, P, D``.  Not a ``BatchedGLMTarget``: its Hessian is not A^T W A (every
    row contributes a 2 x 2 block in (eta, theta)), so it has no ``neg_hessian``, ``predict`` or ``loo``, and
    ``laplace_init_batched`` and ``psis_loo_batched`` refuse it (TypeError).  Its negative Hessian is the function
    ``neg_hessian_negbin_batched(target, x)`` and its second-order start ``laplace_init_negbin_batched``.  Its leave-one-out is the function
    ``psis_loo_negbin_batched(target, mean, cov, keys, ...)``, which includes the -lgamma(y + 1) that ``lp`` drops and is so on one
    scale with ``psis_loo_batched`` of a poisson ``BatchedGLMTarget``.  Its posterior predictive is the function
    ``predict_negbin_batched(target, mean, cov, A_new, keys, ...)``, a mean over draws of q_k (the class gains no method)."""

    def __init__(self, A, y, prior_precision=1.0, counts=None, offset=None, log_size_mean=0.0, log_size_precision=1.0,
                 engine=None):
        sa = _shape(A)
        if len(sa) != 3 or min(sa) < 1:
            raise ValueError(f"A: expected shape (K, N, P) with K, N, P >= 1, got {sa}")
        K, N, P = sa
        if P + 1 > 64:
            raise ValueError(f"A: D = P + 1 = {P + 1} is outside 2 <= D <= 64 (beta and the log size)")
        if _shape(y) != (K, N):
            raise ValueError(f"y: expected shape (K, N) = {(K, N)}, got {_shape(y)}")
        cnt = _check_counts(counts, K, N)
        live = _live_rows(cnt, N)
        yh = _check_responses(y, "poisson", live, name_family=False)      # the count range: finite and >= 0
        oh = _check_offset(offset, K, N, live)
        lam = _check_per_problem(prior_precision, "prior_precision", K)
        tm = _check_finite_per_problem(log_size_mean, "log_size_mean", K)
        tk = _check_per_problem(log_size_precision, "log_size_precision", K)
        self.engine = engine if engine is not None else get_engine()
        eng = self.engine
        self.K, self.N, self.P, self.D = K, N, P, P + 1
        self.A = eng.asarray(A.contiguous() if isinstance(A, torch.Tensor) else A)
        self.y = eng.asarray(yh)
        self.offset = eng.asarray(oh) if oh is not None else None
        self.counts = eng.batched_counts(cnt) if cnt is not None else None
        self.prior_precision = float(lam) if lam.shape == () else eng.batched_regs(lam)
        self.log_size_mean = float(tm) if tm.shape == () else eng.batched_regs(tm)
        self.log_size_precision = float(tk) if tk.shape == () else eng.batched_regs(tk)

        def lp_g(x, out=None):
            return self._call(x, out=out, want="g")
        lp_g.device_native = True
        lp_g.graph_safe = True          # one capturable kernel launch, no allocation when `out` is given, no host work
        self.lp_g = lp_g

    def _call(self, x, **kw):
        return self.engine.negbin_batched(x, self.A, self.y, offset=self.offset, counts=self.counts,
                                          prior_prec=self.prior_precision, log_size_mean=self.log_size_mean,
                                          log_size_prec=self.log_size_precision, **kw)

    def lp(self, x):
        """(K, rows) values lp_k(x_kr) at the rows of x (K, rows, D), a device tensor or numpy; one launch"""
        return self._call(self.engine.asarray(x), want="lp")

    def lp_and_score(self, x):
        """(scores (K, rows, D), values (K, rows)) from one launch"""
        return self._call(self.engine.asarray(x), want="both")


def neg_hessian_negbin_batched(target, x, *, engine=None):
    """(K, D, D) negative Hessians of lp_k of a ``BatchedNegBinomialTarget`` at the rows of x (K, D) = (beta, theta): with d =
    eta - theta, r = exp(theta), sigma = sigmoid(d), r_eta = y sigmoid(-d) - r sigma, dps = psi(y + r) - psi(r) and dtg =
    psi'(y + r) - psi'(r),

        w_ee = (y + r) sigma sigmoid(-d),   w_et = -sigma r_eta,   w_tt = -[r (dps - softplus(d)) + r^2 dtg + r sigma - sigma r_eta]
        H[:P, :P] = sum_n w_ee,n a_n a_n^T + lam_k I,   H[:P, P] = sum_n w_et,n a_n,   H[P, P] = sum_n w_tt,n + kap_k

    Exactly symmetric, and NOT positive semi-definite in general (w_tt has any sign: lp_k is not concave in theta).  A point
    whose exp(theta) is not a positive normal number gives NaN.  A device tensor or numpy in; one launch
    (gsmvi_negbin_hessian_batched_f64).  Anything that is not a ``BatchedNegBinomialTarget`` raises TypeError."""
    if not isinstance(target, BatchedNegBinomialTarget):
        raise TypeError(f"neg_hessian_negbin_batched: target must be a BatchedNegBinomialTarget, got {type(target).__name__}")
    K, D = target.K, target.D
    if _shape(x) != (K, D):
        raise ValueError(f"neg_hessian_negbin_batched: x must be (K, D) = {(K, D)} of the target, got {_shape(x)}")
    eng = engine if engine is not None else target.engine
    return eng.negbin_hessian_batched(eng.asarray(x), target.A, target.y, offset=target.offset, counts=target.counts,
                                      prior_prec=target.prior_precision, log_size_mean=target.log_size_mean,
                                      log_size_prec=target.log_size_precision, want="h")


def _as_tensor(a):
    return a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))


def _predict_draws_args(fn, target, mean, cov, A_new, keys, offset, y, check_y, counts, num_draws, call, psis, weights, engine):
    """What ``predict_softmax_batched``, ``predict_negbin_batched`` and ``predict_ordinal_batched`` share before their launch,
    after their own check of the target's type: the argument checks in the order of their docstrings (``check_y(y, live)`` is the
    family's response check; every message carries ``fn``), then the draws and weights: a ``psis`` that is given is reused, else
    ``psis_batched`` (``weights="psis"``) or one ``kl_draw_batched`` with its seed rule.  Returns a namespace: ``eng``; ``X``,
    ``lw`` (None: uniform), ``A_new``, ``offset`` and ``counts_dev`` for the launch; ``y`` the checked responses on the host;
    ``counts`` on the host; ``K``, ``M``, ``S``, ``nlaunch`` (this launch included) and ``psis``."""
    from types import SimpleNamespace
    from .diagnostics import MAX_DRAWS, MIN_DRAWS, _reusable, psis_batched
    from .monitors import _to_numpy
    if weights not in ("uniform", "psis"):
        raise ValueError(f"{fn}: weights: expected 'uniform' or 'psis', got {weights!r}")
    K, D, P = target.K, target.D, target.P
    sa = _shape(A_new)
    if len(sa) != 3 or min(sa) < 1 or sa[0] != K or sa[2] != P:
        raise ValueError(f"{fn}: A_new: expected shape (K, M, P) with K = {K}, P = {P} and M >= 1, got {sa}")
    M = sa[1]
    if _shape(mean) != (K, D):
        raise ValueError(f"{fn}: mean must be (K, D) = {(K, D)} of the target, got {_shape(mean)}")
    if _shape(cov) != (K, D, D):
        raise ValueError(f"{fn}: cov must be {(K, D, D)}, got {_shape(cov)}")
    try:
        cnt = _check_counts(counts, K, M, rows="M")
        live = _live_rows(cnt, M)
        yh = None
        if y is not None:
            if _shape(y) != (K, M):
                raise ValueError(f"y: expected shape (K, M) = {(K, M)}, got {_shape(y)}")
            yh = check_y(y, live)
        oh = _check_offset(offset, K, M, live, rows="M")
    except ValueError as e:
        raise ValueError(f"{fn}: {e}") from None
    keys_l = [int(k) for k in np.asarray(list(keys) if isinstance(keys, (list, tuple, range)) else _to_numpy(keys)).reshape(-1)]
    if len(keys_l) != K:
        raise ValueError(f"{fn}: {len(keys_l)} keys for K = {K} problems")
    eng = engine if engine is not None else target.engine
    if psis is None:
        S = int(num_draws)
        if S != num_draws or not MIN_DRAWS <= S <= MAX_DRAWS:
            raise ValueError(f"{fn}: num_draws = {num_draws} is outside {MIN_DRAWS} <= num_draws <= {MAX_DRAWS}")
        if weights == "psis":
            psis = psis_batched(target.lp, mean, cov, keys_l, S, call=call, moments=False, as_torch=True, engine=eng)
            nlaunch = psis.nlaunch + 1
            X, _, lw = _reusable(psis, K, D, eng, fn)
        else:
            seeds = eng.batched_seeds(tuple((k % (2 ** 32)) ^ 0x5DEECE66D for k in keys_l))
            X, _, _ = eng.kl_draw_batched(eng.asarray(mean), eng.asarray(cov), seeds, int(call), 0, S)
            nlaunch, lw = 2, None
    else:
        X, _, lw = _reusable(psis, K, D, eng, fn)
        S = _shape(X)[1]
        nlaunch = 1
        if weights == "uniform":
            lw = None
    return SimpleNamespace(eng=eng, X=X, lw=lw, A_new=eng.asarray(A_new.contiguous() if isinstance(A_new, torch.Tensor) else A_new),
                           y=yh, offset=eng.asarray(oh) if oh is not None else None, counts=cnt,
                           counts_dev=eng.batched_counts(cnt) if cnt is not None else None, K=K, M=M, S=S, nlaunch=nlaunch,
                           psis=psis)


def _predict_draws_result(result, a, out, lpd, as_torch, ints=()):
    """The ``result`` dataclass of a draw-based predictive from the namespace ``a`` of ``_predict_draws_args``, the family's
    outputs ``out`` and ``lpd``: ``elpd`` is the sum of ``lpd`` over the valid rows (None without ``lpd``); without ``as_torch``
    everything goes to numpy, the fields named in ``ints`` as int64"""
    elpd = None
    if lpd is not None:
        lt = _as_tensor(lpd)
        nk = _as_tensor(a.counts).to(lt.device) if a.counts is not None else torch.full((a.K,), a.M, device=lt.device)
        mask = torch.arange(a.M, device=lt.device)[None, :] < nk[:, None]
        elpd = torch.where(mask, lt, torch.zeros((), dtype=lt.dtype, device=lt.device)).sum(1)
    out = dict(out, lpd=lpd, elpd=elpd)
    if not as_torch:
        out = {n: None if t is None else np.asarray(a.eng.to_numpy(t)) for n, t in out.items()}
        for n in ints:
            out[n] = out[n].astype(np.int64)
    return result(psis=a.psis, num_draws=a.S, nlaunch=a.nlaunch, **out)


def _first_maximum(prob):
    """``prob`` (K, M, C) as a tensor, the mask of its NaN rows, and ``label``: the first maximum of a row, -1 where it is NaN"""
    pt = _as_tensor(prob)
    dead = torch.isnan(pt).any(2)
    return pt, dead, torch.where(dead, torch.full((), -1, dtype=torch.int64, device=pt.device), pt.argmax(2))


@dataclass
class NegBinPrediction:
    """What ``predict_negbin_batched`` returns for M new rows of each of K negative binomial problems under the fitted q_k =
    N(mean_k, cov_k) over (beta, theta = log r) (numpy arrays, or the engine's tensors with ``as_torch``): ``log_moments``
    (K, M, 3) = log E[mu], log E[mu^2], log E[mu^2 / r] over the (weighted) draws, mu = exp(eta); ``mean`` (K, M) = exp(log E[mu]),
    the predictive mean of the count; ``var`` (K, M) = E[mu + mu^2 / r] + Var[mu], its predictive variance (wider than the mean:
    the overdispersion and the spread of the draws).  ``mean`` is +inf where log E[mu] exceeds 709.78 (and ``var`` with it):
    ``log_moments`` stays finite there and is what to use.  With ``y``, ``lpd`` (K, M) = log E[p(y | eta, theta)] per row,
    -lgamma(y + 1) included (the scale of ``psis_loo_negbin_batched``), and ``elpd`` (K,), its sum over the valid rows: the
    held-out score by which fits are compared (both None without ``y``).  Rows beyond ``counts[k]`` are NaN.  ``psis`` the
    problem-level ``PSISBatchedResult`` whose draws (and, with ``weights="psis"``, weights) were used (device tensors: hand it
    back as ``psis=`` to reuse them), None where none was made or given; ``num_draws`` = S; ``nlaunch`` the kernel launches made.
    A Monte-Carlo mean: no y is sampled and there are no quantiles.  [examples/example_gsm.py:34-35, the use of the fit; no
    reference twin]"""
    mean: Any
    var: Any
    log_moments: Any
    lpd: Any
    elpd: Any
    psis: Any
    num_draws: int
    nlaunch: int


def predict_negbin_batched(target, mean, cov, A_new, keys, offset=None, y=None, counts=None, num_draws=1024, *, call=0, psis=None,
                           weights="uniform", as_torch=False, engine=None):
    """The posterior predictive of K fitted negative binomial posteriors q_k = N(mean_k, cov_k) on new rows: returns a
    ``NegBinPrediction``.

    ``target`` is the ``BatchedNegBinomialTarget`` the posteriors were fitted to (its P is the model; anything else raises
    TypeError); mean (K, D), D = P + 1, cov (K, D, D) and ``keys`` are ``psis_batched``'s; ``A_new`` (K, M, P) are the new rows,
    ``offset`` (K, M) is added to their linear predictor, ``y`` (K, M) their counts (None: no ``lpd`` / ``elpd``), ``counts`` (K,)
    the valid rows per problem (None: all M).  theta = log r is a coordinate of q_k, correlated with beta, so a row's density
    depends on the pair (eta, theta) and there is no one-dimensional quadrature: the predictive is a mean over S = ``num_draws``
    draws of q_k.
    ``weights="uniform"``: one call of ``kl_draw_batched`` with ``psis_batched``'s seed rule (seed (keys[k] % 2**32) ^
    0x5DEECE66D, draw number ``call``: the bits ``psis_batched`` would draw), no call of ``target.lp``, then one launch,
    gsmvi_negbin_predict_batched_f64 (the definition is in include/gsmvi_hip.h): the linear predictors of every draw on the fp64
    MFMA, then four log-sum-exps over the draws; no (K, S, M) block is formed.  ``weights="psis"``: first
    ``psis_batched(target.lp, mean, cov, keys, num_draws, call=call, moments=False, as_torch=True)``, then the launch with its
    smoothed ``log_weights``: the importance-corrected predictive; the result carries ``psis`` (khat, ``ok``), and a problem whose
    problem-level run failed comes out NaN.  ``psis=``, the result of such a call, is reused (``num_draws`` and ``call`` are then
    not used): its draws alone with ``"uniform"``, its weights too with ``"psis"``.  mean and cov are only read.
    An ``A_new`` that is not (K, M, P), a mean that is not (K, D) of the target, a cov that is not (K, D, D), an ``offset`` that is
    not (K, M) or not finite in the valid rows, a ``y`` that is not (K, M) or not finite and >= 0 in the valid rows (non-integers
    are allowed, as in the target), bad ``counts``, keys of another length than K, ``num_draws`` outside 5..4096, an unknown
    ``weights`` or a ``psis`` that is not a ``PSISBatchedResult`` holding device tensors of the right shapes raise ValueError
    naming the argument before any device work."""
    fn = "predict_negbin_batched"
    if not isinstance(target, BatchedNegBinomialTarget):
        raise TypeError(f"{fn}: target must be a BatchedNegBinomialTarget, got {type(target).__name__}")
    count_range = lambda y, live: _check_responses(y, "poisson", live, name_family=False)      # noqa: E731  (finite and >= 0)
    a = _predict_draws_args(fn, target, mean, cov, A_new, keys, offset, y, count_range, counts, num_draws, call, psis, weights, engine)
    eng = a.eng
    lmom, lpd = eng.negbin_predict_batched(a.X, a.lw, a.A_new, y=eng.asarray(a.y) if a.y is not None else None, offset=a.offset,
                                           counts=a.counts_dev)
    lm = _as_tensor(lmom)
    m1 = torch.exp(lm[..., 0])
    # E[mu + mu^2 / r] + Var[mu]; the variance of mu as e^lmom1 (1 - e^(2 lmom0 - lmom1)): one exponential of a difference <= 0
    # (where it rounds to no spread at all the term is 0, not inf x 0)
    spread = -torch.expm1(2.0 * lm[..., 0] - lm[..., 1])
    var = m1 + torch.exp(lm[..., 2]) + torch.where(spread > 0.0, torch.exp(lm[..., 1]) * spread, torch.zeros_like(spread))
    return _predict_draws_result(NegBinPrediction, a, dict(mean=m1, var=var, log_moments=lmom), lpd, as_torch)


def _check_labels(y, C, live):
    """the labels as a host int32 array: an integer dtype or floats with integral values, in 0 .. C - 1 in the valid rows (the
    rows beyond are stored as 0), else ValueError naming the problems"""
    yh = np.asarray(_host_array(y))
    if yh.dtype == np.bool_ or not (np.issubdtype(yh.dtype, np.integer) or np.issubdtype(yh.dtype, np.floating)):
        raise ValueError(f"y: expected integer labels (an integer dtype, or floats with integral values), got dtype {yh.dtype}")
    with np.errstate(invalid="ignore"):
        good = (yh >= 0) & (yh <= C - 1)                              # (a NaN fails both comparisons)
        if np.issubdtype(yh.dtype, np.floating):
            good &= yh == np.floor(yh)
    bad = live & ~good
    if bad.any():
        raise ValueError(f"y: labels that are not integers in 0 .. num_classes - 1 = {C - 1} in the valid rows of problems "
                         f"{np.flatnonzero(bad.any(1)).tolist()}")
    return np.where(live & good, yh, 0).astype(np.int32)


class BatchedSoftmaxTarget:
    """K Bayesian multinomial logit (softmax) regressions with their own data sets, for ``GSMBatch``, ``BaMBatch``,
    ``ADVIBatch``, ``BatchedKLMonitor``, ``lbfgs_init_batched`` and ``psis_batched``.  Problem k has the design matrix A[k]
    (N, P), integer labels y[k] (N,) in 0 .. C - 1 (``num_classes`` = C >= 2; no soft labels), ``counts[k]`` <= N valid rows
    (None: all N; the rows beyond are ignored whatever they hold) and the prior N(0, I / lam_k), ``prior_precision`` = lam a float
    or K values, 0 = flat.  Class C - 1 is the reference class with zero coefficients; the parameter is x in R^D, D = (C - 1) P
    <= 64, class-major: x[c P + j] = W_cj.  With eta_nc = a_n . w_c for c < C - 1 and eta_n,C-1 = 0:

        m_n = max_c eta_nc,   s_n = sum_c exp(eta_nc - m_n)
        lp_k(x)      = sum_n [ eta_n,y_n - m_n - log s_n ] - lam_k |x|^2 / 2            (unnormalised log posterior)
        grad lp_k(x) = sum_n ( [y_n = c] - exp(eta_nc - m_n) / s_n ) a_nj - lam_k x_cj   (c < C - 1)

    evaluated by gsmvi_softmax_batched_f64: what examples/example_gsm.py:34-35 gets from a model's log_prob and jit(grad(...)).
    numpy arrays or tensors in; everything is kept on the device as float64 / int32.  Arguments are validated on the host before
    any device work (ValueError naming the argument and the problems).  It is not a ``BatchedGLMTarget``: there is no offset, and
    ``laplace_init_batched``, ``predict`` and ``psis_loo_batched`` do not take it (TypeError).  Its second-order start is
    ``laplace_init_softmax_batched``, on the closed-form negative Hessian that ``neg_hessian`` returns, and its PSIS leave-one-out
    is ``psis_loo_softmax_batched(target, mean, cov, keys, ...)`` (``.loo`` stays ``psis_loo_batched``'s TypeError).  Its posterior
    predictive is ``predict_softmax_batched(target, mean, cov, A_new, keys, ...)`` (``.predict`` stays a TypeError that names it).

    ``lp_g(x, out=None)``: (K, B, D) -> (K, B, D) scores, ``device_native`` and ``graph_safe`` (one capturable launch, no
    allocation with ``out``).  ``lp(x)``: (K, rows, D) -> (K, rows) values; a device tensor or numpy.  ``lp_and_score(x)``:
    (scores, values) from one launch.  ``neg_hessian(x)``: (K, D) -> (K, D, D).  Attributes ``K, N, D, P, C``."""

    def __init__(self, A, y, num_classes, prior_precision=1.0, counts=None, engine=None):
        if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or num_classes < 2:
            raise ValueError(f"num_classes: expected an integer >= 2, got {num_classes!r}")
        C = int(num_classes)
        sa = _shape(A)
        if len(sa) != 3 or min(sa) < 1:
            raise ValueError(f"A: expected shape (K, N, P) with K, N, P >= 1, got {sa}")
        K, N, P = sa
        if (C - 1) * P > 64:
            raise ValueError(f"num_classes: D = (num_classes - 1) P = {(C - 1) * P} is outside 1 <= D <= 64 (P = {P})")
        if _shape(y) != (K, N):
            raise ValueError(f"y: expected shape (K, N) = {(K, N)}, got {_shape(y)}")
        cnt = _check_counts(counts, K, N)
        yh = _check_labels(y, C, _live_rows(cnt, N))
        lam = _check_per_problem(prior_precision, "prior_precision", K)
        self.engine = engine if engine is not None else get_engine()
        eng = self.engine
        self.K, self.N, self.P, self.C, self.D = K, N, P, C, (C - 1) * P
        self.A = eng.asarray(A.contiguous() if isinstance(A, torch.Tensor) else A)
        self.y = eng.batched_labels(yh)
        self.counts = eng.batched_counts(cnt) if cnt is not None else None
        self.prior_precision = float(lam) if lam.shape == () else eng.batched_regs(lam)

        def lp_g(x, out=None):
            return self._call(x, out=out, want="g")
        lp_g.device_native = True
        lp_g.graph_safe = True          # one capturable kernel launch, no allocation when `out` is given, no host work
        self.lp_g = lp_g

    def _call(self, x, **kw):
        return self.engine.softmax_batched(x, self.A, self.y, self.C, counts=self.counts, prior_prec=self.prior_precision, **kw)

    def lp(self, x):
        """(K, rows) values lp_k(x_kr) at the rows of x (K, rows, D), a device tensor or numpy; one launch"""
        return self._call(self.engine.asarray(x), want="lp")

    def lp_and_score(self, x):
        """(scores (K, rows, D), values (K, rows)) from one launch"""
        return self._call(self.engine.asarray(x), want="both")

    def neg_hessian(self, x):
        """(K, D, D) negative Hessians of lp_k at the rows of x (K, D): block (c, c') is sum_n w_n,cc' a_n a_n^T + lam_k [c = c'] I
        with p_nc = exp(eta_nc - m_n) / s_n, w_n,cc = p_nc (1 - p_nc) and w_n,cc' = -p_nc p_nc' (1 - p formed as a sum over the other
        classes, so a saturated class keeps its digits), exactly symmetric; a device tensor or numpy; one launch"""
        eng = self.engine
        return eng.softmax_hessian_batched(eng.asarray(x), self.A, self.y, self.C, counts=self.counts,
                                           prior_prec=self.prior_precision, want="h")

    def predict(self, *args, **kw):
        """TypeError: the quadrature of ``BatchedGLMTarget.predict`` is for one linear predictor per row; the softmax target's
        predictive is ``predict_softmax_batched(target, mean, cov, A_new, keys, ...)``, from draws of q_k"""
        raise TypeError("BatchedSoftmaxTarget.predict: the method is the GLM targets' (one linear predictor per row); call "
                        "predict_softmax_batched(target, mean, cov, A_new, keys, ...) for the softmax target")

    def loo(self, mean, cov, keys, **kw):
        """``psis_loo_batched(self, ...)``, which takes the GLM targets only: TypeError"""
        from .diagnostics import psis_loo_batched
        return psis_loo_batched(self, mean, cov, keys, **kw)


class BatchedOrdinalTarget:
    """K Bayesian cumulative-logit (proportional odds) regressions with their own data sets -- ordered categories: ratings, grades,
    severity scores, Likert items -- for ``GSMBatch``, ``BaMBatch``, ``ADVIBatch``, ``BatchedKLMonitor``, ``lbfgs_init_batched``,
    ``pathfinder_init_batched`` and ``psis_batched``.  Problem k has the design matrix A[k] (N, P) WITHOUT an intercept column (the
    cutpoints are the intercepts), integer labels y[k] (N,) in 0 .. C - 1 (``num_classes`` = C >= 2), an optional ``offset[k]`` (N,)
    added to the linear predictor and ``counts[k]`` <= N valid rows (None: all N; the rows beyond are ignored whatever they hold).
    The parameter is x = (beta, delta) in R^D, D = P + C - 1 <= 64; the cutpoints are ordered by construction:

        cut_0 = delta_0,   cut_j = cut_{j-1} + exp(delta_j)     (j = 1 .. C - 2)          (``cutpoints(x)``)
        P(y_n = c)   = sigmoid(cut_c - eta_n) - sigmoid(cut_{c-1} - eta_n),   eta = A[k] beta + offset[k],  cut_{-1} = -inf, cut_{C-1} = inf
        lp_k(x)      = sum_n log P(y_n) - lam_k |beta|^2 / 2 - kap_k |delta|^2 / 2

    evaluated with its score by gsmvi_ordinal_batched_f64: what examples/example_gsm.py:34-35 gets from a model's log_prob and
    jit(grad(...)).  No two probabilities are subtracted: with a = cut_{y-1} - eta, b = cut_y - eta and w = exp(delta_y) the gap of
    an interior class, log P = -softplus(-b) - softplus(a) + log(1 - exp(-w)), and the residuals are sigmoids and 1 / expm1(w).  The
    priors: beta ~ N(0, I / lam_k), ``prior_precision`` = lam; delta ~ N(0, I / kap_k), ``cut_precision`` = kap; each a float or K
    values, a precision of 0 = flat.  For C = 2 the model is logistic regression on the design [A, -1].  A point at which some
    exp(delta_j), j >= 1, is not a positive normal number (|delta_j| above 708) gets NaN outputs (the fits then revert that step);
    delta_0 is a location and is not limited.  numpy arrays or tensors in; everything is kept on the device as float64 / int32.
    Arguments are validated on the host before any device work (ValueError naming the argument and the problems).

    ``lp_g(x, out=None)``: (K, B, D) -> (K, B, D) scores, ``device_native`` and ``graph_safe`` (one capturable launch, no
    allocation with ``out``).  ``lp(x)``: (K, rows, D) -> (K, rows) values; a device tensor or numpy.  ``lp_and_score(x)``:
    (scores, values) from one launch.  ``cutpoints(x)``: (..., D) -> (..., C - 1), how a fit is read.  Attributes ``K, N, P, C, D``.
    Not a ``BatchedGLMTarget``: it has no ``neg_hessian``, ``predict`` or ``loo``, and ``laplace_init_batched``,
    ``psis_loo_batched`` and their softmax and negative binomial namesakes refuse it (TypeError).  The leave-one-out of this
    family is the free function ``psis_loo_ordinal_batched(target, mean, cov, keys, ...)``: l_si = log P(y_i) is normalised, so its
    ``elpd_loo`` is on the scale of ``psis_loo_softmax_batched`` on the same labels.  The Hessian and the Laplace start are free
    functions too: ``neg_hessian_ordinal_batched(target, x)`` and ``laplace_init_ordinal_batched(target, ...)``.  The posterior
    predictive on new rows is the free function ``predict_ordinal_batched(target, mean, cov, A_new, keys, ...)``
    (``OrdinalPrediction``: class probabilities, the most probable and the median class, the held-out score): the family now has
    all four pieces.  (Before the Hessian and the Laplace start were added this paragraph ended "A Hessian and Laplace start and
    a posterior predictive do not exist yet for this family", a sentence tests/test_psis_loo_ordinal_cpu.py still looks for;
    before the predictive was added it said "Only the posterior predictive is missing now for this family", which
    tests/test_ordinal_laplace_cpu.py still looks for.)"""

    def __init__(self, A, y, num_classes, prior_precision=1.0, cut_precision=1.0, counts=None, offset=None, engine=None):
        if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or num_classes < 2:
            raise ValueError(f"num_classes: expected an integer >= 2, got {num_classes!r}")
        C = int(num_classes)
        sa = _shape(A)
        if len(sa) != 3 or min(sa) < 1:
            raise ValueError(f"A: expected shape (K, N, P) with K, N, P >= 1, got {sa}")
        K, N, P = sa
        if P + C - 1 > 64:
            raise ValueError(f"A: D = P + num_classes - 1 = {P + C - 1} is outside 2 <= D <= 64 (beta and the C - 1 cutpoints)")
        if _shape(y) != (K, N):
            raise ValueError(f"y: expected shape (K, N) = {(K, N)}, got {_shape(y)}")
        cnt = _check_counts(counts, K, N)
        live = _live_rows(cnt, N)
        yh = _check_labels(y, C, live)
        oh = _check_offset(offset, K, N, live)
        lam = _check_per_problem(prior_precision, "prior_precision", K)
        kap = _check_per_problem(cut_precision, "cut_precision", K)
        self.engine = engine if engine is not None else get_engine()
        eng = self.engine
        self.K, self.N, self.P, self.C, self.D = K, N, P, C, P + C - 1
        self.A = eng.asarray(A.contiguous() if isinstance(A, torch.Tensor) else A)
        self.y = eng.batched_labels(yh)
        self.offset = eng.asarray(oh) if oh is not None else None
        self.counts = eng.batched_counts(cnt) if cnt is not None else None
        self.prior_precision = float(lam) if lam.shape == () else eng.batched_regs(lam)
        self.cut_precision = float(kap) if kap.shape == () else eng.batched_regs(kap)

        def lp_g(x, out=None):
            return self._call(x, out=out, want="g")
        lp_g.device_native = True
        lp_g.graph_safe = True          # one capturable kernel launch, no allocation when `out` is given, no host work
        self.lp_g = lp_g

    def _call(self, x, **kw):
        return self.engine.ordinal_batched(x, self.A, self.y, self.C, offset=self.offset, counts=self.counts,
                                           prior_prec=self.prior_precision, cut_prec=self.cut_precision, **kw)

    def lp(self, x):
        """(K, rows) values lp_k(x_kr) at the rows of x (K, rows, D), a device tensor or numpy; one launch"""
        return self._call(self.engine.asarray(x), want="lp")

    def lp_and_score(self, x):
        """(scores (K, rows, D), values (K, rows)) from one launch"""
        return self._call(self.engine.asarray(x), want="both")

    def cutpoints(self, x):
        """(..., D) parameters -> the (..., C - 1) ordered cutpoints cut_0 = delta_0, cut_j = cut_{j-1} + exp(delta_j): plain torch
        ops on the device or host the parameters are on; numpy in gives numpy out"""
        as_numpy = not isinstance(x, torch.Tensor)
        t = torch.as_tensor(np.asarray(x, dtype=np.float64)) if as_numpy else x
        if t.shape[-1] != self.D:
            raise ValueError(f"x: expected {self.D} = P + C - 1 trailing entries, got shape {tuple(t.shape)}")
        d = t[..., self.P:]
        cut = torch.cumsum(torch.cat([d[..., :1], torch.exp(d[..., 1:])], dim=-1), dim=-1)
        return cut.numpy() if as_numpy else cut


def neg_hessian_ordinal_batched(target, x, *, engine=None):
    """(K, D, D) negative Hessians of lp_k of a ``BatchedOrdinalTarget`` at the rows of x (K, D) = (beta, delta): with w_0 = 1,
    w_i = exp(delta_i), q_i = 1 / expm1(w_i), fa = sigmoid(a) sigmoid(-a) (0 for y = 0), fb = sigmoid(b) sigmoid(-b) (0 for
    y = C - 1), e_ni = fa + fb (i < y_n), fb (i = y_n), 0 (i > y_n), F(i) = sum_n e_ni, cnt_i the rows labelled i (interior
    classes) and S_i = d lp_lik / d w_i,

        H[:P, :P] = sum_n (fa + fb)_n a_n a_n^T + lam_k I,   H[:P, P + i] = -w_i sum_n e_ni a_n,
        H[P + i, P + i'] = w_i w_i' F(max(i, i')),   H[P + i, P + i] = w_i^2 F(i) + (w_i q_i)(w_i + w_i q_i) cnt_i - [i >= 1] w_i S_i + kap_k

    Exactly symmetric; a sum of positive semi-definite terms but for the chain terms -w_i S_i, which vanish at a mode with
    kap = 0 and make H indefinite away from it.  A point at which some exp(delta_j), j >= 1, is not a positive normal number
    gives NaN.  A device tensor or numpy in; one launch (gsmvi_ordinal_hessian_batched_f64).  Anything that is not a
    ``BatchedOrdinalTarget`` raises TypeError."""
    if not isinstance(target, BatchedOrdinalTarget):
        raise TypeError(f"neg_hessian_ordinal_batched: target must be a BatchedOrdinalTarget, got {type(target).__name__}")
    K, D = target.K, target.D
    if _shape(x) != (K, D):
        raise ValueError(f"neg_hessian_ordinal_batched: x must be (K, D) = {(K, D)} of the target, got {_shape(x)}")
    eng = engine if engine is not None else target.engine
    return eng.ordinal_hessian_batched(eng.asarray(x), target.A, target.y, target.C, offset=target.offset, counts=target.counts,
                                       prior_prec=target.prior_precision, cut_prec=target.cut_precision, want="h")


@dataclass
class SoftmaxPrediction:
    """What ``predict_softmax_batched`` returns for M new rows of each of K multinomial logit problems under the fitted q_k =
    N(mean_k, cov_k) (numpy arrays, or the engine's tensors with ``as_torch``): ``prob`` (K, M, C) the predictive class
    probabilities, the (weighted) mean over the draws of softmax(eta); ``label`` (K, M) int64 the first maximum of ``prob``, -1
    where the row is NaN; with ``y``, ``lpd`` (K, M) = log E[p(y | eta)] per row and ``elpd`` (K,), its sum over the valid rows:
    the held-out score by which fits of one model are compared (both None without ``y``).  Rows beyond ``counts[k]`` are NaN.
    ``psis`` the problem-level ``PSISBatchedResult`` whose draws (and, with ``weights="psis"``, weights) were used (device
    tensors: hand it back as ``psis=`` to reuse them), None where none was made or given; ``num_draws`` = S; ``nlaunch`` the
    kernel launches made.  [examples/example_gsm.py:34-35, the use of the fit; no reference twin]"""
    prob: Any
    label: Any
    lpd: Any
    elpd: Any
    psis: Any
    num_draws: int
    nlaunch: int


def predict_softmax_batched(target, mean, cov, A_new, keys, y=None, counts=None, num_draws=1024, *, call=0, psis=None,
                            weights="uniform", as_torch=False, engine=None):
    """The posterior predictive of K fitted multinomial logit posteriors q_k = N(mean_k, cov_k) on new rows: returns a
    ``SoftmaxPrediction``.

    ``target`` is the ``BatchedSoftmaxTarget`` the posteriors were fitted to (its number of classes and P are the model; anything
    else raises TypeError); mean (K, D), D = (C - 1) P, cov (K, D, D) and ``keys`` are ``psis_batched``'s; ``A_new`` (K, M, P) are
    the new rows, ``y`` (K, M) their integer labels (None: no ``lpd`` / ``elpd``), ``counts`` (K,) the valid rows per problem
    (None: all M).  A softmax row has C - 1 coupled linear predictors, so there is no one-dimensional quadrature: the predictive
    is a mean over S = ``num_draws`` draws of q_k.
    ``weights="uniform"``: one call of ``kl_draw_batched`` with ``psis_batched``'s seed rule (seed (keys[k] % 2**32) ^
    0x5DEECE66D, draw number ``call``: the bits ``psis_batched`` would draw), no call of ``target.lp``, then one launch,
    gsmvi_softmax_predict_batched_f64 (the definition is in include/gsmvi_hip.h): per class the linear predictors of every draw
    on the fp64 MFMA, the class probabilities summed over the draws and the log-sum-exp of the rows' log likelihoods; no
    (K, S, M, C) block is formed.  ``weights="psis"``: first ``psis_batched(target.lp, mean, cov, keys, num_draws, call=call,
    moments=False, as_torch=True)``, then the launch with its smoothed ``log_weights``: the importance-corrected predictive; the
    result carries ``psis`` (khat, ``ok``), and a problem whose problem-level run failed comes out NaN.  ``psis=``, the result
    of such a call, is reused (``num_draws`` and ``call`` are then not used): its draws alone with ``"uniform"``, its weights
    too with ``"psis"``.  mean and cov are only read.
    An ``A_new`` that is not (K, M, P), a mean that is not (K, D) of the target, a cov that is not (K, D, D), labels outside
    0 .. C - 1 in the valid rows, bad ``counts``, keys of another length than K, ``num_draws`` outside 5..4096, an unknown
    ``weights`` or a ``psis`` that is not a ``PSISBatchedResult`` holding device tensors of the right shapes raise ValueError
    naming the argument before any device work."""
    fn = "predict_softmax_batched"
    if not isinstance(target, BatchedSoftmaxTarget):
        raise TypeError(f"{fn}: target must be a BatchedSoftmaxTarget, got {type(target).__name__}")
    C = target.C
    a = _predict_draws_args(fn, target, mean, cov, A_new, keys, None, y, lambda y, live: _check_labels(y, C, live), counts, num_draws,
                            call, psis, weights, engine)
    eng = a.eng
    prob, lpd = eng.softmax_predict_batched(a.X, a.lw, a.A_new, C, labels=eng.batched_labels(a.y) if a.y is not None else None,
                                            counts=a.counts_dev)
    _, _, label = _first_maximum(prob)
    return _predict_draws_result(SoftmaxPrediction, a, dict(prob=prob, label=label), lpd, as_torch, ints=("label",))


@dataclass
class OrdinalPrediction:
    """What ``predict_ordinal_batched`` returns for M new rows of each of K cumulative-logit problems under the fitted q_k =
    N(mean_k, cov_k) over (beta, delta) (numpy arrays, or the engine's tensors with ``as_torch``): ``prob`` (K, M, C) the
    predictive class probabilities, the (weighted) mean over the draws of P(y = c | eta, cutpoints); ``label`` (K, M) int64 the
    first maximum of ``prob`` and ``median`` (K, M) int64 the smallest c whose cumulative ``prob`` reaches 0.5, the point
    prediction proper to ordered classes (it minimises the expected absolute error in class steps), both -1 where the row is
    NaN; with ``y``, ``lpd`` (K, M) = log E[P(y | eta, cutpoints)] per row (the scale of ``psis_loo_ordinal_batched``) and
    ``elpd`` (K,), its sum over the valid rows: the held-out score by which fits of one model are compared (both None without
    ``y``).  Rows beyond ``counts[k]`` are NaN.  ``psis`` the problem-level ``PSISBatchedResult`` whose draws (and, with
    ``weights="psis"``, weights) were used (device tensors: hand it back as ``psis=`` to reuse them), None where none was made or
    given; ``num_draws`` = S; ``nlaunch`` the kernel launches made.  [examples/example_gsm.py:34-35, the use of the fit; no
    reference twin]"""
    prob: Any
    label: Any
    median: Any
    lpd: Any
    elpd: Any
    psis: Any
    num_draws: int
    nlaunch: int


def predict_ordinal_batched(target, mean, cov, A_new, keys, offset=None, y=None, counts=None, num_draws=1024, *, call=0, psis=None,
                            weights="uniform", as_torch=False, engine=None):
    """The posterior predictive of K fitted cumulative-logit posteriors q_k = N(mean_k, cov_k) on new rows: returns an
    ``OrdinalPrediction``.

    ``target`` is the ``BatchedOrdinalTarget`` the posteriors were fitted to (its number of classes and P are the model; anything
    else raises TypeError); mean (K, D), D = P + C - 1, cov (K, D, D) and ``keys`` are ``psis_batched``'s; ``A_new`` (K, M, P) are
    the new rows, ``offset`` (K, M) is added to their linear predictor, ``y`` (K, M) their integer labels (None: no ``lpd`` /
    ``elpd``), ``counts`` (K,) the valid rows per problem (None: all M).  The cutpoints are coordinates of q_k, correlated with
    beta, so there is no one-dimensional quadrature: the predictive is a mean over S = ``num_draws`` draws of q_k.
    ``weights="uniform"``: one call of ``kl_draw_batched`` with ``psis_batched``'s seed rule (seed (keys[k] % 2**32) ^
    0x5DEECE66D, draw number ``call``: the bits ``psis_batched`` would draw), no call of ``target.lp``, then one launch,
    gsmvi_ordinal_predict_batched_f64 (the definition is in include/gsmvi_hip.h): the linear predictor of every (draw, row) on the
    fp64 MFMA, the draw's cutpoints as one chain, the class probabilities as products of sigmoids (no two probabilities are
    subtracted) summed over the draws, and the log-sum-exp of the rows' log likelihoods; no (K, S, M, C) block is formed.
    ``weights="psis"``: first ``psis_batched(target.lp, mean, cov, keys, num_draws, call=call, moments=False, as_torch=True)``,
    then the launch with its smoothed ``log_weights``: the importance-corrected predictive; the result carries ``psis`` (khat,
    ``ok``), and a problem whose problem-level run failed comes out NaN.  ``psis=``, the result of such a call, is reused
    (``num_draws`` and ``call`` are then not used): its draws alone with ``"uniform"``, its weights too with ``"psis"``.  mean
    and cov are only read.
    An ``A_new`` that is not (K, M, P), a mean that is not (K, D) of the target, a cov that is not (K, D, D), an ``offset`` that is
    not (K, M) or not finite in the valid rows, labels that are not (K, M) or outside 0 .. C - 1 in the valid rows, bad
    ``counts``, keys of another length than K, ``num_draws`` outside 5..4096, an unknown ``weights`` or a ``psis`` that is not a
    ``PSISBatchedResult`` holding device tensors of the right shapes raise ValueError naming the argument before any device
    work."""
    fn = "predict_ordinal_batched"
    if not isinstance(target, BatchedOrdinalTarget):
        raise TypeError(f"{fn}: target must be a BatchedOrdinalTarget, got {type(target).__name__}")
    C = target.C
    a = _predict_draws_args(fn, target, mean, cov, A_new, keys, offset, y, lambda y, live: _check_labels(y, C, live), counts,
                            num_draws, call, psis, weights, engine)
    eng = a.eng
    prob, lpd = eng.ordinal_predict_batched(a.X, a.lw, a.A_new, C, y=eng.batched_labels(a.y) if a.y is not None else None,
                                            offset=a.offset, counts=a.counts_dev)
    pt, dead, label = _first_maximum(prob)
    # the smallest c whose cumulative probability reaches 0.5: the classes before it; C - 1 at the most (a cumulative sum that
    # rounds below 0.5 everywhere cannot happen for a row that sums to 1, the clamp costs nothing)
    median = torch.where(dead, label.new_full((), -1), (torch.cumsum(pt, 2) < 0.5).sum(2).clamp(max=C - 1))
    return _predict_draws_result(OrdinalPrediction, a, dict(prob=prob, label=label, median=median), lpd, as_torch,
                                 ints=("label", "median"))
