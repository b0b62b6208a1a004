"""gsmvi_amd: MI355X-native GSM / BaM update engine behind the GSM-VI Python API.

Mirrors the reference's public surface for the hot path (reference file:line):
    GSM, gsm_update                              gsmvi/gsm.py:31-133, gsmvi/gsm_numpy.py:27-129
    gsm_update_batched, GSMBatch,
    BatchedGaussianTarget (K problems at once,
    D <= 64: jax.vmap(gsm_update) and its fit)   gsmvi/gsm.py:31-58, gsmvi/gsm_numpy.py:77-129
    bam_update_batched, BaMBatch (K problems at
    once, D <= 64: jax.vmap(bam_update) and the
    dense BaM loop, no retries)                  gsmvi/bam.py:31-114, gsmvi/bam.py:140-216
    BaM, bam_update, bam_lowrank_update,
    Regularizers                                 gsmvi/bam.py:31-274
    KLMonitor (diagnostics callback, host side),
    DeviceKLMonitor (same protocol, on the GPU)  gsmvi/monitors.py:43-125
    BatchedKLMonitor (the same for the K problems
    of GSMBatch / BaMBatch, one launch per chunk) gsmvi/monitors.py:43-125
    ADVIBatch, Adam (the ELBO baseline for K
    problems at once, D <= 64: closed-form
    gradient + Adam in one launch per iteration) gsmvi/advi.py:8-112
    BatchedLogisticTarget (K Bayesian logistic
    regressions, D <= 64: log-density and score
    of all of them in one launch -- the lp / lp_g
    of the three batched fits and the monitor)   examples/example_gsm.py:34-35 (log_prob, jit(grad(.)))
    BatchedGLMTarget (the same launch for K
    Poisson, probit, Gaussian or logistic
    regressions with offsets)                    examples/example_gsm.py:34-35 (log_prob, jit(grad(.)))
    SharedDesignGLMTarget (K such regressions on
    ONE design matrix, with observation weights:
    both products on the fp64 MFMA, no copy of A) examples/example_gsm.py:34-35 (log_prob, jit(grad(.)))
    BatchedSoftmaxTarget (K multinomial logit
    regressions of C classes, (C - 1) P <= 64:
    log-density and score in one launch)         examples/example_gsm.py:34-35 (log_prob, jit(grad(.)))
    BatchedNegBinomialTarget (K negative binomial
    regressions with a fitted log size, P + 1 <= 64:
    log-density and score in one launch)         examples/example_gsm.py:34-35 (log_prob, jit(grad(.)))
    BatchedOrdinalTarget (K cumulative-logit
    regressions of C ordered classes, P + C - 1 <= 64:
    log-density and score in one launch)         examples/example_gsm.py:34-35 (log_prob, jit(grad(.)))
    BatchedGLMTarget.predict, GLMPrediction (the
    posterior predictive of K fitted GLMs on new
    rows: mean, variance of the linear predictor,
    predictive mean, held-out elpd; one launch)  examples/example_gsm.py:34-35, the use of the fit; no reference twin
    psis_batched, psis_weights_batched,
    PSISBatchedResult (is the fitted q_k usable?
    Pareto-smoothed importance diagnostic of K
    Gaussians: khat, ess, log Z, corrected
    moments; one launch after the target's lp)   gsmvi/monitors.py:83-125 (the role; no reference twin)
    psis_loo_batched, LOOBatchedResult,
    BatchedGLMTarget.loo (PSIS leave-one-out of K
    fitted GLM posteriors: elpd_loo, p_loo, se and
    the pointwise khat; one launch after psis_batched) examples/example_gsm.py:34-35, comparing fitted models; no reference twin
    psis_loo_softmax_batched (the same for K fitted
    multinomial logit posteriors: the class-coupled
    pointwise likelihood on the fp64 MFMA; one launch) examples/example_gsm.py:34-35, comparing fitted models; no reference twin
    psis_loo_negbin_batched (the same for K fitted
    negative binomial posteriors, -lgamma(y + 1)
    included: on one scale with the Poisson GLM's) examples/example_gsm.py:34-35, comparing fitted models; no reference twin
    psis_loo_ordinal_batched (the same for K fitted
    cumulative-logit posteriors over (beta, cutpoints):
    on one scale with the multinomial logit's)     examples/example_gsm.py:34-35, comparing fitted models; no reference twin
    psis_loo_shared_batched (the same for K fitted
    GLM posteriors on ONE design matrix, observation
    weights honoured, no copy of A per problem)    examples/example_gsm.py:34-35, comparing fitted models; no reference twin
    predict_softmax_batched, SoftmaxPrediction (the
    posterior predictive of K fitted multinomial
    logit posteriors on new rows, from draws of q_k,
    uniform or PSIS-weighted: class probabilities,
    labels, held-out elpd; one launch after the draws) examples/example_gsm.py:34-35, the use of the fit; no reference twin
    predict_negbin_batched, NegBinPrediction (the same
    for K fitted negative binomial posteriors: mean and
    variance of the predictive count from three log
    moments, held-out elpd on the leave-one-out's scale) examples/example_gsm.py:34-35, the use of the fit; no reference twin
    predict_ordinal_batched, OrdinalPrediction (the same
    for K fitted cumulative-logit posteriors: class
    probabilities, most probable and median class,
    held-out elpd on the leave-one-out's scale)          examples/example_gsm.py:34-35, the use of the fit; no reference twin
    predict_shared_batched (the GLM predictive of K
    fitted posteriors of a SharedDesignGLMTarget on
    ONE set of new rows with per-problem row weights:
    the held-out score of K-fold cross-validation;
    one launch, no copy of the rows per problem)   examples/example_gsm.py:34-35, the use of the fit; no reference twin
    lbfgs_init_batched (the L-BFGS initialiser
    for K problems at once, D <= 64: one launch
    per function evaluation after lp_g and lp)   gsmvi/initializers.py:5-17
    pathfinder_init_batched, PathfinderBatchedResult
    (single-path Pathfinder for K problems, D <= 64:
    the Gaussian along the L-BFGS path with the best
    ELBO estimate; two launches per round more)  gsmvi/initializers.py:5-17 (the role; no reference twin)
    laplace_init_batched (the Newton mode and the
    inverse Hessian of K GLM posteriors, D <= 64:
    one launch per round, fp64-MFMA Gram product) gsmvi/initializers.py:5-17 (the role; no reference twin)
    laplace_init_softmax_batched (the same start
    for K multinomial logit posteriors, D <= 64,
    and BatchedSoftmaxTarget.neg_hessian)        gsmvi/initializers.py:5-17 (the role; no reference twin)
    laplace_init_shared_batched (the same start
    for K GLM posteriors on ONE design matrix, and
    neg_hessian_shared_batched: one staged tile of
    the design per workgroup, no copy per problem) gsmvi/initializers.py:5-17 (the role; no reference twin)
    laplace_init_negbin_batched (the same start for
    K negative binomial posteriors, with a modified
    last pivot where theta has no curvature, and
    neg_hessian_negbin_batched: the bordered Hessian) gsmvi/initializers.py:5-17 (the role; no reference twin)
    laplace_init_ordinal_batched (the same start for
    K cumulative-logit posteriors, with one retry
    without the negative chain terms of the gaps, and
    neg_hessian_ordinal_batched)                 gsmvi/initializers.py:5-17 (the role; no reference twin)
    lbfgs_init, ADVI (initialiser and the ELBO
    baseline of the examples; off the hot path)  gsmvi/initializers.py:5-17, gsmvi/advi.py:8-112
All GSM / BaM numerics run in hand-written HIP kernels (libgsmvi_hip.so, C ABI in include/gsmvi_hip.h)
called through ctypes; torch is used for device memory, streams and torch.distributed only.
There is no CPU fallback: without the library or a GPU every compute entry point raises.
(lbfgs_init and ADVI are the examples' comparison tools, not the update path: scipy / torch autograd.)
"""
from ._lib import load_library, library_path, GsmviError            # noqa: F401
from .engine import HipEngine, get_engine                            # noqa: F401
from .gsm import GSM, gsm_update                                     # noqa: F401
from .bam import BaM, bam_update, bam_lowrank_update, Regularizers   # noqa: F401
from .targets import GaussianTarget, device_score, score_from_logp   # noqa: F401
from .targets import BatchedGaussianTarget, BatchedLogisticTarget    # noqa: F401
from .targets import BatchedGLMTarget, GLMPrediction                 # noqa: F401
from .targets import BatchedSoftmaxTarget                            # noqa: F401
from .targets import SharedDesignGLMTarget                           # noqa: F401
from .targets import BatchedNegBinomialTarget                        # noqa: F401
from .targets import BatchedOrdinalTarget                            # noqa: F401
from .targets import predict_softmax_batched, SoftmaxPrediction      # noqa: F401
from .targets import predict_negbin_batched, NegBinPrediction        # noqa: F401
from .targets import predict_ordinal_batched, OrdinalPrediction      # noqa: F401
from .targets import neg_hessian_shared_batched                      # noqa: F401
from .targets import predict_shared_batched                          # noqa: F401
from .targets import neg_hessian_negbin_batched                      # noqa: F401
from .targets import neg_hessian_ordinal_batched                     # noqa: F401
from .batched import GSMBatch, gsm_update_batched                    # noqa: F401
from .batched import BaMBatch, bam_update_batched, bam_lowrank_update_batched   # noqa: F401
from .batched import ADVIBatch, Adam                                 # noqa: F401
from .monitors import KLMonitor, DeviceKLMonitor, BatchedKLMonitor   # noqa: F401
from .initializers import lbfgs_init, lbfgs_init_batched, LbfgsBatchedResult   # noqa: F401
from .initializers import laplace_init_batched, LaplaceBatchedResult          # noqa: F401
from .initializers import laplace_init_softmax_batched                        # noqa: F401
from .initializers import laplace_init_shared_batched                         # noqa: F401
from .initializers import laplace_init_negbin_batched, LaplaceNegBinBatchedResult   # noqa: F401
from .initializers import laplace_init_ordinal_batched, LaplaceOrdinalBatchedResult   # noqa: F401
from .initializers import pathfinder_init_batched, PathfinderBatchedResult    # noqa: F401
from .diagnostics import psis_batched, psis_weights_batched, PSISBatchedResult   # noqa: F401
from .diagnostics import psis_loo_batched, LOOBatchedResult          # noqa: F401
from .diagnostics import psis_loo_softmax_batched                    # noqa: F401
from .diagnostics import psis_loo_negbin_batched                     # noqa: F401
from .diagnostics import psis_loo_ordinal_batched                    # noqa: F401
from .diagnostics import psis_loo_shared_batched                     # noqa: F401
from .advi import ADVI                                               # noqa: F401

__version__ = "0.1.0"
