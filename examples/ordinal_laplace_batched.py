#!/usr/bin/env python3
"""K ordered-category data sets (the cumulative-logit model of ``BatchedOrdinalTarget``) started with
``laplace_init_ordinal_batched``: Newton rounds on the closed-form Hessian, one HIP launch per round, with one retry without the
negative chain terms of the gaps where the Hessian is indefinite away from the mode -- the role of the reference's lbfgs_init
(gsmvi/initializers.py:5-17).  Then the chain the family now has: start -> ``GSMBatch.fit`` -> ``psis_loo_ordinal_batched``, with
``psis_batched`` saying of the start and of the fit how far each Gaussian is from its posterior.

    python examples/ordinal_laplace_batched.py [K] [P] [C] [N]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 32
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
C = int(sys.argv[3]) if len(sys.argv) > 3 else 8
N = int(sys.argv[4]) if len(sys.argv) > 4 else 400
D = P + C - 1

rs = np.random.RandomState(4)
A = rs.standard_normal((K, N, P))
beta = 0.8 * rs.standard_normal((K, P))
cuts = np.sort(1.5 * rs.standard_normal((K, C - 1)), axis=1)
eta = np.einsum("knp,kp->kn", A, beta)
cdf = 1.0 / (1.0 + np.exp(-(cuts[:, None, :] - eta[:, :, None])))           # P(y <= j)
y = (rs.random_sample((K, N))[:, :, None] > cdf).sum(2)
keys = np.arange(K) + 7

target = gsmvi_amd.BatchedOrdinalTarget(A, y, C, prior_precision=0.1, cut_precision=0.1)
mean, cov, res = gsmvi_amd.laplace_init_ordinal_batched(target)
print(f"laplace_init_ordinal_batched: {int(res.success.sum())} of {K} converged in {res.nlaunch} launches; Newton iterations "
      f"{int(res.nit.min())} - {int(res.nit.max())}; problems with a retried round: {int((res.nmod > 0).sum())} (on the way from "
      f"x0 = 0 their Hessian was indefinite: plain Newton would have stopped there)")
H = gsmvi_amd.neg_hessian_ordinal_batched(target, mean).cpu().numpy()
print(f"smallest eigenvalue of the negative Hessian at the modes: {min(np.linalg.eigvalsh(h).min() for h in H):.3g} (positive: modes)")
err = np.abs(target.cutpoints(mean) - cuts)
print(f"cutpoints against the truth: median |error| {np.median(err):.2f}, max {err.max():.2f}")
ps = gsmvi_amd.psis_batched(target.lp, mean, cov, keys, num_draws=1024, moments=False)
print(f"Laplace start: khat median {np.median(ps.khat):.2f}, max {ps.khat.max():.2f}, usable (below {ps.threshold:.2f}): "
      f"{int((ps.khat < ps.threshold).sum())} of {K}")
fit = gsmvi_amd.GSMBatch(K, D, target.lp, target.lp_g)
m1, c1 = fit.fit(keys, mean=mean, cov=cov, batch_size=8, niter=200, verbose=False)
ps = gsmvi_amd.psis_batched(target.lp, m1, c1, keys, num_draws=1024, moments=False)
print(f"after 200 GSM iterations from the Laplace start: khat median {np.median(ps.khat):.2f}, max {ps.khat.max():.2f}, reverts "
      f"{int(fit.n_reverts.sum())}")
loo = gsmvi_amd.psis_loo_ordinal_batched(target, m1, c1, keys, num_draws=1024)
print(f"psis_loo_ordinal_batched of the fits: elpd_loo per observation median {np.median(loo.elpd_loo) / N:.3f} "
      f"(log(1 / C) = {np.log(1.0 / C):.3f} is a guess at random)")
