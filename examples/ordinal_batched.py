#!/usr/bin/env python3
"""K small rating data sets (C ordered categories: a Likert item, a grade, a severity score), each fitted with
BatchedOrdinalTarget, the cumulative-logit (proportional odds) model -- what examples/example_gsm.py does for one model (its
log_prob and jit(grad(.)) handed to the fit), every posterior scored in one HIP launch per call.  Problem k has labels y_kn with
P(y_kn <= c) = sigmoid(cut_kc - a_kn . beta_k) at planted slopes beta_k and planted ordered cutpoints cut_k.  The parameter is
x = (beta, delta), cut_0 = delta_0 and cut_j = cut_{j-1} + exp(delta_j): ``lbfgs_init_batched`` finds the modes, ``GSMBatch.fit``
the Gaussians, ``target.cutpoints(mean)`` reads the fitted cutpoints, and ``psis_batched`` says of each fit how far its Gaussian
is from its own posterior.

    python examples/ordinal_batched.py [K] [P] [C] [N] [batch] [niter]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 32
P = int(sys.argv[2]) if len(sys.argv) > 2 else 3
C = int(sys.argv[3]) if len(sys.argv) > 3 else 5
N = int(sys.argv[4]) if len(sys.argv) > 4 else 400
batch = int(sys.argv[5]) if len(sys.argv) > 5 else 8
niter = int(sys.argv[6]) if len(sys.argv) > 6 else 300
D = P + C - 1

rs = np.random.RandomState(4)
A = rs.standard_normal((K, N, P))                                   # no intercept column: the cutpoints are the intercepts
beta = 0.8 * rs.standard_normal((K, P))
cuts = np.sort(np.linspace(-1.8, 1.8, C - 1)[None, :] + 0.25 * rs.standard_normal((K, C - 1)), axis=1)
eta = np.einsum("knp,kp->kn", A, beta)
cdf = 1.0 / (1.0 + np.exp(-(cuts[:, None, :] - eta[:, :, None])))   # P(y <= c)
y = (rs.random_sample((K, N))[:, :, None] > cdf).sum(2)
keys = np.arange(K) + 7

target = gsmvi_amd.BatchedOrdinalTarget(A, y, C, prior_precision=0.1, cut_precision=0.01)
mean0, cov0, res = gsmvi_amd.lbfgs_init_batched(np.zeros((K, D)), target.lp, target.lp_g)
fit = gsmvi_amd.GSMBatch(K, D, target.lp, target.lp_g)
mean, cov = fit.fit(keys, mean=mean0, cov=cov0, batch_size=batch, niter=niter, verbose=False)
ps = gsmvi_amd.psis_batched(target.lp, mean, cov, keys, num_draws=1024, moments=False)

got = target.cutpoints(mean)
sd = np.sqrt(np.einsum("kii->ki", cov))
ok = np.asarray(ps.ok)
print(f"lbfgs_init_batched converged: {int(res.success.sum())} of {K}; reverts {int(fit.n_reverts.sum())}")
print(f"cutpoints against the planted ones: median |error| {np.median(np.abs(got - cuts)):.3f}, max {np.abs(got - cuts).max():.3f}")
print(f"slopes against the planted ones, in fitted standard deviations: max {(np.abs(mean[:, :P] - beta) / sd[:, :P]).max():.1f}")
print(f"psis_batched khat (threshold {ps.threshold:.2f}): median {np.median(ps.khat):.2f} max {ps.khat.max():.2f}; "
      f"ok: {int(ok.sum())} of {K} ({100.0 * ok.mean():.0f}%)")
print("problem   planted cutpoints" + " " * (8 * (C - 1) - 15) + "fitted cutpoints" + " " * (8 * (C - 1) - 14) + "khat")
for k in range(min(K, 8)):
    print(f"{k:7d}   " + " ".join(f"{v:+7.3f}" for v in cuts[k]) + "   " + " ".join(f"{v:+7.3f}" for v in got[k]) + f"   {ps.khat[k]:5.2f}")
