#!/usr/bin/env python3
"""K overdispersed count data sets, each fitted twice: with the Poisson target (BatchedGLMTarget, whose variance is pinned to its
mean) and with BatchedNegBinomialTarget, which fits the size r = exp(theta) beside the coefficients -- what
examples/example_gsm.py does for one model (its log_prob and jit(grad(.)) handed to the fit), every posterior of a family scored
in one HIP launch per call.  Problem k has counts y_kn ~ NB(mu = exposure_kn exp(a_kn . beta_k), r_k): variance mu + mu^2 / r_k;
the log exposure is the offset.  Both families start from ``lbfgs_init_batched`` and are fitted with ``GSMBatch``; the recovered
log r is printed against the truth, and ``psis_batched`` says of each fit how far its Gaussian is from its own posterior.  A
Poisson posterior on such data is sharply peaked in the wrong place: its khat may look fine (the Gaussian fits the wrong
posterior well), which is why the comparison that matters is the coefficients' standard deviations and the recovered size.

    python examples/negbin_batched.py [K] [P] [N] [batch] [niter]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 32
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
N = int(sys.argv[3]) if len(sys.argv) > 3 else 300
batch = int(sys.argv[4]) if len(sys.argv) > 4 else 8
niter = int(sys.argv[5]) if len(sys.argv) > 5 else 400
LAM = 0.1

rs = np.random.RandomState(4)
A = np.concatenate([np.ones((K, N, 1)), rs.standard_normal((K, N, P - 1))], axis=2)
beta = np.concatenate([1.5 + 0.5 * rs.standard_normal((K, 1)), 0.4 * rs.standard_normal((K, P - 1))], axis=1)
log_r = rs.uniform(0.0, 2.5, K)                           # sizes from 1 (heavily overdispersed) to 12
exposure = rs.uniform(0.5, 4.0, size=(K, N))
offset = np.log(exposure)
mu = exposure * np.exp(np.einsum("knp,kp->kn", A, beta))
r = np.exp(log_r)[:, None]
y = rs.poisson(rs.gamma(r, mu / r)).astype(np.float64)
keys = np.arange(K) + 7


def fit(target, D):
    mean0, cov0, res = gsmvi_amd.lbfgs_init_batched(np.zeros((K, D)), target.lp, target.lp_g)
    f = gsmvi_amd.GSMBatch(K, D, target.lp, target.lp_g)
    mean, cov = f.fit(keys, mean=mean0, cov=cov0, batch_size=batch, niter=niter, verbose=False)
    ps = gsmvi_amd.psis_batched(target.lp, mean, cov, keys, num_draws=1024, moments=False)
    return mean, cov, res, ps, int(f.n_reverts.sum())


pois = gsmvi_amd.BatchedGLMTarget(A, y, "poisson", prior_precision=LAM, offset=offset)
nb = gsmvi_amd.BatchedNegBinomialTarget(A, y, prior_precision=LAM, offset=offset, log_size_mean=0.0, log_size_precision=0.01)
mp, cp, rp, pp, vp = fit(pois, P)
mn, cn, rn, pn, vn = fit(nb, P + 1)

sd_p, sd_n = np.sqrt(np.einsum("kii->ki", cp)), np.sqrt(np.einsum("kii->ki", cn))
z = (mn[:, P] - log_r) / sd_n[:, P]
print(f"lbfgs_init_batched converged: poisson {int(rp.success.sum())} of {K}, negative binomial {int(rn.success.sum())} of {K}; "
      f"reverts {vp} and {vn}")
print(f"recovered log r against the truth, in fitted standard deviations: median |z| {np.median(np.abs(z)):.2f}, max {np.abs(z).max():.2f}")
print(f"slope coefficients against the truth, in fitted standard deviations (max over problems and slopes): "
      f"poisson {(np.abs(mp[:, 1:] - beta[:, 1:]) / sd_p[:, 1:]).max():.1f}, "
      f"negative binomial {(np.abs(mn[:, 1:P] - beta[:, 1:]) / sd_n[:, 1:P]).max():.1f}")
print(f"psis_batched khat (threshold {pn.threshold:.2f}): poisson median {np.median(pp.khat):.2f} max {pp.khat.max():.2f}; "
      f"negative binomial median {np.median(pn.khat):.2f} max {pn.khat.max():.2f}")
print("problem   true log r   fitted log r (sd)     khat poisson   khat negbin   sd of slope 1: poisson / negbin")
for k in range(min(K, 8)):
    print(f"{k:7d}   {log_r[k]:10.3f}   {mn[k, P]:+.3f} ({sd_n[k, P]:.3f})      {pp.khat[k]:12.2f}   {pn.khat[k]:11.2f}   "
          f"{sd_p[k, 1]:.4f} / {sd_n[k, 1]:.4f}")
