#!/usr/bin/env python3
"""Does the shape parameter earn its place?  K count data sets, half drawn Poisson and half negative binomial with a size r of
about 2, are each fitted twice with ``GSMBatch``: as a Poisson regression (``BatchedGLMTarget("poisson")``, D = P) and as a negative
binomial regression (``BatchedNegBinomialTarget``, D = P + 1: the coefficients and the log size).  ``psis_loo_batched`` and
``psis_loo_negbin_batched`` then give the PSIS leave-one-out log predictive density of every observation under each model.  Both
include -lgamma(y + 1), so the two elpd_loo are on one scale and their difference answers the question.  Printed per problem:
Delta elpd_loo = NB - Poisson and the paired standard error sqrt(n var(elpd_i^NB - elpd_i^Pois)); then per half the median
difference and the share of problems that favour the negative binomial model by more than two standard errors.  The
overdispersed half favours it by several standard errors; the Poisson half does not.

    python examples/loo_negbin_batched.py [K] [P] [N] [batch] [niter] [draws]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
P = int(sys.argv[2]) if len(sys.argv) > 2 else 3
N = int(sys.argv[3]) if len(sys.argv) > 3 else 150
batch = int(sys.argv[4]) if len(sys.argv) > 4 else 8
niter = int(sys.argv[5]) if len(sys.argv) > 5 else 200
draws = int(sys.argv[6]) if len(sys.argv) > 6 else 1024

rs = np.random.RandomState(1)
A = np.concatenate([np.ones((K, N, 1)), rs.standard_normal((K, N, P - 1))], axis=2)
beta = np.concatenate([1.5 + 0.3 * rs.standard_normal((K, 1)), 0.4 * rs.standard_normal((K, P - 1))], axis=1)
mu = np.exp(np.einsum("knp,kp->kn", A, beta))
over = np.arange(K) >= K // 2                            # the second half is overdispersed
size = np.exp(np.log(2.0) + 0.2 * rs.standard_normal(K))
rate = np.where(over[:, None], rs.gamma(size[:, None], mu / size[:, None]), mu)
y = rs.poisson(rate).astype(np.float64)
keys = np.arange(K) + 7


def fit_and_score(name, tgt, loo):
    m0, c0, res = gsmvi_amd.lbfgs_init_batched(np.zeros((K, tgt.D)), tgt.lp, tgt.lp_g)
    mean, cov = gsmvi_amd.GSMBatch(K, tgt.D, tgt.lp, tgt.lp_g).fit(keys, mean=m0, cov=c0, batch_size=batch, niter=niter,
                                                                    verbose=False)
    r = loo(tgt, mean, cov, keys, num_draws=draws)
    worst = np.nanmax(np.where(r.info == -3, np.nan, r.khat), axis=1)
    print(f"{name}: D = {tgt.D}, L-BFGS converged in {int(res.success.sum())} of {K}; {r.nlaunch} launches for {K * N} Pareto fits; "
          f"ok {r.ok.mean():6.1%}; largest pointwise khat, quartiles "
          f"{np.array2string(np.percentile(worst, [25, 50, 75]), precision=2)} (threshold {r.threshold:.3f})")
    return r, mean


pois, _ = fit_and_score("poisson          ", gsmvi_amd.BatchedGLMTarget(A, y, "poisson", prior_precision=1.0), gsmvi_amd.psis_loo_batched)
nb, mean_nb = fit_and_score("negative binomial", gsmvi_amd.BatchedNegBinomialTarget(A, y, prior_precision=1.0, log_size_mean=2.0,
                                                                                 log_size_precision=0.25),
                            gsmvi_amd.psis_loo_negbin_batched)
diff = nb.elpd_loo - pois.elpd_loo
se = np.sqrt(N * np.var(nb.elpd_i - pois.elpd_i, axis=1, ddof=1))               # the pointwise differences are paired
print("problem  data     fitted log r   elpd_loo NB   elpd_loo Pois   Delta = NB - Pois   +- se    Delta / se")
for k in range(K):
    print(f"{k:6d}   {'negbin ' if over[k] else 'poisson'}  {mean_nb[k, -1]:10.2f}   {nb.elpd_loo[k]:11.2f}   {pois.elpd_loo[k]:13.2f}   "
          f"{diff[k]:17.2f}   {se[k]:5.2f}   {diff[k] / se[k]:8.2f}")
for name, half in (("poisson data", ~over), ("negative binomial data (r about 2)", over)):
    z = diff[half] / se[half]
    print(f"{name}: median Delta elpd_loo {np.median(diff[half]):7.2f} +- {np.median(se[half]):5.2f}, median Delta / se "
          f"{np.median(z):6.2f}, NB favoured by more than 2 se in {int((z > 2.0).sum())} of {int(half.sum())}")
