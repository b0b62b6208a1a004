#!/usr/bin/env python3
"""Does a covariate earn its place?  K ordered-category data sets (C classes: ratings, grades) are drawn from a cumulative-logit
model in which the LAST column of the design acts in the first half of the problems and has no effect in the second half.  Each
data set is fitted twice with ``GSMBatch`` on a ``BatchedOrdinalTarget``: with all P columns (D = P + C - 1) and without the last
one (D = P + C - 2).  ``psis_loo_ordinal_batched`` then gives the PSIS leave-one-out log predictive density of every observation
under each model.  Both are logs of normalised categorical probabilities, so the two elpd_loo are on one scale and their
difference answers the question.  Printed per problem: Delta elpd_loo = full - reduced and the paired standard error
sqrt(n var(elpd_i^full - elpd_i^reduced)); then per half the median difference and the share of problems that favour the full
model by more than two standard errors.  Where the covariate acts the full model wins by several standard errors; where it does
not, the reduced model is as good or slightly better.

    python examples/loo_ordinal_batched.py [K] [P] [C] [N] [batch] [niter] [draws]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
P = int(sys.argv[2]) if len(sys.argv) > 2 else 3
C = int(sys.argv[3]) if len(sys.argv) > 3 else 5
N = int(sys.argv[4]) if len(sys.argv) > 4 else 200
batch = int(sys.argv[5]) if len(sys.argv) > 5 else 8
niter = int(sys.argv[6]) if len(sys.argv) > 6 else 200
draws = int(sys.argv[7]) if len(sys.argv) > 7 else 1024

rs = np.random.RandomState(1)
A = rs.standard_normal((K, N, P))
acts = np.arange(K) < K // 2                             # the last covariate acts in the first half
beta = 0.6 * rs.standard_normal((K, P))
beta[:, -1] = np.where(acts, 0.9 * np.where(rs.random_sample(K) < 0.5, -1.0, 1.0), 0.0)
cuts = np.sort(1.5 * rs.standard_normal((K, C - 1)), axis=1)
eta = np.einsum("knp,kp->kn", A, beta)
cdf = 1.0 / (1.0 + np.exp(-(cuts[:, None, :] - eta[:, :, None])))              # P(y <= j)
y = (rs.random_sample((K, N))[:, :, None] > cdf).sum(2)
keys = np.arange(K) + 7


def fit_and_score(name, tgt):
    m0, c0, res = gsmvi_amd.lbfgs_init_batched(np.zeros((K, tgt.D)), tgt.lp, tgt.lp_g)
    mean, cov = gsmvi_amd.GSMBatch(K, tgt.D, tgt.lp, tgt.lp_g).fit(keys, mean=m0, cov=c0, batch_size=batch, niter=niter,
                                                                    verbose=False)
    r = gsmvi_amd.psis_loo_ordinal_batched(tgt, mean, cov, keys, num_draws=draws)
    worst = np.nanmax(np.where(r.info == -3, np.nan, r.khat), axis=1)
    print(f"{name}: D = {tgt.D}, L-BFGS converged in {int(res.success.sum())} of {K}; {r.nlaunch} launches for {K * N} Pareto fits; "
          f"ok {r.ok.mean():6.1%}; largest pointwise khat, quartiles "
          f"{np.array2string(np.percentile(worst, [25, 50, 75]), precision=2)} (threshold {r.threshold:.3f})")
    return r, mean


full, mean_full = fit_and_score("all P columns     ", gsmvi_amd.BatchedOrdinalTarget(A, y, C, prior_precision=1.0, cut_precision=0.25))
red, _ = fit_and_score("without the last  ", gsmvi_amd.BatchedOrdinalTarget(A[:, :, :P - 1].copy(), y, C, prior_precision=1.0,
                                                                            cut_precision=0.25))
diff = full.elpd_loo - red.elpd_loo
se = np.sqrt(N * np.var(full.elpd_i - red.elpd_i, axis=1, ddof=1))              # the pointwise differences are paired
print("problem  covariate   fitted beta_last   elpd_loo full   elpd_loo reduced   Delta = full - reduced   +- se    Delta / se")
for k in range(K):
    print(f"{k:6d}   {'acts   ' if acts[k] else 'is null'}   {mean_full[k, P - 1]:14.2f}   {full.elpd_loo[k]:13.2f}   "
          f"{red.elpd_loo[k]:16.2f}   {diff[k]:22.2f}   {se[k]:5.2f}   {diff[k] / se[k]:8.2f}")
for name, half in (("the covariate acts (|beta| = 0.9)", acts), ("the covariate has no effect", ~acts)):
    z = diff[half] / se[half]
    print(f"{name}: median Delta elpd_loo {np.median(diff[half]):7.2f} +- {np.median(se[half]):5.2f}, median Delta / se "
          f"{np.median(z):6.2f}, full model favoured by more than 2 se in {int((z > 2.0).sum())} of {int(half.sum())}")
