#!/usr/bin/env python3
"""Comparing fitted classification models without held-out rows: K three-class multinomial logit posteriors are fitted by
``laplace_init_softmax_batched`` -> a short ``GSMBatch.fit``; ``psis_loo_softmax_batched`` then draws S points of every q_k and, in
one launch after the PSIS check of q_k itself, gives the PSIS leave-one-out log predictive density of every observation.  Printed
per model: elpd_loo +- se and p_loo of the first problems, the share of problems that are ``ok`` (q_k usable and every pointwise
khat below the threshold) and the quartiles of the largest pointwise khat.  A second model drops the last feature column; the
per-problem difference of elpd_loo, with the standard error of the pointwise differences, says which problems needed it (the
data are generated with coefficients on it in every other problem only).

    python examples/loo_softmax_batched.py [K] [P] [N] [batch] [niter] [draws]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
N = int(sys.argv[3]) if len(sys.argv) > 3 else 150
batch = int(sys.argv[4]) if len(sys.argv) > 4 else 8
niter = int(sys.argv[5]) if len(sys.argv) > 5 else 200
draws = int(sys.argv[6]) if len(sys.argv) > 6 else 1024
C = 3

rs = np.random.RandomState(1)
A = 2.0 * rs.standard_normal((K, N, P)) / np.sqrt(P)
W = rs.standard_normal((K, C - 1, P))
W[::2, :, P - 1] = 0.0                                   # every other problem does not use the last column
eta = np.concatenate([np.einsum("knp,kcp->knc", A, W), np.zeros((K, N, 1))], axis=2)
prob = np.exp(eta - eta.max(axis=2, keepdims=True))
cdf = np.cumsum(prob / prob.sum(axis=2, keepdims=True), axis=2)
y = np.minimum((rs.random_sample((K, N, 1)) > cdf).sum(axis=2), C - 1)
keys = np.arange(K) + 7


def fit_and_score(name, Am):
    d = (C - 1) * Am.shape[2]
    tgt = gsmvi_amd.BatchedSoftmaxTarget(Am, y, C, prior_precision=1.0)
    m0, c0, res = gsmvi_amd.laplace_init_softmax_batched(tgt)
    mean, cov = gsmvi_amd.GSMBatch(K, d, tgt.lp, tgt.lp_g).fit(keys, mean=m0, cov=c0, batch_size=batch, niter=niter, verbose=False)
    r = gsmvi_amd.psis_loo_softmax_batched(tgt, mean, cov, keys, num_draws=draws)
    worst = np.nanmax(np.where(r.info == -3, np.nan, r.khat), axis=1)
    print(f"{name}: D = {d}, Laplace converged in {int(res.success.sum())} of {K}; {r.nlaunch} launches for {K * N} Pareto fits; "
          f"threshold for khat {r.threshold:.3f}")
    print(f"  ok {r.ok.mean():6.1%}   largest pointwise khat, quartiles {np.array2string(np.percentile(worst, [25, 50, 75]), precision=2)}"
          f"   rows over the threshold {int(r.n_bad.sum())} of {K * N}")
    for k in range(min(K, 4)):
        print(f"  problem {k}: elpd_loo {r.elpd_loo[k]:8.2f} +- {r.se[k]:5.2f}   p_loo {r.p_loo[k]:5.2f}")
    return r


full = fit_and_score("full model", A)
small = fit_and_score("last column dropped", A[:, :, :P - 1])
diff = full.elpd_loo - small.elpd_loo
se_diff = np.sqrt(N * np.var(full.elpd_i - small.elpd_i, axis=1, ddof=1))       # the pointwise differences are paired
print(f"elpd_loo(full) - elpd_loo(dropped): median {np.median(diff[1::2]):7.2f} +- {np.median(se_diff[1::2]):5.2f} where the column "
      f"carries coefficients, {np.median(diff[::2]):7.2f} +- {np.median(se_diff[::2]):5.2f} where it does not")
