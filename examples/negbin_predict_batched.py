#!/usr/bin/env python3
"""K overdispersed count data sets (the model of examples/negbin_batched.py) fitted with ``laplace_init_negbin_batched`` and used
on held-out rows: ``predict_negbin_batched`` gives, from draws of q_k over (beta, log r), the predictive mean and variance of every
held-out count and the held-out elpd.  The same data fitted as a Poisson ``BatchedGLMTarget`` gives the comparison: its interval is
the one from ``predict``'s mean with the Poisson variance equal to the mean, which is too narrow for these counts.

    python examples/negbin_predict_batched.py [K] [P] [N] [M]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 32
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
N = int(sys.argv[3]) if len(sys.argv) > 3 else 300
M = int(sys.argv[4]) if len(sys.argv) > 4 else 100

rs = np.random.RandomState(4)
A = np.concatenate([np.ones((K, N + M, 1)), rs.standard_normal((K, N + M, P - 1))], axis=2)
beta = np.concatenate([1.5 + 0.5 * rs.standard_normal((K, 1)), 0.4 * rs.standard_normal((K, P - 1))], axis=1)
log_r = rs.uniform(0.0, 2.5, K)
offset = np.log(rs.uniform(0.5, 4.0, size=(K, N + M)))
mu = np.exp(np.einsum("knp,kp->kn", A, beta) + offset)
r = np.exp(log_r)[:, None]
y = rs.poisson(rs.gamma(r, mu / r)).astype(np.float64)
keys = np.arange(K) + 7
A_fit, y_fit, o_fit = A[:, :N], y[:, :N], offset[:, :N]
A_new, y_new, o_new = A[:, N:], y[:, N:], offset[:, N:]

target = gsmvi_amd.BatchedNegBinomialTarget(A_fit, y_fit, prior_precision=0.1, offset=o_fit, log_size_mean=0.0, log_size_precision=1.0)
mean, cov, res = gsmvi_amd.laplace_init_negbin_batched(target)
pred = gsmvi_amd.predict_negbin_batched(target, mean, cov, A_new, keys, offset=o_new, y=y_new, num_draws=1024)
inside_nb = (np.abs(y_new - pred.mean) <= 2.0 * np.sqrt(pred.var)).mean(1)

poisson = gsmvi_amd.BatchedGLMTarget(A_fit, y_fit, "poisson", prior_precision=0.1, offset=o_fit)
pm, pc, pres = gsmvi_amd.laplace_init_batched(poisson)
pp = poisson.predict(pm, pc, A_new, offset=o_new, y=y_new)
inside_po = (np.abs(y_new - pp.mean) <= 2.0 * np.sqrt(pp.mean)).mean(1)

print(f"{K} problems, {N} training and {M} held-out rows each; negative binomial fits converged: {int(res.success.sum())}, Poisson: "
      f"{int(pres.success.sum())}; predict_negbin_batched: {pred.num_draws} draws, {pred.nlaunch} launches")
print("problem  true r   elpd / row (negbin)  elpd / row (poisson)  inside mean +- 2 sd: negbin  poisson")
for k in range(K):
    print(f"{k:7d}  {np.exp(log_r[k]):6.2f}   {pred.elpd[k] / M:19.3f}  {pp.elpd[k] / M:20.3f}  {inside_nb[k]:26.2f}  {inside_po[k]:7.2f}")
print(f"all      {'':6s}   {pred.elpd.sum() / (K * M):19.3f}  {pp.elpd.sum() / (K * M):20.3f}  {inside_nb.mean():26.2f}  {inside_po.mean():7.2f}")
