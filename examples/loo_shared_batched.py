#!/usr/bin/env python3
"""Which prior precision predicts best?  One logistic regression data set, K values of lambda on a log grid: a
``SharedDesignGLMTarget`` holds the design once, ``laplace_init_shared_batched`` gives the K Gaussians in a handful of launches and
``psis_loo_shared_batched`` the PSIS leave-one-out log predictive density of every observation under every lambda in one more,
with no copy of the design per problem.  Printed per lambda: elpd_loo +- se, p_loo, the largest pointwise khat, and Delta elpd
against the best lambda with the PAIRED standard error sqrt(n var(elpd_i - elpd_i^best)) -- the K fits score the same rows, so
the pointwise differences are what carries the comparison.

    python examples/loo_shared_batched.py [K] [N] [D] [draws]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 16
N = int(sys.argv[2]) if len(sys.argv) > 2 else 200
D = int(sys.argv[3]) if len(sys.argv) > 3 else 20
draws = int(sys.argv[4]) if len(sys.argv) > 4 else 1024

rs = np.random.RandomState(4)
A = rs.standard_normal((N, D)) / np.sqrt(D)
theta = np.where(np.arange(D) < 4, 3.0, 0.0) * rs.standard_normal(D)     # four covariates matter, the rest is noise
y1 = (rs.random_sample(N) < 1.0 / (1.0 + np.exp(-A @ theta))).astype(np.float64)
y = np.ascontiguousarray(np.broadcast_to(y1, (K, N)))                    # the same responses for every lambda
lam = 10.0 ** np.linspace(-3, 3, K)
keys = np.arange(K) + 11

tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, "logistic", prior_precision=lam)
mean, cov, res = gsmvi_amd.laplace_init_shared_batched(tgt)
r = gsmvi_amd.psis_loo_shared_batched(tgt, mean, cov, keys, num_draws=draws)
print(f"{K} values of lambda on one design (N, D) = ({N}, {D}), held once: {A.nbytes / 1e3:.1f} kB against {K * A.nbytes / 1e3:.1f} kB "
      f"replicated; Laplace converged in {int(res.success.sum())} of {K} ({res.nlaunch} launches), then {r.nlaunch} launches for "
      f"{K * N} Pareto fits")
best = int(np.argmax(r.elpd_loo))
diff = r.elpd_loo - r.elpd_loo[best]
se_diff = np.sqrt(N * np.var(r.elpd_i - r.elpd_i[best], axis=1, ddof=1))
print("     lambda   elpd_loo  +- se    p_loo   max khat  ok    Delta elpd  +- se (paired)")
for k in range(K):
    mark = "  <- best" if k == best else ""
    print(f"{lam[k]:11.4g}  {r.elpd_loo[k]:9.2f}  {r.se[k]:5.2f}  {r.p_loo[k]:7.2f}  {np.max(r.khat[k]):9.2f}  {str(bool(r.ok[k])):5s} "
          f"{diff[k]:10.2f}  {se_diff[k]:5.2f}{mark}")
close = np.flatnonzero(diff > -2.0 * np.maximum(se_diff, 1e-12))
print(f"best lambda {lam[best]:.3g} (p_loo {r.p_loo[best]:.1f} of D = {D}); within two paired standard errors of it: lambda in "
      f"[{lam[close].min():.3g}, {lam[close].max():.3g}]")
