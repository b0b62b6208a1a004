#!/usr/bin/env python3
"""K-fold cross-validation of the prior precision on one design, without a copy of it.  One logistic regression data set, F folds x
L values of lambda = F L problems of a ``SharedDesignGLMTarget``: problem (f, l) is fitted with the training weights 1 - mask_f by
``laplace_init_shared_batched`` and scored on its held-out rows by ``predict_shared_batched(target, mean, cov, target.A, y=...,
weights=mask_f)``, whose ``elpd`` is the sum of the log predictive densities of the fold's rows.  Summed over the folds it is the
K-fold estimate of the expected log predictive density of each lambda, printed beside the PSIS leave-one-out estimate
(``psis_loo_shared_batched``) of the L fits on all the data.  The two estimate the same quantity; nothing is asserted here.

    python examples/kfold_shared_batched.py [F] [L] [N] [D] [draws]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

F = int(sys.argv[1]) if len(sys.argv) > 1 else 5
L = int(sys.argv[2]) if len(sys.argv) > 2 else 8
N = int(sys.argv[3]) if len(sys.argv) > 3 else 200
D = int(sys.argv[4]) if len(sys.argv) > 4 else 20
draws = int(sys.argv[5]) if len(sys.argv) > 5 else 1024

rs = np.random.RandomState(4)
A = rs.standard_normal((N, D)) / np.sqrt(D)
theta = np.where(np.arange(D) < 4, 3.0, 0.0) * rs.standard_normal(D)     # four covariates matter, the rest is noise
y1 = (rs.random_sample(N) < 1.0 / (1.0 + np.exp(-A @ theta))).astype(np.float64)
lams = 10.0 ** np.linspace(-3, 3, L)
fold = rs.permutation(N) % F

# problem f L + l: fold f held out, prior precision lams[l]
K = F * L
mask = np.repeat((fold[None, :] == np.arange(F)[:, None]).astype(np.float64), L, axis=0)
y = np.ascontiguousarray(np.broadcast_to(y1, (K, N)))
cv = gsmvi_amd.SharedDesignGLMTarget(A, y, "logistic", prior_precision=np.tile(lams, F), weights=1.0 - mask)
mean, cov, res = gsmvi_amd.laplace_init_shared_batched(cv)
held = gsmvi_amd.predict_shared_batched(cv, mean, cov, cv.A, y=y, weights=mask)
elpd_kfold = held.elpd.reshape(F, L).sum(0)
lpd = np.where(mask > 0, held.lpd, 0.0).reshape(F, L, N).sum(0)          # every row is held out in exactly one fold
se_kfold = np.sqrt(N * lpd.var(axis=1, ddof=1))
print(f"{F} folds x {L} values of lambda = {K} problems on one design (N, D) = ({N}, {D}), held once: {A.nbytes / 1e3:.1f} kB against "
      f"{K * A.nbytes / 1e3:.1f} kB replicated; Laplace converged in {int(res.success.sum())} of {K} ({res.nlaunch} launches), then one "
      f"launch for the {N * L} held-out densities")

# the L fits on all the data and their PSIS leave-one-out
full = gsmvi_amd.SharedDesignGLMTarget(A, y[:L], "logistic", prior_precision=lams)
fmean, fcov, fres = gsmvi_amd.laplace_init_shared_batched(full)
loo = gsmvi_amd.psis_loo_shared_batched(full, fmean, fcov, np.arange(L) + 11, num_draws=draws)

print("     lambda  elpd K-fold  +- se   elpd_loo  +- se   max khat   difference")
for l in range(L):
    print(f"{lams[l]:11.4g}  {elpd_kfold[l]:11.2f}  {se_kfold[l]:5.2f}  {loo.elpd_loo[l]:9.2f}  {loo.se[l]:5.2f}  {np.max(loo.khat[l]):9.2f}  "
          f"{elpd_kfold[l] - loo.elpd_loo[l]:10.2f}")
bk, bl = int(np.argmax(elpd_kfold)), int(np.argmax(loo.elpd_loo))
print(f"best lambda by {F}-fold cross-validation: {lams[bk]:.3g}; by PSIS leave-one-out: {lams[bl]:.3g} (a fold's fit sees "
      f"{N - N // F} of the {N} rows, so its density is a little lower than the leave-one-out's)")
