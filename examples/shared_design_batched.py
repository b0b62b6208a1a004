#!/usr/bin/env python3
"""The Bayesian bootstrap of one logistic regression, K replicates fitted at once: one data set (A, y) under K vectors of
observation weights w_k ~ Dirichlet(1, ..., 1) N (Rubin's bootstrap), each replicate's weighted posterior fitted by ``GSMBatch``
with ``SharedDesignGLMTarget`` scoring all K of them in one HIP launch per call -- examples/example_gsm.py's log_prob and
jit(grad(.)) for K posteriors that share their design matrix, which is held once on the device.  The spread of the K fitted means
is the bootstrap's estimate of the sampling variability of the posterior mean; it is printed beside the posterior standard
deviation of the unweighted fit (replicate 0 has w = 1), which for a well-specified model is of the same size.

    python examples/shared_design_batched.py [K] [D] [N] [batch] [niter]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
D = int(sys.argv[2]) if len(sys.argv) > 2 else 5
N = int(sys.argv[3]) if len(sys.argv) > 3 else 400
batch = int(sys.argv[4]) if len(sys.argv) > 4 else 8
niter = int(sys.argv[5]) if len(sys.argv) > 5 else 500
LAM = 1.0

rs = np.random.RandomState(4)
A = rs.standard_normal((N, D)) / np.sqrt(D)
theta = rs.standard_normal(D)
y1 = (rs.random_sample(N) < 1.0 / (1.0 + np.exp(-A @ theta))).astype(np.float64)
y = np.broadcast_to(y1, (K, N)).copy()                     # the same responses for every replicate
w = N * rs.dirichlet(np.ones(N), size=K)                   # the replicates differ in their weights alone
w[0] = 1.0                                                 # replicate 0: the data set as it is

tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, "logistic", prior_precision=LAM, weights=w)
keys = np.arange(K) + 7
mean0, cov0, res = gsmvi_amd.lbfgs_init_batched(np.zeros((K, D)), tgt.lp, tgt.lp_g)
print(f"lbfgs_init_batched: {int(res.success.sum())} of {K} converged in {res.nlaunch} evaluation rounds")
fit = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g)
mean, cov = fit.fit(keys, mean=mean0, cov=cov0, batch_size=batch, niter=niter, verbose=False)

spread = mean[1:].std(0, ddof=1)
sd0 = np.sqrt(np.diag(cov[0]))
print(f"{K - 1} bootstrap replicates of N = {N}, D = {D}; reverts {int(fit.n_reverts.sum())}")
print("coordinate   true theta   fitted mean (w = 1)   posterior sd (w = 1)   spread of the replicates' means")
for j in range(D):
    print(f"{j:10d}   {theta[j]:+10.4f}   {mean[0, j]:+19.4f}   {sd0[j]:20.4f}   {spread[j]:31.4f}")
print(f"median ratio spread / posterior sd: {np.median(spread / sd0):.2f}")
