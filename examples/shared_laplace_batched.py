#!/usr/bin/env python3
"""A sweep over the prior precision of one logistic regression, K values of lambda fitted at once: one data set (A, y), K priors
N(0, I / lam_k), each posterior started at its Laplace approximation -- ``laplace_init_shared_batched``: the Newton mode and
(A^T W A + lam_k I)^-1 from one HIP launch per round, with the design matrix held once on the device --, refined by
``GSMBatch.fit`` from that start, and checked by ``psis_batched`` before and after the fit.  It fills the role of
examples/example_initializers.py (lbfgs_init, then the fit) for K posteriors that share their covariates.

    python examples/shared_laplace_batched.py [K] [D] [N] [batch] [niter]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 32
D = int(sys.argv[2]) if len(sys.argv) > 2 else 5
N = int(sys.argv[3]) if len(sys.argv) > 3 else 200
batch = int(sys.argv[4]) if len(sys.argv) > 4 else 8
niter = int(sys.argv[5]) if len(sys.argv) > 5 else 200

rs = np.random.RandomState(4)
A = rs.standard_normal((N, D)) / np.sqrt(D)
theta = rs.standard_normal(D)
y1 = (rs.random_sample(N) < 1.0 / (1.0 + np.exp(-A @ theta))).astype(np.float64)
y = np.broadcast_to(y1, (K, N)).copy()                     # the same responses under every prior
lam = np.logspace(-2, 2, K)                                # the sweep: lam_k from 0.01 to 100

tgt = gsmvi_amd.SharedDesignGLMTarget(A, y, "logistic", prior_precision=lam)
keys = np.arange(K) + 7
mean0, cov0, res = gsmvi_amd.laplace_init_shared_batched(tgt)
print(f"laplace_init_shared_batched: {int(res.success.sum())} of {K} converged, at most {int(res.nit.max())} Newton iterations, "
      f"{res.nlaunch} launches")
H = gsmvi_amd.neg_hessian_shared_batched(tgt, mean0).cpu().numpy()
print(f"max |cov H - I| at the modes: {np.abs(cov0 @ H - np.eye(D)).max():.1e}")
before = gsmvi_amd.psis_batched(tgt.lp, mean0, cov0, keys)
fit = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g)
mean, cov = fit.fit(keys, mean=mean0, cov=cov0, batch_size=batch, niter=niter, verbose=False)
after = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, call=1)
print(f"GSMBatch.fit from the Laplace start: {niter} iterations, reverts {int(fit.n_reverts.sum())}")
print(f"PSIS khat, median over the sweep: {np.median(before.khat):.2f} at the Laplace start ({int(before.ok.sum())} of {K} ok), "
      f"{np.median(after.khat):.2f} after the fit ({int(after.ok.sum())} of {K} ok)")
print("      lam   |mode|   |fitted mean|   trace cov (Laplace)   trace cov (fit)   khat (fit)")
for k in range(0, K, max(1, K // 8)):
    print(f"{lam[k]:9.3g}   {np.linalg.norm(mean0[k]):6.3f}   {np.linalg.norm(mean[k]):13.3f}   {np.trace(cov0[k]):19.4f}   "
          f"{np.trace(cov[k]):15.4f}   {after.khat[k]:10.2f}")
