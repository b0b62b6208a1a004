#!/usr/bin/env python3
"""Two starts for the batched GSM fit of K three-class multinomial logit posteriors (the set-up of examples/softmax_batched.py):
the L-BFGS start (``lbfgs_init_batched``: the maximiser of lp and the BFGS inverse-Hessian estimate) and the Laplace start
(``laplace_init_softmax_batched``: the Newton mode and the inverse of the class-coupled negative Hessian there, one launch per
round).  Each start and each fit that follows it is judged by ``psis_batched``: the Pareto khat of the importance ratios
p / q from fresh draws, per problem; below the threshold the Gaussian is a usable proposal for its posterior.

    python examples/softmax_laplace_batched.py [K] [P] [N] [batch] [niter]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
N = int(sys.argv[3]) if len(sys.argv) > 3 else 200
batch = int(sys.argv[4]) if len(sys.argv) > 4 else 8
niter = int(sys.argv[5]) if len(sys.argv) > 5 else 500
C = 3
D = (C - 1) * P

rs = np.random.RandomState(1)
A = rs.standard_normal((K, N, P)) / np.sqrt(P)
W = rs.standard_normal((K, C - 1, P))
eta = np.concatenate([np.einsum("knp,kcp->knc", A, W), np.zeros((K, N, 1))], axis=2)
prob = np.exp(eta - eta.max(axis=2, keepdims=True))
cdf = np.cumsum(prob / prob.sum(axis=2, keepdims=True), axis=2)
y = np.minimum((rs.random_sample((K, N, 1)) > cdf).sum(axis=2), C - 1)
counts = rs.randint(N // 2, N + 1, size=K)                # every problem has its own number of observations
tgt = gsmvi_amd.BatchedSoftmaxTarget(A, y, C, prior_precision=1.0, counts=counts)
keys = np.arange(K) + 99

m_lb, c_lb, r_lb = gsmvi_amd.lbfgs_init_batched(np.zeros((K, D)), tgt.lp, tgt.lp_g)
print(f"L-BFGS : {int(r_lb.success.sum())} of {K} converged, {r_lb.nlaunch} rounds of three launches, max |grad| "
      f"{np.abs(r_lb.jac).max():.2e}")
m_la, c_la, r_la = gsmvi_amd.laplace_init_softmax_batched(tgt)
print(f"Laplace: {int(r_la.success.sum())} of {K} converged, {r_la.nlaunch} rounds of one launch (Newton iterations: most "
      f"{int(r_la.nit.max())}), max |grad| {np.abs(r_la.jac).max():.2e}")


def khat(mean, cov):
    r = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys + 1000, num_draws=256, moments=False)
    return float(np.median(r.khat[r.info == 0])), float(r.ok.mean())


for name, (mean, cov) in {"L-BFGS": (m_lb, c_lb), "Laplace": (m_la, c_la)}.items():
    k0, ok0 = khat(mean, cov)
    m1, c1 = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, mean=mean, cov=cov, batch_size=batch, niter=niter, verbose=False)
    k1, ok1 = khat(m1, c1)
    print(f"{name:8s} start: median khat {k0:.2f}, usable for {100 * ok0:.0f} % of the posteriors; after {niter} GSM iterations "
          f"{k1:.2f}, {100 * ok1:.0f} %")
