#!/usr/bin/env python3
"""K three-class multinomial logit regressions fitted at once: what examples/example_gsm.py does for one model (its log_prob and
jit(grad(.)) handed to the fit) with BatchedSoftmaxTarget scoring all K posteriors in one HIP launch per call.  Problem k has
labels y_kn ~ Categorical(softmax(a_kn . W_k)) with class C - 1 the reference class (zero coefficients), so the parameter is
x[c P + j] = W_cj, D = (C - 1) P.  The family is initialised with ``lbfgs_init_batched``, fitted with ``GSMBatch`` under a
``BatchedKLMonitor``, and every fitted Gaussian is checked with ``psis_batched``: the median khat and the share of problems whose
khat is ``ok`` (below the result's threshold) are printed.

    python examples/softmax_batched.py [K] [C] [P] [N] [batch] [niter]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
C = int(sys.argv[2]) if len(sys.argv) > 2 else 3
P = int(sys.argv[3]) if len(sys.argv) > 3 else 4
N = int(sys.argv[4]) if len(sys.argv) > 4 else 200
batch = int(sys.argv[5]) if len(sys.argv) > 5 else 8
niter = int(sys.argv[6]) if len(sys.argv) > 6 else 500
LAM = 1.0
D = (C - 1) * P

rs = np.random.RandomState(2)
A = rs.standard_normal((K, N, P)) / np.sqrt(P)
W = rs.standard_normal((K, C - 1, P))
eta = np.concatenate([np.einsum("knp,kcp->knc", A, W), np.zeros((K, N, 1))], axis=2)
p = np.exp(eta - eta.max(axis=2, keepdims=True))
cdf = np.cumsum(p / p.sum(axis=2, keepdims=True), axis=2)
y = np.minimum((rs.random_sample((K, N, 1)) > cdf).sum(axis=2), C - 1)
counts = rs.randint(N // 2, N + 1, size=K)                # every problem has its own number of observations

tgt = gsmvi_amd.BatchedSoftmaxTarget(A, y, C, prior_precision=LAM, counts=counts)
keys = np.arange(K) + 7

mean0, cov0, res = gsmvi_amd.lbfgs_init_batched(np.zeros((K, D)), tgt.lp, tgt.lp_g)
print(f"lbfgs_init_batched: {int(res.success.sum())} of {K} converged in {res.nlaunch} evaluation rounds; max |grad| "
      f"{np.abs(res.jac).max():.2e}")
mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=256, checkpoint=100)
fit = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g)
mean, cov = fit.fit(keys, mean=mean0, cov=cov0, batch_size=batch, niter=niter, verbose=False, monitor=mon)
print(f"GSMBatch: {niter} iterations, reverts {int(fit.n_reverts.sum())}; reverse KL estimate, median over the problems: first "
      f"{np.median(mon.rkl[0]):.3f}, last {np.median(mon.rkl[-1]):.3f}")

ps = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=1024)
khat = np.asarray(ps.khat)
print(f"psis_batched: median khat {np.median(khat):.3f}, ok (khat < {ps.threshold:.2f}) for {100.0 * np.mean(np.asarray(ps.ok)):.0f}% of "
      f"{K} problems")
print("problem   fitted mean (first 3 coordinates)        true W (first 3)                         khat")
for k in range(min(K, 5)):
    f3 = lambda v: " ".join(f"{t:+.4f}" for t in v[:3])                                            # noqa: E731
    print(f"{k:7d}   {f3(mean[k]):40s} {f3(W[k].reshape(-1)):40s} {khat[k]:.3f}")
