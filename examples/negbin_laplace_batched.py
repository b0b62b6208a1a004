#!/usr/bin/env python3
"""K overdispersed count data sets (the model of examples/negbin_batched.py) started three ways: ``laplace_init_negbin_batched``
(Newton rounds on the closed-form bordered Hessian, one HIP launch per round, with the last-pivot rule where theta = log r has no
positive curvature), ``lbfgs_init_batched`` and ``pathfinder_init_batched`` -- the role of the reference's lbfgs_init
(gsmvi/initializers.py:5-17).  ``psis_batched`` then says of each start, before any fit, how far its Gaussian is from the
posterior, and a short ``GSMBatch`` fit from the Laplace start shows that it is a start the fit accepts.

    python examples/negbin_laplace_batched.py [K] [P] [N]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 32
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
N = int(sys.argv[3]) if len(sys.argv) > 3 else 300
D = P + 1

rs = np.random.RandomState(4)
A = np.concatenate([np.ones((K, N, 1)), rs.standard_normal((K, N, P - 1))], axis=2)
beta = np.concatenate([1.5 + 0.5 * rs.standard_normal((K, 1)), 0.4 * rs.standard_normal((K, P - 1))], axis=1)
log_r = rs.uniform(0.0, 2.5, K)
offset = np.log(rs.uniform(0.5, 4.0, size=(K, N)))
mu = np.exp(np.einsum("knp,kp->kn", A, beta) + offset)
r = np.exp(log_r)[:, None]
y = rs.poisson(rs.gamma(r, mu / r)).astype(np.float64)
keys = np.arange(K) + 7

target = gsmvi_amd.BatchedNegBinomialTarget(A, y, prior_precision=0.1, offset=offset, log_size_mean=0.0, log_size_precision=1.0)
starts = {
    "laplace": gsmvi_amd.laplace_init_negbin_batched(target),
    "lbfgs": gsmvi_amd.lbfgs_init_batched(np.zeros((K, D)), target.lp, target.lp_g),
    "pathfinder": gsmvi_amd.pathfinder_init_batched(np.zeros((K, D)), target.lp, target.lp_g),
}
mean, cov, res = starts["laplace"]
print(f"laplace_init_negbin_batched: {int(res.success.sum())} of {K} converged in {res.nlaunch} launches; Newton iterations "
      f"{int(res.nit.min())} - {int(res.nit.max())}; problems with a modified last pivot: {int((res.nmod > 0).sum())} "
      f"(at x0 = 0 their Hessian is indefinite in theta: plain Newton would have stopped there)")
H = gsmvi_amd.neg_hessian_negbin_batched(target, mean).cpu().numpy()
print(f"smallest eigenvalue of the negative Hessian at the modes: {min(np.linalg.eigvalsh(h).min() for h in H):.3g} (positive: modes)")
sd = np.sqrt(np.einsum("kii->ki", cov))
z = (mean[:, P] - log_r) / sd[:, P]
print(f"log r against the truth, in Laplace standard deviations: median |z| {np.median(np.abs(z)):.2f}, max {np.abs(z).max():.2f}")
for name, (m, c, _) in starts.items():
    ps = gsmvi_amd.psis_batched(target.lp, m, c, keys, num_draws=1024, moments=False)
    print(f"{name:10s} start: khat median {np.median(ps.khat):6.2f}, max {ps.khat.max():6.2f}, usable (below {ps.threshold:.2f}): "
          f"{int((ps.khat < ps.threshold).sum())} of {K}")
fit = gsmvi_amd.GSMBatch(K, D, target.lp, target.lp_g)
m1, c1 = fit.fit(keys, mean=mean, cov=cov, batch_size=8, niter=200, verbose=False)
ps = gsmvi_amd.psis_batched(target.lp, m1, c1, keys, num_draws=1024, moments=False)
print(f"after 200 GSM iterations from the Laplace start: khat median {np.median(ps.khat):.2f}, max {ps.khat.max():.2f}, reverts "
      f"{int(fit.n_reverts.sum())}")
