#!/usr/bin/env python3
"""Three starts for the batched GSM fit of K logistic posteriors (the set-up of examples/initializers_batched.py): (0, I), the
L-BFGS start (``lbfgs_init_batched``: the maximiser of lp and the BFGS inverse-Hessian estimate) and the Laplace start
(``laplace_init_batched``: the Newton mode and the inverse of the negative Hessian A^T W A + lam I there).  Each fit is followed
by a BatchedKLMonitor whose evaluation count starts at the initialiser's (``offset_evals=res.nlaunch``).  The posteriors have no
exact sampler, so the reverse KL is known up to each posterior's log normaliser: falls and differences are what count.  Printed:
the median reverse KL of the raw Laplace Gaussian (the first checkpoint of its fit, before any GSM step has moved it far), and
the GSM iterations each start needs to reach the final median reverse KL of the (0, I) start.

    python examples/laplace_batched.py [K] [D] [N] [batch] [niter]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
D = int(sys.argv[2]) if len(sys.argv) > 2 else 5
N = int(sys.argv[3]) if len(sys.argv) > 3 else 200
batch = int(sys.argv[4]) if len(sys.argv) > 4 else 8
niter = int(sys.argv[5]) if len(sys.argv) > 5 else 1000

rs = np.random.RandomState(1)
A = rs.standard_normal((K, N, D)) / np.sqrt(D)
theta = rs.standard_normal((K, D))
y = (rs.random_sample((K, N)) < 1.0 / (1.0 + np.exp(-np.einsum("knd,kd->kn", A, theta)))).astype(np.float64)
counts = rs.randint(N // 2, N + 1, size=K)                # every problem has its own number of observations
tgt = gsmvi_amd.BatchedLogisticTarget(A, y, prior_precision=1.0, counts=counts)
keys = np.arange(K) + 99

m_lb, c_lb, r_lb = gsmvi_amd.lbfgs_init_batched(np.zeros((K, D)), tgt.lp, tgt.lp_g)
print(f"L-BFGS : {int(r_lb.success.sum())} of {K} converged, {r_lb.nlaunch} rounds of three launches, max |grad| "
      f"{np.abs(r_lb.jac).max():.2e}")
m_la, c_la, r_la = gsmvi_amd.laplace_init_batched(tgt)
print(f"Laplace: {int(r_la.success.sum())} of {K} converged, {r_la.nlaunch} rounds of one launch (Newton iterations: most "
      f"{int(r_la.nit.max())}), max |grad| {np.abs(r_la.jac).max():.2e}")


def fit(mean, cov, offset):
    mon = gsmvi_amd.BatchedKLMonitor(batch_size_kl=256, checkpoint=max(niter // 50, 1), offset_evals=offset)
    gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, mean=mean, cov=cov, batch_size=batch, niter=niter, verbose=False, monitor=mon)
    return mon


mons = {"(0, I)": fit(None, None, 0), "L-BFGS": fit(m_lb, c_lb, r_lb.nlaunch), "Laplace": fit(m_la, c_la, r_la.nlaunch)}
goal = float(np.median(mons["(0, I)"].rkl[-1]))
print(f"raw Laplace Gaussian: reverse KL + log Z, median over {K} posteriors, {np.median(mons['Laplace'].rkl[0]):.3f} "
      f"(the (0, I) fit ends at {goal:.3f} after {niter} iterations)")
for name, mon in mons.items():
    med = [float(np.median(r)) for r in mon.rkl]
    hit = next((i for i, m in enumerate(med) if m <= goal), None)
    if hit is None:
        print(f"{name:8s} start: {med[0]:.3f} -> {med[-1]:.3f}; did not reach {goal:.3f} in {niter} iterations")
    else:
        print(f"{name:8s} start: {med[0]:.3f} -> {med[-1]:.3f}; reaches {goal:.3f} at iteration {min(hit * mon.checkpoint, niter)} "
              f"({mon.nevals[hit]} evaluations per posterior, the initialiser's included)")
