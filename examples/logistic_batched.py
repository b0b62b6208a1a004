#!/usr/bin/env python3
"""K Bayesian logistic regressions at once: GSM, BaM and the ADVI baseline on the same K synthetic data sets, the same keys and
one BatchedKLMonitor each.  The target is BatchedLogisticTarget: log-density and score of all K posteriors from one HIP launch.
There is no exact sampler, so the monitors get no ``ref_samples`` and the reverse KL is known up to each posterior's
normaliser: its fall from the first to the last checkpoint is what counts, and differences between methods.  The fitted means
are compared with each problem's MAP from a Newton iteration in numpy.

    python examples/logistic_batched.py [K] [D] [N] [batch] [niter]
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
lam = 1.0
tgt = gsmvi_amd.BatchedLogisticTarget(A, y, prior_precision=lam, counts=counts)


def newton_map(Ak, yk):
    x = np.zeros(D)
    for _ in range(50):
        s = 1.0 / (1.0 + np.exp(-(Ak @ x)))
        step = np.linalg.solve((Ak * (s * (1.0 - s))[:, None]).T @ Ak + lam * np.eye(D), Ak.T @ (yk - s) - lam * x)
        x = x + step
        if np.abs(step).max() < 1e-13:
            break
    return x


x_map = np.stack([newton_map(A[k, :counts[k]], y[k, :counts[k]]) for k in range(K)])
keys = np.arange(K) + 99


def monitor():
    return gsmvi_amd.BatchedKLMonitor(batch_size_kl=256, checkpoint=max(niter // 10, 1))


mons = {"GSM": monitor(), "BaM": monitor(), "ADVI": monitor()}
means = {}
means["GSM"], _ = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, batch_size=batch, niter=niter, verbose=False,
                                                               monitor=mons["GSM"])
means["BaM"], _ = gsmvi_amd.BaMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, lambda i: 100.0 / (1 + i), batch_size=batch, niter=niter,
                                                               verbose=False, monitor=mons["BaM"])
means["ADVI"], _, losses = gsmvi_amd.ADVIBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, gsmvi_amd.Adam(1e-2), batch_size=batch,
                                                                         niter=niter, monitor=mons["ADVI"], verbose=False)
for name, mon in mons.items():
    first, last = mon.rkl[0], mon.rkl[-1]
    dist = np.linalg.norm(means[name] - x_map, axis=1)
    print(f"{name:5s} reverse KL + log Z over {K} posteriors, first -> last: median {np.median(first):.3f} -> {np.median(last):.3f} "
          f"(fell for {int((last < first).sum())} of {K}); |mean - MAP| median {np.median(dist):.3f}, worst {dist.max():.3f} "
          f"({mon.nevals[-1]} score evaluations per posterior)")
print(f"ADVI  loss per posterior, first -> last: median {np.median(losses[0]):.2f} -> {np.median(losses[-1]):.2f}")
