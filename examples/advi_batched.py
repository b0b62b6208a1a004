#!/usr/bin/env python3
"""GSM, BaM and the ADVI baseline on the same K Gaussian targets, the same keys and one BatchedKLMonitor each (the comparison
of the reference's examples/example_initializers.py and example_advi.py, for K problems at once): prints the final reverse KL
per method.  With the same keys GSMBatch and ADVIBatch consume the same normals at every iteration.

    python examples/advi_batched.py [K] [D] [batch] [niter]
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
D = int(sys.argv[2]) if len(sys.argv) > 2 else 5
batch = int(sys.argv[3]) if len(sys.argv) > 3 else 8
niter = int(sys.argv[4]) if len(sys.argv) > 4 else 1000

rs = np.random.RandomState(1)
means = rs.random_sample((K, D))
A = rs.normal(size=(K, D, D))
covs = A @ np.swapaxes(A, 1, 2) / D + 0.1 * np.eye(D)
tgt = gsmvi_amd.BatchedGaussianTarget(means, cov=covs)
norms = tgt.mean.new_tensor(-0.5 * D * math.log(2.0 * math.pi) - 0.5 * np.linalg.slogdet(covs)[1])


def lp(x):                                  # the normalised log-density, so that the monitor's KL goes to zero
    return tgt.lp(x) + norms * x.shape[1]


keys = np.arange(K) + 99


def monitor():
    return gsmvi_amd.BatchedKLMonitor(batch_size_kl=256, checkpoint=max(niter // 10, 1))


mons = {"GSM": monitor(), "BaM": monitor(), "ADVI": monitor()}
gsmvi_amd.GSMBatch(K, D, lp, tgt.lp_g).fit(keys, batch_size=batch, niter=niter, verbose=False, monitor=mons["GSM"])
gsmvi_amd.BaMBatch(K, D, lp, tgt.lp_g).fit(keys, lambda i: 100.0 / (1 + i), batch_size=batch, niter=niter, verbose=False,
                                          monitor=mons["BaM"])
_, _, losses = gsmvi_amd.ADVIBatch(K, D, lp, tgt.lp_g).fit(keys, gsmvi_amd.Adam(1e-2), batch_size=batch, niter=niter,
                                                          monitor=mons["ADVI"], verbose=False)
for name, mon in mons.items():
    rkl = mon.rkl[-1]
    print(f"{name:5s} final reverse KL over {K} targets: median {np.median(rkl):.3e}, worst {np.max(rkl):.3e} "
          f"({mon.nevals[-1]} score evaluations per target)")
print(f"ADVI  loss per target, first -> last: median {np.median(losses[0]):.2f} -> {np.median(losses[-1]):.2f}")
