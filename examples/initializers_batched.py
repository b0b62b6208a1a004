#!/usr/bin/env python3
"""The reference's examples/example_initializers.py for K problems at once: the variational family is initialised with
``lbfgs_init_batched`` (the L-BFGS maximiser of lp as the mean, the dense BFGS inverse-Hessian estimate as the covariance) and
then fitted with GSM and ADVI, each followed by a BatchedKLMonitor whose evaluation count starts at the initialiser's
(``offset_evals=res.nlaunch``).  The target is BatchedLogisticTarget (K posteriors, no exact sampler: the reverse KL is known up
to each posterior's log normaliser, so falls and differences are what count).  The same fits started from (0, I) are printed
beside them, and the number of GSM iterations the initialised fit needs to reach the cold start's final median reverse KL.

    python examples/initializers_batched.py [K] [D] [N] [batch] [niter]
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

print("Initialize with LBFGS")
mean_init, cov_init, res = gsmvi_amd.lbfgs_init_batched(np.ones((K, D)), tgt.lp, tgt.lp_g)
print(f"LBFGS fit: {int(res.success.sum())} of {K} converged; evaluations per problem median {int(np.median(res.nfev))}, most "
      f"{int(res.nfev.max())}; {res.nlaunch} evaluation rounds ran; max |grad| {np.abs(res.jac).max():.2e}")


def monitor(offset):
    return gsmvi_amd.BatchedKLMonitor(batch_size_kl=256, checkpoint=max(niter // 50, 1), offset_evals=offset)


def fits(mean, cov, offset):
    mons = {"GSM": monitor(offset), "ADVI": monitor(offset)}
    gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, mean=mean, cov=cov, batch_size=batch, niter=niter, verbose=False,
                                                    monitor=mons["GSM"])
    gsmvi_amd.ADVIBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, gsmvi_amd.Adam(1e-2), mean=mean, cov=cov, batch_size=batch, niter=niter,
                                                     monitor=mons["ADVI"], verbose=False)
    return mons


warm, cold = fits(mean_init, cov_init, res.nlaunch), fits(None, None, 0)
for name in ("GSM", "ADVI"):
    for label, mon in (("from lbfgs_init_batched", warm[name]), ("from (0, I)", cold[name])):
        print(f"{name:5s} {label:24s} reverse KL + log Z, median over {K} posteriors, first -> last checkpoint: "
              f"{np.median(mon.rkl[0]):.3f} -> {np.median(mon.rkl[-1]):.3f}  (evaluations per posterior {mon.nevals[0]} -> "
              f"{mon.nevals[-1]})")
    goal = np.median(cold[name].rkl[-1])
    med = [float(np.median(r)) for r in warm[name].rkl]
    hit = next((i for i, m in enumerate(med) if m <= goal), None)
    if hit is None:
        print(f"{name:5s} the initialised fit did not reach the cold start's final median {goal:.3f} in {niter} iterations")
    else:
        it = min(hit * warm[name].checkpoint, niter)
        print(f"{name:5s} reaches the cold start's final median {goal:.3f} at its checkpoint {hit} (iteration {it}): "
              f"{warm[name].nevals[hit]} evaluations per posterior, the initialiser's {res.nlaunch} included, against "
              f"{cold[name].nevals[-1]}")
