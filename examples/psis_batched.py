#!/usr/bin/env python3
"""The step between "fitted" and "used": can each of K fitted Gaussians be trusted?  K logistic posteriors are fitted by
``laplace_init_batched`` -> ``GSMBatch.fit``; ``psis_batched`` then draws S points of every q_k, asks the target for its values at
them and, in one launch, fits a generalised Pareto tail to the importance ratios of every problem.  Printed: the share of problems
whose khat is below the threshold (``ok``), the quartiles of khat and of the effective sample size, the estimate of the log
evidence log Z_k, and how far the importance-corrected mean moves from the fitted one, for the GSM fit, for its Laplace start and for
a deliberately poor q (the fit with a quarter of its covariance).

    python examples/psis_batched.py [K] [D] [N] [batch] [niter] [draws]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
D = int(sys.argv[2]) if len(sys.argv) > 2 else 5
N = int(sys.argv[3]) if len(sys.argv) > 3 else 100
batch = int(sys.argv[4]) if len(sys.argv) > 4 else 8
niter = int(sys.argv[5]) if len(sys.argv) > 5 else 500
draws = int(sys.argv[6]) if len(sys.argv) > 6 else 1024

rs = np.random.RandomState(1)
A = 2.0 * rs.standard_normal((K, N, D)) / np.sqrt(D)
theta = rs.standard_normal((K, D))
y = (rs.random_sample((K, N)) < 1.0 / (1.0 + np.exp(-np.einsum("knd,kd->kn", A, theta)))).astype(np.float64)

tgt = gsmvi_amd.BatchedLogisticTarget(A, y, prior_precision=1.0)
m_la, c_la, res = gsmvi_amd.laplace_init_batched(tgt)
print(f"Laplace: {int(res.success.sum())} of {K} converged in {res.nlaunch} rounds")
keys = np.arange(K) + 7
m_gsm, c_gsm = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, mean=m_la, cov=c_la, batch_size=batch, niter=niter, verbose=False)

fits = {"GSM fit": (m_gsm, c_gsm), "Laplace start": (m_la, c_la), "GSM fit, cov / 4": (m_gsm, 0.25 * np.asarray(c_gsm))}
print(f"PSIS of {K} logistic posteriors, D = {D}, {draws} draws each (sample block {K * draws * D * 8 / 2**20:.1f} MiB):")
for name, (m, c) in fits.items():
    r = gsmvi_amd.psis_batched(tgt.lp, m, c, keys, num_draws=draws)
    if name == "GSM fit":
        print(f"  threshold for khat: {r.threshold:.3f}")
    fin = r.info == 0
    q = lambda v: np.array2string(np.percentile(v[fin], [25, 50, 75]), precision=2) if fin.any() else "-"     # noqa: E731
    move = np.abs(r.mean - np.asarray(m)).max(1) / np.sqrt(np.einsum("kii->ki", np.asarray(c))).max(1)
    print(f"  {name:18s} ok {r.ok.mean():6.1%}   khat quartiles {q(r.khat)}   ess quartiles {q(r.ess)}   median log Z "
          f"{np.median(r.log_z[fin]) if fin.any() else float('nan'):8.3f}   corrected mean moves {np.median(move[fin]) if fin.any() else float('nan'):.3f} sd")
