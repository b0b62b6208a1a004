#!/usr/bin/env python3
"""The use of a batched fit: held-out predictions of K logistic regressions.  A third of every problem's rows is held out; the rest
is fitted by ``laplace_init_batched`` -> ``GSMBatch.fit``; ``predict`` then scores the held-out rows under each fitted Gaussian,
one launch per call (the posterior predictive needs no sampling: the linear predictor of a new row is one-dimensional Gaussian).
Printed: the median held-out elpd (expected log predictive density, summed over the held-out rows) of the GSM fit, of the
Laplace start and of the plug-in prediction (the fitted mean with ``cov`` = 0), and the median predictive probability of the
fit against the plug-in's on the rows where they differ most.

    python examples/predict_batched.py [K] [D] [N] [batch] [niter]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
D = int(sys.argv[2]) if len(sys.argv) > 2 else 5
N = int(sys.argv[3]) if len(sys.argv) > 3 else 150
batch = int(sys.argv[4]) if len(sys.argv) > 4 else 8
niter = int(sys.argv[5]) if len(sys.argv) > 5 else 500

rs = np.random.RandomState(1)
A = 2.0 * rs.standard_normal((K, N, D)) / np.sqrt(D)
theta = rs.standard_normal((K, D))
y = (rs.random_sample((K, N)) < 1.0 / (1.0 + np.exp(-np.einsum("knd,kd->kn", A, theta)))).astype(np.float64)
held = N // 3
A_fit, y_fit, A_new, y_new = A[:, held:], y[:, held:], A[:, :held], y[:, :held]

tgt = gsmvi_amd.BatchedLogisticTarget(A_fit, y_fit, prior_precision=1.0)
m_la, c_la, res = gsmvi_amd.laplace_init_batched(tgt)
print(f"Laplace: {int(res.success.sum())} of {K} converged in {res.nlaunch} rounds")
m_gsm, c_gsm = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(np.arange(K) + 7, mean=m_la, cov=c_la, batch_size=batch, niter=niter,
                                                               verbose=False)

fits = {"GSM fit": (m_gsm, c_gsm), "Laplace start": (m_la, c_la), "plug-in (cov = 0)": (m_gsm, np.zeros_like(c_gsm))}
pred = {name: tgt.predict(m, c, A_new, y=y_new) for name, (m, c) in fits.items()}
print(f"held-out elpd over {held} rows, median of {K} problems (eta_var of the GSM fit: median "
      f"{np.median(pred['GSM fit'].eta_var):.3f}, largest {pred['GSM fit'].eta_var.max():.3f})")
for name, p in pred.items():
    print(f"  {name:18s} {np.median(p.elpd):9.3f}   (mean over problems {p.elpd.mean():9.3f})")
gap = np.abs(pred["GSM fit"].mean - pred["plug-in (cov = 0)"].mean)
k, n = np.unravel_index(gap.argmax(), gap.shape)
print(f"largest change of a predictive probability by the variance: problem {k}, row {n}: plug-in "
      f"{pred['plug-in (cov = 0)'].mean[k, n]:.3f} -> {pred['GSM fit'].mean[k, n]:.3f} (eta ~ N({pred['GSM fit'].eta_mean[k, n]:.2f}, "
      f"{pred['GSM fit'].eta_var[k, n]:.2f}), y = {y_new[k, n]:.0f})")
