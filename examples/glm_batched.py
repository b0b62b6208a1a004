#!/usr/bin/env python3
"""K Poisson regressions with exposure offsets, fitted at once: what examples/example_gsm.py does for one model (its log_prob
and jit(grad(.)) handed to the fit) with BatchedGLMTarget scoring all K posteriors in one HIP launch per call.  Problem k has
counts y_kn ~ Poisson(exposure_kn exp(a_kn . theta_k)); the log exposure is the offset.  The family is initialised with
``lbfgs_init_batched`` and fitted with ``GSMBatch``; the fitted means are printed beside each posterior's MAP from a numpy
Newton iteration (a Gaussian fit to a log-concave posterior has its mean near the mode; the distance is in units of the
fitted standard deviation).

    python examples/glm_batched.py [K] [D] [N] [batch] [niter]
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
niter = int(sys.argv[5]) if len(sys.argv) > 5 else 500
LAM = 1.0

rs = np.random.RandomState(2)
A = rs.standard_normal((K, N, D)) / np.sqrt(D)
theta = 0.7 * rs.standard_normal((K, D))
exposure = rs.uniform(0.5, 4.0, size=(K, N))
offset = np.log(exposure)
y = rs.poisson(exposure * np.exp(np.einsum("knd,kd->kn", A, theta))).astype(np.float64)
counts = rs.randint(N // 2, N + 1, size=K)                # every problem has its own number of observations


def newton_map(Ak, yk, ok, lam, iters=100):
    """the mode of one posterior: Newton's method on the concave lp, halving a step that does not increase it"""
    lp = lambda x: float(yk @ (Ak @ x + ok) - np.exp(Ak @ x + ok).sum() - 0.5 * lam * x @ x)       # noqa: E731
    x = np.zeros(Ak.shape[1])
    for _ in range(iters):
        m = np.exp(Ak @ x + ok)
        g = Ak.T @ (yk - m) - lam * x
        step = np.linalg.solve((Ak * m[:, None]).T @ Ak + lam * np.eye(len(x)), g)
        t = 1.0
        while lp(x + t * step) < lp(x) and t > 1e-8:
            t *= 0.5
        x = x + t * step
        if np.abs(step).max() < 1e-12:
            break
    return x


tgt = gsmvi_amd.BatchedGLMTarget(A, y, "poisson", prior_precision=LAM, counts=counts, offset=offset)
keys = np.arange(K) + 7

mean0, cov0, res = gsmvi_amd.lbfgs_init_batched(np.zeros((K, D)), tgt.lp, tgt.lp_g)
print(f"lbfgs_init_batched: {int(res.success.sum())} of {K} converged in {res.nlaunch} evaluation rounds; max |grad| "
      f"{np.abs(res.jac).max():.2e}")
fit = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g)
mean, cov = fit.fit(keys, mean=mean0, cov=cov0, batch_size=batch, niter=niter, verbose=False)
modes = np.stack([newton_map(A[k, :counts[k]], y[k, :counts[k]], offset[k, :counts[k]], LAM) for k in range(K)])

sd = np.sqrt(np.einsum("kii->ki", cov))
print(f"L-BFGS means against the Newton MAP: max |difference| {np.abs(mean0 - modes).max():.2e}")
print(f"GSMBatch means against the Newton MAP, in fitted standard deviations: median {np.median(np.abs(mean - modes) / sd):.3f}, "
      f"max {(np.abs(mean - modes) / sd).max():.3f}; reverts {int(fit.n_reverts.sum())}")
print("problem   fitted mean (first 3 coordinates)        Newton MAP                               true theta")
for k in range(min(K, 5)):
    f3 = lambda v: " ".join(f"{t:+.4f}" for t in v[:3])                                            # noqa: E731
    print(f"{k:7d}   {f3(mean[k]):40s} {f3(modes[k]):40s} {f3(theta[k])}")
