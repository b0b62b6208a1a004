#!/usr/bin/env python3
"""A start that is chosen by how well it fits: ``pathfinder_init_batched`` walks the L-BFGS path of K posteriors at once, turns
every accepted iterate into a Gaussian from the pairs held at that moment, estimates its ELBO from a few draws and keeps the best.
The whole pipeline on K logistic and K softmax posteriors: ``pathfinder_init_batched`` -> ``psis_batched`` (can the start be
trusted?) -> ``GSMBatch.fit`` from it -> ``psis_batched`` again.  ``lbfgs_init_batched``'s start (the mode, an identity-based
covariance) goes through the same two checks for comparison.

    python examples/pathfinder_batched.py [K] [N] [batch] [niter] [draws]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100
batch = int(sys.argv[3]) if len(sys.argv) > 3 else 8
niter = int(sys.argv[4]) if len(sys.argv) > 4 else 200
draws = int(sys.argv[5]) if len(sys.argv) > 5 else 1024

rs = np.random.RandomState(1)
keys = np.arange(K) + 7


def logistic(D=5):
    A = 2.0 * rs.standard_normal((K, N, D)) / np.sqrt(D)
    theta = rs.standard_normal((K, D))
    y = (rs.random_sample((K, N)) < 1.0 / (1.0 + np.exp(-np.einsum("knd,kd->kn", A, theta)))).astype(np.float64)
    return gsmvi_amd.BatchedLogisticTarget(A, y, prior_precision=1.0)


def softmax(C=3, P=4):
    A = 2.0 * rs.standard_normal((K, N, P)) / np.sqrt(P)
    W = np.concatenate([rs.standard_normal((K, C - 1, P)), np.zeros((K, 1, P))], axis=1)
    eta = np.einsum("knp,kcp->knc", A, W)
    p = np.exp(eta - eta.max(2, keepdims=True))
    y = (rs.random_sample((K, N, 1)) > np.cumsum(p / p.sum(2, keepdims=True), axis=2)).sum(2).clip(0, C - 1)
    return gsmvi_amd.BatchedSoftmaxTarget(A, y.astype(np.int32), C, prior_precision=1.0)


def report(name, tgt, mean, cov):
    r = gsmvi_amd.psis_batched(tgt.lp, mean, cov, keys, num_draws=draws, moments=False)
    fin = r.info == 0
    print(f"    {name:28s} ELBO from {draws} draws, median {np.median(r.log_ratios.mean(1)[fin]):9.3f}   khat median "
          f"{np.median(r.khat[fin]):5.2f}   ok {r.ok.mean():6.1%}")


for title, tgt in (("logistic", logistic()), ("softmax, 3 classes", softmax())):
    D = tgt.D
    print(f"{K} {title} posteriors, D = {D}, N = {N}:")
    starts = {"lbfgs_init_batched": gsmvi_amd.lbfgs_init_batched(np.zeros((K, D)), tgt.lp, tgt.lp_g),
              "pathfinder_init_batched": gsmvi_amd.pathfinder_init_batched(np.zeros((K, D)), tgt.lp, tgt.lp_g)}
    res = starts["pathfinder_init_batched"][2]
    print(f"  Pathfinder: {int(res.success.sum())} of {K} got a start in {res.nlaunch} rounds ({res.nevals} evaluations of lp per "
          f"problem); the best path point is iteration {np.median(res.best_it):.0f} of {np.median(res.nit):.0f} (medians)")
    for name, (mean, cov, r) in starts.items():
        report(name, tgt, mean, cov)
        gsm = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g)
        m, c = gsm.fit(keys, mean=mean, cov=cov, batch_size=batch, niter=niter, verbose=False)
        report(f"  + GSMBatch.fit, {niter} its", tgt, m, c)
        print(f"      reverts {int(np.asarray(gsm.n_reverts).sum())}")
