#!/usr/bin/env python3
"""Using fitted classification models: K three-class multinomial logit posteriors are fitted on the first N rows of every problem
by ``laplace_init_softmax_batched`` -> a short ``GSMBatch.fit``; ``predict_softmax_batched`` then draws S points of every q_k and,
in one launch, gives the predictive class probabilities of the M held-out rows, their labels and the held-out score (the log
predictive density summed per problem).  Printed: the accuracy and the elpd per held-out row with uniform draws of q_k and with
the PSIS-weighted draws (the importance-corrected predictive: one more launch and one call of ``lp``; the draws are the same), the
share of problems whose q_k the PSIS check calls usable, and the first problems' numbers.

    python examples/predict_softmax_batched.py [K] [P] [N] [M] [batch] [niter] [draws]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
N = int(sys.argv[3]) if len(sys.argv) > 3 else 150
M = int(sys.argv[4]) if len(sys.argv) > 4 else 50
batch = int(sys.argv[5]) if len(sys.argv) > 5 else 8
niter = int(sys.argv[6]) if len(sys.argv) > 6 else 200
draws = int(sys.argv[7]) if len(sys.argv) > 7 else 1024
C = 3
D = (C - 1) * P

rs = np.random.RandomState(1)
A = 2.0 * rs.standard_normal((K, N + M, P)) / np.sqrt(P)
W = rs.standard_normal((K, C - 1, P))
eta = np.concatenate([np.einsum("knp,kcp->knc", A, W), np.zeros((K, N + M, 1))], axis=2)
prob = np.exp(eta - eta.max(axis=2, keepdims=True))
cdf = np.cumsum(prob / prob.sum(axis=2, keepdims=True), axis=2)
y = np.minimum((rs.random_sample((K, N + M, 1)) > cdf).sum(axis=2), C - 1)
keys = np.arange(K) + 7

tgt = gsmvi_amd.BatchedSoftmaxTarget(A[:, :N], y[:, :N], C, prior_precision=1.0)
m0, c0, res = gsmvi_amd.laplace_init_softmax_batched(tgt, as_torch=True)
mean, cov = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g).fit(keys, mean=m0, cov=c0, batch_size=batch, niter=niter, verbose=False,
                                                            as_torch=True)
A_new, y_new = A[:, N:], y[:, N:]
uni = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, y=y_new, num_draws=draws)
imp = gsmvi_amd.predict_softmax_batched(tgt, mean, cov, A_new, keys, y=y_new, num_draws=draws, weights="psis")
ok = np.asarray(imp.psis.ok.cpu().numpy())
print(f"K = {K} problems, D = {D}, {N} training and {M} held-out rows each, S = {uni.num_draws} draws; Laplace converged in "
      f"{int(np.asarray(res.success).sum())} of {K}")
for name, r in (("uniform draws", uni), ("PSIS-weighted", imp)):
    print(f"  {name}: {r.nlaunch} launches   accuracy {(r.label == y_new).mean():6.1%}   elpd per held-out row "
          f"{r.elpd.sum() / (K * M):8.4f}")
print(f"  q_k usable by the PSIS check (khat < {imp.psis.threshold:.3f}): {ok.mean():6.1%}; largest change of a probability by the "
      f"weights {np.abs(imp.prob - uni.prob).max():.3f}")
oracle = np.log(np.take_along_axis(prob[:, N:] / prob[:, N:].sum(axis=2, keepdims=True), y_new[:, :, None], 2)).mean()
print(f"  the generating coefficients' log density per held-out row: {oracle:8.4f}")
for k in range(min(K, 4)):
    print(f"  problem {k}: accuracy {(uni.label[k] == y_new[k]).mean():6.1%}   elpd {uni.elpd[k]:8.2f} (uniform) {imp.elpd[k]:8.2f} (psis)"
          f"   khat {float(imp.psis.khat[k]):5.2f}")
