#!/usr/bin/env python3
"""Using fitted rating models: K cumulative-logit (proportional odds) posteriors over (beta, cutpoints) are fitted on the first N
rows of every problem by ``laplace_init_ordinal_batched``; ``predict_ordinal_batched`` then draws S points of every q_k and, in one
launch, gives the predictive probabilities of the C ordered classes for the M held-out rows, their most probable and their median
class and the held-out score (the log predictive density summed per problem).  Printed: the accuracy of the median class, its mean
absolute error in class steps and the elpd per held-out row with uniform draws of q_k and with the PSIS-weighted draws (the
importance-corrected predictive: one more launch and one call of ``lp``; the draws are the same), the share of problems whose q_k
the PSIS check calls usable, and the first problems' numbers.

    python examples/predict_ordinal_batched.py [K] [P] [C] [N] [M] [draws]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gsmvi_amd

K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
C = int(sys.argv[3]) if len(sys.argv) > 3 else 5
N = int(sys.argv[4]) if len(sys.argv) > 4 else 150
M = int(sys.argv[5]) if len(sys.argv) > 5 else 50
draws = int(sys.argv[6]) if len(sys.argv) > 6 else 1024

rs = np.random.RandomState(1)
A = 2.0 * rs.standard_normal((K, N + M, P)) / np.sqrt(P)
offset = 0.3 * rs.standard_normal((K, N + M))
eta = np.einsum("knp,kp->kn", A, rs.standard_normal((K, P))) + offset
cuts = np.linspace(-1.5, 1.5, C - 1)
cdf = 1.0 / (1.0 + np.exp(-(cuts[None, None, :] - eta[:, :, None])))                  # P(y <= j)
y = (rs.random_sample((K, N + M))[:, :, None] > cdf).sum(2)
keys = np.arange(K) + 7

tgt = gsmvi_amd.BatchedOrdinalTarget(A[:, :N], y[:, :N], C, prior_precision=1.0, cut_precision=1.0, offset=offset[:, :N])
mean, cov, res = gsmvi_amd.laplace_init_ordinal_batched(tgt, as_torch=True)
A_new, o_new, y_new = A[:, N:], offset[:, N:], y[:, N:]
uni = gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, offset=o_new, y=y_new, num_draws=draws)
imp = gsmvi_amd.predict_ordinal_batched(tgt, mean, cov, A_new, keys, offset=o_new, y=y_new, num_draws=draws, weights="psis")
ok = np.asarray(imp.psis.ok.cpu().numpy())
print(f"K = {K} problems, C = {C} classes, D = {P + C - 1}, {N} training and {M} held-out rows each, S = {uni.num_draws} draws; "
      f"Laplace converged in {int(np.asarray(res.success).sum())} of {K}")
for name, r in (("uniform draws", uni), ("PSIS-weighted", imp)):
    print(f"  {name}: {r.nlaunch} launches   accuracy of the median class {(r.median == y_new).mean():6.1%} (most probable class "
          f"{(r.label == y_new).mean():6.1%})   mean |median - y| {np.abs(r.median - y_new).mean():5.3f}   elpd per held-out row "
          f"{r.elpd.sum() / (K * M):8.4f}")
print(f"  q_k usable by the PSIS check (khat < {imp.psis.threshold:.3f}): {ok.mean():6.1%}; largest change of a probability by the "
      f"weights {np.abs(imp.prob - uni.prob).max():.3f}")
edges = np.concatenate([np.zeros((K, M, 1)), cdf[:, N:], np.ones((K, M, 1))], axis=2)
oracle = np.log(np.take_along_axis(np.diff(edges, axis=2), y_new[:, :, None], 2)).mean()
print(f"  the generating model's log density per held-out row: {oracle:8.4f}; chance accuracy {1 / C:6.1%}")
for k in range(min(K, 4)):
    print(f"  problem {k}: accuracy of the median {(uni.median[k] == y_new[k]).mean():6.1%}   elpd {uni.elpd[k]:8.2f} (uniform) "
          f"{imp.elpd[k]:8.2f} (psis)   khat {float(imp.psis.khat[k]):5.2f}")
