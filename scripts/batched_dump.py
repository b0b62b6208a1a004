"""Seeded dump of the batched GSM and BaM kernels' outputs, for before / after comparisons of a library change (DESIGN.md
section 9): at eight (D, B) shapes, K = 13 (a tail slot in the four-problem workgroups), the one-shot update, a 20-iteration
fit and a fit with one NaN target, for both methods -- 48 arrays of results; and the GLM entry points (score and density, the
logistic entry, Hessian and inverse, six Newton rounds, the predictive, three L-BFGS rounds, the leave-one-out) at K = 13 for the
four families with and without an offset, at (D, N, rows of X) shapes on both sides of every packing and tile boundary; and the
softmax entry points (score and density in the three ``want``s, Hessian and inverse, six Newton rounds, the leave-one-out, the
predictive, also with a NaN and with nothing but -inf among one problem's weights and a NaN in one draw) at K = 13, at
(C, P, N, rows of X, S) shapes on both sides of theirs; and the negative binomial and ordinal draw-based predictives at K = 4, at
(P, S, M) and (P, C, S, M) shapes on both sides of every tile boundary, with uniform and given weights, with and without y and
an offset, counts of 0, inside a tile and M, and the same verdict inputs; and the KL monitor's draw (one call and two
chunks) and log-density, Pathfinder's propose and select over five L-BFGS rounds, and one ADVI start and step, at K = 13 and
six D, with the fewest rows and one more than a tile; and the Hessian with its inverse and six Newton rounds from x0 = 0 of the
shared-design, negative binomial and ordinal Laplace entries at K = 13, at the smallest sizes where their mapping changes, with the
count of problems whose last-pivot or retry rule fired (``ist[:, 4] > 0``) printed per kernel.

  python scripts/batched_dump.py OUT.npz                 dump with the library the package loads
  GSMVI_HIP_LIB_VARIANT=old python scripts/batched_dump.py OUT.npz   ... with gsm-vi_amd/libgsmvi_hip_old.so
  python scripts/batched_dump.py --compare A.npz B.npz   bit-for-bit comparison (NaNs compare equal)
"""
import os
import sys

import numpy as np

SHAPES = ((1, 1), (4, 2), (5, 2), (10, 2), (16, 8), (17, 3), (33, 4), (64, 8))


# D: one lane, the four-problem packing's last, the first of one problem per workgroup, the largest; N: one row, a full tile of
# 32, one row more, three tiles; rows of X: one, an odd count above the packed tile of 16, one above the tile of 32
GLM_SHAPES = ((1, 1, 1), (1, 70, 33), (16, 32, 17), (16, 33, 33), (17, 33, 1), (17, 70, 17), (64, 32, 33), (64, 70, 17))
GLM_FAMILIES = ("logistic", "poisson", "probit", "gaussian")


# (C, P): the smallest model, the widest row, the most classes, the four-problem packing's last D, P % 4 != 0, D = 64 with
# P % 4 = 2; N: one row, a full tile of 32, one row more; rows of X as above; S: the fewest draws, one above a tile of 64
SOFTMAX_SHAPES = ((2, 1, 1, 1, 5), (2, 64, 33, 17, 65), (65, 1, 32, 33, 5), (17, 1, 33, 17, 65), (5, 3, 32, 33, 65), (33, 2, 33, 1, 5))


# D of the KL, Pathfinder and ADVI entries: one lane, an odd D, the four-problem packing's last, the first of one problem per
# workgroup, an odd D above it, the largest; rows: the fewest, and one more than a tile of the draw stage
INIT_DIMS = (1, 5, 16, 17, 33, 64)


# the three later Laplace families.  N: one row, a full tile of 32, one row more, three tiles.  Shared design: D on both sides of
# the four-problem packing, one lane and the largest.  Negative binomial: D = P + 1 the same.  Ordinal (P, C): D = 16 and 17, P on a
# block boundary (a block of rows that is all cutpoints), and both ways to D = 64
LAPLACE_N = (1, 32, 33, 70)
SHARED_LAPLACE_D = (1, 16, 17, 64)
NEGBIN_LAPLACE_P = (1, 15, 16, 63)
ORDINAL_LAPLACE_PC = ((1, 2), (13, 4), (13, 5), (16, 2), (16, 5), (1, 64), (40, 25))


def laplace_edges(rs, K, N):
    """what the K = 13 inputs of the three dumps below share: counts 0 for problem 1 and N for problem 2, lam = 0 for problem 0"""
    cnt = np.array([max(1, N - k) for k in range(K)])
    cnt[1], cnt[2] = 0, N
    lam = 0.1 + rs.random_sample(K)
    lam[0] = 0.0
    return cnt, lam


def negbin_laplace_inputs(P, N, K=13):
    """A, y, offset, counts, lam, theta mean and precision (K,) of the negative binomial dump: the recipe of the step tests
    (A = N(0, 1) / sqrt(P), beta* ~ 0.7 N(0, 1), offsets 1 + 0.3 N(0, 1), size 3), so that H at x0 = 0 is indefinite in theta for
    a large share of the problems and the last-pivot rule fires in the first rounds"""
    rs = np.random.RandomState(1000 * N + 10 * P + 3)
    A = rs.standard_normal((K, N, P)) / np.sqrt(P)
    o = 1.0 + 0.3 * rs.standard_normal((K, N))
    mu = np.exp(np.einsum("knp,kp->kn", A, 0.7 * rs.standard_normal((K, P))) + o)
    y = rs.poisson(rs.gamma(3.0, mu / 3.0)).astype(np.float64)
    cnt, lam = laplace_edges(rs, K, N)
    return A, y, o, cnt, lam, 0.2 * rs.standard_normal(K), 0.5 + rs.random_sample(K)


def ordinal_laplace_inputs(P, C, N, K=13):
    """A, labels, offset, counts, lam, kap (K,) of the ordinal dump: labels from a latent logistic variable cut at C - 1 sorted
    points, so every class occurs at the larger N; from x0 = 0 the chain terms make H indefinite where classes are many and
    the retry rule fires"""
    rs = np.random.RandomState(100000 * C + 1000 * P + 10 * N + 7)
    A = rs.standard_normal((K, N, P)) / np.sqrt(P)
    o = 0.3 * rs.standard_normal((K, N))
    z = np.einsum("knp,kp->kn", A, rs.standard_normal((K, P))) + o + rs.logistic(size=(K, N))
    cuts = np.sort(2.5 * rs.standard_normal((K, C - 1)), 1)
    y = (z[:, :, None] > cuts[:, None, :]).sum(2)
    cnt, lam = laplace_edges(rs, K, N)
    return A, y, o, cnt, lam, 0.5 + rs.random_sample(K)


def dump_laplace_families(out, K=13):
    """Hessian + inverse + info at random rows of X, then six Newton rounds from x0 = 0 with every state array after every round,
    for the shared-design, negative binomial and ordinal entries; problem 4 has a NaN in X and in x0"""
    from gsmvi_amd.engine import get_engine
    eng = get_engine()
    host = lambda *ts: np.concatenate([eng.to_numpy(t).astype(np.float64).reshape(K, -1) for t in ts], 1)     # noqa: E731
    state = ("x", "g", "d", "Xt", "sc", "ist")
    fired = {"negbin": 0, "ordinal": 0}

    def points(rs, D):
        X, x0 = rs.standard_normal((K, D)), np.zeros((K, D))
        X[4, D - 1] = x0[4, 0] = np.nan
        return eng.asarray(X), eng.asarray(x0)

    def rounds(tag, step, x0):
        st = eng.laplace_state_batched(x0)
        for r in range(6):
            step(st, r == 0)
            out[tag.replace("_", f"_laplace{r}_", 1)] = host(*(st[n] for n in state))
        return int((eng.to_numpy(st["ist"])[:, 4] > 0).sum())

    for N in LAPLACE_N:
        for D in SHARED_LAPLACE_D:
            for fi, family in enumerate(GLM_FAMILIES):
                rs = np.random.RandomState(20000 * D + 100 * N + fi)
                Ah = rs.standard_normal((N, D)) / np.sqrt(D)
                oh = 0.3 * rs.standard_normal((K, N))
                eta = Ah @ rs.standard_normal((D, K))
                eta = eta.T + oh
                tau_h = 0.5 + rs.random_sample(K)
                if family == "poisson":
                    yh = rs.poisson(np.exp(np.minimum(eta, 3.0))).astype(np.float64)
                elif family == "gaussian":
                    yh = eta + rs.standard_normal((K, N)) / np.sqrt(tau_h)[:, None]
                else:
                    yh = (rs.random_sample((K, N)) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
                _, lam_h = laplace_edges(rs, K, N)
                wh = rs.random_sample((K, N)) * (rs.random_sample((K, N)) < 0.7)       # some zero; problem 1: all zero
                wh[1] = 0.0
                A, y, off = eng.asarray(Ah), eng.asarray(yh), eng.asarray(oh)
                X, x0 = points(rs, D)
                for w in (None, eng.asarray(wh)):
                    model = dict(offset=off, weights=w, prior_prec=eng.batched_regs(lam_h),
                                 noise_prec=eng.batched_regs(tau_h) if family == "gaussian" else 1.0)
                    tag = f"shared_{family}_{'w' if w is not None else 'now'}_D{D}_N{N}"
                    out[tag.replace("_", "_hessian_", 1)] = host(*eng.glm_shared_hessian_batched(X, A, y, family, want="both", **model))
                    rounds(tag, lambda st, start: eng.laplace_shared_step_batched(st, A, y, family, start=start, **model), x0)
        for P in NEGBIN_LAPLACE_P:
            Ah, yh, oh, cnt, lam_h, tm_h, tk_h = negbin_laplace_inputs(P, N, K)
            A, y = eng.asarray(Ah), eng.asarray(yh)
            X, x0 = points(np.random.RandomState(31 * P + N), P + 1)
            for off in (None, eng.asarray(oh)):
                model = dict(offset=off, counts=eng.batched_counts(cnt), prior_prec=eng.batched_regs(lam_h),
                             log_size_mean=eng.batched_regs(tm_h), log_size_prec=eng.batched_regs(tk_h))
                tag = f"negbin_{'off' if off is not None else 'nooff'}_P{P}_N{N}"
                out[tag.replace("_", "_hessian_", 1)] = host(*eng.negbin_hessian_batched(X, A, y, want="both", **model))
                fired["negbin"] += rounds(tag, lambda st, start: eng.negbin_laplace_step_batched(st, A, y, start=start, **model), x0)
        for P, C in ORDINAL_LAPLACE_PC:
            Ah, yh, oh, cnt, lam_h, kap_h = ordinal_laplace_inputs(P, C, N, K)
            A, y = eng.asarray(Ah), eng.batched_labels(yh)
            X, x0 = points(np.random.RandomState(977 * P + 31 * C + N), P + C - 1)
            for off in (None, eng.asarray(oh)):
                model = dict(offset=off, counts=eng.batched_counts(cnt), prior_prec=eng.batched_regs(lam_h),
                             cut_prec=eng.batched_regs(kap_h))
                tag = f"ordinal_{'off' if off is not None else 'nooff'}_P{P}_C{C}_N{N}"
                out[tag.replace("_", "_hessian_", 1)] = host(*eng.ordinal_hessian_batched(X, A, y, C, want="both", **model))
                fired["ordinal"] += rounds(tag, lambda st, start: eng.ordinal_laplace_step_batched(st, A, y, C, start=start, **model), x0)
    print(f"problems that end their six rounds with ist[:, 4] > 0: negbin (last-pivot rule) {fired['negbin']}, "
          f"ordinal (retry rule) {fired['ordinal']}")


def dump_glm(out, K=13):
    """the outputs of every GLM entry point: counts 0 for problem 1 and N for problem 2, lam = 0 for problem 0, K values of
    tau for the gaussian family; every array as float64"""
    from gsmvi_amd.engine import get_engine
    eng = get_engine()
    host = lambda *ts: np.concatenate([eng.to_numpy(t).astype(np.float64).reshape(K, -1) for t in ts], 1)     # noqa: E731
    for D, N, rows in GLM_SHAPES:
        for fi, family in enumerate(GLM_FAMILIES):
            rs = np.random.RandomState(10000 * D + 100 * N + 10 * rows + fi)
            Ah = rs.standard_normal((K, N, D)) / np.sqrt(D)
            oh = 0.3 * rs.standard_normal((K, N))
            eta = np.einsum("knd,kd->kn", Ah, rs.standard_normal((K, D))) + oh
            tau_h = 0.5 + rs.random_sample(K)
            if family == "poisson":
                yh = rs.poisson(np.exp(np.minimum(eta, 3.0))).astype(np.float64)
            elif family == "gaussian":
                yh = eta + rs.standard_normal((K, N)) / np.sqrt(tau_h)[:, None]
            else:
                yh = (rs.random_sample((K, N)) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
            cnt = np.array([max(1, N - k) for k in range(K)])
            cnt[1], cnt[2] = 0, N
            lam_h = 0.1 + rs.random_sample(K)
            lam_h[0] = 0.0
            R = rs.standard_normal((K, D, D))
            A, y, X = eng.asarray(Ah), eng.asarray(yh), eng.asarray(rs.standard_normal((K, rows, D)))
            mean, cov = eng.asarray(0.3 * rs.standard_normal((K, D))), eng.asarray(R @ np.swapaxes(R, 1, 2) / D + 0.1 * np.eye(D))
            for off in (None, eng.asarray(oh)):
                model = dict(offset=off, counts=eng.batched_counts(cnt), prior_prec=eng.batched_regs(lam_h),
                             noise_prec=eng.batched_regs(tau_h) if family == "gaussian" else 1.0)
                tag = f"{family}_{'off' if off is not None else 'nooff'}_D{D}_N{N}_r{rows}"
                out[f"glm_{tag}"] = host(*eng.glm_batched(X, A, y, family, want="both", **model))
                if family == "logistic" and off is None:
                    out[f"logistic_{tag}"] = host(*eng.logistic_batched(X, A, y, model["counts"], model["prior_prec"], want="both"))
                out[f"hessian_{tag}"] = host(*eng.glm_hessian_batched(X[:, 0].contiguous(), A, y, family, want="both", **model))
                st = eng.laplace_state_batched(eng.zeros(K, D))
                for r in range(6):
                    eng.laplace_step_batched(st, A, y, family, start=r == 0, **model)
                    out[f"laplace{r}_{tag}"] = host(*(st[n] for n in ("x", "g", "d", "Xt", "sc", "ist")))
                out[f"predict_{tag}"] = host(*eng.glm_predict_batched(mean, cov, A, family, offset=off, y=y, counts=model["counts"],
                                                                      noise_prec=model["noise_prec"], nodes=8))
                st = eng.lbfgs_state_batched(eng.zeros(K, D))
                for r in range(3):
                    G, lp = eng.glm_batched(st["Xt"].reshape(K, 1, D), A, y, family, want="both", **model)
                    eng.lbfgs_step_batched(lp.reshape(K), G.reshape(K, D), st, start=r == 0)
                    out[f"lbfgs{r}_{tag}"] = host(*(st[n] for n in ("x", "g", "d", "Xt", "S", "Y", "sc", "ist")))
                out[f"lbfgs_cov_{tag}"] = host(eng.lbfgs_hess_inv_batched(st))
                S = 5 if rows == 1 else 65                  # the fewest draws, one above a tile of 64
                rl = np.random.RandomState(rs.randint(2 ** 31))
                Xd, logr = eng.asarray(0.5 * rl.standard_normal((K, S, D))), eng.asarray(rl.standard_normal((K, S)))
                out[f"loo_{tag}"] = host(*eng.psis_loo_batched(Xd, logr, eng.psis_weights_batched(logr)[0], A, y, family, offset=off,
                                                               counts=model["counts"], noise_prec=model["noise_prec"],
                                                               pointwise_loglik=True))


def dump_softmax(out, K=13):
    """the outputs of every softmax entry point: counts 0 for problem 1 and N for problem 2, lam = 0 for problem 0, the reference
    class among the labels; every array as float64"""
    from gsmvi_amd.engine import get_engine
    eng = get_engine()
    host = lambda *ts: np.concatenate([eng.to_numpy(t).astype(np.float64).reshape(K, -1) for t in ts], 1)     # noqa: E731
    for C, P, N, rows, S in SOFTMAX_SHAPES:
        D = (C - 1) * P
        rs = np.random.RandomState(100000 * C + 1000 * P + 10 * N + rows)
        yh = rs.randint(0, C, (K, N))
        yh[:, 0] = C - 1
        cnt = np.array([max(1, N - k) for k in range(K)])
        cnt[1], cnt[2] = 0, N
        lam_h = 0.1 + rs.random_sample(K)
        lam_h[0] = 0.0
        A, y = eng.asarray(rs.standard_normal((K, N, P)) / np.sqrt(P)), eng.batched_labels(yh)
        X = eng.asarray(rs.standard_normal((K, rows, D)))
        Xd, logr = eng.asarray(0.5 * rs.standard_normal((K, S, D))), eng.asarray(rs.standard_normal((K, S)))
        lw = eng.psis_weights_batched(logr)[0]
        model = dict(counts=eng.batched_counts(cnt), prior_prec=eng.batched_regs(lam_h))
        tag = f"C{C}_P{P}_N{N}_r{rows}_S{S}"
        out[f"softmax_g_{tag}"] = host(eng.softmax_batched(X, A, y, C, want="g", **model))
        out[f"softmax_lp_{tag}"] = host(eng.softmax_batched(X, A, y, C, want="lp", **model))
        out[f"softmax_both_{tag}"] = host(*eng.softmax_batched(X, A, y, C, want="both", **model))
        out[f"softmax_hessian_{tag}"] = host(*eng.softmax_hessian_batched(X[:, 0].contiguous(), A, y, C, want="both", **model))
        st = eng.laplace_state_batched(eng.zeros(K, D))
        for r in range(6):
            eng.softmax_laplace_step_batched(st, A, y, C, start=r == 0, **model)
            out[f"softmax_laplace{r}_{tag}"] = host(*(st[n] for n in ("x", "g", "d", "Xt", "sc", "ist")))
        out[f"softmax_loo_{tag}"] = host(*eng.psis_loo_softmax_batched(Xd, logr, lw, A, y, C, counts=model["counts"],
                                                                       pointwise_loglik=True))
        for wname, w in (("uniform", None), ("weighted", lw)):
            prob, _ = eng.softmax_predict_batched(Xd, w, A, C, counts=model["counts"])
            out[f"softmax_predict_{wname}_{tag}"] = host(prob)
            out[f"softmax_predict_{wname}_labels_{tag}"] = host(*eng.softmax_predict_batched(Xd, w, A, C, labels=y,
                                                                                             counts=model["counts"]))
        # the verdict paths: a NaN among problem 3's weights, nothing but -inf for problem 4 (softmax has no draw flag: the NaN
        # in one draw of problem 5 refuses the rows it reaches)
        Xv, lwv = eng.to_numpy(Xd).copy(), eng.to_numpy(lw).copy()
        Xv[5, S // 2, D - 1] = lwv[3, S - 1] = np.nan
        lwv[4] = -np.inf
        out[f"softmax_predict_verdict_{tag}"] = host(*eng.softmax_predict_batched(eng.asarray(Xv), eng.asarray(lwv), A, C, labels=y,
                                                                                  counts=model["counts"]))


# the draw-based predictives of the negative binomial and ordinal families, K = 4.  S: the fewest draws, one below, one above and
# exactly a tile of 64, four tiles and one draw; M: one row, one below, one above and exactly a tile of 16 rows, two tiles and one
# row; P: one column, P % 4 != 0, a multiple of 4, the largest; C: the fewest classes (no interior class), one and two interior
# classes, the most classes
NEGBIN_PREDICT_SHAPES = ((1, 5, 1), (3, 63, 15), (5, 257, 33), (4, 64, 16), (63, 65, 17))                         # (P, S, M)
ORDINAL_PREDICT_SHAPES = ((1, 2, 5, 1), (3, 3, 63, 15), (5, 4, 257, 33), (3, 2, 65, 17), (1, 64, 63, 17), (63, 2, 65, 33))  # (P, C, S, M)


def dump_draw_predict(out, K=4):
    """the negative binomial and ordinal predictives at every shape above: uniform and given lw, with and without y, with and
    without an offset; counts 0 for problem 0, a value that ends inside a tile for problem 1, M for problems 2 and 3.  Then, with
    everything given, the verdict inputs: a NaN in one draw of problem 2 and nothing but -inf among the weights of problem 3"""
    from gsmvi_amd.engine import get_engine
    eng = get_engine()
    host = lambda *ts: np.concatenate([eng.to_numpy(t).astype(np.float64).reshape(K, -1) for t in ts if t is not None], 1)     # noqa: E731

    def runs(tag, launch, rs, S, M, D, Xh, yd, od):
        cnt = eng.batched_counts(np.array([0, max(1, M - 5), M, M]))
        logr = eng.asarray(rs.standard_normal((K, S)))
        lw = eng.psis_weights_batched(logr)[0]
        X = eng.asarray(Xh)
        for wname, w in (("uniform", None), ("weighted", lw)):
            for yname, yv in (("noy", None), ("y", yd)):
                for oname, ov in (("nooff", None), ("off", od)):
                    out[f"{tag}_{wname}_{yname}_{oname}"] = host(*launch(X, w, yv, ov, cnt))
        Xv, lwv = Xh.copy(), eng.to_numpy(lw).copy()
        Xv[2, S // 2, D - 1] = np.nan
        lwv[3] = -np.inf
        out[f"{tag}_verdict"] = host(*launch(eng.asarray(Xv), eng.asarray(lwv), yd, od, cnt))
        Xv[2, S // 2, D - 1], Xv[2, S - 1, 0] = Xh[2, S // 2, D - 1], np.inf              # a beta column instead
        out[f"{tag}_verdict_beta"] = host(*launch(eng.asarray(Xv), eng.asarray(lwv), yd, od, cnt))

    for P, S, M in NEGBIN_PREDICT_SHAPES:
        rs = np.random.RandomState(100000 * P + 100 * S + M)
        A = eng.asarray(rs.standard_normal((K, M, P)) / np.sqrt(P))
        Xh = np.concatenate([0.5 * rs.standard_normal((K, S, P)), 1.0 + 0.3 * rs.standard_normal((K, S, 1))], 2)
        y, o = eng.asarray(rs.poisson(3.0, (K, M)).astype(np.float64)), eng.asarray(0.3 * rs.standard_normal((K, M)))
        runs(f"negbin_predict_P{P}_S{S}_M{M}", lambda X, w, yv, ov, cnt: eng.negbin_predict_batched(X, w, A, y=yv, offset=ov, counts=cnt),
             rs, S, M, P + 1, Xh, y, o)
    for P, C, S, M in ORDINAL_PREDICT_SHAPES:
        rs = np.random.RandomState(1000000 * P + 10000 * C + 100 * S + M)
        A = eng.asarray(rs.standard_normal((K, M, P)) / np.sqrt(P))
        Xh = np.concatenate([0.5 * rs.standard_normal((K, S, P)), -1.0 + 0.3 * rs.standard_normal((K, S, 1)),
                             -0.5 + 0.3 * rs.standard_normal((K, S, C - 2))], 2)
        y, o = eng.batched_labels(rs.randint(0, C, (K, M))), eng.asarray(0.3 * rs.standard_normal((K, M)))
        runs(f"ordinal_predict_P{P}_C{C}_S{S}_M{M}",
             lambda X, w, yv, ov, cnt: eng.ordinal_predict_batched(X, w, A, C, y=yv, offset=ov, counts=cnt), rs, S, M, P + C - 1, Xh, y, o)


def dump_initialisers(out, K=13):
    """the draw and log-density of the KL monitor (the draw as one call and as two chunks), Pathfinder's propose and select over
    five L-BFGS rounds on logistic posteriors (the base from the newest pair and the base 1), and one ADVI start and step;
    problem 3's covariance is not positive definite in the KL entries and in ADVI's start"""
    from gsmvi_amd.engine import get_engine
    import gsmvi_amd
    eng = get_engine()
    host = lambda *ts: np.concatenate([eng.to_numpy(t).astype(np.float64).reshape(K, -1) for t in ts], 1)     # noqa: E731
    seeds = eng.batched_seeds(range(100, 100 + K))
    for D in INIT_DIMS:
        # rows per tile of the draw stage: kb_tile_rows / pf_tile_rows of the two kernels, KB_Q = PF_Q = 4 elements per thread of
        # gb_nt(D) = 64 (D <= 16) or 256 threads; restated here, so it follows a change of either by hand
        tile = max(1, 4 * (64 if D <= 16 else 256) // D)
        rs = np.random.RandomState(7000 + D)
        R = rs.standard_normal((K, D, D))
        covh = R @ np.swapaxes(R, 1, 2) / D + 0.5 * np.eye(D)
        mh = rs.standard_normal((K, D))
        Ah = rs.standard_normal((K, 33, D)) / np.sqrt(D)
        yh = (rs.random_sample((K, 33)) < 1.0 / (1.0 + np.exp(-np.einsum("knd,kd->kn", Ah, mh)))).astype(np.float64)
        tgt = gsmvi_amd.BatchedLogisticTarget(eng.asarray(Ah), eng.asarray(yh), 0.5)
        bad = covh.copy()
        bad[3, D - 1, D - 1] = -1.0
        mean, cov = eng.asarray(0.3 * rs.standard_normal((K, D))), eng.asarray(bad)
        for n in (1, tile + 1):
            tag = f"D{D}_n{n}"
            X, lq, info = eng.kl_draw_batched(mean, cov, seeds, 3, 0, n)
            out[f"kl_draw_{tag}"] = host(X, lq, info)
            if n > 1:                                       # the same rows as two chunks, the second one not at a tile's start
                h = n // 2
                Xa, lqa, ia = eng.kl_draw_batched(mean, cov, seeds, 3, 0, h)
                Xb, lqb, ib = eng.kl_draw_batched(mean, cov, seeds, 3, h, n - h)
                out[f"kl_draw_chunks_{tag}"] = host(Xa, Xb, lqa, lqb, ia, ib)
            Y = eng.asarray(rs.standard_normal((K, n, D)))
            out[f"logq_{tag}"] = host(*eng.logq_batched(mean, cov, Y))
            for h0 in (0.0, 1.0):
                st = eng.lbfgs_state_batched(eng.asarray(0.1 * rs.standard_normal((K, D))))
                pf = eng.pathfinder_state_batched(st["x"], n)
                Xt = st["Xt"].reshape(K, 1, D)
                for r in range(5):
                    eng.lbfgs_step_batched(tgt.lp(Xt).reshape(K), tgt.lp_g(Xt).reshape(K, D), st, start=r == 0)
                    eng.pathfinder_propose_batched(st, pf, seeds, h0=h0)
                    out[f"pf_propose{r}_h{h0:g}_{tag}"] = host(*(pf[k] for k in ("seen", "fresh", "info", "mu", "cov", "X", "logq")))
                    eng.pathfinder_select_batched(tgt.lp(pf["X"]).sum(1), st, pf)
                    out[f"pf_select{r}_h{h0:g}_{tag}"] = host(*(pf[k] for k in ("elbo_last", "npts", "best_elbo", "best_mean",
                                                                                "best_cov", "best_it")))
                out[f"pf_hess_inv_h{h0:g}_{tag}"] = host(eng.lbfgs_hess_inv_batched(st))
            if n <= 32:                                     # ADVI's batch is at most 32
                P = D * (D + 1) // 2
                scales, info = eng.empty(K, P), eng.batched_ints(K)
                X, logq = eng.empty(K, n, D), eng.empty(K)
                eng.advi_init_batched(mean, cov, scales, info, seeds=seeds, X=X, logq=logq)
                out[f"advi_init_{tag}"] = host(scales, info, X, logq)
                loc, sc = mean.clone(), eng.asarray(np.linalg.cholesky(covh)[:, np.tril_indices(D)[0], np.tril_indices(D)[1]])
                mom = tuple(eng.zeros(K, m) for m in (D, D, P, P))
                G = eng.asarray(rs.standard_normal((K, n, D)))
                eng.advi_step_batched(G, loc, sc, mom, 1, 1e-2, seeds=seeds, call=1, Xout=X, logq=logq)
                out[f"advi_step_{tag}"] = host(loc, sc, *mom, X, logq)


def dump(path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gsmvi_amd
    K = 13
    out = {}
    for part, k in ((dump_glm, K), (dump_softmax, K), (dump_draw_predict, 4), (dump_initialisers, K), (dump_laplace_families, K)):
        part(out, k)
        print(f"{part.__name__}: {len(out)} arrays so far", flush=True)
    for D, B in SHAPES:
        rs = np.random.RandomState(100 * D + B)
        A = rs.standard_normal((K, D, D))
        cov = A @ np.swapaxes(A, 1, 2) / D + np.eye(D)
        m = rs.standard_normal((K, D))
        X = m[:, None, :] + rs.standard_normal((K, B, D))
        G = -rs.standard_normal((K, B, D))
        tag = f"D{D}_B{B}"
        out[f"gsm_update_{tag}"] = np.concatenate([a.reshape(K, -1) for a in gsmvi_amd.gsm_update_batched(X, G, m, cov)], 1)
        out[f"bam_update_{tag}"] = np.concatenate([a.reshape(K, -1) for a in gsmvi_amd.bam_update_batched(X, G, m, cov, 2.0)], 1)
        P = np.linalg.inv(cov)
        for nan in (False, True):
            Pn = P.copy()
            if nan:
                Pn[3, 0, 0] = np.nan
            tgt = gsmvi_amd.BatchedGaussianTarget(m, precision=Pn)
            name = "nanfit" if nan else "fit"
            g = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g)
            r = g.fit(np.arange(K), batch_size=B, niter=20, verbose=False)
            out[f"gsm_{name}_{tag}"] = np.concatenate([r[0].reshape(K, -1), r[1].reshape(K, -1), g.n_reverts[:, None]], 1)
            b = gsmvi_amd.BaMBatch(K, D, tgt.lp, tgt.lp_g)
            r = b.fit(np.arange(K), lambda i: 10.0 / (1 + i), batch_size=B, niter=20, verbose=False)
            out[f"bam_{name}_{tag}"] = np.concatenate([r[0].reshape(K, -1), r[1].reshape(K, -1), b.n_reverts[:, None]], 1)
    np.savez(path, **out)
    print(f"{path}: {len(out)} arrays, library {gsmvi_amd.library_path()} variant {os.environ.get('GSMVI_HIP_LIB_VARIANT', '')!r}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), "different contents"
    bad = [k for k in A.files if not (A[k].shape == B[k].shape and
                                      np.array_equal(A[k].view(np.uint64), B[k].view(np.uint64)))]
    print(f"{len(A.files)} arrays compared bit for bit: {len(bad)} differ {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    dump(sys.argv[1])
