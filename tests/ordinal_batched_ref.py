"""Numpy restatements of the batched ordinal target (gsmvi_ordinal_batched_f64, csrc/gsmvi_ordinal_batched.hip and
csrc/gsmvi_ordinal_link.h), the generator of its test inputs and a stand-in engine for the host logic of BatchedOrdinalTarget.
Test-only.  For problem k with design matrix A_k (N, P), labels y_k in 0 .. C - 1, offsets o_k, n_k valid rows, at x = (beta, delta),
cut_0 = delta_0, cut_j = cut_{j-1} + exp(delta_j), a = cut_{y-1} - eta, b = cut_y - eta, w = exp(delta_y) for an interior class:

    t = -[y <= C-2] softplus(-b) - [y >= 1] softplus(a) + [interior] log1mexp(w)
    u_lo = -sigma(a) - [interior] / expm1(w),   u_hi = sigma(-b) + [interior] / expm1(w),   r_eta = sigma(a) - sigma(-b)
    lp_k(x) = sum_n t_n - lam_k |beta|^2 / 2 - kap_k |delta|^2 / 2
    gcut_j = sum_n ([y_n = j + 1] u_lo,n + [y_n = j] u_hi,n)
    grad lp_k(x) = (sum_n r_eta,n a_n - lam_k beta,  sum_{j >= 0} gcut_j - kap_k delta_0,  exp(delta_i) sum_{j >= i} gcut_j - kap_k delta_i)

``link`` is the restatement of the kernel's forms operation by operation, in float64 or np.longdouble; ``score_and_lp`` sums the
observations in ascending order and the cutpoints' suffix sums from j = C - 2 downwards, as the kernel does.  ``score_and_lp_ld`` is
the same in np.longdouble: the reference of the GPU test.  ``link3`` is the C = 3 link per element through ``score_and_lp`` (P = 1,
N = 1, A = 1, beta = 0, eta as the offset, no priors): the quantities of tests/ordinal_link_truth.py."""
import numpy as np
import torch

W_MIN = 2.2250738585072014e-308                  # the smallest positive normal number
LOG2 = 0.6931471805599453


def gap(w):
    """(log1mexp(w), 1 / expm1(w)) of the gaps w = exp(delta_j) > 0, in w's precision: ord_gap of the link header"""
    with np.errstate(all="ignore"):
        lm = np.where(w < LOG2, np.log(-np.expm1(-w)), np.log1p(-np.exp(-w)))
        return lm, 1 / np.expm1(w)


def _sps(z):
    """softplus(z), sigma(z) from one exponential: ord_sps"""
    e = np.exp(-np.abs(z))
    q = 1 + e
    return np.where(z > 0, z, 0) + np.log1p(e), np.where(z >= 0, 1 / q, e / q)


def link(eta, y, cut, lm, qe):
    """(r_eta, u_lo, u_hi, t) at eta (rows, n) for the labels y (n,) in 0 .. C - 1 and the rows' cut, lm, qe (rows, C - 1): the
    kernel's forms, in the precision of the inputs"""
    C = cut.shape[1] + 1
    L = eta.dtype.type
    with np.errstate(all="ignore"):
        lo, hi = (y >= 1)[None, :], (y <= C - 2)[None, :]
        inner = lo & hi
        ya, yb = np.clip(y - 1, 0, C - 2), np.clip(y, 0, C - 2)
        spa, sga = _sps(cut[:, ya] - eta)
        spb, sgb = _sps(-(cut[:, yb] - eta))
        zero = L(0)
        spa, sga, spb, sgb = np.where(lo, spa, zero), np.where(lo, sga, zero), np.where(hi, spb, zero), np.where(hi, sgb, zero)
        t = (-spb - spa) + np.where(inner, lm[:, yb], zero)
        q = np.where(inner, qe[:, yb], zero)
        ulo = np.where(lo, -sga - q, zero)
        uhi = np.where(hi, sgb + q, zero)
        return sga - sgb, ulo, uhi, t


def cutpoints(delta, L=np.float64):
    """(rows, C - 1) parameters -> (cut, w): the cutpoints as one chain in j, and w_j = exp(delta_j) (column 0: 1)"""
    delta = np.asarray(delta, dtype=L)
    with np.errstate(all="ignore"):
        w = np.exp(delta)
        w[:, 0] = 1
        cut = np.empty_like(delta)
        cut[:, 0] = delta[:, 0]
        for j in range(1, delta.shape[1]):
            cut[:, j] = cut[:, j - 1] + w[:, j]
    return cut, w


def _score_and_lp(A, y, offset, counts, lam, kap, X, C, L):
    A, X = np.asarray(A, dtype=L), np.asarray(X, dtype=L)
    y = np.asarray(y)
    K, N, P = A.shape
    lc = C - 1
    assert X.shape[2] == P + lc
    lam, kap = (np.broadcast_to(np.asarray(v, dtype=L), (K,)) for v in (lam, kap))
    G, lp = np.empty(X.shape, dtype=L), np.empty(X.shape[:2], dtype=L)
    for k in range(K):
        n = N if counts is None else int(min(max(int(counts[k]), 0), N))
        Ak, beta, delta = A[k, :n], X[k, :, :P], X[k, :, P:]
        yk = np.clip(y[k, :n].astype(np.int64), 0, C - 1)                 # (the kernel clamps a label as it stages its tile)
        rows = X.shape[1]
        with np.errstate(all="ignore"):
            cut, w = cutpoints(delta, L)
            lm, qe = gap(w)
            eta = np.zeros((rows, n), dtype=L)
            for j in range(P):                                          # the kernel's chain over the columns
                eta = eta + beta[:, j, None] * Ak[None, :, j]
            if offset is not None:
                eta = eta + np.asarray(offset, dtype=L)[k, None, :n]
            re, ulo, uhi, t = link(eta, yk, cut, lm, qe)
            g, gcut, s = np.zeros(beta.shape, dtype=L), np.zeros(delta.shape, dtype=L), np.zeros(rows, dtype=L)
            jj = np.arange(lc)[None, :]
            for i in range(n):                                          # ascending n, one chain per output
                g, s = g + re[:, i, None] * Ak[None, i, :], s + t[:, i]
                gcut = gcut + np.where(yk[i] == jj + 1, ulo[:, i, None], np.where(yk[i] == jj, uhi[:, i, None], L(0)))
            G[k, :, :P] = g - lam[k] * beta
            sfx = np.zeros(rows, dtype=L)
            for j in range(lc - 1, -1, -1):                             # the suffix sums, from j = C - 2 downwards
                sfx = sfx + gcut[:, j]
                G[k, :, P + j] = (sfx if j == 0 else w[:, j] * sfx) - kap[k] * delta[:, j]
            bb, dd = np.zeros(rows, dtype=L), np.zeros(rows, dtype=L)
            for j in range(P):
                bb = bb + beta[:, j] * beta[:, j]
            for j in range(lc):
                dd = dd + delta[:, j] * delta[:, j]
            lp[k] = (s - L(0.5) * lam[k] * bb) - L(0.5) * kap[k] * dd
            w64 = np.exp(X[k, :, P + 1:].astype(np.float64))
        bad = ~np.isfinite(X[k].astype(np.float64)).all(1) | ~((w64 >= W_MIN) & (w64 < np.inf)).all(1)
        G[k, bad] = np.nan
        lp[k, bad] = np.nan
    return G, lp


def score_and_lp(A, y, offset, counts, lam, kap, X, C):
    """A (K, N, P), y (K, N) integers, offset (K, N) or None, counts (K,) or None, lam, kap a number or (K,), X (K, rows,
    P + C - 1) -> G (K, rows, P + C - 1), lp (K, rows) in float64: the kernel's forms, sums in its order, and its row flag"""
    return _score_and_lp(A, y, offset, counts, lam, kap, X, C, np.float64)


def score_and_lp_ld(A, y, offset, counts, lam, kap, X, C):
    """the same in np.longdouble (rounded to float64 by the caller): the GPU test's reference"""
    return _score_and_lp(A, y, offset, counts, lam, kap, X, C, np.longdouble)


def link3_problems(eta, d0, d1, y):
    """the truth grid as one problem per point: A (K, 1, 1) = 1, labels (K, 1), offset (K, 1) = eta, X (K, 1, 3) = (0, d0, d1)"""
    K = len(eta)
    X = np.stack([np.zeros(K), d0, d1], axis=1)[:, None, :]
    return np.ones((K, 1, 1)), np.asarray(y, dtype=np.int32)[:, None], np.asarray(eta, dtype=np.float64)[:, None], X


def link3(eta, d0, d1, y):
    """(t, re, d0, d1) of the C = 3 link per element, float64, through ``score_and_lp`` without priors"""
    A, yy, o, X = link3_problems(eta, d0, d1, y)
    G, lp = score_and_lp(A, yy, o, None, 0.0, 0.0, X, 3)
    return lp[:, 0], G[:, 0, 0], G[:, 0, 1], G[:, 0, 2]


def logistic_score_and_lp(A, y, lam, X):
    """the logistic restatement (the GLM kernel's forms: softplus and sigma from one exponential): lp = sum_n [y eta -
    softplus(eta)] - lam |x|^2 / 2 and its gradient, sums in ascending n; A (K, N, D), y (K, N) in {0, 1}, X (K, rows, D)"""
    K, N, D = A.shape
    G, lp = np.empty(X.shape), np.empty(X.shape[:2])
    for k in range(K):
        eta = np.zeros((X.shape[1], N))
        for j in range(D):
            eta = eta + X[k, :, j, None] * A[k, None, :, j]
        sp, sg = _sps(eta)
        g, s = np.zeros(X[k].shape), np.zeros(X.shape[1])
        for i in range(N):
            g, s = g + (y[k, i] - sg[:, i, None]) * A[k, None, i, :], s + (y[k, i] * eta[:, i] - sp[:, i])
        G[k] = g - lam * X[k]
        lp[k] = s - 0.5 * lam * (X[k] * X[k]).sum(1)
    return G, lp


def make_inputs(K, N, P, C, rows, seed=None, poison=True):
    """The inputs of the tests: RandomState(N + P + 64 C) (or ``seed``); A = N(0, 1) / sqrt(P), offsets 0.3 N(0, 1), beta* ~
    N(0, 1), planted cutpoints sorted N(0, 1.5^2) and y drawn from the model; the last problem (when K > 2) has no label C - 1 (they
    become C - 2: a class absent from the data); counts = N for problem 0, 0 for problem 1 (when K > 1) and max(1, N - 1 - 3 k)
    after it; lam = 0 for problem 0 and 0.1 + U(0, 1) after it, kap = 2 U(0, 1) with kap = 0 for problem 0; X = (N(0, 1), delta_0 ~
    N(0, 1), delta_j ~ U(-2, 1.5)): gaps on both sides of log 2.  ``poison``: the rows beyond counts hold NaN (A), C + 3 and -7 (y)
    and inf (offset).  Returns A, y (int64), offset, counts (int32), lam, kap, X."""
    rs = np.random.RandomState(N + P + 64 * C if seed is None else seed)
    A = rs.standard_normal((K, N, P)) / np.sqrt(P)
    offset = 0.3 * rs.standard_normal((K, N))
    beta = rs.standard_normal((K, P))
    cuts = np.sort(1.5 * rs.standard_normal((K, C - 1)), axis=1)
    eta = np.einsum("knp,kp->kn", A, beta) + offset
    u = rs.random_sample((K, N))
    cdf = 1.0 / (1.0 + np.exp(-(cuts[:, None, :] - eta[:, :, None])))       # P(y <= j)
    y = (u[:, :, None] > cdf).sum(2).astype(np.int64)
    if K > 2:
        y[K - 1] = np.minimum(y[K - 1], max(C - 2, 0))
    counts = np.array([N if k == 0 else 0 if k == 1 else max(1, N - 1 - 3 * k) for k in range(K)], dtype=np.int32)
    lam = 0.1 + rs.random_sample(K)
    lam[0] = 0.0
    kap = 2.0 * rs.random_sample(K)
    kap[0] = 0.0
    X = np.concatenate([rs.standard_normal((K, rows, P + 1)), rs.uniform(-2.0, 1.5, (K, rows, C - 2))], axis=2)
    if poison:
        for k in range(K):
            A[k, counts[k]:] = np.nan
            y[k, counts[k]:] = [C + 3, -7][k % 2]
            offset[k, counts[k]:] = np.inf
    return A, y, offset, counts, lam, kap, X


class RestatementEngine:
    """the engine calls BatchedOrdinalTarget makes, on numpy and the float64 restatement; ``calls`` records every one"""
    name = "restatement-ordinal(test-only)"

    def __init__(self):
        self.calls = []

    def asarray(self, x):
        self.calls.append("asarray")
        return np.array(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)

    def to_numpy(self, a):
        return np.asarray(a)

    def batched_counts(self, values):
        self.calls.append("batched_counts")
        return np.asarray(values, dtype=np.int32).reshape(-1)

    def batched_regs(self, values):
        self.calls.append("batched_regs")
        return np.asarray(values, dtype=np.float64).reshape(-1)

    def batched_labels(self, values):
        self.calls.append("batched_labels")
        return np.ascontiguousarray(values, dtype=np.int32)

    def ordinal_batched(self, X, A, y, C, offset=None, counts=None, prior_prec=1.0, cut_prec=1.0, out=None, lp_out=None, want="g"):
        self.calls.append(("ordinal", want, out is not None))
        self.last = dict(A=A, y=y, C=C, offset=offset, counts=counts, prior_prec=prior_prec, cut_prec=cut_prec)
        assert A.dtype == np.float64 and y.dtype == np.int32 and (counts is None or counts.dtype == np.int32)
        assert offset is None or offset.dtype == np.float64
        G, lp = score_and_lp(A, y, offset, counts, prior_prec, cut_prec, X, C)
        if out is not None:
            out[...] = G
            G = out
        return G if want == "g" else lp if want == "lp" else (G, lp)
