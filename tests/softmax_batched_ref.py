"""Numpy restatement of the batched softmax target (gsmvi_softmax_batched_f64, csrc/gsmvi_softmax_batched.hip), the generator of
its test inputs, the mirror of the launch's X-tile rule and a stand-in engine for the host logic of BatchedSoftmaxTarget.
Test-only.  For problem k with design matrix A_k (N, P), integer labels y_k in 0 .. C - 1, n_k valid rows and prior precision
lam_k, class C - 1 the reference class and x[c P + j] = W_cj:

    eta_nc = a_n . w_c  (c < C-1),   eta_n,C-1 = 0
    m_n    = max_c eta_nc            (over all C values, the 0 included)
    s_n    = sum_{c=0..C-1} exp(eta_nc - m_n) = 1 + rest_n     (class order, the reference class last: ``s_minus_one``)
    lp(x)  = sum_{n<n_k} [ eta_n,y_n - m_n - log s_n ] - lam_k |x|^2 / 2     (log s_n as log1p(rest_n): ``log_s``)
    g_cj   = sum_{n<n_k} ( [y_n = c] - exp(eta_nc - m_n)/s_n ) a_nj - lam_k x_cj      (c < C-1)

with the kernel's NaN rule: a row of X with a non-finite entry, or for which some valid eta is not finite, gets NaN outputs.  It
is pinned to torch autograd of the written density in tests/test_softmax_batched_cpu.py."""
import numpy as np
import torch

# the (C, P) of the GPU grid: smallest; the D = 16 / 17 packing switch; odd D; the D = 64 maximum
SHAPES = [(2, 1), (3, 1), (2, 5), (3, 3),
          (2, 16), (2, 17), (3, 8), (5, 4), (17, 1), (18, 1),
          (4, 7),
          (2, 64), (3, 32), (5, 16), (9, 8), (17, 4), (33, 2), (65, 1)]
NS = [1, 31, 32, 33, 65]                  # the edges of the 32-row tile of A and of its prefetch
NCS = [1, 17, 33]                         # the edges of the 16- and 32-row tiles of X; x_tile(C, P) and x_tile + 1 are added per shape


def x_tile(C, P):
    """rows of X one tile of a launch holds (sb_tq of the kernel file): at most 32 (16 in the four-problem packing), at most 4
    outputs per thread in the score pass, and within 64 KB of LDS per workgroup"""
    D = (C - 1) * P
    nt = 64 if D <= 16 else 256
    cap = min(32 if nt == 256 else 16, 4 * nt // D)
    budget = 64 * 1024 // 8 // (256 // nt) - (32 * (P | 1) + 32)
    return min(cap, budget // ((D | 1) + 1 + 33 * C))


def lds_doubles(C, P, tq, want):
    """LDS doubles per problem of a launch holding tq rows of X; want: 1 = G, 2 = lp, 3 = both"""
    D = (C - 1) * P
    return 32 * (P | 1) + 32 + tq * ((D | 1) + 1 + 33 * ((C - 1) + (1 if want & 2 else 0)))


def nc_grid(C, P):
    t = x_tile(C, P)
    return sorted(set(NCS) | {t, t + 1})


def s_minus_one(e):
    """rest = s - 1 of the terms e (..., C) = exp(eta - m) <= 1 as the kernels sum it (sm_add_term of csrc/gsmvi_softmax_model.h):
    a term is exactly 1 for a class that attains m and below 1 otherwise, so floor(e) tells them apart; the terms below 1 in
    class order (the reference class last), then the count of the terms that are 1, less one"""
    rest, nt = np.zeros(e.shape[:-1], dtype=e.dtype), np.zeros(e.shape[:-1], dtype=e.dtype)
    for c in range(e.shape[-1]):
        f = np.floor(e[..., c])
        rest, nt = rest + (e[..., c] - f), nt + f
    return rest + (nt - 1)


def log_s(rest, s):
    """log s = log1p(rest) for s = 1 + rest as the kernels form it (sm_log_s): log(s) plus what the rounding of s dropped,
    d = rest - (s - 1), times 2 - s for 1 / s below s = 2 and nothing from there on; log(s) alone is 0 where rest < eps / 2"""
    d = rest - (s - 1)
    return np.log(s) + np.where(s < 2, d * (2 - s), 0 * d)


def score_and_lp(A, y, C, counts, lam, X, dtype=np.float64):
    """A (K, N, P), y (K, N) integers, C classes, counts (K,) or None, lam a number or (K,), X (K, rows, (C - 1) P) ->
    G (K, rows, D), lp (K, rows) in ``dtype`` (float64 or np.longdouble); a per-problem loop with the kernel's NaN rule."""
    A, X = np.asarray(A, dtype=dtype), np.asarray(X, dtype=dtype)
    y = np.asarray(y).astype(np.int64)
    K, N, P = A.shape
    rows, D = X.shape[1], X.shape[2]
    assert D == (C - 1) * P
    lam = np.broadcast_to(np.asarray(lam, dtype=dtype), (K,))
    G, lp = np.empty(X.shape, dtype=dtype), np.empty(X.shape[:2], dtype=dtype)
    for k in range(K):
        n = N if counts is None else int(min(max(int(counts[k]), 0), N))
        Ak, yk = A[k, :n], y[k, :n]
        W = X[k].reshape(rows, C - 1, P)
        with np.errstate(all="ignore"):
            eta = np.concatenate([np.einsum("np,rcp->rnc", Ak, W), np.zeros((rows, n, 1), dtype=dtype)], axis=2)    # (rows, n, C)
            m = eta.max(axis=2, keepdims=True) if n else eta[:, :, :1]
            e = np.exp(eta - m)
            rest = s_minus_one(e)
            s = 1 + rest
            hot = (yk[:, None] == np.arange(C)[None, :]).astype(dtype)  # (n, C)
            etay = (eta * hot[None]).sum(axis=2)
            r = hot[None, :, :C - 1] - e[:, :, :C - 1] / s[:, :, None]
            G[k] = np.einsum("rnc,np->rcp", r, Ak).reshape(rows, D) - lam[k] * X[k]
            lp[k] = (etay - m[:, :, 0] - log_s(rest, s)).sum(axis=1) - 0.5 * lam[k] * (X[k] * X[k]).sum(axis=1)
        bad = ~np.isfinite(X[k]).all(axis=1) | ~np.isfinite(eta).all(axis=(1, 2))
        G[k, bad] = np.nan
        lp[k, bad] = np.nan
    return G, lp


def make_inputs(K, N, C, P, rows, scale=1.0, seed=None):
    """The inputs of the tests: RandomState(N + 64 C + P) (or ``seed``); A = scale N(0, 1) / sqrt(P), W* ~ N(0, 1) and the labels
    drawn from the model at W*, counts = N for problem 0 and max(1, N - 1 - 3 k) after it, lam = 0 for problem 0 and 0.1 +
    U(0, 1) after it, X = scale N(0, 1).  Returns A, y (int32), counts (int32), lam, X."""
    rs = np.random.RandomState(N + 64 * C + P if seed is None else seed)
    D = (C - 1) * P
    A = scale * rs.standard_normal((K, N, P)) / np.sqrt(P)
    W = rs.standard_normal((K, C - 1, P))
    eta = np.concatenate([np.einsum("knp,kcp->knc", A, W), np.zeros((K, N, 1))], axis=2)
    p = np.exp(eta - eta.max(axis=2, keepdims=True))
    cdf = np.cumsum(p / p.sum(axis=2, keepdims=True), axis=2)
    u = rs.random_sample((K, N, 1))
    y = np.minimum((u > cdf).sum(axis=2), C - 1).astype(np.int32)
    counts = np.array([N if k == 0 else max(1, N - 1 - 3 * k) for k in range(K)], dtype=np.int32)
    lam = 0.1 + rs.random_sample(K)
    lam[0] = 0.0
    X = scale * rs.standard_normal((K, rows, D))
    return A, y, counts, lam, X


def max_abs_eta(A, counts, X, C):
    """the largest |eta| over the valid rows"""
    K, N, P = A.shape
    W = X.reshape(K, X.shape[1], C - 1, P)
    return max(float(np.abs(np.einsum("np,rcp->rnc", A[k, :counts[k]], W[k])).max()) for k in range(K))


class RestatementEngine:
    """the engine calls BatchedSoftmaxTarget makes, on numpy and the restatement; ``calls`` records every one"""
    name = "restatement-softmax(test-only)"

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

    def batched_labels(self, values):
        self.calls.append("batched_labels")
        return np.ascontiguousarray(values, dtype=np.int32)

    def batched_regs(self, values):
        self.calls.append("batched_regs")
        return np.asarray(values, dtype=np.float64).reshape(-1)

    def softmax_batched(self, X, A, labels, num_classes, counts=None, prior_prec=1.0, out=None, lp_out=None, want="g"):
        self.calls.append(("softmax", num_classes, want, out is not None))
        assert A.dtype == np.float64 and labels.dtype == np.int32 and (counts is None or counts.dtype == np.int32)
        G, lp = score_and_lp(A, labels, num_classes, counts, prior_prec, X)
        if out is not None:
            out[...] = G
            G = out
        return G if want == "g" else lp if want == "lp" else (G, lp)
