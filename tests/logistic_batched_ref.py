"""Numpy restatement of the batched logistic target (csrc/gsmvi_logistic_batched.hip) and the generator of its test inputs.
Test-only.  For problem k with design matrix A_k (N, D), labels y_k in [0, 1], n_k valid rows and prior precision lam_k:

    eta = A_k[:n_k] x,   lp_k(x) = sum_n [ y_n eta_n - softplus(eta_n) ] - lam_k |x|^2 / 2,
    grad lp_k(x) = sum_n ( y_n - sigmoid(eta_n) ) a_n - lam_k x

in the overflow-safe forms e = exp(-|eta|), sigmoid = 1 / (1 + e) for eta >= 0 and e / (1 + e) otherwise, softplus =
max(eta, 0) + log1p(e).  It is pinned to torch autograd of the written density in tests/test_logistic_batched_cpu.py."""
import numpy as np


def sigmoid_softplus(eta):
    e = np.exp(-np.abs(eta))
    sig = np.where(eta >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))
    return sig, np.maximum(eta, 0.0) + np.log1p(e)


def score_and_lp(A, y, counts, lam, X):
    """A (K, N, D), y (K, N), counts (K,) or None, lam a number or (K,), X (K, rows, D) -> G (K, rows, D), lp (K, rows): the loop
    of glm_batched_ref.score_and_lp for the logistic family without an offset (imported here: that module imports this one).
    A row of X with a non-finite entry gets NaN outputs, as the kernel gives it."""
    from glm_batched_ref import score_and_lp as glm_score_and_lp
    return glm_score_and_lp("logistic", A, y, None, counts, lam, 1.0, X)


def make_inputs(K, N, D, rows, scale=1.0, soft=False, seed=None):
    """The inputs of the tests: RandomState(N + D) (or ``seed``); A = scale N(0, 1) / sqrt(D), theta* ~ N(0, 1), y ~
    Bernoulli(sigmoid(A theta*)) (``soft``: y ~ U(0, 1)), counts = N for problem 0 and max(1, N - 1 - 3 k) after it, lam = 0 for
    problem 0 and 0.1 + U(0, 1) after it, X = scale N(0, 1).  Returns A, y, counts (int32), lam, X."""
    rs = np.random.RandomState(N + D if seed is None else seed)
    A = scale * rs.standard_normal((K, N, D)) / np.sqrt(D)
    theta = rs.standard_normal((K, D))
    p, _ = sigmoid_softplus(np.einsum("knd,kd->kn", A, theta))
    u = rs.random_sample((K, N))
    y = u if soft else (u < p).astype(np.float64)
    counts = np.array([N if k == 0 else max(1, N - 1 - 3 * k) for k in range(K)], dtype=np.int32)
    lam = 0.1 + rs.random_sample(K)
    lam[0] = 0.0
    X = scale * rs.standard_normal((K, rows, D))
    return A, y, counts, lam, X


def newton_map(A, y, lam, n=None, iters=50):
    """MAP of one problem by Newton's method (lam > 0 or separable-free data): the examples' yardstick"""
    A, y = np.asarray(A, dtype=np.float64)[:n], np.asarray(y, dtype=np.float64)[:n]
    x = np.zeros(A.shape[1])
    for _ in range(iters):
        sig, _ = sigmoid_softplus(A @ x)
        g = A.T @ (y - sig) - lam * x
        H = (A * (sig * (1.0 - sig))[:, None]).T @ A + lam * np.eye(A.shape[1])
        step = np.linalg.solve(H, g)
        x = x + step
        if np.abs(step).max() < 1e-13:
            break
    return x
