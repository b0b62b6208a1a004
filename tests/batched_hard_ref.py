"""Numpy restatements of the batched core (csrc/gsmvi_batched.hip: k_gsm_batched UPDATE / STEP / INIT, csrc/gsmvi_batched.h:
gb_chol_lds and gb_fit_tail, csrc/gsmvi_bam_batched.hip, csrc/gsmvi_kl_batched.hip) that carry ONE dtype through the whole
computation -- np.longdouble for the answer, np.float64 for the float64 noise floor of the same arithmetic --, the hard input
families the batched fits exist for, and the floor each kernel output is held to.  Test-only.

Restatements (no float64 LAPACK call inside a long double run): the GSM update in the reference's per-sample order
(``gsm_faithful``) and in the kernel's O(B D^2) algebra (``gsm_alg``), both returning (mu', S', mu' - mu0, S' - S0) with the
increments taken in long double from the results AS STORED in ``dtype`` (what a float64 kernel can deliver); the factor
(``chol_right``: the LDS-style right-looking elimination, ``chol_left``: the inner-product order); log q of points and of a
draw by forward substitution; the BaM update through V = L L^T, M = L^T U L, a cyclic Jacobi eigen-decomposition and
S' = L f(M) L^T, f(x) = 2 / (1 + sqrt(1 + 4 x)).  The verdict, the long double factor, the draws and the samples are those
of batched_step_ref.py.

Families (``FAMILIES``; one problem each in every batch, K = 11, and K = 15 with four of them repeated so that at D <= 16,
four problems per workgroup, the last workgroup has a tail slot): easy (batched_step_ref.states); S0 of spectrum condition
1e4, 1e8, 1e12 in a random orthogonal basis; S0 scaled by 1e-8 and 1e8 with samples and scores scaled consistently; graded
units S0 = G C G, G = diag(logspace(0, 6, D)); samples 100 sigma from the mean; scores 1e6 times steeper (a target 1e6
times narrower than q); nearly converged (samples from q, scores of the target q (1 + 1e-6)) at condition 100 and 1e8.

The floor of (case, output) is the larger rel_err (batched_step_ref.rel_err: long double, max-abs norm) of two float64 runs
against the long double run, never below 16 ulp (FLOOR_MIN = 3.6e-15: a float64 run can land on the rounded answer by luck).
GSM: the two operation orders.  Factor, samples, log q: the right-looking factor with forward sums and the left-looking
factor with reversed sums.  BaM: oracle.bam_oracle.bam_lowrank_update_exact and the same with the sample rows reversed.  The
floors come from the CPU restatements alone; no kernel output enters them.  The bar of tests/test_gpu_batched_hard.py is
kernel_err <= M x floor with M = 16: the kernel is a third summation order (sequential FMA loops of at most 64 terms) beside
the two the floor is taken from, so its error is one more draw from the same distribution, and the maximum over up to 4096
entries needs headroom; the 1000 x floor of psis_batched_ref.py covers tree sums of thousands of terms, which these are not.

CPU floors (tests/test_batched_hard_cpu.py::test_print_the_floor_table prints them; the largest over D in {5, 16, 17, 64} and
B in {2, 32}; R0, X0: factor and samples of the INIT state S0, R1, X1: of the accepted S'; logq: of 24 points, kllogq: of the
monitor's draw; "d" is the increment an update adds to its input; bam_*: the BaM update, bam_res its residual):

family           mu        S      dmu       dS       R0       R1       X0       X1     logq   kllogq   bam_mu    bam_S  bam_res
easy        3.6e-15  3.6e-15  3.6e-15  1.1e-14  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15
cond1e4     3.6e-15  3.6e-15  3.6e-15  6.1e-15  5.8e-15  6.3e-15  4.0e-15  4.2e-15  5.5e-15  2.1e-14  3.6e-15  3.6e-15  3.6e-15
cond1e8     3.6e-15  3.6e-15  3.6e-15  3.6e-15  1.4e-12  1.8e-12  8.1e-13  1.2e-12  7.4e-12  1.2e-10  1.1e-13  1.2e-13  1.9e-13
cond1e12    3.6e-15  3.6e-15  3.6e-15  3.6e-15  4.1e-11  3.9e-11  1.3e-11  2.2e-11  1.9e-07  3.8e-07  3.6e-15  3.6e-15  3.6e-15
scale1e-8   3.6e-15  2.4e-12  2.1e-11  1.3e-11  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  4.3e-14  9.8e-14
scale1e8    3.6e-15  3.6e-15  3.6e-15  4.3e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  4.0e-13  5.8e-13  1.6e-12
graded      3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  9.2e-15  3.6e-15  3.6e-15
far         3.6e-15  6.1e-12  3.4e-12  2.0e-10  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  7.3e-09  2.0e-10  5.5e-10
steep       3.6e-15  3.6e-15  3.6e-15  1.3e-14  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  4.3e-06  9.2e-07  4.3e-06
near_c100   3.6e-15  3.6e-15  1.4e-07  2.9e-08  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15  3.6e-15
near_c1e8   2.5e-12  8.3e-12  3.5e-04  1.3e-04  1.3e-12  1.1e-12  6.7e-13  3.6e-13  3.8e-12  5.3e-11  1.8e-11  2.0e-10  3.6e-15
(BaM: steep at B = 32 only -- at B = 2 float64 holds no digit of it, see bam_resolved; D = 64 keeps the families of BAM_D64.)
trajectory gsm D=10 B=2: mean 3.6e-15 6.1e-15 2.2e-13 4.0e-14 7.2e-13 1.1e-10 | cov 3.6e-15 8.9e-15 4.0e-13 3.6e-15 1.5e-14 3.8e-13
trajectory gsm D=33 B=4: mean 3.6e-15 3.6e-15 1.3e-14 4.0e-15 2.5e-14 3.3e-13 | cov 3.6e-15 3.6e-15 3.6e-15 3.6e-15 3.6e-15 3.4e-14
trajectory bam D=10 B=2: mean 4.8e-15 1.6e-14 1.0e-13 9.1e-15 1.5e-13 1.6e-13 | cov 8.3e-15 2.5e-14 2.0e-13 3.6e-15 5.2e-15 1.9e-14
The scale1e-8 floors of S and the increments come from the reference's own order (Sg - mu0 + x rounds at |mu0| before x takes
it back); the kernel's order, (S0 g - d), does not lose there.  All input conditions hold at every shape as generated: the
smallest pivot margin of an S' is 5.0e-12 (cond1e12 at D = 5, B = 2, against 1000 D eps = 1.1e-12), so no family's condition
had to be lowered.

Building every case with every long double reference (``build_all``) takes 8 to 11 s on the development machine's CPU, 4 s of
it the long double Jacobi of the D = 64 BaM cases (test_batched_hard_cpu.py asserts it stays under 20 s).

Planted float32 roundings in the float64 restatement (test_batched_hard_cpu.py::test_planted_float32_roundings_are_caught; the
largest err / floor, where, and whether the suite's fixed bars on the easy states -- 1e-12 on mu and S, 1e-11 on R and X, 1e-9
on log q -- would have caught it too):
  (a) rho            1.5e7 x floor (graded, mu: err 5.3e-8)            fixed bars: caught
  (b) S0 g_b         4.1e7 x floor (near_c100, S' - S0: err 0.11)      fixed bars: caught
  (c) e_b            2.1e8 x floor (far, S': err 6.9e-4)               fixed bars: caught
  (d) multipliers    1.6e8 x floor (cond1e8, R of S0: err 3.5e-5)      fixed bars: caught
A whole float32 rounding is coarse enough for either bar; what the fixed bars miss is a loss of three or four digits
(1e-13 to 1e-12 on an easy state), which the floor's 16 x 3.6e-15 = 5.7e-14 catches.

Kernel ratios kernel_err / floor measured on the MI355X, the largest over the shapes and outputs, per entry point and family
(update: gsm_update_batched; init, step: gsm_fit_init_batched, gsm_fit_step_batched; bam: bam_update_batched and
bam_fit_step_batched, which write the same bits; logq, kl_draw: logq_batched, kl_draw_batched):

family       update     init     step      bam     logq  kl_draw
easy           0.74     0.19     0.17     0.06    0.045     0.13
cond1e4        0.45      1.7      1.4     0.11      1.1      1.8
cond1e8        0.41      1.4      4.7     0.54      1.4        2
cond1e12        0.9      1.2      1.8    0.039     0.83      1.1
scale1e-8         1     0.11     0.12        1     0.07    0.079
scale1e8       0.57      0.2     0.16     0.46    0.073     0.24
graded         0.74     0.24      0.2     0.66     0.09     0.26
far               1     0.15     0.13     0.53    0.031     0.15
steep          0.64     0.17     0.16  flagged     0.03     0.12
near_c100         1     0.13     0.16    0.088     0.53     0.81
near_c1e8       2.3      1.6      1.5      2.5      1.6        2
Per output: update mu 2.3, S' 1.9, mean increment 2.3, S' - S0 1.9; init R 1.6, X 1.7; step R 4.6, X 4.7; bam mu 2.5, S' 1.9,
residual 1.0; logq 1.6; kl_draw X 2.0, log q 2.0; trajectories (50 forced iterations) GSM 1.8, BaM 1.0.
The largest ratio is 4.7 (the STEP's samples on cond1e8; gb_chol_lds scales both factors of an update by 1 / pivot, two
roundings where the restatement has one), so no family needs a margin above M = 16 and no kernel was changed.  BaM's steep
family is flagged at B = 32 (info = 1, NaN, the step reverts) and returned unflagged at B = 2: see bam_may_flag.
"""
import functools
import time

import numpy as np

import batched_step_ref as step
from oracle import bam_oracle as borc

LD = np.longdouble
F64 = np.float64
EPS = float(np.finfo(np.float64).eps)
FLOOR_MIN = 16 * EPS                                        # 3.6e-15
M_BAR = 16.0
D_GRID = (5, 16, 17, 64)                                    # both thread mappings, the odd-D padded draw row, the bound
B_GRID = (2, 32)
FAMILIES = ("easy", "cond1e4", "cond1e8", "cond1e12", "scale1e-8", "scale1e8", "graded", "far", "steep", "near_c100",
            "near_c1e8")
K = len(FAMILIES)                                           # 11
REPEATS = (2, 6, 7, 10)                                     # the problems of the K = 11 batch that slots 11 .. 14 repeat
K_TAIL = K + len(REPEATS)                                   # 15 = 3 workgroups of four + 3: a tail slot at D <= 16
SEEDS = (7, 2 ** 40 + 3, 12345, 2 ** 63 + 11, 2 ** 32, 99, 2 ** 64 - 1, 31337, 2 ** 33 + 5, 4242, 2 ** 50 + 1)
CALL = step.CALL
N_POINTS = 24                                               # rows of logq_batched and kl_draw_batched per problem
KL_CALL = 3
BAM_REGS = (0.3, 2.5, 100.0)
JITTER = 1e-6
BAM_D64 = ("easy", "cond1e8", "graded", "far", "near_c100", "near_c1e8")      # the long double Jacobi is the slow part
NS_BOUND = 1e21                                             # trace(N + I / 4) that the 32 Newton-Schulz steps still close
rel_err = step.rel_err


def pivot_margin(D):
    """every pivot examined is at least this fraction of its diagonal entry: rounding (a few D eps) cannot flip a verdict"""
    return 1000 * D * EPS


def _pi(dtype):
    return dtype(4) * np.arctan(dtype(1))


# ---- the GSM update ----------------------------------------------------------------------------------------------------------
def _with_increments(mu, S, mu0, S0):
    """(mu', S', mu' - mu0, S' - S0): the increments in long double, of the results as their dtype stores them"""
    return mu, S, np.asarray(mu, dtype=LD) - np.asarray(mu0, dtype=LD), np.asarray(S, dtype=LD) - np.asarray(S0, dtype=LD)


def gsm_faithful(X, V, mu0, S0, dtype=LD):
    """the reference's per-sample order (oracle.gsm_oracle.gsm_single_faithful / gsm_update_faithful) in ``dtype``"""
    X, V, m0, A0 = (np.asarray(a, dtype=dtype) for a in (X, V, mu0, S0))
    B, D = X.shape
    one, half, four = dtype(1), dtype(0.5), dtype(4)
    eye = np.eye(D, dtype=dtype)
    dmus, dSs = np.zeros((B, D), dtype=dtype), np.zeros((B, D, D), dtype=dtype)
    for b in range(B):
        x, g = X[b], V[b]
        d = m0 - x
        Sg = A0 @ g
        gSg = g @ Sg
        mv = d @ g
        rho = half * np.sqrt(one + four * (gSg + mv * mv)) - half
        eps0 = Sg - m0 + x
        den = one + rho + mv
        proj = eye - np.outer(d, g) / den
        dmus[b] = one / (one + rho) * (proj @ eps0)
        mu = m0 + dmus[b]
        dSs[b] = np.outer(d, d) - np.outer(mu - x, mu - x)
    return _with_increments(m0 + dmus.sum(0) / dtype(B), A0 + dSs.sum(0) / dtype(B), mu0, S0)


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(F64)


def gsm_alg(X, V, mu0, S0, dtype=LD, plant=None):
    """the O(B D^2) order of oracle.gsm_oracle.gsm_per_sample_terms -- the kernel's algebra -- in ``dtype``.  ``plant`` (float64
    runs only) rounds one value through float32: "rho", "Sg" (S0 g_b) or "e" (e_b)."""
    X, G, m0, A0 = (np.asarray(a, dtype=dtype) for a in (X, V, mu0, S0))
    B = X.shape[0]
    one, half, four = dtype(1), dtype(0.5), dtype(4)
    dvec = m0[None, :] - X
    SG = G @ A0.T
    if plant == "Sg":
        SG = _f32(SG)
    gSg = (G * SG).sum(1)
    mv = (dvec * G).sum(1)
    rho = half * np.sqrt(one + four * (gSg + mv * mv)) - half
    if plant == "rho":
        rho = _f32(rho)
    den = one + rho + mv
    dmu = ((SG - dvec) - dvec * ((gSg - mv) / den)[:, None]) / (one + rho)[:, None]
    evec = dvec + dmu
    if plant == "e":
        evec = _f32(evec)
    mu = m0 + dmu.sum(0) / dtype(B)
    S = A0 + (dvec.T @ dvec - evec.T @ evec) / dtype(B)
    return _with_increments(mu, S, mu0, S0)


# ---- the factor, the samples, log q --------------------------------------------------------------------------------------------
def chol_right(S, dtype=LD, plant=False):
    """upper factor by the right-looking elimination of gb_chol_lds in ``dtype``: row c is final after step c, the trailing
    block loses (S[c, i] / pivot) S[c, j]; ``plant`` rounds the multipliers S[c, i] / pivot through float32"""
    A = np.asarray(S, dtype=dtype).copy()
    D = A.shape[0]
    R = np.zeros((D, D), dtype=dtype)
    for c in range(D):
        p = A[c, c]
        mult = A[c, c + 1:] / p
        if plant:
            mult = _f32(mult)
        with np.errstate(invalid="ignore"):                  # a planted loss may turn a pivot negative: NaN, as on the device
            r = np.sqrt(p)
        R[c, c], R[c, c + 1:] = r, A[c, c + 1:] / r
        A[c + 1:, c + 1:] -= np.outer(mult, A[c, c + 1:])
    return R


def chol_left(S, dtype=LD):
    """the same factor in the inner-product order (row i of R from rows 0 .. i - 1), sums taken from the last term back"""
    A = np.asarray(S, dtype=dtype).copy()
    D = A.shape[0]
    R = np.zeros((D, D), dtype=dtype)
    for i in range(D):
        v = A[i, i:] - (R[:i, i][::-1, None] * R[:i, i:][::-1]).sum(0)
        R[i, i] = np.sqrt(v[0])
        R[i, i + 1:] = v[1:] / R[i, i]
    return R


def chol_ld(S, dtype=LD):
    """batched_step_ref.chol_ld with the signature of the factors here (long double only)"""
    assert dtype is LD
    return step.chol_ld(S)


def sample_in(mean, R, Z, dtype=LD, reverse=False):
    """mean + Z R in ``dtype``; ``reverse`` sums the products from the last row of R back"""
    m, R, Z = np.asarray(mean, dtype=dtype), np.asarray(R, dtype=dtype), np.asarray(Z, dtype=dtype)
    if reverse:
        return m[None, :] + Z[:, ::-1] @ R[::-1]
    return m[None, :] + Z @ R


def _whiten(R, Y, mean, dtype):
    """W with R^T w = y - mean for every row y, by forward substitution in ``dtype``"""
    T = np.asarray(Y, dtype=dtype) - np.asarray(mean, dtype=dtype)[None, :]
    D = R.shape[0]
    W = np.zeros_like(T)
    for c in range(D):
        W[:, c] = T[:, c] / R[c, c]
        T[:, c + 1:] -= W[:, c:c + 1] * R[c:c + 1, c + 1:]
    return W


def _logq_from(W, R, dtype):
    n, D = W.shape
    return -dtype(0.5) * (W * W).sum() - dtype(n) * np.log(np.diag(R)).sum() - dtype(0.5) * dtype(n * D) * np.log(dtype(2) * _pi(dtype))


def logq_points(mean, cov, Y, dtype=LD, factor=chol_right):
    """the sum over the rows y of Y of log N(y; mean, cov) (gsmvi_logq_batched_f64) in ``dtype``"""
    R = factor(cov, dtype)
    return _logq_from(_whiten(R, Y, mean, dtype), R, dtype)


def kl_rows(seed, call, n, D):
    """Z (n, D) of the monitor's draw: the plain layout of gsmvi_randn_f64 (no odd-D padding)"""
    from oracle import gsm_oracle as orc
    return orc.philox_randn(int(seed), int(call), n * D).reshape(n, D).copy()


def kl_draw(mean, cov, Z, dtype=LD, factor=chol_right, reverse=False):
    """(X, logq) of gsmvi_kl_draw_batched_f64: X = mean + Z R, logq = -|Z|^2 / 2 - n sum log R_ii - n D / 2 log 2 pi"""
    R = factor(cov, dtype)
    return sample_in(mean, R, Z, dtype, reverse), _logq_from(np.asarray(Z, dtype=dtype), R, dtype)


# ---- BaM ------------------------------------------------------------------------------------------------------------------------
def jacobi_eigh(A, dtype=LD, max_sweeps=40):
    """(w, W): A = W diag(w) W^T of the symmetric A by cyclic Jacobi rotations in ``dtype``"""
    A = np.array(A, dtype=dtype)
    A = (A + A.T) / dtype(2)
    n = A.shape[0]
    W = np.eye(n, dtype=dtype)
    tiny = dtype(np.finfo(dtype).eps)
    one = dtype(1)
    with np.errstate(all="ignore"):
        for _ in range(max_sweeps):
            off, nrm = np.sqrt(((A - np.diag(np.diag(A))) ** 2).sum()), np.sqrt((A * A).sum())
            if not off > tiny * nrm:
                break
            small = tiny * nrm / dtype(n * n)                # below the rounding of A itself: M's null space stays at rest
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = A[p, q]
                    if abs(apq) <= small or abs(apq) <= dtype(0.01) * tiny * np.sqrt(abs(A[p, p] * A[q, q])):
                        continue
                    theta = (A[q, q] - A[p, p]) / (dtype(2) * apq)
                    t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
                    c = one / np.sqrt(t * t + one)
                    s = t * c
                    rp, rq = A[p, :].copy(), A[q, :].copy()
                    A[p, :], A[q, :] = c * rp - s * rq, s * rp + c * rq
                    cp, cq = A[:, p].copy(), A[:, q].copy()
                    A[:, p], A[:, q] = c * cp - s * cq, s * cp + c * cq
                    A[p, q] = A[q, p] = dtype(0)
                    wp, wq = W[:, p].copy(), W[:, q].copy()
                    W[:, p], W[:, q] = c * wp - s * wq, s * wp + c * wq
    return np.diag(A).copy(), W


def _solve_lower(L, Bm):
    """L^-1 Bm by forward substitution in the dtype of L"""
    Bm = np.array(Bm, dtype=L.dtype)
    for c in range(L.shape[0]):
        Bm[c] = Bm[c] / L[c, c]
        Bm[c + 1:] -= np.outer(L[c + 1:, c], Bm[c])
    return Bm


def bam_uv(X, G, mu0, S0, reg, dtype=LD):
    """U, V of test_gpu_bam_batched._uv (bam.py:50-60) and the batch means, in ``dtype``"""
    X, G, m0, A0 = (np.asarray(a, dtype=dtype) for a in (X, G, mu0, S0))
    B = dtype(X.shape[0])
    reg = dtype(reg)
    xbar, gbar = X.sum(0) / B, G.sum(0) / B
    xd, gd = X - xbar, G - gbar
    r1 = reg / (dtype(1) + reg)
    U = reg * (gd.T @ gd) / B + r1 * np.outer(gbar, gbar)
    Vm = A0 + reg * (xd.T @ xd) / B + r1 * np.outer(m0 - xbar, m0 - xbar)
    return U, Vm, xbar, gbar


def bam_update(X, G, mu0, S0, reg, dtype=LD):
    """(mu', S') with S' = 2 V (I + (I + 4 U V)^(1/2))^-1 = L f(M) L^T, V = L L^T, M = L^T U L, and the mean from its
    definition (bam.py:67), in ``dtype``"""
    U, Vm, xbar, gbar = bam_uv(X, G, mu0, S0, reg, dtype)
    L = step.chol_ld(Vm).astype(dtype).T if dtype is LD else chol_right(Vm, dtype).T
    w, W = jacobi_eigh(L.T @ U @ L, dtype)
    w = np.maximum(w, dtype(0))                              # M is positive semidefinite: a negative eigenvalue is round-off
    f = dtype(2) / (dtype(1) + np.sqrt(dtype(1) + dtype(4) * w))
    LW = L @ W
    S = (LW * f[None, :]) @ LW.T
    S = (S + S.T) / dtype(2)
    # one Newton step on S U S + S = V in the eigenbasis: S + E with E = L W Eh W^T L^T solves it to first order when
    # Eh_ij (1 + f_i w_i + w_j f_j) = (W^T L^-1 (V - S - S U S) L^-T W)_ij; it takes out what the rotations accumulated
    T = _solve_lower(L, Vm - S - S @ U @ S)
    T = W.T @ _solve_lower(L, T.T).T @ W
    g = w * f
    S = S + LW @ (T / (dtype(1) + g[:, None] + g[None, :])) @ LW.T
    S = (S + S.T) / dtype(2)
    reg = dtype(reg)
    mu = np.asarray(mu0, dtype=dtype) / (dtype(1) + reg) + reg / (dtype(1) + reg) * (S @ gbar + xbar)
    return mu, S


def bam_residual(S, X, G, mu0, S0, reg):
    """the backward error of test_gpu_bam_batched._backward_error, |S U S + S - V| / (|S|^2 |U| + |S| + |V|) in 2-norms, with
    the residual and U, V formed in long double (the norms themselves need one digit: float64 SVDs of the long double arrays)"""
    U, Vm, _, _ = bam_uv(X, G, mu0, S0, reg, LD)
    S = np.asarray(S, dtype=LD)
    n2 = lambda A: float(np.linalg.norm(np.asarray(A, dtype=F64), 2))       # noqa: E731
    res = S @ U @ S + S - Vm
    scale = float(np.max(np.abs(res))) or 1.0                # the residual is far below float64's range of V: scale it first
    return n2(res / LD(scale)) * scale / (n2(S) ** 2 * n2(U) + n2(S) + n2(Vm))


def bam_oracle(X, G, mu0, S0, reg, jitter=JITTER, reverse=False):
    """the float64 side: oracle.bam_oracle.bam_lowrank_update_exact, symmetrised, + jitter I; ``reverse``: the sample rows in
    the opposite order (the same update: every statistic is a sum over the rows)"""
    if reverse:
        X, G = X[::-1], G[::-1]
    try:
        with np.errstate(all="ignore"):
            mu, S = borc.bam_lowrank_update_exact(np.ascontiguousarray(X), np.ascontiguousarray(G), mu0, S0, float(reg))
    except (ValueError, np.linalg.LinAlgError):                # the float64 chain cannot run: no float64 answer at all
        return np.full_like(mu0, np.nan), np.full_like(S0, np.nan)
    return mu, 0.5 * (S + S.T) + jitter * np.eye(S.shape[0])


# ---- the input families ---------------------------------------------------------------------------------------------------------
def _basis(rs, D):
    Q, _ = np.linalg.qr(rs.standard_normal((D, D)))
    return Q


def _from_factor(F):
    """S0 = F F^T formed in long double and rounded once (symmetric)"""
    F = np.asarray(F, dtype=LD)
    S = F @ F.T
    return np.asarray((S + S.T) / LD(2), dtype=F64)


def fam_easy(B, D, rs):
    X, V, mu0, S0 = step.states(1, B, D, int(rs.randint(2 ** 31)))
    return X[0], V[0], mu0[0], S0[0]


def fam_cond(B, D, rs, cond):
    """eigenvalues logspace(0, -log10 cond) in a random orthogonal basis; samples one standard deviation from the mean (drawn
    from q), the easy family's unscaled target (scores -(x - t) / 2)"""
    F = _basis(rs, D) * np.sqrt(np.logspace(0.0, -np.log10(cond), D))[None, :]
    mu0 = rs.standard_normal(D)
    X = mu0[None, :] + rs.standard_normal((B, D)) @ F.T
    return X, -0.5 * (X - rs.standard_normal((1, D))), mu0, _from_factor(F)


def fam_scale(B, D, rs, s):
    """the easy state in other units: S0 s, the samples' offsets sqrt(s), the scores 1 / sqrt(s)"""
    X, V, mu0, S0 = fam_easy(B, D, rs)
    r = np.sqrt(s)
    return mu0[None, :] + r * (X - mu0[None, :]), V / r, mu0, S0 * s


def fam_graded(B, D, rs):
    """graded units: S0 = G C G, G = diag(logspace(0, 6, D)), the samples' offsets times G, the scores G^-1"""
    X, V, mu0, S0 = fam_easy(B, D, rs)
    g = np.logspace(0.0, 6.0, D)
    S = S0 * g[:, None] * g[None, :]
    return mu0[None, :] + (X - mu0[None, :]) * g[None, :], V / g[None, :], mu0, 0.5 * (S + S.T)


def fam_far(B, D, rs):
    """samples 100 standard deviations from the mean"""
    X, V, mu0, S0 = fam_easy(B, D, rs)
    L = np.linalg.cholesky(S0)
    X = mu0[None, :] + 100.0 * rs.standard_normal((B, D)) @ L.T
    return X, -0.5 * (X - rs.standard_normal((1, D))), mu0, S0


def fam_steep(B, D, rs):
    """a target 1e6 times narrower than q: the easy state with its scores times 1e6"""
    X, V, mu0, S0 = fam_easy(B, D, rs)
    return X, 1e6 * V, mu0, S0


def fam_near(B, D, rs, cond):
    """nearly converged: samples x = mu0 + F z drawn from q = N(mu0, F F^T), scores -(F F^T)^-1 (x - mu0) / (1 + 1e-6) of the
    target q (1 + 1e-6), formed without an inverse: (F F^T)^-1 F z = Q w^(-1/2) z for F = Q w^(1/2)"""
    Q = _basis(rs, D)
    w = np.logspace(0.0, -np.log10(cond), D)
    F = np.asarray(Q, dtype=LD) * np.sqrt(np.asarray(w, dtype=LD))[None, :]
    mu0 = rs.standard_normal(D)
    Z = np.asarray(rs.standard_normal((B, D)), dtype=LD)
    X = np.asarray(np.asarray(mu0, dtype=LD)[None, :] + Z @ F.T, dtype=F64)
    V = -(Z / np.sqrt(np.asarray(w, dtype=LD))[None, :]) @ np.asarray(Q, dtype=LD).T / LD(1 + 1e-6)
    return X, np.asarray(V, dtype=F64), mu0, _from_factor(F)


GENERATORS = {
    "easy": fam_easy,
    "cond1e4": functools.partial(fam_cond, cond=1e4),
    "cond1e8": functools.partial(fam_cond, cond=1e8),
    "cond1e12": functools.partial(fam_cond, cond=1e12),
    "scale1e-8": functools.partial(fam_scale, s=1e-8),
    "scale1e8": functools.partial(fam_scale, s=1e8),
    "graded": fam_graded,
    "far": fam_far,
    "steep": fam_steep,
    "near_c100": functools.partial(fam_near, cond=1e2),
    "near_c1e8": functools.partial(fam_near, cond=1e8),
}


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def batch(D, B):
    """the K = 11 heterogeneous batch at (D, B): X, V (K, B, D), mu0 (K, D), S0 (K, D, D), one family per problem in the order
    of FAMILIES, and Y (K, N_POINTS, D): points one standard deviation from the mean for logq_batched.  Read-only, shared."""
    out = {n: [] for n in ("X", "V", "mu0", "S0", "Y")}
    for n, fam in enumerate(FAMILIES):
        rs = np.random.RandomState(100000 + 1000 * D + 10 * B + n)
        X, V, mu0, S0 = GENERATORS[fam](B, D, rs)
        Y = np.asarray(step.sample(mu0, step.chol_ld(S0), rs.standard_normal((N_POINTS, D))), dtype=F64)
        for name, a in zip(("X", "V", "mu0", "S0", "Y"), (X, V, mu0, S0, Y)):
            out[name].append(np.ascontiguousarray(a, dtype=F64))
    return _frozen({n: np.stack(v) for n, v in out.items()})


def floor_of(runs, want):
    """the larger rel_err of the float64 ``runs`` against the long double ``want``, at least FLOOR_MIN"""
    worst = max(rel_err(r, want) if np.isfinite(np.asarray(r, dtype=F64)).all() else np.inf for r in runs)
    return max(FLOOR_MIN, worst)


# ---- the references of every case -------------------------------------------------------------------------------------------------
def _tail_refs(mean, S, Zfit, Zkl, Y):
    """long double R, X of the fit tail, (X, logq) of the monitor's draw and logq of the points Y, for the state (mean, S), and
    their floors"""
    Rl = step.chol_ld(S)
    f_runs = [(chol_right(S, F64), False), (chol_left(S, F64), True)]
    want = dict(R=Rl, X=step.sample(mean, Rl, Zfit))
    floors = dict(R=floor_of([r for r, _ in f_runs], Rl),
                  X=floor_of([sample_in(mean, r, Zfit, F64, rev) for r, rev in f_runs], want["X"]))
    if Zkl is not None:
        want["klX"], want["kllogq"] = kl_draw(mean, S, Zkl, LD, chol_ld)
        runs = [kl_draw(mean, S, Zkl, F64, chol_right, False), kl_draw(mean, S, Zkl, F64, chol_left, True)]
        floors["klX"] = floor_of([r[0] for r in runs], want["klX"])
        floors["kllogq"] = floor_of([r[1] for r in runs], want["kllogq"])
        want["logq"] = logq_points(mean, S, Y, LD, chol_ld)
        floors["logq"] = floor_of([logq_points(mean, S, Y, F64, chol_right), logq_points(mean, S, Y, F64, chol_left)],
                                  want["logq"])
    return want, floors


@functools.lru_cache(maxsize=None)
def gsm_case(D, B):
    """per problem k of batch(D, B): ``want[k]`` = the long double mu, S, dmu, dS of the update, info and margin of the
    verdicts of S0 and S', and the fit tails of INIT (state mu0, S0: R0, X0, logq, klX, kllogq) and STEP (the accepted
    state: R1, X1); ``floor[k]`` = the floor of each of those outputs"""
    b = batch(D, B)
    wants, floors = [], []
    for k in range(K):
        X, V, mu0, S0 = (b[n][k] for n in ("X", "V", "mu0", "S0"))
        ld = gsm_faithful(X, V, mu0, S0, LD)
        runs = [gsm_faithful(X, V, mu0, S0, F64), gsm_alg(X, V, mu0, S0, F64)]
        w = dict(zip(("mu", "S", "dmu", "dS"), ld))
        f = {n: floor_of([r[i] for r in runs], ld[i]) for i, n in enumerate(("mu", "S", "dmu", "dS"))}
        S1 = np.asarray(ld[1], dtype=F64)
        S1 = 0.5 * (S1 + S1.T)
        mu1 = np.asarray(ld[0], dtype=F64)
        for tag, S in (("0", S0), ("1", S1)):
            info, piv = step.verdict(S)
            w["info" + tag], w["margin" + tag] = info, step.margin(S, piv)
        w0, f0 = _tail_refs(mu0, S0, step.draw(SEEDS[k], 0, B, D), kl_rows(SEEDS[k], KL_CALL, N_POINTS, D), b["Y"][k])
        w1, f1 = _tail_refs(mu1, S1, step.draw(SEEDS[k], CALL, B, D), None, None)
        for src_w, src_f, tag in ((w0, f0, "0"), (w1, f1, "1")):
            for n in ("R", "X"):
                w[n + tag], f[n + tag] = src_w[n], src_f[n]
        for n in ("klX", "kllogq", "logq"):
            w[n], f[n] = w0[n], f0[n]
        wants.append(w)
        floors.append(f)
    return wants, floors


def bam_families(D):
    return BAM_D64 if D == 64 else FAMILIES


def bam_resolved(floor):
    """False where float64 itself holds no digit of the answer: the low-rank form S' = V - A BB^-1 A^T cancels completely when
    U is huge and B + 1 < D (the steep family at B = 2: oracle errors of 1e2 and above, or a singular BB).  Such a case has no
    float64 answer to hold a float64 kernel to; the GPU test asks of it only what it asks of a flagged problem."""
    return floor["S"] < 1e-2 and floor["mu"] < 1e-2


def bam_may_flag(ns):
    """True where the kernel's float64 chain may legitimately fail: BB = N + I / 2 + (N + I / 4)^(1/2) is factored by a
    Cholesky, and once trace(N + I / 4) reaches 1 / (4 eps) = 1.1e15 the I / 2 that keeps BB positive definite is below the
    rounding of N's own entries (N has rank <= D, so for B + 1 > D only that I / 2 holds its null space up).  Such a problem
    may come back flagged (info = 1, NaN; a STEP reverts it) -- the path of
    test_gpu_bam_batched.py::test_unconverged_square_root_fails_its_problem_alone -- although its Newton-Schulz bound
    (NS_BOUND) still closes.  Of the families only steep is there (trace 1e16 to 2e17); measured on the MI355X it is flagged at
    B = 32 and returned at B = 2, where float64 holds no digit of it (bam_resolved)."""
    return 4.0 * ns >= 1.0 / EPS


def bam_reg(k):
    return BAM_REGS[k % len(BAM_REGS)]


@functools.lru_cache(maxsize=None)
def bam_case(D, B):
    """per problem k of batch(D, B) that BaM keeps at this D (bam_families; None for the others): ``want[k]`` = the long double
    mu and S (= S' + JITTER I), its own residual ``res``, trace(N + I / 4) ``ns``, info and margin of the verdict of S;
    ``floor[k]`` = the floors of mu and S and ``res``: the larger residual of the two float64 oracle runs' S - JITTER I"""
    b = batch(D, B)
    wants, floors = [None] * K, [None] * K
    for k, fam in enumerate(FAMILIES):
        if fam not in bam_families(D):
            continue
        X, V, mu0, S0 = (b[n][k] for n in ("X", "V", "mu0", "S0"))
        reg = bam_reg(k)
        mu, S = bam_update(X, V, mu0, S0, reg, LD)
        eye = np.eye(D, dtype=LD)
        U, Vm, _, _ = bam_uv(X, V, mu0, S0, reg, LD)
        w = dict(mu=mu, S=S + LD(JITTER) * eye, res=bam_residual(S, X, V, mu0, S0, reg),
                 ns=float(np.trace(U @ Vm)) + 0.25 * (B + 1))
        S1 = np.asarray(w["S"], dtype=F64)
        info, piv = step.verdict(0.5 * (S1 + S1.T))
        w["info"], w["margin"] = info, step.margin(S1, piv)
        runs = [bam_oracle(X, V, mu0, S0, reg), bam_oracle(X, V, mu0, S0, reg, reverse=True)]
        f = dict(mu=floor_of([r[0] for r in runs], mu), S=floor_of([r[1] for r in runs], w["S"]),
                 res=max(FLOOR_MIN, max(bam_residual(np.asarray(r[1], dtype=LD) - LD(JITTER) * eye, X, V, mu0, S0, reg)
                                        if np.isfinite(r[1]).all() else np.inf for r in runs)))
        wants[k], floors[k] = w, f
    return wants, floors


# ---- the teacher-forced trajectories ----------------------------------------------------------------------------------------------
TRAJ_SHAPES = ((10, 2), (33, 4))
TRAJ_NITER = 50
TRAJ_K = 6
TRAJ_REG0 = (100.0, 30.0, 10.0, 3.0, 1.0, 0.5)


@functools.lru_cache(maxsize=None)
def traj_inputs(D, B):
    """K = 6 Gaussian targets, covariance condition {10, 1e4, 1e6} x graded units {no, 1e3}; forced samples around the target's
    mean, one target standard deviation away (so every update is an accepted one), and their float64 scores: (forced
    (niter + 1, K, B, D), scores of the same shape, means, precisions)"""
    ms, Ps = np.zeros((TRAJ_K, D)), np.zeros((TRAJ_K, D, D))
    forced = np.zeros((TRAJ_NITER + 1, TRAJ_K, B, D))
    G = np.zeros_like(forced)
    for k in range(TRAJ_K):
        rs = np.random.RandomState(7000 + 100 * D + k)
        cond, graded = (10.0, 1e4, 1e6)[k % 3], k >= 3
        Q = np.asarray(_basis(rs, D), dtype=LD)
        w = np.asarray(np.logspace(0.0, -np.log10(cond), D), dtype=LD)
        g = np.asarray(np.logspace(0.0, 3.0, D) if graded else np.ones(D), dtype=LD)
        F = g[:, None] * Q * np.sqrt(w)[None, :]                             # the target's covariance is F F^T
        P = (Q / w[None, :]) @ Q.T / g[:, None] / g[None, :]
        ms[k] = rs.random_sample(D)
        Ps[k] = np.asarray((P + P.T) / LD(2), dtype=F64)
        Z = rs.standard_normal((TRAJ_NITER + 1, B, D))
        forced[:, k] = np.asarray(np.asarray(ms[k], dtype=LD)[None, None, :] + np.asarray(Z, dtype=LD) @ F.T, dtype=F64)
        G[:, k] = -(forced[:, k] - ms[k][None, None, :]) @ Ps[k].T
    return _frozen(dict(forced=forced, G=G, ms=ms, Ps=Ps))


def traj_regs(i):
    return np.array(TRAJ_REG0) / (1.0 + i)


def run_loop(update, forced, G, D):
    """the fit loop on forced samples for one problem from mean 0, cov I: ``update(X, V, mean, cov, i)`` -> (mean', cov');
    accept when step.verdict finds every pivot good; returns (mean, cov, reverts)"""
    dt = update.dtype
    mean, cov, reverts = np.zeros(D, dtype=dt), np.eye(D, dtype=dt), 0
    for i in range(forced.shape[0]):
        m1, S1 = update(forced[i], G[i], mean, cov, i)
        with np.errstate(all="ignore"):
            ok = step.verdict(S1)[0] == 0
        if ok:
            mean, cov = m1, S1
        else:
            reverts += 1
    return mean, cov, reverts


def _gsm_stepper(fn, dtype):
    def update(X, V, mean, cov, i):
        X, V = np.asarray(X, dtype=dtype), np.asarray(V, dtype=dtype)
        B = dtype(X.shape[0])
        one, half, four = dtype(1), dtype(0.5), dtype(4)
        if fn == "alg":
            dvec = mean[None, :] - X
            SG = V @ cov.T
            gSg, mv = (V * SG).sum(1), (dvec * V).sum(1)
            rho = half * np.sqrt(one + four * (gSg + mv * mv)) - half
            dmu = ((SG - dvec) - dvec * ((gSg - mv) / (one + rho + mv))[:, None]) / (one + rho)[:, None]
            evec = dvec + dmu
            return mean + dmu.sum(0) / B, cov + (dvec.T @ dvec - evec.T @ evec) / B
        dmus, dS = np.zeros_like(X), np.zeros_like(cov)
        eye = np.eye(X.shape[1], dtype=dtype)
        for b in range(X.shape[0]):
            x, g = X[b], V[b]
            d = mean - x
            Sg = cov @ g
            gSg, mv = g @ Sg, d @ g
            rho = half * np.sqrt(one + four * (gSg + mv * mv)) - half
            dmus[b] = one / (one + rho) * ((eye - np.outer(d, g) / (one + rho + mv)) @ (Sg - mean + x))
            mu = mean + dmus[b]
            dS = dS + (np.outer(d, d) - np.outer(mu - x, mu - x))
        return mean + dmus.sum(0) / B, cov + dS / B
    update.dtype = dtype
    return update


def _bam_stepper(kind, k):
    def update(X, V, mean, cov, i):
        reg = traj_regs(i)[k]
        if kind == "ld":
            mu, S = bam_update(np.asarray(X), np.asarray(V), mean, cov, reg, LD)      # the state itself stays long double
            return mu, S + LD(JITTER) * np.eye(S.shape[0], dtype=LD)
        return bam_oracle(X, V, mean, cov, reg, JITTER, reverse=kind == "reversed")
    update.dtype = LD if kind == "ld" else F64
    return update


@functools.lru_cache(maxsize=None)
def traj_case(method, D, B):
    """per problem: the long double loop's (mean, cov, reverts), the reverts of the two float64 loops, and the floors of the
    final mean and cov: float64 loop against long double loop, both float64 orders"""
    t = traj_inputs(D, B)
    out = []
    for k in range(TRAJ_K):
        forced, G = t["forced"][:, k], t["G"][:, k]
        if method == "gsm":
            steppers = [_gsm_stepper("faithful", LD), _gsm_stepper("faithful", F64), _gsm_stepper("alg", F64)]
        else:
            steppers = [_bam_stepper("ld", k), _bam_stepper("oracle", k), _bam_stepper("reversed", k)]
        (m, c, rev), *runs = [run_loop(s, forced, G, D) for s in steppers]
        out.append(dict(mean=m, cov=c, reverts=rev, reverts64=[r[2] for r in runs],
                        floor_mean=floor_of([r[0] for r in runs], m), floor_cov=floor_of([r[1] for r in runs], c)))
    return out


def build_all():
    """every case with every long double reference; returns the seconds it took (from a cold cache)"""
    t0 = time.perf_counter()
    for D in D_GRID:
        for B in B_GRID:
            gsm_case(D, B)
            bam_case(D, B)
    for D, B in TRAJ_SHAPES:
        traj_case("gsm", D, B)
    traj_case("bam", *TRAJ_SHAPES[0])
    return time.perf_counter() - t0
