"""Numpy restatement of one launch of the batched fit tail (csrc/gsmvi_batched.h: gb_fit_tail, gb_chol_lds), per problem: the
new state (S', mu') of a STEP from the oracles, the verdict of a plain right-looking elimination in long double (0, or 1 + the
first pivot that is not > 0 and finite), the upper Cholesky factor in long double, and the draw X = mean + Z R with Z the
problem's Philox stream in the fits' layout.  ``mixed_batch`` builds the K = 7 batch of accepting and planted-to-fail problems
that tests/test_batched_step_cpu.py checks on the CPU and tests/test_gpu_batched_step.py launches.  Test-only."""
import functools

import numpy as np

from oracle import gsm_oracle as orc
from oracle import bam_oracle as borc

LD = np.longdouble
D_GRID = (1, 2, 5, 7, 10, 16, 17, 31, 32, 33, 63, 64)      # the suite's list: every NT, every slice of entries per thread
B_GRID = (1, 2, 32)
BAM_EXTRA = ((16, 22), (16, 23))                            # four | one problems per workgroup at D = 16 (bb_nt)
K = 7                                                       # 4 + 3: a second workgroup with a tail slot when four share one
PLANTED = (1, 3, 4)                                         # slots 1, 3 beside accepting 0, 2; slot 4 opens the next workgroup
NAN_SLOT = 2                                                # the accepting problem that takes one NaN score entry
SEEDS = (7, 2 ** 40 + 3, 12345, 2 ** 63 + 11, 2 ** 32, 99, 2 ** 64 - 1)      # both halves of the key reach Philox
CALL = 5 + 2 ** 33                                          # both halves of the draw number
BAM_REGS = (0.3, 1.0, 7.5, 100.0, 2.5, 2.5, 2.5)
JITTER = 1e-6
MARGIN = 0.05           # every pivot examined is at least this fraction of its diagonal entry away from zero
SHRINK = 1e-3           # a planted problem's samples and scores, around mu0: the update's O(1) term would heal the plant
SHIFT = 0.05            # ... and its samples' common offset from mu0: moves the new mean by O(SHIFT), S' by O(SHIFT^2)


def states(K, B, D, seed):
    """the suite's random one-shot inputs (test_gpu_batched.py::_states): S0 = A A^T / D + 0.1 I, samples around mu0"""
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((K, D, D))
    S0 = A @ np.swapaxes(A, 1, 2) / D + 0.1 * np.eye(D)
    S0 = 0.5 * (S0 + np.swapaxes(S0, 1, 2))
    mu0 = rs.standard_normal((K, D))
    X = mu0[:, None, :] + rs.standard_normal((K, B, D))
    V = -0.5 * (X - rs.standard_normal((K, 1, D)))
    return X, V, mu0, S0


def verdict(S):
    """(info, pivots): right-looking elimination of the upper triangle of S in long double, one pivot per step; info = 0, or
    1 + the first pivot that is not > 0 and finite; pivots = the pivots examined (all D when info = 0)"""
    A = np.array(S, dtype=LD)
    D = A.shape[0]
    piv = []
    for c in range(D):
        p = A[c, c]
        piv.append(p)
        if not (p > 0 and np.isfinite(p)):
            return c + 1, np.array(piv, dtype=LD)
        r = A[c, c + 1:]
        A[c + 1:, c + 1:] -= np.outer(r, r) / p
    return 0, np.array(piv, dtype=LD)


def chol_ld(S, rows=None):
    """upper Cholesky factor R (R^T R = S) in long double; ``rows``: only the first ``rows`` rows, the others zero (what the
    elimination has finished when pivot ``rows`` fails)"""
    A = np.array(S, dtype=LD)
    D = A.shape[0]
    R = np.zeros((D, D), dtype=LD)
    for c in range(D if rows is None else rows):
        p = np.sqrt(A[c, c])
        R[c, c:] = A[c, c:] / p
        R[c, c] = p
        A[c + 1:, c + 1:] -= np.outer(R[c, c + 1:], R[c, c + 1:])
    return R


def draw(seed, call, B, D):
    """Z (B, D) of draw ``call`` of key ``seed``: B x Dz normals, Dz = D rounded up to even, column D dropped"""
    Dz = D + (D & 1)
    return orc.philox_randn(int(seed), int(call), B * Dz).reshape(B, Dz)[:, :D].copy()


def update(method, X, V, mu0, S0, reg=None, jitter=0.0):
    """(mu', S') of one problem: GSM = gsm_update_faithful; BaM = bam_lowrank_update_exact, symmetrised, + jitter I.  A chain
    that cannot run (non-finite input) is the device's poisoned result: all NaN."""
    with np.errstate(all="ignore"):
        if method == "gsm":
            return orc.gsm_update_faithful(X, V, mu0, S0)
        try:
            mu, S = borc.bam_lowrank_update_exact(X, V, mu0, S0, reg)
        except (ValueError, np.linalg.LinAlgError):
            return np.full_like(mu0, np.nan), np.full_like(S0, np.nan)
        return mu, 0.5 * (S + S.T) + jitter * np.eye(S.shape[0])


def sample(mean, R, Z):
    return np.asarray(mean, dtype=LD)[None, :] + np.asarray(Z, dtype=LD) @ np.asarray(R, dtype=LD)


def step_problem(method, X, V, mean, cov, R, n_rev, seed=None, call=0, reg=None, jitter=0.0):
    """one STEP launch for one problem, nothing in place: dict(info, mean, cov, R, n_rev, X); on a revert mean, cov and R are
    the arrays given; R and X are long double (X is None without a seed)"""
    mu1, S1 = update(method, X, V, mean, cov, reg, jitter)
    info, _ = verdict(S1)
    if info == 0:
        out = dict(info=0, mean=mu1, cov=S1, R=chol_ld(S1) if R is not None else None, n_rev=n_rev)
    else:
        out = dict(info=info, mean=mean, cov=cov, R=R, n_rev=n_rev + 1)
    out["X"] = sample(out["mean"], out["R"], draw(seed, call, X.shape[0], X.shape[1])) if seed is not None else None
    return out


def init_problem(mean, cov, seed=None, B=1):
    """one INIT launch for one problem: dict(info, R, X): R (long double) is meaningful only for info = 0; draw 0 of the key"""
    info, _ = verdict(cov)
    R = chol_ld(cov) if info == 0 else None
    X = sample(mean, R, draw(seed, 0, B, mean.shape[0])) if seed is not None and info == 0 else None
    return dict(info=info, R=R, X=X)


def plant(S, c):
    """S with pivot c of its elimination turned into its negative (pivots before c unchanged)"""
    info, piv = verdict(S)
    assert info == 0
    S = np.array(S, copy=True)
    S[c, c] -= 2.0 * float(piv[c])
    return S


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def mixed_batch(method, D, B, nan_case=False):
    """The K = 7 batch of a STEP launch at (D, B), computed once and shared (its arrays are read-only): problems PLANTED fail
    at pivot c = (5 k) % D -- that pivot of S0[k] turned negative, samples and scores shrunk by SHRINK around mu0[k] so that the
    update's positive-semidefinite term cannot heal it, the samples then moved by SHIFT so that the new mean is still far from
    the kept one (shrunk samples alone move it by less than 1e-4 of the samples at B = 32) -- and the others accept;
    ``nan_case``: accepting problem NAN_SLOT gets one NaN score entry.  Besides the inputs: R_kept (the factor of an unrelated positive-definite matrix per problem), n_rev0 =
    3 + k, seeds, regs (BaM), and the reference's results: S1, mu1, codes (the expected info), pivots."""
    X, V, mu0, S0 = states(K, B, D, 100 * D + B)
    for k in PLANTED:
        S0[k] = plant(S0[k], (5 * k) % D)
        X[k] = mu0[k] + SHRINK * (X[k] - mu0[k]) + SHIFT
        V[k] *= SHRINK
    if nan_case:
        V[NAN_SLOT, B - 1, D // 2] = np.nan
    S_other = states(K, 1, D, 100 * D + B + 50000)[3]
    R_kept = np.stack([np.linalg.cholesky(S_other[k]).T for k in range(K)])
    regs = np.array(BAM_REGS) if method == "bam" else None
    mu1, S1, codes, pivots = np.empty((K, D)), np.empty((K, D, D)), [], []
    for k in range(K):
        mu1[k], S1[k] = update(method, X[k], V[k], mu0[k], S0[k], None if regs is None else regs[k], JITTER)
        info, piv = verdict(S1[k])
        codes.append(info)
        pivots.append(piv)
    return _frozen(dict(X=X, V=V, mu0=mu0, S0=S0, R_kept=R_kept, n_rev0=3 + np.arange(K), seeds=SEEDS, regs=regs, mu1=mu1, S1=S1,
                        codes=np.array(codes), pivots=pivots, reverting=[k for k in range(K) if codes[k] != 0]))


def expected_codes(D, nan_case=False):
    return np.array([(5 * k) % D + 1 if k in PLANTED else (1 if nan_case and k == NAN_SLOT else 0) for k in range(K)])


def margin(S, pivots):
    """the smallest |pivot| / |S_ii| over the pivots examined"""
    d = np.abs(np.diag(np.asarray(S, dtype=LD))[:len(pivots)])
    return float(np.min(np.abs(pivots) / d))


def sources(mb, k, B, D, call=CALL):
    """for reverting problem k of a mixed batch: the samples of the right source (the kept mean and factor, draw ``call``) and of
    the wrong ones a faulty tail could draw from -- the new mean; the rows of the factor of S' finished before the failed pivot;
    the low half of ``call`` alone"""
    Z = draw(mb["seeds"][k], call, B, D)
    right = sample(mb["mu0"][k], mb["R_kept"][k], Z)
    with np.errstate(all="ignore"):
        wrong = dict(new_mean=sample(mb["mu1"][k], mb["R_kept"][k], Z),
                     failed_factor=sample(mb["mu0"][k], chol_ld(mb["S1"][k], rows=int(mb["codes"][k]) - 1), Z),
                     call_low_half=sample(mb["mu0"][k], mb["R_kept"][k], draw(mb["seeds"][k], call & 0xFFFFFFFF, B, D)))
    return right, wrong


def rel_err(a, b):
    """max |a - b| / max |b| in long double (conftest.rel_err rounds both to float64 first)"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def distinguishable(mb, B, D):
    """the smallest rel_err between the right source's samples and any wrong source's, over the planted problems; for a
    problem reverted by a NaN the new mean and S' are NaN (no finite samples to confuse), so only the draw number counts"""
    worst = np.inf
    for k in mb["reverting"]:
        right, wrong = sources(mb, k, B, D)
        for name, w in wrong.items():
            if np.isfinite(w).all():
                worst = min(worst, rel_err(w, right))
            else:
                assert k == NAN_SLOT and name != "call_low_half", (k, name)
    return worst
