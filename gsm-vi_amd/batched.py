"""Batched GSM: K independent problems of the same (D, B) in one launch per step (csrc/gsmvi_batched.hip).

The reference's update is a pure function of (samples, vs, mu0, S0) (gsmvi/gsm.py:31-58), so ``jax.vmap(gsm_update)`` batches
it over a leading problem axis; ``gsm_update_batched`` is that call.  ``GSMBatch.fit`` runs the dense fit of gsm_numpy.py:77-129
for K problems at once: one launch plus the score call per iteration, whatever K is.  Bounds: 1 <= D <= 64, 1 <= B <= 32.
"""
import numpy as np

from ._fitloop import Progress, _is_torch, result, scorer, seed_of, takes_out
from .engine import get_engine
from .gsm import _every

MAX_D = 64
MAX_B = 32


def _check_bounds(D, B):
    if not 1 <= D <= MAX_D:
        raise ValueError(f"batched GSM: D = {D} is outside 1 <= D <= {MAX_D} (one problem per workgroup, held in LDS)")
    if not 1 <= B <= MAX_B:
        raise ValueError(f"batched GSM: batch size B = {B} is outside 1 <= B <= {MAX_B}")


def _shape(x):
    return tuple(int(n) for n in x.shape)


def gsm_update_batched(samples, vs, mu0, S0, engine=None):
    """``jax.vmap(gsm_update)`` over K problems (gsmvi/gsm_numpy.py:27-55, gsmvi/gsm.py:31-58): slice k of the result is
    ``gsm_update(samples[k], vs[k], mu0[k], S0[k])``.

    Inputs (K,B,D), (K,B,D), (K,D), (K,D,D); returns new ``(mu, S)`` of shapes (K,D), (K,D,D) and never modifies its inputs.
    numpy in -> float64 numpy out; CUDA torch tensors in -> torch out.  Shape errors raise AssertionError like the reference
    (gsm_numpy.py:43-44); D or B outside 1 <= D <= 64, 1 <= B <= 32 raise ValueError before any device work.
    Reads ALL of each S0[k] (both triangles): the reference's literal S = S0 + mean semantics for any square S0, unlike the
    single-problem ``gsm_update``, which takes a device S0 to be symmetric and reads its upper triangle.
    """
    assert len(samples.shape) == 3
    assert len(vs.shape) == 3
    K, B, D = _shape(samples)
    assert _shape(vs) == (K, B, D) and _shape(mu0) == (K, D) and _shape(S0) == (K, D, D)
    _check_bounds(D, B)
    eng = engine if engine is not None else get_engine()
    want_torch = _is_torch(samples)
    Xd, Gd, m0, S0d = (eng.asarray(a).contiguous() for a in (samples, vs, mu0, S0))
    mu, S = eng.gsm_update_batched(Xd, Gd, m0, S0d)
    return (mu, S) if want_torch else (eng.to_numpy(mu), eng.to_numpy(S))


def _seeds(keys, K):
    """problem k's stream seed: ``seed_of(keys[k])``, as GSM.fit takes it from its key"""
    if _is_torch(keys):
        keys = keys.detach().cpu().numpy()
    keys = list(np.asarray(keys).reshape(-1)) if not isinstance(keys, (list, tuple)) else list(keys)
    if len(keys) != K:
        raise ValueError(f"GSMBatch.fit: {len(keys)} keys for K = {K} problems")
    return [seed_of(int(k), last=False) for k in keys]


class GSMBatch:
    """K independent GSM fits of the same dimension D (gsmvi/gsm_numpy.py:60-129, dense form), one launch per iteration.

    K    : number of problems.
    D    : dimensionality, 1 <= D <= 64.
    lp   : batched log-density (kept for symmetry with GSM; the fit does not call it).
    lp_g : score (K,B,D) -> (K,B,D).  A plain callable receives and returns numpy arrays (through ``host_score``); a callable
           marked ``device_native`` (``gsmvi_amd.device_score``, ``BatchedGaussianTarget.lp_g``) receives and returns float64
           CUDA tensors and keeps the whole iteration on the GPU.
    """

    def __init__(self, K, D, lp, lp_g, engine=None):
        self.K, self.D = int(K), int(D)
        if self.K < 1:
            raise ValueError(f"GSMBatch: K = {K} must be at least 1")
        _check_bounds(self.D, 1)
        self.lp = lp
        self.lp_g = lp_g
        self._engine = engine

    def fit(self, keys, mean=None, cov=None, batch_size=2, niter=5000, nprint=10, verbose=True, *, forced_samples=None,
            as_torch=False, monitor=None):
        """Fit N(mean_k, cov_k) to target k for every k; returns (mean (K,D), cov (K,D,D)) and sets ``n_reverts`` (K ints).

        Problem k is the computation of ``GSM(D, lp_k, lp_g_k).fit(keys[k], method="dense", rng="device", ...)`` with the same
        draws: the z of iteration i is call i of the Philox stream seeded by ``seed_of(keys[k])`` (odd D: the padded layout of
        that fit, B x (D + 1) normals per call, column D dropped); only the round-off of the factorisation differs.  Per problem
        and iteration: update, Cholesky test (gsm_numpy.py:121-146), accept or revert of mean, cov and sampling factor (kept bit
        for bit on a revert), next samples -- one launch after the score.  ``mean`` / ``cov``: (K,D) / (K,D,D), zeros and
        identities by default; a cov[k] that is not positive definite raises ValueError naming k.  ``forced_samples``:
        (niter+1, K, B, D) teacher-forced samples.  Progress prints follow GSM.fit (reverts summed over the problems since
        the last print; no per-iteration synchronisation).  ``monitor`` is not supported.
        """
        if monitor is not None:
            raise TypeError("GSMBatch.fit does not support a monitor; fit without one (or use GSM.fit per problem)")
        K, D, B = self.K, self.D, int(batch_size)
        niter = int(niter)
        _check_bounds(D, B)
        seeds = _seeds(keys, K)
        if mean is not None:
            assert _shape(mean) == (K, D), f"mean: expected shape {(K, D)}"
        if cov is not None:
            assert _shape(cov) == (K, D, D), f"cov: expected shape {(K, D, D)}"
        if forced_samples is not None:
            assert _shape(forced_samples) == (niter + 1, K, B, D), f"forced_samples: expected shape {(niter + 1, K, B, D)}"
        eng = self._engine if self._engine is not None else get_engine()
        mean_t = eng.zeros(K, D) if mean is None else eng.clone(mean).reshape(K, D)
        cov_t = eng.eye_batch(K, D) if cov is None else eng.clone(cov).reshape(K, D, D)
        draw = forced_samples is None
        R = eng.empty(K, D, D)
        X = eng.empty(K, B, D)
        info, n_rev = eng.batched_ints(K), eng.batched_ints(K)
        seeds_t = eng.batched_seeds(seeds) if draw else None
        eng.gsm_fit_init_batched(mean_t, cov_t, R, info, seeds_t, X if draw else None)
        bad = np.flatnonzero(eng.read_ints(info))
        if bad.size:
            raise ValueError(f"GSMBatch.fit: initial covariance is not positive definite for problem(s) {bad.tolist()}")
        score = scorer(eng, self.lp_g)
        out_ok = not getattr(self.lp_g, "device_native", False) or takes_out(self.lp_g)     # (host_score takes out=)
        Gbuf = eng.empty(K, B, D)
        progress = Progress(eng, n_rev, niter, _every(nprint, niter), verbose, read=lambda t: int(eng.read_ints(t).sum()))
        for i in range(niter + 1):
            progress.tick(i)
            if not draw:
                X = eng.asarray(forced_samples[i])
            G = score(X, out=Gbuf) if out_ok else score(X)
            nxt = draw and i < niter
            eng.gsm_fit_step_batched(X, G, mean_t, cov_t, R if draw else None, None, n_rev, seeds_t if nxt else None, i + 1)
        progress.flush()
        self.n_reverts = eng.read_ints(n_rev)
        return result(eng, mean_t, cov_t, as_torch)
