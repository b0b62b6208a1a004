"""Batched GSM, BaM and ADVI: K independent problems of the same (D, B) in one launch per step (csrc/gsmvi_batched.hip,
csrc/gsmvi_bam_batched.hip, csrc/gsmvi_advi_batched.hip).

The reference's updates are pure functions of (samples, vs, mu0, S0[, reg]) (gsmvi/gsm.py:31-58, gsmvi/bam.py:31-114), so
``jax.vmap`` batches them over a leading problem axis; ``gsm_update_batched`` and ``bam_update_batched`` are those calls.
``GSMBatch.fit`` runs the dense fit of gsm_numpy.py:77-129 and ``BaMBatch.fit`` the dense loop of bam.py:140-216 for K
problems at once: one launch plus the score call per iteration, whatever K is.  ``ADVIBatch.fit`` is the ELBO baseline they are
compared against (gsmvi/advi.py:47-112) in the same form.  Bounds: 1 <= D <= 64, 1 <= B <= 32.
"""
import numpy as np

from ._fitloop import Checkpoints, Progress, _is_torch, result, scorer, seed_of, takes_out
from .engine import get_engine
from .bam import _every as _bam_every
from .gsm import _every
from .monitors import lp_sums

MAX_D = 64
MAX_B = 32


def _check_bounds(D, B, what="batched GSM"):
    if not 1 <= D <= MAX_D:
        raise ValueError(f"{what}: D = {D} is outside 1 <= D <= {MAX_D} (one problem per workgroup, held in LDS)")
    if not 1 <= B <= MAX_B:
        raise ValueError(f"{what}: batch size B = {B} is outside 1 <= B <= {MAX_B}")


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


def _check_monitor(monitor, who):
    """a batched fit takes a monitor that follows K problems (``batched = True``: BatchedKLMonitor) or none"""
    if monitor is not None and not getattr(monitor, "batched", False):
        raise TypeError(f"{who}: the monitor must follow K problems (BatchedKLMonitor, or any monitor with batched = True); "
                        "KLMonitor and DeviceKLMonitor follow one problem")


def _seeds(keys, K, who, last):
    """problem k's stream seed: ``seed_of(keys[k], last)``, as GSM.fit (last=False) or BaM.fit (last=True) takes it from its key"""
    if _is_torch(keys):
        keys = keys.detach().cpu().numpy()
    keys = list(np.asarray(keys).reshape(-1)) if not isinstance(keys, (list, tuple)) else list(keys)
    if len(keys) != K:
        raise ValueError(f"{who}: {len(keys)} keys for K = {K} problems")
    return [seed_of(int(k), last=last) for k in keys]


class _BatchFit:
    """The constructor and the fit loop of GSMBatch and BaMBatch.  A subclass gives its name (``_name``; ``_what`` in bound
    errors), the print cadence of its single-problem fit (``_cadence``), the seed of a key (``_last``, as ``seed_of``
    takes it) and, per fit, the launch of an iteration after the score.  (ADVIBatch takes the constructor and runs a loop of its
    own: its state is not (mean, cov, factor) and nothing in it reverts.)"""

    def __init__(self, K, D, lp, lp_g, engine=None):
        self.K, self.D = int(K), int(D)
        if self.K < 1:
            raise ValueError(f"{self._name}: K = {K} must be at least 1")
        _check_bounds(self.D, 1, self._what)
        self.lp = lp
        self.lp_g = lp_g
        self._engine = engine

    def _fit(self, step, keys, mean, cov, batch_size, niter, nprint, verbose, forced_samples, as_torch, monitor):
        """the loop of ``fit``: ``step(eng, i, X, G, mean, cov, R, n_rev, seeds)`` launches iteration i after the score (R is
        None for teacher-forced samples, seeds None when no next samples are drawn)"""
        who = f"{self._name}.fit"
        _check_monitor(monitor, who)
        K, D, B = self.K, self.D, int(batch_size)
        niter = int(niter)
        _check_bounds(D, B, self._what)
        seeds = _seeds(keys, K, who, last=self._last)
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
        eng.gsm_fit_init_batched(mean_t, cov_t, R, info, seeds_t, X if draw else None)     # a BaM fit starts as a GSM fit
        bad = np.flatnonzero(eng.read_ints(info))
        if bad.size:
            raise ValueError(f"{who}: initial covariance is not positive definite for problem(s) {bad.tolist()}")
        score = scorer(eng, self.lp_g)
        out_ok = not getattr(self.lp_g, "device_native", False) or takes_out(self.lp_g)     # (host_score takes out=)
        Gbuf = eng.empty(K, B, D)
        progress = Progress(eng, n_rev, niter, self._cadence(nprint, niter), verbose, read=lambda t: int(eng.read_ints(t).sum()))
        mon = Checkpoints(eng, monitor, self.lp, keys, lambda: (mean_t, cov_t))
        for i in range(niter + 1):
            progress.tick(i)
            mon.tick(i)
            if not draw:
                X = eng.asarray(forced_samples[i])
            G = score(X, out=Gbuf) if out_ok else score(X)
            mon.nevals += B
            nxt = draw and i < niter
            step(eng, i, X, G, mean_t, cov_t, R if draw else None, n_rev, seeds_t if nxt else None)
        progress.flush()
        mon.final(niter)
        self.n_reverts = eng.read_ints(n_rev)
        return result(eng, mean_t, cov_t, as_torch)


class GSMBatch(_BatchFit):
    """K independent GSM fits of the same dimension D (gsmvi/gsm_numpy.py:60-129, dense form), one launch per iteration.

    K    : number of problems.
    D    : dimensionality, 1 <= D <= 64.
    lp   : batched log-density, (K,rows,D) -> (K,) sums or (K,rows) values: handed to a batched ``monitor`` only.
    lp_g : score (K,B,D) -> (K,B,D).  A plain callable receives and returns numpy arrays (through ``host_score``); a callable
           marked ``device_native`` (``gsmvi_amd.device_score``, ``BatchedGaussianTarget.lp_g``) receives and returns float64
           CUDA tensors and keeps the whole iteration on the GPU.
    """

    _name, _what, _cadence, _last = "GSMBatch", "batched GSM", staticmethod(_every), False

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
        the last print; no per-iteration synchronisation).  ``monitor``: a batched monitor (``BatchedKLMonitor``), called as
        ``monitor(i, [mean, cov], lp, keys, nevals=n)`` with the device state every ``monitor.checkpoint`` iterations before the
        score and once after the loop (the reference's cadence, gsm_numpy.py:110-113,127-128); any other monitor raises
        TypeError.  It only reads the state: the fit returns the same bits with or without it.
        """
        def step(eng, i, X, G, m, c, R, n_rev, seeds):
            eng.gsm_fit_step_batched(X, G, m, c, R, None, n_rev, seeds, i + 1)

        return self._fit(step, keys, mean, cov, batch_size, niter, nprint, verbose, forced_samples, as_torch, monitor)


def _reg_values(reg, K, who, what="reg"):
    """a regulariser (or a step size, ``what``) as the engine takes it: a float, or K per-problem values (ValueError for any
    other length)"""
    if _is_torch(reg):
        reg = reg.detach().cpu().numpy()
    r = np.asarray(reg, dtype=np.float64)
    if r.ndim == 0:
        return float(r)
    r = r.reshape(-1)
    if r.size != K:
        raise ValueError(f"{who}: {what} has {r.size} values for K = {K} problems (give one float or K values)")
    return r


def bam_update_batched(samples, vs, mu0, S0, reg, jitter=0.0, engine=None):
    """``jax.vmap(bam_update)`` over K problems (gsmvi/bam.py:31-114): slice k of the result is
    ``bam_update(samples[k], vs[k], mu0[k], S0[k], reg[k])``, symmetrised, with ``jitter`` on its diagonal (bam.py:198-199).

    Inputs (K,B,D), (K,B,D), (K,D), (K,D,D); ``reg`` one float or K values.  Returns new ``(mu, S)`` of shapes (K,D), (K,D,D)
    and never modifies its inputs.  numpy in -> float64 numpy out; CUDA torch tensors in -> torch out.  Shape errors raise
    AssertionError like the reference (bam.py:47-48); D or B outside 1 <= D <= 64, 1 <= B <= 32, or a reg of another length
    than K, raise ValueError before any device work.  The exact rank-B factor of U replaces ARPACK's (as ``bam_update``), so
    B > D is legal.  A problem whose B x B chain fails (non-finite input) comes back as NaN; the others are unaffected.
    """
    assert len(samples.shape) == 3
    assert len(vs.shape) == 3
    K, B, D = _shape(samples)
    assert _shape(vs) == (K, B, D) and _shape(mu0) == (K, D) and _shape(S0) == (K, D, D)
    _check_bounds(D, B, "batched BaM")
    r = _reg_values(reg, K, "bam_update_batched")
    eng = engine if engine is not None else get_engine()
    want_torch = _is_torch(samples)
    Xd, Gd, m0, S0d = (eng.asarray(a).contiguous() for a in (samples, vs, mu0, S0))
    mu, S = eng.bam_update_batched(Xd, Gd, m0, S0d, r if isinstance(r, float) else eng.batched_regs(r), float(jitter))
    return (mu, S) if want_torch else (eng.to_numpy(mu), eng.to_numpy(S))


def bam_lowrank_update_batched(samples, vs, mu0, S0, reg, jitter=0.0, engine=None):
    """``jax.vmap(bam_lowrank_update)`` (gsmvi/bam.py:72-114): the same call as ``bam_update_batched``."""
    return bam_update_batched(samples, vs, mu0, S0, reg, jitter=jitter, engine=engine)


class BaMBatch(_BatchFit):
    """K independent BaM fits of the same dimension D (gsmvi/bam.py:117-216, the dense loop), one launch per iteration.

    K    : number of problems.
    D    : dimensionality, 1 <= D <= 64.
    lp   : batched log-density, as for GSMBatch (handed to a batched ``monitor`` only).
    lp_g : score (K,B,D) -> (K,B,D), as for GSMBatch (a plain callable gets numpy arrays; a ``device_native`` one float64
           CUDA tensors).
    """

    _name, _what, _cadence, _last = "BaMBatch", "batched BaM", staticmethod(_bam_every), True

    def fit(self, keys, regf, mean=None, cov=None, batch_size=2, niter=5000, nprint=10, verbose=True, jitter=1e-6, *,
            forced_samples=None, as_torch=False, monitor=None):
        """Fit N(mean_k, cov_k) to target k for every k; returns (mean (K,D), cov (K,D,D)) and sets ``n_reverts`` (K ints).

        Problem k is the computation of ``BaM(D, lp_k, lp_g_k).fit(keys[k], regf, method="dense", rng="device", ...)`` with the
        same draws: the z of iteration i is call i of the Philox stream seeded by ``seed_of(keys[k], last=True)`` (odd D: B x
        (D + 1) normals per call, column D dropped); only the round-off differs.  Per problem and iteration (bam.py:189-212):
        the update with reg = regf(i), + jitter I, symmetrised, the Cholesky test, accept or revert of mean, cov and sampling
        factor (kept bit for bit on a revert), the next samples -- one launch after the score.  ``regf(i)`` is called exactly
        once per iteration and returns one float or K values (one per problem); ``Regularizers()`` schedules work as in
        BaM.fit.  ``mean`` / ``cov``: (K,D) / (K,D,D), zeros and identities by default; a cov[k] that is not positive definite
        raises ValueError naming k.  ``forced_samples``: (niter+1, K, B, D) teacher-forced samples.
        Deviation from bam.py:189-206: there is no retry loop.  The device update never raises; a failed chain or a
        non-finite score reverts its own problem alone (counted in ``n_reverts``).  An exception from the score or from
        ``regf`` propagates.  ``monitor``: a batched monitor (``BatchedKLMonitor``) with the cadence of GSMBatch.fit
        (bam.py:182-185,214-215); any other monitor raises TypeError.
        """
        def step(eng, i, X, G, m, c, R, n_rev, seeds):
            reg = _reg_values(regf(i), self.K, "BaMBatch.fit")
            eng.bam_fit_step_batched(X, G, m, c, R, reg if isinstance(reg, float) else eng.batched_regs(reg), float(jitter), None,
                                     n_rev, seeds, i + 1)

        return self._fit(step, keys, mean, cov, batch_size, niter, nprint, verbose, forced_samples, as_torch, monitor)


class Adam:
    """Adam as ``ADVIBatch.fit`` takes it: the counterpart of ``optax.adam(lr, b1, b2, eps)`` in the reference's call
    (examples/example_advi.py) and of ``torch.optim.Adam`` at its defaults.  ``lr``: a float, K per-problem values, or a
    callable ``i -> float or K values`` (an optax schedule), asked once per iteration."""

    def __init__(self, lr, b1=0.9, b2=0.999, eps=1e-8):
        self.lr, self.b1, self.b2, self.eps = lr, float(b1), float(b2), float(eps)
        if not (0.0 <= self.b1 < 1.0 and 0.0 <= self.b2 < 1.0):
            raise ValueError(f"Adam: b1 = {b1} and b2 = {b2} must be in [0, 1)")
        if not self.eps >= 0.0:
            raise ValueError(f"Adam: eps = {eps} must not be negative")

    def lr_at(self, i, K, who):
        """the step size of iteration i: a float, or K values"""
        return _reg_values(self.lr(i) if callable(self.lr) else self.lr, K, who, "lr")


class ADVIBatch(_BatchFit):
    """K independent full-rank ADVI fits of the same dimension D (gsmvi/advi.py:8-112), one launch per iteration after the score.

    The ELBO baseline the reference compares GSM and BaM against, for K problems at once: q_k = N(loc_k, L_k L_k^T), Adam on
    (loc_k, the D (D + 1) / 2 entries of L_k) with the closed-form gradient of the reference's loss (advi.py:31-45), so the
    user supplies the score and no autograd runs (csrc/gsmvi_advi_batched.hip).

    K    : number of problems.
    D    : dimensionality, 1 <= D <= 64.
    lp   : batched log-density, (K,rows,D) -> (K,) sums or (K,rows) values: the losses and a batched ``monitor`` call it; may be
           None (then no losses are returned).
    lp_g : score (K,B,D) -> (K,B,D), as for GSMBatch (a plain callable gets numpy arrays; a ``device_native`` one float64 CUDA
           tensors and keeps the whole iteration on the GPU).
    """

    _name, _what, _cadence, _last = "ADVIBatch", "batched ADVI", staticmethod(_every), False

    def fit(self, keys, opt, mean=None, cov=None, batch_size=8, niter=1000, nprint=10, monitor=None, *, verbose=True,
            track_loss=True, forced_z=None, as_torch=False):
        """Fit N(mean_k, cov_k) to target k for every k; returns (mean (K,D), cov (K,D,D), losses (niter+1,K) or None): the
        reference's positional order and defaults (advi.py:47), ``niter + 1`` steps as the reference runs.

        ``opt``: an ``Adam``.  Per problem and iteration i (advi.py:69-73,100): with the samples x_b = loc + L z_b of the current
        state and their scores, losses[i] = -(sum_b lp(x_b) - sum_b log q(x_b)), the gradient, Adam step i + 1, and the next
        samples from the updated state -- one launch after the score.  z of iteration i is call i of the Philox stream seeded
        by ``seed_of(keys[k])``, in the layout of ``GSMBatch.fit``: with the same keys the two fits consume the same normals.
        ``mean`` / ``cov``: (K,D) / (K,D,D), zeros and identities by default; a cov[k] that is not positive definite raises
        ValueError naming k.  ``forced_z``: (niter+1, K, B, D) teacher-forced normals in place of the stream.  The losses
        accumulate on the device and are read once after the loop; ``track_loss=False`` (or ``lp`` None) never calls ``lp`` and
        returns None for them.  A non-finite score is not caught: that problem's state is NaN from then on, as in the
        reference, and no other problem changes.  ``monitor``: a batched monitor (``BatchedKLMonitor``), called as
        ``monitor(i, [mean, cov], lp, keys, nevals=n)`` with the cadence of advi.py:93-98,109-110; the covariance L L^T is formed
        only at a checkpoint, and the fit returns the same bits with or without a monitor; any other monitor raises TypeError.
        """
        who = "ADVIBatch.fit"
        _check_monitor(monitor, who)
        if not isinstance(opt, Adam):
            raise TypeError(f"{who}: opt must be a gsmvi_amd.Adam (the optimiser is built into the step kernel)")
        K, D, B = self.K, self.D, int(batch_size)
        niter = int(niter)
        _check_bounds(D, B, self._what)
        seeds = _seeds(keys, K, who, last=self._last)
        if mean is not None:
            assert _shape(mean) == (K, D), f"mean: expected shape {(K, D)}"
        if cov is not None:
            assert _shape(cov) == (K, D, D), f"cov: expected shape {(K, D, D)}"
        if forced_z is not None:
            assert _shape(forced_z) == (niter + 1, K, B, D), f"forced_z: expected shape {(niter + 1, K, B, D)}"
        lr0 = opt.lr_at(0, K, who)
        eng = self._engine if self._engine is not None else get_engine()
        P = D * (D + 1) // 2
        loc = eng.zeros(K, D) if mean is None else eng.clone(mean).reshape(K, D)
        cov_t = eng.eye_batch(K, D) if cov is None else eng.clone(cov).reshape(K, D, D)
        draw = forced_z is None
        scales, X, logq, info = eng.empty(K, P), eng.empty(K, B, D), eng.empty(K), eng.batched_ints(K)
        seeds_t = eng.batched_seeds(seeds) if draw else None
        Zf = None if draw else eng.asarray(forced_z)
        eng.advi_init_batched(loc, cov_t, scales, info, seeds_t, None if draw else Zf[0], X, logq)
        bad = np.flatnonzero(eng.read_ints(info))
        if bad.size:
            raise ValueError(f"{who}: initial covariance is not positive definite for problem(s) {bad.tolist()}")
        moments = tuple(eng.zeros(K, n) for n in (D, D, P, P))
        score = scorer(eng, self.lp_g)
        out_ok = not getattr(self.lp_g, "device_native", False) or takes_out(self.lp_g)
        Gbuf = eng.empty(K, B, D)
        track = bool(track_loss) and self.lp is not None
        losses = eng.zeros(niter + 1, K) if track else None
        progress = Progress(eng, None, niter, self._cadence(nprint, niter), verbose, read=lambda t: 0)     # (nothing reverts)
        mon = Checkpoints(eng, monitor, self.lp, keys, lambda: (loc, eng.advi_cov_batched(scales, D)))
        for i in range(niter + 1):
            progress.tick(i)
            mon.tick(i)
            G = score(X, out=Gbuf) if out_ok else score(X)
            mon.nevals += B
            if track:
                losses[i] = logq - lp_sums(self.lp, X, eng, K)
            nxt = i < niter
            lr = lr0 if i == 0 else opt.lr_at(i, K, who)
            eng.advi_step_batched(G, loc, scales, moments, i + 1, lr if isinstance(lr, float) else eng.batched_regs(lr),
                                  opt.b1, opt.b2, opt.eps, seeds=seeds_t, call=i + 1, Zcur=None if draw else Zf[i],
                                  Znext=Zf[i + 1] if nxt and not draw else None, Xout=X if nxt else None,
                                  logq=logq if nxt else None)
        mon.final(niter)
        mean_t, cov_t = result(eng, loc, eng.advi_cov_batched(scales, D), as_torch)
        return mean_t, cov_t, (losses if as_torch or losses is None else eng.to_numpy(losses))
