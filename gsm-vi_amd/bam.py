"""BaM fit driver, update functions and regularizer schedules with the reference's signatures
(gsmvi/bam.py).  The update runs in HIP kernels through the engine; see csrc/gsmvi_bam.hip."""
import numpy as np
import torch

from . import _oddpad
from ._fitloop import (KB, Checkpoints, DrawStream, GraphBlock, Progress, _is_torch, _legacy_mvn, eventful, initial_factor,
                       initial_state, result, retry, scorer, seed_of, takes_out)
from .engine import get_engine


def _every(nprint, niter):
    """print cadence of bam.py:177-179: ``nprint`` clamped to niter; every iteration when it is not positive"""
    nprint = min(nprint, niter)
    return max(1, niter // nprint) if nprint > 0 else 1


def bam_lowrank_update(samples, vs, mu0, S0, reg, engine=None, jitter=0.0):
    """Drop-in for ``bam_lowrank_update(samples, vs, mu0, S0, reg)`` (gsmvi/bam.py:72-114).

    The D x B ARPACK factor of U (bam.py:10-13,104) is replaced by an exact rank-B factor of U (Helmert recombination of the centred score rows), so
    there is no B < D restriction; the returned S is symmetrised (the reference symmetrises in
    ``fit``, bam.py:199)."""
    assert len(samples.shape) == 2
    assert len(vs.shape) == 2
    eng = engine if engine is not None else get_engine()
    want_torch = _is_torch(samples)
    Xd, Gd, m0, S0d = eng.asarray(samples), eng.asarray(vs), eng.asarray(mu0), eng.asarray(S0)
    D = int(m0.shape[0])
    if D % 2 == 1 and getattr(eng, "name", "") == "hip":
        # odd D: the (D + 1)-dimensional problem with an inert last coordinate runs on the tuned kernels (_oddpad.py)
        from . import _oddpad
        mu, S, _ = eng.bam_update(_oddpad.pad_rows(eng, Xd, D), _oddpad.pad_rows(eng, Gd, D), _oddpad.pad_vec(eng, m0, D),
                                  _oddpad.pad_mat(eng, S0d, D), float(reg), float(jitter))
        mu, S = mu[:D].contiguous(), S[:D, :D].contiguous()
    else:
        mu, S, _ = eng.bam_update(Xd, Gd, m0, S0d, float(reg), float(jitter))
    return (mu, S) if want_torch else (eng.to_numpy(mu), eng.to_numpy(S))


def bam_update(samples, vs, mu0, S0, reg, engine=None, jitter=0.0):
    """Drop-in for ``bam_update(samples, vs, mu0, S0, reg)`` (gsmvi/bam.py:31-69).  The full-rank
    formula (D x D sqrtm + solve) equals the low-rank one to round-off, so both names
    run the same kernels."""
    return bam_lowrank_update(samples, vs, mu0, S0, reg, engine=engine, jitter=jitter)


class Regularizers:
    """Regularizer schedules for BaM (gsmvi/bam.py:237-274).  As in the reference the schedules
    count CALLS and ignore the ``iteration`` argument, so retries advance them."""

    def __init__(self):
        self.counter = 0

    def reset(self):
        self.counter = 0

    def constant(self, reg0):
        def reg_iter(iteration):
            self.counter += 1
            return reg0
        return reg_iter

    def linear(self, reg0):
        def reg_iter(iteration):
            self.counter += 1
            return reg0 / self.counter
        return reg_iter

    def custom(self, func):
        def reg_iter(iteration):
            self.counter += 1
            return func(self.counter)
        return reg_iter


class BaM:
    """Wrapper class for using BaM updates to fit a distribution (gsmvi/bam.py:117-137).
    ``use_lowrank`` and ``jit_compile`` are accepted for signature compatibility; both update
    forms run the same HIP kernels and there is nothing to jit."""

    def __init__(self, D, lp, lp_g, use_lowrank=False, jit_compile=True, engine=None):
        self.D = D
        self.lp = lp
        self.lp_g = lp_g
        self.use_lowrank = use_lowrank
        self.jit_compile = jit_compile
        self._engine = engine

    def fit(self, key, regf, mean=None, cov=None, batch_size=2, niter=5000, nprint=10, verbose=True,
            check_goodness=True, monitor=None, retries=10, jitter=1e-6, *, sampler="cholesky", rng="auto",
            as_torch=False, forced_samples=None, shard=False, group=None, check_update_flag=False, method="auto",
            root_potrf=False, graph=None, jitter_every=None, _zero_cols_from=None):
        """gsmvi/bam.py:140-216.  Kept: niter+1 iterations (:178); nprint clamp (:177); reg = regf(i)
        per attempt (:196); jitter on the diagonal and symmetrisation (:198-199, done in-kernel);
        retry on any exception up to ``retries`` then re-raise (:189-206); Cholesky accept/revert of
        both mean and cov (:208-212); monitor cadence (:182-185,:214-215).
        Deviation: the JAX threefry key split + per-iteration numpy re-seed (:191-192) is replaced by
        one private RandomState(key) stream (JAX is not a dependency).
        ``shard=True`` (BASELINE config 4: B=128 sharded 16 per GPU; one process per GPU, torch.distributed
        initialised): every rank draws the same Z, samples and scores only its batch_size/world rows, the
        (x_b, g_b) rows are all-gathered (dist.sharded_bam_update) and every replica runs the identical update.
        Retries when sharded are COLLECTIVE: after the score call every rank contributes a fail bit to one
        all-reduce (MAX), so either all ranks retry -- redrawing and advancing the regulariser together -- or
        none does; a rank never re-enters a collective its peers have left (one host synchronisation per
        iteration, small beside the Cholesky of the accept test).
        Deviation (documented): the reference retries on ANY exception inside sample/score/update (:189-206),
        which on its JAX path includes numerical failures surfacing as exceptions from the host callbacks.  The
        device update never raises: a numerical failure poisons the outputs with NaN, the Cholesky accept test
        rejects them and the iteration is a revert (counted in ``n_reverts``), not a retry.
        ``check_update_flag=True`` restores the retry: the update's device flag is read every iteration (one host
        synchronisation) and a non-zero flag raises FloatingPointError into the retry loop.
        ``root_potrf`` (sharded dense fit only; default False): True lets rank 0 run the accept test's Cholesky and broadcast
        the factor and its flag (dist.root_potrf) instead of every rank factoring its identical replica -- saves the
        redundant D^3 work, costs a serial factorisation + an 8 D^2-byte broadcast per iteration; opt-in until measured on
        more than one GPU (see GSM.fit).
        ``method="factor"`` with ``shard=True``: the (x_b, g_b) rows are all-gathered as in the dense form and every replica
        runs the identical factor-form update (dist.sharded_bam_factor_update); retries are collective in the same way.
        ``shard="batch"`` is a synonym of ``shard=True``.  ``shard="cols"``: the COLUMN-sharded factor form -- every rank keeps
        the D / P columns ``dist.col_bounds(D, P, rank)`` of the square factor F and the same entries of the mean; per
        iteration it samples its column slice (all-gathered: B D / P doubles), scores all B samples, and the partial products
        Qt[:, C] F[:, C]^T are all-reduced (B D doubles) before the replicated B x B and 2B x 2B chains and the update of the
        owned block (dist.col_sharded_bam_factor_update).  It is the factor form (``method`` "auto" or "factor"), needs
        sampler="cholesky", no forced samples, D % (64 P) == 0 and 2*batch_size <= min(D, 256).  A jitter cannot be absorbed
        without a D x D factorisation, so it takes ``jitter=0``, or ``jitter_every=0`` (the jitter is dropped); anything else
        raises ValueError before the first collective.  Retries and ``check_update_flag`` are collective as above; the
        covariance is assembled (one all-gather of the blocks) only for the monitor and the return value.  ``shard_stats``
        reports the bytes of one iteration's exchanges and of the owned block.
        ``graph=True``: factor-form fits replay blocks of 16 iterations as one hipGraph (the regulariser table on the device:
        engine.bam_reg_source); bit-identical to the eager loop and, measured, not faster on an idle host -- off by default.
        ``method="auto"`` (round 6): "dense" -- the reference's own loop: update, + jitter * I, symmetrise, Cholesky accept test
        (:189-212) -- whenever ``jitter`` > 0, i.e. at the reference's default arguments (1e-10 from the restated reference loop on the
        same samples: tests/test_gpu_bam.py::test_default_fit_is_the_reference_loop); "factor" for ``jitter`` = 0 where that form
        exists (below), or when ``jitter_every`` is given.  Round 5 took the factor form up to jitter = 1e-6 and dropped the shift:
        2e-5 .. 3e-5 (B = 128) and 1.7e-4 (B = 32) of max|cov| from the reference loop at D = 1024, above the 1e-5 bar.
        ``method="factor"`` (needs 2*batch_size <= min(D, 256), sampler="cholesky", no forced samples):
        the state is (mean, F) with cov = F^T F; every iteration samples with F itself and applies the factor-form BaM
        update (engine.bam_factor_update) -- four passes over F, no D x D covariance, no D^3 Cholesky for the accept
        test (the update's own 2B x 2B positive-definiteness test decides accept/revert, counted in ``n_reverts``).
        The covariance is formed once, for the return value (and for each monitor call).  ``jitter``: a diagonal shift is not a
        low-rank change of a factor, so the fit carries the shift it OWES -- jitter x the accepted updates since the last
        absorption, counted on the device -- adds it to every covariance it hands out, and every ``jitter_every`` (default
        BaM.JITTER_EVERY = 4; 0 = never, the round-5 behaviour) accepted updates absorbs it: F <- chol(F^T F + owed I)
        (gsmvi_gram_shift_f64 + gsmvi_potrf_f64).  Deferring is not free -- the distance to the reference's loop grows in
        proportion to the period (4: 7e-6 at B = 128, 1.8e-5 at B = 32; 16: no better than dropping the jitter;
        profiles/r06/jitter_period.json) -- which is why this form is opt-in whenever jitter > 0.  Everything else -- niter+1
        iterations, reg = regf(i) per attempt, retries, monitor cadence -- is the loop above.
        ``method="dense"`` takes any batch size up to 1024 (the device chain's bound; tuned to 128, a blocked MFMA path above)."""
        eng = self._engine if self._engine is not None else get_engine()
        D, B = self.D, int(batch_size)
        assert method in ("auto", "dense", "factor"), "method must be 'auto', 'dense' or 'factor'"
        if isinstance(shard, str):
            if shard not in ("batch", "cols"):
                raise ValueError(f"BaM.fit: shard must be False, True, 'batch' or 'cols', not {shard!r}")
            shard = True if shard == "batch" else "cols"
        if shard == "cols":
            self._check_cols_args(D, B, method, sampler, forced_samples, jitter, jitter_every, group)
            self.method_used = "factor"
            return self._fit_factor_cols(eng, key, regf, mean, cov, B, niter, nprint, verbose, monitor, retries, rng, as_torch,
                                         check_update_flag, group)
        if _zero_cols_from is None and _oddpad.applies(eng, D, sampler, forced_samples):
            # odd D: the (D + 1)-dimensional problem with an inert last coordinate runs on the tuned kernels (_oddpad.py).
            # (the corner of cov' picks up the jitter like every diagonal entry; it touches nothing else)
            if method == "auto":
                method = self._auto_method(D, B, sampler, forced_samples, jitter, jitter_every)
            inner = BaM(D + 1, self.lp, _oddpad.wrap_score(eng, self.lp_g, D), use_lowrank=self.use_lowrank,
                        jit_compile=self.jit_compile, engine=eng)
            return _oddpad.fit_padded(self, inner, (key, regf), dict(
                batch_size=batch_size, niter=niter, nprint=nprint, verbose=verbose, check_goodness=check_goodness,
                retries=retries, jitter=jitter, sampler=sampler, rng=rng, shard=shard, group=group,
                check_update_flag=check_update_flag, method=method, root_potrf=root_potrf, graph=graph,
                jitter_every=jitter_every), mean, cov, monitor, as_torch, defaults={"graph_replays": 0, "graph_fallback": None})
        self._zc = _zero_cols_from
        if method == "auto":
            method = self._auto_method(D, B, sampler, forced_samples, jitter, jitter_every)
        self.method_used = method
        if method == "factor":
            assert sampler == "cholesky" and forced_samples is None, \
                "method='factor' samples with its own factor (sampler='cholesky', no forced samples)"
            return self._fit_factor(eng, key, regf, mean, cov, B, niter, nprint, verbose, monitor, retries, rng, as_torch,
                                    check_update_flag, shard, group, graph, float(jitter),
                                    self.JITTER_EVERY if jitter_every is None else int(jitter_every))
        bmax = getattr(eng, "bam_max_batch", None)
        if bmax is not None and B > bmax:               # deterministic: raised here, not inside the retry loop
            raise ValueError(f"BaM.fit: batch_size {B} exceeds the device update's limit of {bmax}")
        mean_t, cov_t = initial_state(eng, D, mean, cov)
        seed = seed_of(key, last=True)
        rs = np.random.RandomState(seed)
        assert rng in ("auto", "numpy", "device"), "rng must be 'auto', 'numpy' or 'device'"
        # counter-based device stream (as GSM.fit: see its docstring): one `call` per draw, retries included
        draws = DrawStream(eng, B, D, seed, rs, rng == "device" or (rng == "auto" and sampler == "cholesky"), self._zc)
        score = scorer(eng, self.lp_g)
        lo, hi, world = 0, B, 1
        if shard:
            assert sampler == "cholesky" and forced_samples is None, "shard=True needs the replicated z-stream"
            from .dist import sharded_bam_update, shard_bounds, voted_score, _world_rank, root_potrf as _root_potrf
            world, rank = _world_rank(group)
            lo, hi = shard_bounds(B, world, rank)
        collective = bool(shard) and world > 1
        mean_new, cov_new = eng.empty(D), eng.empty(D, D)
        R, R_new = eng.empty(D, D), eng.empty(D, D)
        Xbuf = eng.empty(hi - lo, D)
        flag, uflag, n_rev = eng.new_flag(), eng.new_flag(), eng.new_flag()
        use_factor = sampler == "cholesky" and forced_samples is None
        if use_factor:                      # the sampling factor of the initial covariance
            initial_factor(eng, cov_t, flag, out=R)
        progress = Progress(eng, n_rev, niter, _every(nprint, niter), verbose)
        mon = Checkpoints(eng, monitor, self.lp, key, lambda: (mean_t, cov_t))

        def attempt(i):
            if forced_samples is not None:
                X = eng.asarray(forced_samples[i])
            elif sampler == "svd":
                X = eng.asarray(_legacy_mvn(rs, eng.to_numpy(mean_t), eng.to_numpy(cov_t), B))
            else:
                X = eng.sample(draws.next()[lo:hi], mean_t, R, out=Xbuf)     # only this rank's rows when sharded
            vs = voted_score(score, X, group) if collective else score(X)
            mon.nevals += B
            reg = regf(i)
            if shard:
                sharded_bam_update(eng, X, vs, mean_t, cov_t, reg, jitter, group=group, out=(mean_new, cov_new), flag=uflag)
            else:
                eng.bam_update(X, vs, mean_t, cov_t, reg, jitter, out=(mean_new, cov_new), flag=uflag)
            if check_update_flag:
                self._check_flag(eng, uflag, collective, group)

        i = 0
        for i in range(niter + 1):
            progress.tick(i)
            mon.tick(i)
            retry(retries, attempt, i)
            if shard and root_potrf and world > 1:          # opt-in: one rank factors, the others receive
                _root_potrf(eng, cov_new, R_new, flag, group=group)
            else:
                eng.potrf(cov_new, out=R_new, flag=flag)
            eng.commit(flag, mean_new, cov_new, mean_t, cov_t, n_rev)
            if use_factor:
                eng.commit(flag, mean_new, R_new, mean_t, R, None)
        mon.final(i)
        self.n_reverts = eng.read_flag(n_rev)
        return result(eng, mean_t, cov_t, as_torch)

    # How often the factor form absorbs the jitter it owes (bam.py:198: cov_new += jitter * I after EVERY update).  A diagonal
    # shift is not a low-rank change of a square factor: the fit carries the owed shift and every JITTER_EVERY accepted updates
    # re-factorises F^T F + owed * I (gsmvi_gram_shift_f64 + gsmvi_potrf_f64).  Deferring is NOT free: the update responds to the
    # shift of its input covariance with an amplification of ~sqrt(cond Sigma), so the distance to the reference's loop on the
    # same samples grows with the period -- measured on the c4-like target of tests/test_gpu_bam.py (profiles/r06/
    # jitter_period.json): see the table in DESIGN.md section 8.2.  0 = never absorb (the round-5 behaviour: jitter ignored).
    JITTER_EVERY = 4

    @staticmethod
    def _auto_method(D, B, sampler, forced_samples, jitter, jitter_every):
        """method="auto" (round 6).  The factor form wherever it exists (2B <= min(D, 256), the device Cholesky sampler, no
        teacher-forced samples) AND the call asks for no jitter; with the reference's default jitter = 1e-6 (bam.py:140,198)
        the default is the reference's own loop -- "dense": the same update + the same shift + the same Cholesky accept test,
        1e-10 from the reference restatement on the same samples.  Round 5 took the factor form up to jitter = 1e-6 and
        dropped the shift; that moved the default 2e-5 .. 3e-5 of max|cov| away from the reference loop (above the 1e-5 bar of
        BASELINE.json), and absorbing the shift every K iterations only brings that down in proportion to K (K = 16: no better
        than dropping it; K = 4: ~4e-6 at (1024, 128) at the cost of a D^3 factorisation every fourth iteration).  The fast form
        therefore is OPT-IN for calls with jitter: method="factor" (absorbs every ``jitter_every`` = 4 accepted updates), or
        jitter=0."""
        exists = sampler == "cholesky" and forced_samples is None and 2 * B <= min(D, 256)
        if not exists:
            return "dense"
        if float(jitter) == 0.0:
            return "factor"
        return "factor" if (jitter_every is not None and int(jitter_every) > 0) else "dense"

    @staticmethod
    def _check_cols_args(D, B, method, sampler, forced_samples, jitter, jitter_every, group):
        """shard="cols": everything that would make the column-sharded factor form wrong is refused here, before the first
        collective (every rank sees the same arguments, so every rank raises)."""
        if method not in ("auto", "factor"):
            raise ValueError("BaM.fit: shard='cols' is the column-sharded FACTOR form (method 'auto' or 'factor')")
        if sampler != "cholesky" or forced_samples is not None:
            raise ValueError("BaM.fit: shard='cols' samples with its own factor (sampler='cholesky', no forced samples)")
        import torch.distributed as _dist
        world = _dist.get_world_size(group) if _dist.is_initialized() else 1
        if D % (64 * world) != 0:
            raise ValueError(f"BaM.fit: shard='cols' needs D ({D}) to be a multiple of 64 x the number of ranks ({world})")
        if 2 * B > min(D, 256):
            raise ValueError("BaM.fit: shard='cols' (factor form) needs 2*batch_size <= min(D, 256)")
        if float(jitter) != 0.0 and (jitter_every is None or int(jitter_every) != 0):
            raise ValueError("BaM.fit: shard='cols' cannot absorb a jitter (that takes a factorisation of the whole D x D "
                             "covariance): pass jitter=0, or jitter_every=0 to drop the jitter")

    @staticmethod
    def _check_flag(eng, flag, collective, group):
        """check_update_flag: raises FloatingPointError (into the retry loop) when the update's device flag is set -- on ANY rank
        when sharded.  The replicas run the identical update on identical inputs, so their flags agree; the failure vote makes
        the retry decision collective anyway (advisor, round 4): a rank that retried alone would pair its next all-gather with
        its peers' NEXT iteration."""
        bad = eng.read_flag(flag) != 0
        if collective:
            from .dist import failure_vote
            bad = failure_vote(bad, group, flag.device if _is_torch(flag) else "cpu")
        if bad:
            raise FloatingPointError("BaM update flagged a numerical failure (device flag != 0)")

    # ------------------------------------------------------------------------------
    def _fit_factor_cols(self, eng, key, regf, mean, cov, B, niter, nprint, verbose, monitor, retries, rng, as_torch,
                         check_update_flag, group=None):
        """Column-sharded factor-form BaM fit (see ``fit(shard="cols")``): the loop of gsmvi/bam.py:140-216 on the state
        (mean[C], F[:, C]) per rank -- niter+1 iterations, reg = regf(i) per attempt, collective retries, the update's own
        2B x 2B test deciding accept / revert (counted in ``n_reverts``).  The draw stream is the one of the replicated factor
        fit (``method="factor"``), so both follow the same path.  The initial factorisation is replicated (once per fit)."""
        from .dist import col_assemble, col_bounds, col_gather_samples, col_sharded_bam_factor_update, voted_score, _world_rank
        D = self.D
        world, rank = _world_rank(group)
        lo, hi = col_bounds(D, world, rank)
        self._zc = None
        self.jitter_every_used = 0                 # (the jitter is dropped: _check_cols_args)
        self.n_absorbed = 0
        mean_a, cov0 = initial_state(eng, D, mean, cov)
        flag, n_rev = eng.new_flag(), eng.new_flag()
        Fc_a = eng.clone(initial_factor(eng, cov0, flag)[:, lo:hi])    # the owned block, D x D / P, its own leading dimension
        del cov0
        bufs = [(mean_a, Fc_a), (eng.clone(mean_a), eng.empty(D, hi - lo))]
        a = 0
        seed = seed_of(key, last=True)
        assert rng in ("auto", "numpy", "device"), "rng must be 'auto', 'numpy' or 'device'"
        draws = DrawStream(eng, B, D, seed, np.random.RandomState(seed), rng != "numpy")
        score = scorer(eng, self.lp_g)
        self.shard_stats = {}

        def state():
            m, F = col_assemble(eng, *bufs[a], group)
            return m, eng.gram(F)

        progress = Progress(eng, n_rev, niter, _every(nprint, niter), verbose)
        mon = Checkpoints(eng, monitor, self.lp, key, state)

        def attempt(i):
            st = {} if i == 0 else None            # the exchanges of one (successful) iteration
            (m_c, F_c), (m_n, F_n) = bufs[a], bufs[1 - a]
            Z = draws.next()
            X = col_gather_samples(eng, eng.sample_cols(Z, m_c[lo:hi], F_c), group, stats=st)
            vs = voted_score(score, X, group) if world > 1 else score(X)
            mon.nevals += B
            reg = regf(i)
            col_sharded_bam_factor_update(eng, Z, X, vs, m_c, F_c, reg, group=group, out=(m_n, F_n), flag=flag, n_reverts=n_rev,
                                          stats=st)
            if check_update_flag:
                self._check_flag(eng, flag, world > 1, group)
            if st is not None:
                self.shard_stats.update(st)

        for i in range(niter + 1):
            progress.tick(i)
            mon.tick(i)
            retry(retries, attempt, i)
            a = 1 - a                   # the kernel already returned the reverted state when its test failed: accept = swap
        mon.final(niter)
        self.n_reverts = eng.read_flag(n_rev)
        self.shard_stats["block_bytes"] = D * (hi - lo) * 8
        return result(eng, *state(), as_torch)

    # ------------------------------------------------------------------------------
    def _fit_factor(self, eng, key, regf, mean, cov, B, niter, nprint, verbose, monitor, retries, rng, as_torch,
                    check_update_flag, shard=False, group=None, graph=None, jitter=0.0, jitter_every=0):
        """Factor-form BaM fit (see ``fit(method="factor")``): the loop of gsmvi/bam.py:140-216 on the state (mean, F).
        ``shard=True``: every rank draws the same Z, samples and scores only its batch_size/world rows; the (x_b, g_b) rows
        are all-gathered and every replica applies the identical factor update (dist.sharded_bam_factor_update)."""
        D = self.D
        assert 2 * B <= min(D, 256), "method='factor' needs 2*batch_size <= min(D, 256)"
        mean_t, cov0 = initial_state(eng, D, mean, cov)
        flag, n_rev = eng.new_flag(), eng.new_flag()
        F = initial_factor(eng, cov0, flag)                 # one factorisation for the whole fit
        seed = seed_of(key, last=True)
        assert rng in ("auto", "numpy", "device"), "rng must be 'auto', 'numpy' or 'device'"
        dev_rng = rng != "numpy"
        draws = DrawStream(eng, B, D, seed, np.random.RandomState(seed), dev_rng, self._zc)
        native = bool(getattr(self.lp_g, "device_native", False))
        score = scorer(eng, self.lp_g)
        lo, hi, world = 0, B, 1
        if shard:
            from .dist import sharded_bam_factor_update, shard_bounds, voted_score, _world_rank
            world, rank = _world_rank(group)
            lo, hi = shard_bounds(B, world, rank)
        collective = bool(shard) and world > 1
        bufs = [(mean_t, F), (eng.empty(D), eng.empty(D, D))]
        Xbuf = eng.empty(hi - lo, D)
        a = 0
        # the jitter of bam.py:198 in factor form: owed = jitter * (accepted updates since the last absorption), absorbed every
        # jitter_every updates by F <- chol(F^T F + owed I) (JITTER_EVERY above); the covariance the monitor and the caller see
        # carries what is still owed, so cov_i = the reference's cov_i up to the response of the last < jitter_every updates
        absorb = jitter > 0.0 and jitter_every > 0
        self.jitter_every_used = jitter_every if absorb else 0
        self.n_absorbed = 0
        pend = 0
        if absorb:
            Cbuf, pflag, mark = eng.empty(D, D), eng.new_flag(), eng.new_flag()

        def cov_of(Fm):
            if absorb and pend > 0:
                return eng.gram(Fm, shift_dev=eng.owed_shift(jitter, pend, n_rev, mark, advance=False))
            return eng.gram(Fm)

        def absorb_now():
            (mu_c, F_c), (mu_o, F_o) = bufs[a], bufs[1 - a]
            eng.gram(F_c, out=Cbuf, shift_dev=eng.owed_shift(jitter, pend, n_rev, mark))
            eng.potrf(Cbuf, out=F_o, flag=pflag)            # the other buffer pair is scratch between two updates
            eng.commit(pflag, mu_c, F_o, mu_o, F_c, None)   # F <- R iff the factorisation succeeded (F^T F + owed I is positive
            self.n_absorbed += 1                            # definite unless the state itself is not finite: then F stays)

        progress = Progress(eng, n_rev, niter, _every(nprint, niter), verbose)
        mon = Checkpoints(eng, monitor, self.lp, key, lambda: (bufs[a][0], cov_of(bufs[a][1])))

        def attempt(i):
            (mu_a, F_a), (mu_b, F_b) = bufs[a], bufs[1 - a]
            Z = draws.next()
            X = eng.sample(Z[lo:hi], mu_a, F_a, out=Xbuf)          # only this rank's rows when sharded
            vs = voted_score(score, X, group) if collective else score(X)
            mon.nevals += B
            reg = regf(i)
            if shard:
                sharded_bam_factor_update(eng, Z, X, vs, mu_a, F_a, reg, group=group, out=(mu_b, F_b), flag=flag,
                                          n_reverts=n_rev)
            else:
                eng.bam_factor_update(Z, X, vs, mu_a, F_a, reg, out=(mu_b, F_b), flag=flag, n_reverts=n_rev)
            if check_update_flag:
                self._check_flag(eng, flag, collective, group)

        # Blocks of KB iterations replayed as ONE hipGraph (as GSM.fit): the launches must all be capturable (a `graph_safe`
        # device score, the counter-based draw stream, no collective, no per-iteration flag read) and the one number that changes
        # between iterations -- reg = regf(i), evaluated on the host by the reference (bam.py:196) -- is read by the kernels from
        # a device word at execution time (engine.bam_reg_source / gsmvi_bam_set_reg_source): iteration k of the block reads word k
        # of a KB-word table that is refilled (regf(i) .. regf(i + KB - 1), one small copy) before every replay.  Blocks with a
        # print or a monitor call, the first block and the tail run eagerly with the by-value argument -- same kernels, same
        # numbers (tests/test_gpu_bam.py: bit-identical).  OFF unless graph=True: measured (scripts/bam_graph_ab.py, marginal
        # iteration of 1200- against 400-iteration fits) the replayed block is not faster than eager launches on this host --
        # 70.9 vs 71.5 us at (256, 8), 151.8 vs 150.1 at (1024, 32), 448 vs 440 at (1024, 128) -- the device is never waiting for
        # the host (enqueueing an update takes 45 - 195 us of host time against 69 - 445 us of device time), and the capture
        # costs ~3 ms.  The 148-against-139 us "eager vs replayed" of a single update is an artefact of timing each eager call
        # from an idle device.  It is kept for callers whose host is slower or shared.
        use_graph = (graph is True and dev_rng and native and not shard and not absorb
                     and not check_update_flag and niter + 1 >= 3 * KB and bool(getattr(self.lp_g, "graph_safe", False)))
        self.graph_replays = 0
        self.graph_fallback = None
        if use_graph:
            out_ok = takes_out(self.lp_g)
            ctr = [torch.zeros(1, dtype=torch.int64, device=draws.block.device) for _ in range(2)]
            reg_blk = torch.zeros(KB, dtype=torch.float64, device=draws.block.device)
            reg_host = [torch.zeros(KB, dtype=torch.float64).pin_memory() for _ in range(4)]
            reg_done = [None] * 4
            Gbuf = eng.empty(hi - lo, D)

            def capture():
                """KB iterations (KB even: the ping-pong state ends where it started); the draw counter and the regulariser
                table live on the device."""
                try:
                    for half in range(2):
                        h0 = half * (KB // 2)
                        Zh = draws.block[h0:h0 + KB // 2]
                        eng.normal_batch(KB // 2, B, D, seed, 0, out=Zh, call_in=ctr[half], call_out=ctr[1 - half])
                        draws.zero(Zh)
                        for k in range(KB // 2):
                            eng.bam_reg_source(reg_blk[h0 + k:h0 + k + 1])
                            (mu_a, F_a), (mu_b, F_b) = bufs[k & 1], bufs[1 - (k & 1)]
                            Xk = eng.sample(Zh[k], mu_a, F_a, out=Xbuf)
                            vk = self.lp_g(Xk, out=Gbuf) if out_ok else self.lp_g(Xk)
                            eng.bam_factor_update(Zh[k], Xk, vk, mu_a, F_a, 1.0, out=(mu_b, F_b), flag=flag, n_reverts=n_rev)   # (reg: ignored, word k is read)
                finally:
                    eng.bam_reg_source(None)

            def prepare(i_first):
                slot = self.graph_replays % 4
                if reg_done[slot] is not None:
                    reg_done[slot].synchronize()                # the copy that last read this pinned slot has run
                for k in range(KB):
                    rk = float(regf(i_first + k))
                    if not rk > 0.0:                             # (what the by-value entry point checks on the host)
                        raise ValueError(f"BaM.fit: regf({i_first + k}) = {rk}: reg must be positive")
                    reg_host[slot][k] = rk
                reg_blk.copy_(reg_host[slot], non_blocking=True)
                reg_done[slot] = torch.cuda.Event()
                reg_done[slot].record()
                ctr[0].fill_(draws.call)

            graph = GraphBlock(self, "BaM.fit", capture)

        i = 0
        while i <= niter:
            blk_end = min(i + KB, niter + 1)
            # (the first block always runs eagerly: every kernel has been launched, and the context sized, before a capture)
            if (use_graph and i > 0 and a == 0 and blk_end - i == KB and draws.call % KB == 0
                    and not eventful(progress, mon, i, blk_end)):
                if graph.run(lambda: prepare(i)):
                    draws.call += KB
                    mon.nevals += B * KB
                    i = blk_end
                else:                                           # capture unsupported here: stay eager for the rest of the fit
                    use_graph = False
                continue
            for i in range(i, blk_end):
                progress.tick(i)
                mon.tick(i)
                retry(retries, attempt, i)
                a = 1 - a               # the kernel already returned the reverted state when its test failed: accept = swap
                if absorb:
                    pend += 1
                    if pend >= jitter_every:
                        absorb_now()
                        pend = 0
            i = blk_end
        mon.final(niter)
        self.n_reverts = eng.read_flag(n_rev)
        return result(eng, bufs[a][0], cov_of(bufs[a][1]), as_torch)
