"""Pieces shared by the fit loops of gsm.py and bam.py: start-up, the draw stream, the progress prints, the monitor
cadence, the retry loop of the reference and the hipGraph block.  Each driver keeps its own loop; what differs between the
drivers stays with them."""
import functools
import inspect
import warnings

import numpy as np
import torch

KB = 16     # the device draws come a block of KB calls per launch (the stream does not depend on the state)


def _is_torch(x):
    return isinstance(x, torch.Tensor)


def _legacy_mvn(rs, mean, cov, size):
    """Compat sampler: the exact stream of ``np.random.multivariate_normal`` after
    ``np.random.seed(key)`` (gsmvi/gsm_numpy.py:105,116): z from MT19937, SVD factor of cov."""
    D = mean.shape[0]
    z = rs.standard_normal((size, D))
    _, s, vt = np.linalg.svd(cov)
    return mean + z @ (np.sqrt(s)[:, None] * vt)


def _host_draw(rs, B, D, zc):
    """(B, D) standard normals from the host stream (rng="numpy": the reference's z-stream, gsm_numpy.py:105,116).  In the padded
    fit of an odd-D problem (zc = the literal D, _oddpad.py) the stream is drawn at the LITERAL width and the inert columns are
    zeros, so a seed gives the same draws as the literal-D problem (round-5 advice: it drew (B, D + 1) and shifted the stream)."""
    if zc is None:
        return rs.standard_normal((B, D))
    z = np.zeros((B, D))
    z[:, :zc] = rs.standard_normal((B, zc))
    return z


def seed_of(key, last):
    """The seed of the fit's streams: GSM takes ``int(key)`` (the first element of a torch key), BaM (``last``) the last
    element of any key."""
    if last:
        return int(np.asarray(key.cpu() if _is_torch(key) else key).flatten()[-1])
    return int(key) if not _is_torch(key) else int(key.flatten()[0])


def initial_state(eng, D, mean, cov):
    """Copies of the initial (mean, cov) -- zeros and the identity by default; the user's arrays are never aliased."""
    return (eng.zeros(D) if mean is None else eng.clone(mean).reshape(D),
            eng.eye(D) if cov is None else eng.clone(cov).reshape(D, D))


def initial_factor(eng, cov, flag, out=None):
    """The Cholesky factor of the initial covariance (into ``out`` when given); a covariance that is not positive definite
    raises ValueError."""
    F, _ = eng.potrf(cov, out=out, flag=flag)
    if eng.read_flag(flag) != 0:
        raise ValueError("initial covariance is not positive definite")
    return F


def scorer(eng, lp_g):
    """X -> lp_g(X): a ``device_native`` score is called as it is, any other through ``eng.host_score``."""
    return lp_g if getattr(lp_g, "device_native", False) else functools.partial(eng.host_score, lp_g)


def takes_out(lp_g):
    """does the score accept an ``out=`` buffer (a graph-captured score must write into a fixed one)"""
    try:
        return "out" in inspect.signature(lp_g).parameters
    except (TypeError, ValueError):
        return False


def result(eng, mean, cov, as_torch):
    return (mean, cov) if as_torch else (eng.to_numpy(mean), eng.to_numpy(cov))


class DrawStream:
    """The whitened draws Z (B, D) of a fit, one per ``next()`` call.  Device (``block`` is not None): the counter-based
    stream, launched a block of KB calls at a time into ``block``; ``call`` counts the draws taken, and a draw's index in the
    stream is its call.  ``limit`` clips the last block to ``limit - call`` draws (GSM: one draw per iteration); without it
    every launch is a whole block (BaM: retries take draws too).  Host: the RandomState stream (``_host_draw``).  The inert
    columns ``zc:`` of a padded odd-D fit (_oddpad.py) are zeros either way."""

    def __init__(self, eng, B, D, seed, rs, device, zc=None, limit=None):
        self.eng, self.B, self.D, self.seed, self.rs, self.zc, self.limit = eng, B, D, seed, rs, zc, limit
        self.block = eng.empty(KB, B, D) if device else None
        self.call = 0

    def next(self):
        c = self.call
        self.call += 1
        if self.block is None:
            return self.zero(self.eng.normal_from_host(_host_draw(self.rs, self.B, self.D, self.zc)))
        if c % KB == 0:
            n = KB if self.limit is None else min(KB, self.limit - c)
            self.eng.normal_batch(n, self.B, self.D, self.seed, c, out=self.block[:n])
            self.zero(self.block)
        return self.block[c % KB]

    def zero(self, Z):
        if self.zc is not None:
            Z[..., self.zc:] = 0.0
        return Z


class Progress:
    """"Iteration i of niter" every ``every`` iterations with the reverts counted on the device since the last print (read
    only here, so the loop never synchronises per iteration); ``flush()`` prints the reverts after the last print.  ``read``
    (default ``eng.read_flag``) turns the counter into a number (a batched fit sums its per-problem counters)."""

    def __init__(self, eng, n_rev, niter, every, verbose, read=None):
        self.eng, self.n_rev, self.niter, self.every, self.verbose = eng, n_rev, niter, every, verbose
        self.read = read
        self.seen = 0

    def due(self, i):
        return self.verbose and i % self.every == 0

    def tick(self, i):
        if self.verbose and i % self.every == 0:
            print(f"Iteration {i} of {self.niter}")
            self._reverts()

    def flush(self):
        if self.verbose:
            self._reverts()

    def _reverts(self):
        r = self.eng.read_flag(self.n_rev) if self.read is None else self.read(self.n_rev)
        if r > self.seen:
            print(f"Bad update for covariance matrix. Revert ({r - self.seen} since last print)")
            self.seen = r


def monitor_state(eng, mean, cov, native):
    """[mean, cov] as a monitor takes them: the device arrays for a ``device_native`` monitor, numpy copies otherwise"""
    return [mean, cov] if native else [eng.to_numpy(mean).copy(), eng.to_numpy(cov).copy()]


class Checkpoints:
    """The monitor cadence of the reference (gsm_numpy.py:103,110-113,119,127-128; bam.py:182-185,214-215): ``monitor`` is
    called every ``monitor.checkpoint`` iterations and once at the end with the score evaluations since its last call
    (``nevals``, counted by the loop).  ``state()`` returns the current (mean, cov)."""

    def __init__(self, eng, monitor, lp, key, state):
        self.eng, self.monitor, self.lp, self.key, self.state = eng, monitor, lp, key, state
        self.native = bool(getattr(monitor, "device_native", False)) if monitor is not None else False
        self.nevals = 1

    def due(self, i):
        return self.monitor is not None and i % self.monitor.checkpoint == 0

    def tick(self, i):
        if self.monitor is not None and i % self.monitor.checkpoint == 0:
            self.final(i)
            self.nevals = 0

    def final(self, i):
        if self.monitor is not None:
            self.monitor(i, monitor_state(self.eng, *self.state(), self.native), self.lp, self.key, nevals=self.nevals)


def eventful(progress, checkpoints, i, end):
    """does any of the iterations [i, end) print or call the monitor (such a block runs eagerly)"""
    return any(progress.due(j) or checkpoints.due(j) for j in range(i, end))


def retry(retries, attempt, i):
    """attempt(i) until it returns; on an exception retry up to ``retries`` times, then re-raise (gsmvi/bam.py:189-206)."""
    j = 0
    while True:
        try:
            return attempt(i)
        except Exception as e:                      # noqa: BLE001 -- reference behaviour
            if j < retries:
                j += 1
                print(f"Failed with exception {e}")
                print(f"Trying again {j} of {retries}")
            else:
                raise e


class GraphBlock:
    """A block of KB iterations captured ONCE into a hipGraph (``capture()`` issues its launches) and replayed.  The capture
    runs on a side stream behind the current one.  A failed FIRST capture warns (``who``: the fit's name), records the
    exception in ``fit.graph_fallback`` and returns False: the caller goes on with eager launches.  ``fit.graph_replays``
    counts the replays."""

    def __init__(self, fit, who, capture):
        self.fit, self.who, self.capture, self.graph = fit, who, capture, None

    def run(self, prepare):
        """capture on first use, ``prepare()`` (what the replay reads from the device), replay; True when replayed"""
        try:
            if self.graph is None:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                g = torch.cuda.CUDAGraph()
                with torch.cuda.stream(side):
                    torch.cuda.synchronize()
                    with torch.cuda.graph(g, stream=side):
                        self.capture()
                torch.cuda.current_stream().wait_stream(side)
                self.graph = g
            prepare()
            self.graph.replay()
        except Exception as exc:                    # noqa: BLE001 -- capture unsupported here: stay eager for the rest of the fit
            if self.graph is not None:
                raise
            warnings.warn(f"{self.who}: hipGraph capture of an iteration block failed ({type(exc).__name__}: {exc}); "
                          "the fit continues with eager launches (same numbers, more launch overhead)", RuntimeWarning)
            self.fit.graph_fallback = exc
            torch.cuda.synchronize()
            return False
        self.fit.graph_replays += 1
        return True
