"""HipEngine: the device-side operations of the GSM/BaM hot path on torch-ROCm storage.

Every numeric operation is one call into libgsmvi_hip.so on the current torch stream; torch only
allocates tensors.  The fit drivers (gsm.py, bam.py) talk to an *engine object* with this
interface, which is how the CPU test-suite exercises their host logic with an oracle-backed
engine (tests/engines.py) while the product default is always this class.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("gsmvi_amd needs an AMD GPU visible to torch (torch.cuda.is_available() is False); "
                           "there is no CPU fallback.")


def _unheld_entry(pool):
    """The first (pinned tensor, numpy view) entry of a host_score pool whose numpy array nobody outside the pool holds, or None.
    ``sys.getrefcount(e[1])`` is 2 for an array referenced by the pool's tuple alone (the tuple + getrefcount's own argument:
    measured on CPython 3.10; round-5 advice -- the threshold stood at 3 and handed out an array that ONE outside holder, a
    recording wrapper or a retained view such as x[:, :k] whose ``.base`` is the array, still referenced)."""
    import sys
    for e in pool:
        if sys.getrefcount(e[1]) <= 2:
            return e
    return None


def _device_index(device):
    """the index of ``device``: None = torch's current device, an int, or anything torch.device takes (no index: 0)"""
    if device is None:
        return torch.cuda.current_device()
    return device if isinstance(device, int) else (torch.device(device).index or 0)


def _ptr(t):
    """the raw device address of a tensor; None travels as NULL"""
    return None if t is None else C.c_void_p(t.data_ptr())


class HipEngine:
    """One context (workspace + launch heuristics) on one device; grows on demand."""

    name = "hip"
    factor_max_rows = 256      # largest 2B of the factor-form updates (GSMVI_FACTOR_NMAX; the 2B x 2B chain: one workgroup up to 64,
                               # one-workgroup factorisations up to 128, two-level blocked above)
    bam_max_batch = 1024       # B <= 1024 (round 6; 640 before): the B x B chain's last stage (k_bam_post_big, csrc/gsmvi_bam_small.hip) owns
                               # one entry per thread of a 1024-thread workgroup.  The one-workgroup chain covers B <= 128, larger
                               # batches take the blocked multi-workgroup Cholesky and an O(B^2 D) substitution: they work, untuned

    def __init__(self, device=None, max_D=0, max_B=0):
        self.lib = _lib.load_library()
        _require_gpu()
        self.device = torch.device("cuda", _device_index(device))
        self._ctx = C.c_void_p()
        self._max_D = 0
        self._max_B = 0
        self._tuning = {}
        self._retired = []         # outgrown contexts: kept alive, a captured hipGraph may still launch into their workspace
        self._ctx_captured = False  # has the current context been used under stream capture (a graph may hold its pointers)
        self._stage = {}           # shape -> [pinned staging tensor, event behind its last host -> device copy] (from_host)
        self._hs = {}              # shape -> pinned buffers of the host-callable round trip (host_score)
        self.host_score_profile = None   # a dict here makes host_score accumulate its three phases (benchmarks only)
        self._reg_word = None      # the device word BaM's regulariser is read from (bam_reg_source), kept alive while it is the source
        self._gh_tables = {}       # Q -> device copy of the Q-point Gauss-Hermite table (glm_predict_batched)
        if max_D and max_B:
            self._ensure(max_D, max_B)

    # ---- context management -------------------------------------------------------------
    def _ensure(self, D, B):
        if self._ctx and D <= self._max_D and B <= self._max_B:
            return
        newD, newB = max(D, self._max_D), max(B, self._max_B)
        if self._ctx:
            # The outgrown context is RETIRED, not destroyed: kernels enqueued on it may still be running and, worse, a hipGraph
            # captured earlier (GSM.fit's replayed blocks, a user's torch.cuda.graph around engine calls) holds raw pointers
            # into its workspace.  It costs its workspace (~100 MiB at D=4096) until release_retired() / close().
            # (advisor, round 4) A long-lived engine that sweeps growing shapes must not hoard them: a context that was never
            # used while a stream capture was active cannot be referenced by a graph -- it is destroyed behind a device
            # synchronisation; and the workspace grows geometrically (at least 1.5x per regrow in the dimension that grew), so
            # the retired list of an ever-growing sweep stays logarithmic.
            if self._ctx_captured:
                self._retired.append(self._ctx)
            else:
                torch.cuda.synchronize(self.device)
                self.lib.gsmvi_destroy(self._ctx)
            self._ctx = C.c_void_p()
            self._ctx_captured = False
            if newD > self._max_D:
                newD = max(newD, (3 * self._max_D + 1) // 2)
            if newB > self._max_B:
                newB = max(newB, (3 * self._max_B + 1) // 2)
        ctx = C.c_void_p()
        _lib.check("gsmvi_create", self.lib.gsmvi_create(C.byref(ctx), self.device.index, newD, newB))
        self._ctx, self._max_D, self._max_B = ctx, newD, newB
        for k, v in self._tuning.items():          # knobs survive a context regrow
            self._call_ctx("gsmvi_set_tuning", k.encode(), int(v))
        if self._reg_word is not None:             # ... and so does the regulariser's device source (bam_reg_source): a regrown
            self._call_ctx("gsmvi_bam_set_reg_source", _ptr(self._reg_word))     # context that fell back to the by-value argument would be WRONG

    def _any_ctx(self):
        """a context of any size: the entry points that use no (D, B) workspace need one all the same"""
        self._ensure(max(self._max_D, 1), max(self._max_B, 1))

    def _call(self, name, *args):
        """one launch: entry point ``name`` on the current context and torch stream; a non-zero status raises (_lib.check).
        Call it after the method's ``_ensure``: the context is read here."""
        _lib.check(name, getattr(self.lib, name)(self._ctx, self._stream(), *args))

    def _call_ctx(self, name, *args):
        """the same for the entry points that take the context and no stream (knobs, path bits, profile)"""
        _lib.check(name, getattr(self.lib, name)(self._ctx, *args))

    def release_retired(self):
        """Destroy the contexts a regrow left behind.  Only when no captured graph that used them will be replayed again."""
        if self._retired:
            torch.cuda.synchronize(self.device)
            for c in self._retired:
                self.lib.gsmvi_destroy(c)
            self._retired = []

    def close(self):
        self.release_retired()
        if self._ctx:
            torch.cuda.synchronize(self.device)
            self.lib.gsmvi_destroy(self._ctx)
            self._ctx = C.c_void_p()
            self._max_D = self._max_B = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tuning(self, name, value):
        self._tuning[name] = int(value)
        self._any_ctx()
        self._call_ctx("gsmvi_set_tuning", name.encode(), int(value))

    # ---- array helpers ------------------------------------------------------------------
    def asarray(self, x):
        """float64 device tensor with unit inner stride (copies host data to the device)."""
        if isinstance(x, torch.Tensor):
            t = x.to(device=self.device, dtype=torch.float64)
        else:
            t = torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64)), device=self.device)
        if t.dim() >= 1 and t.stride(-1) != 1:
            t = t.contiguous()
        return t

    def clone(self, x):
        """Owned device copy (the drivers never alias or mutate the caller's arrays)."""
        return self.asarray(x).clone()

    def to_numpy(self, t):
        return t.detach().to("cpu").numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    # ---- the host-callable round trip of the fit loops (gsmvi/gsm_numpy.py:117: vs = self.lp_g(samples) on host arrays) ----
    def to_host(self, t):
        """A device tensor as a FRESH numpy array, through pinned memory: one non-blocking copy on the current stream and
        one stream synchronisation (a pageable ``.cpu()`` stages through the driver's bounce buffer and blocks twice).  The
        array owns its (pinned) storage -- torch's caching host allocator hands the block out again only after the array is
        dropped -- so a callable that keeps its argument (a recording wrapper, say) is not overwritten by the next iteration."""
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t.detach(), non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return h.numpy()

    def from_host(self, a, out=None):
        """A host array as a float64 device tensor (``out`` when given), through a pinned staging buffer owned by the engine:
        a host memcpy into the buffer, then ONE non-blocking copy on the current stream -- no host synchronisation.  The
        buffer of a shape is reused; an event recorded behind its last copy is waited for before it is overwritten (the fit
        loops never get there early: their next device -> host copy is ordered behind it on the same stream)."""
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        a = np.asarray(a)
        key = tuple(a.shape)
        ent = self._stage.get(key)
        if ent is None:
            if len(self._stage) >= 8:                          # (a fit uses one or two shapes; do not hoard pinned memory)
                self._stage.clear()
            ent = self._stage[key] = [torch.empty(a.shape, dtype=torch.float64, pin_memory=True), None]
        buf, ev = ent
        if ev is not None:
            ev.synchronize()
        np.copyto(buf.numpy(), a, casting="unsafe")           # (also the float32 -> float64 conversion of gsm_numpy.py:47)
        out = self.empty(*a.shape) if out is None else out
        assert tuple(out.shape) == key, f"lp_g returned shape {key}, expected {tuple(out.shape)}"
        out.copy_(buf, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        ent[1] = ev
        return out

    def host_score(self, lp_g, X, out=None):
        """vs = lp_g(samples) for a HOST callable (gsm_numpy.py:117; examples/example_gsm_numpy.py:24-29): samples to the host,
        the user's numpy code, scores back to the device.  Per call: one non-blocking device -> host copy into a pinned
        buffer, ONE stream synchronisation, the callable, a host memcpy of its result into a pinned staging buffer and one
        non-blocking host -> device copy -- no allocation, no event, no second synchronisation (round 5; before: pageable
        ``.cpu()`` and ``.to(device)``, two blocking copies through the driver's bounce buffers).
        Buffers are cached per shape.  The samples array handed to the callable comes from a small pool and is reused only
        when nobody else holds a reference to it (a callable that records its argument keeps it intact); the score staging
        buffer is overwritten only behind this call's own synchronisation, which orders it behind the previous upload on the
        same stream (a different stream since the last call: a full device synchronisation first)."""
        key = tuple(X.shape)
        hs = self._hs.get(key)
        if hs is None:
            if len(self._hs) >= 8:
                self._hs.clear()
            gp = torch.empty(key, dtype=torch.float64, pin_memory=True)
            hs = self._hs[key] = {"pool": [], "gpin": gp, "gnp": gp.numpy(), "stream": None}
        stream = torch.cuda.current_stream(self.device)
        if hs["stream"] is not None and hs["stream"] != stream.cuda_stream:
            torch.cuda.synchronize(self.device)
        hs["stream"] = stream.cuda_stream
        ent = _unheld_entry(hs["pool"])
        if ent is None:
            xp = torch.empty(key, dtype=torch.float64, pin_memory=True)
            ent = (xp, xp.numpy())
            if len(hs["pool"]) < 4:
                hs["pool"].append(ent)
        prof = self.host_score_profile                        # None, or a dict the call-path benchmark reads (bench.callpath_rates)
        if prof is not None:
            import time
            t0 = time.perf_counter()
        ent[0].copy_(X.detach(), non_blocking=True)
        stream.synchronize()                                  # (polling an event instead was measured: no difference)
        if prof is not None:
            t1 = time.perf_counter()
        g = lp_g(ent[1])
        if prof is not None:
            t2 = time.perf_counter()
        if isinstance(g, torch.Tensor):
            g = g.detach().cpu().numpy()
        g = np.asarray(g)
        out = self.empty(*key) if out is None else out
        assert g.shape == key and tuple(out.shape) == key, f"lp_g returned shape {g.shape}, expected {key}"
        np.copyto(hs["gnp"], g, casting="unsafe")             # (also float32 -> float64: gsm_numpy.py:47 returns float64)
        out.copy_(hs["gpin"], non_blocking=True)
        if prof is not None:
            t3 = time.perf_counter()
            prof["calls"] = prof.get("calls", 0) + 1
            prof["d2h_and_sync_s"] = prof.get("d2h_and_sync_s", 0.0) + (t1 - t0)     # waits for the device work in front of it too
            prof["callable_s"] = prof.get("callable_s", 0.0) + (t2 - t1)
            prof["stage_and_h2d_enqueue_s"] = prof.get("stage_and_h2d_enqueue_s", 0.0) + (t3 - t2)
        return out

    def empty(self, *shape):
        return torch.empty(*shape, dtype=torch.float64, device=self.device)

    def eye(self, D):
        return torch.eye(D, dtype=torch.float64, device=self.device)

    def zeros(self, *shape):
        return torch.zeros(*shape, dtype=torch.float64, device=self.device)

    def new_flag(self):
        return torch.zeros(1, dtype=torch.int32, device=self.device)

    def read_flag(self, flag):
        return int(flag.item())          # synchronises

    def flag_tensor(self, flag):
        """the tensor a collective moves for a flag (dist.root_potrf): the flag itself"""
        return flag

    def flag_assign(self, flag, t):
        """adopt the received value (nothing to do: the collective wrote into the flag's own storage)"""
        return flag

    def normal_from_host(self, z_host):
        """Upload a host (B,D) array of standard normals (parity mode: numpy MT19937 stream)."""
        return self.from_host(z_host)

    def normal(self, B, D, seed, call=0, out=None, raw=None):
        """(B, D) standard normals from the counter-based device stream (csrc/gsmvi_rng.hip): a pure function of
        (seed, call, element index).  Replaces the z-stream of np.random.multivariate_normal
        (gsmvi/gsm_numpy.py:105,116); ``call`` is the fit iteration."""
        self._any_ctx()
        Z = self.empty(B, D) if out is None else out
        assert Z.is_contiguous() and Z.numel() == B * D
        self._call("gsmvi_randn_f64", int(seed) & (2 ** 64 - 1), int(call), B * D, _ptr(Z), _ptr(raw))
        return Z

    def normal_batch(self, ncalls, B, D, seed, call0=0, out=None, call_in=None, call_out=None):
        """(ncalls, B, D) standard normals: slice c is bit-identical to ``normal(B, D, seed, call0 + c)`` -- one launch for a
        block of fit iterations (the draw stream does not depend on the state).  ``call_in`` / ``call_out``: device int64
        words (1-element tensors); *call_in is added to call0 on the device and *call_out receives *call_in + ncalls, so a
        graph-captured launch advances through the stream on every replay."""
        self._any_ctx()
        Z = self.empty(ncalls, B, D) if out is None else out
        assert Z.is_contiguous() and Z.numel() == ncalls * B * D
        self._call("gsmvi_randn_batch_f64", int(seed) & (2 ** 64 - 1), int(call0), int(ncalls), B * D,
                   _ptr(Z), _ptr(call_in), _ptr(call_out))
        return Z

    def _stream(self):
        if not self._ctx_captured and torch.cuda.is_current_stream_capturing():
            self._ctx_captured = True       # this context's workspace is now referenced by a graph: never destroy it on regrow
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _mat(t, name):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64, \
            f"{name}: expected a float64 CUDA tensor"
        assert t.dim() == 2 and t.stride(1) == 1, f"{name}: expected a 2-D tensor with unit inner stride"
        return _ptr(t), int(t.stride(0)) if t.shape[0] > 1 else int(max(t.stride(0), t.shape[1]))

    @staticmethod
    def _vec(t, name):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 1 \
            and (t.numel() <= 1 or t.stride(0) == 1), f"{name}: expected a contiguous float64 CUDA vector"
        return _ptr(t)

    # ---- the hot path -------------------------------------------------------------------
    def gsm_update(self, X, G, mu0, S0, out=None, general=False):
        """(mu, S) = gsm_update(samples, vs, mu0, S0)   [gsmvi/gsm_numpy.py:27-55].  S0 must be symmetric (a covariance)
        unless ``general=True``, which reads all of S0 (gsmvi_gsm_update_general_f64: the reference's literal
        S0 + mean semantics for any square S0; not a performance path)."""
        assert X.dim() == 2 and G.dim() == 2            # gsm_numpy.py:43-44
        B, D = X.shape
        assert G.shape == (B, D) and mu0.shape == (D,) and S0.shape == (D, D)
        self._ensure(D, B)
        mu, S = (self.empty(D), self.empty(D, D)) if out is None else out
        name = "gsmvi_gsm_update_general_f64" if general else "gsmvi_gsm_update_f64"
        self._call(name, D, B, *self._mat(X, "samples"), *self._mat(G, "vs"), self._vec(mu0, "mu0"), *self._mat(S0, "S0"),
                   self._vec(mu, "mu"), *self._mat(S, "S"))
        return mu, S

    def record_len(self, D):
        return int(self.lib.gsmvi_gsm_record_len(int(D)))

    def gsm_local_stage(self, X, G, mu0, S0, out=None):
        """Per-sample records [d | e | dmu] for this rank's samples (batch-sharded path;
        gsmvi/gsm_numpy.py:7-18 for each local sample)."""
        Bl, D = X.shape
        self._ensure(D, Bl)
        rec = self.empty(Bl, self.record_len(D)) if out is None else out
        self._call("gsmvi_gsm_local_stage_f64", D, Bl, *self._mat(X, "samples"), *self._mat(G, "vs"), self._vec(mu0, "mu0"),
                   *self._mat(S0, "S0"), *self._mat(rec, "rec"))
        return rec

    def gsm_apply(self, rec, mu0, S0, out=None):
        """Combined rank-2B update from ALL samples' records (gsmvi/gsm_numpy.py:17-23,50-53)."""
        B = rec.shape[0]
        D = mu0.shape[0]
        self._ensure(D, B)
        mu, S = (self.empty(D), self.empty(D, D)) if out is None else out
        self._call("gsmvi_gsm_apply_f64", D, B, *self._mat(rec, "rec"), self._vec(mu0, "mu0"), *self._mat(S0, "S0"),
                   self._vec(mu, "mu"), *self._mat(S, "S"))
        return mu, S

    # ---- row-block sharded covariance ---------------------------------
    def gsm_rows_stage(self, G, S0_rows, out=None):
        """Columns [row0, row0+nrows) of G S0 from the owned row block of the symmetric S0 (gsm_numpy.py:7)."""
        B, D = G.shape
        nr = S0_rows.shape[0]
        assert S0_rows.shape == (nr, D)
        self._ensure(D, B)
        SGc = self.empty(B, nr) if out is None else out
        self._call("gsmvi_gsm_rows_stage_f64", D, B, nr, *self._mat(G, "vs"), *self._mat(S0_rows, "S0_rows"),
                   *self._mat(SGc, "SGcols"))
        return SGc

    def gsm_records(self, X, G, mu0, SG, out=None):
        """Records [d | e | dmu] of all samples from the gathered SG = G S0 (gsm_numpy.py:8-17)."""
        B, D = X.shape
        assert SG.shape == (B, D) and SG.is_contiguous()
        self._ensure(D, B)
        rec = self.empty(B, self.record_len(D)) if out is None else out
        self._call("gsmvi_gsm_records_f64", D, B, *self._mat(X, "samples"), *self._mat(G, "vs"), self._vec(mu0, "mu0"),
                   _ptr(SG), *self._mat(rec, "rec"))
        return rec

    def gsm_apply_rows(self, rec, mu0, S0_rows, row0, out=None):
        """(mu, S_rows): the rank-2B update restricted to the owned rows, and the full new mean."""
        B = rec.shape[0]
        D = mu0.shape[0]
        nr = S0_rows.shape[0]
        self._ensure(D, B)
        mu, S = (self.empty(D), self.empty(nr, D)) if out is None else out
        self._call("gsmvi_gsm_apply_rows_f64", D, B, int(row0), nr, *self._mat(rec, "rec"), self._vec(mu0, "mu0"),
                   *self._mat(S0_rows, "S0_rows"), self._vec(mu, "mu"), *self._mat(S, "S_rows"))
        return mu, S

    def gsm_factor_update(self, Z, X, G, mu0, F0, out=None, flag=None, n_reverts=None):
        """Factor-form update: Sigma = F^T F, X = mu0 + Z F0.  Returns (mu, F, flag); flag != 0 means
        the 2B x 2B positive-definite test failed and (mu, F) = (mu0, F0) (revert; counted in n_reverts)."""
        B, D = Z.shape
        self._ensure(D, B)
        mu, F = (self.empty(D), self.empty(D, D)) if out is None else out
        flag = self.new_flag() if flag is None else flag
        self._call("gsmvi_gsm_factor_update_f64", D, B, *self._mat(Z, "Z"), *self._mat(X, "X"), *self._mat(G, "G"),
                   self._vec(mu0, "mu0"), *self._mat(F0, "F0"), self._vec(mu, "mu"), *self._mat(F, "F"),
                   _ptr(flag), _ptr(n_reverts))
        return mu, F, flag

    def bam_factor_update(self, Z, X, G, mu0, F0, reg, out=None, flag=None, n_reverts=None):
        """Factor-form BaM update: Sigma = F^T F, X = mu0 + Z F0.  Returns (mu, F, flag); F^T F equals the S of
        ``bam_update`` (jitter 0) to round-off; flag != 0: (mu, F) = (mu0, F0) (revert; counted in n_reverts)."""
        B, D = Z.shape
        self._ensure(D, B)
        mu, F = (self.empty(D), self.empty(D, D)) if out is None else out
        flag = self.new_flag() if flag is None else flag
        self._call("gsmvi_bam_factor_update_f64", D, B, *self._mat(Z, "Z"), *self._mat(X, "X"), *self._mat(G, "G"),
                   self._vec(mu0, "mu0"), *self._mat(F0, "F0"), float(reg), self._vec(mu, "mu"), *self._mat(F, "F"),
                   _ptr(flag), _ptr(n_reverts))
        return mu, F, flag

    def gsm_factor_local_stage(self, Z_l, X_l, G_l, mu0, F0, out=None):
        """Records [x - mu0 | u | u F0] of this rank's samples (batch-sharded factor path)."""
        Bl, D = Z_l.shape
        self._ensure(D, Bl)
        rec = self.empty(Bl, self.record_len(D)) if out is None else out
        self._call("gsmvi_gsm_factor_local_stage_f64", D, Bl, *self._mat(Z_l, "Z"), *self._mat(X_l, "X"),
                   *self._mat(G_l, "G"), self._vec(mu0, "mu0"), *self._mat(F0, "F0"), *self._mat(rec, "rec"))
        return rec

    def gsm_factor_apply(self, Z, rec, mu0, F0, out=None, flag=None, n_reverts=None):
        """(mu, F, flag) from the replicated draws Z and ALL samples' records (batch-sharded factor path)."""
        B, D = Z.shape
        assert rec.shape[0] == B
        self._ensure(D, B)
        mu, F = (self.empty(D), self.empty(D, D)) if out is None else out
        flag = self.new_flag() if flag is None else flag
        self._call("gsmvi_gsm_factor_apply_f64", D, B, *self._mat(Z, "Z"), *self._mat(rec, "rec"), self._vec(mu0, "mu0"),
                   *self._mat(F0, "F0"), self._vec(mu, "mu"), *self._mat(F, "F"), _ptr(flag),
                   _ptr(n_reverts))
        return mu, F, flag

    # ---- column-sharded factor form (dist.col_sharded_gsm_factor_update) --------------------------
    def sample_cols(self, Z, mu_cols, Fcols, out=None):
        """X[:, C] = mu[C] + Z F[:, C]: the owned column slice of x = mu + z F (gsm_numpy.py:116) from the owned block of F."""
        B, D = Z.shape
        nc = Fcols.shape[1]
        assert Fcols.shape == (D, nc) and mu_cols.shape == (nc,)
        self._ensure(D, B)
        X = self.empty(B, nc) if out is None else out
        self._call("gsmvi_sample_cols_f64", D, B, nc, *self._mat(Z, "Z"), self._vec(mu_cols, "mu_cols"),
                   *self._mat(Fcols, "Fcols"), *self._mat(X, "Xcols"))
        return X

    def gsm_factor_w_partial(self, G, col0, Fcols, out=None):
        """The rank's PARTIAL sum of W = G F^T over its owned columns: G[:, C] F[:, C]^T (B x D) -- gsmvi_gsm_rows_stage_f64 on the
        block (the caller all-reduces the partials)."""
        nc = Fcols.shape[1]
        self._ensure(Fcols.shape[0], G.shape[0])         # (the product's output is D wide: the context must be sized for D, not for the block)
        return self.gsm_rows_stage(G[:, col0:col0 + nc], Fcols, out=out)

    def gsm_factor_apply_cols(self, Z, W, X, mu0, F0cols, col0, out=None, flag=None, n_reverts=None):
        """(mu, Fcols, flag): the factor-form update of the OWNED column block from the replicated draws Z, the all-reduced
        W = G F^T and the gathered samples X; mu is full length, entries C written (gsmvi_gsm_factor_apply_cols_f64)."""
        B, D = Z.shape
        nc = F0cols.shape[1]
        assert W.shape == (B, D) and W.is_contiguous() and X.shape == (B, D) and F0cols.shape == (D, nc)
        self._ensure(D, B)
        mu, F = (self.empty(D), self.empty(D, nc)) if out is None else out
        flag = self.new_flag() if flag is None else flag
        self._call("gsmvi_gsm_factor_apply_cols_f64", D, B, int(col0), nc, *self._mat(Z, "Z"), _ptr(W),
                   *self._mat(X, "X"), self._vec(mu0, "mu0"), *self._mat(F0cols, "F0cols"), self._vec(mu, "mu"),
                   *self._mat(F, "Fcols"), _ptr(flag), _ptr(n_reverts))
        return mu, F, flag

    def bam_factor_wq_partial(self, G, col0, F0cols, reg, out=None):
        """The rank's PARTIAL sum of Wq = Qt F0^T over its owned columns: Qt[:, C] F0[:, C]^T (B x D), Qt the Helmert / gbar rows
        of G (gsmvi_bam_factor_wq_partial_f64; the caller all-reduces the partials, dist.col_sharded_bam_factor_update)."""
        B, D = G.shape
        nc = F0cols.shape[1]
        assert F0cols.shape == (D, nc)
        self._ensure(D, B)                         # (the product's output is D wide: sized for (D, B), not for the block)
        Wq = self.empty(B, D) if out is None else out
        assert Wq.shape == (B, D) and Wq.is_contiguous()
        self._call("gsmvi_bam_factor_wq_partial_f64", D, B, int(col0), nc, *self._mat(G, "G"), *self._mat(F0cols, "F0cols"),
                   float(reg), _ptr(Wq))
        return Wq

    def bam_factor_apply_cols(self, Z, X, G, Wq, mu0, F0cols, col0, reg, out=None, flag=None, n_reverts=None):
        """(mu, Fcols, flag): the factor-form BaM update of the OWNED column block from the replicated draws Z, the gathered
        samples X, the scores G and the all-reduced Wq; mu is full length, entries C written (gsmvi_bam_factor_apply_cols_f64)."""
        B, D = Z.shape
        nc = F0cols.shape[1]
        assert Wq.shape == (B, D) and Wq.is_contiguous() and X.shape == (B, D) and G.shape == (B, D) and F0cols.shape == (D, nc)
        self._ensure(D, B)
        mu, F = (self.empty(D), self.empty(D, nc)) if out is None else out
        flag = self.new_flag() if flag is None else flag
        self._call("gsmvi_bam_factor_apply_cols_f64", D, B, int(col0), nc, *self._mat(Z, "Z"), *self._mat(X, "X"),
                   *self._mat(G, "G"), _ptr(Wq), self._vec(mu0, "mu0"), *self._mat(F0cols, "F0cols"),
                   float(reg), self._vec(mu, "mu"), *self._mat(F, "Fcols"), _ptr(flag), _ptr(n_reverts))
        return mu, F, flag

    def gram(self, F, out=None, shift=0.0, shift_dev=None):
        """cov = F^T F (gsmvi_gram_f64): the covariance a square factor represents -- return value of the
        factor-form fit and what its monitor sees (gsm_numpy.py:129).  Not on the per-iteration path.
        ``shift`` / ``shift_dev`` (a 1-element float64 device tensor): cov = F^T F + (shift + shift_dev) I
        (gsmvi_gram_shift_f64) -- the jitter a factor-form BaM fit owes (bam.py:198)."""
        D = F.shape[0]
        assert F.shape == (D, D)
        self._ensure(D, max(self._max_B, 1))
        Cm = self.empty(D, D) if out is None else out
        if shift == 0.0 and shift_dev is None:
            self._call("gsmvi_gram_f64", D, *self._mat(F, "F"), *self._mat(Cm, "C"))
        else:
            self._call("gsmvi_gram_shift_f64", D, *self._mat(F, "F"), float(shift), _ptr(shift_dev), *self._mat(Cm, "C"))
        return Cm

    def owed_shift(self, jitter, pend, n_rev, mark, advance=True):
        """The diagonal shift a factor-form BaM fit owes its covariance: jitter * (accepted updates since the last absorption)
        as a 1-element device tensor, without a host synchronisation.  ``pend`` = updates ATTEMPTED since then (host count),
        ``n_rev`` = the device counter of reverts, ``mark`` = its value at the last absorption (a device int32 word, advanced
        to ``n_rev`` when ``advance``): a reverted update adds no jitter in the reference (bam.py:198 sits before the accept
        test, :208-212 discards the shifted matrix with the update)."""
        s = (float(pend) - (n_rev - mark).to(torch.float64)) * float(jitter)
        if advance:
            mark.copy_(n_rev)
        return s

    def whiten_rows(self, X, mu, R):
        """(Z, logdiag): Z = (X - mu) R^-1 for the rows of X and logdiag = sum_i log R_ii (a 1-element device
        tensor); log N(x_b; mu, R^T R) = -|z_b|^2/2 - logdiag - D/2 log(2 pi)   [gsmvi/monitors.py:107]."""
        n, D = X.shape
        self._ensure(D, max(self._max_B, 1))
        Z = self.empty(n, D)
        ld = self.empty(1)
        self._call("gsmvi_whiten_rows_f64", D, n, *self._mat(R, "R"), *self._mat(X, "X"),
                   self._vec(mu, "mu") if mu is not None else None, *self._mat(Z, "Z"), _ptr(ld))
        return Z, ld

    # kernel-family bits of include/gsmvi_hip.h (GSMVI_PATH_*)
    PATH_BITS = {"panel_fast": 0x1, "panel_wide": 0x2, "panel_generic": 0x4, "panel_t_fast": 0x8, "panel_t_generic": 0x10,
                 "scalars_fast": 0x20, "scalars_generic": 0x40, "cov_sym": 0x80, "cov_generic": 0x100, "fupd_fast": 0x200,
                 "fupd_generic": 0x400, "lowrank_fast": 0x800, "lowrank_generic": 0x1000, "batched": 0x2000,
                 "batched_bam": 0x4000, "batched_kl": 0x8000, "batched_advi": 0x10000, "batched_target": 0x20000,
                 "batched_lbfgs": 0x40000, "batched_laplace": 0x80000, "batched_predict": 0x100000,
                 "batched_psis": 0x200000, "batched_loo": 0x400000, "gsm_two_launch": 0x800000,
                 "batched_softmax": 0x1000000, "panel_chunk512": 0x2000000, "batched_pathfinder": 0x4000000,
                 "cov_fold_diag": 0x8000000, "batched_softmax_laplace": 0x10000000, "cov_s0_last": 0x20000000,
                 "cov_store_wt": 0x40000000, "panel_qm_whole": 0x80000000}
    PATH_GENERIC_MASK = 0x4 | 0x10 | 0x40 | 0x100 | 0x400 | 0x1000

    def last_path(self, reset=True):
        """Names of the kernel families launched on this context since the last reset (gsmvi_last_path): how tests and
        profiles check that an off-grid shape stayed on the tuned kernels (no name ending in ``_generic``)."""
        self._any_ctx()
        bits = C.c_uint(0)
        self._call_ctx("gsmvi_last_path", C.byref(bits), int(bool(reset)))
        return {k for k, v in self.PATH_BITS.items() if bits.value & v}

    def bam_reg_source(self, word):
        """gsmvi_bam_set_reg_source: ``word`` (a 1-element float64 device tensor) makes every BaM update launched from now on
        read its regulariser from that word when its kernels EXECUTE (a captured graph can then be replayed with another
        value; the ``reg`` argument is ignored); ``None`` restores the by-value argument."""
        self._any_ctx()
        self._reg_word = word
        self._call_ctx("gsmvi_bam_set_reg_source", _ptr(word))

    def set_profiling(self, on):
        self._any_ctx()
        self._call_ctx("gsmvi_set_profiling", int(bool(on)))

    def get_profile(self):
        """Kernel durations (ms) of the last profiled update: panel, scalars, cov_update (-1: that launch did not run, as
        ``scalars`` in the two-launch form of the dense update)."""
        ms = (C.c_float * 3)()
        self._call_ctx("gsmvi_get_profile", ms, 3)
        return {"panel": ms[0], "scalars": ms[1], "cov_update": ms[2]}

    def gaussian_score(self, X, m, P, out=None):
        """G = -(X - m) P   [examples/example_gsm_numpy.py:24-29]."""
        B, D = X.shape
        self._ensure(D, B)
        G = self.empty(B, D) if out is None else out
        self._call("gsmvi_gaussian_score_f64", D, B, *self._mat(X, "X"), self._vec(m, "m"), *self._mat(P, "P"),
                   *self._mat(G, "G"))
        return G

    def potrf(self, S, out=None, flag=None):
        """Upper Cholesky factor R (R^T R = S) and a device flag (0 = positive definite)."""
        D = S.shape[0]
        self._ensure(D, max(self._max_B, 1))
        R = self.empty(D, D) if out is None else out
        flag = self.new_flag() if flag is None else flag
        self._call("gsmvi_potrf_f64", D, *self._mat(S, "S"), *self._mat(R, "R"), _ptr(flag))
        return R, flag

    def sample(self, Z, mu, R, out=None):
        """X = mu + Z R   [replaces np.random.multivariate_normal, gsmvi/gsm_numpy.py:116]."""
        B, D = Z.shape
        self._ensure(D, B)
        X = self.empty(B, D) if out is None else out
        self._call("gsmvi_sample_f64", D, B, *self._mat(Z, "Z"), self._vec(mu, "mu"), *self._mat(R, "R"), *self._mat(X, "X"))
        return X

    def commit(self, flag, mu_new, S_new, mu, S, n_reverts=None):
        """In place: (mu, S) <- (mu_new, S_new) iff flag == 0   [gsmvi/gsm_numpy.py:121-125]."""
        D = mu.shape[0]
        self._ensure(D, max(self._max_B, 1))
        self._call("gsmvi_commit_f64", D, _ptr(flag), self._vec(mu_new, "mu_new"),
                   *self._mat(S_new, "S_new"), self._vec(mu, "mu"), *self._mat(S, "S"), _ptr(n_reverts))

    # ---- batched GSM: K independent problems of one (D, B) (csrc/gsmvi_batched.hip) -------------------------------------
    batched_max_D = 64         # one problem per workgroup slot, held in LDS from its first read to its last write
    batched_max_B = 32

    @staticmethod
    def _packed(t, shape, name):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous(), \
            f"{name}: expected a contiguous float64 CUDA tensor"
        assert tuple(t.shape) == tuple(shape), f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}"
        return _ptr(t)

    @staticmethod
    def _ints(t, K, name):
        if t is None:
            return None
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == K, \
            f"{name}: expected a contiguous int32 CUDA tensor of {K} entries"
        return _ptr(t)

    def eye_batch(self, K, D):
        return torch.eye(D, dtype=torch.float64, device=self.device).expand(K, D, D).contiguous()

    def batched_ints(self, K):
        """K device int32 zeros: per-problem flags and revert counters"""
        return torch.zeros(K, dtype=torch.int32, device=self.device)

    def read_ints(self, t):
        return t.cpu().numpy().astype(np.int64)          # synchronises

    def batched_counts(self, values):
        """K per-problem counts as a device int32 tensor"""
        return torch.as_tensor(np.asarray(values, dtype=np.int32).reshape(-1), device=self.device)

    def batched_seeds(self, seeds):
        """the problems' draw keys as a device uint64 array (stored as int64: the same bits)"""
        return torch.tensor(np.array([int(s) & (2 ** 64 - 1) for s in seeds], dtype=np.uint64).view(np.int64),
                            device=self.device)

    def gsm_update_batched(self, X, G, mu0, S0, out=None):
        """(mu_k, S_k) = gsm_update(X_k, G_k, mu0_k, S0_k) for every k  [gsmvi/gsm_numpy.py:27-55 under jax.vmap]; reads all
        of each S0_k."""
        K, B, D = X.shape
        self._any_ctx()
        mu, S = (self.empty(K, D), self.empty(K, D, D)) if out is None else out
        self._call("gsmvi_gsm_update_batched_f64", K, D, B, self._packed(X, (K, B, D), "samples"),
                   self._packed(G, (K, B, D), "vs"), self._packed(mu0, (K, D), "mu0"), self._packed(S0, (K, D, D), "S0"),
                   self._packed(mu, (K, D), "mu"), self._packed(S, (K, D, D), "S"))
        return mu, S

    def gsm_fit_init_batched(self, mean, cov, R, info, seeds=None, X=None):
        """R_k = chol(cov_k) (upper), info[k] = 0 or 1 + the first bad pivot; with ``seeds``: X_k = mean_k + Z_k R_k, Z_k = draw 0
        of the problem's stream"""
        K, D = mean.shape
        B = X.shape[1] if X is not None else 1
        self._any_ctx()
        self._call("gsmvi_gsm_fit_init_batched_f64", K, D, B, self._packed(mean, (K, D), "mean"),
                   self._packed(cov, (K, D, D), "cov"), self._packed(R, (K, D, D), "R"), self._ints(info, K, "info"),
                   _ptr(seeds), self._dp(X, (K, B, D), "X"))

    def gsm_fit_step_batched(self, X, G, mean, cov, R=None, info=None, n_reverts=None, seeds=None, call=0):
        """One batched fit iteration after the score (csrc/gsmvi_batched.hip): update, Cholesky test and accept / revert of
        (mean, cov, R) per problem; with ``seeds`` X is overwritten with the samples of draw ``call``."""
        K, B, D = X.shape
        self._any_ctx()
        self._call("gsmvi_gsm_fit_step_batched_f64", K, D, B, self._packed(X, (K, B, D), "X"),
                   self._packed(G, (K, B, D), "G"), self._packed(mean, (K, D), "mean"), self._packed(cov, (K, D, D), "cov"),
                   self._dp(R, (K, D, D), "R"), self._ints(info, K, "info"), self._ints(n_reverts, K, "n_reverts"),
                   _ptr(seeds), int(call))

    def gaussian_score_batched(self, X, m, P, out=None):
        """G_k = -(X_k - m_k) P_k for K Gaussian targets  [examples/example_gsm_numpy.py:24-29]."""
        K, B, D = X.shape
        self._any_ctx()
        G = self.empty(K, B, D) if out is None else out
        self._call("gsmvi_gaussian_score_batched_f64", K, D, B, self._packed(X, (K, B, D), "X"),
                   self._packed(m, (K, D), "m"), self._packed(P, (K, D, D), "P"), self._packed(G, (K, B, D), "G"))
        return G

    # ---- batched BaM: K independent problems of one (D, B) (csrc/gsmvi_bam_batched.hip) -----------------------------------
    def _reg_arg(self, reg, K):
        """(scalar, device pointer) of a regulariser: a number -> (reg, NULL); a (K,) float64 CUDA tensor -> (0, its data)"""
        if isinstance(reg, torch.Tensor):
            assert reg.is_cuda and reg.dtype == torch.float64 and reg.is_contiguous() and reg.numel() == K, \
                f"reg: expected a contiguous float64 CUDA tensor of {K} entries"
            return 0.0, _ptr(reg)
        return float(reg), None

    def batched_regs(self, values):
        """K per-problem regularisers as a device float64 tensor"""
        return torch.as_tensor(np.asarray(values, dtype=np.float64).reshape(-1), device=self.device)

    def bam_update_batched(self, X, G, mu0, S0, reg, jitter=0.0, out=None, info=None):
        """(mu_k, S_k) = bam_update(X_k, G_k, mu0_k, S0_k, reg_k) for every k  [gsmvi/bam.py:72-114 under jax.vmap]; S_k
        symmetrised, jitter on its diagonal; ``reg`` a number or a (K,) device tensor; info[k] != 0: problem k's chain failed
        (its outputs are NaN)."""
        K, B, D = X.shape
        self._any_ctx()
        mu, S = (self.empty(K, D), self.empty(K, D, D)) if out is None else out
        r, rp = self._reg_arg(reg, K)
        self._call("gsmvi_bam_update_batched_f64", K, D, B, self._packed(X, (K, B, D), "samples"),
                   self._packed(G, (K, B, D), "vs"), self._packed(mu0, (K, D), "mu0"), self._packed(S0, (K, D, D), "S0"), r,
                   rp, float(jitter), self._packed(mu, (K, D), "mu"), self._packed(S, (K, D, D), "S"),
                   self._ints(info, K, "info"))
        return mu, S

    def bam_fit_step_batched(self, X, G, mean, cov, R=None, reg=1.0, jitter=0.0, info=None, n_reverts=None, seeds=None,
                             call=0):
        """One batched BaM fit iteration after the score (csrc/gsmvi_bam_batched.hip): update + jitter I, Cholesky test and
        accept / revert of (mean, cov, R) per problem; with ``seeds`` X is overwritten with the samples of draw ``call``."""
        K, B, D = X.shape
        self._any_ctx()
        r, rp = self._reg_arg(reg, K)
        px = self._packed(X, (K, B, D), "X")
        self._call("gsmvi_bam_fit_step_batched_f64", K, D, B, px, self._packed(G, (K, B, D), "G"),
                   self._packed(mean, (K, D), "mean"), self._packed(cov, (K, D, D), "cov"), self._dp(R, (K, D, D), "R"), r,
                   rp, float(jitter), self._ints(info, K, "info"), self._ints(n_reverts, K, "n_reverts"), _ptr(seeds),
                   int(call), px if seeds is not None else None)

    # ---- batched KL monitor: K Gaussians of one D (csrc/gsmvi_kl_batched.hip) ----------------------------------------------
    def kl_draw_batched(self, mean, cov, seeds, call, s0, nc, out=None, info=None):
        """Rows s0 .. s0 + nc - 1 of draw ``call`` of every problem's q_k = N(mean_k, cov_k)  [gsmvi/monitors.py:101-103]:
        X_k = mean_k + Z_k R_k with Z_k those rows of ``normal(n, D, seeds[k], call)``; returns (X (K, nc, D), logq (K,) = the
        sum of log q_k over the rows [monitors.py:104-113], info (K,) int32: 0, or 1 + the first bad pivot of cov_k, whose X
        rows and logq are NaN)."""
        K, D = mean.shape
        self._any_ctx()
        mean, cov = mean.contiguous(), cov.contiguous()
        X, logq = (self.empty(K, nc, D), self.empty(K)) if out is None else out
        info = self.batched_ints(K) if info is None else info
        assert isinstance(seeds, torch.Tensor) and seeds.is_cuda and seeds.dtype == torch.int64 and seeds.is_contiguous() \
            and seeds.numel() == K, f"seeds: expected {K} keys from batched_seeds()"
        self._call("gsmvi_kl_draw_batched_f64", K, D, int(nc), int(s0), self._packed(mean, (K, D), "mean"),
                   self._packed(cov, (K, D, D), "cov"), _ptr(seeds), int(call),
                   self._packed(X, (K, nc, D), "X"), self._packed(logq, (K,), "logq"), self._ints(info, K, "info"))
        return X, logq, info

    def take_rows(self, A, idx):
        """(K, len(idx), D): the rows ``idx`` of every problem's block of A (K, N, D), packed (the forward-KL batch)"""
        return torch.index_select(A, 1, torch.as_tensor(np.asarray(idx, dtype=np.int64), device=A.device)).contiguous()

    def logq_batched(self, mean, cov, Y, out=None, info=None):
        """(logq (K,), info (K,)): logq_k = sum over the rows of Y_k (K, nc, D) of log N(y; mean_k, cov_k)
        [gsmvi/monitors.py:104-113], by forward substitution with the upper factor of cov_k; NaN where cov_k is not positive
        definite (info[k] = 1 + the first bad pivot)."""
        K, nc, D = Y.shape
        self._any_ctx()
        mean, cov, Y = mean.contiguous(), cov.contiguous(), Y.contiguous()
        logq = self.empty(K) if out is None else out
        info = self.batched_ints(K) if info is None else info
        self._call("gsmvi_logq_batched_f64", K, D, nc, self._packed(mean, (K, D), "mean"),
                   self._packed(cov, (K, D, D), "cov"), self._packed(Y, (K, nc, D), "Y"), self._packed(logq, (K,), "logq"),
                   self._ints(info, K, "info"))
        return logq, info

    # ---- batched ADVI: K full-rank ELBO fits of one (D, B) (csrc/gsmvi_advi_batched.hip) ----------------------------------
    @staticmethod
    def _dp(t, shape, name):
        return HipEngine._packed(t, shape, name) if t is not None else None

    def advi_init_batched(self, mean, cov, scales, info, seeds=None, Z=None, X=None, logq=None):
        """scales_k = packed lower Cholesky factor of cov_k (np.tril_indices order), info[k] = 0 or 1 + the first bad pivot; with
        ``seeds`` (draw 0) or ``Z`` (given normals): X_k = mean_k + Z_k L_k^T and logq[k] = sum_b log q_k(x_kb)
        [gsmvi/advi.py:80-86]"""
        K, D = mean.shape
        B = X.shape[1] if X is not None else 1
        P = D * (D + 1) // 2
        self._any_ctx()
        self._call("gsmvi_advi_init_batched_f64", K, D, B, self._packed(mean, (K, D), "mean"),
                   self._packed(cov, (K, D, D), "cov"), self._packed(scales, (K, P), "scales"), self._ints(info, K, "info"),
                   _ptr(seeds), self._dp(Z, (K, B, D), "Z"), self._dp(X, (K, B, D), "X"), self._dp(logq, (K,), "logq"))

    def advi_step_batched(self, G, loc, scales, moments, t, lr, b1=0.9, b2=0.999, eps=1e-8, seeds=None, call=0, Zcur=None,
                          Znext=None, Xout=None, logq=None):
        """One batched ADVI iteration after the score (csrc/gsmvi_advi_batched.hip): the closed-form ELBO gradient and Adam step
        ``t`` on (loc, scales) and ``moments`` = (m_loc, v_loc, m_s, v_s), all in place [gsmvi/advi.py:31-45,69-73]; ``lr`` a
        number or a (K,) device tensor; with ``Xout`` the next samples and their ``logq`` from the updated state (z = draw
        ``call`` of ``seeds``, or ``Znext``; the z behind G is draw ``call`` - 1, or ``Zcur``)."""
        K, B, D = G.shape
        P = D * (D + 1) // 2
        self._any_ctx()
        m_loc, v_loc, m_s, v_s = moments
        r, rp = self._reg_arg(lr, K)
        self._call("gsmvi_advi_step_batched_f64", K, D, B, self._packed(G, (K, B, D), "G"), self._packed(loc, (K, D), "loc"),
                   self._packed(scales, (K, P), "scales"), self._packed(m_loc, (K, D), "m_loc"),
                   self._packed(v_loc, (K, D), "v_loc"), self._packed(m_s, (K, P), "m_s"), self._packed(v_s, (K, P), "v_s"),
                   int(t), r, rp, float(b1), float(b2), float(eps), _ptr(seeds), int(call),
                   self._dp(Zcur, (K, B, D), "Zcur"), self._dp(Znext, (K, B, D), "Znext"), self._dp(Xout, (K, B, D), "Xout"),
                   self._dp(logq, (K,), "logq"))

    def advi_cov_batched(self, scales, D, out=None):
        """cov_k = L_k L_k^T (K, D, D), exactly symmetric, from the packed factors (K, D (D + 1) / 2)  [gsmvi/advi.py:25-29]"""
        K = scales.shape[0]
        self._any_ctx()
        cov = self.empty(K, D, D) if out is None else out
        self._call("gsmvi_advi_cov_batched_f64", K, D, self._packed(scales, (K, D * (D + 1) // 2), "scales"),
                   self._packed(cov, (K, D, D), "cov"))
        return cov

    # ---- batched logistic target: K regressions of one (N, D) (csrc/gsmvi_logistic_batched.hip) ---------------------------
    @staticmethod
    def _check_want(want, a, b):
        """``want`` of the entries with two outputs: one of them or "both", else ValueError"""
        if want not in (a, b, "both"):
            raise ValueError(f"want = {want!r}: expected {a!r}, {b!r} or 'both'")

    def _want_g_lp(self, want, X, out, lp_out):
        """The ``want`` protocol of the target launches at the rows of X (K, nc, D): checks ``want``; returns G (K, nc, D)
        (``out`` when given; None for "lp"), lp (K, nc) (``lp_out`` when given; None for "g") and what the method returns"""
        self._check_want(want, "g", "lp")
        K, nc, D = X.shape
        G = lp = None
        if want != "lp":
            G = self.empty(K, nc, D) if out is None else out
        if want != "g":
            lp = self.empty(K, nc) if lp_out is None else lp_out
        return G, lp, (G if want == "g" else lp if want == "lp" else (G, lp))

    def logistic_batched(self, X, A, y, counts=None, prior_prec=1.0, out=None, lp_out=None, want="g"):
        """Score and / or log-density of K Bayesian logistic regressions at the rows of X (K, nc, D), one launch
        [examples/example_gsm.py:34-35 for this model]: A (K, N, D), y (K, N), ``counts`` None or K device int32 valid rows,
        ``prior_prec`` a number or a (K,) device tensor.  ``want`` = "g" -> G (K, nc, D) (no logarithm is evaluated), "lp" -> the
        values (K, nc), "both" -> (G, lp)."""
        G, lp, ret = self._want_g_lp(want, X, out, lp_out)
        X = X.contiguous()
        K, nc, D = X.shape
        N = A.shape[1]
        self._any_ctx()
        r, rp = self._reg_arg(prior_prec, K)
        self._call("gsmvi_logistic_batched_f64", K, D, nc, N, self._packed(A, (K, N, D), "A"), self._packed(y, (K, N), "y"),
                   self._ints(counts, K, "counts"), r, rp, self._packed(X, (K, nc, D), "X"), self._dp(G, (K, nc, D), "out"),
                   self._dp(lp, (K, nc), "lp_out"))
        return ret

    # ---- batched softmax target: K multinomial logit regressions of one (N, C, P) (csrc/gsmvi_softmax_batched.hip) ----------
    def _softmax_model_args(self, K, D, A, labels, num_classes, counts, prior_prec=None, prefix=""):
        """The model of the five softmax entry points, checked against the K problems and D columns of the caller's points or
        draws: the sizes (C, P, N) and the arrays A, labels, counts_dev and -- with ``prior_prec``, which the leave-one-out and the predictive
        do not have -- the prior's two arguments, each in the order of include/gsmvi_hip.h.  ``labels`` None (the predictive
        without them) passes NULL; ``prefix`` names the checked array in the message."""
        N, P, Cc = A.shape[1], A.shape[2], int(num_classes)
        if Cc < 2 or (Cc - 1) * P != D:
            raise ValueError(f"{prefix}expected (num_classes - 1) P = {(Cc - 1) * P} columns, got {D}")
        if labels is not None:
            assert labels.is_cuda and labels.dtype == torch.int32 and labels.is_contiguous() and tuple(labels.shape) == (K, N), \
                f"labels: expected a contiguous int32 CUDA tensor of shape {(K, N)}"
        model = (self._packed(A, (K, N, P), "A"), _ptr(labels) if labels is not None else None, self._ints(counts, K, "counts"))
        return (Cc, P, N), model + (self._reg_arg(prior_prec, K) if prior_prec is not None else ())

    def softmax_batched(self, X, A, labels, num_classes, counts=None, prior_prec=1.0, out=None, lp_out=None, want="g"):
        """Score and / or log-density of K Bayesian multinomial logit regressions at the rows of X (K, nc, D), D = (C - 1) P,
        class-major, class C - 1 the reference class, one launch [examples/example_gsm.py:34-35 for this model]: A (K, N, P),
        ``labels`` (K, N) device int32 in 0 .. C - 1, ``num_classes`` = C, ``counts`` None or K device int32 valid rows,
        ``prior_prec`` a number or a (K,) device tensor.  ``want`` = "g" -> G (K, nc, D) (no logarithm is evaluated), "lp" -> the
        values (K, nc), "both" -> (G, lp)."""
        G, lp, ret = self._want_g_lp(want, X, out, lp_out)
        X = X.contiguous()
        K, nc, D = X.shape
        (Cc, P, N), model = self._softmax_model_args(K, D, A, labels, num_classes, counts, prior_prec, prefix="X: ")
        self._any_ctx()
        self._call("gsmvi_softmax_batched_f64", K, Cc, P, nc, N, *model, self._packed(X, (K, nc, D), "X"),
                   self._dp(G, (K, nc, D), "out"), self._dp(lp, (K, nc), "lp_out"))
        return ret

    def batched_labels(self, values):
        """(K, N) integer labels as a device int32 tensor"""
        return torch.as_tensor(np.ascontiguousarray(values, dtype=np.int32), device=self.device)

    # ---- batched GLM targets: the same launch for a family of links (csrc/gsmvi_logistic_batched.hip) -----------------------
    GLM_FAMILIES = {"logistic": 0, "poisson": 1, "probit": 2, "gaussian": 3}     # GSMVI_GLM_* of include/gsmvi_hip.h

    def _glm_family_args(self, family, noise_prec, K):
        """(GSMVI_GLM_* code, noise_prec, noise_prec_dev) of every GLM entry point; an unknown family: ValueError"""
        if family not in self.GLM_FAMILIES:
            raise ValueError(f"family = {family!r}: expected one of {sorted(self.GLM_FAMILIES)}")
        t, tp = self._reg_arg(noise_prec, K)
        return self.GLM_FAMILIES[family], 1.0 if tp is not None else t, tp     # (the scalar is unused with K values)

    def glm_batched(self, X, A, y, family, offset=None, counts=None, prior_prec=1.0, noise_prec=1.0, out=None, lp_out=None,
                    want="g"):
        """Score and / or log-density of K generalised linear models at the rows of X (K, nc, D), one launch
        [examples/example_gsm.py:34-35 for these models]: ``family`` "logistic", "poisson" (log link), "probit" or "gaussian"
        (identity link, noise precision ``noise_prec``: a number or a (K,) device tensor, this family only); A (K, N, D), y
        (K, N), ``offset`` None or (K, N) added to A x, ``counts`` None or K device int32 valid rows, ``prior_prec`` a number or
        a (K,) device tensor.  ``want`` = "g" -> G (K, nc, D), "lp" -> the values (K, nc), "both" -> (G, lp)."""
        G, lp, ret = self._want_g_lp(want, X, out, lp_out)
        fam, t, tp = self._glm_family_args(family, noise_prec, X.shape[0])
        X = X.contiguous()
        K, nc, D = X.shape
        N = A.shape[1]
        self._any_ctx()
        r, rp = self._reg_arg(prior_prec, K)
        self._call("gsmvi_glm_batched_f64", K, D, nc, N, fam, self._packed(A, (K, N, D), "A"), self._packed(y, (K, N), "y"),
                   self._dp(offset, (K, N), "offset"), self._ints(counts, K, "counts"), t, tp, r, rp,
                   self._packed(X, (K, nc, D), "X"), self._dp(G, (K, nc, D), "out"), self._dp(lp, (K, nc), "lp_out"))
        return ret

    # ---- batched negative binomial target: K count regressions with a fitted size (csrc/gsmvi_negbin_batched.hip) -------------
    def negbin_batched(self, X, A, y, offset=None, counts=None, prior_prec=1.0, log_size_mean=0.0, log_size_prec=1.0, out=None,
                       lp_out=None, want="g"):
        """Score and / or log-density of K negative binomial regressions at the rows of X (K, nc, P + 1) = (beta, theta), theta =
        log of the size, one launch [examples/example_gsm.py:34-35 for this model]: A (K, N, P), y (K, N) >= 0, ``offset`` None or
        (K, N) added to A beta, ``counts`` None or K device int32 valid rows; ``prior_prec`` (of beta), ``log_size_mean`` and
        ``log_size_prec`` (the prior N(mean, 1 / prec) of theta) each a number or a (K,) device tensor.  ``want`` = "g" -> G
        (K, nc, P + 1), "lp" -> the values (K, nc), "both" -> (G, lp)."""
        N, P = A.shape[1], A.shape[2]
        if X.shape[2] != P + 1:
            raise ValueError(f"X: expected P + 1 = {P + 1} columns (beta, then the log size), got {X.shape[2]}")
        G, lp, ret = self._want_g_lp(want, X, out, lp_out)
        X = X.contiguous()
        K, nc, D = X.shape
        self._any_ctx()
        r, rp = self._reg_arg(prior_prec, K)
        m, mp = self._reg_arg(log_size_mean, K)
        s, sp = self._reg_arg(log_size_prec, K)
        self._call("gsmvi_negbin_batched_f64", K, P, nc, N, self._packed(A, (K, N, P), "A"), self._packed(y, (K, N), "y"),
                   self._dp(offset, (K, N), "offset"), self._ints(counts, K, "counts"), m, mp, s, sp, r, rp,
                   self._packed(X, (K, nc, D), "X"), self._dp(G, (K, nc, D), "out"), self._dp(lp, (K, nc), "lp_out"))
        return ret

    # ---- batched ordinal target: K cumulative-logit regressions of C ordered classes (csrc/gsmvi_ordinal_batched.hip) -----------
    def ordinal_batched(self, X, A, y, C, offset=None, counts=None, prior_prec=1.0, cut_prec=1.0, out=None, lp_out=None, want="g"):
        """Score and / or log-density of K cumulative-logit (proportional odds) regressions at the rows of X (K, nc, P + C - 1) =
        (beta, delta), cut_0 = delta_0 and cut_j = cut_{j-1} + exp(delta_j), one launch [examples/example_gsm.py:34-35 for this
        model]: A (K, N, P) without an intercept column, ``y`` (K, N) device int32 labels in 0 .. C - 1, ``C`` the number of
        classes, ``offset`` None or (K, N) added to A beta, ``counts`` None or K device int32 valid rows; ``prior_prec`` (of beta)
        and ``cut_prec`` (of delta) each a number or a (K,) device tensor.  ``want`` = "g" -> G (K, nc, P + C - 1), "lp" -> the
        values (K, nc), "both" -> (G, lp)."""
        N, P, Cc = A.shape[1], A.shape[2], int(C)
        if Cc < 2:
            raise ValueError(f"C: expected at least 2 classes, got {Cc}")
        if X.shape[2] != P + Cc - 1:
            raise ValueError(f"X: expected P + C - 1 = {P + Cc - 1} columns (beta, then the C - 1 cutpoint parameters), got {X.shape[2]}")
        G, lp, ret = self._want_g_lp(want, X, out, lp_out)
        X = X.contiguous()
        K, nc, D = X.shape
        assert y.is_cuda and y.dtype == torch.int32 and y.is_contiguous() and tuple(y.shape) == (K, N), \
            f"y: expected a contiguous int32 CUDA tensor of shape {(K, N)}"
        self._any_ctx()
        r, rp = self._reg_arg(prior_prec, K)
        c, cp = self._reg_arg(cut_prec, K)
        self._call("gsmvi_ordinal_batched_f64", K, P, Cc, nc, N, self._packed(A, (K, N, P), "A"), _ptr(y),
                   self._dp(offset, (K, N), "offset"), self._ints(counts, K, "counts"), r, rp, c, cp,
                   self._packed(X, (K, nc, D), "X"), self._dp(G, (K, nc, D), "out"), self._dp(lp, (K, nc), "lp_out"))
        return ret

    # ---- shared-design GLM target: K problems on one design matrix (csrc/gsmvi_glm_shared_batched.hip) -----------------------
    def glm_shared_batched(self, X, A, y, family, offset=None, weights=None, prior_prec=1.0, noise_prec=1.0, out=None,
                           lp_out=None, want="g"):
        """Score and / or log-density of K generalised linear models that share ONE design matrix, at the rows of X (K, nc, D),
        one launch on the fp64 MFMA [examples/example_gsm.py:34-35 for these models]: ``family`` and the precisions as in
        ``glm_batched``; A (N, D) shared, y (K, N), ``offset`` None or (K, N) added to A x, ``weights`` None or (K, N)
        observation weights >= 0 (a weight of 0 removes the observation whatever it holds).  ``want`` = "g" -> G (K, nc, D),
        "lp" -> the values (K, nc), "both" -> (G, lp)."""
        G, lp, ret = self._want_g_lp(want, X, out, lp_out)
        fam, t, tp = self._glm_family_args(family, noise_prec, X.shape[0])
        X = X.contiguous()
        K, nc, D = X.shape
        N = A.shape[0]
        self._any_ctx()
        r, rp = self._reg_arg(prior_prec, K)
        self._call("gsmvi_glm_shared_batched_f64", K, D, nc, N, fam, self._packed(A, (N, D), "A"), self._packed(y, (K, N), "y"),
                   self._dp(offset, (K, N), "offset"), self._dp(weights, (K, N), "weights"), t, tp, r, rp,
                   self._packed(X, (K, nc, D), "X"), self._dp(G, (K, nc, D), "out"), self._dp(lp, (K, nc), "lp_out"))
        return ret

    # ---- batched L-BFGS initialiser: K minimisations of one D (csrc/gsmvi_lbfgs_batched.hip) --------------------------------
    def lbfgs_state_batched(self, x0):
        """The state of K L-BFGS runs started at the rows of x0 (K, D), as include/gsmvi_hip.h lays it out: a dict of device
        arrays x, g, d, Xt (K, D), S, Y (K, 10, D), sc (K, 24), ist (K, 8) int32 and the one-element counter ``stopped``"""
        K, D = x0.shape
        x = self.asarray(x0).clone(memory_format=torch.contiguous_format)
        return {"x": x, "g": self.zeros(K, D), "d": self.zeros(K, D), "Xt": x.clone(), "S": self.zeros(K, 10, D),
                "Y": self.zeros(K, 10, D), "sc": self.zeros(K, 24), "ist": torch.zeros(K, 8, dtype=torch.int32, device=self.device),
                "stopped": self.new_flag()}

    @staticmethod
    def _ist(state, K):
        """the int32 words ``ist`` (K, 8) of an L-BFGS or Laplace state, checked, as a raw pointer"""
        ist = state["ist"]
        assert isinstance(ist, torch.Tensor) and ist.is_cuda and ist.dtype == torch.int32 and ist.is_contiguous() \
            and tuple(ist.shape) == (K, 8), f"ist: expected a contiguous int32 CUDA tensor of shape {(K, 8)}"
        return _ptr(ist)

    def lbfgs_step_batched(self, fv, gv, state, start=False, sign=-1.0, maxiter=1000, maxfun=1000, gtol=1e-5,
                           ftol=2.220446049250313e-09):
        """One launch of the batched L-BFGS initialiser (csrc/gsmvi_lbfgs_batched.hip) after the evaluation at ``state["Xt"]``:
        phi = sign fv (K,), its gradient sign gv (K, D) (sign = -1: lp and its score).  ``start``: the first evaluation;
        otherwise accept or reject the trial point of every running problem, update its state in place and write its next
        trial point; ``state["stopped"]`` (optional) grows by the problems that stopped  [gsmvi/initializers.py:5-17]"""
        K, D = state["x"].shape
        self._any_ctx()
        stopped = state.get("stopped")
        self._call("gsmvi_lbfgs_step_batched_f64", K, D, int(bool(start)), self._packed(fv, (K,), "fv"),
                   self._packed(gv, (K, D), "gv"), float(sign), self._packed(state["x"], (K, D), "x"),
                   self._packed(state["g"], (K, D), "g"), self._packed(state["d"], (K, D), "d"),
                   self._packed(state["S"], (K, 10, D), "S"), self._packed(state["Y"], (K, 10, D), "Y"),
                   self._packed(state["sc"], (K, 24), "sc"), self._ist(state, K),
                   self._packed(state["Xt"], (K, D), "Xt"), self._ints(stopped, 1, "stopped"), int(maxiter), int(maxfun),
                   float(gtol), float(ftol))

    def lbfgs_hess_inv_batched(self, state, out=None):
        """cov_k (K, D, D) = the dense BFGS inverse-Hessian product of the pairs held in ``state`` (S, Y, ist) on an identity
        base, exactly symmetric  [scipy.optimize.LbfgsInvHessProduct.todense, gsmvi/initializers.py:15]"""
        K, _, D = state["S"].shape
        self._any_ctx()
        cov = self.empty(K, D, D) if out is None else out
        self._call("gsmvi_lbfgs_hess_inv_batched_f64", K, D, self._packed(state["S"], (K, 10, D), "S"),
                   self._packed(state["Y"], (K, 10, D), "Y"), self._ist(state, K),
                   self._packed(cov, (K, D, D), "cov"))
        return cov

    # ---- batched Pathfinder initialiser: ELBO-selected Gaussians along the L-BFGS path (csrc/gsmvi_pathfinder_batched.hip) ------
    pathfinder_max_draws = 4096

    def pathfinder_state_batched(self, x0, M):
        """The state of K Pathfinder selections over L-BFGS runs started at the rows of x0 (K, D), with M draws per path point:
        a dict of device arrays seen (K) int32 = -1, fresh, info, npts (K) int32, mu (K, D), cov (K, D, D), X (K, M, D), logq,
        elbo_last (K), and the best point so far: best_elbo (K) = -inf, best_mean (K, D) = x0, best_cov (K, D, D) = I,
        best_it (K) int32 = -1"""
        K, D = x0.shape
        M = int(M)
        assert 1 <= M <= self.pathfinder_max_draws, f"M = {M} is outside 1 <= M <= {self.pathfinder_max_draws}"
        ints = lambda v: torch.full((K,), v, dtype=torch.int32, device=self.device)      # noqa: E731
        return {"seen": ints(-1), "fresh": ints(0), "mu": self.zeros(K, D), "cov": self.zeros(K, D, D), "X": self.zeros(K, M, D),
                "logq": self.zeros(K), "info": ints(0), "elbo_last": torch.full((K,), float("nan"), dtype=torch.float64,
                                                                                device=self.device),
                "best_elbo": torch.full((K,), float("-inf"), dtype=torch.float64, device=self.device),
                "best_mean": self.asarray(x0).clone(memory_format=torch.contiguous_format), "best_cov": self.eye_batch(K, D),
                "best_it": ints(-1), "npts": ints(0)}

    def pathfinder_propose_batched(self, lbfgs_state, pf_state, seeds, h0=0.0):
        """The first Pathfinder launch of a round, after ``lbfgs_step_batched``: for every problem whose L-BFGS run accepted a
        point since its last proposal (``pf_state["fresh"]``), the Gaussian of the held pairs on the base ``h0`` I (0: the newest
        pair's s.y / y.y) -> mu, cov, and M draws of draw number nit of the problem's stream -> X, logq; any other problem gets
        its point in every row of X and a NaN logq  [the role of gsmvi/initializers.py:5-17]"""
        K, M, D = pf_state["X"].shape
        self._any_ctx()
        st, pf = lbfgs_state, pf_state
        assert isinstance(seeds, torch.Tensor) and seeds.is_cuda and seeds.dtype == torch.int64 and seeds.is_contiguous() \
            and seeds.numel() == K, f"seeds: expected {K} keys from batched_seeds()"
        self._call("gsmvi_pathfinder_propose_batched_f64", K, D, M, self._packed(st["x"], (K, D), "x"),
                   self._packed(st["g"], (K, D), "g"), self._packed(st["S"], (K, 10, D), "S"),
                   self._packed(st["Y"], (K, 10, D), "Y"), self._packed(st["sc"], (K, 24), "sc"), self._ist(st, K), _ptr(seeds),
                   self._ints(pf["seen"], K, "seen"), float(h0), self._ints(pf["fresh"], K, "fresh"),
                   self._packed(pf["mu"], (K, D), "mu"), self._packed(pf["cov"], (K, D, D), "cov"),
                   self._packed(pf["X"], (K, M, D), "X"), self._packed(pf["logq"], (K,), "logq"), self._ints(pf["info"], K, "info"))

    def pathfinder_select_batched(self, lpsum, lbfgs_state, pf_state):
        """The second Pathfinder launch of a round, after lp of ``pf_state["X"]`` summed over the rows (``lpsum`` (K,)): the ELBO
        estimate (lpsum - logq) / M of every fresh problem -> elbo_last, npts += fresh, and a finite estimate above best_elbo
        (strictly: the first maximum wins) replaces best_elbo, best_mean, best_cov, best_it"""
        K, M, D = pf_state["X"].shape
        self._any_ctx()
        pf = pf_state
        self._call("gsmvi_pathfinder_select_batched_f64", K, D, M, self._packed(lpsum, (K,), "lpsum"),
                   self._packed(pf["logq"], (K,), "logq"), self._ints(pf["fresh"], K, "fresh"), self._ints(pf["info"], K, "info"),
                   self._ist(lbfgs_state, K), self._packed(pf["mu"], (K, D), "mu"), self._packed(pf["cov"], (K, D, D), "cov"),
                   self._packed(pf["elbo_last"], (K,), "elbo_last"), self._ints(pf["npts"], K, "npts"),
                   self._packed(pf["best_elbo"], (K,), "best_elbo"), self._packed(pf["best_mean"], (K, D), "best_mean"),
                   self._packed(pf["best_cov"], (K, D, D), "best_cov"), self._ints(pf["best_it"], K, "best_it"))

    # ---- batched Laplace initialiser: Hessian, inverse and Newton rounds of the GLM targets (csrc/gsmvi_laplace_batched.hip) ----
    def _hess_call(self, name, model_args, X, want, out, cov_out, info_out):
        """The Hessian entry ``name`` of a Laplace family at the rows of X (K, D) after its model's arguments, for a caller that
        has made its context (``_any_ctx``) where it always did among its own checks: allocates what
        ``want`` asks for and ``out`` / ``cov_out`` / ``info_out`` do not give, and returns H, (cov, info) or (H, cov, info)"""
        K, D = X.shape
        H = cov = info = None
        if want != "cov":
            H = self.empty(K, D, D) if out is None else out
        if want != "h":
            cov = self.empty(K, D, D) if cov_out is None else cov_out
            info = torch.zeros(K, dtype=torch.int32, device=self.device) if info_out is None else info_out
        self._call(name, *model_args, self._packed(X, (K, D), "X"), self._dp(H, (K, D, D), "out"),
                   self._dp(cov, (K, D, D), "cov_out"), self._ints(info, K, "info_out"))
        return H if want == "h" else (cov, info) if want == "cov" else (H, cov, info)

    def _laplace_step_args(self, state, K, D, start, maxiter, maxfun, gtol):
        """the eleven arguments every Laplace step entry ends with, after its model's: start, the state, the limits"""
        return (int(bool(start)), self._packed(state["x"], (K, D), "x"), self._packed(state["g"], (K, D), "g"),
                self._packed(state["d"], (K, D), "d"), self._packed(state["sc"], (K, 4), "sc"), self._ist(state, K),
                self._packed(state["Xt"], (K, D), "Xt"), self._ints(state.get("stopped"), 1, "stopped"), int(maxiter),
                int(maxfun), float(gtol))

    def _glm_model_args(self, A, y, family, offset, counts, prior_prec, noise_prec):
        """the model's arguments of the two Laplace entry points, in the order of include/gsmvi_hip.h"""
        K, N, D = A.shape
        fam, t, tp = self._glm_family_args(family, noise_prec, K)
        r, rp = self._reg_arg(prior_prec, K)
        return (K, D, N, fam, self._packed(A, (K, N, D), "A"), self._packed(y, (K, N), "y"),
                self._dp(offset, (K, N), "offset"), self._ints(counts, K, "counts"), t, tp, r, rp)

    def glm_hessian_batched(self, X, A, y, family, offset=None, counts=None, prior_prec=1.0, noise_prec=1.0, want="h", out=None,
                            cov_out=None, info_out=None):
        """The negative Hessian H_k = A_k^T W A_k + lam_k I of lp_k at the rows of X (K, D) and / or its inverse, one launch
        (the Gram product on the fp64 MFMA)  [no reference twin; the model of examples/example_gsm.py:34-35]: ``want`` = "h" ->
        H (K, D, D), "cov" -> (cov, info), "both" -> (H, cov, info); ``info`` (K,) int32: 0, or 1 + the first failing pivot, and
        then cov_k = I.  The other arguments are ``glm_batched``'s."""
        self._check_want(want, "h", "cov")
        self._any_ctx()
        return self._hess_call("gsmvi_glm_hessian_batched_f64",
                               self._glm_model_args(A, y, family, offset, counts, prior_prec, noise_prec), X.contiguous(), want,
                               out, cov_out, info_out)

    def laplace_state_batched(self, x0):
        """The state of K Newton runs started at the rows of x0 (K, D), as include/gsmvi_hip.h lays it out: a dict of device
        arrays x, g, d, Xt (K, D), sc (K, 4), ist (K, 8) int32 and the one-element counter ``stopped``"""
        K, D = x0.shape
        x = self.asarray(x0).clone(memory_format=torch.contiguous_format)
        return {"x": x, "g": self.zeros(K, D), "d": self.zeros(K, D), "Xt": x.clone(), "sc": self.zeros(K, 4),
                "ist": torch.zeros(K, 8, dtype=torch.int32, device=self.device), "stopped": self.new_flag()}

    def laplace_step_batched(self, state, A, y, family, offset=None, counts=None, prior_prec=1.0, noise_prec=1.0, start=False,
                             maxiter=100, maxfun=200, gtol=1e-8):
        """One damped Newton round of every running problem of ``state`` (csrc/gsmvi_laplace_batched.hip): f, g and H at
        ``state["Xt"]`` in one sweep over A, then accept or reject, the stopping tests, the next direction and trial point;
        ``state["stopped"]`` (optional) grows by the problems that stopped  [the role of gsmvi/initializers.py:5-17]"""
        K, D = state["x"].shape
        self._any_ctx()
        self._call("gsmvi_laplace_step_batched_f64", *self._glm_model_args(A, y, family, offset, counts, prior_prec, noise_prec),
                   *self._laplace_step_args(state, K, D, start, maxiter, maxfun, gtol))

    # ---- batched softmax Laplace initialiser: the same for the multinomial logit (csrc/gsmvi_softmax_laplace_batched.hip) -------
    def softmax_hessian_batched(self, X, A, labels, num_classes, counts=None, prior_prec=1.0, want="h", out=None, cov_out=None,
                                info_out=None):
        """The negative Hessian of lp_k of K multinomial logit posteriors at the rows of X (K, D), D = (C - 1) P class-major,
        and / or its inverse, one launch (the class-coupled Gram product on the fp64 MFMA)  [no reference twin; the model of
        examples/example_gsm.py:34-35]: block (c, c') of H_k is sum_n w_n,cc' a_n a_n^T + lam_k [c = c'] I with w_n,cc =
        p_nc (1 - p_nc) and w_n,cc' = -p_nc p_nc'.  ``want`` = "h" -> H (K, D, D), "cov" -> (cov, info), "both" -> (H, cov, info);
        ``info`` (K,) int32: 0, or 1 + the first failing pivot, and then cov_k = I.  The other arguments are ``softmax_batched``'s."""
        self._check_want(want, "h", "cov")
        X = X.contiguous()
        K, D = X.shape
        self._any_ctx()
        (Cc, P, N), model = self._softmax_model_args(K, D, A, labels, num_classes, counts, prior_prec)
        return self._hess_call("gsmvi_softmax_hessian_batched_f64", (K, Cc, P, N, *model), X, want, out, cov_out, info_out)

    def softmax_laplace_step_batched(self, state, A, labels, num_classes, counts=None, prior_prec=1.0, start=False, maxiter=100,
                                     maxfun=200, gtol=1e-8):
        """One damped Newton round of every running problem of ``state`` (``laplace_state_batched``) for the multinomial logit
        posteriors (csrc/gsmvi_softmax_laplace_batched.hip): f, g and H at ``state["Xt"]`` in one sweep over A, then the round of
        ``laplace_step_batched``, the same state machine  [the role of gsmvi/initializers.py:5-17]"""
        K, D = state["x"].shape
        self._any_ctx()
        (Cc, P, N), model = self._softmax_model_args(K, D, A, labels, num_classes, counts, prior_prec)
        self._call("gsmvi_softmax_laplace_step_batched_f64", K, Cc, P, N, *model,
                   *self._laplace_step_args(state, K, D, start, maxiter, maxfun, gtol))

    # ---- shared-design Laplace initialiser: the same for K GLMs on one design matrix (csrc/gsmvi_laplace_shared_batched.hip) -----
    def _glm_shared_model_args(self, K, A, y, family, offset, weights, prior_prec, noise_prec):
        """the model's arguments of the two shared-design Laplace entry points, in the order of include/gsmvi_hip.h"""
        N, D = A.shape
        fam, t, tp = self._glm_family_args(family, noise_prec, K)
        r, rp = self._reg_arg(prior_prec, K)
        return (K, D, N, fam, self._packed(A, (N, D), "A"), self._packed(y, (K, N), "y"), self._dp(offset, (K, N), "offset"),
                self._dp(weights, (K, N), "weights"), t, tp, r, rp)

    def glm_shared_hessian_batched(self, X, A, y, family, offset=None, weights=None, prior_prec=1.0, noise_prec=1.0, want="h",
                                   out=None, cov_out=None, info_out=None):
        """The negative Hessian H_k = A^T diag(v_k w_k) A + lam_k I of lp_k of K GLMs that share ONE design matrix, at the rows
        of X (K, D), and / or its inverse, one launch (the Gram product on the fp64 MFMA, one staged tile of A per workgroup)
        [no reference twin; the model of examples/example_gsm.py:34-35]: ``want`` = "h" -> H (K, D, D), "cov" -> (cov, info),
        "both" -> (H, cov, info); ``info`` (K,) int32: 0, or 1 + the first failing pivot, and then cov_k = I.  The other
        arguments are ``glm_shared_batched``'s."""
        self._check_want(want, "h", "cov")
        X = X.contiguous()
        K, D = X.shape
        self._any_ctx()
        return self._hess_call("gsmvi_glm_shared_hessian_batched_f64",
                               self._glm_shared_model_args(K, A, y, family, offset, weights, prior_prec, noise_prec), X, want, out,
                               cov_out, info_out)

    def laplace_shared_step_batched(self, state, A, y, family, offset=None, weights=None, prior_prec=1.0, noise_prec=1.0,
                                    start=False, maxiter=100, maxfun=200, gtol=1e-8):
        """One damped Newton round of every running problem of ``state`` (``laplace_state_batched``) for K GLMs that share ONE
        design matrix (csrc/gsmvi_laplace_shared_batched.hip): f, g and H at ``state["Xt"]`` in one sweep over A, then the round
        of ``laplace_step_batched``, the same state machine  [the role of gsmvi/initializers.py:5-17]"""
        K, D = state["x"].shape
        self._any_ctx()
        self._call("gsmvi_laplace_shared_step_batched_f64",
                   *self._glm_shared_model_args(K, A, y, family, offset, weights, prior_prec, noise_prec),
                   *self._laplace_step_args(state, K, D, start, maxiter, maxfun, gtol))

    # ---- negative binomial Laplace initialiser: the same for K count regressions with a fitted size
    # (csrc/gsmvi_negbin_laplace_batched.hip) --------------------------------------------------------------------------------------
    def _negbin_model_args(self, A, y, offset, counts, prior_prec, log_size_mean, log_size_prec):
        """the model's arguments of the two negative binomial Laplace entry points, in the order of include/gsmvi_hip.h"""
        K, N, P = A.shape
        r, rp = self._reg_arg(prior_prec, K)
        m, mp = self._reg_arg(log_size_mean, K)
        s, sp = self._reg_arg(log_size_prec, K)
        return (K, P, N, self._packed(A, (K, N, P), "A"), self._packed(y, (K, N), "y"), self._dp(offset, (K, N), "offset"),
                self._ints(counts, K, "counts"), m, mp, s, sp, r, rp)

    def negbin_hessian_batched(self, X, A, y, offset=None, counts=None, prior_prec=1.0, log_size_mean=0.0, log_size_prec=1.0,
                               want="h", out=None, cov_out=None, info_out=None):
        """The negative Hessian of lp_k of K negative binomial regressions at the rows of X (K, P + 1) = (beta, theta), and / or
        its inverse, one launch (the P x P block and the border column as one Gram product on the fp64 MFMA)  [no reference twin;
        the model of examples/example_gsm.py:34-35]: bordered, H[:P, :P] = sum_n w_ee a a^T + lam I, H[:P, P] = sum_n w_et a,
        H[P, P] = sum_n w_tt + kap, and not positive semi-definite in general.  ``want`` = "h" -> H (K, D, D), "cov" -> (cov,
        info), "both" -> (H, cov, info); ``info`` (K,) int32: 0, or 1 + the first failing pivot, and then cov_k = I.  The other
        arguments are ``negbin_batched``'s."""
        self._check_want(want, "h", "cov")
        X = X.contiguous()
        K, D = X.shape
        if D != A.shape[2] + 1:
            raise ValueError(f"X: expected P + 1 = {A.shape[2] + 1} columns (beta, then the log size), got {D}")
        self._any_ctx()
        return self._hess_call("gsmvi_negbin_hessian_batched_f64",
                               self._negbin_model_args(A, y, offset, counts, prior_prec, log_size_mean, log_size_prec), X, want, out,
                               cov_out, info_out)

    def negbin_laplace_step_batched(self, state, A, y, offset=None, counts=None, prior_prec=1.0, log_size_mean=0.0,
                                    log_size_prec=1.0, start=False, maxiter=100, maxfun=200, gtol=1e-8):
        """One damped Newton round of every running problem of ``state`` (``laplace_state_batched``) for K negative binomial
        regressions (csrc/gsmvi_negbin_laplace_batched.hip): f, g and H at ``state["Xt"]`` in one sweep over A, then the round of
        ``laplace_step_batched`` with the last-pivot rule of include/gsmvi_hip.h; ``state["ist"][:, 4]`` counts the rounds with a
        modified pivot  [the role of gsmvi/initializers.py:5-17]"""
        K, D = state["x"].shape
        if D != A.shape[2] + 1:
            raise ValueError(f"state: expected P + 1 = {A.shape[2] + 1} columns (beta, then the log size), got {D}")
        self._any_ctx()
        self._call("gsmvi_negbin_laplace_step_batched_f64",
                   *self._negbin_model_args(A, y, offset, counts, prior_prec, log_size_mean, log_size_prec),
                   *self._laplace_step_args(state, K, D, start, maxiter, maxfun, gtol))

    # ---- ordinal Laplace initialiser: the same for K cumulative-logit regressions (csrc/gsmvi_ordinal_laplace_batched.hip) --------
    def _ordinal_model_args(self, D, A, y, C, offset, counts, prior_prec, cut_prec, what):
        """the model's arguments of the two ordinal Laplace entry points, in the order of include/gsmvi_hip.h"""
        K, N, P = A.shape
        Cc = int(C)
        if Cc < 2:
            raise ValueError(f"C: expected at least 2 classes, got {Cc}")
        if D != P + Cc - 1:
            raise ValueError(f"{what}: expected P + C - 1 = {P + Cc - 1} columns (beta, then the C - 1 cutpoint parameters), got {D}")
        assert y.is_cuda and y.dtype == torch.int32 and y.is_contiguous() and tuple(y.shape) == (K, N), \
            f"y: expected a contiguous int32 CUDA tensor of shape {(K, N)}"
        r, rp = self._reg_arg(prior_prec, K)
        c, cp = self._reg_arg(cut_prec, K)
        return (K, P, Cc, N, self._packed(A, (K, N, P), "A"), _ptr(y), self._dp(offset, (K, N), "offset"),
                self._ints(counts, K, "counts"), r, rp, c, cp)

    def ordinal_hessian_batched(self, X, A, y, C, offset=None, counts=None, prior_prec=1.0, cut_prec=1.0, want="h", out=None,
                                cov_out=None, info_out=None):
        """The negative Hessian of lp_k of K cumulative-logit regressions at the rows of X (K, P + C - 1) = (beta, delta), and / or
        its inverse, one launch (the P x P block and the C - 1 border columns as one Gram product on the fp64 MFMA, the
        delta-delta block from per-class sums)  [no reference twin; the model of examples/example_gsm.py:34-35]: the forms are in
        include/gsmvi_hip.h; H is not positive semi-definite away from the mode (the chain terms of exp(delta_i)).  ``want`` =
        "h" -> H (K, D, D), "cov" -> (cov, info), "both" -> (H, cov, info); ``info`` (K,) int32: 0, or 1 + the first failing
        pivot, and then cov_k = I.  The other arguments are ``ordinal_batched``'s."""
        self._check_want(want, "h", "cov")
        X = X.contiguous()
        K, D = X.shape
        model = self._ordinal_model_args(D, A, y, C, offset, counts, prior_prec, cut_prec, "X")
        self._any_ctx()
        return self._hess_call("gsmvi_ordinal_hessian_batched_f64", model, X, want, out, cov_out, info_out)

    def ordinal_laplace_step_batched(self, state, A, y, C, offset=None, counts=None, prior_prec=1.0, cut_prec=1.0, start=False,
                                     maxiter=100, maxfun=200, gtol=1e-8):
        """One damped Newton round of every running problem of ``state`` (``laplace_state_batched``) for K cumulative-logit
        regressions (csrc/gsmvi_ordinal_laplace_batched.hip): f, g and H at ``state["Xt"]`` in one sweep over A, then the round of
        ``laplace_step_batched`` with the retry rule of include/gsmvi_hip.h; ``state["ist"][:, 4]`` counts the rounds whose
        direction came from the retried matrix  [the role of gsmvi/initializers.py:5-17]"""
        K, D = state["x"].shape
        model = self._ordinal_model_args(D, A, y, C, offset, counts, prior_prec, cut_prec, "state")
        self._any_ctx()
        self._call("gsmvi_ordinal_laplace_step_batched_f64", *model,
                   *self._laplace_step_args(state, K, D, start, maxiter, maxfun, gtol))

    # ---- batched GLM posterior predictive: the use of K fitted Gaussians (csrc/gsmvi_glm_predict_batched.hip) -----------------
    @staticmethod
    def gauss_hermite(Q):
        """(nodes t, log weights) of the Q-point Gauss-Hermite rule (weight exp(-t^2)) as float64 arrays: the table
        gsmvi_glm_predict_batched_f64 is handed (numpy.polynomial.hermite.hermgauss; no table lives in the library)"""
        t, w = np.polynomial.hermite.hermgauss(int(Q))
        return np.asarray(t, dtype=np.float64), np.log(np.asarray(w, dtype=np.float64))

    def _gh_table(self, Q):
        """the device copy of ``gauss_hermite(Q)``, uploaded once per Q and kept on the engine"""
        if Q not in self._gh_tables:
            t, lw = self.gauss_hermite(Q)
            self._gh_tables[Q] = (self.asarray(t), self.asarray(lw))
        return self._gh_tables[Q]

    def glm_predict_batched(self, mean, cov, A, family, offset=None, y=None, counts=None, noise_prec=1.0, nodes=32):
        """The posterior predictive of K fitted GLMs at the rows of A (K, M, D) under q_k = N(mean_k, cov_k), one launch (the
        product A cov on the fp64 MFMA)  [examples/example_gsm.py:34-35, the use of the fit; no reference twin]: returns
        (eta_mean, eta_var, pmean (K, M), lpd (K, M), elpd (K,)), the last two None without ``y``.  ``family``, ``offset``,
        ``counts`` and ``noise_prec`` are ``glm_batched``'s; ``nodes`` = Q Gauss-Hermite nodes, 1 .. 64."""
        fam, t, tp = self._glm_family_args(family, noise_prec, A.shape[0])
        Q = int(nodes)
        if not 1 <= Q <= 64:
            raise ValueError(f"nodes = {nodes!r}: expected 1 .. 64")
        K, M, D = A.shape
        self._any_ctx()
        gt, gl = self._gh_table(Q)
        em, ev, pm = self.empty(K, M), self.empty(K, M), self.empty(K, M)
        lpd = elpd = None
        if y is not None:
            lpd, elpd = self.empty(K, M), self.empty(K)
        self._call("gsmvi_glm_predict_batched_f64", K, D, M, fam, self._packed(A, (K, M, D), "A"),
                   self._dp(offset, (K, M), "offset"), self._dp(y, (K, M), "y"), self._ints(counts, K, "counts"), t, tp,
                   self._packed(mean, (K, D), "mean"), self._packed(cov, (K, D, D), "cov"), Q,
                   self._packed(gt, (Q,), "gh_t"), self._packed(gl, (Q,), "gh_logw"), self._packed(em, (K, M), "eta_mean"),
                   self._packed(ev, (K, M), "eta_var"), self._packed(pm, (K, M), "pmean"), self._dp(lpd, (K, M), "lpd"),
                   self._dp(elpd, (K,), "elpd"))
        return em, ev, pm, lpd, elpd

    # ---- the same for K fitted GLMs on ONE set of new rows, weighted (csrc/gsmvi_glm_shared_predict_batched.hip) ----------------
    def glm_shared_predict_batched(self, mean, cov, A, family, offset=None, y=None, weights=None, noise_prec=1.0, nodes=32):
        """The posterior predictive of K fitted GLMs at the rows of ONE matrix A (M, D) under q_k = N(mean_k, cov_k), with row
        weights, one launch and no copy of A per problem (gsmvi_glm_shared_predict_batched_f64; the definition is in
        include/gsmvi_hip.h)  [no reference twin]: returns (eta_mean, eta_var, pmean (K, M), lpd (K, M), elpd (K,)), the last two
        None without ``y``.  Row m of problem k is valid iff ``weights`` is None or weights[k, m] > 0; the other rows are NaN,
        their ``y`` and ``offset`` are never read, and elpd[k] = sum over the valid rows of weights[k, m] lpd[k, m].  The other
        arguments are ``glm_predict_batched``'s; the Gauss-Hermite table is the engine's cached one."""
        K = mean.shape[0]
        fam, t, tp = self._glm_family_args(family, noise_prec, K)
        Q = int(nodes)
        if not 1 <= Q <= 64:
            raise ValueError(f"nodes = {nodes!r}: expected 1 .. 64")
        M, D = A.shape
        self._any_ctx()
        gt, gl = self._gh_table(Q)
        em, ev, pm = self.empty(K, M), self.empty(K, M), self.empty(K, M)
        lpd = elpd = None
        if y is not None:
            lpd, elpd = self.empty(K, M), self.empty(K)
        self._call("gsmvi_glm_shared_predict_batched_f64", K, D, M, fam, self._packed(A, (M, D), "A"),
                   self._dp(offset, (K, M), "offset"), self._dp(y, (K, M), "y"), self._dp(weights, (K, M), "weights"), t, tp,
                   self._packed(mean, (K, D), "mean"), self._packed(cov, (K, D, D), "cov"), Q,
                   self._packed(gt, (Q,), "gh_t"), self._packed(gl, (Q,), "gh_logw"), self._packed(em, (K, M), "eta_mean"),
                   self._packed(ev, (K, M), "eta_var"), self._packed(pm, (K, M), "pmean"), self._dp(lpd, (K, M), "lpd"),
                   self._dp(elpd, (K,), "elpd"))
        return em, ev, pm, lpd, elpd

    # ---- batched Pareto-smoothed importance diagnostic of K fitted Gaussians (csrc/gsmvi_psis_batched.hip) ----------------------
    def psis_weights_batched(self, logr):
        """The PSIS stage on the log ratios logr (K, S), 5 <= S <= 4096, one launch (gsmvi_psis_weights_batched_f64; the steps
        are in include/gsmvi_hip.h): returns (lw (K, S) normalised smoothed log weights, khat (K,), ess (K,), log_z (K,), info
        (K,) int32: 0, -1 = non-finite ratios (the problem's outputs are NaN), -2 = tail too short to fit (khat = +inf))."""
        logr = logr.contiguous()
        K, S = logr.shape
        self._any_ctx()
        lw, khat, ess, log_z, info = self.empty(K, S), self.empty(K), self.empty(K), self.empty(K), self.batched_ints(K)
        self._call("gsmvi_psis_weights_batched_f64", K, S, self._packed(logr, (K, S), "logr"),
                   self._packed(lw, (K, S), "lw"), self._packed(khat, (K,), "khat"), self._packed(ess, (K,), "ess"),
                   self._packed(log_z, (K,), "log_z"), self._ints(info, K, "info"))
        return lw, khat, ess, log_z, info

    def psis_batched(self, mean, cov, X, lp, moments=True):
        """The fused diagnostic of q_k = N(mean_k, cov_k) from its draws X (K, S, D) and the target's values lp (K, S) at them,
        one launch (gsmvi_psis_batched_f64): log q_k per row by forward substitution with the upper factor of cov_k, the PSIS
        stage on logr = lp - log q, and with ``moments`` the importance-weighted mean and covariance.  Returns (logr (K, S), lw
        (K, S), khat, ess, log_z (K,), mean_is (K, D), cov_is (K, D, D) -- both None without ``moments`` --, info (K,) int32:
        psis_weights_batched's codes, or 1 + the first bad pivot of cov_k, whose outputs are all NaN)."""
        K, S, D = X.shape
        self._any_ctx()
        mean, cov, X, lp = mean.contiguous(), cov.contiguous(), X.contiguous(), lp.contiguous()
        logr, lw, khat, ess, log_z = self.empty(K, S), self.empty(K, S), self.empty(K), self.empty(K), self.empty(K)
        mean_is, cov_is = (self.empty(K, D), self.empty(K, D, D)) if moments else (None, None)
        info = self.batched_ints(K)
        self._call("gsmvi_psis_batched_f64", K, D, S, self._packed(mean, (K, D), "mean"),
                   self._packed(cov, (K, D, D), "cov"), self._packed(X, (K, S, D), "X"), self._packed(lp, (K, S), "lp"),
                   self._packed(logr, (K, S), "logr"), self._packed(lw, (K, S), "lw"), self._packed(khat, (K,), "khat"),
                   self._packed(ess, (K,), "ess"), self._packed(log_z, (K,), "log_z"), self._dp(mean_is, (K, D), "mean_is"),
                   self._dp(cov_is, (K, D, D), "cov_is"), self._ints(info, K, "info"))
        return logr, lw, khat, ess, log_z, mean_is, cov_is, info

    # ---- batched PSIS leave-one-out of K fitted GLM posteriors (csrc/gsmvi_psis_loo_batched.hip) ----------------------------------
    def _loo_call(self, name, head, K, N, S, D, X, logr, lw, pointwise_loglik):
        """The end of the five ``psis_loo_*_batched``: the outputs, the launch of ``name`` on the entry's own leading arguments
        ``head`` followed by the nine that every entry ends with, and what they all return"""
        X, logr, lw = X.contiguous(), logr.contiguous(), lw.contiguous()
        elpd, lpd, khat, ess = self.empty(K, N), self.empty(K, N), self.empty(K, N), self.empty(K, N)
        info = self.batched_ints(K * N).view(K, N)
        loglik = self.empty(K, N, S) if pointwise_loglik else None
        self._call(name, *head, self._packed(X, (K, S, D), "X"), self._packed(logr, (K, S), "logr"),
                   self._packed(lw, (K, S), "lw"), self._dp(loglik, (K, N, S), "loglik"), self._packed(elpd, (K, N), "elpd"),
                   self._packed(lpd, (K, N), "lpd"), self._packed(khat, (K, N), "khat"), self._packed(ess, (K, N), "ess"),
                   self._ints(info, K * N, "info"))
        return elpd, lpd, khat, ess, info, loglik

    def psis_loo_tile(self, D, S):
        """gsmvi_psis_loo_tile: the observations one workgroup of ``psis_loo_batched`` takes at (D, S); a pure function, no GPU"""
        return int(self.lib.gsmvi_psis_loo_tile(int(D), int(S)))

    def psis_loo_batched(self, X, logr, lw, A, y, family, offset=None, counts=None, noise_prec=1.0, pointwise_loglik=False):
        """PSIS leave-one-out of K fitted GLM posteriors from the draws X (K, S, D) of q_k and the problem-level ratios ``logr``
        and smoothed weights ``lw`` (K, S) of ``psis_batched`` on the same draws, one launch (gsmvi_psis_loo_batched_f64; the
        definition is in include/gsmvi_hip.h)  [no reference twin]: returns (elpd, lpd, khat, ess (K, N), info (K, N) int32: 0,
        -1 = non-finite ratios (the row's outputs are NaN), -2 = tail too short (khat = +inf), -3 = not a valid row, loglik
        (K, N, S) or None without ``pointwise_loglik``).  ``family``, ``offset``, ``counts`` and ``noise_prec`` are
        ``glm_batched``'s."""
        K, S, D = X.shape
        N = A.shape[1]
        fam, t, tp = self._glm_family_args(family, noise_prec, K)
        self._any_ctx()
        head = (fam, K, N, D, S, self._packed(A, (K, N, D), "A"), self._packed(y, (K, N), "y"),
                self._dp(offset, (K, N), "offset"), self._ints(counts, K, "counts"), t, tp)
        return self._loo_call("gsmvi_psis_loo_batched_f64", head, K, N, S, D, X, logr, lw, pointwise_loglik)

    # ---- the same for K fitted multinomial logit posteriors (csrc/gsmvi_psis_loo_softmax_batched.hip) --------------------------
    def psis_loo_softmax_tile(self, C, P, S):
        """gsmvi_psis_loo_softmax_tile: the observations one workgroup of ``psis_loo_softmax_batched`` takes at (C, P, S); a pure
        function, no GPU"""
        return int(self.lib.gsmvi_psis_loo_softmax_tile(int(C), int(P), int(S)))

    def psis_loo_softmax_batched(self, X, logr, lw, A, labels, num_classes, counts=None, pointwise_loglik=False):
        """PSIS leave-one-out of K fitted multinomial logit posteriors from the draws X (K, S, D) of q_k, D = (C - 1) P
        class-major, and the problem-level ratios ``logr`` and smoothed weights ``lw`` (K, S) of ``psis_batched`` on the same draws,
        one launch (gsmvi_psis_loo_softmax_batched_f64; the definition is in include/gsmvi_hip.h)  [no reference twin]: returns
        what ``psis_loo_batched`` returns, (elpd, lpd, khat, ess (K, N), info (K, N) int32, loglik (K, N, S) or None).  ``A``
        (K, N, P), ``labels`` (K, N) int32, ``num_classes`` and ``counts`` are ``softmax_batched``'s."""
        K, S, D = X.shape
        (Cc, P, N), model = self._softmax_model_args(K, D, A, labels, num_classes, counts)
        self._any_ctx()
        return self._loo_call("gsmvi_psis_loo_softmax_batched_f64", (K, Cc, P, N, S, *model), K, N, S, D, X, logr, lw,
                              pointwise_loglik)

    # ---- the same for K fitted negative binomial posteriors (csrc/gsmvi_psis_loo_negbin_batched.hip) ---------------------------
    def psis_loo_negbin_tile(self, P, S):
        """gsmvi_psis_loo_negbin_tile: the observations one workgroup of ``psis_loo_negbin_batched`` takes at (P, S); a pure
        function, no GPU"""
        return int(self.lib.gsmvi_psis_loo_negbin_tile(int(P), int(S)))

    def psis_loo_negbin_batched(self, X, logr, lw, A, y, offset=None, counts=None, pointwise_loglik=False):
        """PSIS leave-one-out of K fitted negative binomial posteriors from the draws X (K, S, P + 1) = (beta, theta) of q_k, theta
        the log of the size, and the problem-level ratios ``logr`` and smoothed weights ``lw`` (K, S) of ``psis_batched`` on the
        same draws, one launch (gsmvi_psis_loo_negbin_batched_f64; the definition is in include/gsmvi_hip.h)  [no reference twin]:
        returns what ``psis_loo_batched`` returns, (elpd, lpd, khat, ess (K, N), info (K, N) int32, loglik (K, N, S) or None).  The
        pointwise log likelihood includes -lgamma(y + 1), as the poisson family of ``psis_loo_batched`` does: the two elpd are on
        one scale.  ``A`` (K, N, P), ``y`` (K, N), ``offset`` and ``counts`` are ``negbin_batched``'s."""
        K, S, D = X.shape
        N, P = A.shape[1], A.shape[2]
        if D != P + 1:
            raise ValueError(f"X: expected P + 1 = {P + 1} columns (beta, then the log size), got {D}")
        self._any_ctx()
        head = (K, P, N, S, self._packed(A, (K, N, P), "A"), self._packed(y, (K, N), "y"), self._dp(offset, (K, N), "offset"),
                self._ints(counts, K, "counts"))
        return self._loo_call("gsmvi_psis_loo_negbin_batched_f64", head, K, N, S, D, X, logr, lw, pointwise_loglik)

    # ---- the same for K fitted cumulative-logit posteriors (csrc/gsmvi_psis_loo_ordinal_batched.hip) ---------------------------
    def psis_loo_ordinal_tile(self, P, C, S):
        """gsmvi_psis_loo_ordinal_tile: the observations one workgroup of ``psis_loo_ordinal_batched`` takes at (P, C, S); a pure
        function, no GPU"""
        return int(self.lib.gsmvi_psis_loo_ordinal_tile(int(P), int(C), int(S)))

    def psis_loo_ordinal_batched(self, X, logr, lw, A, y, C, offset=None, counts=None, pointwise_loglik=False):
        """PSIS leave-one-out of K fitted cumulative-logit posteriors from the draws X (K, S, P + C - 1) = (beta, delta) of q_k,
        delta the C - 1 cutpoint parameters, and the problem-level ratios ``logr`` and smoothed weights ``lw`` (K, S) of
        ``psis_batched`` on the same draws, one launch (gsmvi_psis_loo_ordinal_batched_f64; the definition is in
        include/gsmvi_hip.h)  [no reference twin]: returns what ``psis_loo_batched`` returns, (elpd, lpd, khat, ess (K, N), info
        (K, N) int32, loglik (K, N, S) or None).  The pointwise log likelihood is the log of the label's probability, already
        normalised: elpd is on the scale of ``psis_loo_softmax_batched``.  ``A`` (K, N, P), ``y`` (K, N) int32 labels, ``C``,
        ``offset`` and ``counts`` are ``ordinal_batched``'s."""
        K, S, D = X.shape
        N, P = A.shape[1], A.shape[2]
        Cc = int(C)
        if D != P + Cc - 1:
            raise ValueError(f"X: expected P + C - 1 = {P + Cc - 1} columns (beta, then the C - 1 cutpoint parameters), got {D}")
        self._any_ctx()
        head = (K, P, Cc, N, S, self._packed(A, (K, N, P), "A"), self._ints(y, K * N, "y"), self._dp(offset, (K, N), "offset"),
                self._ints(counts, K, "counts"))
        return self._loo_call("gsmvi_psis_loo_ordinal_batched_f64", head, K, N, S, D, X, logr, lw, pointwise_loglik)

    # ---- the same for K fitted GLM posteriors on ONE design matrix, weighted (k_psis_loo_batched<FAM, true> of the same file) ---
    def psis_loo_shared_batched(self, X, logr, lw, A, y, family, offset=None, weights=None, noise_prec=1.0, pointwise_loglik=False):
        """PSIS leave-one-out of K fitted GLM posteriors that share ONE design matrix, from the draws X (K, S, D) of q_k and the
        problem-level ratios ``logr`` and smoothed weights ``lw`` (K, S) of ``psis_batched`` on the same draws, one launch with no
        copy of A per problem (gsmvi_psis_loo_shared_batched_f64; the definition is in include/gsmvi_hip.h)  [no reference twin]:
        returns what ``psis_loo_batched`` returns, (elpd, lpd, khat, ess (K, N), info (K, N) int32, loglik (K, N, S) or None).
        ``A`` (N, D) shared, ``y`` (K, N), ``offset`` and ``weights`` None or (K, N), ``family`` and ``noise_prec`` are
        ``glm_shared_batched``'s.  Row i of problem k is valid iff its weight is > 0 (any subset of the rows; the others get
        info = -3 and NaN); the pointwise log likelihood is that of one unit observation, unweighted, and leaving row i out removes
        weight x log likelihood from the ratios.  The tile of observations per workgroup is ``psis_loo_tile(D, S)``."""
        K, S, D = X.shape
        N = A.shape[0]
        fam, t, tp = self._glm_family_args(family, noise_prec, K)
        self._any_ctx()
        head = (fam, K, N, D, S, self._packed(A, (N, D), "A"), self._packed(y, (K, N), "y"),
                self._dp(offset, (K, N), "offset"), self._dp(weights, (K, N), "weights"), t, tp)
        return self._loo_call("gsmvi_psis_loo_shared_batched_f64", head, K, N, S, D, X, logr, lw, pointwise_loglik)

    # ---- batched softmax posterior predictive: the use of K fitted multinomial logit posteriors (csrc/gsmvi_softmax_predict_batched.hip)
    def softmax_predict_lds_bytes(self, C, P):
        """gsmvi_softmax_predict_lds_bytes: the dynamic LDS in bytes of one workgroup of ``softmax_predict_batched`` at (C, P), 0
        out of bounds; a pure function, no GPU"""
        return int(self.lib.gsmvi_softmax_predict_lds_bytes(int(C), int(P)))

    def softmax_predict_batched(self, X, lw, A, num_classes, labels=None, counts=None):
        """The posterior predictive of K fitted multinomial logit posteriors at the rows of A (K, M, P) from the draws X (K, S, D)
        of q_k, D = (C - 1) P class-major, weighted by the normalised log weights ``lw`` (K, S) (``psis_batched``'s; None:
        uniform), one launch (gsmvi_softmax_predict_batched_f64; the definition is in include/gsmvi_hip.h)  [no reference twin]:
        returns (prob (K, M, C), lpd (K, M) or None without ``labels``).  ``labels`` (K, M) int32, ``num_classes`` and ``counts``
        are ``softmax_batched``'s, for the new rows."""
        K, S, D = X.shape
        (Cc, P, M), model = self._softmax_model_args(K, D, A, labels, num_classes, counts)
        self._any_ctx()
        X = X.contiguous()
        lw = lw.contiguous() if lw is not None else None
        prob = self.empty(K, M, Cc)
        lpd = self.empty(K, M) if labels is not None else None
        self._call("gsmvi_softmax_predict_batched_f64", K, Cc, P, M, S, *model, self._packed(X, (K, S, D), "X"),
                   self._dp(lw, (K, S), "lw"), self._packed(prob, (K, M, Cc), "prob"), self._dp(lpd, (K, M), "lpd"))
        return prob, lpd

    # ---- the same use of K fitted negative binomial posteriors (csrc/gsmvi_negbin_predict_batched.hip) ---------------------------
    def negbin_predict_batched(self, X, lw, A_new, y=None, offset=None, counts=None):
        """The posterior predictive of K fitted negative binomial posteriors at the rows of A_new (K, M, P) from the draws X
        (K, S, P + 1) = (beta, theta) of q_k, weighted by the normalised log weights ``lw`` (K, S) (``psis_batched``'s; None:
        uniform), one launch (gsmvi_negbin_predict_batched_f64; the definition is in include/gsmvi_hip.h)  [no reference twin]:
        returns (lmom (K, M, 3) = log E[mu], log E[mu^2], log E[mu^2 / r], lpd (K, M) or None without ``y``).  ``y`` (K, M),
        ``offset`` and ``counts`` are ``negbin_batched``'s, for the new rows."""
        K, S, D = X.shape
        M, P = A_new.shape[1], A_new.shape[2]
        if D != P + 1:
            raise ValueError(f"X: expected P + 1 = {P + 1} columns (beta, then the log size), got {D}")
        self._any_ctx()
        X = X.contiguous()
        lw = lw.contiguous() if lw is not None else None
        lmom = self.empty(K, M, 3)
        lpd = self.empty(K, M) if y is not None else None
        self._call("gsmvi_negbin_predict_batched_f64", K, P, M, S, self._packed(A_new, (K, M, P), "A_new"),
                   self._dp(y, (K, M), "y"), self._dp(offset, (K, M), "offset"), self._ints(counts, K, "counts"),
                   self._packed(X, (K, S, D), "X"), self._dp(lw, (K, S), "lw"), self._packed(lmom, (K, M, 3), "lmom"),
                   self._dp(lpd, (K, M), "lpd"))
        return lmom, lpd

    # ---- the same use of K fitted cumulative-logit posteriors (csrc/gsmvi_ordinal_predict_batched.hip) ---------------------------
    def ordinal_predict_lds_bytes(self, P, C):
        """gsmvi_ordinal_predict_lds_bytes: the dynamic LDS in bytes of one workgroup of ``ordinal_predict_batched`` at (P, C), 0
        out of bounds; a pure function, no GPU"""
        return int(self.lib.gsmvi_ordinal_predict_lds_bytes(int(P), int(C)))

    def ordinal_predict_batched(self, X, lw, A, C, y=None, offset=None, counts=None):
        """The posterior predictive of K fitted cumulative-logit posteriors at the rows of A (K, M, P) from the draws X
        (K, S, P + C - 1) = (beta, delta) of q_k, delta the C - 1 cutpoint parameters, weighted by the normalised log weights
        ``lw`` (K, S) (``psis_batched``'s; None: uniform), one launch (gsmvi_ordinal_predict_batched_f64; the definition is in
        include/gsmvi_hip.h)  [no reference twin]: returns (prob (K, M, C), lpd (K, M) or None without ``y``).  ``y`` (K, M) int32
        labels, ``C``, ``offset`` and ``counts`` are ``ordinal_batched``'s, for the new rows."""
        K, S, D = X.shape
        M, P = A.shape[1], A.shape[2]
        Cc = int(C)
        if D != P + Cc - 1:
            raise ValueError(f"X: expected P + C - 1 = {P + Cc - 1} columns (beta, then the C - 1 cutpoint parameters), got {D}")
        self._any_ctx()
        X = X.contiguous()
        lw = lw.contiguous() if lw is not None else None
        prob = self.empty(K, M, Cc)
        lpd = self.empty(K, M) if y is not None else None
        self._call("gsmvi_ordinal_predict_batched_f64", K, P, Cc, M, S, self._packed(A, (K, M, P), "A"),
                   self._ints(y, K * M, "y"), self._dp(offset, (K, M), "offset"), self._ints(counts, K, "counts"),
                   self._packed(X, (K, S, D), "X"), self._dp(lw, (K, S), "lw"), self._packed(prob, (K, M, Cc), "prob"),
                   self._dp(lpd, (K, M), "lpd"))
        return prob, lpd

    def bam_update(self, X, G, mu0, S0, reg, jitter=0.0, out=None, flag=None):
        """(mu, S) of BaM [gsmvi/bam.py:72-114]; S symmetrised, jitter on the diagonal."""
        assert X.dim() == 2 and G.dim() == 2            # bam.py:47-48
        B, D = X.shape
        if B > self.bam_max_batch:                      # a deterministic limit: never inside a retry loop
            raise ValueError(f"BaM update: batch size {B} exceeds the device chain's limit of {self.bam_max_batch}")
        self._ensure(D, B)
        mu, S = (self.empty(D), self.empty(D, D)) if out is None else out
        flag = self.new_flag() if flag is None else flag
        self._call("gsmvi_bam_update_f64", D, B, *self._mat(X, "samples"), *self._mat(G, "vs"), self._vec(mu0, "mu0"),
                   *self._mat(S0, "S0"), float(reg), float(jitter), self._vec(mu, "mu"), *self._mat(S, "S"),
                   _ptr(flag))
        return mu, S, flag


_ENGINES = {}


def get_engine(device=None):
    """Process-wide engine per device (created on first use; raises if the library or GPU is missing).
    ONE context = ONE workspace: calls through the shared engine must not run concurrently on two streams or two
    threads; give every extra stream / thread its own ``HipEngine(device)`` (as bench.py --in-flight does)."""
    _lib.load_library()
    _require_gpu()
    idx = _device_index(device)
    if idx not in _ENGINES:
        _ENGINES[idx] = HipEngine(idx)
    return _ENGINES[idx]
