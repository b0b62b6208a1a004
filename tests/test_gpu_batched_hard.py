"""The batched core on the GPU, held to its float64 noise floor on hard inputs (tests/batched_hard_ref.py: the long double
restatements, the families, the floors; its conditions are asserted on the CPU by tests/test_batched_hard_cpu.py): the GSM
update with its increments, the fit INIT and STEP with their factor and samples, the BaM update and step with the defining
equation's residual, log q of points and of the monitor's draws, isolation of the problems of a heterogeneous batch, and a
teacher-forced trajectory against the same loop in long double.  Everywhere kernel_err <= M x floor with M = 16; every test
prints its kernel_err / floor ratios per family before it asserts."""
import functools

import numpy as np
import pytest

import batched_hard_ref as ref
import batched_step_ref as step

pytestmark = pytest.mark.gpu

LD = ref.LD
SHAPES = [(D, B) for D in ref.D_GRID for B in ref.B_GRID]
KL_CHUNK = 7
# margins above M = 16 for one (entry point, family, output), each with its arithmetic reason: none is needed
MARGINS = {}


class _Ratios:
    """collects kernel_err / floor of one test, prints the largest per (entry point, family, output), then fails if any
    exceeded its margin"""

    def __init__(self, where):
        self.where, self.worst, self.failed = where, {}, []

    def check(self, entry, fam, out, got, want, floor):
        """``want`` None: ``got`` is itself the error (a residual)"""
        if want is None:
            err = float(got)
        else:
            err = ref.rel_err(got, want) if np.isfinite(np.asarray(got, dtype=np.float64)).all() else np.inf
        key = (entry, fam, out)
        self.worst[key] = max(self.worst.get(key, 0.0), err / floor)
        if not err <= MARGINS.get(key, ref.M_BAR) * floor:
            self.failed.append((key, err, floor))

    def done(self):
        for entry in sorted({k[0] for k in self.worst}):
            for fam in ref.FAMILIES:
                row = [(k[2], r) for k, r in self.worst.items() if k[0] == entry and k[1] == fam]
                if row:
                    print(f"RATIO {self.where} {entry:9s} {fam:10s} " + " ".join(f"{n}={r:.2g}" for n, r in row))
        assert not self.failed, (self.where, self.failed)


def _eng():
    import gsmvi_amd
    return gsmvi_amd.get_engine()


def _inputs(D, B, idx):
    b = ref.batch(D, B)
    return {n: np.ascontiguousarray(b[n][list(idx)]) for n in ("X", "V", "mu0", "S0", "Y")}


@functools.lru_cache(maxsize=None)
def _run(entry, D, B, idx):
    """one launch of ``entry`` on the problems ``idx`` of batch(D, B); every output as numpy (shared: never modified)"""
    eng = _eng()
    a = _inputs(D, B, idx)
    n = len(idx)
    X, V, mean, cov = (eng.asarray(a[name].copy()) for name in ("X", "V", "mu0", "S0"))
    seeds = eng.batched_seeds([ref.SEEDS[k] for k in idx])
    info, n_rev = eng.batched_counts([-1] * n), eng.batched_counts([0] * n)
    regs = eng.batched_regs(np.array([ref.bam_reg(k) for k in idx]))
    out = {}
    if entry == "update":
        mu, S = eng.gsm_update_batched(X, V, mean, cov)
        out.update(mu=mu, S=S)
    elif entry == "init":
        R, Xo = eng.empty(n, D, D), eng.empty(n, B, D)
        eng.gsm_fit_init_batched(mean, cov, R, info, seeds, Xo)
        out.update(R=R, Xo=Xo)
    elif entry == "step":
        R = eng.zeros(n, D, D)
        eng.gsm_fit_step_batched(X, V, mean, cov, R, info, n_rev, seeds, ref.CALL)
        out.update(R=R, Xo=X)
    elif entry == "bam_update":
        mu, S = eng.bam_update_batched(X, V, mean, cov, regs, ref.JITTER, info=info)
        out.update(mu=mu, S=S)
    elif entry == "bam_step":
        eng.bam_fit_step_batched(X, V, mean, cov, None, regs, ref.JITTER, info, n_rev)
    elif entry == "logq":
        logq, info = eng.logq_batched(mean, cov, eng.asarray(a["Y"].copy()))
        out.update(logq=logq)
    elif entry == "kl_draw":
        Xo, logq, info = eng.kl_draw_batched(mean, cov, seeds, ref.KL_CALL, 0, ref.N_POINTS)
        parts = [eng.kl_draw_batched(mean, cov, seeds, ref.KL_CALL, s0, min(KL_CHUNK, ref.N_POINTS - s0))[0]
                 for s0 in range(0, ref.N_POINTS, KL_CHUNK)]
        import torch
        out.update(Xo=Xo, logq=logq, chunks=torch.cat(parts, dim=1))
    else:
        raise AssertionError(entry)
    out = {name: t.cpu().numpy() for name, t in out.items()}
    out.update(info=eng.read_ints(info), n_rev=eng.read_ints(n_rev), mean=mean.cpu().numpy(), cov=cov.cpu().numpy(),
               X=X.cpu().numpy(), V=V.cpu().numpy())
    for v in out.values():
        v.setflags(write=False)
    return out


def _batches(D, bam=False):
    """the index lists of the K = 11 batch and of the K = 15 batch with its repeats (BaM: the families it keeps at this D)"""
    keep = [k for k, fam in enumerate(ref.FAMILIES) if not bam or fam in ref.bam_families(D)]
    return tuple(keep), tuple(keep + [k for k in ref.REPEATS if k in keep])


def _untouched(out, D, B, idx, names):
    a = _inputs(D, B, idx)
    for name, src in names:
        assert np.array_equal(out[name], a[src]), (name, "input modified")


@pytest.mark.parametrize("D,B", SHAPES)
def test_gsm_update_with_its_increments(D, B):
    """mean, S', the mean's increment and S' - S0 against long double, each at its own floor: on the nearly converged and far
    families the increment is 1e-7 of S' and below, so a wrong increment is invisible in S' itself"""
    import gsmvi_amd
    want, floor = ref.gsm_case(D, B)
    rat = _Ratios(f"D={D} B={B}")
    for idx in _batches(D):
        a = _inputs(D, B, idx)
        args = [a[n].copy() for n in ("X", "V", "mu0", "S0")]
        mu, S = gsmvi_amd.gsm_update_batched(*args)                     # the public entry point, numpy in and out
        for got, n in zip(args, ("X", "V", "mu0", "S0")):
            assert np.array_equal(got, a[n])                            # inputs untouched
        low = _run("update", D, B, idx)
        assert np.array_equal(mu, low["mu"]) and np.array_equal(S, low["S"])
        _untouched(low, D, B, idx, (("X", "X"), ("V", "V"), ("mean", "mu0"), ("cov", "S0")))
        for j, k in enumerate(idx):
            fam = ref.FAMILIES[k]
            assert np.array_equal(S[j], S[j].T), fam
            rat.check("update", fam, "mu", mu[j], want[k]["mu"], floor[k]["mu"])
            rat.check("update", fam, "S", S[j], want[k]["S"], floor[k]["S"])
            rat.check("update", fam, "dmu", np.asarray(mu[j], dtype=LD) - np.asarray(a["mu0"][j], dtype=LD), want[k]["dmu"],
                      floor[k]["dmu"])
            rat.check("update", fam, "dS", np.asarray(S[j], dtype=LD) - np.asarray(a["S0"][j], dtype=LD), want[k]["dS"],
                      floor[k]["dS"])
    rat.done()


@pytest.mark.parametrize("D,B", SHAPES)
def test_gsm_fit_init_and_step_with_seeds(D, B):
    """INIT: the factor of S0 and the first samples; STEP: every problem accepts, writes the UPDATE launch's bits, the factor
    of the covariance it wrote and the samples of the accepted state"""
    want, floor = ref.gsm_case(D, B)
    rat = _Ratios(f"D={D} B={B}")
    for idx in _batches(D):
        a = _inputs(D, B, idx)
        ini, stp, upd = _run("init", D, B, idx), _run("step", D, B, idx), _run("update", D, B, idx)
        assert np.array_equal(ini["info"], np.zeros(len(idx))) and np.array_equal(stp["info"], np.zeros(len(idx)))
        assert np.array_equal(stp["n_rev"], np.zeros(len(idx)))
        _untouched(ini, D, B, idx, (("mean", "mu0"), ("cov", "S0")))
        _untouched(stp, D, B, idx, (("V", "V"),))
        assert np.array_equal(stp["mean"], upd["mu"]) and np.array_equal(stp["cov"], upd["S"])      # the accepted bits
        for j, k in enumerate(idx):
            fam = ref.FAMILIES[k]
            for out in (ini, stp):
                assert np.array_equal(np.tril(out["R"][j], -1), np.zeros((D, D))) and (np.diag(out["R"][j]) > 0).all(), fam
            rat.check("init", fam, "R", ini["R"][j], want[k]["R0"], floor[k]["R0"])
            rat.check("init", fam, "X", ini["Xo"][j], want[k]["X0"], floor[k]["X0"])
            R1 = step.chol_ld(stp["cov"][j])
            rat.check("step", fam, "R", stp["R"][j], R1, floor[k]["R1"])
            rat.check("step", fam, "X", stp["Xo"][j], step.sample(stp["mean"][j], R1, step.draw(ref.SEEDS[k], ref.CALL, B, D)),
                      floor[k]["X1"])
    rat.done()


def _bam_residual(S, a, j, k):
    return ref.bam_residual(np.asarray(S, dtype=LD) - LD(ref.JITTER) * np.eye(S.shape[0], dtype=LD), a["X"][j], a["V"][j],
                            a["mu0"][j], a["S0"][j], ref.bam_reg(k))


@pytest.mark.parametrize("D,B", SHAPES)
def test_bam_update_and_step(D, B):
    """mean and S' against the long double restatement at the BaM floor, the long double residual of S U S + S = V of the
    kernel's S' against that of the float64 oracle's under the same rule, symmetry; the step accepts and writes those bits.
    A case whose chain float64 may not carry (ref.bam_may_flag: the steep family, trace(N + I / 4) beyond 1 / (4 eps)) may
    come back flagged -- info = 1, NaN, the step reverts, the neighbours untouched (the isolation test) --; returned
    unflagged it is held to its floor like any other, unless float64 holds no digit of it (ref.bam_resolved: steep at B = 2),
    where it is asked only for a finite symmetric result that the step accepts or reverts."""
    want, floor = ref.bam_case(D, B)
    rat = _Ratios(f"D={D} B={B}")
    for idx in _batches(D, bam=True):
        a = _inputs(D, B, idx)
        upd, stp = _run("bam_update", D, B, idx), _run("bam_step", D, B, idx)
        _untouched(upd, D, B, idx, (("X", "X"), ("V", "V"), ("mean", "mu0"), ("cov", "S0")))
        _untouched(stp, D, B, idx, (("X", "X"), ("V", "V")))
        for j, k in enumerate(idx):
            fam = ref.FAMILIES[k]
            mu, S = upd["mu"][j], upd["S"][j]
            accepted = np.array_equal(stp["mean"][j], mu) and np.array_equal(stp["cov"][j], S) and stp["info"][j] == 0 \
                and stp["n_rev"][j] == 0
            reverted = np.array_equal(stp["mean"][j], a["mu0"][j]) and np.array_equal(stp["cov"][j], a["S0"][j]) \
                and stp["info"][j] != 0 and stp["n_rev"][j] == 1
            if upd["info"][j] != 0 or not ref.bam_resolved(floor[k]):
                assert ref.bam_may_flag(want[k]["ns"]) or not ref.bam_resolved(floor[k]), (fam, "flagged", upd["info"][j])
                if upd["info"][j] == 1:
                    assert np.isnan(mu).all() and np.isnan(S).all() and reverted, fam
                else:
                    assert upd["info"][j] == 0 and np.isfinite(mu).all() and np.isfinite(S).all(), fam
                    assert np.array_equal(S, S.T) and (accepted or reverted), fam
                print(f"FLAG D={D} B={B} {fam}: info {upd['info'][j]}, step info {stp['info'][j]}")
                continue
            assert upd["info"][j] == 0 and accepted, (fam, upd["info"][j], stp["info"][j])
            assert np.array_equal(S, S.T), fam
            rat.check("bam", fam, "mu", mu, want[k]["mu"], floor[k]["mu"])
            rat.check("bam", fam, "S", S, want[k]["S"], floor[k]["S"])
            rat.check("bam", fam, "res", _bam_residual(S, a, j, k), None, floor[k]["res"])
    rat.done()


@pytest.mark.parametrize("D,B", SHAPES)
def test_logq_of_points_and_of_the_monitors_draws(D, B):
    """logq_batched on 24 points per problem and kl_draw_batched on its own draws (the states of batch(D, B): B only selects the
    states): X and log q against long double at their floors, info zero, the chunked draws bit-equal to the whole"""
    want, floor = ref.gsm_case(D, B)
    rat = _Ratios(f"D={D} B={B}")
    for idx in _batches(D):
        lq, kl = _run("logq", D, B, idx), _run("kl_draw", D, B, idx)
        assert np.array_equal(lq["info"], np.zeros(len(idx))) and np.array_equal(kl["info"], np.zeros(len(idx)))
        assert np.array_equal(kl["chunks"], kl["Xo"])
        for out in (lq, kl):
            _untouched(out, D, B, idx, (("mean", "mu0"), ("cov", "S0")))
        for j, k in enumerate(idx):
            fam = ref.FAMILIES[k]
            rat.check("logq", fam, "logq", lq["logq"][j], want[k]["logq"], floor[k]["logq"])
            rat.check("kl_draw", fam, "X", kl["Xo"][j], want[k]["klX"], floor[k]["klX"])
            rat.check("kl_draw", fam, "logq", kl["logq"][j], want[k]["kllogq"], floor[k]["kllogq"])
    rat.done()


@pytest.mark.parametrize("D", [16, 17])
def test_every_problem_gives_the_same_bits_in_any_batch(D):
    """every problem of the K = 15 batch gives the bits it gives in the K = 11 batch and alone (K = 1), in every entry point:
    neighbours of other scales, conditions and Newton-Schulz step counts share its workgroup at D = 16"""
    B = 2
    for entry in ("update", "init", "step", "bam_update", "bam_step", "logq", "kl_draw"):
        small, big = _batches(D, bam=entry.startswith("bam"))
        a, b = _run(entry, D, B, small), _run(entry, D, B, big)
        alone = {k: _run(entry, D, B, (k,)) for k in small}
        for name in a:
            for j, k in enumerate(big):
                i = small.index(k)
                assert np.array_equal(b[name][j], a[name][i], equal_nan=True), (entry, name, ref.FAMILIES[k], "K = 15 | K = 11")
                assert np.array_equal(alone[k][name][0], a[name][i], equal_nan=True), (entry, name, ref.FAMILIES[k], "K = 1")


def _scores(G):
    """a host score that hands out the precomputed scores of the forced samples, one iteration per call"""
    count = [0]

    def lp_g(X):
        count[0] += 1
        return G[count[0] - 1].copy()
    return lp_g


@pytest.mark.parametrize("method,D,B", [("gsm",) + ref.TRAJ_SHAPES[0], ("gsm",) + ref.TRAJ_SHAPES[1], ("bam",) + ref.TRAJ_SHAPES[0]])
def test_teacher_forced_trajectory_follows_the_long_double_loop(method, D, B):
    """50 iterations on forced samples: the reverts of every problem and the final mean and covariance against the same loop in
    long double, at the floor of the float64 loops (both operation orders) against it"""
    import gsmvi_amd
    t, want = ref.traj_inputs(D, B), ref.traj_case(method, D, B)
    K = ref.TRAJ_K
    if method == "gsm":
        fit = gsmvi_amd.GSMBatch(K, D, None, _scores(t["G"]))
        mean, cov = fit.fit(np.arange(K), niter=ref.TRAJ_NITER, batch_size=B, verbose=False, forced_samples=np.array(t["forced"]))
    else:
        fit = gsmvi_amd.BaMBatch(K, D, None, _scores(t["G"]))
        mean, cov = fit.fit(range(K), ref.traj_regs, batch_size=B, niter=ref.TRAJ_NITER, verbose=False, jitter=ref.JITTER,
                            forced_samples=np.array(t["forced"]))
    assert fit.n_reverts.tolist() == [o["reverts"] for o in want]
    worst, failed = [], []
    for k, o in enumerate(want):
        for name, got, w, fl in (("mean", mean[k], o["mean"], o["floor_mean"]), ("cov", cov[k], o["cov"], o["floor_cov"])):
            err = ref.rel_err(got, w)
            worst.append(f"{name}[{k}]={err / fl:.2g}")
            if not err <= ref.M_BAR * fl:
                failed.append((name, k, err, fl))
    print(f"RATIO trajectory {method} D={D} B={B} " + " ".join(worst))
    assert not failed, failed
