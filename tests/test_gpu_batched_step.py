"""The tail of the batched fit step on the GPU, launch by launch (csrc/gsmvi_batched.h: gb_chol_lds, gb_fit_tail, as run by
k_gsm_batched<NT, GB_STEP / GB_INIT> and k_bam_batched<NT, BB_STEP>): the factor against a long double Cholesky, the verdict's
code, what an accept writes and a revert keeps, and the next samples from the accepted or the KEPT state, on the mixed batch
of tests/batched_step_ref.py (its conditions are asserted on the CPU by tests/test_batched_step_cpu.py); both halves of seed
and draw number; the unpadded strides of the batched BaM kernel; fits that revert and recover."""
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

import batched_step_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

K = ref.K
TOL = {"gsm": 1e-12, "bam": 1e-8}        # the one-shot tolerances of test_gpu_batched.py / test_gpu_bam_batched.py
TOL_R = TOL_X = 1e-11                    # test_gpu_kl_batched.py::test_init_and_cov, the same in-LDS factorisation


def _batch_sizes(method, D):
    return list(ref.B_GRID) + ([B for D_, B in ref.BAM_EXTRA if D_ == D] if method == "bam" else [])


def _launch(method, D, B, nan_case=False, draws=True):
    """one STEP launch on the mixed batch from uploaded states; every output as numpy"""
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    mb = ref.mixed_batch(method, D, B, nan_case)
    X, V, mean, cov, R = (eng.asarray(np.array(mb[n], copy=True)) for n in ("X", "V", "mu0", "S0", "R_kept"))
    info, n_rev = eng.batched_counts([-1] * K), eng.batched_counts(mb["n_rev0"])
    seeds = eng.batched_seeds(mb["seeds"]) if draws else None
    if method == "gsm":
        eng.gsm_fit_step_batched(X, V, mean, cov, R if draws else None, info, n_rev, seeds, ref.CALL)
    else:
        eng.bam_fit_step_batched(X, V, mean, cov, R if draws else None, eng.batched_regs(np.array(mb["regs"])), ref.JITTER,
                                 info, n_rev, seeds, ref.CALL)
    out = {n: t.cpu().numpy() for n, t in (("X", X), ("V", V), ("mean", mean), ("cov", cov), ("R", R))}
    out["info"], out["n_rev"] = eng.read_ints(info), eng.read_ints(n_rev)
    return out


_step = functools.lru_cache(maxsize=None)(_launch)       # the default strides: shared by the tests, never modified


def _one_shot(method, mb):
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    args = [eng.asarray(np.array(mb[n], copy=True)) for n in ("X", "V", "mu0", "S0")]
    if method == "gsm":
        mu, S = eng.gsm_update_batched(*args)
    else:
        mu, S = eng.bam_update_batched(*args, eng.batched_regs(np.array(mb["regs"])), ref.JITTER)
    return mu.cpu().numpy(), S.cpu().numpy()


def _check_step(method, D, B, nan_case, out, mb, worst):
    """every assertion of a STEP launch with draws"""
    assert np.array_equal(out["info"], ref.expected_codes(D, nan_case)), (D, B, out["info"])
    assert np.array_equal(out["info"], mb["codes"])
    assert np.array_equal(out["n_rev"], mb["n_rev0"] + (mb["codes"] != 0)), (D, B, out["n_rev"])
    assert np.array_equal(out["V"], mb["V"], equal_nan=True)                 # the scores are read only
    mu_o, S_o = _one_shot(method, mb)
    for k in range(K):
        Z = ref.draw(mb["seeds"][k], ref.CALL, B, D)
        where = (method, D, B, nan_case, k)
        if mb["codes"][k] == 0:
            assert np.array_equal(out["mean"][k], mu_o[k]) and np.array_equal(out["cov"][k], S_o[k]), where
            assert rel_err(out["mean"][k], mb["mu1"][k]) <= TOL[method], where
            assert rel_err(out["cov"][k], mb["S1"][k]) <= TOL[method], where
            Rk = out["R"][k]
            assert np.array_equal(np.tril(Rk, -1), np.zeros((D, D))) and (np.diag(Rk) > 0).all(), where
            e_r = ref.rel_err(Rk, ref.chol_ld(out["cov"][k]))
            e_x = ref.rel_err(out["X"][k], ref.sample(out["mean"][k], Rk, Z))
        else:
            assert np.array_equal(out["mean"][k], mb["mu0"][k]) and np.array_equal(out["cov"][k], mb["S0"][k]), where
            assert np.array_equal(out["R"][k], mb["R_kept"][k]), where
            e_r = 0.0
            e_x = ref.rel_err(out["X"][k], ref.sample(mb["mu0"][k], mb["R_kept"][k], Z))
        worst["R"], worst["X"] = max(worst["R"], e_r), max(worst["X"], e_x)
        assert e_r <= TOL_R and e_x <= TOL_X, (where, e_r, e_x)


@pytest.mark.parametrize("method", ["gsm", "bam"])
@pytest.mark.parametrize("D", ref.D_GRID)
def test_step_with_draws_on_the_mixed_batch(method, D):
    """(a) + (e): accepting problems write the one-shot update's bits, a factor that is the Cholesky factor of the covariance
    written and samples mean + Z R of them; planted problems report 1 + their pivot, keep mean, cov and R bit for bit and draw
    from the KEPT mean and factor; one accepting problem with a single NaN score entry reverts with code 1"""
    worst = {"R": 0.0, "X": 0.0}
    for B in _batch_sizes(method, D):
        for nan_case in (False, True):
            mb = ref.mixed_batch(method, D, B, nan_case)
            assert ref.distinguishable(mb, B, D) > 1e-3          # a wrong source of a revert's samples cannot pass TOL_X
            _check_step(method, D, B, nan_case, _step(method, D, B, nan_case), mb, worst)
    print(f"{method} D={D}: worst rel err R {worst['R']:.2e}  X' {worst['X']:.2e}")


@pytest.mark.parametrize("method", ["gsm", "bam"])
@pytest.mark.parametrize("D", ref.D_GRID)
def test_step_without_seeds_keeps_the_samples(method, D):
    """(b) forced-samples mode (no seeds, no R): the verdicts and accepted bits of the launch with draws, X untouched"""
    for B in _batch_sizes(method, D):
        for nan_case in (False, True):
            mb, a = ref.mixed_batch(method, D, B, nan_case), _step(method, D, B, nan_case)
            b = _launch(method, D, B, nan_case, draws=False)
            assert np.array_equal(b["info"], a["info"]) and np.array_equal(b["n_rev"], a["n_rev"]), (D, B)
            assert np.array_equal(b["mean"], a["mean"]) and np.array_equal(b["cov"], a["cov"]), (D, B)
            assert np.array_equal(b["X"], mb["X"]), (D, B)
            assert not np.array_equal(a["X"], mb["X"])


@pytest.mark.parametrize("D", ref.D_GRID)
def test_init_factor_code_and_first_samples(D):
    """(c) INIT: R against the long double factor, the planted covariances' codes, the first samples (draw 0) with keys whose
    high halves are set; the clean problems do not notice the planted ones"""
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    clean = [k for k in range(K) if k not in ref.PLANTED]
    worst = {"R": 0.0, "X": 0.0}
    for B in ref.B_GRID:
        mb = ref.mixed_batch("gsm", D, B)
        runs = []
        for sel in (list(range(K)), clean):
            mean, cov = eng.asarray(mb["mu0"][sel].copy()), eng.asarray(mb["S0"][sel].copy())
            R, X, info = eng.empty(len(sel), D, D), eng.empty(len(sel), B, D), eng.batched_counts([-1] * len(sel))
            eng.gsm_fit_init_batched(mean, cov, R, info, eng.batched_seeds([mb["seeds"][k] for k in sel]), X)
            assert np.array_equal(mean.cpu().numpy(), mb["mu0"][sel]) and np.array_equal(cov.cpu().numpy(), mb["S0"][sel])
            runs.append((R.cpu().numpy(), X.cpu().numpy(), eng.read_ints(info)))
        (R, X, info), (Rc, Xc, info_c) = runs
        assert np.array_equal(info, ref.expected_codes(D)) and np.array_equal(info_c, np.zeros(len(clean))), (D, B, info)
        assert np.array_equal(R[clean], Rc) and np.array_equal(X[clean], Xc), (D, B)
        R2, info2 = eng.empty(K, D, D), eng.batched_counts([-1] * K)
        eng.gsm_fit_init_batched(eng.asarray(mb["mu0"].copy()), eng.asarray(mb["S0"].copy()), R2, info2)        # no draws
        assert np.array_equal(R2.cpu().numpy()[clean], Rc) and np.array_equal(eng.read_ints(info2), info)
        for k in clean:
            want = ref.init_problem(mb["mu0"][k], mb["S0"][k], mb["seeds"][k], B)
            assert np.array_equal(np.tril(R[k], -1), np.zeros((D, D))) and (np.diag(R[k]) > 0).all()
            e_r = ref.rel_err(R[k], want["R"])
            from_device_R = ref.sample(mb["mu0"][k], R[k], ref.draw(mb["seeds"][k], 0, B, D))
            e_x = max(ref.rel_err(X[k], want["X"]), ref.rel_err(X[k], from_device_R))
            worst["R"], worst["X"] = max(worst["R"], e_r), max(worst["X"], e_x)
            assert e_r <= TOL_R and e_x <= TOL_X, (D, B, k, e_r, e_x)
    print(f"init D={D}: worst rel err R {worst['R']:.2e}  X {worst['X']:.2e}")


@pytest.mark.parametrize("D", [5, 16, 33, 64])
def test_bam_unpadded_strides_give_the_same_bits(D):
    """(d) the knob "bam_batched_pad" = 0 changes every LDS row stride of k_bam_batched, so addresses only: every output of
    the step equals the padded run bit for bit (and passes the same checks)"""
    import gsmvi_amd
    eng = gsmvi_amd.get_engine()
    for B in (2, 32):
        for nan_case in (False, True):
            a = _step("bam", D, B, nan_case)
            try:
                eng.set_tuning("bam_batched_pad", 0)
                b = _launch("bam", D, B, nan_case)
                b0 = _launch("bam", D, B, nan_case, draws=False)
            finally:
                eng.set_tuning("bam_batched_pad", 1)
            for name in a:
                assert np.array_equal(a[name], b[name], equal_nan=name == "V"), (D, B, nan_case, name)
            assert np.array_equal(b0["mean"], a["mean"]) and np.array_equal(b0["cov"], a["cov"])
            assert np.array_equal(b0["info"], a["info"]) and np.array_equal(b0["n_rev"], a["n_rev"])
            _check_step("bam", D, B, nan_case, b, ref.mixed_batch("bam", D, B, nan_case), {"R": 0.0, "X": 0.0})


def test_bam_boundary_shapes_sit_on_both_sides_of_the_switch():
    """(16, 22) is the last B at which four problems of D = 16 share a workgroup, (16, 23) the first with one: the library's
    own host arithmetic, read through the debug build's query in a child process (the pattern of test_bam_batched_cpu.py)"""
    from gsmvi_amd import _lib
    code = ("import ctypes as C, json, sys\n"
            "lib = C.CDLL(sys.argv[1])\n"
            "f = lib.gsmvi_debug_bam_batched_lds\n"
            "f.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]\n"
            "out = {}\n"
            "for D, B in ((16, 22), (16, 23), (16, 32), (16, 1), (17, 1)):\n"
            "    for pad in (0, 1):\n"
            "        n, p = C.c_size_t(0), C.c_int(0)\n"
            "        st = f(D, B, pad, C.byref(n), C.byref(p))\n"
            "        out[f'{D},{B},{pad}'] = [st, n.value, p.value]\n"
            "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.library_path(debug=True)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(v[0] == 0 for v in got.values())
    assert (ref.BAM_EXTRA[0], ref.BAM_EXTRA[1]) == ((16, 22), (16, 23))
    for pad in (0, 1):
        assert [got[f"{D},{B},{pad}"][2] for D, B in ((16, 1), (16, 22), (16, 23), (16, 32), (17, 1))] == [4, 4, 1, 1, 1]


# ---- (f) fits that revert and recover ---------------------------------------------------------------------------------------
def _targets(K, D, seed, cond=3.0):
    """the suite's well-conditioned Gaussian targets (test_gpu_batched.py::_targets)"""
    ms, covs, Ps = np.zeros((K, D)), np.zeros((K, D, D)), np.zeros((K, D, D))
    for k in range(K):
        rs = np.random.RandomState(seed + k)
        Q, _ = np.linalg.qr(rs.standard_normal((D, D)))
        c = (Q * np.logspace(0.0, np.log10(cond), D)) @ Q.T
        covs[k] = 0.5 * (c + c.T)
        ms[k], Ps[k] = rs.random_sample(D), np.linalg.inv(covs[k])
    return ms, covs, Ps


def _score(ms, Ps, when=(), rows=None):
    """host score of K (or, given 2-d samples, one) Gaussian targets, NaN in ``rows`` (or everywhere) on the calls numbered in
    ``when``: a fit calls its score once per iteration"""
    from oracle import gsm_oracle as orc
    count = [0]

    def lp_g(X):
        G = orc.gaussian_score(X, ms, Ps) if X.ndim == 2 else np.stack([orc.gaussian_score(X[k], ms[k], Ps[k])
                                                                        for k in range(X.shape[0])])
        if count[0] in when:
            G[slice(None) if rows is None else rows] = np.nan
        count[0] += 1
        return G
    return lp_g


SCHEDULE = (3, 4, 10)


@pytest.mark.parametrize("D,B", [(10, 2), (33, 4)])
def test_gsm_fit_reverts_and_recovers_like_the_single_fit(D, B):
    import gsmvi_amd
    K8, niter, j = 8, 60, 5
    ms, covs, Ps = _targets(K8, D, 7 * D)
    keys = [31 * k + 5 for k in range(K8)]
    f0, f1 = gsmvi_amd.GSMBatch(K8, D, None, _score(ms, Ps)), gsmvi_amd.GSMBatch(K8, D, None, _score(ms, Ps, SCHEDULE, j))
    m0, c0 = f0.fit(keys, batch_size=B, niter=niter, verbose=False)
    m1, c1 = f1.fit(keys, batch_size=B, niter=niter, verbose=False)
    assert f0.n_reverts.tolist() == [0] * K8 and f1.n_reverts.tolist() == [3 if k == j else 0 for k in range(K8)]
    single = gsmvi_amd.GSM(D, None, _score(ms[j], Ps[j], SCHEDULE))
    ms1, cs1 = single.fit(keys[j], batch_size=B, niter=niter, verbose=False, method="dense", rng="device")
    assert single.n_reverts == 3
    assert rel_err(m1[j], ms1) < 1e-8 and rel_err(c1[j], cs1) < 1e-8, (rel_err(m1[j], ms1), rel_err(c1[j], cs1))
    assert not np.array_equal(m1[j], m0[j])
    keep = [k for k in range(K8) if k != j]
    assert np.array_equal(m1[keep], m0[keep]) and np.array_equal(c1[keep], c0[keep])


@pytest.mark.parametrize("D,B", [(10, 2), (33, 4)])
def test_bam_fit_reverts_and_recovers(D, B):
    """BaM has no retry-free single fit to compare with (BaMBatch.fit's docstring): the problem alone, K = 1, stands in"""
    import gsmvi_amd
    K8, niter, j = 8, 60, 5
    ms, covs, Ps = _targets(K8, D, 7 * D)
    keys = [31 * k + 5 for k in range(K8)]
    regf = lambda i: 100.0 / (1 + i)
    f0, f1 = gsmvi_amd.BaMBatch(K8, D, None, _score(ms, Ps)), gsmvi_amd.BaMBatch(K8, D, None, _score(ms, Ps, SCHEDULE, j))
    m0, c0 = f0.fit(keys, regf, batch_size=B, niter=niter, verbose=False)
    m1, c1 = f1.fit(keys, regf, batch_size=B, niter=niter, verbose=False)
    assert f0.n_reverts.tolist() == [0] * K8 and f1.n_reverts.tolist() == [3 if k == j else 0 for k in range(K8)]
    keep = [k for k in range(K8) if k != j]
    assert np.array_equal(m1[keep], m0[keep]) and np.array_equal(c1[keep], c0[keep])
    assert not np.array_equal(m1[j], m0[j]) and np.isfinite(m1[j]).all() and np.isfinite(c1[j]).all()
    alone = gsmvi_amd.BaMBatch(1, D, None, _score(ms[j:j + 1], Ps[j:j + 1], SCHEDULE))
    ma, ca = alone.fit([keys[j]], regf, batch_size=B, niter=niter, verbose=False)
    assert alone.n_reverts.tolist() == [3]
    assert np.array_equal(ma[0], m1[j]) and np.array_equal(ca[0], c1[j])
