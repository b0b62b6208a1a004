"""The batched fit step without a GPU: the conditions on the mixed batch of tests/batched_step_ref.py that
tests/test_gpu_batched_step.py relies on (expected codes, the pivot margin, positive definite accepting problems,
distinguishable sources of a reverting problem's samples), for every case the GPU tests launch; the reference's own pieces;
and the oracle-backed batched engines of tests/engines.py on the same batch (the pivot code, the kept state, the draws)."""
import numpy as np
import pytest

import batched_step_ref as ref
from engines import OracleBatchedBaMEngine, OracleBatchedEngine

CASES = [("gsm", D, B) for D in ref.D_GRID for B in ref.B_GRID] + [("bam", D, B) for D in ref.D_GRID for B in ref.B_GRID] \
    + [("bam", D, B) for D, B in ref.BAM_EXTRA]


def test_verdict_and_factor_on_known_matrices():
    S = np.array([[4.0, 2.0, 0.0], [2.0, 5.0, 3.0], [0.0, 3.0, 10.0]])
    info, piv = ref.verdict(S)
    assert info == 0 and np.allclose(piv.astype(np.float64), [4.0, 4.0, 7.75], rtol=1e-15)
    R = ref.chol_ld(S)
    assert np.array_equal(np.tril(R, -1), np.zeros((3, 3))) and ref.rel_err(R.T @ R, S) < 1e-18
    assert ref.rel_err(R, np.linalg.cholesky(S).T) < 1e-15
    for c in range(3):
        info, piv = ref.verdict(ref.plant(S, c))
        assert info == c + 1 and len(piv) == c + 1 and np.allclose(float(piv[c]), -[4.0, 4.0, 7.75][c], rtol=1e-15)
        assert np.array_equal(ref.chol_ld(ref.plant(S, c), rows=c)[:c], R[:c])
    for bad in (np.nan, np.inf, -np.inf, 0.0):
        T = S.copy()
        T[1, 1] = bad
        assert ref.verdict(T)[0] == 2
    T = S.copy()
    T[0, 2] = np.nan                                        # an off-diagonal NaN reaches a later pivot
    assert ref.verdict(T)[0] == 3
    assert ref.verdict(np.full((4, 4), np.nan))[0] == 1


def test_draw_is_the_fits_layout():
    from oracle import gsm_oracle as orc
    for D in (1, 4, 5):
        Dz = D + (D & 1)
        Z = ref.draw(2 ** 63 + 11, ref.CALL, 3, D)
        assert Z.shape == (3, D) and np.array_equal(Z, orc.philox_randn(2 ** 63 + 11, ref.CALL, 3 * Dz).reshape(3, Dz)[:, :D])
    assert ref.CALL >> 32 and ref.CALL & 0xFFFFFFFF and not np.array_equal(ref.draw(7, ref.CALL, 2, 4), ref.draw(7, 5, 2, 4))
    assert any(s >> 32 and s & 0xFFFFFFFF for s in ref.SEEDS) and 2 ** 40 + 3 in ref.SEEDS and 2 ** 63 + 11 in ref.SEEDS


@pytest.mark.parametrize("nan_case", [False, True])
@pytest.mark.parametrize("method,D,B", CASES)
def test_mixed_batch_meets_its_conditions(method, D, B, nan_case):
    mb = ref.mixed_batch(method, D, B, nan_case)
    assert np.array_equal(mb["codes"], ref.expected_codes(D, nan_case))
    for k in range(ref.K):
        if nan_case and k == ref.NAN_SLOT:
            assert np.isnan(mb["S1"][k]).all()              # every entry: no order of elimination can find a good pivot first
            continue
        assert len(mb["pivots"][k]) == (mb["codes"][k] or D)
        assert ref.margin(mb["S1"][k], mb["pivots"][k]) >= ref.MARGIN, k      # round-off cannot move a verdict
        assert np.isfinite(mb["S1"][k]).all() and np.isfinite(mb["mu1"][k]).all()
        if mb["codes"][k] == 0:
            if method == "bam":
                assert np.array_equal(mb["S1"][k], mb["S1"][k].T)
            assert np.linalg.eigvalsh(0.5 * (mb["S1"][k] + mb["S1"][k].T)).min() > 0.0
    assert mb["reverting"] == sorted(ref.PLANTED + ((ref.NAN_SLOT,) if nan_case else ()))
    assert ref.distinguishable(mb, B, D) > 1e-3             # a wrong source cannot pass the samples' 1e-11
    for k in range(ref.K):                                  # the kept factor is an opaque upper triangle, unrelated to cov
        Rk = mb["R_kept"][k]
        assert np.array_equal(np.tril(Rk, -1), np.zeros((D, D))) and (np.diag(Rk) > 0).all()
        assert ref.rel_err(Rk.T @ Rk, mb["S0"][k]) > 1e-2


def _run_engine(method, mb, with_seeds=True):
    """one step of the oracle-backed engine on the mixed batch, as the GPU test launches it"""
    X, V, mean, cov, R = (np.array(mb[n], copy=True) for n in ("X", "V", "mu0", "S0", "R_kept"))
    info, n_rev = np.zeros(ref.K, dtype=np.int64), np.array(mb["n_rev0"], dtype=np.int64)
    seeds = np.array([int(s) for s in mb["seeds"]], dtype=np.uint64) if with_seeds else None
    if method == "gsm":
        OracleBatchedEngine().gsm_fit_step_batched(X, V, mean, cov, R if with_seeds else None, info, n_rev, seeds, ref.CALL)
    else:
        OracleBatchedBaMEngine().bam_fit_step_batched(X, V, mean, cov, R if with_seeds else None, np.array(mb["regs"]), ref.JITTER,
                                                      info, n_rev, seeds, ref.CALL)
    return X, mean, cov, R, info, n_rev


@pytest.mark.parametrize("method", ["gsm", "bam"])
@pytest.mark.parametrize("D", ref.D_GRID)
def test_oracle_engines_report_the_pivot_code_and_draw_from_the_kept_state(method, D):
    B = 2
    for nan_case in (False, True):
        mb = ref.mixed_batch(method, D, B, nan_case)
        X, mean, cov, R, info, n_rev = _run_engine(method, mb)
        assert np.array_equal(info, mb["codes"])
        assert np.array_equal(n_rev, mb["n_rev0"] + (mb["codes"] != 0))
        for k in range(ref.K):
            Z = ref.draw(mb["seeds"][k], ref.CALL, B, D)
            if mb["codes"][k]:
                assert np.array_equal(mean[k], mb["mu0"][k]) and np.array_equal(cov[k], mb["S0"][k])
                assert np.array_equal(R[k], mb["R_kept"][k])
                assert ref.rel_err(X[k], ref.sample(mb["mu0"][k], mb["R_kept"][k], Z)) <= 1e-14
            else:
                tol = 1e-12 if method == "gsm" else 1e-8
                assert ref.rel_err(mean[k], mb["mu1"][k]) <= tol and ref.rel_err(cov[k], mb["S1"][k]) <= tol
                assert ref.rel_err(R[k], ref.chol_ld(cov[k])) <= 1e-13
                assert ref.rel_err(X[k], ref.sample(mean[k], R[k], Z)) <= 1e-14
        X2, mean2, cov2, _, info2, n_rev2 = _run_engine(method, mb, with_seeds=False)
        assert np.array_equal(info2, info) and np.array_equal(n_rev2, n_rev)
        assert np.array_equal(mean2, mean) and np.array_equal(cov2, cov) and np.array_equal(X2, mb["X"], equal_nan=True)


def test_oracle_engines_init_reports_the_pivot_code():
    D, B = 7, 2
    mb = ref.mixed_batch("gsm", D, B)
    for eng in (OracleBatchedEngine(), OracleBatchedBaMEngine()):
        R, info, X = np.zeros((ref.K, D, D)), np.zeros(ref.K, dtype=np.int64), np.zeros((ref.K, B, D))
        eng.gsm_fit_init_batched(np.array(mb["mu0"]), np.array(mb["S0"]), R, info, np.array(mb["seeds"], dtype=np.uint64), X)
        assert np.array_equal(info, ref.expected_codes(D))
        for k in range(ref.K):
            if k not in ref.PLANTED:
                out = ref.init_problem(mb["mu0"][k], mb["S0"][k], mb["seeds"][k], B)
                assert ref.rel_err(R[k], out["R"]) <= 1e-13 and ref.rel_err(X[k], out["X"]) <= 1e-13


def test_step_problem_restates_the_launch():
    D, B = 10, 2
    for method in ("gsm", "bam"):
        mb = ref.mixed_batch(method, D, B)
        for k in (0, 1):
            reg = None if method == "gsm" else mb["regs"][k]
            out = ref.step_problem(method, mb["X"][k], mb["V"][k], mb["mu0"][k], mb["S0"][k], mb["R_kept"][k], 3 + k,
                                   mb["seeds"][k], ref.CALL, reg, ref.JITTER)
            assert out["info"] == mb["codes"][k] and out["n_rev"] == 3 + k + (k == 1)
            Z = ref.draw(mb["seeds"][k], ref.CALL, B, D)
            if k == 1:
                assert np.array_equal(out["mean"], mb["mu0"][k]) and np.array_equal(out["cov"], mb["S0"][k])
                assert np.array_equal(out["R"], mb["R_kept"][k])
                assert ref.rel_err(out["X"], ref.sources(mb, k, B, D)[0]) == 0.0
            else:
                assert ref.rel_err(out["R"].T @ out["R"], mb["S1"][k]) < 1e-17
                assert ref.rel_err(out["X"], ref.sample(mb["mu1"][k], out["R"], Z)) == 0.0
