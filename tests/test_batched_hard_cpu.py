"""The hard batches of tests/batched_hard_ref.py without a GPU: the restatements against the pinned oracles, the conditions on
the inputs that tests/test_gpu_batched_hard.py relies on (every problem accepts in long double, every pivot examined clear of
zero, BaM's Newton-Schulz bound, the long double BaM result solving its defining equation), the float64 noise floor of every
case as one table, what building it all costs, and that a value rounded through float32 at one place exceeds the new bars.

Measured on the development machine's CPU: ``build_all`` from a cold cache takes 8 to 11 s (D = 64 BaM, the long double
Jacobi, is 4 s of it).

Planted float32 roundings: each of (a) rho, (b) S0 g_b, (c) e_b, (d) the factorisation's multipliers exceeds 16 x floor by a
factor of 1e7 to 2e8 somewhere, and the suite's fixed bars on the easy states (1e-12 on mu and S, 1e-11 on R and X, 1e-9 on
log q) would have caught each of the four as well; the table is in the docstring of tests/batched_hard_ref.py."""
import numpy as np
import pytest

import batched_hard_ref as ref
import batched_step_ref as step
from oracle import bam_oracle as borc
from oracle import gsm_oracle as orc

LD = ref.LD
SHAPES = [(D, B) for D in ref.D_GRID for B in ref.B_GRID]
GSM_OUT = ("mu", "S", "dmu", "dS", "R0", "X0", "R1", "X1", "logq", "klX", "kllogq")


def test_building_every_reference_stays_under_twenty_seconds():
    for f in (ref.batch, ref.gsm_case, ref.bam_case, ref.traj_inputs, ref.traj_case):
        f.cache_clear()
    seconds = ref.build_all()
    print(f"build_all: {seconds:.1f} s")
    assert seconds < 20.0, seconds


def test_restatements_agree_with_the_pinned_oracles():
    X, V, mu0, S0 = (a[0] for a in step.states(1, 8, 33, 5))
    mu_o, S_o = orc.gsm_update_faithful(X, V, mu0, S0)
    for fn, (mu_r, S_r) in ((ref.gsm_faithful, (mu_o, S_o)), (ref.gsm_alg, orc.gsm_update_batched(X, V, mu0, S0))):
        mu, S, dmu, dS = fn(X, V, mu0, S0, np.float64)
        assert mu.dtype == np.float64 and ref.rel_err(mu, mu_r) < 4e-16 and ref.rel_err(S, S_r) < 4e-16
        assert dmu.dtype == LD and np.array_equal(np.asarray(dmu, dtype=np.float64), mu - mu0)
        mu_l, S_l, _, _ = fn(X, V, mu0, S0, LD)
        assert mu_l.dtype == LD and S_l.dtype == LD and ref.rel_err(mu_o, mu_l) < 1e-15 and ref.rel_err(S_o, S_l) < 1e-15
    a, b = ref.gsm_faithful(X, V, mu0, S0, LD), ref.gsm_alg(X, V, mu0, S0, LD)
    assert ref.rel_err(a[0], b[0]) < 1e-18 and ref.rel_err(a[1], b[1]) < 1e-18           # two orders, one answer
    R = step.chol_ld(S0)
    assert ref.rel_err(ref.chol_right(S0, LD), R) < 1e-18 and ref.rel_err(ref.chol_left(S0, LD), R) < 1e-18
    assert ref.chol_right(S0, np.float64).dtype == np.float64 and ref.rel_err(ref.chol_right(S0, np.float64), R) < 1e-14
    assert ref.rel_err(ref.chol_left(S0, np.float64), np.linalg.cholesky(S0).T) < 1e-14

    def mvn_logpdf(Y, m, S):
        r = Y - m[None, :]
        return -0.5 * np.einsum("bi,bi->b", r, np.linalg.solve(S, r.T).T) - 0.5 * np.linalg.slogdet(S)[1] \
            - 0.5 * len(m) * np.log(2 * np.pi)
    Y = mu0[None, :] + np.random.RandomState(1).standard_normal((24, 33))
    want = mvn_logpdf(Y, mu0, S0).sum()
    for factor in (ref.chol_right, ref.chol_left):
        assert abs(float(ref.logq_points(mu0, S0, Y, LD, factor)) - want) < 1e-11 * abs(want)
    Z = ref.kl_rows(2 ** 40 + 3, 3, 24, 5)
    assert np.array_equal(Z, orc.philox_randn(2 ** 40 + 3, 3, 120).reshape(24, 5))      # the plain layout, no padded column
    Xd, lq = ref.kl_draw(mu0[:5], S0[:5, :5], Z, LD)
    assert ref.rel_err(Xd, step.sample(mu0[:5], step.chol_ld(S0[:5, :5]), Z)) < 1e-18
    assert abs(float(lq) - mvn_logpdf(np.asarray(Xd, dtype=np.float64), mu0[:5], S0[:5, :5]).sum()) < 1e-11 * abs(float(lq))
    A = np.random.RandomState(2).standard_normal((9, 9))
    w, W = ref.jacobi_eigh(A + A.T, LD)
    assert ref.rel_err((W * w[None, :]) @ W.T, np.asarray(A + A.T, dtype=LD)) < 1e-17
    assert ref.rel_err(W.T @ W, np.eye(9)) < 1e-17 and ref.rel_err(np.sort(w), np.linalg.eigvalsh(A + A.T)) < 1e-14
    mu_b, S_b = ref.bam_update(X, V, mu0, S0, 2.5, LD)
    mu_o, S_o = borc.bam_lowrank_update_exact(X, V, mu0, S0, 2.5)
    assert ref.rel_err(mu_o, mu_b) < 1e-12 and ref.rel_err(S_o, S_b) < 1e-12
    mu_f, S_f = borc.bam_update_full(X, V, mu0, S0, 2.5)                                # bam.py:31-69, the full-rank form
    assert ref.rel_err(mu_f, mu_b) < 1e-10 and ref.rel_err(S_f, S_b) < 1e-10


@pytest.mark.parametrize("D,B", SHAPES)
def test_gsm_inputs_meet_their_conditions(D, B):
    b = ref.batch(D, B)
    assert b["X"].shape == (ref.K, B, D) and not b["S0"].flags.writeable
    assert all(np.array_equal(S, S.T) for S in b["S0"]) and all(np.isfinite(b[n]).all() for n in b)
    want, floor = ref.gsm_case(D, B)
    for k, fam in enumerate(ref.FAMILIES):
        assert want[k]["info0"] == 0 and want[k]["info1"] == 0, (fam, "accepts in long double")
        assert want[k]["margin0"] >= ref.pivot_margin(D) and want[k]["margin1"] >= ref.pivot_margin(D), (fam, want[k]["margin0"],
                                                                                                       want[k]["margin1"])
        assert all(ref.FLOOR_MIN <= floor[k][n] < 1e-2 for n in GSM_OUT), (fam, floor[k])
    # the families are what they say: far samples, a tiny increment of the nearly converged problems, the units
    sig = lambda k: float(np.max(np.abs(b["X"][k] - b["mu0"][k][None, :]) / np.sqrt(np.diag(b["S0"][k]))[None, :]))  # noqa: E731
    assert sig(ref.FAMILIES.index("far")) > 30 and sig(0) < 6      # the largest of B D draws of 100 N(0, 1) / sigma_i
    for fam in ("near_c100", "near_c1e8"):
        k = ref.FAMILIES.index(fam)
        assert ref.rel_err(want[k]["S"], b["S0"][k]) < 1e-4 and float(np.max(np.abs(want[k]["dS"]))) > 0
    assert abs(np.max(np.diag(b["S0"][4])) / np.max(np.diag(b["S0"][5])) / 1e-16 - 1) < 10
    d = np.diag(b["S0"][ref.FAMILIES.index("graded")])
    assert d[-1] / d[0] > 1e10
    for k, c in ((1, 1e4), (2, 1e8), (3, 1e12), (10, 1e8)):
        w = np.asarray(ref.jacobi_eigh(b["S0"][k], LD)[0], dtype=np.float64)
        assert 0.3 * c < w.max() / w.min() < 3 * c, (k, w.max() / w.min())


@pytest.mark.parametrize("D,B", SHAPES)
def test_bam_inputs_meet_their_conditions(D, B):
    want, floor = ref.bam_case(D, B)
    kept = [k for k in range(ref.K) if want[k] is not None]
    assert [ref.FAMILIES[k] for k in kept] == list(ref.bam_families(D))
    assert {ref.bam_reg(k) for k in kept} == set(ref.BAM_REGS)
    for k in kept:
        fam = ref.FAMILIES[k]
        assert want[k]["res"] < 1e-17, (fam, want[k]["res"])                 # the long double S' solves S U S + S = V
        assert want[k]["info"] == 0 and want[k]["margin"] >= ref.pivot_margin(D), (fam, want[k]["margin"])
        assert want[k]["ns"] < 0.01 * ref.NS_BOUND, (fam, want[k]["ns"])     # the Newton-Schulz chain closes: no flagged case
        assert ref.bam_resolved(floor[k]) == (not (fam == "steep" and B == 2)), (fam, floor[k])
        assert ref.bam_may_flag(want[k]["ns"]) == (fam == "steep"), (fam, want[k]["ns"])     # no other family may be flagged


def _table(rows, header):
    return "\n".join([header] + rows)


def test_print_the_floor_table():
    """the float64 floors, the largest over the shapes, one row per family"""
    worst = {fam: {n: 0.0 for n in GSM_OUT + ("bam_mu", "bam_S", "bam_res")} for fam in ref.FAMILIES}
    for D, B in SHAPES:
        _, fg = ref.gsm_case(D, B)
        _, fb = ref.bam_case(D, B)
        for k, fam in enumerate(ref.FAMILIES):
            for n in GSM_OUT:
                worst[fam][n] = max(worst[fam][n], fg[k][n])
            if fb[k] is not None and ref.bam_resolved(fb[k]):
                for n in ("mu", "S", "res"):
                    worst[fam]["bam_" + n] = max(worst[fam]["bam_" + n], fb[k][n])
    cols = ("mu", "S", "dmu", "dS", "R0", "R1", "X0", "X1", "logq", "kllogq", "bam_mu", "bam_S", "bam_res")
    rows = [f"{fam:10s} " + " ".join(f"{worst[fam][n]:8.1e}" for n in cols) for fam in ref.FAMILIES]
    print(_table(rows, f"{'family':10s} " + " ".join(f"{n:>8s}" for n in cols)))
    traj = []
    for method, (D, B) in (("gsm", ref.TRAJ_SHAPES[0]), ("gsm", ref.TRAJ_SHAPES[1]), ("bam", ref.TRAJ_SHAPES[0])):
        t = ref.traj_case(method, D, B)
        traj.append(f"trajectory {method} D={D} B={B}: mean " + " ".join(f"{o['floor_mean']:.1e}" for o in t)
                    + " | cov " + " ".join(f"{o['floor_cov']:.1e}" for o in t))
    print("\n".join(traj))
    assert worst["easy"]["S"] == ref.FLOOR_MIN and worst["cond1e12"]["R0"] > 100 * ref.FLOOR_MIN


@pytest.mark.parametrize("method,D,B", [("gsm",) + ref.TRAJ_SHAPES[0], ("gsm",) + ref.TRAJ_SHAPES[1], ("bam",) + ref.TRAJ_SHAPES[0]])
def test_trajectories_accept_every_step_in_every_arithmetic(method, D, B):
    for o in ref.traj_case(method, D, B):
        assert o["reverts"] == 0 and o["reverts64"] == [0, 0]
        assert o["floor_mean"] < 1e-6 and o["floor_cov"] < 1e-6 and np.isfinite(np.asarray(o["cov"], dtype=np.float64)).all()


# ---- sensitivity: the new bars bite --------------------------------------------------------------------------------------------
OLD_BAR = {"mu": 1e-12, "S": 1e-12, "R": 1e-11, "X": 1e-11, "logq": 1e-9}     # the suite's fixed bars on the easy states


def _planted_errors(plant, D, B):
    """{(family, output): (err, floor)} of the float64 restatement with one float32 rounding planted"""
    b = ref.batch(D, B)
    want, floor = ref.gsm_case(D, B)
    out = {}
    for k, fam in enumerate(ref.FAMILIES):
        X, V, mu0, S0 = (b[n][k] for n in ("X", "V", "mu0", "S0"))
        if plant == "mult":
            R = ref.chol_right(S0, np.float64, plant=True)
            Z = step.draw(ref.SEEDS[k], 0, B, D)
            got = {"R0": R, "X0": ref.sample_in(mu0, R, Z, np.float64),
                   "logq": ref._logq_from(ref._whiten(R, b["Y"][k], mu0, np.float64), R, np.float64)}
        else:
            got = dict(zip(("mu", "S", "dmu", "dS"), ref.gsm_alg(X, V, mu0, S0, np.float64, plant=plant)))
        for n, v in got.items():
            out[(fam, n)] = (ref.rel_err(v, want[k][n]), floor[k][n])
    return out


@pytest.mark.parametrize("plant", ["rho", "Sg", "e", "mult"])
def test_planted_float32_roundings_are_caught(plant):
    """(a) rho, (b) S0 g_b, (c) e_b, (d) the multipliers of the factorisation, each rounded through float32 in the float64
    restatement: the error exceeds M x floor on at least one output of at least one family"""
    best, easy_old = (0.0, None), False
    for D, B in ((17, 2), (64, 32)):
        for (fam, n), (err, floor) in _planted_errors(plant, D, B).items():
            if err / floor > best[0]:
                best = (err / floor, (fam, n, D, B, err, floor))
            if fam == "easy" and n.rstrip("01") in OLD_BAR and err > OLD_BAR[n.rstrip("01")]:
                easy_old = True
    print(f"planted {plant}: largest err / floor {best[0]:.1e} at {best[1]}; the fixed bars on the easy states "
          f"{'would' if easy_old else 'would NOT'} have caught it")
    assert best[0] > ref.M_BAR, best
