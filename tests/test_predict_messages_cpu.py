"""The host messages of the three draw-based predictives (``predict_softmax_batched``, ``predict_negbin_batched``,
``predict_ordinal_batched``), character for character: exception type and full text of every argument check their docstrings
list.  The three functions share their checks; what a caller reads must not depend on which one raised it, and must not change
when the checks move.  No GPU: stand-in engines, and every check fires before any engine call."""
import re

import numpy as np
import pytest

import negbin_predict_ref as nref
import ordinal_predict_ref as oref
import softmax_predict_ref as sref
import gsmvi_amd

K, N, M, CLASSES = 3, 12, 7, 4
KEYS = [1, 2, 3]


def _softmax():
    rs = np.random.default_rng(3)
    P = 2
    tgt = gsmvi_amd.BatchedSoftmaxTarget(rs.standard_normal((K, N, P)), rs.integers(0, CLASSES, (K, N)), CLASSES, 1.0,
                                         engine=sref.StandInEngine())
    return tgt, rs.standard_normal((K, M, P)), rs.integers(0, CLASSES, (K, M))


def _negbin():
    rs = np.random.default_rng(4)
    P = 3
    tgt = gsmvi_amd.BatchedNegBinomialTarget(rs.standard_normal((K, N, P)), rs.poisson(3.0, (K, N)).astype(np.float64), 1.0,
                                             log_size_mean=1.5, log_size_precision=1.0, engine=nref.StandInEngine())
    return tgt, rs.standard_normal((K, M, P)), rs.poisson(3.0, (K, M)).astype(np.float64)


def _ordinal():
    rs = np.random.default_rng(5)
    P = 3
    tgt = gsmvi_amd.BatchedOrdinalTarget(rs.standard_normal((K, N, P)), rs.integers(0, CLASSES, (K, N)), CLASSES, 1.0, 1.0,
                                         engine=oref.StandInEngine())
    return tgt, rs.standard_normal((K, M, P)), rs.integers(0, CLASSES, (K, M))


FAMILIES = {
    "softmax": (gsmvi_amd.predict_softmax_batched, "BatchedSoftmaxTarget", _softmax),
    "negbin": (gsmvi_amd.predict_negbin_batched, "BatchedNegBinomialTarget", _negbin),
    "ordinal": (gsmvi_amd.predict_ordinal_batched, "BatchedOrdinalTarget", _ordinal),
}
LABELS_RANGE = f"y: labels that are not integers in 0 .. num_classes - 1 = {CLASSES - 1} in the valid rows of problems [2]"
Y_RANGE = {"softmax": LABELS_RANGE, "ordinal": LABELS_RANGE, "negbin": "y: values negative or non-finite in the valid rows of problems [2]"}


def _raises(exc, text, fn, *args, **kw):
    with pytest.raises(exc, match="^" + re.escape(text) + "$") as e:
        fn(*args, **kw)
    assert type(e.value) is exc


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_argument_check_by_type_and_full_text(family):
    fn, cls, make = FAMILIES[family]
    name = fn.__name__
    tgt, A_new, y_new = make()
    eng = tgt.engine
    P, D = tgt.P, tgt.D
    mean, cov = np.zeros((K, D)), np.tile(np.eye(D), (K, 1, 1))
    eng.calls.clear()
    pr = lambda *a, **kw: fn(tgt, *a, **kw)      # noqa: E731

    # the target's type: every other class, the other two families' among them
    for other, what in ((3, "int"), (None, "NoneType"), (tgt.lp, "method")):
        _raises(TypeError, f"{name}: target must be a {cls}, got {what}", fn, other, mean, cov, A_new, KEYS)
    for fam, (_, ocls, omake) in FAMILIES.items():
        if fam != family:
            _raises(TypeError, f"{name}: target must be a {cls}, got {ocls}", fn, omake()[0], mean, cov, A_new, KEYS)
    # weights
    for w, shown in (("PSIS", "'PSIS'"), (None, "None"), (1, "1")):
        _raises(ValueError, f"{name}: weights: expected 'uniform' or 'psis', got {shown}", pr, mean, cov, A_new, KEYS, weights=w)
    # A_new
    head = f"{name}: A_new: expected shape (K, M, P) with K = {K}, P = {P} and M >= 1, got "
    _raises(ValueError, head + f"({K}, {M}, 1)", pr, mean, cov, A_new[:, :, :1], KEYS)
    _raises(ValueError, head + f"(2, {M}, {P})", pr, mean, cov, A_new[:2], KEYS)
    _raises(ValueError, head + f"({M}, {P})", pr, mean, cov, A_new[0], KEYS)
    _raises(ValueError, head + f"({K}, 0, {P})", pr, mean, cov, A_new[:, :0], KEYS)
    # mean, cov
    _raises(ValueError, f"{name}: mean must be (K, D) = ({K}, {D}) of the target, got ({K}, {D - 1})", pr, mean[:, :D - 1], cov, A_new,
            KEYS)
    _raises(ValueError, f"{name}: cov must be ({K}, {D}, {D}), got ({K}, {D - 1}, {D})", pr, mean, cov[:, :D - 1], A_new, KEYS)
    # y: shape and range (a value beyond counts is not looked at)
    _raises(ValueError, f"{name}: y: expected shape (K, M) = ({K}, {M}), got ({K}, 3)", pr, mean, cov, A_new, KEYS, y=y_new[:, :3])
    bad_y = y_new.copy()
    bad_y[2, 1] = -1
    _raises(ValueError, f"{name}: {Y_RANGE[family]}", pr, mean, cov, A_new, KEYS, y=bad_y)
    if family == "negbin":
        nan_y = y_new.copy()
        nan_y[2, 1] = np.nan
        _raises(ValueError, f"{name}: {Y_RANGE[family]}", pr, mean, cov, A_new, KEYS, y=nan_y)
    else:
        high_y = y_new.copy()
        high_y[2, 1] = CLASSES
        _raises(ValueError, f"{name}: {Y_RANGE[family]}", pr, mean, cov, A_new, KEYS, y=high_y)
        _raises(ValueError, f"{name}: {Y_RANGE[family]}", pr, mean, cov, A_new, KEYS, y=np.where(bad_y == -1, 0.5, bad_y))
        _raises(ValueError, f"{name}: y: expected integer labels (an integer dtype, or floats with integral values), got dtype bool",
                pr, mean, cov, A_new, KEYS, y=y_new.astype(bool))
    # offset (softmax has none)
    if family != "softmax":
        _raises(ValueError, f"{name}: offset: expected shape (K, M) = ({K}, {M}), got ({K}, 3)", pr, mean, cov, A_new, KEYS,
                offset=np.zeros((K, 3)))
        bad_o = np.zeros((K, M))
        bad_o[1, 2] = np.inf
        _raises(ValueError, f"{name}: offset: non-finite values in the valid rows of problems [1]", pr, mean, cov, A_new, KEYS,
                offset=bad_o)
        # counts come before y, y before offset
        _raises(ValueError, f"{name}: {Y_RANGE[family]}", pr, mean, cov, A_new, KEYS, y=bad_y, offset=bad_o)
    # counts
    _raises(ValueError, f"{name}: counts: values outside 0 .. M = {M} for problems [1]", pr, mean, cov, A_new, KEYS,
            counts=np.array([1, M + 1, 2]))
    _raises(ValueError, f"{name}: counts: values outside 0 .. M = {M} for problems [0, 2]", pr, mean, cov, A_new, KEYS,
            counts=np.array([-1, M, M + 3]))
    _raises(ValueError, f"{name}: counts: expected {K} integers, got shape ({K},), dtype float64", pr, mean, cov, A_new, KEYS,
            counts=np.array([1.0, 2.0, 2.0]))
    _raises(ValueError, f"{name}: counts: expected {K} integers, got shape (2,), dtype int64", pr, mean, cov, A_new, KEYS,
            counts=np.array([1, 2]))
    _raises(ValueError, f"{name}: counts: values outside 0 .. M = {M} for problems [1]", pr, mean, cov, A_new, KEYS, y=bad_y,
            counts=np.array([1, M + 1, 2]))
    # keys
    _raises(ValueError, f"{name}: 2 keys for K = {K} problems", pr, mean, cov, A_new, [1, 2])
    _raises(ValueError, f"{name}: 4 keys for K = {K} problems", pr, mean, cov, A_new, np.arange(4))
    # num_draws
    for S in (4, 4097, 5.5):
        _raises(ValueError, f"{name}: num_draws = {S} is outside 5 <= num_draws <= 4096", pr, mean, cov, A_new, KEYS, num_draws=S)
        _raises(ValueError, f"{name}: num_draws = {S} is outside 5 <= num_draws <= 4096", pr, mean, cov, A_new, KEYS, num_draws=S,
                weights="psis")
    # a psis of the wrong kind, with either weights
    for w in ("uniform", "psis"):
        _raises(ValueError, f"{name}: psis must be a PSISBatchedResult of psis_batched(..., as_torch=True), got dict", pr, mean, cov,
                A_new, KEYS, psis=dict(samples=None), weights=w)
        _raises(ValueError, f"{name}: psis must be a PSISBatchedResult of psis_batched(..., as_torch=True), got ndarray", pr, mean,
                cov, A_new, KEYS, psis=np.zeros((K, 8, D)), weights=w)
    assert not [c for c in eng.calls if isinstance(c, tuple)]                   # nothing reached the engine
