"""The host messages of the two batched GLM target classes and of ``laplace_init_batched``, character for character: the
classes share one constructor and one ``predict``, and what a caller reads must not depend on which class raised it."""
import numpy as np
import pytest

import glm_batched_ref as gref
import logistic_batched_ref as lref
from gsmvi_amd import BatchedGLMTarget, BatchedLogisticTarget, laplace_init_batched

K, N, D, M = 3, 12, 4, 5
A, Y, COUNTS, LAM, _ = lref.make_inputs(K, N, D, 2)                   # counts = [12, 8, 5]


def _message(exc, fn, *args, **kw):
    with pytest.raises(exc) as e:
        fn(*args, **kw)
    return str(e.value)


def _logistic(**kw):
    return BatchedLogisticTarget(**{**dict(A=A, y=Y, prior_precision=LAM, counts=COUNTS, engine=gref.RestatementEngine()), **kw})


def _glm(family="logistic", **kw):
    return BatchedGLMTarget(**{**dict(A=A, y=Y, family=family, prior_precision=LAM, counts=COUNTS,
                                      engine=gref.RestatementEngine()), **kw})


def _bad(a, k, n, v):
    b = np.array(a, dtype=np.float64)
    b[k, n] = v
    return b


def test_constructor_messages_of_both_classes():
    for mk in (_logistic, _glm):
        assert _message(ValueError, mk, y=Y[:, :11]) == "y: expected shape (K, N) = (3, 12), got (3, 11)"
        assert _message(ValueError, mk, counts=[1, 2]) == "counts: expected 3 integers, got shape (2,), dtype int64"
        assert _message(ValueError, mk, counts=[12, 13, 1]) == "counts: values outside 0 .. N = 12 for problems [1]"
        assert _message(ValueError, mk, prior_precision=[0.1, 0.2]) == \
            "prior_precision: expected a number or 3 values, got shape (2,)"
        for lam in (-0.5, [0.1, np.nan, 0.3]):
            assert _message(ValueError, mk, prior_precision=lam) == "prior_precision: expected finite values >= 0"
    assert _message(ValueError, _logistic, y=_bad(Y, 1, 3, 1.5)) == \
        "y: values outside [0, 1] or non-finite in the valid rows of problems [1]"
    assert _message(ValueError, _glm, y=_bad(Y, 1, 3, 1.5)) == \
        "y: values outside [0, 1] or non-finite in the valid rows of problems [1] (family 'logistic')"
    assert _message(ValueError, _glm, "probit", y=_bad(Y, 1, 3, np.nan)) == \
        "y: values outside [0, 1] or non-finite in the valid rows of problems [1] (family 'probit')"
    assert _message(ValueError, _glm, "poisson", y=_bad(Y, 0, 11, -1.0)) == \
        "y: values negative or non-finite in the valid rows of problems [0] (family 'poisson')"
    assert _message(ValueError, _glm, "gaussian", y=_bad(Y, 2, 4, np.inf)) == \
        "y: values non-finite in the valid rows of problems [2] (family 'gaussian')"
    assert _message(ValueError, _glm, family="cauchy") == \
        "family: expected one of ('logistic', 'poisson', 'probit', 'gaussian'), got 'cauchy'"
    # the arguments that the GLM class alone has
    assert _message(ValueError, _glm, "gaussian", noise_precision=[1.0, 2.0]) == \
        "noise_precision: expected a number or 3 values, got shape (2,)"
    assert _message(ValueError, _glm, "poisson", noise_precision=2.0) == \
        "noise_precision: only family 'gaussian' has one (family 'poisson': leave it at 1.0)"
    assert _message(ValueError, _glm, "gaussian", noise_precision=0.0) == "noise_precision: expected finite values > 0"
    assert _message(ValueError, _glm, "gaussian", noise_precision=[1.0, -2.0, np.inf]) == \
        "noise_precision: expected finite values > 0 (problems [1, 2])"
    assert _message(ValueError, _glm, offset=np.zeros((K, N - 1))) == "offset: expected shape (K, N) = (3, 12), got (3, 11)"
    assert _message(ValueError, _glm, offset=_bad(np.zeros((K, N)), 2, 0, np.nan)) == \
        "offset: non-finite values in the valid rows of problems [2]"
    # what the logistic class reads as after the shared constructor
    t = _logistic()
    assert (t.family, t.offset, t.noise_precision) == ("logistic", None, 1.0)


def test_predict_messages_of_both_classes():
    mean, cov, An, yn = np.zeros((K, D)), np.tile(np.eye(D), (K, 1, 1)), A[:, :M], Y[:, :M]
    for tgt in (_logistic(), _glm()):
        assert _message(ValueError, tgt.predict, mean, cov, An, y=yn[:, :4]) == "y: expected shape (K, M) = (3, 5), got (3, 4)"
        assert _message(ValueError, tgt.predict, mean, cov, An, counts=[6, 1, 1]) == \
            "counts: values outside 0 .. M = 5 for problems [0]"
        assert _message(ValueError, tgt.predict, mean, cov, An, offset=np.zeros((K, 4))) == \
            "offset: expected shape (K, M) = (3, 5), got (3, 4)"
        assert _message(ValueError, tgt.predict, mean, cov, An, offset=_bad(np.zeros((K, M)), 1, 1, np.inf)) == \
            "offset: non-finite values in the valid rows of problems [1]"
    assert _message(ValueError, _logistic().predict, mean, cov, An, y=_bad(yn, 0, 2, -0.5)) == \
        "y: values outside [0, 1] or non-finite in the valid rows of problems [0]"
    assert _message(ValueError, _glm().predict, mean, cov, An, y=_bad(yn, 0, 2, -0.5)) == \
        "y: values outside [0, 1] or non-finite in the valid rows of problems [0] (family 'logistic')"
    assert _message(ValueError, _glm("poisson").predict, mean, cov, An, y=_bad(yn, 2, 0, np.nan)) == \
        "y: values negative or non-finite in the valid rows of problems [2] (family 'poisson')"


def test_laplace_type_error_names_both_classes():
    assert _message(TypeError, laplace_init_batched, 3) == \
        "laplace_init_batched: target must be a BatchedGLMTarget or a BatchedLogisticTarget, got int"
    assert _message(TypeError, laplace_init_batched, object()) == \
        "laplace_init_batched: target must be a BatchedGLMTarget or a BatchedLogisticTarget, got object"
