"""The messages of the five batched softmax entry points about their model, character for character, at the C ABI with a NULL
context (every argument is checked before the context, so no device is needed): the entries share one model check and one set of
overlap rows (csrc/gsmvi_softmax_model.h), and what a caller reads must not depend on which entry reported it."""
import ctypes as C

import pytest

from gsmvi_amd import _lib

SHAPE = "P must be at least 1 and D = (C - 1) P in [1, 64]"
K_PACKED = "K must be in [1, 2^24 - 1] (one problem per workgroup) or [1, 2^26 - 4] (four)"
K_TILED = "K must be in [1, 2^24 - 1]"

# entry -> (its arguments after (ctx, stream) in the order of include/gsmvi_hip.h, the name of its row count, its K rule, one of
# the arrays it writes under the name its messages use); "lam" marks an entry with a prior
ENTRIES = {
    "gsmvi_softmax_batched_f64": ("K C P nc N A labels counts lam lam_dev X G lp", "N", K_PACKED, "G"),
    "gsmvi_softmax_hessian_batched_f64": ("K C P N A labels counts lam lam_dev X H cov info", "N", K_PACKED, "H"),
    "gsmvi_softmax_laplace_step_batched_f64":
        ("K C P N A labels counts lam lam_dev start x g d sc ist Xt stopped maxiter maxfun gtol", "N", K_PACKED, "x"),
    "gsmvi_psis_loo_softmax_batched_f64":
        ("K C P N S A labels counts X logr lw loglik elpd lpd khat ess info", "N", K_TILED, "elpd"),
    "gsmvi_softmax_predict_batched_f64": ("K C P N S A labels counts X lw prob lpd", "M", K_TILED, "prob"),
}
SLOT = 65536
SCALARS = dict(K=2, C=3, P=2, N=5, nc=3, S=8, lam=1.0, lam_dev=None, start=0, maxiter=10, maxfun=20, gtol=1e-8)


@pytest.fixture(scope="module")
def abi():
    lib = _lib.load_library()
    buf = (C.c_double * (SLOT // 8 * 24))()    # 24 disjoint arrays of 64 KB: the largest here, H at D = 64, takes 32 KB
    base = C.cast(buf, C.c_void_p).value

    def call(fn, **kw):
        """(status, message) of entry ``fn`` with valid arguments, a NULL context, and ``kw`` in place of the named ones"""
        names = ENTRIES[fn][0].split()
        args = {n: SCALARS[n] if n in SCALARS else base + SLOT * i for i, n in enumerate(names)}
        assert set(kw) <= set(args), (fn, kw)
        args.update(kw)
        st = getattr(lib, fn)(None, None, *(args[n] for n in names))
        return st, (lib.gsmvi_last_error() or b"").decode()

    call.slot = lambda fn, name: base + SLOT * ENTRIES[fn][0].split().index(name)        # the default address of an array
    call.keepalive = buf
    return call


@pytest.mark.parametrize("fn", sorted(ENTRIES))
def test_model_messages_of_every_entry(abi, fn):
    _, rows, k_rule, _ = ENTRIES[fn]
    bad = lambda msg: (1, f"{fn}: {msg}")                            # noqa: E731  GSMVI_ERR_BAD_ARG
    assert abi(fn) == bad("ctx is NULL")                             # valid arguments end at the context
    for c in (1, 0, -3):
        assert abi(fn, C=c) == bad("C must be at least 2"), c
    for c, p in ((3, 0), (3, -1), (3, 33), (2, 65), (66, 1), (2 ** 31 - 1, 2)):
        assert abi(fn, C=c, P=p) == bad(SHAPE), (c, p)
    for c, p in ((2, 1), (2, 64), (65, 1), (17, 1), (5, 3), (33, 2)):
        assert abi(fn, K=1, C=c, P=p, N=1) == bad("ctx is NULL"), (c, p)
    for k in (0, -1, 2 ** 26 - 3):
        assert abi(fn, K=k) == bad(k_rule), k
    assert abi(fn, K=2 ** 24, C=2, P=17) == bad(k_rule)             # one problem per workgroup in the packed entries
    for n in (0, -5):
        assert abi(fn, N=n) == bad(f"{rows} must be at least 1"), n
    if "lam" in ENTRIES[fn][0].split():
        for lam in (-1.0, float("nan"), float("inf")):
            assert abi(fn, lam=lam) == bad("prior_prec must be finite and >= 0"), lam
        assert abi(fn, lam=-1.0, lam_dev=abi.slot(fn, "lam_dev")) == bad("ctx is NULL")     # the scalar is unused with K values
        assert abi(fn, lam=0.0) == bad("ctx is NULL")


@pytest.mark.parametrize("fn", sorted(ENTRIES))
def test_overlap_messages_name_the_models_arrays(abi, fn):
    names, _, _, written = ENTRIES[fn]
    for arg, shown in (("A", "A"), ("labels", "labels"), ("counts", "counts_dev"), ("lam_dev", "prior_prec_dev")):
        if arg not in names.split():
            continue
        at = abi.slot(fn, arg)
        assert abi(fn, **{arg: at, written: at}) == (1, f"{fn}: {written} overlaps {shown}"), arg
        assert abi(fn, **{arg: at, written: at + 4}) == (1, f"{fn}: {written} overlaps {shown}"), arg
    # the model's read-only arrays may overlap each other
    at = abi.slot(fn, "A")
    assert abi(fn, labels=at, counts=at) == (1, f"{fn}: ctx is NULL")


def test_the_models_message_comes_before_the_entrys_own(abi):
    """two bad arguments at once: the model's is reported (the rule of the GLM entries)"""
    fn = "gsmvi_softmax_batched_f64"
    assert abi(fn, lam=-1.0, nc=0) == (1, f"{fn}: prior_prec must be finite and >= 0")
    assert abi(fn, lam=-1.0, X=None) == (1, f"{fn}: prior_prec must be finite and >= 0")
    assert abi(fn, lam=-1.0, G=None, lp=None) == (1, f"{fn}: prior_prec must be finite and >= 0")
    assert abi(fn, nc=0) == (1, f"{fn}: nc must be at least 1")
