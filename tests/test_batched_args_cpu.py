"""The argument checks of the eight batched entry points, without a GPU (NULL context): the shape check, and the overlap rule
walked through every entry point's table of arrays -- an array a kernel may write must not overlap any other array of the
call, read-only arrays may overlap each other, and BaM's Xout may be X itself.  The context is reported last."""
import ctypes as C
import itertools

import pytest

from gsmvi_amd import _lib

K, D, B = 2, 4, 2          # B is nc for the two KL entry points
SLOT = 4096                # every array in a slot of its own: no array is longer than 2 x 16 x 8 = 256 bytes
DV, DM, DX = D * 8, D * D * 8, B * D * 8
PER_PROBLEM = {"X": DX, "G": DX, "Y": DX, "Xout": DX, "mu0": DV, "mu": DV, "mean": DV, "m": DV, "S0": DM, "S": DM,
               "cov": DM, "R": DM, "P": DM, "reg_dev": 8, "seeds_dev": 8, "seeds": 8, "logq_sum": 8, "info_dev": 4,
               "n_reverts_dev": 4, "info": 4}
# the arguments after (ctx, stream, K, D): "B" (nc for KL), the arrays by name -- "!" marks the written ones -- and the
# scalars as they are (reg, jitter, call, s0)
ENTRY = {
    "gsmvi_gsm_update_batched_f64": ["B", "X", "G", "mu0", "S0", "mu!", "S!"],
    "gsmvi_gsm_fit_init_batched_f64": ["B", "mean", "cov", "R!", "info_dev!", "seeds_dev", "X!"],
    "gsmvi_gsm_fit_step_batched_f64": ["B", "X!", "G", "mean!", "cov!", "R!", "info_dev!", "n_reverts_dev!", "seeds_dev", 0],
    "gsmvi_gaussian_score_batched_f64": ["B", "X", "m", "P", "G!"],
    "gsmvi_bam_update_batched_f64": ["B", "X", "G", "mu0", "S0", 1.0, "reg_dev", 0.0, "mu!", "S!", "info_dev!"],
    "gsmvi_bam_fit_step_batched_f64": ["B", "X!", "G", "mean!", "cov!", "R!", 1.0, "reg_dev", 0.0, "info_dev!",
                                       "n_reverts_dev!", "seeds_dev", 0, "Xout!"],
    "gsmvi_kl_draw_batched_f64": ["B", 0, "mean", "cov", "seeds", 0, "X!", "logq_sum!", "info!"],
    "gsmvi_logq_batched_f64": ["B", "mean", "cov", "Y", "logq_sum!", "info!"],
}

_buf = (C.c_char * (SLOT * 16))()
BASE = C.cast(_buf, C.c_void_p).value


def arrays(fn):
    """(name, written) of the arrays of fn, in argument order"""
    return [(a.rstrip("!"), a.endswith("!")) for a in ENTRY[fn][1:] if isinstance(a, str)]


def placed(fn, **moved):
    """name -> address: each array of fn in a slot of its own, except the `moved` ones"""
    at = {a: BASE + SLOT * (i + 1) for i, (a, _) in enumerate(arrays(fn))}
    at.update(moved)
    return at


def call(fn, at=None, k=K, d=D, b=B):
    """fn with a NULL context and its arrays at `at` (default: placed(fn)): (status, message)"""
    at = at or placed(fn)
    args = [b if a == "B" else at[a.rstrip("!")] if isinstance(a, str) else a for a in ENTRY[fn]]
    lib = _lib.load_library()
    st = getattr(lib, fn)(None, None, k, d, *args)
    return st, (lib.gsmvi_last_error() or b"").decode()


@pytest.mark.parametrize("fn", ENTRY)
def test_shapes_and_null_arrays_are_checked_before_the_context(fn):
    assert call(fn) == (1, f"{fn}: ctx is NULL")
    assert call(fn, d=0)[1].startswith(f"{fn}: D must be")
    assert call(fn, d=65)[1].startswith(f"{fn}: D must be")
    assert call(fn, k=0)[1].startswith(f"{fn}: K must be")
    assert call(fn, k=4 * (2**24 - 1) + 1)[1].startswith(f"{fn}: K must be")
    if "kl" in fn or "logq" in fn:
        assert call(fn, b=0)[1].startswith(f"{fn}: nc must be")
    else:
        assert call(fn, b=0)[1].startswith(f"{fn}: B must be")
        assert call(fn, b=33)[1].startswith(f"{fn}: B must be")
    first = arrays(fn)[0][0]                       # required by every entry point
    assert call(fn, placed(fn, **{first: None})) == (1, f"{fn}: NULL array")


@pytest.mark.parametrize("fn", ENTRY)
def test_every_written_array_against_every_other_array(fn):
    """a written array one element over either end of any other array is refused, the message naming both; two read-only
    arrays may overlap, even start at the same address"""
    size = {a: K * PER_PROBLEM[a] for a, _ in arrays(fn)}
    for (a, wa), (b, wb) in itertools.permutations(arrays(fn), 2):
        home = placed(fn)[b]
        for at in (home + size[b] - 4, home - size[a] + 4) + (() if wa or wb else (home,)):
            st, msg = call(fn, placed(fn, **{a: at}))
            if wa or wb:
                assert st == 1 and msg in (f"{fn}: {a} overlaps {b}", f"{fn}: {b} overlaps {a}"), (a, b, msg)
            else:
                assert (st, msg) == (1, f"{fn}: ctx is NULL"), (a, b, msg)


def test_xout_may_be_x_itself():
    fn = "gsmvi_bam_fit_step_batched_f64"
    assert call(fn, placed(fn, Xout=placed(fn)["X"])) == (1, f"{fn}: ctx is NULL")
    assert call(fn, placed(fn, Xout=placed(fn)["X"] + 8))[1] == f"{fn}: Xout overlaps X"
