"""The rejections of the C ABI's entry points (csrc/gsmvi_abi.hip), status and message text, against a recorded table.

Every case is ONE check line of the source, or two faults at once whose answer pins the ORDER of the checks; each was written
by reading the checks, never by trying arguments: a combination the library accepts would launch a kernel on bad pointers, so
none may be here, and no argument whose NULL the library accepts is passed as NULL (``mu`` of gsmvi_gsm_apply_rows_f64,
``n_reverts_dev``, ``info_dev`` of gsmvi_bam_update_f64, ``mu`` / ``logdiag_dev`` of gsmvi_whiten_rows_f64).  Nothing is
launched: every call returns from its argument checks, the whole table takes milliseconds.

Shapes: D = 8, B = 2 on a context created for (8, 2); the bounds of the factor forms (2B > D, 2B > 256) need a batch the small
context refuses first, so they run on a context for (512, 129), and the D-only bound of the batch-sharded local stage
(D > 16384) on one for (16386, 2).  All device buffers are real and large enough for every shape named here.

tests/golden/abi_args.json holds (entry, case) -> (status, message).  It is recorded by this file: with GSMVI_ABI_ARGS_RECORD set
to a path, the test writes the table there instead of comparing (run on the commit whose behaviour is the reference)."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "abi_args.json")
RECORD_ENV = "GSMVI_ABI_ARGS_RECORD"
CONTEXTS = {"main": (8, 2), "big": (512, 129), "wide": (16386, 2)}
D, B, LREC = 8, 2, 24                                            # LREC = gsmvi_gsm_record_len(8) = 3 D
NBUF = 12                                                        # distinct device buffers "@0" .. "@11" of 512 x 512 doubles


def _entries():
    """[(entry, case, context key or None, [arguments behind ctx])]; "@i" = device buffer i, "@i+8" = 8 bytes into it,
    "@flag" / "@nrev" = int32 words; the stream (second argument of the entries that take one) is the NULL stream."""
    out = []

    def entry(name, sig, base, common=True, nulls=(), lds=(), alias=(), extra=(), stream=True, d10=None, bname="B"):
        names = sig.split()
        assert set(base) == set(names), (name, sorted(set(base) ^ set(names)))

        def case(label, over, ctx="main"):
            vals = dict(base, **over)
            out.append((name, label, ctx, stream, [vals[k] for k in names]))

        if common:                                               # check_common: ctx, (D, B) positive, inside the workspace
            case("ctx NULL", {}, ctx=None)
            case("D = 0", {"D": 0})
            case("B = 0", {bname: 0})
            big = {k: 32 for k in names if k.startswith("ld")}
            case("D = 10 (beyond the workspace)", dict(big, D=10, **(d10 or {})))
            case("ctx NULL, D = 0", {"D": 0}, ctx=None)
        for p in nulls:
            case(f"{p} NULL", {p: None})
        for ld, bound in lds:
            case(f"{ld} = {bound - 1} (one below its bound)", {ld: bound - 1})
        for a, b in alias:
            case(f"{a} aliases {b}", {a: base[b]})
        if nulls and lds:
            case(f"{nulls[0]} NULL, {lds[0][0]} small", {nulls[0]: None, lds[0][0]: lds[0][1] - 1})
        for label, over, ctx in extra:
            case(label, over, ctx)

    # ---- the entries without a (D, B) workspace check in front -----------------------------------------------------------------
    entry("gsmvi_set_tuning", "name value", {"name": b"panel_kc", "value": 0}, common=False, stream=False,
          extra=[("ctx NULL", {}, None), ("name NULL", {"name": None}, "main"), ("unknown knob", {"name": b"no_such_knob"}, "main")])
    entry("gsmvi_last_path", "bits reset", {"bits": "@bits", "reset": 0}, common=False, stream=False,
          extra=[("ctx NULL", {}, None), ("bits NULL", {"bits": None}, "main")])
    entry("gsmvi_bam_set_reg_source", "reg_dev", {"reg_dev": None}, common=False, stream=False, extra=[("ctx NULL", {}, None)])
    entry("gsmvi_set_profiling", "on", {"on": 0}, common=False, stream=False, extra=[("ctx NULL", {}, None)])
    entry("gsmvi_get_profile", "ms n", {"ms": "@ms", "n": 3}, common=False, stream=False,
          extra=[("ctx NULL", {}, None), ("ms NULL", {"ms": None}, "main"), ("n = 0", {"n": 0}, "main")])
    entry("gsmvi_commit_f64", "D info_dev mu_new S_new lds_new mu S lds n_reverts_dev",
          {"D": D, "info_dev": "@flag", "mu_new": "@0", "S_new": "@1", "lds_new": D, "mu": "@2", "S": "@3", "lds": D,
           "n_reverts_dev": "@nrev"}, common=False, nulls=("info_dev", "mu_new", "S_new", "mu", "S"),
          lds=(("lds_new", D), ("lds", D)), extra=[("ctx NULL", {}, None), ("D = 0", {"D": 0}, "main"), ("ctx NULL, D = 0", {"D": 0}, None)])
    entry("gsmvi_potrf_f64", "D S lds R ldr info_dev", {"D": D, "S": "@0", "lds": D, "R": "@1", "ldr": D, "info_dev": "@flag"},
          common=False, nulls=("S", "R", "info_dev"), lds=(("lds", D), ("ldr", D)), alias=(("R", "S"),),
          extra=[("ctx NULL", {}, None), ("D = 0", {"D": 0}, "main"), ("ctx NULL, D = 0", {"D": 0}, None),
                 ("D = 10 (beyond the workspace)", {"D": 10, "lds": 32, "ldr": 32}, "main")])
    gram = {"D": D, "F": "@0", "ldf": D, "C": "@1", "ldc": D}
    gx = [("ctx NULL", {}, None), ("D = 0", {"D": 0}, "main"), ("ctx NULL, D = 0", {"D": 0}, None)]
    entry("gsmvi_gram_f64", "D F ldf C ldc", gram, common=False, nulls=("F", "C"), lds=(("ldf", D), ("ldc", D)),
          alias=(("C", "F"),), extra=gx)
    entry("gsmvi_gram_shift_f64", "D F ldf shift shift_dev C ldc", dict(gram, shift=0.5, shift_dev=None), common=False,
          nulls=("F", "C"), lds=(("ldf", D), ("ldc", D)), alias=(("C", "F"),),
          extra=gx + [("shift NaN", {"shift": float("nan")}, "main"), ("C aliases F, shift NaN", {"C": "@0", "shift": float("nan")}, "main")])
    entry("gsmvi_whiten_rows_f64", "D nrows R ldr X ldx mu Z ldz logdiag_dev",
          {"D": D, "nrows": B, "R": "@0", "ldr": D, "X": "@1", "ldx": D, "mu": "@2", "Z": "@3", "ldz": D, "logdiag_dev": "@4"},
          common=False, nulls=("R", "X", "Z"), lds=(("ldr", D), ("ldx", D), ("ldz", D)),
          extra=[("ctx NULL", {}, None), ("D = 0", {"D": 0}, "main"), ("nrows = 0", {"nrows": 0}, "main"),
                 ("D = 8194 (the residual row lives in LDS)", {"D": 8194, "ldr": 8194, "ldx": 8194, "ldz": 8194}, "main")])

    # ---- the diagnostics of include/gsmvi_hip_debug.h (debug library only; the copy takes a stream and no context: its "ctx NULL"
    # slot is that stream) -----------------------------------------------------------------------------------------------------
    reg = [("ctx NULL", {}, None), ("out NULL", {"out": None}, "main"), ("region = -1", {"region": -1}, "main"),
           ("region = 3", {"region": 3}, "main")]
    entry("gsmvi_debug_read_workspace", "region offset out n", {"region": 0, "offset": 0, "out": "@hd", "n": 4}, common=False,
          stream=False, extra=reg)
    entry("gsmvi_debug_workspace_ptr", "region out", {"region": 0, "out": "@hp"}, common=False, stream=False, extra=reg)
    entry("gsmvi_debug_read_stamps", "out n", {"out": "@hu", "n": 4}, common=False, stream=False,
          extra=[("ctx NULL", {}, None), ("out NULL", {"out": None}, "main"), ("n = 0", {"n": 0}, "main")])
    entry("gsmvi_debug_stream_copy_f64", "dst src n", {"dst": "@0", "src": "@1", "n": 1024}, common=False, stream=False,
          extra=[("dst NULL", {"dst": None}, None), ("src NULL", {"src": None}, None), ("n = 0", {"n": 0}, None),
                 ("n = 1023 (odd)", {"n": 1023}, None), ("dst 8 bytes off 16-byte alignment", {"dst": "@0+8"}, None),
                 ("src 8 bytes off 16-byte alignment", {"src": "@1+8"}, None)])

    # ---- the dense GSM update and its stages -----------------------------------------------------------------------------------
    upd = {"D": D, "B": B, "X": "@0", "ldx": D, "G": "@1", "ldg": D, "mu0": "@2", "S0": "@3", "lds0": D, "mu": "@4", "S": "@5",
           "lds": D}
    for name in ("gsmvi_gsm_update_f64", "gsmvi_gsm_update_general_f64"):
        entry(name, "D B X ldx G ldg mu0 S0 lds0 mu S lds", upd, nulls=("X", "G", "mu0", "S0", "mu", "S"),
              lds=(("ldx", D), ("ldg", D), ("lds0", D), ("lds", D)), alias=(("S", "S0"), ("mu", "mu0")))
    entry("gsmvi_gsm_local_stage_f64", "D B X ldx G ldg mu0 S0 lds0 rec ldrec",
          {"D": D, "B": B, "X": "@0", "ldx": D, "G": "@1", "ldg": D, "mu0": "@2", "S0": "@3", "lds0": D, "rec": "@4", "ldrec": LREC},
          nulls=("X", "G", "mu0", "S0", "rec"), lds=(("ldx", D), ("ldg", D), ("lds0", D), ("ldrec", 3 * D)))
    entry("gsmvi_gsm_apply_f64", "D B rec ldrec mu0 S0 lds0 mu S lds",
          {"D": D, "B": B, "rec": "@0", "ldrec": LREC, "mu0": "@1", "S0": "@2", "lds0": D, "mu": "@3", "S": "@4", "lds": D},
          nulls=("rec", "mu0", "S0", "mu", "S"), lds=(("ldrec", 3 * D), ("lds0", D), ("lds", D)), alias=(("S", "S0"), ("mu", "mu0")))
    entry("gsmvi_gsm_rows_stage_f64", "D B nrows G ldg S0rows lds0 SGcols ldsg",
          {"D": D, "B": B, "nrows": D, "G": "@0", "ldg": D, "S0rows": "@1", "lds0": D, "SGcols": "@2", "ldsg": D},
          nulls=("G", "S0rows", "SGcols"), lds=(("ldg", D), ("lds0", D), ("ldsg", D)),
          extra=[("nrows = 0", {"nrows": 0}, "main"), ("nrows = 9 (beyond the context's max_D)", {"nrows": 9, "ldsg": 16}, "main")])
    entry("gsmvi_gsm_records_f64", "D B X ldx G ldg mu0 SG rec ldrec",
          {"D": D, "B": B, "X": "@0", "ldx": D, "G": "@1", "ldg": D, "mu0": "@2", "SG": "@3", "rec": "@4", "ldrec": LREC},
          nulls=("X", "G", "mu0", "SG", "rec"), lds=(("ldx", D), ("ldg", D), ("ldrec", LREC)))
    entry("gsmvi_gsm_apply_rows_f64", "D B row0 nrows rec ldrec mu0 S0rows lds0 mu Srows lds",
          {"D": D, "B": B, "row0": 0, "nrows": D, "rec": "@0", "ldrec": LREC, "mu0": "@1", "S0rows": "@2", "lds0": D, "mu": "@3",
           "Srows": "@4", "lds": D}, nulls=("rec", "mu0", "S0rows", "Srows"), lds=(("lds0", D), ("lds", D), ("ldrec", LREC)),
          alias=(("Srows", "S0rows"), ("mu", "mu0")),
          extra=[("row0 = -1", {"row0": -1}, "main"), ("nrows = 0", {"nrows": 0}, "main"),
                 ("row0 + nrows = 9 > D", {"row0": 1}, "main")])
    entry("gsmvi_gaussian_score_f64", "D B X ldx m P ldp G ldg",
          {"D": D, "B": B, "X": "@0", "ldx": D, "m": "@1", "P": "@2", "ldp": D, "G": "@3", "ldg": D},
          nulls=("X", "m", "P", "G"), lds=(("ldx", D), ("ldp", D), ("ldg", D)))
    entry("gsmvi_sample_f64", "D B Z ldz mu R ldr X ldx",
          {"D": D, "B": B, "Z": "@0", "ldz": D, "mu": "@1", "R": "@2", "ldr": D, "X": "@3", "ldx": D},
          nulls=("Z", "mu", "R", "X"), lds=(("ldz", D), ("ldr", D), ("ldx", D)))
    entry("gsmvi_sample_cols_f64", "D B ncols Z ldz mu_cols Fcols ldf Xcols ldx",
          {"D": D, "B": B, "ncols": D, "Z": "@0", "ldz": D, "mu_cols": "@1", "Fcols": "@2", "ldf": D, "Xcols": "@3", "ldx": D},
          nulls=("Z", "mu_cols", "Fcols", "Xcols"), lds=(("ldz", D), ("ldf", D), ("ldx", D)),
          extra=[("ncols = 0", {"ncols": 0}, "main"), ("ncols = 9 > D", {"ncols": 9, "ldf": 16, "ldx": 16}, "main")])

    # ---- the dense BaM update ---------------------------------------------------------------------------------------------------
    entry("gsmvi_bam_update_f64", "D B X ldx G ldg mu0 S0 lds0 reg jitter mu S lds info_dev",
          dict(upd, reg=1.0, jitter=0.0, info_dev="@flag"), nulls=("X", "G", "mu0", "S0", "mu", "S"),
          lds=(("ldx", D), ("ldg", D), ("lds0", D), ("lds", D)), alias=(("S", "S0"), ("mu", "mu0")),
          extra=[("reg = 0", {"reg": 0.0}, "main"), ("reg = -1", {"reg": -1.0}, "main"),
                 ("S aliases S0, reg = 0", {"S": "@3", "reg": 0.0}, "main")])

    # ---- the factor forms -------------------------------------------------------------------------------------------------------
    def bound(extra_over=None):                                  # 2B > D and 2B > 256, on the context that admits those batches
        o = extra_over or {}
        big = {k: 512 for k in ("ldz", "ldx", "ldg", "ldf0", "ldf")}
        return [("2B = 10 > D", dict({"B": 5}, **o), "big"),
                ("2B = 258 > 256", dict({k: v for k, v in big.items()}, D=512, B=129, **o), "big")]

    fac = {"D": D, "B": B, "Z": "@0", "ldz": D, "X": "@1", "ldx": D, "G": "@2", "ldg": D, "mu0": "@3", "F0": "@4", "ldf0": D,
           "mu": "@5", "F": "@6", "ldf": D, "info_dev": "@flag", "n_reverts_dev": "@nrev"}
    fsig = "D B Z ldz X ldx G ldg mu0 F0 ldf0 mu F ldf info_dev n_reverts_dev"
    flds = (("ldz", D), ("ldx", D), ("ldg", D), ("ldf0", D), ("ldf", D))

    def only(d, sig):
        return {k: d[k] for k in sig.split()}

    def fit(cases, sig):                                         # drop the overrides an entry has no parameter for
        return [(lbl, {k: v for k, v in o.items() if k in sig.split()}, c) for lbl, o, c in cases]

    entry("gsmvi_gsm_factor_update_f64", fsig, fac, nulls=("Z", "X", "G", "mu0", "F0", "mu", "F", "info_dev"), lds=flds,
          alias=(("F", "F0"), ("mu", "mu0")), extra=bound())
    entry("gsmvi_bam_factor_update_f64", fsig.replace("ldf0 mu", "ldf0 reg mu"), dict(fac, reg=1.0),
          nulls=("Z", "X", "G", "mu0", "F0", "mu", "F", "info_dev"), lds=flds, alias=(("F", "F0"), ("mu", "mu0")),
          extra=bound() + [("reg = 0", {"reg": 0.0}, "main"), ("reg = -1", {"reg": -1.0}, "main"),
                           ("F aliases F0, reg = 0", {"F": "@4", "reg": 0.0}, "main"),
                           ("reg = 0, 2B = 10 > D", {"reg": 0.0, "B": 5}, "big")])
    lsig = "D B Z ldz X ldx G ldg mu0 F0 ldf0 rec ldrec"
    entry("gsmvi_gsm_factor_local_stage_f64", lsig, dict(only(fac, "D B Z ldz X ldx G ldg mu0 F0 ldf0"), rec="@7", ldrec=LREC),
          nulls=("Z", "X", "G", "mu0", "F0", "rec"), lds=(("ldz", D), ("ldx", D), ("ldg", D), ("ldf0", D), ("ldrec", LREC)),
          extra=[("D = 16386 > 16384", {"D": 16386, "ldz": 16386, "ldx": 16386, "ldg": 16386, "ldf0": 16386, "ldrec": 49158}, "wide")])
    asig = "D B Z ldz rec ldrec mu0 F0 ldf0 mu F ldf info_dev n_reverts_dev"
    entry("gsmvi_gsm_factor_apply_f64", asig, dict(only(fac, "D B Z ldz mu0 F0 ldf0 mu F ldf info_dev n_reverts_dev"), rec="@7", ldrec=LREC),
          nulls=("Z", "rec", "mu0", "F0", "mu", "F", "info_dev"), lds=(("ldz", D), ("ldf0", D), ("ldf", D), ("ldrec", LREC)),
          alias=(("F", "F0"), ("mu", "mu0")),
          extra=fit(bound(), asig)[:1] + [("2B = 258 > 256", {"D": 512, "B": 129, "ldz": 512, "ldf0": 512, "ldf": 512, "ldrec": 1536}, "big")])

    # ---- the column-sharded factor forms: the owned block [col0, col0 + ncols) ------------------------------------------------------
    def block(bad_bound):
        return [("col0 = 4 (not a multiple of 64)", {"col0": 4, "ncols": 4}, "main"),
                ("ncols = 4 (ragged, not the last block)", {"ncols": 4}, "main"),
                ("col0 + ncols = 16 > D", {"ncols": 16, "ldf0": 16, "ldf": 16}, "main"),
                ("col0 = 4, 2B = 10 > D", dict({"col0": 4, "ncols": 4}, **bad_bound), "big")]

    csig = "D B col0 ncols Z ldz W X ldx mu0 F0cols ldf0 mu Fcols ldf info_dev n_reverts_dev"
    cols = {"D": D, "B": B, "col0": 0, "ncols": D, "Z": "@0", "ldz": D, "W": "@1", "X": "@2", "ldx": D, "mu0": "@3", "F0cols": "@4",
            "ldf0": D, "mu": "@5", "Fcols": "@6", "ldf": D, "info_dev": "@flag", "n_reverts_dev": "@nrev"}
    wide = {"D": 512, "B": 129, "ncols": 512, "ldz": 512, "ldx": 512, "ldg": 512, "ldf0": 512, "ldf": 512}
    even = [("D = 7 (odd)", {"D": 7, "ncols": 7}, "main"), ("ldf0 = 9 (odd)", {"ldf0": 9}, "main"),
            ("F0cols 8 bytes off 16-byte alignment", {"F0cols": "@4+8"}, "main")]
    evenf = [("ldf = 9 (odd)", {"ldf": 9}, "main"), ("Fcols 8 bytes off 16-byte alignment", {"Fcols": "@6+8"}, "main")]
    entry("gsmvi_gsm_factor_apply_cols_f64", csig, cols, d10={"ncols": 10},
          nulls=("Z", "W", "X", "mu0", "F0cols", "mu", "Fcols", "info_dev"), lds=(("ldz", D), ("ldx", D), ("ldf0", D), ("ldf", D)),
          alias=(("Fcols", "F0cols"), ("mu", "mu0")),
          extra=fit(block({"B": 5}) + even + evenf + [("2B = 10 > D", {"B": 5}, "big"), ("2B = 258 > 256", wide, "big")], csig))
    wsig = "D B col0 ncols G ldg F0cols ldf0 reg Wq_part"
    entry("gsmvi_bam_factor_wq_partial_f64", wsig,
          {"D": D, "B": B, "col0": 0, "ncols": D, "G": "@0", "ldg": D, "F0cols": "@4", "ldf0": D, "reg": 1.0, "Wq_part": "@1"},
          d10={"ncols": 10}, nulls=("G", "F0cols", "Wq_part"), lds=(("ldf0", D), ("ldg", D)),
          alias=(("Wq_part", "G"), ("Wq_part", "F0cols")),
          extra=fit(block({"B": 5}) + even + [("reg = 0", {"reg": 0.0}, "main"), ("reg = -1", {"reg": -1.0}, "main"),
                                              ("Wq_part aliases G, reg = 0", {"Wq_part": "@0", "reg": 0.0}, "main"),
                                              ("2B = 10 > D", {"B": 5}, "big"), ("2B = 258 > 256", wide, "big")], wsig))
    bsig = "D B col0 ncols Z ldz X ldx G ldg Wq mu0 F0cols ldf0 reg mu Fcols ldf info_dev n_reverts_dev"
    entry("gsmvi_bam_factor_apply_cols_f64", bsig,
          {"D": D, "B": B, "col0": 0, "ncols": D, "Z": "@0", "ldz": D, "X": "@2", "ldx": D, "G": "@7", "ldg": D, "Wq": "@1", "mu0": "@3",
           "F0cols": "@4", "ldf0": D, "reg": 1.0, "mu": "@5", "Fcols": "@6", "ldf": D, "info_dev": "@flag", "n_reverts_dev": "@nrev"},
          d10={"ncols": 10}, nulls=("Z", "X", "G", "Wq", "mu0", "F0cols", "mu", "Fcols", "info_dev"),
          lds=(("ldf0", D), ("ldz", D), ("ldx", D), ("ldg", D), ("ldf", D)),
          alias=(("Fcols", "F0cols"), ("mu", "mu0"), ("Fcols", "Wq")),
          extra=fit(block({"B": 5}) + even + evenf + [("reg = 0", {"reg": 0.0}, "main"), ("reg = -1", {"reg": -1.0}, "main"),
                                                      ("mu aliases mu0, reg = 0", {"mu": "@3", "reg": 0.0}, "main"),
                                                      ("2B = 10 > D", {"B": 5}, "big"), ("2B = 258 > 256", wide, "big")], bsig))
    return out


def test_table_is_unambiguous_and_matches_the_ctypes_signatures():
    """CPU: (entry, case) pairs are unique and every argument list has the length of the entry's ctypes signature"""
    from gsmvi_amd import _lib
    seen = set()
    for name, label, ctx, stream, args in _entries():
        assert (name, label) not in seen, (name, label)
        seen.add((name, label))
        assert len(args) + 1 + int(stream) == len({**_lib._SIGS, **_lib._DEBUG_SIGS}[name][1]), name
    assert len(seen) >= 300


def test_fixture_holds_exactly_the_table():
    """CPU: tests/golden/abi_args.json has one record per case of the table, no more"""
    rec = json.load(open(FIXTURE))
    assert sorted((r["entry"], r["case"]) for r in rec["records"]) == sorted((n, c) for n, c, _, _, _ in _entries())


@pytest.mark.gpu
def test_entry_points_reject_as_recorded():
    import torch
    from gsmvi_amd import _lib
    lib = _lib.load_library()
    dbg = C.CDLL(_lib.library_path(debug=True))                  # the same objects, diagnostics exported as well
    dbg.gsmvi_last_error.restype = C.c_char_p
    for name, (res, argtypes) in _lib._DEBUG_SIGS.items():
        getattr(dbg, name).restype, getattr(dbg, name).argtypes = res, argtypes
    dev = torch.device("cuda", 0)
    bufs = [torch.zeros(512 * 512, dtype=torch.float64, device=dev) for _ in range(NBUF)]
    words = {"@flag": torch.zeros(4, dtype=torch.int32, device=dev), "@nrev": torch.zeros(4, dtype=torch.int32, device=dev)}
    bits, ms = C.c_uint(0), (C.c_float * 3)()
    host = {"@bits": C.byref(bits), "@ms": ms, "@hd": (C.c_double * 4)(), "@hp": C.byref(C.c_void_p()),
            "@hu": (C.c_ulonglong * 4)()}

    def value(v):
        if isinstance(v, str) and v.startswith("@"):
            if v in host:
                return host[v]
            if v in words:
                return words[v].data_ptr()
            idx, _, off = v[1:].partition("+")
            return bufs[int(idx)].data_ptr() + int(off or 0)
        return v

    ctxs = {}
    try:
        for key, (mD, mB) in CONTEXTS.items():
            ctxs[key] = C.c_void_p()
            _lib.check("gsmvi_create", lib.gsmvi_create(C.byref(ctxs[key]), 0, mD, mB))
        got = []
        for name, label, ctx, stream, args in _entries():
            head = [ctxs[ctx] if ctx else None] + ([None] if stream else [])
            use = dbg if name.startswith("gsmvi_debug_") else lib
            status = getattr(use, name)(*head, *[value(a) for a in args])
            assert status != 0, f"{name} [{label}] was accepted"    # (by construction it never is: see the module's docstring)
            got.append({"entry": name, "case": label, "status": int(status), "message": use.gsmvi_last_error().decode()})
        torch.cuda.synchronize(dev)
    finally:
        for c in ctxs.values():
            if c:
                lib.gsmvi_destroy(c)
    if os.environ.get(RECORD_ENV):
        with open(os.environ[RECORD_ENV], "w") as f:
            json.dump({"records": got}, f, indent=0)
            f.write("\n")
        return
    want = {(r["entry"], r["case"]): (r["status"], r["message"]) for r in json.load(open(FIXTURE))["records"]}
    bad = [(g["entry"], g["case"], (g["status"], g["message"]), want.get((g["entry"], g["case"])))
           for g in got if want.get((g["entry"], g["case"])) != (g["status"], g["message"])]
    assert not bad, bad[:10]
    assert len(got) == len(want)
