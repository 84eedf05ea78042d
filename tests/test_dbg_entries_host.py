"""The two instruments of the poison tests (include/dark_amd.h: dk_dbg_mail_fill, dk_dbg_ws_peek): what needs no GPU."""
import ctypes as C
import os
import re

import dark_amd
from conftest import ROOT
from dark_amd import _lib


def test_null_context():
    lib = dark_amd.load_library()
    buf = (C.c_uint8 * 64)()
    assert lib.dk_dbg_mail_fill(None, 0) == _lib.DK_E_ARG
    assert lib.dk_dbg_mail_fill(None, 165) == _lib.DK_E_ARG
    assert lib.dk_dbg_ws_peek(None, 64, C.cast(buf, C.c_void_p)) == _lib.DK_E_ARG
    assert lib.dk_dbg_ws_peek(None, 0, None) == _lib.DK_E_ARG
    assert not any(buf)


def test_layer_entries_of_the_lfirst_path():
    """dk_dbg_dev_lf_rerank and dk_dbg_dev_lf_refine (tests/test_gpu_lfirst_layer.py): a null context is refused before any argument is looked
    at; both are declared in the header for a full context (the parameter's name is ctx: tests/test_gpu_decoder_ctx.py::test_refusals goes by
    it) and signed in _lib with as many arguments as the header has"""
    lib = dark_amd.load_library()
    counts = (C.c_uint32 * 4)(7, 7, 7, 7)
    assert lib.dk_dbg_dev_lf_rerank(None, None, 8, None, 0, None, 0, None, None, None, 100, None, None, None, None, None, None, None, None, 0, None, 0, 0,
                                    C.cast(counts, C.c_void_p), 0) == _lib.DK_E_ARG
    assert list(counts) == [7, 7, 7, 7]
    out = (C.c_uint32 * 8)(*([7] * 8))
    assert lib.dk_dbg_dev_lf_refine(None, None, 100, None, None, None, None, 10, 4, 0, None, None, C.cast(out, C.c_void_p)) == _lib.DK_E_ARG
    assert list(out) == [7] * 8
    with open(os.path.join(ROOT, "include", "dark_amd.h")) as f:
        header = f.read()
    for name in ("dk_dbg_dev_lf_rerank", "dk_dbg_dev_lf_refine"):
        assert re.search(r"\bint %s\(dk_ctx \*ctx," % name, header), name
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1).split(",")), name


def test_layer_entry_of_the_in_place_rounds():
    """dk_dbg_dev_in_place (tests/test_gpu_in_place.py): the same three facts"""
    lib = dark_amd.load_library()
    out = (C.c_uint32 * 8)(*([7] * 8))
    assert lib.dk_dbg_dev_in_place(None, 100, 4, 10, None, None, None, None, 5, None, None, None, None, None, -1, 0, -1, 0, None, None, None, None,
                                   C.cast(out, C.c_void_p)) == _lib.DK_E_ARG
    assert list(out) == [7] * 8
    with open(os.path.join(ROOT, "include", "dark_amd.h")) as f:
        header = f.read()
    name = "dk_dbg_dev_in_place"
    assert re.search(r"\bint %s\(dk_ctx \*ctx," % name, header)
    assert len(_lib.SIGNATURES[name][1]) == len(re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1).split(","))


def test_layer_entries_of_the_general_round_and_the_period_kernels():
    """dk_dbg_dev_round (tests/test_gpu_round.py) and dk_dbg_dev_period (tests/test_gpu_period.py): the same three facts"""
    lib = dark_amd.load_library()
    out = (C.c_uint32 * 8)(*([7] * 8))
    o = C.cast(out, C.c_void_p)
    assert lib.dk_dbg_dev_round(None, None, 100, 4, 10, None, None, None, None, 5, None, 0, 0, None, None, None, None, None, None, None, None, None, None, None, None,
                                None, o) == _lib.DK_E_ARG
    assert lib.dk_dbg_dev_period(None, None, 100, 0, None, o, o, 3, o, 100, o, 10, 10, None, 0, o) == _lib.DK_E_ARG
    assert list(out) == [7] * 8
    with open(os.path.join(ROOT, "include", "dark_amd.h")) as f:
        header = f.read()
    for name in ("dk_dbg_dev_round", "dk_dbg_dev_period"):
        assert re.search(r"\bint %s\(dk_ctx \*ctx," % name, header), name
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1).split(",")), name


def test_layer_entry_of_the_initial_sort():
    """dk_dbg_dev_initial_sort (tests/test_gpu_initial_sort.py): the same three facts"""
    lib = dark_amd.load_library()
    out = (C.c_uint32 * 4)(*([7] * 4))
    starts = (C.c_uint32 * 256)(*([7] * 256))
    code = (C.c_uint8 * 256)()
    assert lib.dk_dbg_dev_initial_sort(None, None, 100, C.cast(code, C.c_void_p), 2, 8, None, 1, None, None, None, None, C.cast(starts, C.c_void_p),
                                       C.cast(out, C.c_void_p)) == _lib.DK_E_ARG
    assert list(out) == [7] * 4 and list(starts) == [7] * 256
    with open(os.path.join(ROOT, "include", "dark_amd.h")) as f:
        header = f.read()
    name = "dk_dbg_dev_initial_sort"
    assert re.search(r"\bint %s\(dk_ctx \*ctx," % name, header)
    assert len(_lib.SIGNATURES[name][1]) == len(re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1).split(","))


def test_layer_entries_of_the_packed_sort():
    """dk_dbg_dev_packed_first and dk_dbg_dev_packed_round (tests/test_gpu_packed_round.py): the same three facts"""
    lib = dark_amd.load_library()
    out = (C.c_uint32 * 8)(*([7] * 8))
    code = (C.c_uint16 * 256)(*([7] * 256))
    ns = (C.c_size_t * 1)(100)
    o = C.cast(out, C.c_void_p)
    assert lib.dk_dbg_dev_packed_first(None, None, 1, C.cast(ns, C.c_void_p), None, None, None, None, C.cast(code, C.c_void_p), o) == _lib.DK_E_ARG
    assert lib.dk_dbg_dev_packed_round(None, 1, C.cast(ns, C.c_void_p), 4, None, 10, None, None, None, None, None, o) == _lib.DK_E_ARG
    assert list(out) == [7] * 8 and list(code) == [7] * 256
    with open(os.path.join(ROOT, "include", "dark_amd.h")) as f:
        header = f.read()
    for name in ("dk_dbg_dev_packed_first", "dk_dbg_dev_packed_round"):
        assert re.search(r"\bint %s\(dk_ctx \*ctx," % name, header), name
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1).split(",")), name


def test_declared_for_either_purpose():
    """a decoder context serves both: the header names the parameter any_ctx, which tests/test_gpu_decoder_ctx.py::test_refusals goes by"""
    with open(os.path.join(ROOT, "include", "dark_amd.h")) as f:
        header = f.read()
    for name in ("dk_dbg_mail_fill", "dk_dbg_ws_peek"):
        assert re.search(r"\bint %s\(dk_ctx \*any_ctx," % name, header), name
        assert name in _lib.SIGNATURES
