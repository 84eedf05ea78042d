"""The matching-statistics entries (include/dark_amd.h: dk_dev_sa_match*, dk_dev_sa_smems*, their host forms): what needs no GPU."""
import ctypes as C
import os
import re

import numpy as np

import dark_amd
from conftest import ROOT
from dark_amd import _lib, saca
from dark_amd.context import SA_SMEM_DTYPE, Context

ENTRIES = ("dk_dev_sa_match", "dk_dev_sa_match_packed", "dk_sa_match", "dk_dev_sa_smems", "dk_dev_sa_smems_packed", "dk_sa_smems")


def header():
    with open(os.path.join(ROOT, "include", "dark_amd.h")) as f:
        return f.read()


def test_the_record_is_16_bytes():
    assert C.sizeof(_lib.SaSmem) == 16 and SA_SMEM_DTYPE.itemsize == 16
    assert [name for name, _ in _lib.SaSmem._fields_] == list(SA_SMEM_DTYPE.names) == ["at", "len", "lo", "hi"]
    assert [getattr(_lib.SaSmem, name).offset for name in SA_SMEM_DTYPE.names] == [SA_SMEM_DTYPE.fields[name][1] for name in SA_SMEM_DTYPE.names] == [0, 4, 8, 12]
    assert re.search(r"typedef struct dk_sa_smem \{ uint32_t at, len, lo, hi; \} dk_sa_smem;", header())


def test_the_six_declarations():
    """full contexts only, and none of the names falls into the families the refusal tests of check, search and LCP enumerate by substring"""
    h = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, h)
        assert m and m.group(1).startswith("dk_ctx *full_ctx,"), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
        assert not re.search(r"sa_search|sa_check|lcp", name)
        assert ("query_block" in m.group(1)) == name.endswith("_packed")
        assert ("min_len" in m.group(1)) == ("smems" in name) == ("uint64_t *total" in m.group(1))
    assert sorted(re.findall(r"\b(dk_[a-z0-9_]*sa_(?:match|smems)[a-z0-9_]*)\s*\(", h)) == sorted(ENTRIES)


def test_the_python_layers_have_the_entries():
    for name in ("dev_sa_match", "dev_sa_match_packed", "sa_match", "dev_sa_smems", "dev_sa_smems_packed", "sa_smems"):
        assert callable(getattr(Context, name)), name
    assert callable(saca.Constructor.match) and callable(saca.Constructor.smems)
    with open(os.path.join(ROOT, "include", "dark.hpp")) as f:
        mirror = f.read()
    assert "dk_sa_match(ctx_.get()" in mirror and "dk_sa_smems(ctx_.get()" in mirror


def test_null_context():
    """refused before anything is read or written"""
    lib = dark_amd.load_library()
    total = C.c_uint64(7)
    one, blk = (C.c_size_t * 1)(1), (C.c_uint32 * 1)(0)
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.dk_dev_sa_match(None, p, 1, p, p, 1, one, 5, p, p, p) == _lib.DK_E_ARG
    assert lib.dk_dev_sa_match_packed(None, p, 1, one, p, p, 1, one, blk, 5, p, p, p) == _lib.DK_E_ARG
    assert lib.dk_sa_match(None, p, 1, p, p, 1, one, 5, p, p, p) == _lib.DK_E_ARG
    assert lib.dk_dev_sa_smems(None, p, 1, p, p, 1, one, 0, 5, 4, p, C.byref(total)) == _lib.DK_E_ARG
    assert lib.dk_dev_sa_smems_packed(None, p, 1, one, p, p, 1, one, blk, 0, 5, 4, p, C.byref(total)) == _lib.DK_E_ARG
    assert lib.dk_sa_smems(None, p, 1, p, p, 1, one, 0, 5, 4, p, C.byref(total)) == _lib.DK_E_ARG
    assert total.value == 7 and not buf.any()


def test_the_border_is_the_searchs_knob():
    """one constant and one knob for both pairs of kernels (tests/test_tuning_knobs.py wants every knob in a tuning source)"""
    with open(os.path.join(ROOT, "dark_amd", "csrc", "sa_query.hip")) as f:
        src = f.read()
    assert src.count('DK_KNOB("DK_SA_SEARCH_LANE_MAX", SA_SEARCH_LANE_MAX)') == 2 and len(re.findall(r"DK_KNOB\(", src)) == 2
    assert re.search(r"constexpr uint32_t SM_TILE = 1024;", src)
