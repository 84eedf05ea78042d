"""Packed suffix arrays (dk_dev_suffix_array_packed, dk_suffix_array_packed) without a GPU: the header declares them, the built library
exports them, the binding knows them, and both refuse a null context before they touch anything."""
import ctypes as C
import os
import re

import dark_amd
from dark_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dark_amd.h")
NAMES = ("dk_dev_suffix_array_packed", "dk_suffix_array_packed")


def test_header_declares_both():
    with open(HEADER) as f:
        text = f.read()
    for name in NAMES:
        assert re.search(r"^int %s\s*\(dk_ctx \*ctx," % name, text, re.M), name


def test_library_exports_and_binding_holds_both():
    lib = dark_amd.load_library()
    for name in NAMES:
        assert hasattr(lib, name), "libdark_amd.so lacks %s" % name
        assert name in _lib.SIGNATURES, "python binding lacks %s" % name
        assert _lib.SIGNATURES[name][0] is C.c_int


def test_null_context_is_an_argument_error():
    lib = dark_amd.load_library()
    ns = (C.c_size_t * 1)(4)
    text = (C.c_uint8 * 4)(1, 2, 3, 4)
    sa = (C.c_uint32 * 4)(7, 7, 7, 7)
    origin = (C.c_uint32 * 1)(7)
    assert lib.dk_dev_suffix_array_packed(None, C.addressof(text), 1, ns, C.addressof(sa), None, None) == _lib.DK_E_ARG
    assert lib.dk_dev_suffix_array_packed(None, C.addressof(text), 1, ns, C.addressof(sa), C.addressof(text), origin) == _lib.DK_E_ARG
    assert lib.dk_suffix_array_packed(None, C.addressof(text), 1, ns, C.addressof(sa)) == _lib.DK_E_ARG
    assert list(sa) == [7, 7, 7, 7] and origin[0] == 7
