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


def test_declared_for_either_purpose():
    """a decoder context serves both: the header names the parameter any_ctx, which tests/test_gpu_decoder_ctx.py::test_refusals goes by"""
    with open(os.path.join(ROOT, "include", "dark_amd.h")) as f:
        header = f.read()
    for name in ("dk_dbg_mail_fill", "dk_dbg_ws_peek"):
        assert re.search(r"\bint %s\(dk_ctx \*any_ctx," % name, header), name
        assert name in _lib.SIGNATURES
