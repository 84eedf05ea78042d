"""The FM-index's host side (include/dark_amd.h, csrc/fm_index.hip): the size of the index and the argument checks that need no GPU."""
import ctypes as C

import dark_amd
from dark_amd import _lib
from dark_amd.context import fm_index_bytes

MAX_TOTAL = 0x7FFFFFFE


def index_bound(total, count):
    """checkpoints total + 2 KiB at most, 1040 bytes per block, a header of 256 bytes"""
    return 1.25 * total + 2048 * count + 65536


def test_size_of_the_index():
    assert fm_index_bytes(1, 1) > 0
    sizes = [1, 2, 1023, 1024, 1025, 4096, 100000, 1 << 20, (1 << 26) + 1, MAX_TOTAL]
    for count in (1, 2, 1000, 65536):
        last = 0
        for total in sizes:
            if count > total:
                assert fm_index_bytes(total, count) == 0
                continue
            b = fm_index_bytes(total, count)
            assert b % 4 == 0 and last < b + 1 and 0 < b <= index_bound(total, count), (total, count, b)
            assert b >= total  # the checkpoints: 1024 bytes per 1024 positions
            last = b
    for total in (65536, 1 << 24):
        row = [fm_index_bytes(total, count) for count in (1, 2, 3, 100, 65535, 65536)]
        assert row == sorted(row) and len(set(row)) == len(row)
    assert fm_index_bytes(100000, 1) < fm_index_bytes(100000 + 1024, 1)


def test_refused_arguments_give_no_size():
    for total, count in ((0, 1), (1, 0), (0, 0), (MAX_TOTAL + 1, 1), (1 << 40, 1), (1 << 20, 65537), (5, 6)):
        assert fm_index_bytes(total, count) == 0, (total, count)
    assert fm_index_bytes(-1, 1) == 0


def test_null_context():
    lib = dark_amd.load_library()
    buf = (C.c_uint8 * 64)()
    words = (C.c_uint32 * 16)()
    ns, ls, bs = (C.c_size_t * 1)(8), (C.c_size_t * 1)(2), (C.c_uint32 * 1)(0)
    p, w = C.cast(buf, C.c_void_p), C.cast(words, C.c_void_p)
    assert lib.dk_dev_fm_build(None, p, 8, 0, w) == _lib.DK_E_ARG
    assert lib.dk_dev_fm_build_packed(None, p, 1, ns, w, w) == _lib.DK_E_ARG
    assert lib.dk_dev_fm_count(None, p, 8, w, p, 1, ls, w, w) == _lib.DK_E_ARG
    assert lib.dk_dev_fm_count_packed(None, p, 1, ns, w, p, 1, ls, bs, w, w) == _lib.DK_E_ARG
    assert lib.dk_fm_count(None, p, 8, 0, p, 1, ls, w, w) == _lib.DK_E_ARG
    assert lib.dk_dbg_dev_fm_rank(None, p, 8, w, w, p, 1, w) == _lib.DK_E_ARG
