"""The near entries, fm.classes and the approximate archive search (include/dark_amd.h: dk_dev_fm_near*, dark_amd/fm.py, dark_amd/search.py,
dark_amd/cli.py --mismatches / -i): what needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dark_amd
from conftest import ROOT
from dark_amd import _lib, cli, fm, search
from dark_amd.context import FM_NEAR_HIT_DTYPE, FM_NEAR_MAX_K, FM_NEAR_MAX_PATTERN, FM_NEAR_NODE_LIMIT
from fm_near_model import NEAR_HIT_DTYPE, class_masks, exact_classes


def header():
    with open(os.path.join(ROOT, "include", "dark_amd.h")) as f:
        return f.read()


def test_the_record_is_16_bytes():
    assert FM_NEAR_HIT_DTYPE.itemsize == 16 and FM_NEAR_HIT_DTYPE == NEAR_HIT_DTYPE
    assert list(FM_NEAR_HIT_DTYPE.names) == ["pattern", "block", "position", "cost"]
    assert [FM_NEAR_HIT_DTYPE.fields[name][1] for name in FM_NEAR_HIT_DTYPE.names] == [0, 4, 8, 12]
    h = header()
    assert re.search(r"typedef struct dk_fm_near_hit \{ uint32_t pattern, block, position, cost; \} dk_fm_near_hit;", h)
    assert re.search(r"#define DK_FM_NEAR_MAX_PATTERN 128u", h) and FM_NEAR_MAX_PATTERN == _lib.FM_NEAR_MAX_PATTERN == 128
    assert re.search(r"#define DK_FM_NEAR_MAX_K 3u", h) and FM_NEAR_MAX_K == _lib.FM_NEAR_MAX_K == 3
    assert re.search(r"#define DK_FM_NEAR_NODE_LIMIT \(1u << 20\)", h) and FM_NEAR_NODE_LIMIT == _lib.FM_NEAR_NODE_LIMIT == 1 << 20


def test_null_context():
    lib = dark_amd.load_library()
    total, cut = C.c_uint64(7), C.c_uint64(9)
    one = (C.c_size_t * 1)(2)
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.dk_dev_fm_near(None, p, 2, p, p, 32, p, 1, one, 1, 0, 1, p, p, C.byref(total), C.byref(cut)) == _lib.DK_E_ARG
    assert lib.dk_dev_fm_near_packed(None, p, 1, one, p, p, 32, p, 1, one, 1, 0, 1, p, p, C.byref(total), C.byref(cut)) == _lib.DK_E_ARG
    assert total.value == 7 and cut.value == 9 and not any(buf)
    h = header()
    for name in ("dk_dev_fm_near", "dk_dev_fm_near_packed"):  # served by contexts of either purpose
        assert re.search(r"\bint %s\(dk_ctx \*any_ctx," % name, h), name
        assert name in _lib.SIGNATURES
    assert "dk_fm_near" not in _lib.SIGNATURES and "NO host-memory form and NO C++ mirror" in h


def test_classes_bit_positions():
    got = fm.classes(bytes([0, 7, 8, 255]))
    assert got.shape == (4, 32) and got.dtype == np.uint8
    assert class_masks(got) == [1 << 0, 1 << 7, 1 << 8, 1 << 255]
    assert got[0, 0] == 1 and got[1, 0] == 0x80 and got[2, 1] == 1 and got[3, 31] == 0x80 and int(got.astype(np.int64).sum()) == 1 + 0x80 + 1 + 0x80
    for p in (b"", b"a", b"Hello, World! 09@[`{\x00\xff"):
        assert np.array_equal(fm.classes(p), exact_classes(p)) and fm.classes(p).shape == (len(p), 32)
    assert np.array_equal(fm.classes(np.frombuffer(b"xyz", np.uint8)), exact_classes(b"xyz"))


def test_classes_ignore_case_and_wildcard():
    p = b"aZ@[`{09\xc1\xe1 mM"
    masks = class_masks(fm.classes(p, ignore_case=True))
    want = []
    for c in p:
        both = {c, c ^ 0x20} if chr(c).isascii() and chr(c).isalpha() else {c}
        want.append(sum(1 << x for x in both))
    assert masks == want
    assert masks[0] == (1 << 0x61) | (1 << 0x41) and masks[1] == (1 << 0x5A) | (1 << 0x7A)
    assert [bin(m).count("1") for m in masks] == [2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2]  # the neighbours of the letters and bytes >= 0x80 stay
    wild = fm.classes(b"a?c?", wildcard=ord("?"))
    assert class_masks(wild) == [1 << 97, (1 << 256) - 1, 1 << 99, (1 << 256) - 1]
    both = fm.classes(b"a?C", ignore_case=True, wildcard=63)
    assert class_masks(both) == [(1 << 97) | (1 << 65), (1 << 256) - 1, (1 << 99) | (1 << 67)]
    assert np.array_equal(fm.classes(b"a?c"), exact_classes(b"a?c"))  # no wildcard unless one is named


@pytest.mark.parametrize("argv", [["--mismatches", "1", "book.dark"], ["-i", "book.dark"], ["--ignore-case", "book.txt"],
                                  ["--grep", "x", "--mismatches", "4", "book.dark"], ["--grep", "x", "--mismatches", "-1", "book.dark"],
                                  ["--grep", "x", "--mismatches", "two", "book.dark"],
                                  ["--grep", "x", "--mismatches", "1", "--across-blocks", "book.dark"],
                                  ["--grep-hex", "41", "-i", "--across-blocks", "book.dark"],
                                  ["--grep", "x" * 129, "-i", "book.dark"], ["--grep-hex", "41" * 129, "--mismatches", "2", "book.dark"]])
def test_argument_errors(argv, capsys, tmp_path, monkeypatch):
    """refused by the argument parser (status 2), before any file or GPU is looked at"""
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "usage:" in err and ("--mismatches" in err or "--ignore-case" in err) and os.listdir(str(tmp_path)) == []


def test_across_with_near_is_refused_before_anything_is_opened(tmp_path):
    missing = str(tmp_path / "no_such.dark")
    for kw in (dict(mismatches=1), dict(ignore_case=True), dict(mismatches=2, ignore_case=True)):
        with pytest.raises(ValueError):
            next(search.search_archive(missing, "exp", [b"abc"], across=True, **kw))
    with pytest.raises(ValueError):
        next(search.search_archive(missing, "exp", [b"abc"], mismatches=4))
