"""The find entries and the archive search (include/dark_amd.h: dk_dev_fm_find*, dark_amd/search.py, dark_amd/cli.py --grep): what needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dark_amd
from conftest import ROOT
from dark_amd import _lib, cli, search
from dark_amd.context import FM_HIT_DTYPE

MiB = 1 << 20


def test_the_record_is_16_bytes():
    assert C.sizeof(_lib.FmHit) == 16 and FM_HIT_DTYPE.itemsize == 16
    assert [name for name, _ in _lib.FmHit._fields_] == list(FM_HIT_DTYPE.names) == ["pattern", "block", "position", "slot"]
    assert [getattr(_lib.FmHit, name).offset for name in FM_HIT_DTYPE.names] == [FM_HIT_DTYPE.fields[name][1] for name in FM_HIT_DTYPE.names] == [0, 4, 8, 12]
    with open(os.path.join(ROOT, "include", "dark_amd.h")) as f:
        header = f.read()
    assert re.search(r"typedef struct dk_fm_hit \{ uint32_t pattern, block, position, slot; \} dk_fm_hit;", header)
    assert re.search(r"#define DK_FM_FIND_MAX_PAIRS \(1u << 24\)", header) and _lib.FM_FIND_MAX_PAIRS == 1 << 24


def test_null_context():
    lib = dark_amd.load_library()
    total = C.c_uint64(7)
    one = (C.c_size_t * 1)(1)
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.dk_dev_fm_find(None, p, 1, p, p, 32, p, 1, one, 1, p, p, C.byref(total)) == _lib.DK_E_ARG
    assert lib.dk_dev_fm_find_packed(None, p, 1, one, p, p, 32, p, 1, one, 1, p, p, C.byref(total)) == _lib.DK_E_ARG
    assert lib.dk_fm_find(None, p, 1, 0, 32, p, 1, one, 1, p, p, C.byref(total)) == _lib.DK_E_ARG
    assert total.value == 7 and not any(buf)
    with open(os.path.join(ROOT, "include", "dark_amd.h")) as f:
        header = f.read()
    for name in ("dk_dev_fm_find", "dk_dev_fm_find_packed", "dk_fm_find"):  # served by contexts of either purpose
        assert re.search(r"\bint %s\(dk_ctx \*any_ctx," % name, header), name
        assert name in _lib.SIGNATURES


def shape(segments):
    return [(kind, len(ks), nb) for kind, ks, nb in segments]


def test_plan():
    assert search.plan([]) == []
    assert search.plan([5, 1, 7]) == [("pack", [0, 1, 2], 13)]
    # a record above 16 MiB between small ones: a segment of its own, and the packs on either side do not join
    assert search.plan([3, 4, 16 * MiB + 1, 5, 16 * MiB, 6]) == [("pack", [0, 1], 7), ("big", [2], 16 * MiB + 1), ("pack", [3, 4, 5], 16 * MiB + 11)]
    assert search.plan([16 * MiB + 1, 16 * MiB + 2]) == [("big", [0], 16 * MiB + 1), ("big", [1], 16 * MiB + 2)]
    # a sum crossing 64 MiB: the record that would cross it opens the next pack; exactly 64 MiB still fits
    assert shape(search.plan([16 * MiB] * 4 + [1])) == [("pack", 4, 64 * MiB), ("pack", 1, 1)]
    assert shape(search.plan([16 * MiB] * 3 + [16 * MiB - 1, 1, 1])) == [("pack", 5, 64 * MiB), ("pack", 1, 1)]
    assert shape(search.plan([10 * MiB] * 13)) == [("pack", 6, 60 * MiB), ("pack", 6, 60 * MiB), ("pack", 1, 10 * MiB)]
    # more records than a pack holds
    got = search.plan([1] * 65537)
    assert shape(got) == [("pack", 65536, 65536), ("pack", 1, 1)] and got[1][1] == [65536]
    # every record once, in order
    rng = np.random.default_rng(5)
    sizes = rng.choice([1, 100, 5 * MiB, 16 * MiB, 16 * MiB + 1, 40 * MiB], size=200).tolist()
    got = search.plan(sizes)
    assert [k for _, ks, _ in got for k in ks] == list(range(200))
    for kind, ks, nb in got:
        assert nb == sum(sizes[k] for k in ks)
        assert (kind == "big" and len(ks) == 1 and nb > 16 * MiB) or (kind == "pack" and nb <= 64 * MiB and max(sizes[k] for k in ks) <= 16 * MiB)


def test_plan_is_the_packed_decoders():
    """the constants are the CLI's own, so a segment here is a pack there"""
    assert (search.PACK_BYTES, search.PACKED_MAX_BLOCKS, search.PACKED_MAX_BLOCK_BYTES) == (cli.PACK_BYTES, cli.PACKED_MAX_BLOCKS, cli.PACKED_MAX_BLOCK_BYTES)
    assert (cli.PACK_BYTES, cli.PACKED_MAX_BLOCKS, cli.PACKED_MAX_BLOCK_BYTES) == (64 * MiB, _lib.DK_PACKED_MAX_BLOCKS, _lib.DK_PACKED_MAX_BLOCK_BYTES)


@pytest.mark.parametrize("argv", [["--grep", "x", "book.txt"], ["--grep-hex", "6", "book.dark"], ["--grep-hex", "zz", "book.dark"],
                                  ["--grep", "x", "--gpus", "2", "book.dark"], ["--grep", "", "book.dark"],
                                  ["--grep", "x", "--context-bytes", "-1", "book.dark"], ["--grep", "x", "--max-hits", "-1", "book.dark"]])
def test_cli_argument_errors(argv, capsys, tmp_path, monkeypatch):
    """refused by the argument parser (status 2, as grep's own errors), before any file or GPU is looked at"""
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    assert "usage:" in capsys.readouterr().err and os.listdir(str(tmp_path)) == []


def test_enclosing_line():
    w = b"one\ntwo three\nfour"
    assert cli.enclosing_line(w, 8, 5) == b"two three"       # "three": newlines on both sides
    assert cli.enclosing_line(w, 0, 3) == b"one"             # at the window's head
    assert cli.enclosing_line(w, 14, 4) == b"four"           # at its end
    assert cli.enclosing_line(b"abc", 1, 1) == b"abc"        # no newline within the window
    assert cli.enclosing_line(b"a\nb\nc", 1, 3) == b"a\nb\nc"[0:5]  # a pattern that holds newlines keeps them
    assert cli._escape(b"a\tb\xff\\ ~") == "a\\x09b\\xff\\ ~"
