"""The seams entries and the archive search across block borders (include/dark_amd.h: dk_dev_fm_seams*, dark_amd/search.py, dark_amd/cli.py
--across-blocks): what needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dark_amd
from conftest import ROOT
from dark_amd import _lib, cli, search
from dark_amd.context import FM_SEAM_HIT_DTYPE
from fm_seams_model import SEAM_DTYPE

MiB = 1 << 20


def test_the_record_is_16_bytes():
    assert FM_SEAM_HIT_DTYPE.itemsize == 16 and FM_SEAM_HIT_DTYPE == SEAM_DTYPE
    assert list(FM_SEAM_HIT_DTYPE.names) == ["pattern", "block", "back", "reserved"]
    assert [FM_SEAM_HIT_DTYPE.fields[name][1] for name in FM_SEAM_HIT_DTYPE.names] == [0, 4, 8, 12]
    with open(os.path.join(ROOT, "include", "dark_amd.h")) as f:
        header = f.read()
    assert re.search(r"typedef struct dk_fm_seam_hit \{ uint32_t pattern, block, back, reserved /\* 0 \*/; \} dk_fm_seam_hit;", header)
    assert re.search(r"#define DK_FM_SEAM_MAX_PATTERN 4096u", header) and _lib.FM_SEAM_MAX_PATTERN == 4096


def test_null_context():
    lib = dark_amd.load_library()
    total = C.c_uint64(7)
    one = (C.c_size_t * 1)(2)
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.dk_dev_fm_seams(None, p, 2, p, p, 32, p, 1, p, 1, one, 1, p, p, C.byref(total)) == _lib.DK_E_ARG
    assert lib.dk_dev_fm_seams_packed(None, p, 1, one, p, p, 32, p, 1, p, 1, one, 1, p, p, C.byref(total)) == _lib.DK_E_ARG
    assert total.value == 7 and not any(buf)
    with open(os.path.join(ROOT, "include", "dark_amd.h")) as f:
        header = f.read()
    for name in ("dk_dev_fm_seams", "dk_dev_fm_seams_packed"):  # served by contexts of either purpose
        assert re.search(r"\bint %s\(dk_ctx \*any_ctx," % name, header), name
        assert name in _lib.SIGNATURES
    assert "dk_fm_seams" not in _lib.SIGNATURES and "NO host-memory form" in header  # a single block has no inner border


def test_plan_with_pack_bytes():
    rng = np.random.default_rng(5)
    sizes = rng.choice([1, 100, 5 * MiB, 16 * MiB, 16 * MiB + 1, 40 * MiB], size=200).tolist()
    assert search.plan(sizes, None) == search.plan(sizes) == search.plan(sizes, search.PACK_BYTES)
    assert search.plan([], 10) == []
    # a sum crossing the limit opens the next pack; exactly the limit still fits; a record above it gets a pack of its own
    assert search.plan([4, 4, 4, 4, 1], 16) == [("pack", [0, 1, 2, 3], 16), ("pack", [4], 1)]
    assert search.plan([4, 4, 4, 5, 1], 16) == [("pack", [0, 1, 2], 12), ("pack", [3, 4], 6)]
    assert search.plan([4, 40, 4, 4], 16) == [("pack", [0], 4), ("pack", [1], 40), ("pack", [2, 3], 8)]
    assert search.plan([4096] * 49, 4096) == [("pack", [k], 4096) for k in range(49)]
    assert [len(ks) for _, ks, _ in search.plan([4096] * 48 + [3392], 16384)] == [4] * 12 + [1]
    assert search.plan([3, 16 * MiB + 1, 5], 4) == [("pack", [0], 3), ("big", [1], 16 * MiB + 1), ("pack", [2], 5)]
    for limit in (1, 1000, 6 * MiB, 100 * MiB):
        got = search.plan(sizes, limit)
        assert [k for _, ks, _ in got for k in ks] == list(range(200))
        for kind, ks, nb in got:
            assert nb == sum(sizes[k] for k in ks) and (nb <= limit or len(ks) == 1)


@pytest.mark.parametrize("argv", [["--across-blocks", "book.dark"], ["--across-blocks", "book.txt"], ["--across-blocks", "-b", "4096", "book.txt"],
                                  ["--across-blocks", "--count-only", "book.dark"]])
def test_across_blocks_goes_with_grep(argv, capsys, tmp_path, monkeypatch):
    """refused by the argument parser (status 2), before any file or GPU is looked at"""
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "usage:" in err and "--across-blocks" in err and os.listdir(str(tmp_path)) == []
