"""The tuning build's switches (csrc/context.hpp DK_KNOB) must reach the library that reads them.  A DK_KNOB in a source that the tuning build
compiles without -DDK_TUNING (dark_amd/build.py TUNING_SOURCES) silently becomes its default: a test that sets it passes without testing
anything.  And the test hooks that lower the suffix sort's limits (tests/test_gpu_fallbacks.py) must not exist in the product library."""
import glob
import os
import re

from conftest import ROOT

LIB = os.path.join(ROOT, "dark_amd", "libdark_amd.so")
TUNING_LIB = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")
TEST_HOOKS = ("DK_LF_DEEP_CAP", "DK_LF_ARENA", "DK_LF_GIANT_CAP", "DK_LF_GIANT_ARENA", "DK_LF_GIANT_ROUNDS", "DK_LF_ROUNDS", "DK_PACKED_ROUNDS")


def _knob_names():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "dark_amd", "csrc", "*")):
        with open(path, encoding="utf-8", errors="replace") as f:
            names |= set(re.findall(r'\b(?:DK_KNOB|tuning_knob)\(\s*"([^"]+)"', f.read()))
    return names


def _read(path):
    assert os.path.exists(path), "build the tuning library: python dark_amd/build.py --tuning (__graft_entry__.build() does)"
    with open(path, "rb") as f:
        return f.read()


def test_every_knob_is_read_by_the_tuning_build():
    names = _knob_names()
    assert set(TEST_HOOKS) <= names and "DK_POISON" in names, sorted(names)
    lib = _read(TUNING_LIB)
    missing = sorted(k for k in names if k.encode() + b"\0" not in lib)
    assert not missing, "knobs the tuning build compiles away (add their source to TUNING_SOURCES in dark_amd/build.py): %s" % missing


def test_test_hooks_stay_out_of_the_product_library():
    lib = _read(LIB)
    present = sorted(k for k in TEST_HOOKS if k.encode() in lib)
    assert not present, present
