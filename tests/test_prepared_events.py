"""The host coder's prepared events and its six-stage form: tools/prepared_events_check.cpp, a stand-alone program, built
plain, under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer, and run as it is -- nothing is loaded into this
process.  It compares single steps of the prepared-event loop with RangeState::narrow from chosen quotients, crafted events (threshold
cuts, shifts of two and three bytes in a row and at a batch's first and last event) through the prepare stage, and DC streams through the
six-thread form with the one-thread form's bytes: distances all zero, distances up to 2^31 - 2, 2048 k - 1 / 2048 k / 2048 k + 1
decisions for k = 1, 2, 17, a frontier that advances in pieces, a poisoned frontier."""
import os
import subprocess

import pytest

from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = [os.path.join(ROOT, "tools", "prepared_events_check.cpp"), os.path.join(ROOT, "dark_amd", "csrc", "bbb.cpp")]
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++")
TSAN_ENV = {"TSAN_OPTIONS": "halt_on_error=0 report_signal_unsafe=0"}


def _build(exe, flags, opt):
    cmd = [CLANG, opt, "-g", "-std=c++17", "-march=x86-64-v3", "-I" + os.path.join(ROOT, "include"), "-o", exe] + flags + SRC + ["-lpthread"]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitizer" in (build.stderr or "").lower() and "not found" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("prepared_events")
    made = {}

    def get(kind):
        if kind not in made:
            flags, opt = {"plain": ([], "-O2"), "asan": (["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "-O1"),
                          "tsan": (["-fsanitize=thread"], "-O2")}[kind]
            made[kind] = _build(str(d / ("check_" + kind)), flags, opt)
        return made[kind]
    return get


def _run(exe, what, env=None):
    run = subprocess.run([exe, what], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    print(run.stdout[-2000:])
    assert run.returncode == 0 and "bad: 0" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    assert "ThreadSanitizer" not in run.stderr, run.stderr[-6000:]


@pytest.mark.parametrize("what", ["steps", "events", "streams"])
def test_plain(exes, what):
    _run(exes("plain"), what)


@pytest.mark.parametrize("what", ["steps", "events", "streams"])
def test_under_asan_ubsan(exes, what):
    _run(exes("asan"), what)


@pytest.mark.parametrize("what", ["events", "streams"])
def test_under_tsan(exes, what):
    _run(exes("tsan"), what, env=TSAN_ENV)
