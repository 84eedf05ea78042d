"""The host pipeline's range coder takes the next quotient from the previous one: tests/cpp_coder_chain.cpp, a stand-alone
program, codes crafted streams of uniform events through code_uniform and demands RangeState::narrow's bytes (totals 2, 3, 4095, 4096, 4097
and 3 * 2^12 - 1, intervals wider than the next total, intervals of one unit, shifts of one, two and three bytes, threshold cuts, streams of
exactly one batch, one batch and one event, one batch and a stretch, an end inside the careful path near the buffer's end, one byte too
little), and runs every thread form against the one-thread form on a DC stream of 2^21 distances and of one stretch more.  CPU builds under
AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer; nothing is loaded into this process."""
import os
import struct
import subprocess

import pytest

from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = [os.path.join(ROOT, "tests", "cpp_coder_chain.cpp"), os.path.join(ROOT, "dark_amd", "csrc", "bbb.cpp")]
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++")


def _build(exe, flags, opt="-O1"):
    cmd = [CLANG, opt, "-g", "-std=c++17", "-march=x86-64-v3", "-I" + os.path.join(ROOT, "include"), "-o", exe] + flags + SRC + ["-lpthread"]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitizer" in (build.stderr or "").lower() and "not found" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("coder_chain") / "check_asan"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


@pytest.fixture(scope="module")
def tsan_exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("coder_chain") / "check_tsan"), ["-fsanitize=thread"], opt="-O2")


@pytest.fixture(scope="module")
def dc_stream_file(tmp_path_factory, orc):
    """the DC stream of 4.5 MB of wiki-like text (2.4 M distances: the smallest stream the pipeline takes by itself is 2^21), in the layout of
    tools/make_dc_sample.py"""
    from dark_amd import datagen
    t = datagen.wiki_like(4_500_000, 2)
    bwt, origin = orc.bwt_forward(t)
    dc = orc.dc_encode(bwt)
    assert len(dc["d"]) >= (1 << 21) + 4096
    path = str(tmp_path_factory.mktemp("coder_chain") / "dc_stream.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<QQI", len(t), len(dc["d"]), origin))
        f.write(dc["init"].tobytes())
        f.write(dc["d"].tobytes())
        f.write(dc["sym"].tobytes())
    return path


def _run(exe, args, env=None):
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=env)
    print(run.stdout[-1500:])
    assert run.returncode == 0 and "bad: 0" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    assert "ThreadSanitizer" not in run.stderr, run.stderr[-6000:]


def test_crafted_events_under_asan_ubsan(asan_exe):
    _run(asan_exe, ["events"])


def test_crafted_events_under_tsan(tsan_exe):
    _run(tsan_exe, ["events"], env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 report_signal_unsafe=0"))


def test_thread_forms_under_asan_ubsan(asan_exe, dc_stream_file):
    _run(asan_exe, ["forms", dc_stream_file])


def test_thread_forms_under_tsan(tsan_exe, dc_stream_file):
    _run(tsan_exe, ["forms", dc_stream_file], env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 report_signal_unsafe=0"))
