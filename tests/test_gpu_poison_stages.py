"""Every device stage on a poisoned workspace and behind a poisoned mailbox.  The workspace (dk_ctx::ws_alloc, csrc/context.cpp) and the
mailbox (csrc/mailbox.hpp) outlive a call: a kernel that reads a word which its own call never wrote reads what the call before left there --
zeros on a fresh context, and mostly the right thing in a test file that feeds one context near-identical calls.  DK_POISON=<byte> of the
tuning build (dark_amd/libdark_amd_tuning.so) fills every workspace allocation with the byte first, rounding slack included, and
dk_dbg_mail_fill does the same to the mailbox between calls: such a read then gives the same wrong answer every time.

One fresh process per (stage group, byte) -- knobs are read once per process -- runs tests/poison_worker.py, which drives the stage tests' own
helpers and compares with their CPU models (DESIGN.md section 3 has the table of who writes and who reads every allocation):
  dc        the carry levels of csrc/dc.hip and of the k_pdc_* pass (tests/dc_shapes.py)
  inverse   k_ibwt_* / k_pib_* on correct inputs and on the no-BWT classes a-g, on a full context and on decoder contexts of exactly their input
  packed    the segmented sort, its guard, k_pk_emit, the packed inverse and decode, all five models through dev_packed_encode
  lcp       phi, the long and the giant list, single and packed, and a suffix array that is refused
  sa        sa_check on valid and damaged arrays, sa_search on both sides of its kernels' border, in one block and in a pack
  fm        the FM-index: build and count, the locate and extract structures at steps 8 and 32, snippets; full and decoder contexts
  rerank    one regrouping of the suffix sort (rerank, classify_and_read) on built lists of a few tiles: first, narrow and later forms
The bytes, in this order: 0 imitates a fresh allocation, 255 the all-ones sentinels (IB_END, DK_FM_NO_HIT, LCP_MARK, the 0xFF fills), 165
neither; each hides what the others show.  First in every worker: dbg_ws_peek returns the byte and the library is the tuning build --
otherwise the run proves nothing and fails."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

TUNING_LIB = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")
WORKER = os.path.join(ROOT, "tests", "poison_worker.py")
TIMEOUT = 240  # seconds per subprocess, as in tests/test_gpu_fallbacks.py; a group takes a few
GROUPS = ("dc", "inverse", "packed", "lcp", "sa", "fm", "rerank")
BYTES = (0, 255, 165)
# what a group must have gone through (stats()["routes"] of its calls, asserted case by case in the worker as the stage's own test does)
ROUTES = {"packed": {"packed_guard"}, "lcp": {"lcp_long", "lcp_giant", "packed_guard"}}

_dead = []  # a subprocess that died by a signal or ran out of time: nothing more is started


@pytest.mark.parametrize("byte,group", [(b, g) for b in BYTES for g in GROUPS], ids=["%s-%d" % (g, b) for b in BYTES for g in GROUPS])
def test_stage_group(group, byte):
    if _dead:
        pytest.fail("not started: an earlier run of this module died (%s)" % _dead[0])
    assert os.path.exists(TUNING_LIB), "build the tuning library: python dark_amd/build.py --tuning (__graft_entry__.build() does)"
    what = "%s DK_POISON=%d" % (group, byte)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DK_")}
    env.update(DARK_AMD_LIB=TUNING_LIB, DK_POISON=str(byte))
    try:
        p = subprocess.run([sys.executable, WORKER, group, str(byte)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _dead.append("%s timed out" % what)
        pytest.fail("%s: no answer within %d s\n%s" % (what, TIMEOUT, str(e.stderr or "")[-3000:]))
    if p.returncode < 0 or p.returncode in (134, 139):
        _dead.append("%s: %s" % (what, "signal %d" % -p.returncode if p.returncode < 0 else "exit status %d" % p.returncode))
        pytest.fail("%s died (%d)\n%s" % (what, p.returncode, p.stderr[-3000:]))
    if p.returncode != 0 and any(w in p.stderr for w in ("DK_E_HIP", "illegal memory access", "HSA_STATUS_ERROR", "Memory access fault")):
        _dead.append("%s: a HIP error" % what)  # (the card has faulted although the process ended by itself)
    assert p.returncode == 0, "%s failed\n%s%s" % (what, p.stdout[-2000:], p.stderr[-6000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1][7:])
    print("%s: %s" % (what, res))
    # the positive control: the worker has seen the byte in fresh allocations of every context, before its first case and after its last
    assert res["group"] == group and res["byte"] == byte and res["contexts"] >= 1 and res["peeks"] >= 12 * res["contexts"], res
    assert res["fills"] >= 10, res
    assert ROUTES.get(group, set()) <= set(res["routes"]), res
