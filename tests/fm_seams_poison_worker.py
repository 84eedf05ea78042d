"""The FM-index's seams on a poisoned workspace behind a poisoned mailbox: the process tests/test_gpu_fm_seams.py starts once.

    python tests/fm_seams_poison_worker.py fm_seams BYTE      with DARK_AMD_LIB = dark_amd/libdark_amd_tuning.so and DK_POISON = BYTE in the environment

The contexts come from tests/poison_worker.py's open_ctx (the tuning build, the poison live, dk_dbg_mail_fill(BYTE) in front of every call), the
calls from the helpers of tests/test_gpu_fm_seams.py, and the answers are compared with tests/fm_seams_model.py: a pack whose pairs fill more
than one row of the scan and whose strip holds whole blocks, touching and parted edges; a truncated list; the single-block form; on a full
context and on a decoder context."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison_worker as W  # noqa: E402  (reads the group's name and the byte from the command line)

import numpy as np  # noqa: E402

from fm_seams_model import seams_model  # noqa: E402
from test_gpu_fm import words  # noqa: E402
from test_gpu_fm_seams import gpu_seams, pack_of, same_records  # noqa: E402

TEXTS = words(b"ab", range(1, 6)) + [b"abracadabra" * 40, b"a" * 7, b"abra" * 3, b"a" * 1025]


def run(ctx):
    pats = words(b"ab", range(0, 4)) + [b"abra", b"raab", b"aabra", b"a" * 9, b"bbbbba"]
    assert len(TEXTS) * len(pats) > 256  # more than one row of the scan
    prev = b"abab"
    want_occ, want, want_total = seams_model(TEXTS, pats, prev, fast=True)
    assert want_total > 100
    for step in (1, 32):
        W.say("%s context, the pack, step %d" % (ctx.purpose, step))
        d_bwt, idx, ext, sizes = pack_of(ctx, TEXTS, step)
        for max_hits in (want_total + 1, 9, 0):
            occ, recs, total = gpu_seams(ctx, d_bwt, sizes, idx, ext, step, prev, pats, max_hits)
            assert total == want_total and np.array_equal(occ, want_occ), (step, max_hits)
            same_records(recs, want[:max_hits], "step %d max_hits %d:" % (step, max_hits))
    W.say("%s context, one block" % ctx.purpose)
    t = TEXTS[-4]
    one_occ, one, one_total = seams_model([t], pats, prev + b"r")
    assert one_total > 0
    d_bwt, idx, ext, sizes = pack_of(ctx, [t], 8)
    occ, recs, total = gpu_seams(ctx, d_bwt, sizes, idx, ext, 8, prev + b"r", pats, one_total)
    assert total == one_total and np.array_equal(occ, one_occ)
    same_records(recs, one)


if __name__ == "__main__":
    t0 = time.perf_counter()
    total = sum(len(t) for t in TEXTS)
    full = W.open_ctx(total)
    run(full)
    W.done_with(full)
    dec = W.open_ctx(total, "decoder", 128)
    run(dec)
    W.done_with(dec)
    W.REPORT["seconds"] = round(time.perf_counter() - t0, 2)
    assert W.REPORT["contexts"] == 2 and W.REPORT["peeks"] >= 12 * W.REPORT["contexts"] and W.REPORT["fills"] > 0, W.REPORT
    W.REPORT["routes"] = sorted(W.REPORT["routes"])
    print("RESULT " + json.dumps(W.REPORT))
