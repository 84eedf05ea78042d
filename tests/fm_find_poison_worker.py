"""The FM-index's find on a poisoned workspace behind a poisoned mailbox: the process tests/test_gpu_fm_find.py starts once.

    python tests/fm_find_poison_worker.py fm_find BYTE      with DARK_AMD_LIB = dark_amd/libdark_amd_tuning.so and DK_POISON = BYTE in the environment

The contexts come from tests/poison_worker.py's open_ctx (the tuning build, the poison live, dk_dbg_mail_fill(BYTE) in front of every call), the
calls from the helpers of tests/test_gpu_fm_find.py, and the answers are compared with tests/fm_find_model.py: a pack whose pairs fill more than
one row of the scan, a truncated list, the single-block and the host form, on a full context and on a decoder context."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison_worker as W  # noqa: E402  (reads the group's name and the byte from the command line)

import numpy as np  # noqa: E402

from fm_find_model import block_structures, find_model  # noqa: E402
from test_gpu_fm import words  # noqa: E402
from test_gpu_fm_find import gpu_find, pack_of, same_records  # noqa: E402


def run(ctx):
    texts = words(b"ab", range(1, 7)) + [b"abracadabra" * 40, b"a" * 1025]
    pats = words(b"abc", range(0, 3)) + [b"abra", b"a" * 1024]
    assert len(texts) * len(pats) > 256  # more than one row of the scan
    want_occ, want, want_total = find_model(texts, pats)
    for step in (1, 32):
        W.say("%s context, the pack, step %d" % (ctx.purpose, step))
        d_bwt, idx, loc, sizes = pack_of(ctx, texts, step)
        for max_hits in (want_total + 1, 9, 0):
            occ, recs, total = gpu_find(ctx, d_bwt, sizes, idx, loc if max_hits else None, step, pats, max_hits)
            assert total == want_total and np.array_equal(occ, want_occ), (step, max_hits)
            same_records(recs, want[:max_hits], "step %d max_hits %d:" % (step, max_hits))
    W.say("%s context, one block and the host form" % ctx.purpose)
    t = texts[-2]
    one_occ, one, one_total = find_model([t], pats)
    d_bwt, idx, loc, sizes = pack_of(ctx, [t], 8)
    occ, recs, total = gpu_find(ctx, d_bwt, sizes, idx, loc, 8, pats, one_total)
    assert total == one_total and np.array_equal(occ, one_occ)
    same_records(recs, one)
    _, L, origin = block_structures(t)
    occ, recs, total = ctx.fm_find(L, origin, pats, max_hits=50, step=8)
    assert total == one_total and np.array_equal(occ, one_occ[:, 0])
    same_records(recs, one[:50])


if __name__ == "__main__":
    t0 = time.perf_counter()
    total = sum(m * 2 ** m for m in range(1, 7)) + 440 + 1025  # the pack of run()
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
